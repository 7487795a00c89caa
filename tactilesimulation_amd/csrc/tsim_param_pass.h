// tsim_param_pass.h — what the two parameter-gradient kernels share (k_param_grad: tsim_param_grad.hip, k_param_grad_body: tsim_param_grad_body.hip;
// only those two units and tsim_tangent_body.hip, whose pre-pass walks the same slots, include it: it needs Ctx).  A pass is launched with nchunk x ceil(B / NS) blocks of one wavefront (NS = TS_WAVE / LPE slots);
// a slot is (environment, chunk of sub-steps): it walks the chunk's taped sub-steps with the adjoint solution z of each and leaves one row of
// partial sums.  Every helper returns one scalar by value: a value that reaches the kernel through a returned struct loses what the compiler knows
// about it (the lane's range), and k_param_grad's code moves (profiles/r13_param_pass_scaffold.md).
#pragma once
#include "tsim_kernels.h"
#include "tsim_param_grad.h"

// block -> (chunk, NS neighbouring environments): every slot of a wavefront walks the same sub-steps (the walk has barriers)
template <int LPE, class R> __device__ __forceinline__ int pg_chunk(const PgCommon<R>& a) {
  constexpr int NS = TS_WAVE / LPE;
  return (int)blockIdx.x / ((a.B + NS - 1) / NS);
}
// the slot's environment; >= a.B in an idle slot of a chunk's last block, which repeats the last environment and stores nothing
template <int LPE, class R> __device__ __forceinline__ int pg_slot_env(const PgCommon<R>& a, int chunk) {
  constexpr int NS = TS_WAVE / LPE;
  return ((int)blockIdx.x - chunk * ((a.B + NS - 1) / NS)) * NS + (int)threadIdx.x / LPE;
}
// the slot's context on environment env's tables, and the world link
template <int LPE, class R> __device__ __forceinline__ void pg_ctx(const PgCommon<R>& a, R* lds, Ctx<R>& c, int lane, int env) {
  constexpr int NS = TS_WAVE / LPE;
  ctx_init<R>(c, a.I, a.F, lds, NS, (int)threadIdx.x / LPE, lane, LPE, a.stage_cpt != 0, a.Fenv ? a.Fenv + (size_t)env * a.fstride : nullptr);
  init_world(c, lane, LPE);
}
// the slot's row of the partial sums [nchunk][B][P]
template <class R> __device__ __forceinline__ R* pg_row(const PgCommon<R>& a, int chunk, int env) { return a.part + ((size_t)chunk * a.B + env) * a.P; }

// sub-step j of the launch's n: its tape index t (it is a BDF2 step if the model integrates so and t >= 2: k_backward's choice), the scale ca of its
// residual, its tape record
template <class R> __device__ __forceinline__ int pg_t(const PgCommon<R>& a, int j) { return a.t_end - (a.n - 1 - j); }
template <class R> __device__ __forceinline__ R pg_ca(const Ctx<R>& c, bool bdf2) { return bdf2 ? R(2.25) / (c.h * c.h) : R(1) / (c.h * c.h); }
template <class R> __device__ __forceinline__ const R* pg_rec(const PgCommon<R>& a, int t, int env, int REC) { return a.tape + ((size_t)t * a.B + env) * REC; }
// this lane's dof (lane < nr) of the taped state t and of its z; the acceleration c.qa is the caller's.  Its first line has a twin, pg_load_taped
// below: the two passes that use them are each other's transpose only while both load the taped state alike — edit them together
template <class R> __device__ __forceinline__ void pg_load_state(const PgCommon<R>& a, Ctx<R>& c, const R* rec, int t, int env, int nr, int lane) {
  c.qD[lane] = rec_q(rec)[lane]; c.q[lane] = (R)c.qD[lane]; c.qd[lane] = rec[rec_qd<R>(nr) + lane];
  c.z[lane] = a.z[((size_t)(t - 1) * a.B + env) * nr + lane];
}
// ... of the taped state alone, for a pass that has no adjoint solution (k_tangent_body_src, tsim_tangent_body.hip: the same scaffold walked
// with directions in place of z)
template <class R> __device__ __forceinline__ void pg_load_taped(Ctx<R>& c, const R* rec, int nr, int lane) {
  c.qD[lane] = rec_q(rec)[lane]; c.q[lane] = (R)c.qD[lane]; c.qd[lane] = rec[rec_qd<R>(nr) + lane];
}
