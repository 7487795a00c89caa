// tsim_param_grad.h — arguments of the two parameter-gradient passes and their reduction (csrc/tsim_param_grad.hip, csrc/tsim_param_grad_body.hip;
// include/tsim.h tsim_set_param_grad, tsim_set_param_grad_groups; their launch: tsim_launch.h).
//
// What it adds, per environment, for the physical parameters of the numeric tables (DESIGN.md §4 "Parameter gradient"):
//     dL/dp = sum_t -(dg_t/dp)^T z_t  +  sum_{seeded frames} (dtactile/dp)^T w_tac
// g_t = r_t / ca_t is the scaled residual of taped sub-step t and z_t the adjoint solution k_backward computed for it (k_backward_z saves them).
// Once z is saved the sub-steps no longer depend on each other: a slot of k_param_grad is (environment, chunk of sub-steps), and the chunks'
// partial sums are added in a fixed order by k_param_reduce — no float atomics, the same bits from run to run.
#pragma once
#include <hip/hip_runtime.h>

// compact parameter vector of an environment: [pair kn kt mu kd] x npair, [sensor kn kt mu kd] x nsensor, [dof damping] x nr
__host__ __device__ inline int ts_pg_count(int npair, int nsensor, int nr) { return 4 * npair + 4 * nsensor + nr; }

// What both passes take (k_param_grad, k_param_grad_body; the helpers that read it: tsim_param_pass.h; the host fills it: tsim_hip.hip
// launch_param_pass).  The order is part of the kernels: what only a kernel's prologue reads comes first, and what its sub-step loop reads last —
// B n t_end, then tape z next to the pointers PgArgs adds — so that the scalar loads of the arguments group as they did before the two passes
// shared this block (another order costs k_param_grad's rotation-vector instantiations scalar-register spills: profiles/r13_param_pass_scaffold.md).
template <class R> struct PgCommon {
  const int* I; const R* F; const R* Fenv; int fstride;
  int nchunk, chunk_len;                             // slots = nchunk x B; chunk k covers sub-steps [k chunk_len, (k + 1) chunk_len) of the n
  int P;                                             // length of the pass's compact vector (ts_pg_count / ts_pgb_count)
  R* part;                                           // [nchunk][B][P] partial sums
  int stage_cpt;
  int tk;                                            // the tape records hold K (ts_rec)
  int B, n, t_end;
  const R* tape; const R* z;                         // z: [cap][B][nr], sub-step t at row t - 1 (k_backward_z)
};
template <class R> struct PgArgs : PgCommon<R> {
  const int* tac_slot; const R* df_dtac; int seed_stride, frames;      // the seed layout of the adjoint launch this pass follows (BwdArgs)
};

// The body groups (tsim_set_param_grad_groups: TSIM_PG_INERTIAL / MOTOR / LIMIT), a pass of their own (k_param_grad_body) with its own compact vector:
// [link mass com(3) inertia(6)] x nl, [motor lo hi P D] x nu, [dof lim_lo lim_hi lim_k] x nr.  It evaluates the taped state WITH the sub-step's
// discrete accelerations (the contact pass needs none) and reads the tape records before the sub-step for them.
__host__ __device__ inline int ts_pgb_count(int nl, int nu, int nr) { return 10 * nl + 4 * nu + 3 * nr; }
enum { TS_PG_CONTACT = 1, TS_PG_INERTIAL = 2, TS_PG_MOTOR = 4, TS_PG_LIMIT = 8 };      // = TSIM_PG_* of include/tsim.h

template <class R> struct PgBodyArgs : PgCommon<R> {
  int groups;                                        // TS_PG_*: the groups that are evaluated
};

// The reduction of either pass (k_param_reduce): a pass's compact vector is up to three segments of records, and entry q of a segment belongs to
// column col0 + (q / per) * rec + q % per of the caller's buffer (per entries out of every rec-wide table record).  A segment that is off is skipped.
struct PgSeg { int count, per, rec, col0, on; };     // count: entries of the segment in the compact vector (per x records)
template <class R> struct PgReduceArgs {
  const R* part; int nchunk, B, P;                   // P = the three counts together
  R* out; int stride;                                // caller's buffer [B][stride] (stride = tsim_table_size)
  PgSeg seg[3];
};

void ts_param_reduce_launch(const PgReduceArgs<float>& a, hipStream_t st);
void ts_param_reduce_launch(const PgReduceArgs<double>& a, hipStream_t st);
