// tsim_param_grad.h — arguments of the parameter-gradient pass (csrc/tsim_param_grad.hip; include/tsim.h tsim_set_param_grad; its launch: tsim_launch.h).
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

template <class R> struct PgArgs {
  const int* I; const R* F; const R* Fenv; int fstride;
  int B, n, t_end;
  int seed_stride, frames; const int* tac_slot;      // the seed layout of the adjoint launch this pass follows (BwdArgs)
  const R* tape; const R* z;                         // z: [cap][B][nr], sub-step t at row t - 1 (k_backward_z)
  const R* df_dtac;
  int nchunk, chunk_len;                             // slots = nchunk x B; chunk k covers sub-steps [k chunk_len, (k + 1) chunk_len) of the n
  int P;                                             // ts_pg_count
  R* part;                                           // [nchunk][B][P] partial sums
  int stage_cpt;
  int tk;                                            // the tape records hold K (ts_rec)
};
template <class R> struct PgReduceArgs {
  const R* part; int nchunk, B, P;
  R* out; int stride;                                // caller's buffer [B][stride] (stride = tsim_table_size)
  int npair, nsensor, nr, foff_pair, foff_sensor, foff_dof;
};

// The body groups (tsim_set_param_grad_groups: TSIM_PG_INERTIAL / MOTOR / LIMIT), a pass of their own (k_param_grad_body) with its own compact vector:
// [link mass com(3) inertia(6)] x nl, [motor lo hi P D] x nu, [dof lim_lo lim_hi lim_k] x nr.  It evaluates the taped state WITH the sub-step's
// discrete accelerations (the contact pass needs none) and reads the tape records before the sub-step for them.
__host__ __device__ inline int ts_pgb_count(int nl, int nu, int nr) { return 10 * nl + 4 * nu + 3 * nr; }
enum { TS_PG_CONTACT = 1, TS_PG_INERTIAL = 2, TS_PG_MOTOR = 4, TS_PG_LIMIT = 8 };      // = TSIM_PG_* of include/tsim.h

template <class R> struct PgBodyArgs {
  const int* I; const R* F; const R* Fenv; int fstride;
  int B, n, t_end;
  const R* tape; const R* z;                         // as PgArgs
  int nchunk, chunk_len;
  int P;                                             // ts_pgb_count
  R* part;                                           // [nchunk][B][P] partial sums
  int stage_cpt, tk;
  int groups;                                        // TS_PG_*: the groups that are evaluated
};
template <class R> struct PgBodyReduceArgs {
  const R* part; int nchunk, B, P;
  R* out; int stride;
  int nl, nu, nr, foff_link, foff_motor, foff_dof;
  int groups;                                        // only these groups' columns are added to
};

void ts_param_reduce_launch(const PgReduceArgs<float>& a, hipStream_t st);
void ts_param_reduce_launch(const PgReduceArgs<double>& a, hipStream_t st);
void ts_param_reduce_body_launch(const PgBodyReduceArgs<float>& a, hipStream_t st);
void ts_param_reduce_body_launch(const PgBodyReduceArgs<double>& a, hipStream_t st);
