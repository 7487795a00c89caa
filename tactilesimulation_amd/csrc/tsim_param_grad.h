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

void ts_param_reduce_launch(const PgReduceArgs<float>& a, hipStream_t st);
void ts_param_reduce_launch(const PgReduceArgs<double>& a, hipStream_t st);
