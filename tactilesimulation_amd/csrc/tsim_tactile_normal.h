// tsim_tactile_normal.h — arguments and LDS layout of the tactile normal equations (csrc/tsim_tactile_normal.hip k_tactile_normal;
// include/tsim.h tsim_tactile_normal_equations; its launch: tsim_launch.h, its plan: tsim_hip.hip tactile_normal_plan).
//
// What it computes, per environment and MASKED frame f of the window (DESIGN.md §4 "Tactile normal equations"), with x = (q, qd), the tactile
// block H = [C_f | F_f] [ndof_tactile][Z] (C_f: tsim_tactile_jacobians', F_f: the dense form of tsim_param_jacobians' Ft), a diagonal W and r:
//     N = H^T W H [Z][Z]      n = H^T W r [Z]
// without H ever leaving the block: a taxel's three rows are formed in LDS and reduced there.  It depends on ONE tape record, the frame's last;
// nothing is solved.  A slot is (environment, frame) on the parameter passes' scaffold (tsim_param_pass.h, chunk = frame).
#pragma once
#include <hip/hip_runtime.h>
#include "tsim_param_grad.h"

// Columns of a tile row, in this order: the 2 nr state columns, the sensor's four parameter columns (with_params), r (with a residual), and the
// row's weight last.  The symmetric product runs over the first zc = ts_tn_zc of them; the row stride is odd, so that the lanes' row writes
// (stride 3 rows) fall on different banks.
__host__ __device__ inline int ts_tn_zc(int nr, int with_params, int with_resid) { return 2 * nr + (with_params ? 4 : 0) + (with_resid ? 1 : 0); }
__host__ __device__ inline int ts_tn_stride(int nr, int with_params) { return (ts_tn_zc(nr, with_params, 1) + 1) | 1; }
// entries (d <= e) of the symmetric zc x zc block; entry (d, e) at d zc - d (d - 1) / 2 + e - d
__host__ __device__ inline int ts_tn_entries(int zc) { return zc * (zc + 1) / 2; }
// LDS reals a slot holds next to its context (behind the contexts of all the block's slots, at TnArgs::xoff):
//   Q0 [nr][12], Q1 [nr][6]     the staged pair's per-dof records, as k_tactile_jacobian's (tsim_tactile_jacobian.h)
//   ACC [entries]               the running sums of the symmetric block, sized for a residual whether one is given or not
//   TILE [rows][3][stride]      the rows of the chunk's taxels; rows <= lanes per environment taxels are evaluated at a time
// The launch shape depends on with_params and on nothing else of the call.
__host__ __device__ inline int ts_tn_slot_reals(int nr, int with_params, int rows) {
  return ((18 * nr + 3) & ~3) + ((ts_tn_entries(ts_tn_zc(nr, with_params, 1)) + 3) & ~3) + ((3 * rows * ts_tn_stride(nr, with_params) + 3) & ~3);
}
// behind the slots' blocks, once per block: the (d, e) of every entry as d | e << 8 (int32), sized likewise
__host__ __device__ inline int ts_tn_table_bytes(int nr, int with_params) { return ((ts_tn_entries(ts_tn_zc(nr, with_params, 1)) * 4 + 15) / 16) * 16; }
enum { TS_TN_MIN_ROWS = 4 };      // the fewest taxels per trip the plan goes down to before it refuses

// PgCommon: nchunk = the frames, chunk_len = the sub-steps of a frame; z, part and P are not used
template <class R> struct TnArgs : PgCommon<R> {
  int cull;
  int xoff;                                                  // reals from the start of the block's LDS to slot 0's block
  int toff;                                                  // bytes from the start of the block's LDS to the entry table
  int rows;                                                  // taxels of a slot per trip of the chunk loop (<= lanes per environment)
  int with_params;
  const int32_t* tac_slot;                                   // [nframes] slot of the frame in the outputs or < 0: not masked (null: slot f)
  const R* weight;                                           // [ndof_tactile] or null: ones
  const R* resid;                                            // [num_masked][B][ndof_tactile] or null
  R* N_out;                                                  // [num_masked][B][Z][Z]
  R* n_out;                                                  // [num_masked][B][Z] (with resid)
};
