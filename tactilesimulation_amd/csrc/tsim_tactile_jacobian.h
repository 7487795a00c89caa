// tsim_tactile_jacobian.h — arguments and LDS layout of the per-frame tactile Jacobians (csrc/tsim_tactile_jacobian.hip k_tactile_jacobian;
// include/tsim.h tsim_tactile_jacobians; its launch: tsim_launch.h, its plan: tsim_hip.hip ts_plan).
//
// What it computes, per environment and MASKED frame f of the window (DESIGN.md §4 "Tactile Jacobians"), with x = (q, qd):
//     C_f = dtactile / dx at the frame's END state   [ndof_tactile][2 nr], stored column by column: Ct [2 nr][ndof_tactile]
// the Jacobian of the read-out map tac(q, qd) with q and qd as independent variables.  It depends on ONE tape record, the frame's last; nothing is
// solved.  A slot is (environment, frame) on the parameter passes' scaffold (tsim_param_pass.h, chunk = frame), as the frame Jacobians' is.
#pragma once
#include <hip/hip_runtime.h>
#include "tsim_param_grad.h"

// LDS reals a slot holds next to its context (behind the contexts of all the block's slots, at TjArgs::xoff), for the pair that is staged:
//   Q0 [nr][12]   the dofs' mode-0 records (dth, drho, dw, dv) of pair_stage_tangent: the 12-vector of q-column k
//   Q1 [nr][6]    the velocity half (dw, dv) of their mode-1 records: the 12-vector of qd-column k is (0, 0, Q1[k])
// (both staging calls write c.PT, the second over the first)
__host__ __device__ inline int ts_tj_slot_reals(int nr) { return (18 * nr + 3) & ~3; }

// PgCommon: nchunk = the frames, chunk_len = the sub-steps of a frame; z, part and P are not used
template <class R> struct TjArgs : PgCommon<R> {
  int cull;
  int xoff;                                                  // reals from the start of the block's LDS to slot 0's block
  const int32_t* tac_slot;                                   // [nframes] slot of the frame in Ct_out or < 0: not masked (null: slot f)
  R* Ct_out;                                                 // [num_masked][B][2 nr][ndof_tactile]
};
