// tsim_param_jacobian.h — arguments and LDS layout of the per-frame parameter Jacobians (csrc/tsim_param_jacobian.hip k_param_jacobian;
// include/tsim.h tsim_param_jacobians; its launch: tsim_launch.h, its plan: tsim_hip.hip ts_plan).
//
// What it computes, per environment and frame f of the window (DESIGN.md §4 "Parameter Jacobians"), with x = (q, qd) and p the selected columns of
// the environment's contact-group parameters (ts_pg_count's compact vector: pair kn kt mu kd, sensor kn kt mu kd, dof damping):
//     E_f = dx_{f+1} / dp at fixed (x_f, u_f)   [2 nr][ncols] ,   F_f = dtactile / dp at fixed x_{f+1}, stored compactly: Ft [4][ndof_tactile]
// E by k_tangent's BDF1 recursion (tsim_tangent.h) over the frame's taped sub-steps, every column starting at zero and driven by its own
// -(dg/dp_col); F from the frame's LAST tape record alone (row k: every taxel w.r.t. field k — kn kt mu kd — of its OWN sensor).  A frame's
// matrices depend on that frame's tape records alone, so a slot is (environment, frame) on the parameter passes' scaffold (tsim_param_pass.h,
// chunk = frame), as the frame Jacobians' is.
#pragma once
#include <hip/hip_runtime.h>
#include "tsim_param_grad.h"
#include "tsim_frame_jacobian.h"      // TS_FJ_RHS: the right-hand sides of one elimination

enum { TS_PJ_MAX_COLS = 32 };      // = TSIM_PARAM_JACOBIAN_MAX_COLS of include/tsim.h

// LDS reals a slot holds next to its context (behind the contexts of all the block's slots, at PjArgs::xoff), sized for TS_PJ_MAX_COLS columns
// whatever the launch selects, so that the lanes per environment — and with them the order of every sum — depend neither on ncols nor on the
// outputs asked for:
//   X  [TS_PJ_MAX_COLS][2 nr]   the columns' tangents (dq, dqd) of the state one sub-step back
//   W  [TS_FJ_RHS][nr]          a pass's parameter terms -(dg/dp_col), then its sources, then its solutions
// (no mass matrix: h M dqd0 is k_tangent's own product, mass_times_z, per column — see tsim_param_jacobian.hip)
__host__ __device__ inline int ts_pj_slot_reals(int nr) { return (TS_PJ_MAX_COLS * 2 * nr + TS_FJ_RHS * nr + 3) & ~3; }

// PgCommon: nchunk = the frames, chunk_len = the sub-steps of a frame; z, part and P are not used
template <class R> struct PjArgs : PgCommon<R> {
  int cull;
  int xoff;                                                  // reals from the start of the block's LDS to slot 0's block
  int ncols;                                                 // selected columns (E_out); 0 without E_out
  int col[TS_PJ_MAX_COLS];                                   // their compact indices, in ts_pg_count order (read with uniform indices only)
  const int32_t* tac_slot;                                   // [nframes] slot of the frame in Ft_out or < 0: not masked (null: slot f)
  R *E_out, *Ft_out;                                         // [nframes][B][2 nr][ncols], [num_masked][B][4][ndof_tactile]; null: not written
};
