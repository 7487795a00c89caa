// tsim_frame_jacobian.h — arguments and LDS layout of the per-frame transition Jacobians (csrc/tsim_frame_jacobian.hip k_frame_jacobian;
// include/tsim.h tsim_frame_jacobians; its launch: tsim_launch.h, its plan: tsim_hip.hip ts_plan).
//
// What it computes, per environment and frame f of the window (DESIGN.md §4 "Frame Jacobians"), with x = (q, qd):
//     A_f = dx_{f+1} / dx_f   [2 nr][2 nr] ,   B_f = dx_{f+1} / du_f   [2 nr][nu] ,   Jvar_f = dvariables / dq at the frame's end   [3 nvar][nr]
// by k_tangent's BDF1 recursion (tsim_tangent.h) over the frame's taped sub-steps, seeded with the identity: ncol = 2 nr + nu columns, column d < 2 nr
// the unit tangent of state entry d, column 2 nr + m the unit du of motor m held for the frame.  A frame's matrices depend on that frame's tape
// records alone, so a slot is (environment, frame) on the parameter passes' scaffold (tsim_param_pass.h, chunk = frame).
#pragma once
#include <hip/hip_runtime.h>
#include "tsim_param_grad.h"

enum { TS_FJ_RHS = 8 };      // right-hand sides one elimination of the taped Newton matrix carries (solve_lanes_many, tsim_eval.h)

// LDS reals a slot holds next to its context (behind the contexts of all the block's slots, at FjArgs::xoff):
//   X  [ncol][2 nr]    the columns' tangents (dq, dqd) of the state one sub-step back
//   MM [nr][nr]        the mass matrix of the taped point
//   W  [TS_FJ_RHS][nr] a pass's sources, then its solutions
//   DU [nu]            dtu / ca of the motors (0: a clipped force control)
__host__ __device__ inline int ts_fj_ncol(int nr, int nu) { return 2 * nr + nu; }
__host__ __device__ inline int ts_fj_slot_reals(int nr, int nu) { return (ts_fj_ncol(nr, nu) * 2 * nr + nr * nr + TS_FJ_RHS * nr + nu + 3) & ~3; }

// PgCommon: nchunk = the frames, chunk_len = the sub-steps of a frame; z, part and P are not used
template <class R> struct FjArgs : PgCommon<R> {
  int cull;
  int xoff;                                                  // reals from the start of the block's LDS to slot 0's block
  R *A_out, *B_out, *Jvar_out;                               // [nframes][B][2 nr][2 nr], [nframes][B][2 nr][nu], [nframes][B][3 nvar][nr]; null: not written
};
