// tsim_tangent.h — arguments and LDS layout of the forward-mode tangent pass (csrc/tsim_tangent.hip k_tangent; include/tsim.h tsim_tangent_episode;
// its launch: tsim_launch.h, its plan: tsim_hip.hip ts_plan).
//
// What it computes, per environment and direction d (DESIGN.md §4 "Tangent pass"): the derivative of the frames' outputs along
// (du_d, dq0_d, dqd0_d, dp_d), sub-step by sub-step over the tape and forwards in time — the transpose of what k_backward and k_param_grad do:
//     s = -K dq0 + h M dqd0 + D du - (dg/dp) dp ,   H y = s ,   dq1 = dq0 + y ,   dqd1 = cv y          (BDF1; BDF2: the four-history form)
// with H the taped Newton matrix, K = dg/dq of the taped point (c.H after phase3 with the seeds (1, 0, 0)) and M the mass matrix.
#pragma once
#include <hip/hip_runtime.h>
#include "tsim_param_grad.h"

enum { TS_TAN_MAX_DIR = 8 };      // = TSIM_TANGENT_MAX_DIR of include/tsim.h

// LDS reals a slot holds next to its context (behind the contexts of all the block's slots, at TanArgs::xoff), per direction:
//   TS [nhist][nr]  tangent of the state one step back (q, qd) and, for a BDF2 model (nhist = 4), two steps back
//   TP [P]          the direction's compact parameter vector (ts_pg_count: the contact columns of its dtables row; P = 0 without dtables)
//   TB [max(nr,12)] D du - (dg/dp) dp of the sub-step; at a frame's end the tangent of a (sensor, primitive) pair's relative pose and twist
//   TU [nu]         du of the frame
// The block is sized for the launch's own ndir — TactilePush at four environments per wavefront is within 3 KB of the 40 KB that let four blocks
// share a compute unit — but the lanes per environment are chosen for TS_TAN_MAX_DIR directions with parameters (tsim_hip.hip ts_plan), so the
// shape of the launch, and with it the order of every sum, depends neither on ndir nor on which inputs are given.
__host__ __device__ inline int ts_tan_dir_reals(int nr, int nu, int P, int nhist) { return nhist * nr + P + (nr > 12 ? nr : 12) + nu; }
__host__ __device__ inline int ts_tan_slot_reals(int nr, int nu, int P, int nhist, int ndir) { return (ndir * ts_tan_dir_reals(nr, nu, P, nhist) + 3) & ~3; }

template <class R> struct TanArgs {
  const int* I; const R* F; const R* Fenv; int fstride;      // fstride: tsim_table_size, the stride of Fenv AND of dtab
  int B, n, t_end, nsub, nframes, ndir;                      // the newest n = nframes x nsub taped sub-steps, t_end the newest
  int tk;                                                    // the tape records hold K (ts_rec)
  int stage_cpt, cull;
  int xoff;                                                  // reals from the start of the block's LDS to slot 0's tangent block
  const int* tac_slot;                                       // slot of frame f in dtac_out (< 0: none), null: slot f
  const R* tape;
  const R *du, *dq0, *dqd0, *dtab;                           // [ndir][nframes][B][nu], [ndir][B][nr] x 2, [ndir][B][fstride]; null: zeros
  R *dq_out, *dqd_out, *dvar_out, *dtac_out;                 // [ndir][nframes][B][.], dtac_out [ndir][n_masked][B][3 ntax]; null: not written
  const R* src;                                              // [ndir][n][B][nr]: the body columns' part of the source, -(dg/dp_body) dp_d per sub-step
                                                             // (k_tangent_body_src wrote it); null: none
};

// The body-group columns as directions (tsim_set_param_grad_groups: TSIM_PG_INERTIAL / MOTOR / LIMIT on, dtables given): their part of a sub-step's
// source depends on the taped state only, not on the tangents, so a pass of its own computes it for every sub-step at once before k_tangent runs
// (k_tangent_body_src, tsim_tangent_body.hip) — on the parameter passes' scaffold (PgCommon, tsim_param_pass.h: a slot is (environment, chunk of
// sub-steps); z, part and P are not used) — and k_tangent adds it where a direction's TB is finished.  It is k_param_grad_body read forwards.
template <class R> struct TanBodyArgs : PgCommon<R> {
  int groups;                                                // TS_PG_*: the body groups whose columns are read
  int ndir;
  const R* dtab;                                             // [ndir][B][fstride]
  R* src;                                                    // [ndir][n][B][nr], sub-step j of the launch's n at row j
};
