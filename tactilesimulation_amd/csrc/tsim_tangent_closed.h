// tsim_tangent_closed.h — the policy half of the forward-mode tangent pass through the fused closed-loop episode (csrc/tsim_tangent_closed.hip
// k_closed_tangent; include/tsim_env.h tsim_push_closed_tangent, which states the recursion and the frame-0 convention).
//
// k_closed_tangent is ts_tangent_walk (tsim_tangent_kernel.h) with POLICY on: at a frame's start the frame's du is not read from TanArgs::du but
// formed here, in the slot, as the exact transpose of push_policy_backward (tsim_policy_push.h) — observation tangent from the tangent state at
// the frame's start and the tactile tangent this slot wrote at the previous frame's end, the three dense layers around the recorded ELU outputs
// with the per-layer sources (policy-parameter directions), the tanh of the recorded pre-tanh output, the caller's dact.
#pragma once
#include <hip/hip_runtime.h>
#include "tsim_kernels.h"
#include "tsim_policy_push.h"
#include "tsim_tangent.h"

template <class R> struct TanClosedArgs : TanArgs<R> {      // (TanArgs::du and TanArgs::tac_slot are not read: du is formed in the slot, frame f's tactile tangent is row f)
  PushPolicy<R> pol;                                         // forward layouts W1T, b*, W2T, W3; goal; the records u_out, h1_out, h2_out (read only)
  const R *s1, *s2, *s3;                                     // [ndir][nframes][B][64 | 64 | 3] sources on the layers' pre-activations; null: zeros
  const R* dact;                                             // [ndir][nframes][B][6] direct tangent of the applied action; null: zeros
  const R* dtac0;                                            // [ndir][B][390] tangent of the tactile part of the first observation; null: zeros
  R *dupol_out, *du_out;                                     // [ndir][nframes][B][3], [ndir][nframes][B][6]; null: not written
};

// Frame fr begins: TU_d (the six actuator inputs' tangent the frame's sub-steps use) for every direction d, one direction at a time through the
// policy scratch (pp_scr: the pair-staging records, idle between two frames).  The dense layers run wave-wide (pp_dense64: lane of the wavefront =
// output unit, all slots at once), the output layer and the action mapping per slot.  c.q0 is the taped state before the frame (the value
// push_policy_backward is given), TS the slot's tangent state at the frame's start.
template <int LPE, class R>
__device__ __forceinline__ void ts_closed_policy_tangent(const Ctx<R>& c, int lane, bool valid, const TanClosedArgs<R>& a, int fr, int env, const R* TS, R* TU, int DS) {
  constexpr int OPL = PP_HID / LPE, NS = TS_WAVE / LPE;
  const PushPolicy<R>& P = a.pol;
  const PPScr<LPE, R> S = pp_scr<LPE>(c);
  const int mode = ts_u(P.mode), nin = ts_u(P.nin), nin_pad = ts_u(P.nin_pad);
  const int B = a.B, T = a.nframes, ndir = a.ndir;
  const size_t rec = (size_t)fr * B + env, TB_ = (size_t)T * B;
  const int unit = (int)threadIdx.x;
  // per slot of the wavefront: its record of the frame, and elu' of this lane's unit from the recorded outputs
  size_t recs[NS]; R e1[NS], e2[NS];
#pragma unroll
  for (int s_ = 0; s_ < NS; ++s_) {
    recs[s_] = (size_t)fr * B + min((int)blockIdx.x * NS + s_, B - 1);
    e1[s_] = pp_elu_grad_from_output(P.h1_out[recs[s_] * PP_HID + unit]);
    e2[s_] = pp_elu_grad_from_output(P.h2_out[recs[s_] * PP_HID + unit]);
  }
  double fac = 0.0;                                     // 1 - tanh^2 of the recorded pre-tanh output (lanes 0..2)
  if (lane < 3) { const double t = tanh((double)P.u_out[rec * 3 + lane]); fac = 1.0 - t * t; }
  double sn, cs; t_sincos_d((double)c.q0[0], sn, cs);
  const R* g = P.goal + (size_t)env * 3;
  const double gx = g[0], gy = g[1], ox = (double)c.q0[3], oy = (double)c.q0[4];
  if (mode == TSIM_PUSH_OBS_TACTILE && fr > 0) ts_own_stores_visible();      // dtac_out[d][fr - 1] is this slot's own earlier store
  for (int d = 0; d < ndir; ++d) {
    // ---- the observation's tangent into LDS.  Frame 0: the goal / pose part is zero (the adjoint does not propagate the first observation's
    //      dependence on the initial state), the tactile part is the caller's dtac0
    const R* dq = TS + d * DS;
    R dgl = R(0), dobj = R(0);
    if (fr > 0 && lane < 3) {
      const double d0 = (double)dq[0];
      dgl = lane == 0 ? (R)((-sn * gx + cs * gy) * d0 - (double)dq[1]) : (lane == 1 ? (R)((-cs * gx - sn * gy) * d0 - (double)dq[2]) : (R)(-d0));
      if (mode == TSIM_PUSH_OBS_PRIVILEGE)
        dobj = lane == 0 ? (R)((-sn * ox + cs * oy) * d0 + cs * (double)dq[3] + sn * (double)dq[4] - (double)dq[1])
             : (lane == 1 ? (R)((-cs * ox - sn * oy) * d0 - sn * (double)dq[3] + cs * (double)dq[4] - (double)dq[2]) : (R)((double)dq[6] - d0));
    }
    if (mode == TSIM_PUSH_OBS_TACTILE) {
      constexpr int NX = (PP_OBS_PAD - 3 + LPE - 1) / LPE;
      const R* tsrc = fr == 0 ? (a.dtac0 ? a.dtac0 + ((size_t)d * B + env) * PP_NTAC : nullptr)
                              : a.dtac_out + (((size_t)d * T + (fr - 1)) * B + env) * PP_NTAC;
      R xv[NX];
#pragma unroll
      for (int m = 0; m < NX; ++m) { const int i = lane + LPE * m; xv[m] = (tsrc && i < PP_NTAC) ? __builtin_nontemporal_load(tsrc + i) : R(0); }
      if (lane < 3) S.xs[lane] = dgl;
#pragma unroll
      for (int m = 0; m < NX; ++m) { const int i = lane + LPE * m; if (3 + i < PP_OBS_PAD) S.xs[3 + i] = xv[m]; }
    } else {
      for (int i = lane; i < nin_pad; i += LPE) S.xs[i] = R(0);
      const int go = mode == TSIM_PUSH_OBS_PRIVILEGE ? 3 : 0;
      if (lane < 3) S.xs[go + lane] = dgl;
      if (mode == TSIM_PUSH_OBS_PRIVILEGE && lane < 3) S.xs[lane] = dobj;
    }
    TS_SYNC();
    // ---- dh1 = elu'(h1) (W1 dobs + s1), dh2 = elu'(h2) (W2 dh1 + s2): wave-wide, lane = unit
    R acc[NS];
#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) acc[s_] = a.s1 ? a.s1[((size_t)d * TB_ + recs[s_]) * PP_HID + unit] : R(0);
    pp_dense64<NS, PP_ROWS1>(P.W1T, nin_pad, nin, S.xs0, S.stride, acc);
#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) S.hs0[s_ * S.stride + unit] = e1[s_] * acc[s_];
    TS_SYNC();
#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) acc[s_] = a.s2 ? a.s2[((size_t)d * TB_ + recs[s_]) * PP_HID + unit] : R(0);
    pp_dense64<NS, PP_ROWS2>(P.W2T, PP_HID, PP_HID, S.hs0, S.stride, acc);
#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) S.hs0[s_ * S.stride + PP_HID + unit] = e2[s_] * acc[s_];
    TS_SYNC();
    // ---- dupol = W3 dh2 + s3 per slot, then the action mapping: du_act = [(1 - tanh^2(u)) dupol, 0, 0, 0] + dact
    R h2[OPL], w[OPL], up[3];
    pp_ld<OPL>(S.hs + PP_HID + OPL * lane, h2);
#pragma unroll
    for (int a_ = 0; a_ < 3; ++a_) {
      pp_ld<OPL>(P.W3 + (size_t)a_ * PP_HID + OPL * lane, w);
      R s = R(0);
#pragma unroll
      for (int o = 0; o < OPL; ++o) s += w[o] * h2[o];
      up[a_] = seg_sum<LPE>(s) + (a.s3 ? a.s3[((size_t)d * TB_ + rec) * PP_ACT + a_] : R(0));
    }
    if (lane < 6) {
      R v = R(0);
      if (lane < 3) {
        const R dup = lane == 0 ? up[0] : (lane == 1 ? up[1] : up[2]);
        v = (R)((double)dup * fac);
        if (valid && a.dupol_out) a.dupol_out[((size_t)d * TB_ + rec) * PP_ACT + lane] = dup;
      }
      if (a.dact) v += a.dact[((size_t)d * TB_ + rec) * 6 + lane];
      TU[d * DS + lane] = v;
      if (valid && a.du_out) a.du_out[((size_t)d * TB_ + rec) * 6 + lane] = v;
    }
    TS_SYNC();                                         // the scratch is the next direction's, then the pair staging of the sub-step
  }
}
