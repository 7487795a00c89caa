// tsim_launch.h — launch plans of the simulation kernels and the one launcher that runs them.
//
// A plan (TsPlan, made by tsim_hip.hip ts_plan and nowhere else) names one instantiation of k_forward, k_backward, k_backward_z, k_closed_backward_z, k_debug_eval,
// k_frame_records, k_param_grad, k_param_grad_body, k_tangent, k_tangent_body_src, k_closed_tangent, k_frame_jacobian, k_tactile_jacobian, k_param_jacobian or k_tactile_normal and the shape of its launch.  TsLaunch<MS, POLICY, R>::run launches it, for every view alike: MS = void, the generic kernels
// (tsim_hip.hip; the parameter passes: tsim_param_grad.hip, tsim_param_grad_body.hip; the tangent pass: tsim_tangent.hip, tsim_tangent_body.hip, tsim_tangent_closed.hip), or a compiled-in model (tsim_static.h), whose translation units hold nothing but the
// explicit instantiations of TsLaunch for their view: they are built with flags of their own (host/buildhash.py HIP_UNITS).
#pragma once
#include <type_traits>
#include "tsim_kernels.h"
#include "tsim_param_grad.h"
#include "tsim_tangent.h"
#include "tsim_tangent_closed.h"
#include "tsim_frame_jacobian.h"
#include "tsim_tactile_jacobian.h"
#include "tsim_param_jacobian.h"
#include "tsim_tactile_normal.h"
#include "tsim_static_pusher.h"

enum TsKernel { TS_K_FORWARD, TS_K_BACKWARD, TS_K_BACKWARD_Z, TS_K_DEBUG_EVAL, TS_K_PARAM_GRAD, TS_K_PARAM_GRAD_BODY, TS_K_FRAME_RECORDS,
                TS_K_CLOSED_BACKWARD_Z,        // the closed-loop adjoint that saves z (k_closed_backward_z): POLICY launches only
                TS_K_TANGENT,                  // the forward-mode tangent pass (k_tangent, tsim_tangent.hip): generic view only
                TS_K_TANGENT_BODY,             // its pre-pass for the body-group columns (k_tangent_body_src, tsim_tangent_body.hip): generic view only
                TS_K_CLOSED_TANGENT,           // the tangent pass through the fused closed loop (k_closed_tangent, tsim_tangent_closed.hip): generic view only, TactilePush (NRM 8)
                TS_K_FRAME_JACOBIAN,           // the per-frame transition Jacobians (k_frame_jacobian, tsim_frame_jacobian.hip): generic view only
                TS_K_TACTILE_JACOBIAN,         // the per-frame tactile Jacobians (k_tactile_jacobian, tsim_tactile_jacobian.hip): generic view only
                TS_K_PARAM_JACOBIAN,           // the per-frame parameter Jacobians (k_param_jacobian, tsim_param_jacobian.hip): generic view only
                TS_K_TACTILE_NORMAL };         // the tactile normal equations (k_tactile_normal, tsim_tactile_normal.hip): generic view only
// the view of a launch: the generic kernels, a compiled-in model fully static, or its structure-static twin (parameters at run time)
enum { TS_KM_GENERIC = 0, TS_KM_STATIC = 1, TS_KM_PARAM = 2 };
using TsParamPusher = TsParam<TsStaticPusher>;

struct TsPlan {
  int kernel = TS_K_FORWARD, variant = TS_KM_GENERIC;
  int nrm = 8; bool expj = false; int lpe = TS_WAVE;      // rows of the register solve, rotation-vector joint compiled in, lanes per environment
  bool policy = false;                                    // the TactilePush policy between the frames (tsim_policy_push.h)
  bool default_opts = false;                              // every option at its default: the TsDefaultOpts<> instantiation (tsim_static.h)
  bool frame_rec = false;                                 // ... and no frame ends in the kernel: k_forward_fr (set by launch_forward for such a launch)
  unsigned grid = 0; size_t lds = 0;
  bool fused = false;      // the view's model is FUSED (ts_static_fused): its forward writes K next to H on the tape, its adjoint reads it
};

// NRM of a view: 0 for the generic kernels (any), else the compiled-in model's
template <class MS> constexpr int ts_view_nrm() { return ts_static_nr<MS>() == 0 ? 0 : (ts_static_nr<MS>() <= 8 ? 8 : 16); }

// The instantiations there are, in one list: ts_plan runs the generic kernels where a compiled-in model has none, TsLaunch compiles exactly these
// (tests/test_capi_symbols.py pins the set).  Every view: NRM 8 / 16 at 16 / 32 / 64 lanes per environment, a rotation-vector joint only at NRM 16
// and 64 lanes; the closed loop: TactilePush's forward and adjoint and the adjoint's SAVEZ twin k_closed_backward_z (NRM 8), the twin nowhere else.  A compiled-in model (ms_nrm != 0): its own NRM, no parameter pass and no tangent pass;
// fp64 not at 16 lanes (four environments' LDS is over the cap); the closed loop and the debug kernel at fp32 and 16 lanes only; the TsDefaultOpts<>
// twin of the forward kernel at fp32 and 16 lanes, and there its k_forward_fr twin; k_frame_records wherever a FUSED compiled-in model has a forward kernel.
constexpr bool ts_instantiated(int kernel, int ms_nrm, bool fp32, bool policy, bool default_opts, int nrm, bool expj, int lpe) {
  if ((expj && (nrm != 16 || lpe != 64)) || (nrm != 8 && nrm != 16) || (lpe != 16 && lpe != 32 && lpe != 64)) return false;
  if (kernel == TS_K_CLOSED_TANGENT) return ms_nrm == 0 && !policy && !default_opts && nrm == 8 && !expj;      // (launched through the POLICY = false launcher: the policy is the kernel's own)
  if (policy != (kernel == TS_K_CLOSED_BACKWARD_Z) && kernel != TS_K_FORWARD && kernel != TS_K_BACKWARD) return false;
  if (policy && (nrm != 8 || expj)) return false;
  if (ms_nrm == 0) return !default_opts && kernel != TS_K_FRAME_RECORDS;
  if (kernel == TS_K_PARAM_GRAD || kernel == TS_K_PARAM_GRAD_BODY || kernel == TS_K_TANGENT || kernel == TS_K_TANGENT_BODY || kernel == TS_K_FRAME_JACOBIAN || kernel == TS_K_TACTILE_JACOBIAN || kernel == TS_K_PARAM_JACOBIAN || kernel == TS_K_TACTILE_NORMAL || nrm != ms_nrm || expj) return false;
  if (default_opts) return kernel == TS_K_FORWARD && fp32 && lpe == 16;
  if (policy || kernel == TS_K_DEBUG_EVAL) return fp32 && lpe == 16;
  return fp32 || lpe != 16;
}

template <class R, bool EXPJ, int LPE> __global__ void __launch_bounds__(TS_WAVE) k_param_grad(PgArgs<R> a);      // tsim_param_grad.hip
template <class R, bool EXPJ, int LPE> __global__ void __launch_bounds__(TS_WAVE) k_param_grad_body(PgBodyArgs<R> a);      // tsim_param_grad_body.hip
template <class R, int NRM, bool EXPJ, int LPE> __global__ void __launch_bounds__(TS_WAVE) k_tangent(TanArgs<R> a);      // tsim_tangent.hip
template <class R, int NRM, bool EXPJ, int LPE> __global__ void __launch_bounds__(TS_WAVE) k_tangent_src(TanArgs<R> a);      // tsim_tangent_body.hip: k_tangent that adds TanArgs::src
template <class R, bool EXPJ, int LPE> __global__ void __launch_bounds__(TS_WAVE) k_tangent_body_src(TanBodyArgs<R> a);      // tsim_tangent_body.hip
template <class R, int NRM, bool EXPJ, int LPE, bool SRC> __global__ void __launch_bounds__(TS_WAVE) k_closed_tangent(TanClosedArgs<R> a);      // tsim_tangent_closed.hip

template <class R, int NRM, bool EXPJ, int LPE> __global__ void __launch_bounds__(TS_WAVE) k_frame_jacobian(FjArgs<R> a);      // tsim_frame_jacobian.hip
template <class R, int NRM, bool EXPJ, int LPE> __global__ void __launch_bounds__(TS_WAVE) k_tactile_jacobian(TjArgs<R> a);      // tsim_tactile_jacobian.hip
template <class R, int NRM, bool EXPJ, int LPE> __global__ void __launch_bounds__(TS_WAVE) k_param_jacobian(PjArgs<R> a);      // tsim_param_jacobian.hip
template <class R, int NRM, bool EXPJ, int LPE> __global__ void __launch_bounds__(TS_WAVE) k_tactile_normal(TnArgs<R> a);      // tsim_tactile_normal.hip

template <int N> using TsInt = std::integral_constant<int, N>;
template <bool B> using TsBool = std::integral_constant<bool, B>;

// run(): the launch of the instantiation plan p names, in view MS (void: generic) with the policy or without; false where there is none (the
// plan is for another view or kernel).  The members are defined out of the class, not inline, so that `extern template` below keeps a
// compiled-in view's kernels out of every unit but its own.
template <class MS, bool POLICY, class R> struct TsLaunch {
  // f(NRM, EXPJ, LPE) as constants for the plan's shape, instantiated only where ts_instantiated lists the instantiation
  template <int K, class F> static bool shape(const TsPlan& p, F&& f) {
    if (p.kernel != K || p.policy != POLICY) return false;
    auto at = [&](auto nrm, auto expj, auto lpe) {
      if constexpr (ts_instantiated(K, ts_view_nrm<MS>(), sizeof(R) == 4, POLICY, false, nrm, expj, lpe)) { f(nrm, expj, lpe); return true; }
      else return false;
    };
    auto lanes = [&](auto nrm, auto expj) { return p.lpe == 16 ? at(nrm, expj, TsInt<16>()) : p.lpe == 32 ? at(nrm, expj, TsInt<32>()) : p.lpe == 64 && at(nrm, expj, TsInt<64>()); };
    if (p.expj) return p.nrm == 16 && lanes(TsInt<16>(), TsBool<true>());
    return p.nrm == 8 ? lanes(TsInt<8>(), TsBool<false>()) : p.nrm == 16 && lanes(TsInt<16>(), TsBool<false>());
  }
  static bool run(const TsPlan& p, hipStream_t st, const FwdArgs<R>& a);
  static bool run(const TsPlan& p, hipStream_t st, const FwdArgs<R>& a, int fpc, TsSubRange sub);      // k_frame_records (TS_K_FRAME_RECORDS): fpc frames per block, the environments of sub
  static bool run(const TsPlan& p, hipStream_t st, const BwdArgs<R>& a, R* zsave = nullptr);      // zsave: k_backward_z (TS_K_BACKWARD_Z), k_closed_backward_z
  static bool run_closed_z(const TsPlan& p, hipStream_t st, const BwdArgs<R>& a, R* zsave);      // TS_K_CLOSED_BACKWARD_Z; run() hands it over (a member of its own: the generic view's is instantiated in tsim_closed_backward_z.hip)
  static bool run(const TsPlan& p, hipStream_t st, const DbgArgs<R>& a);
  static bool run(const TsPlan& p, hipStream_t st, const PgArgs<R>& a);
  static bool run(const TsPlan& p, hipStream_t st, const PgBodyArgs<R>& a);
  static bool run(const TsPlan& p, hipStream_t st, const TanArgs<R>& a);
  static bool run(const TsPlan& p, hipStream_t st, const TanBodyArgs<R>& a);
  static bool run(const TsPlan& p, hipStream_t st, const FjArgs<R>& a);
  static bool run(const TsPlan& p, hipStream_t st, const TjArgs<R>& a);
  static bool run(const TsPlan& p, hipStream_t st, const PjArgs<R>& a);
  static bool run(const TsPlan& p, hipStream_t st, const TnArgs<R>& a);
  static bool run_tangent_src(const TsPlan& p, hipStream_t st, const TanArgs<R>& a);      // TS_K_TANGENT with a.src given: k_tangent_src (a member of its own: instantiated in tsim_tangent_body.hip)
  static bool run_closed_tangent(const TsPlan& p, hipStream_t st, const TanClosedArgs<R>& a);      // TS_K_CLOSED_TANGENT, SRC = (a.src given) (instantiated in tsim_tangent_closed.hip)
};

template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run(const TsPlan& p, hipStream_t st, const FwdArgs<R>& a) {
  return shape<TS_K_FORWARD>(p, [&](auto nrm, auto expj, auto lpe) {
    if constexpr (ts_instantiated(TS_K_FORWARD, ts_view_nrm<MS>(), sizeof(R) == 4, POLICY, true, nrm, expj, lpe)) {
      if (p.default_opts && p.frame_rec) {
        if constexpr (!POLICY && ts_static_fused<MS, R>()) { hipLaunchKernelGGL((k_forward_fr<R, nrm, lpe, MS>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a); return; }
      }
      if (p.default_opts) { hipLaunchKernelGGL((k_forward<R, nrm, expj, lpe, POLICY, TsDefaultOpts<MS>>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a); return; }
    }
    hipLaunchKernelGGL((k_forward<R, nrm, expj, lpe, POLICY, MS>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a);
  });
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run(const TsPlan& p, hipStream_t st, const FwdArgs<R>& a, int fpc, TsSubRange sub) {
  if constexpr (!POLICY && ts_static_fused<MS, R>())
    return shape<TS_K_FRAME_RECORDS>(p, [&](auto, auto, auto lpe) { hipLaunchKernelGGL((k_frame_records<R, lpe, MS>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a, fpc, sub); });
  else return false;
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run(const TsPlan& p, hipStream_t st, const BwdArgs<R>& a, R* zsave) {
  if (p.kernel == TS_K_CLOSED_BACKWARD_Z) return run_closed_z(p, st, a, zsave);
  if (p.kernel == TS_K_BACKWARD_Z)
    return shape<TS_K_BACKWARD_Z>(p, [&](auto nrm, auto expj, auto lpe) { hipLaunchKernelGGL((k_backward_z<R, nrm, expj, lpe, POLICY, MS>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a, zsave); });
  return shape<TS_K_BACKWARD>(p, [&](auto nrm, auto expj, auto lpe) { hipLaunchKernelGGL((k_backward<R, nrm, expj, lpe, POLICY, MS>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a); });
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run_closed_z(const TsPlan& p, hipStream_t st, const BwdArgs<R>& a, R* zsave) {
  return shape<TS_K_CLOSED_BACKWARD_Z>(p, [&](auto nrm, auto expj, auto lpe) { hipLaunchKernelGGL((k_closed_backward_z<R, nrm, expj, lpe, MS>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a, zsave); });
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run(const TsPlan& p, hipStream_t st, const DbgArgs<R>& a) {
  return shape<TS_K_DEBUG_EVAL>(p, [&](auto, auto, auto lpe) { hipLaunchKernelGGL((k_debug_eval<R, lpe, MS>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a); });
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run(const TsPlan& p, hipStream_t st, const PgArgs<R>& a) {
  return shape<TS_K_PARAM_GRAD>(p, [&](auto, auto expj, auto lpe) { hipLaunchKernelGGL((k_param_grad<R, expj, lpe>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a); });
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run(const TsPlan& p, hipStream_t st, const PgBodyArgs<R>& a) {
  return shape<TS_K_PARAM_GRAD_BODY>(p, [&](auto, auto expj, auto lpe) { hipLaunchKernelGGL((k_param_grad_body<R, expj, lpe>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a); });
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run(const TsPlan& p, hipStream_t st, const TanArgs<R>& a) {
  return shape<TS_K_TANGENT>(p, [&](auto nrm, auto expj, auto lpe) { hipLaunchKernelGGL((k_tangent<R, nrm, expj, lpe>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a); });
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run(const TsPlan& p, hipStream_t st, const TanBodyArgs<R>& a) {
  return shape<TS_K_TANGENT_BODY>(p, [&](auto, auto expj, auto lpe) { hipLaunchKernelGGL((k_tangent_body_src<R, expj, lpe>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a); });
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run(const TsPlan& p, hipStream_t st, const FjArgs<R>& a) {
  return shape<TS_K_FRAME_JACOBIAN>(p, [&](auto nrm, auto expj, auto lpe) { hipLaunchKernelGGL((k_frame_jacobian<R, nrm, expj, lpe>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a); });
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run(const TsPlan& p, hipStream_t st, const TjArgs<R>& a) {
  return shape<TS_K_TACTILE_JACOBIAN>(p, [&](auto nrm, auto expj, auto lpe) { hipLaunchKernelGGL((k_tactile_jacobian<R, nrm, expj, lpe>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a); });
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run(const TsPlan& p, hipStream_t st, const PjArgs<R>& a) {
  return shape<TS_K_PARAM_JACOBIAN>(p, [&](auto nrm, auto expj, auto lpe) { hipLaunchKernelGGL((k_param_jacobian<R, nrm, expj, lpe>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a); });
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run(const TsPlan& p, hipStream_t st, const TnArgs<R>& a) {
  return shape<TS_K_TACTILE_NORMAL>(p, [&](auto nrm, auto expj, auto lpe) { hipLaunchKernelGGL((k_tactile_normal<R, nrm, expj, lpe>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a); });
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run_tangent_src(const TsPlan& p, hipStream_t st, const TanArgs<R>& a) {
  return shape<TS_K_TANGENT>(p, [&](auto nrm, auto expj, auto lpe) { hipLaunchKernelGGL((k_tangent_src<R, nrm, expj, lpe>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a); });
}
template <class MS, bool POLICY, class R> bool TsLaunch<MS, POLICY, R>::run_closed_tangent(const TsPlan& p, hipStream_t st, const TanClosedArgs<R>& a) {
  return shape<TS_K_CLOSED_TANGENT>(p, [&](auto nrm, auto expj, auto lpe) {
    if (a.src) hipLaunchKernelGGL((k_closed_tangent<R, nrm, expj, lpe, true>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a);
    else hipLaunchKernelGGL((k_closed_tangent<R, nrm, expj, lpe, false>), dim3(p.grid), dim3(TS_WAVE), p.lds, st, a);
  });
}

// ... in the plan's view
template <bool POLICY, class R, class A, class... Z> bool ts_launch(const TsPlan& p, hipStream_t st, const A& a, Z... z) {
  if (p.variant == TS_KM_STATIC) return TsLaunch<TsStaticPusher, POLICY, R>::run(p, st, a, z...);
  if (p.variant == TS_KM_PARAM) return TsLaunch<TsParamPusher, POLICY, R>::run(p, st, a, z...);
  return TsLaunch<void, POLICY, R>::run(p, st, a, z...);
}
// instantiated in their own units: tsim_static_pusher.hip, tsim_param_pusher.hip, their _policy twins, tsim_param_grad.hip, tsim_param_grad_body.hip,
// tsim_closed_backward_z.hip, tsim_tangent.hip, tsim_tangent_body.hip, tsim_tangent_closed.hip, tsim_frame_jacobian.hip, tsim_tactile_jacobian.hip,
// tsim_param_jacobian.hip, tsim_tactile_normal.hip
extern template struct TsLaunch<TsStaticPusher, false, float>;
extern template struct TsLaunch<TsStaticPusher, false, double>;
extern template struct TsLaunch<TsStaticPusher, true, float>;
extern template struct TsLaunch<TsStaticPusher, true, double>;
extern template struct TsLaunch<TsParamPusher, false, float>;
extern template struct TsLaunch<TsParamPusher, false, double>;
extern template struct TsLaunch<TsParamPusher, true, float>;
extern template struct TsLaunch<TsParamPusher, true, double>;
extern template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const PgArgs<float>&);
extern template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const PgArgs<double>&);
extern template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const PgBodyArgs<float>&);
extern template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const PgBodyArgs<double>&);
extern template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const TanArgs<float>&);
extern template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const TanArgs<double>&);
extern template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const TanBodyArgs<float>&);
extern template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const TanBodyArgs<double>&);
extern template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const FjArgs<float>&);
extern template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const FjArgs<double>&);
extern template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const TjArgs<float>&);
extern template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const TjArgs<double>&);
extern template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const PjArgs<float>&);
extern template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const PjArgs<double>&);
extern template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const TnArgs<float>&);
extern template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const TnArgs<double>&);
extern template bool TsLaunch<void, false, float>::run_tangent_src(const TsPlan&, hipStream_t, const TanArgs<float>&);
extern template bool TsLaunch<void, false, double>::run_tangent_src(const TsPlan&, hipStream_t, const TanArgs<double>&);
extern template bool TsLaunch<void, false, float>::run_closed_tangent(const TsPlan&, hipStream_t, const TanClosedArgs<float>&);
extern template bool TsLaunch<void, false, double>::run_closed_tangent(const TsPlan&, hipStream_t, const TanClosedArgs<double>&);
extern template bool TsLaunch<void, true, float>::run_closed_z(const TsPlan&, hipStream_t, const BwdArgs<float>&, float*);
extern template bool TsLaunch<void, true, double>::run_closed_z(const TsPlan&, hipStream_t, const BwdArgs<double>&, double*);
void ts_closed_slots_launch(int32_t* slots, int nframes, hipStream_t st);      // tsim_closed_backward_z.hip: slots[f] = f, the last frame -1
