// tsim_adjoint_pre.hip — k_adjoint_seeds and k_backward_pre (tsim_adjoint_pre.h) for the TactilePush model, fully static and structure-static, fp32 at
// 16 lanes per environment.  A unit of its own, so that no existing kernel's code moves; built with the static model's flags
// (-ffinite-math-only -fno-signed-zeros -O2, host/buildhash.py), as tsim_static_pusher.hip is: the pre-pass runs that unit's ts_static_output_vjp.
#include <hip/hip_runtime.h>
#include "tsim_adjoint_pre.h"

template <class MS>
static void adjoint_pre_launch(const TsPlan& plan, hipStream_t st, const BwdArgs<float>& a, float* sseed, int nfrec) {
  constexpr int LPE = 16, NS = TS_WAVE / LPE;
  const long long items = (long long)(a.n / a.seed_stride) * a.B;
  if (items > 0) {
    const size_t lds = ts_ap_lds_bytes(nfrec, NS, a.Fenv != nullptr, (int)sizeof(float));
    hipLaunchKernelGGL((k_adjoint_seeds<float, LPE, MS>), dim3((unsigned)((items + NS - 1) / NS)), dim3(TS_WAVE), lds, st, a, sseed);
  }
  hipLaunchKernelGGL((k_backward_pre<float, 8, false, LPE, MS>), dim3(plan.grid), dim3(TS_WAVE), plan.lds, st, a, (const float*)sseed);
}

bool ts_adjoint_pre_launch(const TsPlan& plan, hipStream_t st, const BwdArgs<float>& a, float* sseed, int nfrec) {
  if (plan.kernel != TS_K_BACKWARD || plan.policy || plan.lpe != 16 || plan.nrm != 8 || plan.expj || !plan.fused) return false;
  if (plan.variant == TS_KM_STATIC) { adjoint_pre_launch<TsStaticPusher>(plan, st, a, sseed, nfrec); return true; }
  if (plan.variant == TS_KM_PARAM) { adjoint_pre_launch<TsParamPusher>(plan, st, a, sseed, nfrec); return true; }
  return false;
}
