// tsim_adjoint_pre.h — the seed pre-pass of the fused episode adjoint and the chain kernel that reads its result (tsim_adjoint_pre.hip).
//
// The fused k_backward (tsim_kernels_backward.h) is one wavefront per SIMD that walks n sub-steps one after another.  On the sub-step that
// ends a frame it ran ts_static_output_vjp: a link sweep with tangents, the (sensor, primitive) poses and the taxel loop of the tactile seed.
// None of that reads lambda or z: it depends on the taped state and on the caller's seeds alone.  In the chain it cost 0.19 of k_backward's
// 0.49 ms per 20-step launch at B = 4096 (profiles/r30_adjoint_prepass.md).
//   k_adjoint_seeds   one item = (frame f, environment) of the launch, four items per wavefront at 16 lanes each — the chain kernel's own lane
//                     mapping, so ts_static_output_vjp runs unchanged and sums in the same order: the vectors are the in-kernel path's, bit for bit.
//                     It writes sseed[f][env][sq (nr) | sv (nr)],  sq = (dvar/dq)^T w_var + (dtac/dq)^T w_tac,  sv = (dtac/dqd)^T w_tac,  at the taped
//                     state as k_backward stages it (q, qd of record t, qdd = (qd_t - qd_{t-1}) / h).  f counts the frames of THIS launch (0: oldest).
//                     No atomics; a slot's result does not depend on its neighbours.  Its block holds the float tables and 56 reals per slot in
//                     LDS, not the contexts of the simulation kernels, and several wavefronts share a SIMD.
//   k_backward_pre    k_backward with PRE on: a seeded sub-step adds df_dq, then sq and sv (fetched one iteration ahead, next to H and K).
// The mass matrix stays in the chain (ts_static_mass_times_z): the scheduler already hides most of its sweep under the fp64 solve, and taking it out
// measured 0.037 ms per launch, below what a pass over (environment, sub-step) items and its 230 MB buffer would have to pay back (same note).
// fp32, 16 lanes, BDF1, TsStaticPusher and TsParam<TsStaticPusher>; everything else keeps the in-kernel path (tsim_hip.hip launch_backward).
#pragma once
#include "tsim_launch.h"

// LDS of a k_adjoint_seeds block, in reals: the float records (one copy, or one per slot with per-environment tables), then per slot
// qD [8] as doubles and q, qd, qa, lamq, lamv [8] each
__host__ __device__ inline int ts_ap_tab_reals(int nfrec, int nslot, bool env_tables) { return ((env_tables ? nslot : 1) * (nfrec + 2) + 3) & ~3; }
__host__ __device__ inline int ts_ap_slot_reals(int esz) { return 8 * (8 / esz) + 5 * 8; }
__host__ __device__ inline size_t ts_ap_lds_bytes(int nfrec, int nslot, bool env_tables, int esz) {
  return (size_t)(ts_ap_tab_reals(nfrec, nslot, env_tables) + nslot * ts_ap_slot_reals(esz)) * esz;
}

// (wavefronts per SIMD the registers are budgeted for: four, fully static, at 119 VGPRs; the structure-static twin spills at 128 and gets three)
template <class R, int LPE, class MS>
__global__ void __launch_bounds__(TS_WAVE) __attribute__((amdgpu_waves_per_eu(MS::PARAM ? 3 : 4))) k_adjoint_seeds(BwdArgs<R> a, R* sseed) {
  using T = TsTopo<MS>;
  static_assert(T::NR <= 8 && T::NR <= LPE, "k_adjoint_seeds: eight reals per slot array");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  R* lds = reinterpret_cast<R*>(smem_raw);
  constexpr int NS = TS_WAVE / LPE, nr = T::NR, nu = MS::Iv(TSIM_IH_NU), nfrec = MS::Iv(TSIM_IH_FOFF_CPT);
  const int slot = threadIdx.x / LPE, lane = threadIdx.x % LPE;
  const long long total = (long long)(a.n / a.seed_stride) * a.B, item0 = (long long)blockIdx.x * NS + slot;
  const bool valid = item0 < total;
  const long long item = valid ? item0 : total - 1;      // (a slot past the end repeats the last item and stores nothing)
  const int fr = (int)(item / a.B), env = (int)(item % a.B);
  // the context: what ts_static_output_vjp reads — the float records (from LDS), the sensor int records and taxel arrays (global), q / qd / qa
  Ctx<R> c{};
  R* mf = lds;
  if (a.Fenv) {
    mf += slot * (nfrec + 2);
    const R* Fe = a.Fenv + (size_t)env * a.fstride;
    for (int i = lane; i < nfrec; i += LPE) mf[i] = Fe[i];
  } else {
    for (int i = threadIdx.x; i < nfrec; i += TS_WAVE) mf[i] = a.F[i];
  }
  TS_SYNC();
  c.I = a.I; c.LI = a.I; c.F = mf; c.Fg = a.F; c.cull = a.cull;
  c.nl = MS::Iv(TSIM_IH_NL); c.nr = nr; c.nu = nu; c.nvar = MS::Iv(TSIM_IH_NVAR); c.npair = MS::Iv(TSIM_IH_NPAIR); c.ncpt = MS::Iv(TSIM_IH_NCPT);
  c.nsensor = MS::Iv(TSIM_IH_NSENSOR); c.ntax = a.I[TSIM_IH_NTAXEL]; c.nd = nr;      // (the taxel layout is the batch's own: blob_equals_static)
  c.off_link = MS::Iv(TSIM_IH_OFF_LINK); c.off_dof = MS::Iv(TSIM_IH_OFF_DOF); c.off_motor = MS::Iv(TSIM_IH_OFF_MOTOR); c.off_var = MS::Iv(TSIM_IH_OFF_VAR);
  c.off_pair = MS::Iv(TSIM_IH_OFF_PAIR); c.off_sensor = MS::Iv(TSIM_IH_OFF_SENSOR); c.off_sprim = MS::Iv(TSIM_IH_OFF_SPRIM);
  c.foff_link = MS::Iv(TSIM_IH_FOFF_LINK); c.foff_dof = MS::Iv(TSIM_IH_FOFF_DOF); c.foff_motor = MS::Iv(TSIM_IH_FOFF_MOTOR); c.foff_var = MS::Iv(TSIM_IH_FOFF_VAR);
  c.foff_pair = MS::Iv(TSIM_IH_FOFF_PAIR); c.foff_sensor = MS::Iv(TSIM_IH_FOFF_SENSOR); c.foff_cpt = nfrec; c.foff_tax = MS::Iv(TSIM_IH_FOFF_TAXEL);
  c.h = mf[TSIM_FH_H]; c.gx = mf[TSIM_FH_GX]; c.gy = mf[TSIM_FH_GY]; c.gz = mf[TSIM_FH_GZ]; c.tol = mf[TSIM_FH_TOL];
  c.cv = R(1) / c.h; c.ca = R(1) / (c.h * c.h);
  {
    R* p = lds + ts_ap_tab_reals(nfrec, NS, a.Fenv != nullptr) + slot * ts_ap_slot_reals((int)sizeof(R));
    c.qD = reinterpret_cast<double*>(p); p += 8 * (8 / (int)sizeof(R));
    c.q = p; p += 8; c.qd = p; p += 8; c.qa = p; p += 8; c.lamq = p; p += 8; c.lamv = p;
  }
  // the frame's last sub-step j of the launch's n, its tape record t and the one before it (k_backward's staging, BDF1)
  const int j = (fr + 1) * a.seed_stride - 1, t = a.t_end - (a.n - 1 - j);
  const int REC = ts_rec(nr, nu, (int)sizeof(R), a.tk), oqd = rec_qd<R>(nr);
  const R* r1 = a.tape + ((size_t)t * a.B + env) * REC;
  const R* r0 = a.tape + ((size_t)(t - 1) * a.B + env) * REC;
  if (lane < nr) {
    const double q1 = rec_q(r1)[lane];
    const R qd1 = r1[oqd + lane], qd0 = r0[oqd + lane];
    c.qD[lane] = q1; c.q[lane] = (R)q1; c.qd[lane] = qd1; c.qa[lane] = (qd1 - qd0) / c.h;
    c.lamq[lane] = R(0); c.lamv[lane] = R(0);
  }
  TS_SYNC();
  // the seeds of the frame, as k_backward picks them (frames = 1)
  const int nvar3 = 3 * c.nvar, ntac3 = 3 * c.ntax;
  const size_t so = (size_t)fr * a.B + env;
  const int tslot = a.tac_slot ? a.tac_slot[fr] : 0;
  const size_t sot = a.tac_slot ? (size_t)max(tslot, 0) * a.B + env : so;
  const R* wtac = (a.df_dtac && ntac3 && tslot >= 0) ? a.df_dtac + sot * ntac3 : nullptr;
  ts_static_output_vjp<R, LPE, MS>(c, lane, (a.df_dvar && nvar3) ? a.df_dvar + so * nvar3 : nullptr, wtac);      // lamq = 0 + sq, lamv = 0 + sv
  if (valid && lane < nr) {
    R* o = sseed + (size_t)item * (2 * nr);
    o[lane] = c.lamq[lane]; o[nr + lane] = c.lamv[lane];
  }
}

// the chain kernel behind it: the fused k_backward (no policy, no z saved) with PRE on
template <class R, int NRM, bool EXPJ, int LPE, class MS>
__global__ void TS_KLB_BWD k_backward_pre(BwdArgs<R> a, const R* sseed) {
  constexpr bool POLICY = false, SAVEZ = false, PRE = true; R* const zsave = nullptr;
  static_assert(ts_static_fused<MS, R>(), "k_backward_pre: a fused compiled-in model");
#include "tsim_kernels_backward.h"
}

// Launches k_adjoint_seeds, then k_backward_pre, on st for the plan's view (TS_KM_STATIC / TS_KM_PARAM; fp32, 16 lanes, NRM 8: the caller checks).
// plan: the k_backward plan of the launch (grid and LDS of the chain).  sseed: [n / seed_stride][B][2 nr] reals at least.  nfrec: the batch's
// staged float records.  False: no instantiation for the plan.
bool ts_adjoint_pre_launch(const TsPlan& plan, hipStream_t st, const BwdArgs<float>& a, float* sseed, int nfrec);
