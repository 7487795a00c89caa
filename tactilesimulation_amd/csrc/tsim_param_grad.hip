// tsim_param_grad.hip — the parameter-gradient pass (include/tsim.h tsim_set_param_grad; the math: tsim_param_grad.h).
// Runs after the adjoint launch it belongs to (k_backward_z, which left z of every sub-step), on the same stream:
//   k_param_grad    slot = (environment, chunk of sub-steps), 16 / 32 / 64 lanes as the adjoint launch: per sub-step a value-only link sweep of the
//                   taped state, then per dynamics pair lanes = contact points (the wrench's parameter derivatives dotted with the z-weighted
//                   motion of the pair, one reduction of 4 numbers), the damping term, and at seeded sub-steps the tactile term over the taxels;
//   k_param_reduce  one thread per (environment, parameter): the chunks' partial sums added in chunk order into the caller's table gradient
//                   (the body pass's reduction too: the columns are an argument).
// The slot mapping, the sub-step header and the taped-state load are tsim_param_pass.h's, shared with k_param_grad_body.
// Built like the generic kernels (tsim_hip.hip): no fast-math flags, the fp64 instantiation follows the fp64 adjoint to round-off.
#include <hip/hip_runtime.h>
#include "tsim_kernels.h"
#include "tsim_param_pass.h"
#include "tsim_launch.h"

// Adds v[k] to out[i0 + k], k < 4.  Entry i of a slot's partial row is always touched by lane i % LPE of the slot — zeroing included — so every
// read-modify-write sees its own earlier stores (program order of one lane; no cross-lane ordering is relied on).
template <int LPE, class R> __device__ __forceinline__ void pg_add4(R* out, int i0, const R (&v)[4], int lane, bool valid) {
#pragma unroll
  for (int k = 0; k < 4; ++k) if (valid && lane == (i0 + k) % LPE) out[i0 + k] += v[k];
}

template <class R, bool EXPJ, int LPE>
__global__ void __launch_bounds__(TS_WAVE) k_param_grad(PgArgs<R> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  R* lds = reinterpret_cast<R*>(smem_raw);
  const int lane = threadIdx.x % LPE, chunk = pg_chunk<LPE>(a), e_ = pg_slot_env<LPE>(a, chunk);      // (the scaffold: tsim_param_pass.h)
  const bool valid = e_ < a.B;                                 // an idle slot of a chunk's last block repeats the last environment and stores nothing
  const int env = min(e_, a.B - 1);
  Ctx<R> c; pg_ctx<LPE>(a, lds, c, lane, env);
  const int nr = c.nr, REC = ts_rec(nr, c.nu, (int)sizeof(R), a.tk);
  const int npair = c.npair, nsensor = c.nsensor, ntac3 = 3 * c.ntax;
  R* out = pg_row(a, chunk, env);
  const int idamp = 4 * npair + 4 * nsensor;
  if (valid) for (int i = lane; i < idamp; i += LPE) out[i] = R(0);
  const bool bdf2_model = ts_u(c.I[TSIM_IH_INTEGRATOR]) == 2;
  R gdamp = R(0);                                             // this lane's dof: -sum z qd1 / ca
  const int j0 = chunk * a.chunk_len, j1 = min(a.n, j0 + a.chunk_len);
  for (int j = j0; j < j1; ++j) {
    const int t = pg_t(a, j);
    const R ca = pg_ca(c, bdf2_model && t >= 2);
    const R* rec = pg_rec(a, t, env, REC);
    TS_SYNC();
    if (lane < nr) { pg_load_state(a, c, rec, t, env, nr, lane); c.qa[lane] = R(0); }
    TS_SYNC();
    phase1<R, false, EXPJ>(c, lane, R(0), R(0), R(0));         // link poses, twists and joint columns W of the taped state
    TS_SYNC();
    if (lane < nr) gdamp -= c.z[lane] * c.qd[lane] / ca;       // g_j contains d_j qd_j / ca
    // ---- dynamics pairs: g_j contains W_j . (inB_j - inA_j) Ww / ca (pair_fold, phase3), Ww the pair's wrench in the world frame.  So
    //      -z^T dg/dp = -(Z . dWw/dp) / ca with Z = sum_j z_j (inB_j - inA_j) W_j, and Z . Ww = Zp . w for the wrench w = (sum x x F, sum F) in the
    //      primitive frame and Zp = Z in that frame: per contact point x, dF/dp . (Zp_l + Zp_a x x).
    for (int pk = 0; pk < npair; ++pk) {
      const int* pi = c.I + c.off_pair + pk * TSIM_PI_SIZE;
      const int flags = ts_u(pi[TSIM_PI_FLAGS]);
      if (!(flags & 1)) continue;                              // sensing only: no force in the dynamics, exactly zero
      TS_SYNC();
      const bool near_ = pair_stage_value(c, pk, 0, lane == 0);
      TS_SYNC();
      if (!__any(near_)) continue;                             // the pair's points are out of reach of its primitive (exact: pair_stage_value)
      const int la = ts_u(pi[TSIM_PI_LINKA]), lb = ts_u(pi[TSIM_PI_LINKB]);
      R zw[6] = {R(0), R(0), R(0), R(0), R(0), R(0)};
      if (lane < nr) {
        const R inA = ((anc_of(c.I, c.off_link, la) >> lane) & 1) ? R(1) : R(0);
        const R inB = ((anc_of(c.I, c.off_link, lb) >> lane) & 1) ? R(1) : R(0);
        const S6<R> w = ld6(c.WP + lane * 6) * (c.z[lane] * (inB - inA));
        zw[0] = w.a.x; zw[1] = w.a.y; zw[2] = w.a.z; zw[3] = w.l.x; zw[4] = w.l.y; zw[5] = w.l.z;
      }
      seg_sum_many<LPE, 6>(zw);
      const R* S = c.PP;
      const S6<R> Zp = to_frame(ldm(S + PP_RP), ldv(S + PP_PP), mk6<R>(mk3<R>(zw[0], zw[1], zw[2]), mk3<R>(zw[3], zw[4], zw[5])));
      const M3<double> RPAd = ldm(c.PPd); const V3<double> pPAd = ldv(c.PPd + 9);
      const V3<R> wrel = ldv(S + PP_WREL), vrel = ldv(S + PP_VREL);
      const int pt0 = ts_u(pi[TSIM_PI_PT0]), npt = ts_u(pi[TSIM_PI_NPT]), prim = ts_u(pi[TSIM_PI_PRIM]);
      const R* pf = c.F + c.foff_pair + pk * TSIM_PF_SIZE;
      R s4[4] = {R(0), R(0), R(0), R(0)};
      for (int base = 0; base < npt; base += LPE) {
        if (base + lane >= npt) continue;
        const V3<R> cp = ld_cpt(c, pt0 + base + lane);
        V3<double> xPd = mulMv(RPAd, cvt3<double>(cp)) + pPAd;
        if (flags & 2) xPd.z -= (double)pf[TSIM_PF_SHAPE];   // sphere on plane: the sphere's lowest point (pair_points_matrix)
        const V3<R> xP = cvt3<R>(xPd);
        V3<R> F; M3<R> Jx, Jv; ContactGeo<R> geo;
        if (contact_law<R, false>(prim, pf + TSIM_PF_SHAPE, pf + TSIM_PF_KN, xP, vrel + cross3(wrel, xP), F, Jx, Jv, xPd, nullptr, false, &geo)) {
          V3<R> dF[4];
          contact_law_dparam(geo, pf + TSIM_PF_KN, dF);
          const V3<R> vP = Zp.l + cross3(Zp.a, xP);
#pragma unroll
          for (int k = 0; k < 4; ++k) s4[k] += dot3(dF[k], vP);
        }
      }
      seg_sum_many<LPE, 4>(s4);
#pragma unroll
      for (int k = 0; k < 4; ++k) s4[k] = -s4[k] / ca;
      pg_add4<LPE>(out, 4 * pk, s4, lane, valid);
    }
    // ---- sensors: the tactile output of a seeded frame is  o = A^T sum_prim R_PA^T F(x; sensor's kn kt mu kd)  per taxel (readout), so
    //      w . do/dp = sum over taxels and primitives of  wP . dF/dp,  wP = R_PA A w  (vjp_taxels)
    const bool seeded = (j + 1) % a.seed_stride == 0;
    if (seeded && a.df_dtac && ntac3) {
      const int fr = j / a.seed_stride;
      const size_t so = a.frames ? (size_t)fr * a.B + env : (size_t)env * (a.n / a.seed_stride) + fr;
      const int tslot = (a.frames && a.tac_slot) ? a.tac_slot[fr] : 0;
      const size_t sot = (a.frames && a.tac_slot) ? (size_t)max(tslot, 0) * a.B + env : so;
      if (__any(tslot >= 0)) {                                 // (the same frame in every slot of the wavefront: uniform)
        const R* wtac = a.df_dtac + sot * ntac3;
        for (int s = 0; s < nsensor; ++s) {
          const int* si = c.I + c.off_sensor + s * TSIM_SI_SIZE;
          const R* sf = c.F + c.foff_sensor + s * TSIM_SF_SIZE;
          const int t0 = ts_u(si[TSIM_SI_TAX0]), nt = ts_u(si[TSIM_SI_NTAX]), sp0 = ts_u(si[TSIM_SI_SPRIM0]), nsp = ts_u(si[TSIM_SI_NSPRIM]);
          R s4[4] = {R(0), R(0), R(0), R(0)};
          for (int jp = 0; jp < nsp; ++jp) {
            const int pk = ts_u(c.I[c.off_sprim + sp0 + jp]);
            const int prim = ts_u(c.I[c.off_pair + pk * TSIM_PI_SIZE + TSIM_PI_PRIM]);
            const R* shape = c.F + c.foff_pair + pk * TSIM_PF_SIZE + TSIM_PF_SHAPE;
            TS_SYNC();
            pair_stage_value(c, pk, 0, lane == 0);
            TS_SYNC();
            const R* S = c.PP;
            const M3<double> RPAd = ldm(c.PPd); const V3<double> pPAd = ldv(c.PPd + 9);
            const M3<R> RPA = ldm(S + PP_RPA);
            const V3<R> wrel = ldv(S + PP_WREL), vrel = ldv(S + PP_VREL);
            for (int base = 0; base < nt; base += LPE) {
              if (base + lane >= nt || tslot < 0) continue;
              const int tx = t0 + base + lane;
              const R w0 = wtac[3 * tx], w1 = wtac[3 * tx + 1], w2 = wtac[3 * tx + 2];
              if (w0 == R(0) && w1 == R(0) && w2 == R(0)) continue;
              const R* tp = c.Fg + c.foff_tax + tx;
              const V3<double> xPd = mulMv(RPAd, mk3<double>((double)tp[0], (double)tp[c.ntax], (double)tp[2 * c.ntax])) + pPAd;
              const V3<R> xP = cvt3<R>(xPd);
              V3<R> F; M3<R> Jx, Jv; ContactGeo<R> geo;
              if (!contact_law<R, false>(prim, shape, sf, xP, vrel + cross3(wrel, xP), F, Jx, Jv, xPd, nullptr, false, &geo)) continue;
              V3<R> dF[4];
              contact_law_dparam(geo, sf, dF);
              const V3<R> wl = mk3<R>(w0 * tp[3 * c.ntax] + w1 * tp[6 * c.ntax] + w2 * tp[9 * c.ntax],
                                      w0 * tp[4 * c.ntax] + w1 * tp[7 * c.ntax] + w2 * tp[10 * c.ntax],
                                      w0 * tp[5 * c.ntax] + w1 * tp[8 * c.ntax] + w2 * tp[11 * c.ntax]);
              const V3<R> wP = mulMv(RPA, wl);
#pragma unroll
              for (int k = 0; k < 4; ++k) s4[k] += dot3(dF[k], wP);
            }
          }
          seg_sum_many<LPE, 4>(s4);
          pg_add4<LPE>(out, 4 * npair + 4 * s, s4, lane, valid);
        }
      }
    }
  }
  if (valid && lane < nr) out[idamp + lane] = gdamp;
}

// Either pass's reduction (PgReduceArgs: the segments of the pass's compact vector and the columns they belong to)
template <class R>
__global__ void __launch_bounds__(256) k_param_reduce(PgReduceArgs<R> a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.B * a.P) return;
  const int env = i / a.P, p = i - env * a.P;
  PgSeg g = a.seg[0];
  int q = p;
  if (q >= g.count) { q -= g.count; g = a.seg[1]; if (q >= g.count) { q -= g.count; g = a.seg[2]; } }
  if (!g.on) return;
  R s = R(0);
  for (int k = 0; k < a.nchunk; ++k) s += a.part[((size_t)k * a.B + env) * a.P + p];      // fixed order: bit-identical from run to run
  a.out[(size_t)env * a.stride + g.col0 + (q / g.per) * g.rec + q % g.per] += s;
}

// the launch itself: tsim_launch.h, as every simulation kernel's (the plan: tsim_hip.hip launch_param_pass)
template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const PgArgs<float>&);
template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const PgArgs<double>&);
void ts_param_reduce_launch(const PgReduceArgs<float>& a, hipStream_t st) {
  hipLaunchKernelGGL(k_param_reduce<float>, dim3((unsigned)((a.B * a.P + 255) / 256)), dim3(256), 0, st, a);
}
void ts_param_reduce_launch(const PgReduceArgs<double>& a, hipStream_t st) {
  hipLaunchKernelGGL(k_param_reduce<double>, dim3((unsigned)((a.B * a.P + 255) / 256)), dim3(256), 0, st, a);
}
