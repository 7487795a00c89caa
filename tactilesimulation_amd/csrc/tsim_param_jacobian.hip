// tsim_param_jacobian.hip — the per-frame parameter Jacobians of a taped episode in one launch (include/tsim.h tsim_param_jacobians; the math and
// the LDS layout: tsim_param_jacobian.h, DESIGN.md §4 "Parameter Jacobians").
//   k_param_jacobian   slot = (environment, frame) on the parameter passes' scaffold (tsim_param_pass.h, chunk = frame), 16 / 32 / 64 lanes per
//                      environment; every slot of a wavefront walks the same frame.  E: per sub-step the taped point is evaluated once, as
//                      k_frame_jacobian evaluates it (K = dg/dq in c.H, seeds (1, 0, 0)), and the selected columns' sources
//                      s = -K dq0 + h M dqd0 - dg/dp_col are solved TS_FJ_RHS at a time (solve_lanes_many, tsim_eval.h).  The source is formed
//                      with k_tangent's own operations in k_tangent's order — M (h dqd0) by mass_times_z per column, not by a mass matrix formed
//                      once: with a matrix formed from unit vectors the fp32 product rounds differently, the columns then differ from k_tangent's
//                      by 5e-6 of their scale, and through C that is over the tangent's 1e-4 on the tactile identity (profiles/r26) -, so that
//                      what is left between the two kernels is the elimination's last bit.  -dg/dp_col is
//                      k_tangent's parameter term for a unit direction (tsim_tangent_kernel.h "dynamics pairs"), restated here so that the
//                      tangent kernels' code does not move: G[field] of the column's dynamics pair on every dof lane, qd_j / ca on lane j for dof
//                      j's damping, nothing for a sensor column.  A pair is evaluated in the passes that hold one of its columns, and only there.
//                      F: at the frame's end the last taped point's link states are still in LDS; per sensor and paired primitive in the order
//                      of k_tangent's tactile section, lanes = taxels evaluate the contact law once and emit A^T R_PA^T dF/dp_k, k = kn kt mu kd.
// It reads the tape and writes the caller's buffers, nothing else.  With E_out null nothing is solved (phase 1 of the frame's last record only,
// so BDF2 and rotation-vector models are accepted there); with E_out, BDF1 models only (the host refuses a BDF2 model).
// Built like the generic kernels: no fast-math flags.  A unit of its own, so that no other kernel's code moves.
#include <hip/hip_runtime.h>
#include "tsim_kernels.h"
#include "tsim_param_pass.h"
#include "tsim_param_jacobian.h"
#include "tsim_launch.h"

template <class R, int NRM, bool EXPJ, int LPE>
__global__ void __launch_bounds__(TS_WAVE) k_param_jacobian(PjArgs<R> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  R* lds = reinterpret_cast<R*>(smem_raw);
  const int slot = threadIdx.x / LPE, lane = threadIdx.x % LPE, frame = pg_chunk<LPE>(a);      // (the scaffold: tsim_param_pass.h)
  const int tslot = !a.Ft_out ? -1 : a.tac_slot ? a.tac_slot[frame] : frame;
  const bool solve = a.E_out != nullptr;
  if (!solve && tslot < 0) return;      // nothing to do for this frame: the whole block (every slot is on this frame) leaves before it loads anything
  const int e_ = pg_slot_env<LPE>(a, frame);
  const bool valid = e_ < a.B;
  const int env = min(e_, a.B - 1);
  Ctx<R> c; pg_ctx<LPE>(a, lds, c, lane, env);
  c.cull = a.cull;
  const int nr = c.nr, nu = c.nu, ntax = c.ntax, npair = c.npair, nsensor = c.nsensor, REC = ts_rec(nr, nu, (int)sizeof(R), a.tk);
  const int oqd = rec_qd<R>(nr), oH = rec_H<R>(nr), ou = rec_u<R>(nr);
  const int XS = 2 * nr, ncols = a.ncols, idamp = 4 * npair + 4 * nsensor;
  // the slot's block (tsim_param_jacobian.h): column k at X + k * XS
  R* X = lds + a.xoff + slot * ts_pj_slot_reals(nr);
  R* W = X + TS_PJ_MAX_COLS * XS;
  for (int i = lane; i < ncols * XS; i += LPE) X[i] = R(0);      // x_f does not depend on p
  const int j1 = (frame + 1) * a.chunk_len;
  // without E nothing is solved: only the frame's last taped point is evaluated, for Ft
  for (int j = solve ? frame * a.chunk_len : j1 - 1; j < j1; ++j) {
    const int t = pg_t(a, j);
    const R* rec = pg_rec(a, t, env, REC);
    const R* rec0 = pg_rec(a, t - 1, env, REC);
    TS_SYNC();
    if (lane < nr) {      // the taped point, as k_frame_jacobian loads it
      pg_load_taped(c, rec, nr, lane);
      c.q0[lane] = (R)rec_q(rec0)[lane]; c.qd0[lane] = rec0[oqd + lane];
      c.qa[lane] = (c.qd[lane] - c.qd0[lane]) / c.h;
    }
    if (lane < nu) c.u[lane] = rec[ou + lane];
    for (int e = lane; e < nr * nr; e += LPE) c.H2[e] = rec[oH + e];      // the taped Newton matrix
    TS_SYNC();
    phase1<R, true, EXPJ>(c, lane, R(1), R(0), R(0));
    if (!solve) break;
    phase2<R, NRM, LPE>(c, lane, R(1));
    phase3<R, EXPJ, LPE>(c, lane, R(1), R(0));
    TS_SYNC();
    // ---- TS_FJ_RHS columns per pass: W = -dg/dp_col, s = -K dq0 + h M dqd0 + W, H y = s for all of them at once, dq1 = dq0 + y, dqd1 = cv y
    for (int c0 = 0; c0 < ncols; c0 += TS_FJ_RHS) {
      const int nb = min((int)TS_FJ_RHS, ncols - c0);
      // dof damping: g_j holds d_j qd_j / ca.  Every other column: zero until its pair is evaluated below (a sensor column: zero)
      if (lane < nr)
        for (int k = 0; k < nb; ++k) W[k * nr + lane] = a.col[c0 + k] - idamp == lane ? -(c.qd[lane] / c.ca) : R(0);
      // dynamics pairs: (dg/dp_k)_j = W_j . (inB_j - inA_j) dWw/dp_k / ca with dWw/dp_k the world form of (sum x x dF/dp_k, sum dF/dp_k) over
      // the contact points (k_tangent's "dynamics pairs", for unit directions)
      for (int pk = 0; pk < npair; ++pk) {
        bool sel = false;
        for (int k = 0; k < nb; ++k) sel = sel || (a.col[c0 + k] >> 2) == pk;      // (a compact index under 4 npair: pair pk's; others are >= 4 npair)
        if (!sel) continue;
        const int* pi = c.I + c.off_pair + pk * TSIM_PI_SIZE;
        const int flags = ts_u(pi[TSIM_PI_FLAGS]);
        if (!(flags & 1)) continue;                     // sensing only: no force in the dynamics, exactly zero
        TS_SYNC();
        const bool near_ = pair_stage_value(c, pk, 0, lane == 0);
        TS_SYNC();
        if (!__any(near_)) continue;
        const int la = ts_u(pi[TSIM_PI_LINKA]), lb = ts_u(pi[TSIM_PI_LINKB]);
        const R* S = c.PP;
        const M3<double> RPAd = ldm(c.PPd); const V3<double> pPAd = ldv(c.PPd + 9);
        const V3<R> wrel = ldv(S + PP_WREL), vrel = ldv(S + PP_VREL);
        const int pt0 = ts_u(pi[TSIM_PI_PT0]), npt = ts_u(pi[TSIM_PI_NPT]), prim = ts_u(pi[TSIM_PI_PRIM]);
        const R* pf = c.F + c.foff_pair + pk * TSIM_PF_SIZE;
        R w4[4][6];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int e = 0; e < 6; ++e) w4[k][e] = R(0);
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
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const V3<R> nk = cross3(xP, dF[k]);
              w4[k][0] += nk.x; w4[k][1] += nk.y; w4[k][2] += nk.z; w4[k][3] += dF[k].x; w4[k][4] += dF[k].y; w4[k][5] += dF[k].z;
            }
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) seg_sum_many<LPE, 6>(w4[k]);
        if (lane < nr) {
          const R inA = ((anc_of(c.I, c.off_link, la) >> lane) & 1) ? R(1) : R(0);
          const R inB = ((anc_of(c.I, c.off_link, lb) >> lane) & 1) ? R(1) : R(0);
          const M3<R> RP = ldm(S + PP_RP); const V3<R> pP = ldv(S + PP_PP);
          const S6<R> Wj = ld6(c.WP + lane * 6);
          R G[4];
#pragma unroll
          for (int k = 0; k < 4; ++k)
            G[k] = dot6(Wj, wrench_to_world(RP, pP, mk6<R>(mk3<R>(w4[k][0], w4[k][1], w4[k][2]), mk3<R>(w4[k][3], w4[k][4], w4[k][5])))) * (inB - inA) / c.ca;
          for (int k = 0; k < nb; ++k) {
            const int ci = a.col[c0 + k];
            if ((ci >> 2) != pk) continue;
            const int f = ci & 3;      // kn kt mu kd
            W[k * nr + lane] = -(f == 0 ? G[0] : f == 1 ? G[1] : f == 2 ? G[2] : G[3]);
          }
        }
      }
      TS_SYNC();
      for (int k = 0; k < nb; ++k) {      // k_tangent's "per direction": kv = -dq0, mv = h dqd0, s = K kv + M mv + TB
        const R* x = X + (c0 + k) * XS;
        if (lane < nr) c.z[lane] = c.h * x[nr + lane];
        TS_SYNC();
        const R ym = mass_times_z<LPE>(c, lane);      // (its scratch is c.PT, which no pair staging of this kernel's sub-step loop reads)
        if (lane < nr) {
          R kq = R(0);
          for (int i = 0; i < nr; ++i) kq += c.H[lane * nr + i] * -x[i];
          W[k * nr + lane] = kq + ym + W[k * nr + lane];
        }
      }
      TS_SYNC();
      solve_lanes_many<R, NRM, LPE, TS_FJ_RHS>(c.H2, W, nr, nb, lane);
      if (lane < nr) {
        for (int k = 0; k < nb; ++k) {
          R* x = X + (c0 + k) * XS;
          const R y = W[k * nr + lane];
          x[lane] += y; x[nr + lane] = c.cv * y;
        }
      }
      TS_SYNC();
    }
  }
  TS_SYNC();
  // ================================================================ the frame's end: E row-major (rows: the state at the end, columns: the selection)
  const size_t fe = (size_t)frame * a.B + env;
  if (valid && solve) {
    R* o = a.E_out + fe * XS * ncols;
    for (int e = lane; e < XS * ncols; e += LPE) { const int i = e / ncols, k = e - i * ncols; o[e] = X[k * XS + i]; }
  }
  if (tslot < 0) return;
  // ---- Ft: the parameter term of k_tangent's tactile expression, out = A^T R_PA^T F so d out / dp_k = A^T R_PA^T dF/dp_k, p the SENSOR's kn kt mu kd
  const size_t ntac3 = (size_t)3 * ntax;
  R* out = a.Ft_out + ((size_t)tslot * a.B + env) * 4 * ntac3;      // row k at out + k * ntac3: one tactile frame
  for (int s = 0; s < nsensor; ++s) {
    const int* si = c.I + c.off_sensor + s * TSIM_SI_SIZE;
    const R* sf = c.F + c.foff_sensor + s * TSIM_SF_SIZE;
    const int tx0 = ts_u(si[TSIM_SI_TAX0]), nt = ts_u(si[TSIM_SI_NTAX]), sp0 = ts_u(si[TSIM_SI_SPRIM0]), nsp = ts_u(si[TSIM_SI_NSPRIM]);
    for (int jp = 0; jp < nsp || jp == 0; ++jp) {
      const bool has_prim = jp < nsp;      // a sensor without primitives: its taxels' rows are exact zeros
      PairPose<R> Pp; int prim = 0; const R* shape = c.F;
      if (has_prim) {
        const int pk = ts_u(c.I[c.off_sprim + sp0 + jp]);
        prim = ts_u(c.I[c.off_pair + pk * TSIM_PI_SIZE + TSIM_PI_PRIM]);
        shape = c.F + c.foff_pair + pk * TSIM_PF_SIZE + TSIM_PF_SHAPE;
        TS_SYNC();
        pair_stage_value(c, pk, 0, lane == 0);
        TS_SYNC();
        const R* S = c.PP;
        Pp.RPAd = ldm(c.PPd); Pp.pPAd = ldv(c.PPd + 9);
        Pp.RPA = ldm(S + PP_RPA); Pp.pPA = ldv(S + PP_PPA); Pp.wrel = ldv(S + PP_WREL); Pp.vrel = ldv(S + PP_VREL);
      }
      for (int base = 0; base < nt; base += LPE) {
        if (base + lane >= nt) continue;
        const int tx = tx0 + base + lane;
        const R* tp = c.Fg + c.foff_tax + tx;
        bool live = false;
        V3<R> xP = zero3<R>(), F = zero3<R>(); M3<R> Jx, Jv; ContactGeo<R> geo;
        if (has_prim) {
          const V3<double> xPd = mulMv(Pp.RPAd, mk3<double>((double)tp[0], (double)tp[ntax], (double)tp[2 * ntax])) + Pp.pPAd;
          xP = cvt3<R>(xPd);
          live = contact_law<R, true>(prim, shape, sf, xP, Pp.vrel + cross3(Pp.wrel, xP), F, Jx, Jv, xPd, nullptr, true, &geo);
        }
        // one writer per element: this lane owns taxel tx in every primitive's pass, the first pass stores (an unloaded taxel: exact zeros), a
        // later one adds to its own earlier store
        if (!valid || (jp > 0 && !live)) continue;
        R* o = out + (size_t)3 * tx;
        V3<R> dFp[4];
        if (live) contact_law_dparam(geo, sf, dFp);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          R o0 = R(0), o1 = R(0), o2 = R(0);
          if (live) {
            const V3<R> vl = mulMtv(Pp.RPA, dFp[k]);
            o0 = tp[3 * ntax] * vl.x + tp[4 * ntax] * vl.y + tp[5 * ntax] * vl.z;
            o1 = tp[6 * ntax] * vl.x + tp[7 * ntax] * vl.y + tp[8 * ntax] * vl.z;
            o2 = tp[9 * ntax] * vl.x + tp[10 * ntax] * vl.y + tp[11 * ntax] * vl.z;
          }
          R* ok = o + k * ntac3;
          if (jp == 0) { ok[0] = o0; ok[1] = o1; ok[2] = o2; }
          else { ok[0] += o0; ok[1] += o1; ok[2] += o2; }
        }
      }
    }
  }
}

// the launch itself: tsim_launch.h, as every simulation kernel's (the plan: tsim_hip.hip ts_plan)
template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const PjArgs<float>&);
template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const PjArgs<double>&);
