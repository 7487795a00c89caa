// tsim_tangent_kernel.h — the body of the forward-mode tangent kernel (tsim_tangent.hip, which says what it does), as a function of the launch's
// arguments with one switch: SRC, whether the body columns' part of the sources is added (TanArgs::src, written by k_tangent_body_src).  Two kernels
// are made of it: k_tangent (SRC = false, tsim_tangent.hip), instruction for instruction the kernel it was before the switch existed, and
// k_tangent_src (SRC = true, tsim_tangent_body.hip), launched only when a body group is on and dtables is given — reading src in the one kernel
// cost its fp64 instantiations 2 - 8 more spilled vector registers (profiles/r18_tangent_body.md).
// A second switch, POLICY (with the launch's argument type A = TanClosedArgs), makes k_closed_tangent (tsim_tangent_closed.hip): a frame's du is then
// not read from TanArgs::du but formed in the slot by the policy's tangent (tsim_tangent_closed.h).  Both switches are `if constexpr`: with POLICY off
// the body is the one it was.
#pragma once
#include <hip/hip_runtime.h>
#include "tsim_kernels.h"
#include "tsim_tangent.h"
#include "tsim_tangent_closed.h"

template <class R, int NRM, bool EXPJ, int LPE, bool SRC, bool POLICY = false, class A = TanArgs<R>>
__device__ __forceinline__ void ts_tangent_walk(const A& a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  R* lds = reinterpret_cast<R*>(smem_raw);
  constexpr int NS = TS_WAVE / LPE;
  const int slot = threadIdx.x / LPE, lane = threadIdx.x % LPE;
  const bool valid = (int)blockIdx.x * NS + slot < a.B;      // an idle slot of the last block repeats the last environment and stores nothing
  const int env = min((int)blockIdx.x * NS + slot, a.B - 1);
  Ctx<R> c; ctx_init<R>(c, a.I, a.F, lds, NS, slot, lane, LPE, a.stage_cpt != 0, a.Fenv ? a.Fenv + (size_t)env * a.fstride : nullptr);
  c.cull = a.cull;
  const int nr = c.nr, nu = c.nu, REC = ts_rec(nr, nu, (int)sizeof(R), a.tk);
  const int nvar = c.nvar, ntac3 = 3 * c.ntax, npair = c.npair, nsensor = c.nsensor;
  const int P = ts_pg_count(npair, nsensor, nr), idamp = 4 * npair + 4 * nsensor;
  const int ndir = a.ndir, T = a.nframes, B = a.B;
  R* H2 = c.H2;      // taped Newton matrix of the sub-step
  init_world(c, lane, LPE);
  // the slot's tangent block (tsim_tangent.h): direction d at TS + d * DS
  const bool bdf2_model = ts_u(c.I[TSIM_IH_INTEGRATOR]) == 2;
  const int NH = bdf2_model ? 4 : 2, PL = a.dtab ? P : 0, DS = ts_tan_dir_reals(nr, nu, PL, NH);
  R* TS = lds + a.xoff + slot * ts_tan_slot_reals(nr, nu, PL, NH, ndir);
  R* TP = TS + NH * nr;
  R* TB = TP + PL;
  R* TT = TB;                    // (TB is dead once the sub-step's directions are solved)
  R* TU = TB + (nr > 12 ? nr : 12);
  for (int d = 0; d < ndir; ++d) {
    if (lane < nr) {
      const size_t o = ((size_t)d * B + env) * nr + lane;
      TS[d * DS + lane] = a.dq0 ? a.dq0[o] : R(0);
      TS[d * DS + nr + lane] = a.dqd0 ? a.dqd0[o] : R(0);
      if (bdf2_model) { TS[d * DS + 2 * nr + lane] = R(0); TS[d * DS + 3 * nr + lane] = R(0); }
    }
    if (a.dtab) {      // the contact columns of the direction's row, in the order of ts_pg_count; no other entry is read
      const R* row = a.dtab + ((size_t)d * B + env) * a.fstride;
      for (int i = lane; i < P; i += LPE) {
        const int col = i < 4 * npair ? c.foff_pair + (i >> 2) * TSIM_PF_SIZE + TSIM_PF_KN + (i & 3)
                      : i < idamp ? c.foff_sensor + ((i - 4 * npair) >> 2) * TSIM_SF_SIZE + TSIM_SF_KN + ((i - 4 * npair) & 3)
                                  : c.foff_dof + (i - idamp) * TSIM_DF_SIZE + TSIM_DF_DAMPING;
        TP[d * DS + i] = row[col];
      }
    }
  }
  int nmask = T;      // rows of dtac_out per direction: the masked frames
  if (a.tac_slot) { nmask = 0; for (int f = 0; f < T; ++f) nmask = max(nmask, a.tac_slot[f] + 1); }
  TS_SYNC();
  // The tape record of sub-step t (q1, qd1, u, H) is fetched ONE ITERATION AHEAD into registers, as the adjoint kernel does backwards
  // (tsim_kernels_backward.h): record t supplies q1, qd1 now and q0, qd0 of the next iteration.
  constexpr int NHL = (NRM * NRM + LPE - 1) / LPE;
  const int oqd = rec_qd<R>(nr), oH = rec_H<R>(nr), ou = rec_u<R>(nr);
  const int t_first = a.t_end - a.n + 1;
  double pq1 = 0.0, pq0 = 0.0; R pqd1 = R(0), pqd0 = R(0), pqdm = R(0), pu = R(0), pH[NHL];     // pqdm: qd two records back (BDF2)
  {
    const R* r1 = a.tape + ((size_t)t_first * B + env) * REC;
    const R* r0 = a.tape + ((size_t)(t_first - 1) * B + env) * REC;
    if (lane < nr) { pq1 = rec_q(r1)[lane]; pqd1 = r1[oqd + lane]; pq0 = rec_q(r0)[lane]; pqd0 = r0[oqd + lane]; }
    if (bdf2_model && t_first >= 2 && lane < nr) pqdm = a.tape[((size_t)(t_first - 2) * B + env) * REC + oqd + lane];
    if (lane < nu) pu = r1[ou + lane];
#pragma unroll
    for (int i = 0; i < NHL; ++i) { const int e = lane + i * LPE; pH[i] = e < nr * nr ? r1[oH + e] : R(0); }
  }
  for (int j = 0; j < a.n; ++j) {
    const int t = t_first + j;
    const bool bdf2 = bdf2_model && t >= 2;
    c.cv = bdf2 ? R(1.5) / c.h : R(1) / c.h;
    c.ca = bdf2 ? R(2.25) / (c.h * c.h) : R(1) / (c.h * c.h);
    if (lane < nr) {
      c.qD[lane] = pq1; c.q[lane] = (R)pq1; c.q0[lane] = (R)pq0; c.qd0[lane] = pqd0;
      c.qd[lane] = pqd1;
      c.qa[lane] = bdf2 ? (R(3) * pqd1 - R(4) * pqd0 + pqdm) / (R(2) * c.h) : (pqd1 - pqd0) / c.h;      // as k_backward
    }
    if (lane < nu) c.u[lane] = pu;
#pragma unroll
    for (int i = 0; i < NHL; ++i) { const int e = lane + i * LPE; if (e < nr * nr) H2[e] = pH[i]; }
    if (j + 1 < a.n) {                                  // next iteration: sub-step t + 1
      const R* r1 = a.tape + ((size_t)(t + 1) * B + env) * REC;
      pqdm = pqd0; pq0 = pq1; pqd0 = pqd1;
      if (lane < nr) { pq1 = rec_q(r1)[lane]; pqd1 = r1[oqd + lane]; }
      if (lane < nu) pu = r1[ou + lane];
#pragma unroll
      for (int i = 0; i < NHL; ++i) { const int e = lane + i * LPE; pH[i] = e < nr * nr ? r1[oH + e] : R(0); }
    }
    // (issued here, a whole sub-step ahead of their use: see the note in tsim_kernels_backward.h)
    __builtin_amdgcn_sched_barrier(0);
    TS_SYNC();
    const int fr = j / a.nsub;
    if (j % a.nsub == 0) {                              // a frame begins: its du
      if constexpr (POLICY) ts_closed_policy_tangent<LPE>(c, lane, valid, a, fr, env, TS, TU, DS);      // ... from the policy's tangent, in the slot
      else {
        for (int d = 0; d < ndir; ++d)
          if (lane < nu) TU[d * DS + lane] = a.du ? a.du[(((size_t)d * T + fr) * B + env) * nu + lane] : R(0);
      }
    }
    // ---- the taped point, once for all directions: K = dg/dq in c.H (seeds (1, 0, 0)), link states and tangents in LDS
    phase1<R, true, EXPJ>(c, lane, R(1), R(0), R(0));
    phase2<R, NRM, LPE>(c, lane, R(1));
    phase3<R, EXPJ, LPE>(c, lane, R(1), R(0));
    // ---- TB_d = D du_d - (dg/dp) dp_d, lanes = dofs.  Motor: -(dg/du) = dtu / ca on the motor's dof (k_backward); damping: g_j holds d_j qd_j / ca
    if (lane < nr) {
      for (int d = 0; d < ndir; ++d) {
        R acc = R(0);
        for (int m = 0; m < nu; ++m) {
          const int* mi = ts_motor_rec(c, m);
          if (mi[TSIM_MI_DOF] != lane) continue;
          const R* mf = c.F + c.foff_motor + m * TSIM_MF_SIZE;
          R dtu;
          if (mi[TSIM_MI_CTRL] == 0) dtu = (c.u[m] >= R(-1) && c.u[m] <= R(1)) ? R(0.5) * (mf[TSIM_MF_HI] - mf[TSIM_MF_LO]) : R(0);
          else dtu = mf[TSIM_MF_P];
          acc += TU[d * DS + m] * dtu / c.ca;
        }
        if (a.dtab) acc -= TP[d * DS + idamp + lane] * c.qd[lane] / c.ca;
        if constexpr (SRC) acc += a.src[(((size_t)d * a.n + j) * B + env) * nr + lane];      // the body columns' part (k_tangent_body_src)
        TB[d * DS + lane] = acc;
      }
    }
    // ---- dynamics pairs (k_param_grad is the transpose): g_j holds W_j . (inB_j - inA_j) Ww / ca, Ww the pair's wrench in the world frame, so
    //      (dg/dp_k)_j = W_j . (inB_j - inA_j) dWw/dp_k / ca with dWw/dp_k the world form of (sum x x dF/dp_k, sum dF/dp_k) over the contact points
    if (a.dtab) {
      for (int pk = 0; pk < npair; ++pk) {
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
          for (int d = 0; d < ndir; ++d) {
            const R* dp = TP + d * DS + 4 * pk;
            TB[d * DS + lane] -= G[0] * dp[0] + G[1] * dp[1] + G[2] * dp[2] + G[3] * dp[3];
          }
        }
      }
    }
    TS_SYNC();
    // ---- per direction: s = K kv + M mv + TB, H y = s, dq1 = y - kv, dqd1 = cv y.  BDF1: kv = -dq0, mv = h dqd0.  BDF2 (the transpose of the
    //      four-history update of k_backward): kv = -4/3 dq0 + 1/3 dq_1, mv = 8h/9 dqd0 - 2h/9 dqd_1.
    for (int d = 0; d < ndir; ++d) {
      R* T0 = TS + d * DS;
      R kv = R(0);
      if (lane < nr) {
        R mv;
        if (!bdf2) { kv = -T0[lane]; mv = c.h * T0[nr + lane]; }
        else {
          kv = R(-4.0 / 3) * T0[lane] + R(1.0 / 3) * T0[2 * nr + lane];
          mv = R(8.0 / 9) * c.h * T0[nr + lane] - R(2.0 / 9) * c.h * T0[3 * nr + lane];
        }
        c.dq[lane] = kv; c.z[lane] = mv;
      }
      TS_SYNC();
      const R ym = mass_times_z<LPE>(c, lane);
      if (lane < nr) {
        R kq = R(0);
        for (int k = 0; k < nr; ++k) kq += c.H[lane * nr + k] * c.dq[k];
        c.rhs[lane] = kq + ym + TB[d * DS + lane];
      }
      TS_SYNC();
      solve_newton<R, NRM, LPE, double>(H2, c.rhs, c.z, nr, false, lane);
      if (lane < nr) {
        const R y = c.z[lane];
        if (bdf2_model) { T0[2 * nr + lane] = T0[lane]; T0[3 * nr + lane] = T0[nr + lane]; }
        T0[lane] = y - kv; T0[nr + lane] = c.cv * y;
      }
      TS_SYNC();
    }
    if ((j + 1) % a.nsub != 0) continue;
    // ================================================================ a frame ends: its outputs' tangents (the link state of the taped point is still in LDS)
    for (int d = 0; d < ndir; ++d) {
      if (valid && lane < nr) {
        const size_t o = (((size_t)d * T + fr) * B + env) * nr + lane;
        if (a.dq_out) a.dq_out[o] = TS[d * DS + lane];
        if (a.dqd_out) a.dqd_out[o] = TS[d * DS + nr + lane];
      }
    }
    if (a.dvar_out && nvar) {      // lanes = (direction, variable): dvar_e = sum_k (W_k.a x x_e + W_k.l) dq_k over the dofs above the variable's link
      const int ntask = ndir * nvar;
      for (int t0 = 0; t0 < ntask; t0 += LPE) {
        const int task = t0 + lane;
        if (task >= ntask) continue;
        const int d = task / nvar, e = task - d * nvar;
        const int l = c.I[c.off_var + e * TSIM_VI_SIZE + TSIM_VI_LINK];
        const int anc = anc_of(c.I, c.off_link, l);
        const V3<R> x = mulMv(ldm(c.LP + l * LK_SIZE + LK_R), ldv(c.F + c.foff_var + e * TSIM_VF_SIZE)) + ldv(c.LP + l * LK_SIZE + LK_P);
        V3<R> acc = zero3<R>();
        for (int k = 0; k < nr; ++k) {
          if (!((anc >> k) & 1)) continue;
          const S6<R> Wk = ld6(c.WP + k * 6);
          acc = acc + (cross3(Wk.a, x) + Wk.l) * TS[d * DS + k];
        }
        if (valid) {
          R* o = a.dvar_out + (((size_t)d * T + fr) * B + env) * (3 * nvar) + 3 * e;
          o[0] = acc.x; o[1] = acc.y; o[2] = acc.z;
        }
      }
    }
    const int tslot = a.tac_slot ? a.tac_slot[fr] : fr;
    if (!a.dtac_out || !ntac3 || !__any(tslot >= 0)) { TS_SYNC(); continue; }      // (the same frame in every slot of the wavefront: uniform)
    for (int s = 0; s < nsensor; ++s) {
      const int* si = c.I + c.off_sensor + s * TSIM_SI_SIZE;
      const R* sf = c.F + c.foff_sensor + s * TSIM_SF_SIZE;
      const int tx0 = ts_u(si[TSIM_SI_TAX0]), nt = ts_u(si[TSIM_SI_NTAX]), sp0 = ts_u(si[TSIM_SI_SPRIM0]), nsp = ts_u(si[TSIM_SI_NSPRIM]);
      for (int jp = 0; jp < nsp || jp == 0; ++jp) {
        const bool has_prim = jp < nsp;      // a sensor without primitives: its taxels read exact zeros
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
          // lanes = dofs stage the pair's per-dof records, then lanes = (direction, component) form the direction's 12-vector
          // (dth, drho, dw, dv) = sum_k T_k dq_k, and the velocity half once more with dqd (records of mode 1)
          pair_stage_tangent(c, pk, 0, lane, R(1), 0);
          TS_SYNC();
          for (int t0 = 0; t0 < ndir * 12; t0 += LPE) {
            const int task = t0 + lane;
            if (task >= ndir * 12) continue;
            const int d = task / 12, e = task - d * 12;
            R acc = R(0);
            for (int k = 0; k < nr; ++k) acc += c.PT[k * PT_SIZE + e] * TS[d * DS + k];
            TT[d * DS + e] = acc;
          }
          TS_SYNC();
          pair_stage_tangent(c, pk, 0, lane, R(1), 1);
          TS_SYNC();
          for (int t0 = 0; t0 < ndir * 12; t0 += LPE) {
            const int task = t0 + lane;
            if (task >= ndir * 12) continue;
            const int d = task / 12, e = task - d * 12;
            if (e < 6) continue;
            R acc = R(0);
            for (int k = 0; k < nr; ++k) acc += c.PT[k * PT_SIZE + e] * TS[d * DS + nr + k];
            TT[d * DS + e] += acc;
          }
          TS_SYNC();
        }
        // lanes = taxels: the contact law once, every direction from it.  out = A^T R_PA^T F, so
        //   d out = A^T R_PA^T (Jx dx + Jv dxd - dth x F + dF/dp_sensor dp),  dx = dth x x + drho,  dxd = dv + dw x x + wrel x dx
        for (int base = 0; base < nt; base += LPE) {
          if (base + lane >= nt || tslot < 0) continue;
          const int tx = tx0 + base + lane;
          const R* tp = c.Fg + c.foff_tax + tx;
          bool live = false;
          V3<R> xP = zero3<R>(), F = zero3<R>(); M3<R> Jx, Jv; ContactGeo<R> geo;
          if (has_prim) {
            const V3<double> xPd = mulMv(Pp.RPAd, mk3<double>((double)tp[0], (double)tp[c.ntax], (double)tp[2 * c.ntax])) + Pp.pPAd;
            xP = cvt3<R>(xPd);
            live = contact_law<R, true>(prim, shape, sf, xP, Pp.vrel + cross3(Pp.wrel, xP), F, Jx, Jv, xPd, nullptr, true, &geo);
          }
          V3<R> dFp[4];
          if (live && a.dtab) contact_law_dparam(geo, sf, dFp);
          for (int d = 0; d < ndir; ++d) {
            R* o = a.dtac_out + (((size_t)d * nmask + tslot) * B + env) * ntac3 + 3 * tx;
            R o0 = R(0), o1 = R(0), o2 = R(0);
            if (live) {
              const R* tt = TT + d * DS;
              const V3<R> dth = ldv(tt), drho = ldv(tt + 3), dw = ldv(tt + 6), dv = ldv(tt + 9);
              const V3<R> dx = cross3(dth, xP) + drho;
              const V3<R> dxd = dv + cross3(dw, xP) + cross3(Pp.wrel, dx);
              V3<R> dF = mulMv(Jx, dx) + mulMv(Jv, dxd) - cross3(dth, F);
              if (a.dtab) {
                const R* dp = TP + d * DS + 4 * npair + 4 * s;
                dF = dF + dFp[0] * dp[0] + dFp[1] * dp[1] + dFp[2] * dp[2] + dFp[3] * dp[3];
              }
              const V3<R> vl = mulMtv(Pp.RPA, dF);
              o0 = tp[3 * c.ntax] * vl.x + tp[4 * c.ntax] * vl.y + tp[5 * c.ntax] * vl.z;
              o1 = tp[6 * c.ntax] * vl.x + tp[7 * c.ntax] * vl.y + tp[8 * c.ntax] * vl.z;
              o2 = tp[9 * c.ntax] * vl.x + tp[10 * c.ntax] * vl.y + tp[11 * c.ntax] * vl.z;
            }
            // one writer per element: this lane owns taxel tx in every primitive's pass, the first pass stores (an unloaded taxel: exact
            // zeros), a later one adds to its own earlier store
            if (!valid) continue;
            if (jp == 0) { o[0] = o0; o[1] = o1; o[2] = o2; }
            else if (live) { o[0] += o0; o[1] += o1; o[2] += o2; }
          }
        }
      }
    }
    TS_SYNC();
  }
}
