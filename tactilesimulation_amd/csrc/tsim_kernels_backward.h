// tsim_kernels_backward.h — the BODY of the adjoint kernel, included textually by k_backward, by its SAVEZ twin k_backward_z and by the closed loop's
// SAVEZ twin k_closed_backward_z (POLICY fixed to true) (tsim_kernels.h), which differ only in `SAVEZ` (a constexpr bool) and `zsave`.  Textual inclusion rather than a shared device function: k_backward must stay the
// kernel it was, code bytes and registers (a body behind a function call boundary, even inlined, schedules differently; host/buildhash.py's
// kernel table shows it).  Not a header of its own: it has no meaning outside those function bodies.
// `PRE` (a constexpr bool like SAVEZ, with `sseed`): on in k_backward_pre alone (tsim_adjoint_pre.h), the twin a fused episode launch runs behind
// k_adjoint_seeds: a seeded sub-step adds the two vectors that pass wrote for its frame instead of running ts_static_output_vjp in the chain.
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  R* lds = reinterpret_cast<R*>(smem_raw);
  constexpr int NS = TS_WAVE / LPE;
  const int slot = threadIdx.x / LPE, lane = threadIdx.x % LPE;
  const bool valid = (int)blockIdx.x * NS + slot < a.B;
  const int env = min((int)blockIdx.x * NS + slot, a.B - 1);
  // (the context's sizes stay run-time values HERE: with them folded the adjoint kernel is 10 % shorter and 18 % SLOWER — 0.82 -> 0.96 ms per 20-step
  // launch, round 6; the forward kernel gains 5 % from the same fold)
  Ctx<R> c; ctx_init<R, MS>(c, a.I, a.F, lds, NS, slot, lane, LPE, a.stage_cpt != 0, a.Fenv ? a.Fenv + (size_t)env * a.fstride : nullptr);
  c.cull = a.cull;
  const int nr = c.nr, nu = c.nu, REC = ts_rec(nr, nu, (int)sizeof(R), a.tk);
  const int nvar3 = 3 * c.nvar, ntac3 = 3 * c.ntax;
  R* H2 = c.H2;    // taped Newton matrix of the sub-step
  init_world(c, lane, LPE);
  if (a.cyc && blockIdx.x == 0) c.stamps = a.cyc;
  if (lane < nr) { c.lamq[lane] = a.lamq[(size_t)env * nr + lane]; c.lamv[lane] = a.lamv[(size_t)env * nr + lane]; }
  // BDF2 models: taped sub-step t >= 2 is a BDF2 step (the first one after a reset is the BDF1 start-up, k_forward).  Its new state
  // depends on the TWO states before it, so next to the adjoint of the state one step back (lamq, lamv) the kernel carries what later
  // sub-steps already contributed to the state two steps back (lq1, lv1: one value per lane, in registers; second half of the buffers).
  const bool bdf2_model = ts_integrator<MS>(c) == 2;      // (a compile-time constant for a compiled-in model: its BDF2 branches fold away)
  const size_t half = (size_t)a.B * nr;
  R lq1 = R(0), lv1 = R(0);
  if (bdf2_model && lane < nr) { lq1 = a.lamq[half + (size_t)env * nr + lane]; lv1 = a.lamv[half + (size_t)env * nr + lane]; }
  TS_SYNC();
  R du_frame = R(0);
  R pol_dq = R(0); bool pol_have = false;      // POLICY: what the NEXT frame's observation put on this frame's final state (q[0..2]; tactile: pol.dobs_tac)
  // A statically known model (tsim_static_eval.h): no evaluation at all — the tape holds, next to H, the position partial K of the same
  // iterate (k_forward), so y_q = K^T z is a product and M z a value-only link sweep (the evaluation of the taped point with tangents, pairs
  // and point loops it replaces cost as much as a forward evaluation round).  Only a sub-step that carries a loss seed needs the link
  // states with tangents (ts_static_output_vjp runs its own sweep).
  constexpr bool kFused = ts_static_fused<MS, R>();
  // The tape record of sub-step t (q1, qd1, u, H, K) and the state before it (q, qd of record t - 1) are fetched ONE ITERATION AHEAD
  // into registers: a lone wavefront cannot hide the ~2 x 1.5 k cycles of HBM latency of dependent loads at the top of every
  // sub-step, but the loads for the next sub-step fly during the whole of this one.  (Record t - 1 supplies q0, qd0 now and
  // q1, qd1 of the next iteration, so each iteration fetches u, H, K of record t - 1 and q, qd of record t - 2.)
  constexpr int NHL = (NRM * NRM + LPE - 1) / LPE;
  const int oqd = rec_qd<R>(nr), oH = rec_H<R>(nr), ou = rec_u<R>(nr), oK = rec_K<R>(nr, nu);
  double pq1 = 0.0, pq0 = 0.0; R pqd1 = R(0), pqd0 = R(0), pqdm = R(0), pu = R(0), pH[NHL];     // pqdm: qd two records back (BDF2)
  R pK[kFused ? NHL : 1];
  R* KT = c.H;      // the fused path's taped K of the sub-step (c.H is not used otherwise there)
  {
    const R* r1 = a.tape + ((size_t)a.t_end * a.B + env) * REC;
    const R* r0 = a.tape + ((size_t)(a.t_end - 1) * a.B + env) * REC;
    if (lane < nr) { pq1 = rec_q(r1)[lane]; pqd1 = r1[oqd + lane]; pq0 = rec_q(r0)[lane]; pqd0 = r0[oqd + lane]; }
    if (bdf2_model && a.t_end >= 2 && lane < nr) pqdm = a.tape[((size_t)(a.t_end - 2) * a.B + env) * REC + oqd + lane];
    if (lane < nu) pu = r1[ou + lane];
#pragma unroll
    for (int i = 0; i < NHL; ++i) { const int e = lane + i * LPE; pH[i] = e < nr * nr ? r1[oH + e] : R(0); }
    if constexpr (kFused) {
#pragma unroll
      for (int i = 0; i < NHL; ++i) { const int e = lane + i * LPE; pK[i] = (a.tk && e < nr * nr) ? r1[oK + e] : R(0); }
    }
  }
  // PRE: the seed partials of a frame, sseed[frame][env][sq (nr) | sv (nr)] (k_adjoint_seeds), fetched one iteration ahead like the record
  [[maybe_unused]] R psq = R(0), psv = R(0);
  if constexpr (PRE) {
    if (a.n % a.seed_stride == 0 && lane < nr) {      // sub-step n - 1 ends a frame
      const R* sp = sseed + ((size_t)((a.n - 1) / a.seed_stride) * a.B + env) * (2 * nr);
      psq = sp[lane]; psv = sp[nr + lane];
    }
  }
  for (int j = a.n - 1; j >= 0; --j) {
    const int t = a.t_end - (a.n - 1 - j);
    const bool bdf2 = bdf2_model && t >= 2;
    c.cv = bdf2 ? R(1.5) / c.h : R(1) / c.h;
    c.ca = bdf2 ? R(2.25) / (c.h * c.h) : R(1) / (c.h * c.h);
    if (lane < nr) {
      c.qD[lane] = pq1; c.q[lane] = (R)pq1; c.q0[lane] = (R)pq0; c.qd0[lane] = pqd0;
      c.qd[lane] = pqd1;                              // taped velocity of the new state
      // discrete acceleration from the taped velocities, no position cancellation: BDF1 (qd1 - qd0) / h, BDF2 (3 qd1 - 4 qd0 + qd_1) / 2h
      c.qa[lane] = bdf2 ? (R(3) * pqd1 - R(4) * pqd0 + pqdm) / (R(2) * c.h) : (pqd1 - pqd0) / c.h;
    }
    if (lane < nu) c.u[lane] = pu;
#pragma unroll
    for (int i = 0; i < NHL; ++i) { const int e = lane + i * LPE; if (e < nr * nr) H2[e] = pH[i]; }
    if constexpr (kFused) {
#pragma unroll
      for (int i = 0; i < NHL; ++i) { const int e = lane + i * LPE; if (e < nr * nr) KT[e] = pK[i]; }
    }
    TS_STAMP(c);
    [[maybe_unused]] const R sq_now = psq, sv_now = psv;
    if constexpr (PRE) {
      if (j > 0 && j % a.seed_stride == 0 && lane < nr) {      // the next iteration's sub-step j - 1 ends a frame
        const R* sp = sseed + ((size_t)((j - 1) / a.seed_stride) * a.B + env) * (2 * nr);
        psq = sp[lane]; psv = sp[nr + lane];
      }
    }
    if (j > 0) {                                      // next iteration: sub-step t - 1
      const R* r1 = a.tape + ((size_t)(t - 1) * a.B + env) * REC;
      const R* r0 = a.tape + ((size_t)(t - 2) * a.B + env) * REC;
      pq1 = pq0; pqd1 = pqd0;
      if (lane < nr) { pq0 = rec_q(r0)[lane]; pqd0 = r0[oqd + lane]; }
      if (bdf2_model && t >= 3 && lane < nr) pqdm = a.tape[((size_t)(t - 3) * a.B + env) * REC + oqd + lane];
      if (lane < nu) pu = r1[ou + lane];
#pragma unroll
      for (int i = 0; i < NHL; ++i) { const int e = lane + i * LPE; pH[i] = e < nr * nr ? r1[oH + e] : R(0); }
      if constexpr (kFused) {
#pragma unroll
        for (int i = 0; i < NHL; ++i) { const int e = lane + i * LPE; pK[i] = (a.tk && e < nr * nr) ? r1[oK + e] : R(0); }
      }
    }
    // (the loads above must be ISSUED here, a whole sub-step ahead of their use: with the model's sizes as compile-time constants the scheduler
    // otherwise sinks them to the top of the next iteration and a lone wavefront waits ~2 us of HBM latency per sub-step — measured in round 6:
    // k_backward 0.82 -> 0.96 ms per 20-step launch with 10 % FEWER instructions)
    __builtin_amdgcn_sched_barrier(0);
    TS_SYNC();
    TS_STAMP(c);
    const bool seeded = (j + 1) % a.seed_stride == 0;
    if constexpr (kFused) { }      // (a seeded sub-step runs its own link sweep inside ts_static_output_vjp)
    else if constexpr (std::is_void<MS>::value) phase1<R, true, EXPJ>(c, lane, R(1), R(0), R(0));
    else phase1_static_levels<R, MS, true>(c, lane, R(1), R(0), R(0));
    TS_STAMP(c);
    // direct partials of the loss w.r.t. this sub-step's outputs
    if (seeded) {
      const int fr = j / a.seed_stride;
      const size_t so = a.frames ? (size_t)fr * a.B + env : (size_t)env * (a.n / a.seed_stride) + fr;
      const int tslot = (a.frames && a.tac_slot) ? a.tac_slot[fr] : 0;
      const size_t sot = (a.frames && a.tac_slot) ? (size_t)max(tslot, 0) * a.B + env : so;
      if (a.df_dq && lane < nr) c.lamq[lane] += a.df_dq[so * nr + lane];
      if (POLICY && pol_have && lane < nr) c.lamq[lane] += pol_dq;       // state part of the next frame's observation (goal; privilege: box pose)
      TS_SYNC();
      const R* wtac_ = (a.df_dtac && ntac3 && tslot >= 0) ? a.df_dtac + sot * ntac3 : nullptr;
      if (POLICY) wtac_ = (pol_have && a.pol.mode == TSIM_PUSH_OBS_TACTILE) ? a.pol.dobs_tac + ((size_t)(fr + 1) * a.B + env) * PP_NTAC : nullptr;   // tactile part (frame fr + 1's observation)
      if constexpr (PRE) { if (lane < nr) { c.lamq[lane] += sq_now; c.lamv[lane] += sv_now; } TS_SYNC(); }
      else if constexpr (kFused) ts_static_output_vjp<R, LPE, MS>(c, lane, (a.df_dvar && nvar3) ? a.df_dvar + so * nvar3 : nullptr, wtac_);
      else output_vjp<LPE>(c, lane, (a.df_dvar && nvar3) ? a.df_dvar + so * nvar3 : nullptr, wtac_);
    }
    TS_STAMP(c);
#ifdef TS_BWD_REEVAL      // A/B builds only (profiles/r06_tape_ab.md): what a tape WITHOUT the Newton matrix would cost — the matrix of the taped point is evaluated
                          // again here (the forward kernel's evaluation with tangents) and the adjoint solve uses it instead of the taped one
    if (lane < nr) {
      c.qp[lane] = c.q0[lane] + c.h * c.qd0[lane]; c.qdp[lane] = c.qd0[lane];
      c.dl[lane] = (R)(c.qD[lane] - (double)c.qp[lane]); c.qpD[lane] = c.qD[lane] - (double)c.dl[lane];
    }
    TS_SYNC();
    evaluate<R, NRM, EXPJ, LPE, MS>(c, lane, R(1), c.cv, c.ca, true);
    for (int e = lane; e < nr * nr; e += LPE) {
      const R h_ = c.H[e];
      if constexpr (kFused) KT[e] = H2[e];      // the fused evaluation leaves K in c.H2
      H2[e] = h_;
    }
    TS_SYNC();
#endif
    if (lane < nr) c.rhs[lane] = c.lamq[lane] + c.cv * c.lamv[lane];      // d qd1 / d q1 = cv
    TS_SYNC();
    solve_newton<R, NRM, LPE, double, ts_static_nr<MS>()>(H2, c.rhs, c.z, nr, true, lane);
    TS_STAMP(c);
    R ym, yq = R(0);
    if constexpr (!kFused) {
      phase2<R, NRM, LPE, MS>(c, lane, R(1));
      TS_STAMP(c);
      phase3<R, EXPJ, LPE>(c, lane, R(1), R(0));       // c.H = h^2 dr/dq
      TS_STAMP(c);
      ym = mass_times_z<LPE>(c, lane);
      if (lane < nr) for (int i = 0; i < nr; ++i) yq += c.z[i] * c.H[i * nr + lane];
    } else {
      TS_STAMP(c);
      ym = ts_static_mass_times_z<R, MS>(c, lane);      // (its barriers also order the solve's z before the product below)
      constexpr int NRS = ts_static_nr<MS>();
      if (lane < NRS) {
#pragma unroll
        for (int i = 0; i < NRS; ++i) yq += c.z[i] * KT[i * NRS + lane];
      }
      TS_STAMP(c);
    }
    TS_STAMP(c);
    if constexpr (SAVEZ) { if (valid && lane < nr) zsave[((size_t)(t - 1) * a.B + env) * nr + lane] = c.z[lane]; }
    if (lane < nr) {
      if (!bdf2) {                                    // BDF1: new state from (q0, qd0) only
        c.lamq[lane] = c.lamq[lane] - yq + lq1;       // lq1, lv1: what a later BDF2 step put on this sub-step's (q0, qd0) as ITS (q_1, qd_1)
        c.lamv[lane] = c.h * ym + lv1;
        lq1 = R(0); lv1 = R(0);
      } else {
        // BDF2 in predictor form: with a_w = d qd1 / d p_w and dqp_w = d qpred / d p_w for p = (q0, qd0, q_1, qd_1),
        //   -(dg/dp_w)^T z + a_w lam_v = a_w (lam_v - R_v^T z / ca) + dqp_w M z ,   R_v^T z / ca = (rhs - K^T z - M z) / cv
        // (H = K + (cv R_v + ca M) / ca; rhs = H^T z).  a = (-2/h, 0, 1/2h, 0), dqp = (4/3, 8h/9, -1/3, -2h/9).
        const R d = c.lamv[lane] - (c.rhs[lane] - yq - ym) / c.cv;
        const R o0 = R(-2) / c.h * d + R(4.0 / 3) * ym, o1 = R(8.0 / 9) * c.h * ym;
        const R o2 = R(0.5) / c.h * d - R(1.0 / 3) * ym, o3 = R(-2.0 / 9) * c.h * ym;
        c.lamq[lane] = o0 + lq1; c.lamv[lane] = o1 + lv1;
        lq1 = o2; lv1 = o3;
      }
    }
    if (lane < nu) {
      const int* mi = ts_motor_rec(c, lane);
      const R* mf = c.F + c.foff_motor + lane * TSIM_MF_SIZE;
      R dtu;
      if (mi[TSIM_MI_CTRL] == 0) dtu = (c.u[lane] >= R(-1) && c.u[lane] <= R(1)) ? R(0.5) * (mf[TSIM_MF_HI] - mf[TSIM_MF_LO]) : R(0);
      else dtu = mf[TSIM_MF_P];
      const R du = c.z[mi[TSIM_MI_DOF]] * dtu / c.ca;         // -(dg/du)^T z, g = r / ca
      if (!a.frames) { if (valid) a.df_du[((size_t)env * a.n + j) * nu + lane] = du; }
      else {
        du_frame += du;
        if (j % a.seed_stride == 0 && valid && a.df_du) a.df_du[((size_t)(j / a.seed_stride) * a.B + env) * nu + lane] = du_frame;
      }
    }
    if (a.frames && j % a.seed_stride == 0) {              // a frame is undone
      if (POLICY) {
        // ... and so is the policy call in front of it: dL/d(action) -> MLP -> observation -> the state / tactile frame before it
        TS_SYNC();
        const int fr0 = j / a.seed_stride;
        pol_dq = push_policy_backward<LPE>(c, lane, valid, a.pol, (size_t)fr0 * a.B + env, env, du_frame, c.q0);
        pol_have = true;
        ts_own_stores_visible();                           // dobs_tac is read back by this slot as the previous frame's tactile seed
      }
      du_frame = R(0);
    }
    TS_SYNC();
  }
  if (lane < nr && valid) {
    a.lamq[(size_t)env * nr + lane] = c.lamq[lane]; a.lamv[(size_t)env * nr + lane] = c.lamv[lane];
    if (bdf2_model) { a.lamq[half + (size_t)env * nr + lane] = lq1; a.lamv[half + (size_t)env * nr + lane] = lv1; }
  }
