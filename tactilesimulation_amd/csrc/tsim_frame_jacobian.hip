// tsim_frame_jacobian.hip — the per-frame transition Jacobians of a taped episode in one launch (include/tsim.h tsim_frame_jacobians; the math and
// the LDS layout: tsim_frame_jacobian.h, DESIGN.md §4 "Frame Jacobians").
//   k_frame_jacobian   slot = (environment, frame) on the parameter passes' scaffold (tsim_param_pass.h, chunk = frame), 16 / 32 / 64 lanes per
//                      environment; every slot of a wavefront walks the same frame.  Per sub-step the taped point is evaluated once, as k_tangent
//                      evaluates it (K = dg/dq in c.H, seeds (1, 0, 0)), the mass matrix is formed once (nr products with unit vectors), and the
//                      2 nr + nu columns' sources s = -K dq0 + h M dqd0 + D du are solved TS_FJ_RHS at a time: one elimination of the taped Newton
//                      matrix per pass (solve_lanes_many, tsim_eval.h), ceil(ncol / 8) per sub-step instead of ncol.
// It reads the tape and writes the caller's buffers, nothing else.  BDF1 models only (the host refuses a BDF2 model).
// Built like the generic kernels: no fast-math flags.  A unit of its own, so that no other kernel's code moves.
#include <hip/hip_runtime.h>
#include "tsim_kernels.h"
#include "tsim_param_pass.h"
#include "tsim_frame_jacobian.h"
#include "tsim_launch.h"

template <class R, int NRM, bool EXPJ, int LPE>
__global__ void __launch_bounds__(TS_WAVE) k_frame_jacobian(FjArgs<R> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  R* lds = reinterpret_cast<R*>(smem_raw);
  const int slot = threadIdx.x / LPE, lane = threadIdx.x % LPE, frame = pg_chunk<LPE>(a), e_ = pg_slot_env<LPE>(a, frame);      // (the scaffold: tsim_param_pass.h)
  const bool valid = e_ < a.B;
  const int env = min(e_, a.B - 1);
  Ctx<R> c; pg_ctx<LPE>(a, lds, c, lane, env);
  c.cull = a.cull;
  const int nr = c.nr, nu = c.nu, nvar = c.nvar, REC = ts_rec(nr, nu, (int)sizeof(R), a.tk);
  const int oqd = rec_qd<R>(nr), oH = rec_H<R>(nr), ou = rec_u<R>(nr);
  const int XS = 2 * nr, ncol = ts_fj_ncol(nr, nu);
  // the slot's block (tsim_frame_jacobian.h): column d at X + d * XS
  R* X = lds + a.xoff + slot * ts_fj_slot_reals(nr, nu);
  R* MM = X + ncol * XS;
  R* W = MM + nr * nr;
  R* DU = W + TS_FJ_RHS * nr;
  const bool solve = a.A_out || a.B_out;
  for (int i = lane; i < ncol * XS; i += LPE) X[i] = (i / XS == i % XS) ? R(1) : R(0);      // identity on the state columns, zero on the du columns
  const int j1 = (frame + 1) * a.chunk_len;
  // without A and B nothing is solved: only the frame's last taped point is evaluated, for Jvar
  for (int j = solve ? frame * a.chunk_len : j1 - 1; j < j1; ++j) {
    const int t = pg_t(a, j);
    const R* rec = pg_rec(a, t, env, REC);
    const R* rec0 = pg_rec(a, t - 1, env, REC);
    TS_SYNC();
    if (lane < nr) {      // the taped point, as k_tangent loads it
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
    // ---- the mass matrix, column by column (symmetric: stored as rows), and D: dtu / ca per motor (k_tangent's motor term for a unit du)
    for (int k = 0; k < nr; ++k) {
      if (lane < nr) c.z[lane] = lane == k ? R(1) : R(0);
      TS_SYNC();
      const R mk = mass_times_z<LPE>(c, lane);
      if (lane < nr) MM[lane * nr + k] = mk;
    }
    if (lane < nu) {
      const int* mi = ts_motor_rec(c, lane);
      const R* mf = c.F + c.foff_motor + lane * TSIM_MF_SIZE;
      R dtu;
      if (mi[TSIM_MI_CTRL] == 0) dtu = (c.u[lane] >= R(-1) && c.u[lane] <= R(1)) ? R(0.5) * (mf[TSIM_MF_HI] - mf[TSIM_MF_LO]) : R(0);
      else dtu = mf[TSIM_MF_P];
      DU[lane] = dtu / c.ca;
    }
    TS_SYNC();
    // ---- TS_FJ_RHS columns per pass: s = -K dq0 + h M dqd0 + D du, H y = s for all of them at once, dq1 = dq0 + y, dqd1 = cv y
    for (int c0 = 0; c0 < ncol; c0 += TS_FJ_RHS) {
      const int nb = min((int)TS_FJ_RHS, ncol - c0);
      if (lane < nr) {
        for (int k = 0; k < nb; ++k) {
          const R* x = X + (c0 + k) * XS;
          R kq = R(0), ym = R(0);
          for (int i = 0; i < nr; ++i) { kq -= c.H[lane * nr + i] * x[i]; ym += MM[lane * nr + i] * (c.h * x[nr + i]); }
          const int m = c0 + k - XS;
          R tb = R(0);
          if (m >= 0 && ts_motor_rec(c, m)[TSIM_MI_DOF] == lane) tb = DU[m];
          W[k * nr + lane] = kq + ym + tb;
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
  // ================================================================ the frame's end: row-major matrices (rows: the state at the end)
  const size_t fe = (size_t)frame * a.B + env;
  if (valid && a.A_out) {
    R* o = a.A_out + fe * XS * XS;
    for (int e = lane; e < XS * XS; e += LPE) { const int i = e / XS, d = e - i * XS; o[e] = X[d * XS + i]; }
  }
  if (valid && a.B_out) {
    R* o = a.B_out + fe * XS * nu;
    for (int e = lane; e < XS * nu; e += LPE) { const int i = e / nu, m = e - i * nu; o[e] = X[(XS + m) * XS + i]; }
  }
  if (a.Jvar_out && nvar) {      // lanes = (variable, dof): k_tangent's dvar_e = sum_k (W_k.a x x_e + W_k.l) dq_k, per dof above the variable's link
    for (int t0 = 0; t0 < nvar * nr; t0 += LPE) {
      const int task = t0 + lane;
      if (task >= nvar * nr) continue;
      const int e = task / nr, k = task - e * nr;
      const int l = c.I[c.off_var + e * TSIM_VI_SIZE + TSIM_VI_LINK];
      V3<R> v = zero3<R>();
      if ((anc_of(c.I, c.off_link, l) >> k) & 1) {
        const V3<R> x = mulMv(ldm(c.LP + l * LK_SIZE + LK_R), ldv(c.F + c.foff_var + e * TSIM_VF_SIZE)) + ldv(c.LP + l * LK_SIZE + LK_P);
        const S6<R> Wk = ld6(c.WP + k * 6);
        v = cross3(Wk.a, x) + Wk.l;
      }
      if (valid) {
        R* o = a.Jvar_out + (fe * 3 * nvar + 3 * e) * nr + k;
        o[0] = v.x; o[nr] = v.y; o[2 * nr] = v.z;
      }
    }
  }
}

// the launch itself: tsim_launch.h, as every simulation kernel's (the plan: tsim_hip.hip ts_plan)
template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const FjArgs<float>&);
template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const FjArgs<double>&);
