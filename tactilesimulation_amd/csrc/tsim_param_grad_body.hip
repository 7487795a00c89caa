// tsim_param_grad_body.hip — the body groups of the parameter gradient (include/tsim.h tsim_set_param_grad_groups: link inertia, motors, limits; the
// math: DESIGN.md §4 "Parameter gradient: body groups").  Runs after k_backward_z like the contact pass (tsim_param_grad.hip), only when a body group
// is asked for, on the contact pass's scaffold (tsim_param_pass.h: the slots — (environment, chunk of sub-steps), 16 / 32 / 64 lanes as the adjoint
// launch —, the sub-step header, the taped-state load) and with its reduction (k_param_reduce, tsim_param_grad.hip, given this pass's columns):
//   k_param_grad_body    per sub-step a value-only link sweep of the taped state WITH its discrete accelerations (the contact pass evaluates with
//                        none); lanes = (link, component) form Z_i = sum of z_j W_j over the dofs above link i, lanes = (link, parameter) the ten
//                        derivatives of Z_i . F_i; lanes = motors and lanes = dofs the joint-space terms;
// A translation unit of its own: k_param_grad stays, instruction for instruction, the kernel it was (adding a kernel to its unit moved its fp64
// instantiations by a few hundred code bytes).  Built like the generic kernels: no fast-math flags.
#include <hip/hip_runtime.h>
#include "tsim_kernels.h"
#include "tsim_param_pass.h"
#include "tsim_param_body.h"      // pgb_dinertia: shared with k_tangent_body_src
#include "tsim_launch.h"

template <class R, bool EXPJ, int LPE>
__global__ void __launch_bounds__(TS_WAVE) k_param_grad_body(PgBodyArgs<R> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  R* lds = reinterpret_cast<R*>(smem_raw);
  const int lane = threadIdx.x % LPE, chunk = pg_chunk<LPE>(a), e_ = pg_slot_env<LPE>(a, chunk);      // (the scaffold: tsim_param_pass.h)
  const bool valid = e_ < a.B;
  const int env = min(e_, a.B - 1);
  Ctx<R> c; pg_ctx<LPE>(a, lds, c, lane, env);
  const int nr = c.nr, nu = c.nu, nl = c.nl, REC = ts_rec(nr, nu, (int)sizeof(R), a.tk);
  const int oqd = rec_qd<R>(nr), ou = rec_u<R>(nr);
  // the tangent records are not used by a value-only sweep: Z_i (6 per link) and the links' running sums (10 per link) live there
  // (16 (nl + 1) reals of the (nl + 1) nr DT_SIZE the slot has)
  R* Zl = c.DT;
  R* acc = c.DT + 6 * (nl + 1);
  const int nzt = 6 * nl, nlt = 10 * nl;
  for (int t0 = 0; t0 < nlt; t0 += LPE) if (t0 + lane < nlt) acc[t0 + lane] = R(0);
  R gm[4] = {R(0), R(0), R(0), R(0)};                         // this lane's motor: lo hi P D
  R gl[3] = {R(0), R(0), R(0)};                               // this lane's dof: lim_lo lim_hi lim_k
  const bool inertial = (a.groups & TS_PG_INERTIAL) != 0, motor = (a.groups & TS_PG_MOTOR) != 0, limit = (a.groups & TS_PG_LIMIT) != 0;
  const bool bdf2_model = ts_u(c.I[TSIM_IH_INTEGRATOR]) == 2;
  const int j0 = chunk * a.chunk_len, j1 = min(a.n, j0 + a.chunk_len);
  for (int j = j0; j < j1; ++j) {
    const int t = pg_t(a, j);
    const bool bdf2 = bdf2_model && t >= 2;
    const R ca = pg_ca(c, bdf2);
    const R* rec = pg_rec(a, t, env, REC);
    const R* rec0 = pg_rec(a, t - 1, env, REC);
    TS_SYNC();
    if (lane < nr) {
      pg_load_state(a, c, rec, t, env, nr, lane);
      // the sub-step's discrete acceleration.  fp64: as k_backward forms it, from the taped velocities.  fp32: the taped velocities are rounded to
      // 24 bits and their difference over h is what the inertial derivatives are proportional to (6e-8 |qd| / h of error, 1e-4 of a gentle
      // acceleration), while the taped POSITIONS are double: there the velocities are formed again from them, as the integrator defines them
      double qa;
      if constexpr (sizeof(R) == 8) {
        const double v1 = rec[oqd + lane], v0 = rec0[oqd + lane];
        qa = bdf2 ? (3.0 * v1 - 4.0 * v0 + a.tape[((size_t)(t - 2) * a.B + env) * REC + oqd + lane]) / (2.0 * c.h) : (v1 - v0) / c.h;
      } else {
        const double hd = (double)c.h;
        auto pos = [&](int s) { return rec_q(a.tape + ((size_t)s * a.B + env) * REC)[lane]; };
        auto vel = [&](int s) -> double {      // velocity of taped state s: the reset's own (s = 0), else the integrator's difference of positions
          if (s == 0) return (double)a.tape[((size_t)env) * REC + oqd + lane];
          if (bdf2_model && s >= 2) return (3.0 * pos(s) - 4.0 * pos(s - 1) + pos(s - 2)) / (2.0 * hd);
          return (pos(s) - pos(s - 1)) / hd;
        };
        qa = bdf2 ? (3.0 * vel(t) - 4.0 * vel(t - 1) + vel(t - 2)) / (2.0 * hd) : (vel(t) - vel(t - 1)) / hd;
      }
      c.qa[lane] = (R)qa;
    }
    if (lane < nu) c.u[lane] = rec[ou + lane];
    TS_SYNC();
    if (inertial) {
      phase1<R, false, EXPJ>(c, lane, R(0), R(0), R(0));       // link poses, twists V, accelerations A (gravity: the world's), joint columns W
      TS_SYNC();
      // ---- g_j contains W_j . sum_{i in subtree(j)} F_i / ca,  F_i = I_i A_i + V_i x* I_i V_i.  So -z^T dg/dp = -(Z_i . dF_i/dp) / ca with
      //      Z_i = sum_{j above i} z_j W_j, and  Z . F = Z . I A - (V x Z) . I V  is two of the bilinear forms pgb_dinertia differentiates.
      for (int t0 = 0; t0 < nzt; t0 += LPE) {                  // lanes = (link, component of Z)
        const int ti = t0 + lane;
        if (ti < nzt) {
          const int i = ti / 6 + 1, comp = ti - (i - 1) * 6;
          const int anc = anc_of(c.I, c.off_link, i);
          R s = R(0);
          for (int d = 0; d < nr; ++d) if ((anc >> d) & 1) s += c.z[d] * c.WP[d * 6 + comp];
          Zl[i * 6 + comp] = s;
        }
      }
      TS_SYNC();
      for (int t0 = 0; t0 < nlt; t0 += LPE) {                  // lanes = (link, parameter)
        const int ti = t0 + lane;
        if (ti < nlt) {
          const int i = ti / 10 + 1, p = ti - (i - 1) * 10;
          const R* X = c.LP + i * LK_SIZE;
          const M3<R> XR = ldm(X + LK_R);
          const V3<R> cw = ldv(X + LK_C);
          const S6<R> V = ld6(X + LK_W), A = ld6(X + LK_AW), Z = ld6(Zl + i * 6);
          const R m = c.F[c.foff_link + (i - 1) * TSIM_LF_SIZE + TSIM_LF_MASS];
          const R d = pgb_dinertia(p, m, XR, cw, Z, A) - pgb_dinertia(p, m, XR, cw, crm(V, Z), V);
          acc[ti] -= d / ca;
        }
      }
    }
    // ---- motors (phase3_joint_space): g_j contains -tau / ca; force control tau = lo + (clip(u) + 1) (hi - lo) / 2, position control
    //      tau = P (u - q) - D qd.  The other two columns of a motor get nothing: exactly zero.
    if (motor && lane < nu) {
      const int* mi = ts_motor_rec(c, lane);
      const int dj = mi[TSIM_MI_DOF];
      const R zc = c.z[dj] / ca;
      if (mi[TSIM_MI_CTRL] == 0) {
        const R s = (fmin(fmax(c.u[lane], R(-1)), R(1)) + R(1)) * R(0.5);
        gm[0] += zc * (R(1) - s); gm[1] += zc * s;
      } else { gm[2] += zc * (c.u[lane] - c.q[dj]); gm[3] -= zc * c.qd[dj]; }
    }
    // ---- limits: below lo g_j contains -k (lo - q) / ca, above hi +k (q - hi) / ca: the derivative of the piece the state is on
    if (limit && lane < nr) {
      const R* df = c.F + c.foff_dof + lane * TSIM_DF_SIZE;
      const R k = df[TSIM_DF_LIM_K], zc = c.z[lane] / ca;
      if (k > R(0)) {
        if (c.q[lane] < df[TSIM_DF_LIM_LO]) { gl[0] += zc * k; gl[2] += zc * (df[TSIM_DF_LIM_LO] - c.q[lane]); }
        else if (c.q[lane] > df[TSIM_DF_LIM_HI]) { gl[1] += zc * k; gl[2] -= zc * (c.q[lane] - df[TSIM_DF_LIM_HI]); }
      }
    }
  }
  TS_SYNC();
  R* out = pg_row(a, chunk, env);
  if (valid) {
    for (int t0 = 0; t0 < nlt; t0 += LPE) if (t0 + lane < nlt) out[t0 + lane] = acc[t0 + lane];
    if (lane < nu) {
#pragma unroll
      for (int k = 0; k < 4; ++k) out[nlt + 4 * lane + k] = gm[k];
    }
    if (lane < nr) {
#pragma unroll
      for (int k = 0; k < 3; ++k) out[nlt + 4 * nu + 3 * lane + k] = gl[k];
    }
  }
}

// the launch itself: tsim_launch.h, as every simulation kernel's (the plan: tsim_hip.hip launch_param_pass)
template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const PgBodyArgs<float>&);
template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const PgBodyArgs<double>&);
