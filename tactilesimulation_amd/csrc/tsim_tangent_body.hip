// tsim_tangent_body.hip — the body-group columns of dtables as directions of the tangent pass (include/tsim.h tsim_tangent_episode with a body group on
// in tsim_set_param_grad_groups; the math: DESIGN.md §4 "Tangent pass").  The body parameters reach the outputs only through the residual, and
//     src_d[t] = -(dg_t / dp_body) dp_d
// depends on the taped state alone, not on the tangents: it is computed for every sub-step at once, before k_tangent walks the tape, which adds it to
// the direction's source of the sub-step (TanArgs::src).
//   k_tangent_src        k_tangent reading src (the one body of both: tsim_tangent_kernel.h)
//   k_tangent_body_src   k_param_grad_body (tsim_param_grad_body.hip) read forwards, on its scaffold (tsim_param_pass.h: a slot is (environment, chunk
//                        of sub-steps), 16 / 32 / 64 lanes as the adjoint launch).  Per sub-step one value-only link sweep of the taped state WITH
//                        its discrete accelerations, shared by all directions; per direction lanes = (link, wrench component) form
//                        dF_i = dI_i A_i + V_i x* dI_i V_i from the direction's ten numbers of the link, then lanes = dofs the sum over the dof's
//                        subtree, the motor terms and the limit terms.  The direction's entries are read from global memory where they are used.
// Every sum has a fixed order — the links ascending, then the motors, then the limit — and there are no atomics: a direction's bits depend neither on
// ndir nor on the other directions, nor on the chunk layout.
// A translation unit of its own, so that no other kernel's code moves.  Built like the generic kernels: no fast-math flags.
#include <hip/hip_runtime.h>
#include "tsim_kernels.h"
#include "tsim_param_pass.h"
#include "tsim_param_body.h"
#include "tsim_tangent.h"
#include "tsim_tangent_kernel.h"
#include "tsim_launch.h"

template <class R, bool EXPJ, int LPE>
__global__ void __launch_bounds__(TS_WAVE) k_tangent_body_src(TanBodyArgs<R> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  R* lds = reinterpret_cast<R*>(smem_raw);
  const int lane = threadIdx.x % LPE, chunk = pg_chunk<LPE>(a), e_ = pg_slot_env<LPE>(a, chunk);      // (the scaffold: tsim_param_pass.h)
  const bool valid = e_ < a.B;
  const int env = min(e_, a.B - 1);
  Ctx<R> c; pg_ctx<LPE>(a, lds, c, lane, env);
  const int nr = c.nr, nu = c.nu, nl = c.nl, REC = ts_rec(nr, nu, (int)sizeof(R), a.tk);
  const int oqd = rec_qd<R>(nr), ou = rec_u<R>(nr);
  // the tangent records are not used by a value-only sweep: the direction's dF_i (6 per link) live there, as k_param_grad_body's Z_i do
  R* dFl = c.DT;
  const int nzt = 6 * nl;
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
      pg_load_taped(c, rec, nr, lane);
      // the sub-step's discrete acceleration, formed as k_param_grad_body forms it (its comment there): in fp32 from the taped double positions, not
      // from the rounded taped velocities k_tangent uses — the two passes are each other's transpose only at the same accelerations
      double qa;
      if constexpr (sizeof(R) == 8) {
        const double v1 = rec[oqd + lane], v0 = rec0[oqd + lane];
        qa = bdf2 ? (3.0 * v1 - 4.0 * v0 + a.tape[((size_t)(t - 2) * a.B + env) * REC + oqd + lane]) / (2.0 * c.h) : (v1 - v0) / c.h;
      } else {
        const double hd = (double)c.h;
        auto pos = [&](int s) { return rec_q(a.tape + ((size_t)s * a.B + env) * REC)[lane]; };
        auto vel = [&](int s) -> double {
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
    }
    for (int d = 0; d < a.ndir; ++d) {
      const R* row = a.dtab + ((size_t)d * a.B + env) * a.fstride;      // the direction's row of the environment
      if (inertial) {
        // ---- g_j contains W_j . sum_{i in subtree(j)} F_i / ca,  F_i = I_i A_i + V_i x* I_i V_i.  Component k of dF_i:
        //      e_k . dI A - (V x e_k) . dI V, the two bilinear forms pgb_dinertia differentiates, summed over the link's ten numbers
        for (int t0 = 0; t0 < nzt; t0 += LPE) {                  // lanes = (link, component of dF)
          const int ti = t0 + lane;
          if (ti < nzt) {
            const int i = ti / 6 + 1, comp = ti - (i - 1) * 6;
            const R* X = c.LP + i * LK_SIZE;
            const M3<R> XR = ldm(X + LK_R);
            const V3<R> cw = ldv(X + LK_C);
            const S6<R> V = ld6(X + LK_W), A = ld6(X + LK_AW);
            const R one = R(1), zero = R(0);
            const S6<R> E = mk6<R>(mk3<R>(comp == 0 ? one : zero, comp == 1 ? one : zero, comp == 2 ? one : zero),
                                   mk3<R>(comp == 3 ? one : zero, comp == 4 ? one : zero, comp == 5 ? one : zero));
            const S6<R> VE = crm(V, E);
            const R m = c.F[c.foff_link + (i - 1) * TSIM_LF_SIZE + TSIM_LF_MASS];
            const R* dp = row + c.foff_link + (i - 1) * TSIM_LF_SIZE + TSIM_LF_MASS;      // mass, com[3], inertia[6]
            R s = R(0);
#pragma unroll
            for (int p = 0; p < 10; ++p) s += (pgb_dinertia(p, m, XR, cw, E, A) - pgb_dinertia(p, m, XR, cw, VE, V)) * dp[p];
            dFl[i * 6 + comp] = s;
          }
        }
        TS_SYNC();
      }
      if (lane < nr) {
        R s = R(0);
        if (inertial) {                                          // the links of the dof's subtree, ascending
          const S6<R> Wj = ld6(c.WP + lane * 6);
          for (int i = 1; i <= nl; ++i)
            if ((anc_of(c.I, c.off_link, i) >> lane) & 1) s -= dot6(Wj, ld6(dFl + i * 6)) / ca;
        }
        // ---- motors (phase3_joint_space): g_j contains -tau / ca; force control tau = lo + (clip(u) + 1) (hi - lo) / 2, position control
        //      tau = P (u - q) - D qd.  The other two columns of a motor give nothing: exactly zero.
        if (motor) {
          for (int m = 0; m < nu; ++m) {
            const int* mi = ts_motor_rec(c, m);
            if (mi[TSIM_MI_DOF] != lane) continue;
            const R* dp = row + c.foff_motor + m * TSIM_MF_SIZE;
            if (mi[TSIM_MI_CTRL] == 0) {
              const R sc = (fmin(fmax(c.u[m], R(-1)), R(1)) + R(1)) * R(0.5);
              s += ((R(1) - sc) * dp[TSIM_MF_LO] + sc * dp[TSIM_MF_HI]) / ca;
            } else s += ((c.u[m] - c.q[lane]) * dp[TSIM_MF_P] - c.qd[lane] * dp[TSIM_MF_D]) / ca;
          }
        }
        // ---- limits: below lo g_j contains -k (lo - q) / ca, above hi +k (q - hi) / ca: the derivative of the piece the state is on
        if (limit) {
          const R* df = c.F + c.foff_dof + lane * TSIM_DF_SIZE;
          const R* dp = row + c.foff_dof + lane * TSIM_DF_SIZE;
          const R k = df[TSIM_DF_LIM_K];
          if (k > R(0)) {
            if (c.q[lane] < df[TSIM_DF_LIM_LO]) s += (k * dp[TSIM_DF_LIM_LO] + (df[TSIM_DF_LIM_LO] - c.q[lane]) * dp[TSIM_DF_LIM_K]) / ca;
            else if (c.q[lane] > df[TSIM_DF_LIM_HI]) s += (k * dp[TSIM_DF_LIM_HI] - (c.q[lane] - df[TSIM_DF_LIM_HI]) * dp[TSIM_DF_LIM_K]) / ca;
          }
        }
        if (valid) a.src[(((size_t)d * a.n + j) * a.B + env) * nr + lane] = s;
      }
      if (inertial) TS_SYNC();                                   // dFl is the next direction's
    }
  }
}

// k_tangent with the switch on (tsim_tangent_kernel.h): where a direction's source of the sub-step is finished, src is added.  Nothing else differs
template <class R, int NRM, bool EXPJ, int LPE>
__global__ void __launch_bounds__(TS_WAVE) k_tangent_src(TanArgs<R> a) { ts_tangent_walk<R, NRM, EXPJ, LPE, true>(a); }

// the launches themselves: tsim_launch.h, as every simulation kernel's (the plans: tsim_hip.hip launch_tangent)
template bool TsLaunch<void, false, float>::run_tangent_src(const TsPlan&, hipStream_t, const TanArgs<float>&);
template bool TsLaunch<void, false, double>::run_tangent_src(const TsPlan&, hipStream_t, const TanArgs<double>&);
template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const TanBodyArgs<float>&);
template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const TanBodyArgs<double>&);
