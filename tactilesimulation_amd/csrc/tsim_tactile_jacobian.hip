// tsim_tactile_jacobian.hip — the per-frame tactile Jacobians of a taped episode in one launch (include/tsim.h tsim_tactile_jacobians; the math and
// the LDS layout: tsim_tactile_jacobian.h, DESIGN.md §4 "Tactile Jacobians").
//   k_tactile_jacobian   slot = (environment, frame) on the parameter passes' scaffold (tsim_param_pass.h, chunk = frame), 16 / 32 / 64 lanes per
//                        environment; every slot of a wavefront is on the same frame, and a block whose frame is not masked returns at once.  The
//                        frame's LAST taped point is evaluated as k_frame_jacobian's Jvar-only path evaluates it (phase 1 alone, seeds (1, 0, 0):
//                        link states and their tangents); then, per sensor and paired primitive in the order of k_tangent's tactile section
//                        (tsim_tangent_kernel.h), the pair's per-dof records are staged in both modes and kept behind the contexts, and lanes =
//                        taxels evaluate the contact law once and emit all 2 nr columns from it.
// It reads the tape and writes the caller's buffer, nothing else.  NRM does not enter the code (nothing is solved): it is a template parameter so
// that the launch plan names this kernel's instantiations as it names every other's.
// Built like the generic kernels: no fast-math flags.  A unit of its own, so that no other kernel's code moves.
#include <hip/hip_runtime.h>
#include "tsim_kernels.h"
#include "tsim_param_pass.h"
#include "tsim_tactile_jacobian.h"
#include "tsim_launch.h"

template <class R, int NRM, bool EXPJ, int LPE>
__global__ void __launch_bounds__(TS_WAVE) k_tactile_jacobian(TjArgs<R> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  R* lds = reinterpret_cast<R*>(smem_raw);
  const int slot = threadIdx.x / LPE, lane = threadIdx.x % LPE, frame = pg_chunk<LPE>(a);      // (the scaffold: tsim_param_pass.h)
  const int tslot = a.tac_slot ? a.tac_slot[frame] : frame;
  if (tslot < 0) return;      // not masked: the whole block (every slot is on this frame) leaves before it loads anything
  const int e_ = pg_slot_env<LPE>(a, frame);
  const bool valid = e_ < a.B;
  const int env = min(e_, a.B - 1);
  Ctx<R> c; pg_ctx<LPE>(a, lds, c, lane, env);
  c.cull = a.cull;
  const int nr = c.nr, nu = c.nu, ntax = c.ntax, nsensor = c.nsensor, REC = ts_rec(nr, nu, (int)sizeof(R), a.tk);
  const int XS = 2 * nr;
  const size_t ntac3 = (size_t)3 * ntax;
  // the slot's block (tsim_tactile_jacobian.h)
  R* Q0 = lds + a.xoff + slot * ts_tj_slot_reals(nr);
  R* Q1 = Q0 + 12 * nr;
  // the frame's last taped point: only its (q, qd) is read (the acceleration enters no pose and no velocity)
  const R* rec = pg_rec(a, pg_t(a, (frame + 1) * a.chunk_len - 1), env, REC);
  if (lane < nr) { pg_load_taped(c, rec, nr, lane); c.qa[lane] = R(0); }
  TS_SYNC();
  phase1<R, true, EXPJ>(c, lane, R(1), R(0), R(0));
  R* out = a.Ct_out + ((size_t)tslot * a.B + env) * XS * ntac3;      // column d at out + d * ntac3: one tactile frame
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
        // lanes = dofs stage the pair's per-dof records; the directions are unit vectors, so a record IS its column's 12-vector
        pair_stage_tangent(c, pk, 0, lane, R(1), 0);
        TS_SYNC();
        for (int i = lane; i < 12 * nr; i += LPE) Q0[i] = c.PT[(i / 12) * PT_SIZE + i % 12];
        TS_SYNC();
        pair_stage_tangent(c, pk, 0, lane, R(1), 1);
        TS_SYNC();
        for (int i = lane; i < 6 * nr; i += LPE) Q1[i] = c.PT[(i / 6) * PT_SIZE + PT_DW + i % 6];
        TS_SYNC();
      }
      // lanes = taxels: the contact law once, every column from it.  out = A^T R_PA^T F, so
      //   d out = A^T R_PA^T (Jx dx + Jv dxd - dth x F),  dx = dth x x + drho,  dxd = dv + dw x x + wrel x dx
      for (int base = 0; base < nt; base += LPE) {
        if (base + lane >= nt) continue;
        const int tx = tx0 + base + lane;
        const R* tp = c.Fg + c.foff_tax + tx;
        bool live = false;
        V3<R> xP = zero3<R>(), F = zero3<R>(); M3<R> Jx, Jv;
        if (has_prim) {
          const V3<double> xPd = mulMv(Pp.RPAd, mk3<double>((double)tp[0], (double)tp[ntax], (double)tp[2 * ntax])) + Pp.pPAd;
          xP = cvt3<R>(xPd);
          live = contact_law<R, true>(prim, shape, sf, xP, Pp.vrel + cross3(Pp.wrel, xP), F, Jx, Jv, xPd, nullptr, true);
        }
        // one writer per element: this lane owns taxel tx in every primitive's pass, the first pass stores (an unloaded taxel: exact zeros), a
        // later one adds to its own earlier store
        if (!valid || (jp > 0 && !live)) continue;
        R* o = out + (size_t)3 * tx;
        if (!live) {
          for (int d = 0; d < XS; ++d) { R* od = o + d * ntac3; od[0] = R(0); od[1] = R(0); od[2] = R(0); }
          continue;
        }
        // the taxel's frame A (rows) times R_PA^T, once for all columns
        M3<R> AR;
        {
          const M3<R> Rt = Pp.RPA;
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const R ax = tp[(3 + 3 * r) * ntax], ay = tp[(4 + 3 * r) * ntax], az = tp[(5 + 3 * r) * ntax];
            const V3<R> row = mulMv(Rt, mk3<R>(ax, ay, az));      // (A R^T)_r = (R a_r)^T
            AR.m[3 * r] = row.x; AR.m[3 * r + 1] = row.y; AR.m[3 * r + 2] = row.z;
          }
        }
        for (int d = 0; d < XS; ++d) {
          V3<R> dF;
          if (d < nr) {
            const R* tt = Q0 + 12 * d;
            const V3<R> dth = ldv(tt), drho = ldv(tt + 3), dw = ldv(tt + 6), dv = ldv(tt + 9);
            const V3<R> dx = cross3(dth, xP) + drho;
            const V3<R> dxd = dv + cross3(dw, xP) + cross3(Pp.wrel, dx);
            dF = mulMv(Jx, dx) + mulMv(Jv, dxd) - cross3(dth, F);
          } else {
            const R* tt = Q1 + 6 * (d - nr);
            dF = mulMv(Jv, ldv(tt + 3) + cross3(ldv(tt), xP));
          }
          const V3<R> v = mulMv(AR, dF);
          R* od = o + d * ntac3;
          if (jp == 0) { od[0] = v.x; od[1] = v.y; od[2] = v.z; }
          else { od[0] += v.x; od[1] += v.y; od[2] += v.z; }
        }
      }
    }
  }
}

// the launch itself: tsim_launch.h, as every simulation kernel's (the plan: tsim_hip.hip ts_plan)
template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const TjArgs<float>&);
template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const TjArgs<double>&);
