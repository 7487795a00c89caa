// tsim_tactile_normal.hip — the tactile normal equations of a taped episode in one launch (include/tsim.h tsim_tactile_normal_equations; the math
// and the LDS layout: tsim_tactile_normal.h, DESIGN.md §4 "Tactile normal equations").
//   k_tactile_normal   slot = (environment, frame) on the parameter passes' scaffold (tsim_param_pass.h, chunk = frame), 16 / 32 / 64 lanes per
//                      environment; every slot of a wavefront is on the same frame, and a block whose frame is not masked returns at once.  The
//                      frame's LAST taped point is evaluated as k_tactile_jacobian evaluates it (phase 1 alone, seeds (1, 0, 0)).  Per sensor the
//                      taxels are walked `rows` at a time: lanes = taxels evaluate the contact law once per paired primitive and SUM the taxel's
//                      three rows of H = [C | F | r] over the primitives into the slot's LDS tile (H^T W H is not additive over primitives: the
//                      row must be complete before it is multiplied), with k_tactile_jacobian's expressions for the state columns and
//                      k_param_jacobian's for the sensor's four parameter columns, restated here so that neither kernel's code moves.  Then
//                      lanes = entries (d <= e) of the symmetric block add the LOADED taxels' rows, in ascending taxel order, to running sums in
//                      LDS: one fixed summation order at every launch shape, no atomics.  A trip in which no lane of the wavefront holds a loaded
//                      taxel has no product pass.  A sensor's parameter rows and columns are written at its end (the blocks between two sensors'
//                      columns: zeros), the state block at the frame's end; every entry is computed once and mirrored.
// It reads the tape and writes the caller's buffers, nothing else.  NRM does not enter the code (nothing is solved): it is a template parameter so
// that the launch plan names this kernel's instantiations as it names every other's.
// Built like the generic kernels: no fast-math flags.  A unit of its own, so that no other kernel's code moves.
#include <hip/hip_runtime.h>
#include "tsim_kernels.h"
#include "tsim_param_pass.h"
#include "tsim_tactile_normal.h"
#include "tsim_launch.h"

template <class R, int NRM, bool EXPJ, int LPE>
__global__ void __launch_bounds__(TS_WAVE) k_tactile_normal(TnArgs<R> a) {
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
  const bool wp = a.with_params != 0, hr = a.resid != nullptr;
  // the tile's columns (tsim_tactile_normal.h): state, parameters at PC, r at RC, the weight at WC; the product runs over the first ZC
  const int XS = 2 * nr, PC = XS, RC = XS + (wp ? 4 : 0), ZC = RC + (hr ? 1 : 0), TS = ts_tn_stride(nr, a.with_params), WC = TS - 1;
  const int NE = ts_tn_entries(ZC), CR = a.rows;
  const int Z = XS + (wp ? 4 * nsensor : 0);
  const size_t ntac3 = (size_t)3 * ntax;
  // the slot's block
  R* Q0 = lds + a.xoff + slot * ts_tn_slot_reals(nr, a.with_params, CR);
  R* Q1 = Q0 + 12 * nr;
  R* ACC = Q0 + ((18 * nr + 3) & ~3);
  R* TILE = ACC + ((ts_tn_entries(ts_tn_zc(nr, a.with_params, 1)) + 3) & ~3);
  int* tab = reinterpret_cast<int*>(smem_raw + a.toff);
  auto idx = [ZC](int d, int e) { return d * ZC - d * (d - 1) / 2 + e - d; };
  for (int k = threadIdx.x; k < ZC * ZC; k += TS_WAVE) {
    const int d = k / ZC, e = k - d * ZC;
    if (d <= e) tab[idx(d, e)] = d | (e << 8);
  }
  for (int k = lane; k < NE; k += LPE) ACC[k] = R(0);
  // the frame's last taped point: only its (q, qd) is read (the acceleration enters no pose and no velocity)
  const R* rec = pg_rec(a, pg_t(a, (frame + 1) * a.chunk_len - 1), env, REC);
  if (lane < nr) { pg_load_taped(c, rec, nr, lane); c.qa[lane] = R(0); }
  TS_SYNC();
  phase1<R, true, EXPJ>(c, lane, R(1), R(0), R(0));
  const size_t fe = (size_t)tslot * a.B + env;
  R* Nout = a.N_out + fe * Z * Z;
  R* nout = hr ? a.n_out + fe * Z : nullptr;
  const R* rin = hr ? a.resid + fe * ntac3 : nullptr;
  const unsigned long long slot_bits = LPE == TS_WAVE ? ~0ull : ((1ull << (LPE % TS_WAVE)) - 1);
  for (int s = 0; s < nsensor; ++s) {
    const int* si = c.I + c.off_sensor + s * TSIM_SI_SIZE;
    const R* sf = c.F + c.foff_sensor + s * TSIM_SF_SIZE;
    const int tx0 = ts_u(si[TSIM_SI_TAX0]), nt = ts_u(si[TSIM_SI_NTAX]), sp0 = ts_u(si[TSIM_SI_SPRIM0]), nsp = ts_u(si[TSIM_SI_NSPRIM]);
    PairPose<R> Pp; int prim = 0; const R* shape = c.F;
    // the pair of the sensor's primitive jp: its pose, and the dofs' records behind the contexts (k_tactile_jacobian's staging)
    auto stage = [&](int jp) {
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
    };
    // one primitive (every reference model): staged once for the sensor.  Several: the trip loop is outside the primitive loop, because a
    // taxel's row must be summed over the primitives before the product, and each trip stages each primitive again
    if (nsp == 1) stage(0);
    for (int base = 0; base < nt; base += CR) {
      const bool mine = lane < CR && base + lane < nt;
      const int tx = tx0 + base + lane;
      const R* tp = c.Fg + c.foff_tax + tx;
      R* row = TILE + 3 * lane * TS;      // this lane's taxel: rows 3 lane .. 3 lane + 2 of the tile (lane < CR)
      bool loaded = false;                // some primitive so far has loaded this lane's taxel: its row is in the tile
      for (int jp = 0; jp < nsp; ++jp) {
        if (nsp > 1) stage(jp);
        if (!mine) continue;
        // lanes = taxels: the contact law once, every column from it.  out = A^T R_PA^T F, so
        //   d out = A^T R_PA^T (Jx dx + Jv dxd - dth x F),  dx = dth x x + drho,  dxd = dv + dw x x + wrel x dx
        V3<R> F = zero3<R>(); M3<R> Jx, Jv; ContactGeo<R> geo;
        const V3<double> xPd = mulMv(Pp.RPAd, mk3<double>((double)tp[0], (double)tp[ntax], (double)tp[2 * ntax])) + Pp.pPAd;
        const V3<R> xP = cvt3<R>(xPd);
        if (!contact_law<R, true>(prim, shape, sf, xP, Pp.vrel + cross3(Pp.wrel, xP), F, Jx, Jv, xPd, nullptr, true, &geo)) continue;
        // the taxel's frame A (rows) times R_PA^T, once for all columns
        M3<R> AR;
        {
          const M3<R> Rt = Pp.RPA;
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const R ax = tp[(3 + 3 * r) * ntax], ay = tp[(4 + 3 * r) * ntax], az = tp[(5 + 3 * r) * ntax];
            const V3<R> rw = mulMv(Rt, mk3<R>(ax, ay, az));      // (A R^T)_r = (R a_r)^T
            AR.m[3 * r] = rw.x; AR.m[3 * r + 1] = rw.y; AR.m[3 * r + 2] = rw.z;
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
          if (!loaded) { row[d] = v.x; row[TS + d] = v.y; row[2 * TS + d] = v.z; }
          else { row[d] += v.x; row[TS + d] += v.y; row[2 * TS + d] += v.z; }
        }
        if (wp) {      // d out / dp_k = A^T R_PA^T dF/dp_k, p the SENSOR's kn kt mu kd (k_param_jacobian's Ft)
          V3<R> dFp[4];
          contact_law_dparam(geo, sf, dFp);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const V3<R> vl = mulMtv(Pp.RPA, dFp[k]);
            const R o0 = tp[3 * ntax] * vl.x + tp[4 * ntax] * vl.y + tp[5 * ntax] * vl.z;
            const R o1 = tp[6 * ntax] * vl.x + tp[7 * ntax] * vl.y + tp[8 * ntax] * vl.z;
            const R o2 = tp[9 * ntax] * vl.x + tp[10 * ntax] * vl.y + tp[11 * ntax] * vl.z;
            if (!loaded) { row[PC + k] = o0; row[TS + PC + k] = o1; row[2 * TS + PC + k] = o2; }
            else { row[PC + k] += o0; row[TS + PC + k] += o1; row[2 * TS + PC + k] += o2; }
          }
        }
        if (!loaded) {
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            row[r * TS + WC] = a.weight ? a.weight[(size_t)3 * tx + r] : R(1);
            if (hr) row[r * TS + RC] = rin[(size_t)3 * tx + r];
          }
        }
        loaded = true;
      }
      // the product pass, only where some lane of the WAVEFRONT holds a loaded taxel (the trip's other rows are exact zeros of H)
      const unsigned long long bal = __ballot(loaded);
      if (bal == 0) continue;
      TS_SYNC();
      const unsigned long long mine_bits = (bal >> (slot * LPE)) & slot_bits;      // this slot's loaded taxels, ascending
      for (int k = lane; k < NE; k += LPE) {
        const int de = tab[k], d = de & 255, e = de >> 8;
        R acc = ACC[k];
        for (unsigned long long mm = mine_bits; mm; mm &= mm - 1) {
          const R* t = TILE + 3 * (__ffsll((long long)mm) - 1) * TS;
#pragma unroll
          for (int r = 0; r < 3; ++r) acc += (t[r * TS + WC] * t[r * TS + d]) * t[r * TS + e];
        }
        ACC[k] = acc;
      }
      TS_SYNC();
    }
    if (!wp) continue;
    // ---- the sensor's end: its four parameter rows over every column, mirrored into the state rows; the other sensors' columns are zeros
    TS_SYNC();
    const int p0 = XS + 4 * s;
    if (valid) {
      for (int i = lane; i < 4 * Z; i += LPE) {
        const int k = i / Z, j = i - k * Z;
        R v = R(0);
        if (j < XS) v = ACC[idx(j, PC + k)];
        else if (j >= p0 && j < p0 + 4) v = ACC[idx(PC + min(k, j - p0), PC + max(k, j - p0))];
        Nout[(size_t)(p0 + k) * Z + j] = v;
        if (j < XS) Nout[(size_t)j * Z + p0 + k] = v;
      }
      if (hr && lane < 4) nout[p0 + lane] = ACC[idx(PC + lane, RC)];
    }
    TS_SYNC();
    for (int k = lane; k < NE; k += LPE) {      // the next sensor's parameter sums start at zero; the state block's run on
      const int de = tab[k], d = de & 255, e = de >> 8;
      if ((e >= PC && e < PC + 4) || (d >= PC && d < PC + 4)) ACC[k] = R(0);
    }
    TS_SYNC();
  }
  // ---- the frame's end: the state block, every entry from the one sum of its (d <= e), and the state rows of n
  TS_SYNC();
  if (!valid) return;
  for (int i = lane; i < XS * XS; i += LPE) {
    const int d = i / XS, e = i - d * XS;
    Nout[(size_t)d * Z + e] = ACC[idx(min(d, e), max(d, e))];
  }
  if (hr)
    for (int j = lane; j < XS; j += LPE) nout[j] = ACC[idx(j, RC)];
}

// the launch itself: tsim_launch.h, as every simulation kernel's (the plan: tsim_hip.hip tactile_normal_plan)
template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const TnArgs<float>&);
template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const TnArgs<double>&);
