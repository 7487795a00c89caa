// tsim_hip.hip — kernels + C ABI (include/tsim.h) of the MI355X-native batched tactile-simulation step.
//
// Kernels (block = one 64-lane wavefront carrying 64 / LPE environments of LPE lanes each; see tsim_device.h):
//   k_forward   : nframes env-steps of num_steps implicit BDF1 / BDF2 sub-steps (Newton + line search) with the action of
//                 the frame held, tape append, q / qd / variables / tactile read-out per frame
//                                                                <- sim.set_u + sim.forward + getters
//                                                                   (envs/redmax_torch_functions.py:131-136; nframes > 1:
//                                                                   the episode loop of :46-57)
//   k_backward  : adjoint of the newest n taped sub-steps, carrying (lam_q, lam_v) across calls
//                                                                <- sim.backward_steps(n)  (:151-170), sim.backward() (:92)
//   k_readout   : variables + tactile at the current state       <- get_variables / get_tactile_force_vector
//   k_debug_eval: one residual + Newton-matrix evaluation (parity tests)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/tsim.h"
#include "tsim_eval.h"
#include "tsim_policy_push.h"
#include "tsim_static_pusher.h"


#include "tsim_kernels.h"
#include "tsim_param_grad.h"
#include "tsim_launch.h"
#include "tsim_adjoint_pre.h"
#include "tsim_batch.h"      // the batch, the error text, the device guard, the precision dispatch, the owned buffers (host only)

// ================================================================================================ LPT ordering
// One block: counting sort of the environments by their residual-evaluation count of the last launch, descending
// (64 bins; order inside a bin is irrelevant), dealt out to the wavefronts like cards: rank r goes to slot r / nwaves of
// wavefront r % nwaves (slot 0) or nwaves - 1 - r % nwaves (the other slots: see `deal` below).  The expensive environments start first AND sit in different wavefronts — the slots of a
// wavefront are sub-step-synchronous, so two expensive environments in one wavefront cost the sum of their per-sub-step
// maxima (measured: a batch sorted by work runs 22 % slower than the unsorted one, profiles/r01_imbalance_exp.json).
// Runs on the same stream right after k_forward.
// Episode launches (nframes > 1) are ordered by the per-environment TOTALS of the previous episode launch of the same length — useful
// when consecutive episodes resemble each other (the bench replays one table; a GD epoch with fixed start states and a slowly
// changing policy), harmless when they do not (any order is a valid one).  bin = (evals - lo) * 64 / span maps the totals onto the
// 64 bins (lo = 2 evaluations per sub-step, the minimum of a converging Newton loop; span = 2.5 per sub-step); per-step launches keep
// bin = evals (lo 0, span 64).
__global__ void __launch_bounds__(1024) k_order_by_evals(const int* evals, int* order, int B, int ns, int lo, int span, int deal) {
  __shared__ int hist[64], base[64];
  const int t = threadIdx.x;
  if (t < 64) hist[t] = 0;
  __syncthreads();
  auto bin = [lo, span](int ev) { return min(max((ev - lo) * 64 / span, 0), 63); };
  for (int e = t; e < B; e += 1024) atomicAdd(&hist[bin(evals[e])], 1);
  __syncthreads();
  if (t == 0) { int acc = 0; for (int k = 63; k >= 0; --k) { base[k] = acc; acc += hist[k]; } }
  __syncthreads();
  const int nwaves = (B + ns - 1) / ns;
  for (int e = t; e < B; e += 1024) {
    const int r = atomicAdd(&base[bin(evals[e])], 1);           // rank of environment e, 0 = most expensive
    int w = r % nwaves;                                         // slot r / nwaves of wavefront r % nwaves (B % ns == 0)
    const int sl = r / nwaves;
    // deal 2 (round 6, the default): every slot but the first is dealt BACKWARDS — the most expensive environments then share their wavefronts with
    // the cheapest of each quantile, whose slots finish first and become their line-search helpers earliest (D'Claw at B = 2048, two environments per
    // wavefront: 34.9 -> 32.4 ms per 50-step launch; TactilePush 2.766 -> 2.747 ms; TactileInsertion unchanged; profiles/r06_lpt_deal_ab.json).
    // A/B at creation, TSIM_LPT_DEAL: 0 = every slot dealt forwards (rounds 1 - 5), 1 = every other slot backwards (snake: no better than 0).
    if ((deal == 1 && (sl & 1)) || (deal == 2 && sl > 0)) w = nwaves - 1 - w;
    order[w * ns + sl] = e;
  }
}

// ================================================================================================ read-out kernels
// get_variables / get_tactile_force_vector on demand (tsim_readout), in two launches:
//   k_readout   one wavefront per environment: forward kinematics from the taped state, the end-effector variables, and — for the
//               taxel kernel — the pose record of every (sensor, primitive) combination: pose of the sensor link in the primitive's
//               frame (R precision and double) and the relative twist there (what pair_stage_value stages in LDS for the in-kernel
//               read-out of k_forward);
//   k_taxels    lanes = taxels, nothing else: 3 position constants, an fp32 "certainly outside" test, the double-precision position,
//               the penalty law, 12 B out (the 9 axis constants only where a force acts).  ~40 registers instead of the 178 the
//               kinematics need, so 8+ wavefronts per SIMD cover the L2 latency of the constants: this is the one kernel of the path
//               whose time is memory traffic (RollingBall: 40 000 taxels, 480 KB per environment and read-out).
template <class R> struct ReadArgs { const int* I; const R* F; const R* Fenv; int fstride; int B, t0; const R* tape; R* var_out; R* poseR; double* poseD; int nspt; int stage_cpt; int tk; };

template <class R>
__global__ void __launch_bounds__(TS_WAVE) k_readout(ReadArgs<R> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  R* lds = reinterpret_cast<R*>(smem_raw);
  const int env = blockIdx.x, lane = threadIdx.x;
  Ctx<R> c; ctx_init(c, a.I, a.F, lds, 1, 0, lane, TS_WAVE, a.stage_cpt != 0, a.Fenv ? a.Fenv + (size_t)blockIdx.x * a.fstride : nullptr);
  const int nr = c.nr, REC = ts_rec(nr, c.nu, (int)sizeof(R), a.tk);
  init_world(c, lane, TS_WAVE);
  const R* st = a.tape + ((size_t)a.t0 * a.B + env) * REC;
  if (lane < nr) { c.qD[lane] = rec_q(st)[lane]; c.q[lane] = (R)c.qD[lane]; c.qd[lane] = st[rec_qd<R>(nr) + lane]; c.qa[lane] = R(0); }
  TS_SYNC();
  phase1<R, false, true>(c, lane, R(0), R(0), R(0));
  readout<TS_WAVE>(c, lane, env, true, false, a.var_out != nullptr, false, a.var_out, (R*)nullptr);       // variables only
  if (!a.poseR) return;
  int k = 0;
  for (int s = 0; s < c.nsensor; ++s) {
    const int* si = c.I + c.off_sensor + s * TSIM_SI_SIZE;
    for (int j = 0; j < si[TSIM_SI_NSPRIM]; ++j, ++k) {
      TS_SYNC();
      pair_stage_value(c, c.I[c.off_sprim + si[TSIM_SI_SPRIM0] + j], 0, lane == 0);
      TS_SYNC();
      const size_t rec = (size_t)env * a.nspt + k;
      if (lane < TP_R_SIZE) a.poseR[rec * TP_R_SIZE + lane] = c.PP[lane];          // PP_RPA (9), PP_PPA (3), PP_WREL (3), PP_VREL (3)
      if (lane < TP_D_SIZE) a.poseD[rec * TP_D_SIZE + lane] = c.PPd[lane];
    }
  }
}

template <class R> struct TaxArgs { const int* I; const R* F; const R* Fenv; int fstride; const R* poseR; const double* poseD; int nspt; R* tac_out; int slice;
  // blockIdx.x = frame * B + environment: the pose records are [frames][B][nspt] (one frame for tsim_readout; all frames of an episode
  // launch whose read-out was deferred, launch_forward); frame f goes to slot tac_slot[f] of tac_out (null: slot f; < 0: not read out)
  int B; const int* tac_slot;
  // model constants the host knows (header entries and the offset of the staging table): as kernel arguments they cost the prologue no
  // dependent global loads (header -> table offset -> table -> record was four L2 round trips per block, ~2 us of a 28 us kernel)
  int ntax, nsensor, foff_sensor, foff_pair, foff_taxel, tt_off; };

// Per-block staging of everything k_taxels needs that does not depend on the taxel: the block works on ONE environment, so the sensor
// ranges, the primitive of every (sensor, primitive) record with its shape, the sensors' penalty parameters and the pose records are
// put in LDS once; inside the taxel loop the only global accesses left are the taxel's own constants and its 12 output bytes.  (Read
// from global memory in the loop they are chains of dependent ~600-cycle loads — index -> record -> value — and the loop was exactly
// that latency: 55 us for 256 x 40 000 taxels.)  The integer part of the staging (per sensor: end of its taxel range, first record,
// number of records; per record: primitive type, contact pair) is a MODEL constant: the host builds it once (build_sched, ts_tax_table)
// so that the prologue is one cooperative copy instead of a serial walk of dependent global loads by thread 0.
enum { TX_MAXS = 16, TX_MAXK = 64 };
// the three outputs of a taxel, as NON-TEMPORAL stores: the read-out is a pure write stream (0.49 GB at 1024 environments, 1.97 GB at 4096: 2 - 7 x
// the Infinity Cache) that nothing on the device reads back.  Measured (profiles/r04_readout_hbm.md): 1024 environments 4.45 -> 5.40 TB/s,
// 4096 environments 4.4 - 4.8 -> 4.7 - 5.0 TB/s  (Ordinary stores, the A/B's losing side: profiles/r04_readout_hbm.md.)
template <class R> __device__ __forceinline__ void ts_store3(R* o, R a, R b, R c) {
  __builtin_nontemporal_store(a, o); __builtin_nontemporal_store(b, o + 1); __builtin_nontemporal_store(c, o + 2);
}
// One taxel against the staged tables of its environment (LDS): per sensor the end of its taxel range, its first (sensor, primitive)
// record and their number, its penalty parameters; per record the primitive type, its shape, the pose record (R part, double part) and
// the bounding sphere in the sensor-link frame.  The three outputs go out as ONE 12-byte (fp64: 24-byte) store per lane.
template <class R>
__device__ __forceinline__ void taxel_eval(int t, V3<R> xa, int nsensor, const int* sEnd, const int* sKb, const int* sNsp, const int* sPrim, const R* sSf,
                                           const R* sShape, const R* sP, const double* sD, const R* sC, const R* tax, int ntax, R* out) {
  int s = 0;                                                         // sensor of taxel t
  while (s < nsensor - 1 && t >= sEnd[s]) ++s;
  const int kb = sKb[s], nsp = sNsp[s];
  const R* sf = sSf + s * TSIM_SF_SIZE;
  const R* tp = tax + t;
  V3<R> Fl = zero3<R>();                                             // force on the taxel, sensor-link frame
  for (int j = 0; j < nsp; ++j) {
    const R* Cc = sC + (kb + j) * 4;
    const V3<R> dc = xa - ldv(Cc);
    if (Cc[3] >= R(0) && dot3(dc, dc) > Cc[3]) continue;              // outside the primitive's bounding sphere (+ margin)
    const int prim = sPrim[kb + j];
    const R* shape = sShape + (kb + j) * 4;
    const R* P = sP + (kb + j) * TP_R_SIZE;
    const double* D = sD + (kb + j) * TP_D_SIZE;
    const M3<R> RPA = ldm(P);
    // fp32 kernels: the exact shape's distance from an fp32 position, before the double-precision one
    if (sizeof(R) == 4 && !(prim_distance<R>(prim, shape, mulMv(RPA, xa) + ldv(P + 9)) < R(TS_FAR_MARGIN))) continue;
    const V3<double> xPd = mulMv(ldm(D), cvt3<double>(xa)) + ldv(D + 9);
    const V3<R> xP = cvt3<R>(xPd);
    V3<R> Fc; M3<R> Jx, Jv;
    if (contact_law<R, false>(prim, shape, sf, xP, ldv(P + 15) + cross3(ldv(P + 12), xP), Fc, Jx, Jv, xPd)) Fl = Fl + mulMtv(RPA, Fc);
  }
  R o0 = R(0), o1 = R(0), o2 = R(0);
  if (Fl.x != R(0) || Fl.y != R(0) || Fl.z != R(0)) {                // the nine axis constants only for taxels that carry a force
    o0 = Fl.x * tp[3 * ntax] + Fl.y * tp[4 * ntax] + Fl.z * tp[5 * ntax];
    o1 = Fl.x * tp[6 * ntax] + Fl.y * tp[7 * ntax] + Fl.z * tp[8 * ntax];
    o2 = Fl.x * tp[9 * ntax] + Fl.y * tp[10 * ntax] + Fl.z * tp[11 * ntax];
  }
  ts_store3(out + 3 * t, o0, o1, o2);
}
// bounding sphere of a (sensor, primitive) record in the sensor-link frame: centre c_A = -R_PA^T p_PA and (radius + margin)^2, < 0 for planes
template <class R> __device__ __forceinline__ void taxel_bound(const R* P, int prim, const R* sh, R* C) {
  const V3<R> cA = mulMtv(ldm(P), ldv(P + 9)) * R(-1);
  R rb = R(-1);
  if (prim == TSIM_P_SPHERE) rb = sh[0];
  else if (prim == TSIM_P_CUBOID) rb = t_sqrt(sh[0] * sh[0] + sh[1] * sh[1] + sh[2] * sh[2]);
  else if (prim == TSIM_P_CYLINDER) rb = t_sqrt(sh[0] * sh[0] + sh[1] * sh[1]);
  C[0] = cA.x; C[1] = cA.y; C[2] = cA.z;
  C[3] = rb < R(0) ? R(-1) : (rb + R(TS_FAR_MARGIN)) * (rb + R(TS_FAR_MARGIN));
}
enum { TS_TAX_UNROLL = 2 };      // taxels per thread and loop iteration: their loads are in flight together (1 / 2 / 4 measured: profiles/r03_readout_ab.md)
template <class R>
__global__ void __launch_bounds__(256) k_taxels(TaxArgs<R> a) {
  const int rec_env = blockIdx.x, env = rec_env % a.B, frame = rec_env / a.B;
  const int tslot = a.tac_slot ? a.tac_slot[frame] : frame;
  if (tslot < 0) return;                                                // block-uniform
  const int* I = a.I;
  const R* F = a.Fenv ? a.Fenv + (size_t)env * a.fstride : a.F;        // this environment's float records (domain randomisation)
  const int ntax = a.ntax, nsensor = a.nsensor;
  __shared__ int sEnd[TX_MAXS], sKb[TX_MAXS], sNsp[TX_MAXS], sPrim[TX_MAXK];
  __shared__ R sSf[TX_MAXS * TSIM_SF_SIZE], sShape[TX_MAXK * 4], sP[TX_MAXK * TP_R_SIZE];
  __shared__ double sD[TX_MAXK * TP_D_SIZE];
  __shared__ __attribute__((aligned(16))) R sC[TX_MAXK * 4];          // per record: the primitive's centre in the sensor-link frame, (bounding radius + margin)^2
  {
    const int* TT = I + a.tt_off;
    const int foff_sensor = a.foff_sensor, foff_pair = a.foff_pair;
    for (int i = threadIdx.x; i < nsensor; i += 256) { sEnd[i] = TT[3 * i]; sKb[i] = TT[3 * i + 1]; sNsp[i] = TT[3 * i + 2]; }
    for (int i = threadIdx.x; i < a.nspt; i += 256) sPrim[i] = TT[3 * nsensor + 2 * i];
    for (int i = threadIdx.x; i < a.nspt * 4; i += 256) sShape[i] = F[foff_pair + TT[3 * nsensor + 2 * (i >> 2) + 1] * TSIM_PF_SIZE + TSIM_PF_SHAPE + (i & 3)];
    for (int i = threadIdx.x; i < nsensor * TSIM_SF_SIZE; i += 256) sSf[i] = F[foff_sensor + i];
    for (int i = threadIdx.x; i < a.nspt * TP_R_SIZE; i += 256) sP[i] = a.poseR[(size_t)rec_env * a.nspt * TP_R_SIZE + i];
    for (int i = threadIdx.x; i < a.nspt * TP_D_SIZE; i += 256) sD[i] = a.poseD[(size_t)rec_env * a.nspt * TP_D_SIZE + i];
    __syncthreads();
    // "Certainly outside" in 7 instructions: a taxel at x_A (sensor-link frame) cannot touch a primitive whose bounding sphere (centre
    // c_A = -R_PA^T p_PA, radius r_b) it is farther from than r_b + TS_FAR_MARGIN.  Most taxels of a large pad are nowhere near the
    // primitive, and for them this replaces the rotation into the primitive's frame (12 LDS reads, ~25 instructions); the margin is
    // far above the rounding of the test, so the set of taxels contact_law accepts is unchanged.  Planes have no bound (radius < 0).
    for (int k = threadIdx.x; k < a.nspt; k += 256) taxel_bound<R>(sP + k * TP_R_SIZE, sPrim[k], sShape + k * 4, sC + 4 * k);
    __syncthreads();
  }
  const R* tax = a.F + a.foff_taxel;                          // SoA planes: position (3), axis0, axis1, normal (9); shared
  R* out = a.tac_out + ((size_t)tslot * a.B + env) * 3 * ntax;
  const int te = min(ntax, ((int)blockIdx.y + 1) * a.slice);
  // One taxel: its three outputs go out as ONE 12-byte (fp64: 24-byte) store per lane — consecutive lanes, consecutive addresses: a
  // wavefront's store instruction covers 768 contiguous bytes (global_store_dwordx3 in the ISA).  Routing them through LDS for 16-byte
  // vectors instead was measured twice and is slower both ways (block-wide with barriers: round 2; wave-private without: round 3,
  // 2.45 -> 2.12 TB/s on the bench leg, profiles/r03_readout_ab.md).
  auto taxel = [&](int t, V3<R> xa) { taxel_eval<R>(t, xa, nsensor, sEnd, sKb, sNsp, sPrim, sSf, sShape, sP, sD, sC, tax, ntax, out); };
  if (nsensor == 1 && a.nspt == 1 && sC[3] >= R(0)) {
    // One sensor against one bounded primitive (RollingBall's pad and ball, TactilePush's pad and box), in two passes per 1024 taxels:
    //   pass 1  lanes = taxels: 3 loads, the bounding-sphere test against centre / radius^2 held in registers (7 instructions), zeros
    //           stored for the taxels outside; the few inside are appended to a list in LDS;
    //   pass 2  lanes = LISTED taxels: the penalty law, with full wavefronts.
    // Without the list a wavefront runs the ~1000-instruction law whenever ONE of its 64 taxels is near the primitive — 15 % of the
    // wavefronts of the RollingBall pad for 5 % of its taxels, and that was the kernel's time (12.4 M vector instructions for
    // 10.2 M taxels; profiles/r03_readout_ab.md).  A taxel's result does not depend on the lane that computes it: same bits as before.
    enum { CH = 8 };
    __shared__ int sList[256 * CH];
    __shared__ int sCount;
    const V3<R> cA = ldv(sC);
    const R r2 = sC[3];
    const R* px = tax; const R* py = tax + ntax; const R* pz = tax + 2 * ntax;
    // chunks are dealt to the environment's blocks round-robin, not as contiguous slices: the taxels near the primitive lie in a band of
    // the pad (RollingBall: ~50 of 200 rows), and with contiguous slices two of an environment's eight blocks ran the law for all of them
    // while the others stored zeros — the kernel lasted as long as those two
    const int te = ntax;
    for (int base = (int)blockIdx.y * 256 * CH; base < te; base += (int)gridDim.y * 256 * CH) {
      if (threadIdx.x == 0) sCount = 0;
      __syncthreads();
      V3<R> xa[CH];
#pragma unroll
      for (int r = 0; r < CH; ++r) {                                   // all loads of the chunk in flight together
        const int tr = min(base + (int)threadIdx.x + 256 * r, te - 1);
        xa[r] = mk3<R>(px[tr], py[tr], pz[tr]);
      }
#pragma unroll
      for (int r = 0; r < CH; ++r) {
        const int tr = base + (int)threadIdx.x + 256 * r;
        if (tr < te) {
          const V3<R> dc = xa[r] - cA;
          if (dot3(dc, dc) > r2) ts_store3(out + 3 * tr, R(0), R(0), R(0));
          else sList[atomicAdd(&sCount, 1)] = tr;
        }
      }
      __syncthreads();
      const int n = sCount;
      for (int i = threadIdx.x; i < n; i += 256) {
        const int tr = sList[i];
        taxel(tr, mk3<R>(px[tr], py[tr], pz[tr]));
      }
      __syncthreads();
    }
    return;
  }
  for (int t = (int)blockIdx.y * a.slice + (int)threadIdx.x; t < te; t += 256 * TS_TAX_UNROLL) {
    V3<R> xa[TS_TAX_UNROLL];
#pragma unroll
    for (int r = 0; r < TS_TAX_UNROLL; ++r) {                          // positions of all of this iteration's taxels first: loads in flight together
      const int tr = min(t + 256 * r, te - 1);
      xa[r] = mk3<R>(tax[tr], tax[tr + ntax], tax[tr + 2 * ntax]);
    }
#pragma unroll
    for (int r = 0; r < TS_TAX_UNROLL; ++r)
      if (t + 256 * r < te) taxel(t + 256 * r, xa[r]);
  }
}

// Small pads, many records (the frames of an episode launch: 81 920 records of 130 taxels on BASELINE's headline batch): one block per
// record is all prologue (k_taxels above: ~3 us of dependent loads and two barriers for 130 taxels).  Here a block stages TXS_RPB records
// at once — one cooperative copy, one barrier — and its threads then run over (record, taxel) items; consecutive items are consecutive
// taxels of one record, so loads and the 12-byte stores stay contiguous.  Same taxel_eval, same tables: the same bits as k_taxels.
// sub: the launch covers the environments order[e0 .. e0 + n) only — item g of its nrec = frames x n is frame g / n of the g % n-th of them —; the
// records and the outputs keep their place, frame * B + environment.  (e0 = 0, n = B, no order: item g is record g, as ever.)
enum { TXS_RPB = 16, TXS_MAXK = 8, TXS_MAXS = 4, TXS_MAX_TAXELS = 1024 };
template <class R>
__global__ void __launch_bounds__(256) k_taxels_small(TaxArgs<R> a, int nrec, TsSubRange sub) {
  const int rec0 = blockIdx.x * TXS_RPB, nr_ = min((int)TXS_RPB, nrec - rec0);
  const int ntax = a.ntax, nsensor = a.nsensor, nspt = a.nspt;
  __shared__ int sEnd[TXS_MAXS], sKb[TXS_MAXS], sNsp[TXS_MAXS], sPrim[TXS_MAXK], sPair[TXS_MAXK], sSlot[TXS_RPB], sEnv[TXS_RPB], sRec[TXS_RPB];
  __shared__ R sSf[TXS_RPB][TXS_MAXS * TSIM_SF_SIZE], sShape[TXS_RPB][TXS_MAXK * 4], sP[TXS_RPB][TXS_MAXK * TP_R_SIZE];
  __shared__ double sD[TXS_RPB][TXS_MAXK * TP_D_SIZE];
  __shared__ __attribute__((aligned(16))) R sC[TXS_RPB][TXS_MAXK * 4];
  __shared__ R sX[3 * TXS_MAX_TAXELS];                                  // the taxels' positions (shared by all records): no global load left in the item loop
  const R* tax = a.F + a.foff_taxel;
  for (int i = threadIdx.x; i < 3 * ntax; i += 256) sX[i] = tax[i];
  const int* TT = a.I + a.tt_off;
  for (int i = threadIdx.x; i < nsensor; i += 256) { sEnd[i] = TT[3 * i]; sKb[i] = TT[3 * i + 1]; sNsp[i] = TT[3 * i + 2]; }
  for (int i = threadIdx.x; i < nspt; i += 256) { sPrim[i] = TT[3 * nsensor + 2 * i]; sPair[i] = TT[3 * nsensor + 2 * i + 1]; }
  for (int i = threadIdx.x; i < nr_; i += 256) {
    const int fr = (rec0 + i) / sub.n, ei = sub.e0 + (rec0 + i) - fr * sub.n, env = sub.order ? sub.order[ei] : ei;
    sSlot[i] = a.tac_slot ? a.tac_slot[fr] : fr; sEnv[i] = env; sRec[i] = fr * a.B + env;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nr_ * nspt * TP_R_SIZE; i += 256) { const int r = i / (nspt * TP_R_SIZE), e = i % (nspt * TP_R_SIZE); sP[r][e] = a.poseR[(size_t)sRec[r] * nspt * TP_R_SIZE + e]; }
  for (int i = threadIdx.x; i < nr_ * nspt * TP_D_SIZE; i += 256) { const int r = i / (nspt * TP_D_SIZE), e = i % (nspt * TP_D_SIZE); sD[r][e] = a.poseD[(size_t)sRec[r] * nspt * TP_D_SIZE + e]; }
  for (int i = threadIdx.x; i < nr_ * nsensor * TSIM_SF_SIZE; i += 256) {
    const int r = i / (nsensor * TSIM_SF_SIZE), e = i % (nsensor * TSIM_SF_SIZE);
    const R* F = a.Fenv ? a.Fenv + (size_t)sEnv[r] * a.fstride : a.F;
    sSf[r][e] = F[a.foff_sensor + e];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nr_ * nspt * 4; i += 256) {
    const int r = i / (nspt * 4), e = i % (nspt * 4);
    const R* F = a.Fenv ? a.Fenv + (size_t)sEnv[r] * a.fstride : a.F;
    sShape[r][e] = F[a.foff_pair + sPair[e >> 2] * TSIM_PF_SIZE + TSIM_PF_SHAPE + (e & 3)];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nr_ * nspt; i += 256) { const int r = i / nspt, k = i % nspt; taxel_bound<R>(sP[r] + k * TP_R_SIZE, sPrim[k], sShape[r] + k * 4, sC[r] + 4 * k); }
  __syncthreads();
  for (int item = threadIdx.x; item < nr_ * ntax; item += 256) {
    const int r = item / ntax, t = item - r * ntax;
    const int tslot = sSlot[r];
    if (tslot < 0) continue;
    R* out = a.tac_out + ((size_t)tslot * a.B + sEnv[r]) * 3 * ntax;
    taxel_eval<R>(t, mk3<R>(sX[t], sX[t + ntax], sX[t + 2 * ntax]), nsensor, sEnd, sKb, sNsp, sPrim, sSf[r], sShape[r], sP[r], sD[r], sC[r], tax, ntax, out);
  }
}

// ================================================================================================ branch signature
// Diagnostics (tsim_debug_signature): for the taped sub-steps t_first+1 .. t_first+n of every environment, which contact
// points / taxels penetrate and on which smooth piece of the penalty law (stick / slip, face of the primitive) each one is,
// recomputed from the taped state (q as double, qd) exactly as the backward kernel re-evaluates it.  Two trajectories with
// equal signatures went through the same smooth pieces, so their gradients are comparable; where they differ, one of them
// crossed a contact / friction kink.  One environment per 64-lane block; lanes = points.
template <class R> struct SigArgs { const int* I; const R* F; const R* Fenv; int fstride; int B, t_first, n; const R* tape; unsigned* out; int stage_cpt; int tk; };

__device__ __forceinline__ unsigned wave_sum_u32(unsigned x) {
  for (int off = 32; off > 0; off >>= 1) x += (unsigned)lane_gather((int)x, (int)threadIdx.x ^ off);
  return x;
}

template <class R>
__global__ void __launch_bounds__(TS_WAVE) k_signature(SigArgs<R> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  R* lds = reinterpret_cast<R*>(smem_raw);
  const int env = blockIdx.x, lane = threadIdx.x;
  Ctx<R> c; ctx_init(c, a.I, a.F, lds, 1, 0, lane, TS_WAVE, a.stage_cpt != 0, a.Fenv ? a.Fenv + (size_t)blockIdx.x * a.fstride : nullptr);
  const int nr = c.nr, REC = ts_rec(nr, c.nu, (int)sizeof(R), a.tk);
  init_world(c, lane, TS_WAVE);
  for (int j = 0; j < a.n; ++j) {
    const R* st = a.tape + ((size_t)(a.t_first + 1 + j) * a.B + env) * REC;
    TS_SYNC();
    if (lane < nr) { c.qD[lane] = rec_q(st)[lane]; c.q[lane] = (R)c.qD[lane]; c.qd[lane] = st[rec_qd<R>(nr) + lane]; c.qa[lane] = R(0); }
    TS_SYNC();
    phase1<R, false, true>(c, lane, R(0), R(0), R(0));
    unsigned cnt = 0, sum = 0;
    for (int pk = 0; pk < c.npair; ++pk) {                     // dynamics-active contact pairs
      const int* pi = c.I + c.off_pair + pk * TSIM_PI_SIZE;
      if (!(pi[TSIM_PI_FLAGS] & 1)) continue;
      const R* pf = c.F + c.foff_pair + pk * TSIM_PF_SIZE;
      TS_SYNC();
      pair_stage_value(c, pk, 0, lane == 0);
      TS_SYNC();
      const R* S = c.PP;
      const M3<double> RPAd = ldm(c.PPd); const V3<double> pPAd = ldv(c.PPd + 9);
      const V3<R> wrel = ldv(S + PP_WREL), vrel = ldv(S + PP_VREL);
      for (int i = lane; i < pi[TSIM_PI_NPT]; i += TS_WAVE) {
        V3<double> xPd = mulMv(RPAd, cvt3<double>(ld_cpt(c, pi[TSIM_PI_PT0] + i))) + pPAd;
        if (pi[TSIM_PI_FLAGS] & 2) xPd.z -= (double)pf[TSIM_PF_SHAPE];
        const V3<R> xP = cvt3<R>(xPd);
        V3<R> F; M3<R> Jx, Jv; int br = 0;
        if (contact_law<R, false>(pi[TSIM_PI_PRIM], pf + TSIM_PF_SHAPE, pf + TSIM_PF_KN, xP, vrel + cross3(wrel, xP), F, Jx, Jv, xPd, &br)) {
          ++cnt; sum += ts_sig_mix((unsigned)pk, (unsigned)i, (unsigned)(1 + br));
        }
      }
    }
    for (int s = 0; s < c.nsensor; ++s) {                      // taxels against the primitives paired with their sensor
      const int* si = c.I + c.off_sensor + s * TSIM_SI_SIZE;
      const R* sf = c.F + c.foff_sensor + s * TSIM_SF_SIZE;
      for (int jp = 0; jp < si[TSIM_SI_NSPRIM]; ++jp) {
        const int pk = c.I[c.off_sprim + si[TSIM_SI_SPRIM0] + jp];
        const int* pi = c.I + c.off_pair + pk * TSIM_PI_SIZE;
        const R* pf = c.F + c.foff_pair + pk * TSIM_PF_SIZE;
        TS_SYNC();
        pair_stage_value(c, pk, 0, lane == 0);
        TS_SYNC();
        const R* S = c.PP;
        const V3<R> wrel = ldv(S + PP_WREL), vrel = ldv(S + PP_VREL);
        for (int i = lane; i < si[TSIM_SI_NTAX]; i += TS_WAVE) {
          const R* tp = c.Fg + c.foff_tax + si[TSIM_SI_TAX0] + i;
          const V3<double> xPd = mulMv(ldm(c.PPd), mk3<double>((double)tp[0], (double)tp[c.ntax], (double)tp[2 * c.ntax])) + ldv(c.PPd + 9);
          const V3<R> xP = cvt3<R>(xPd);
          V3<R> F; M3<R> Jx, Jv; int br = 0;
          if (contact_law<R, false>(pi[TSIM_PI_PRIM], pf + TSIM_PF_SHAPE, sf, xP, vrel + cross3(wrel, xP), F, Jx, Jv, xPd, &br)) {
            ++cnt; sum += ts_sig_mix(0x10000u + (unsigned)(si[TSIM_SI_SPRIM0] + jp), (unsigned)i, (unsigned)(1 + br));
          }
        }
      }
    }
    cnt = wave_sum_u32(cnt); sum = wave_sum_u32(sum);
    if (lane == 0) { unsigned* o = a.out + ((size_t)j * a.B + env) * 2; o[0] = cnt; o[1] = sum; }
  }
}

// ================================================================================================ host side
int tsim_fail_(const std::string& m) { return fail(m); }      // for the library's other translation units (tsim_model.cpp)

// The state changed other than by a forward launch (or is about to, in a captured graph): tsim_readout recomputes the kinematics.
static void pose_invalidate(tsim_batch* b, hipStream_t st) {
  b->pose_valid = 0;
  if (capturing(st)) b->pose_off = 1;
}


// sweep schedule of the link tree (layout: ts_sched in tsim_device.h)
static std::vector<int32_t> build_sched(const std::vector<int32_t>& I, const std::vector<double>& F) {
  const int nl = I[TSIM_IH_NL], nr = I[TSIM_IH_NR], ol = I[TSIM_IH_OFF_LINK];
  std::vector<int> parent(nl + 1, 0), branch(nl + 1, -1), dof_link(nr, 0);
  std::vector<std::vector<int>> links;                       // links of each root branch, parents before children
  for (int i = 1; i <= nl; ++i) {
    const int32_t* li = &I[ol + (i - 1) * TSIM_LI_SIZE];
    parent[i] = li[TSIM_LI_PARENT];
    if (parent[i] == 0) { branch[i] = (int)links.size(); links.emplace_back(); }
    else branch[i] = branch[parent[i]];
    links[branch[i]].push_back(i);
    for (int k = li[TSIM_LI_DOF0]; k < li[TSIM_LI_DOF0] + li[TSIM_LI_NDOF]; ++k) dof_link[k] = i;
  }
  int nsteps = 0;
  for (auto& l : links) nsteps = std::max(nsteps, (int)l.size());
  std::vector<int> leader(links.size(), -1);                 // lowest dof lane of each branch
  for (int k = nr - 1; k >= 0; --k) leader[branch[dof_link[k]]] = k;
  const int npair = I[TSIM_IH_NPAIR], op = I[TSIM_IH_OFF_PAIR];
  const int nu = I[TSIM_IH_NU], om = I[TSIM_IH_OFF_MOTOR];
  std::vector<int32_t> S(TS_SCHED_ENT + nsteps * 16 + nl * TS_LR_SIZE + npair * TSIM_PI_SIZE + 16 + nu * TSIM_MI_SIZE, 0);
  S[0] = (int32_t)S.size(); S[1] = nsteps;
  for (int l = 0; l < 16; ++l) S[TS_SCHED_BRANCH + l] = l < nr ? branch[dof_link[l]] : -1;
  for (size_t b = 0; b < links.size() && b < 16; ++b) S[TS_SCHED_LEADER + b] = leader[b];
  S[TS_SCHED_NB] = (int32_t)links.size();
  for (int st = 0; st < nsteps; ++st)
    for (int l = 0; l < nr && l < 16; ++l) {
      const int br = branch[dof_link[l]];
      if (st < (int)links[br].size()) S[TS_SCHED_ENT + st * 16 + l] = links[br][st] | ((leader[br] == l) ? 0x100 : 0);
    }
  const int rec0 = TS_SCHED_ENT + nsteps * 16;
  for (int i = 1; i <= nl; ++i) {
    const int32_t* li = &I[ol + (i - 1) * TSIM_LI_SIZE];
    int32_t* r = &S[rec0 + (i - 1) * TS_LR_SIZE];
    r[TS_LR_PARENT] = li[TSIM_LI_PARENT]; r[TS_LR_JTYPE] = li[TSIM_LI_JTYPE]; r[TS_LR_DOF0] = li[TSIM_LI_DOF0];
    r[TS_LR_NDOF] = li[TSIM_LI_NDOF]; r[TS_LR_ANCMASK] = li[TSIM_LI_ANCMASK]; r[TS_LR_BRANCH] = branch[i];
  }
  for (int e = 0; e < npair * TSIM_PI_SIZE; ++e) S[rec0 + nl * TS_LR_SIZE + e] = I[op + e];      // pair int records
  {                                                                                              // taxel staging table (k_taxels), offset in S[TS_SCHED_TAXTAB]
    const int ns_ = I[TSIM_IH_NSENSOR], os = I[TSIM_IH_OFF_SENSOR], osp = I[TSIM_IH_OFF_SPRIM];
    S[TS_SCHED_TAXTAB] = (int32_t)S.size();
    int kb = 0;
    for (int s = 0; s < ns_; ++s) {
      const int32_t* si = &I[os + s * TSIM_SI_SIZE];
      S.push_back(si[TSIM_SI_TAX0] + si[TSIM_SI_NTAX]); S.push_back(kb); S.push_back(si[TSIM_SI_NSPRIM]);
      kb += si[TSIM_SI_NSPRIM];
    }
    for (int s = 0; s < ns_; ++s) {
      const int32_t* si = &I[os + s * TSIM_SI_SIZE];
      for (int j = 0; j < si[TSIM_SI_NSPRIM]; ++j) {
        const int pk = I[osp + si[TSIM_SI_SPRIM0] + j];
        S.push_back(I[op + pk * TSIM_PI_SIZE + TSIM_PI_PRIM]); S.push_back(pk);
      }
    }
    S[0] = (int32_t)S.size();
  }
  {   // bounding sphere of each contact pair's points, link-A frame (ts_pair_bound): centre of the points' box, radius rounded UP
    S[TS_SCHED_PBOUND] = (int32_t)S.size();
    const int ncpt = I[TSIM_IH_NCPT], fc = I[TSIM_IH_FOFF_CPT];
    for (int pk = 0; pk < npair; ++pk) {
      const int32_t* pi = &I[op + pk * TSIM_PI_SIZE];
      const int p0_ = pi[TSIM_PI_PT0], n_ = pi[TSIM_PI_NPT];
      float bd[4] = {0.f, 0.f, 0.f, -1.f};
      if (n_ > 0 && !(pi[TSIM_PI_FLAGS] & 2)) {
        double lo[3], hi[3], cc[3];
        for (int a_ = 0; a_ < 3; ++a_) { lo[a_] = 1e300; hi[a_] = -1e300; }
        for (int i = 0; i < n_; ++i) for (int a_ = 0; a_ < 3; ++a_) { const double v = F[fc + a_ * ncpt + p0_ + i]; lo[a_] = std::min(lo[a_], v); hi[a_] = std::max(hi[a_], v); }
        for (int a_ = 0; a_ < 3; ++a_) { bd[a_] = (float)(0.5 * (lo[a_] + hi[a_])); cc[a_] = (double)bd[a_]; }      // the centre the device will use
        double r2 = 0.0;
        for (int i = 0; i < n_; ++i) { double d2 = 0.0; for (int a_ = 0; a_ < 3; ++a_) { const double d = F[fc + a_ * ncpt + p0_ + i] - cc[a_]; d2 += d * d; } r2 = std::max(r2, d2); }
        bd[3] = (float)(std::sqrt(r2) * (1.0 + 1e-6) + 1e-7);
      }
      for (int e = 0; e < 4; ++e) { int32_t w; std::memcpy(&w, &bd[e], 4); S.push_back(w); }
    }
    S[0] = (int32_t)S.size();
  }
  const int dm0 = rec0 + nl * TS_LR_SIZE + npair * TSIM_PI_SIZE;                                 // dof -> motor, motor int records
  for (int j = 0; j < 16; ++j) S[dm0 + j] = -1;
  for (int m = 0; m < nu; ++m) {
    const int j = I[om + m * TSIM_MI_SIZE + TSIM_MI_DOF];
    if (j >= 0 && j < 16) S[dm0 + j] = S[dm0 + j] == -1 ? m : -2;
    for (int e = 0; e < TSIM_MI_SIZE; ++e) S[dm0 + 16 + m * TSIM_MI_SIZE + e] = I[om + m * TSIM_MI_SIZE + e];
  }
  return S;
}

// Does the batch's model equal a compiled-in static model (int blob and float records, bit for bit)?  Then its launches may use the
// instantiation that has the model's structure folded in (tsim_static.h); any edit of a record (tsim_update_model) drops back to the
// generic kernels, and so do per-environment tables.
// Is the batch's model the compiled-in one in everything the static kernels take from it?  All int records and all float records in front of
// the per-point arrays, bit for bit — EXCEPT the taxel layout (number of taxels, a sensor's taxel range and image shape): the static code reads
// none of it (the read-out kernels and the tactile adjoint take taxels from the batch's own blob), so a TactilePush pad re-gridded to
// 13 x 13 taxels (BASELINE configs[1]) runs on the same instantiation as the XML's 13 x 10.
template <class MS> static bool blob_ints_static(const tsim_batch* b) {
  if ((int)b->I.size() != MS::NI || b->I[TSIM_IH_FOFF_CPT] != MS::NFREC) return false;
  auto taxel_layout = [&](int i) {
    if (i == TSIM_IH_NTAXEL || i == TSIM_IH_NF || i == TSIM_IH_NDOF_TACTILE) return true;
    const int os = MS::Iv(TSIM_IH_OFF_SENSOR), ns = MS::Iv(TSIM_IH_NSENSOR);
    if (i >= os && i < os + ns * TSIM_SI_SIZE) { const int f = (i - os) % TSIM_SI_SIZE; return f == TSIM_SI_TAX0 || f == TSIM_SI_NTAX || f == TSIM_SI_ROWS || f == TSIM_SI_COLS; }
    return false;
  };
  for (int i = 0; i < MS::NI; ++i) if (b->I[i] != MS::Iv(i) && !taxel_layout(i)) return false;
  return true;
}
template <class MS> static bool blob_equals_static(const tsim_batch* b) {
  if (!blob_ints_static<MS>(b)) return false;
  // fp64 batches: the doubles, bit for bit.  fp32 batches: the FLOATS, bit for bit — the fp32 kernels see a model's reals only after their conversion to
  // float (upload_model; ts_F casts the compiled-in constant the same way), so a blob that differs from the asset below float resolution (another host's
  // BLAS in the Python compiler, the native loader of tsim_model.cpp: last bits of mesh-derived mass properties) IS the compiled-in model to them.
  for (int i = 0; i < MS::NFREC; ++i) {
    if (b->dtype == TSIM_F32) { const float x = (float)b->F[i], y = (float)MS::Fv(i); if (std::memcmp(&x, &y, sizeof(float)) != 0) return false; }
    else if (std::memcmp(&b->F[i], (const double[]){MS::Fv(i)}, sizeof(double)) != 0) return false;
  }
  return true;
}
// ... or in its STRUCTURE only: all ints (but the taxel layout) and the structural floats of the compiled asset (TsParam::Fk: exact 0, 1, -1)
template <class MS> static bool blob_has_structure(const tsim_batch* b) {
  if (!blob_ints_static<MS>(b)) return false;
  for (int i = 0; i < MS::NFREC; ++i) if (MS::Fk(i) && !(b->F[i] == MS::Fv(i))) return false;
  return true;
}
static void detect_static_model(tsim_batch* b) {
  b->static_id = blob_has_structure<TsParam<TsStaticPusher>>(b) ? 1 : 0;
  b->static_exact = b->static_id == 1 && blob_equals_static<TsStaticPusher>(b);
}
// is there an instantiation of the compiled-in model for this kernel at this shape (the batch's precision; tsim_launch.h ts_instantiated)?
static bool pusher_instantiated(const tsim_batch* b, int kernel, bool policy, bool default_opts, int lpe) {
  constexpr int nrm = ts_view_nrm<TsStaticPusher>();
  return ts_instantiated(kernel, nrm, b->dtype == TSIM_F32, policy, default_opts, nrm, false, lpe);
}
// the view the batch's model may run on (TS_KM_*, tsim_launch.h), under lanes per environment forced to lpe_forced (0: none): a forced shape
// the compiled-in model has no instantiation at (fp64 at 16 lanes: its LDS is over the automatic cap) keeps the generic kernels
static int kernel_mode(const tsim_batch* b, int lpe_forced) {
  if (b->static_id == 0 || b->no_static) return TS_KM_GENERIC;
  if (lpe_forced && !pusher_instantiated(b, TS_K_FORWARD, false, false, lpe_forced)) return TS_KM_GENERIC;
  if (b->dFenv) return b->env_struct_ok ? TS_KM_PARAM : TS_KM_GENERIC;      // (the table check is fp32 only: fp64 batches with per-environment tables stay generic)
  return b->static_exact ? TS_KM_STATIC : TS_KM_PARAM;
}
// every solver / scheduling option of the batch at its default: the forward launch of a compiled-in model may use the TsDefaultOpts<> instantiation
// (tsim_static.h), which has them as constants.  (TSIM_NO_DEFAULT_OPTS=1 at creation keeps the run-time-option kernel: A/B.)
static bool default_options(const tsim_batch* b) {
  return b->cross_kinks == 1 && b->eval_budget == 0 && b->value_trials == 2 && b->trial_helpers == 1 && b->value_first == 1 && !b->ab_lockstep && !b->ab_no_default_opts;
}
static int upload_model(tsim_batch* b, hipStream_t st) {
  detect_static_model(b);
  HIPCHK(hipMemcpyAsync(b->dI, b->I.data(), b->I.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  {
    std::vector<int32_t> S = build_sched(b->I, b->F);              // appended to the device copy at I[TSIM_IH_NI]
    if ((int)S.size() != b->nsched) return fail("sweep schedule size changed");
    b->tt_off = b->I[TSIM_IH_NI] + S[TS_SCHED_TAXTAB];
    HIPCHK(hipMemcpyAsync((int32_t*)b->dI + b->I.size(), S.data(), S.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return by_real(b, [&](auto r) {
    const std::vector<decltype(r)> f(b->F.begin(), b->F.end());      // the float records in the batch's real type
    HIPCHK(hipMemcpyAsync(b->dF, f.data(), f.size() * sizeof(r), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));   // f is a temporary
    return 0;
  });
}

// Zero-fill by a plain kernel.  hipMemsetAsync nodes did NOT reliably take effect when a captured HIP graph was replayed
// (the carried adjoint kept the previous episode's final value at B >= 2048: policy gradients of 1e16 ... NaN in the graphed GD
// loop as soon as an episode's data changed; profiles/r02_graphed_rollout_fix.md) — a kernel node does.
__global__ void k_zero_words(uint32_t* p, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0u;
}
static int zero_async(void* p, size_t bytes, hipStream_t st) {
  const size_t n = bytes / 4;                       // all buffers zeroed here hold 4- or 8-byte reals
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_zero_words, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (uint32_t*)p, n);
  HIPCHK(hipGetLastError());
  return 0;
}

// do the per-environment tables [B][nfrec] keep the structural floats of the compiled-in model (mask km: 1 = structural; ref: the batch's
// shared records, which do)?  flag != 0: some environment does not
__global__ void k_check_structure(const float* tables, const float* ref, const unsigned char* km, int nfrec, size_t n, int* flag) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int f = (int)(i % (size_t)nfrec);
  if (km[f] && !(tables[i] == ref[f])) atomicOr(flag, 1);
}
// the float header of every per-environment row (time step, gravity, Newton tolerance) is the shared model's: see tsim_set_env_tables
template <class R> __global__ void k_env_header(R* tables, const R* ref, int nfrec, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * TSIM_FH_SIZE) tables[(size_t)(i / TSIM_FH_SIZE) * nfrec + i % TSIM_FH_SIZE] = ref[i % TSIM_FH_SIZE];
}
// scatter [B][nr] q / qd into tape record 0
template <class R> __global__ void k_set_state(R* tape, const R* q, const R* qd, int B, int nr, int rec) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * nr) return;
  int env = i / nr, k = i % nr;
  rec_q(tape + (size_t)env * rec)[k] = (double)q[i];
  tape[(size_t)env * rec + rec_qd<R>(nr) + k] = qd ? qd[i] : R(0);
}
// masked variant: only environments with mask[env] != 0 get the new state (record t of the tape)
template <class R> __global__ void k_set_state_masked(R* tape_rec, const R* q, const R* qd, const int32_t* mask, double* prev, R h, int B, int nr, int rec) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * nr) return;
  int env = i / nr, k = i % nr;
  if (!mask[env]) return;
  rec_q(tape_rec + (size_t)env * rec)[k] = (double)q[i];
  tape_rec[(size_t)env * rec + rec_qd<R>(nr) + k] = qd ? qd[i] : R(0);
  if (prev) { const double v = qd ? (double)qd[i] : 0.0; prev[(size_t)env * 2 * nr + k] = (double)q[i] - (double)h * v; prev[(size_t)env * 2 * nr + nr + k] = v; }
}
template <class R> __global__ void k_get_state(const R* tape_rec, R* q, R* qd, int B, int nr, int rec) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * nr) return;
  int env = i / nr, k = i % nr;
  if (q) q[i] = (R)rec_q(tape_rec + (size_t)env * rec)[k];
  if (qd) qd[i] = tape_rec[(size_t)env * rec + rec_qd<R>(nr) + k];
}

// dynamic LDS of a block of nslot environments
static size_t lds_bytes_for(const tsim_batch* b, int nslot) {
  const int reals = ts_lds_reals(b->nl, b->nr, b->nu, b->nfrec, b->I[TSIM_IH_NCPT], b->stage_cpt != 0, nslot, bool(b->dFenv), b->nsched + (int)b->I.size(), (int)b->esz);
  return ((size_t)reals * b->esz + 15) / 16 * 16;
}
// Launch shape of the forward / backward kernels.
// Lanes per environment (LPE): one environment per wavefront uses <= nr of the 64 lanes in most phases; packing 2 or 4
// environments into a wavefront divides the instruction count per environment.  These kernels hold one wavefront per
// SIMD (~270 registers; holding them to 256 for two per SIMD spills and is slower at every batch size measured,
// profiles/r01_launch_shape_ab.txt) and a lone wavefront is latency-bound, so the time of a launch is
//     rounds x latency(LPE),   rounds = ceil(wavefronts / #SIMDs),   latency(64 : 32 : 16) ~ 1 : 0.93 : 1.02
// (phase stamps, tools/phase_cycles.py).  The launch takes the LPE that minimises it, subject to the block's LDS
// leaving room for four blocks per CU.
// lpe_forced: the shape asked for (0: automatic).
struct LaunchShape { int lpe; unsigned grid; size_t lds; };
static LaunchShape launch_shape(const tsim_batch* b, int lpe_forced) {
  LaunchShape L;
  int lpe = lpe_forced;
  const size_t lds_cap = lpe_forced ? 64 * 1024 : 40 * 1024;
  if (!lpe) {
    lpe = TS_WAVE;
    double best = 1e30;
    const int cand[3] = {64, 32, 16};
    // (the fused static kernels: 1 : 1.13 : 1.24 — their rounds get cheaper with more lanes per environment, so a batch that fills the SIMDs
    // with one environment per wavefront takes that shape: TactilePush 13 x 13 at B = 1024, forward only: 9.0 / 8.0 / 7.3 M env-steps/s)
    const bool fused_static = kernel_mode(b, 0) != TS_KM_GENERIC;
    const double lat_generic[3] = {1.0, 0.93, 1.02}, lat_static[3] = {1.0, 1.13, 1.24};
    const double* lat = fused_static ? lat_static : lat_generic;
    for (int i = 0; i < 3; ++i) {
      const int ns = TS_WAVE / cand[i];
      if (i > 0 && lds_bytes_for(b, ns) > lds_cap) break;
      const long long waves = ((long long)b->B + ns - 1) / ns;
      const double t = (double)((waves + b->n_simd - 1) / b->n_simd) * lat[i];
      if (t < best) { best = t; lpe = cand[i]; }
    }
  }
  if (b->has_exp) lpe = TS_WAVE;
  while (lpe < TS_WAVE && lds_bytes_for(b, TS_WAVE / lpe) > lds_cap) lpe *= 2;
  L.lpe = lpe;
  const int ns = TS_WAVE / lpe;
  L.grid = (unsigned)((b->B + ns - 1) / ns);
  L.lds = lds_bytes_for(b, ns);
  return L;
}
// Stage the contact-point arrays in LDS (one copy per block) if they are small and the launch keeps its lanes-per-environment shape with
// them; re-decided whenever what the shape depends on changes (forced lanes, per-environment tables on / off).
static void decide_stage_cpt(tsim_batch* b) {
  b->stage_cpt = 0;
  if ((size_t)3 * b->I[TSIM_IH_NCPT] * b->esz > TS_CPT_LDS_BYTES) return;
  if (b->dFenv && b->ab_no_envtab_cpt) return;      // A/B: the round-3 behaviour (contact points from global memory next to per-environment tables)
  const int lpe0 = launch_shape(b, b->lpe_forced).lpe;
  b->stage_cpt = 1;
  if (launch_shape(b, b->lpe_forced).lpe != lpe0 || lds_bytes_for(b, 1) > 64 * 1024) b->stage_cpt = 0;
}
// What the launch shape depends on may have changed (forced lanes, the view, the model, per-environment tables): the block orders of the last
// launches are for another shape, and the staging is decided again (the flag travels with every launch as a kernel argument: nothing on the device to update)
static void shape_changed(tsim_batch* b) {
  b->order_valid = 0; b->order_ep_n = 0;
  decide_stage_cpt(b);
}
// ================================================================================================ launch plan
// Which instantiation of a simulation kernel a launch runs, at which shape — decided here and nowhere else (tsim_launch.h launches the plan).
// kernel: TS_K_*; policy: the closed loop; lpe: lanes per environment asked for by this launch (0: the batch's, TSIM_LPE /
// tsim_set_lanes_per_env); the precision is the batch's.  The view is the batch's (kernel_mode) — for the adjoint kernels only on a tape whose
// K the forward wrote (tape_k_ok: the fused adjoint reads it) — where it has an instantiation (ts_instantiated), else the generic kernels.
enum { TS_TAN_LDS_CAP = 64 * 1024 };      // dynamic LDS of a k_tangent block
// A launch whose every slot holds a block of reals behind the contexts (the tangent passes, the frame Jacobians).  shape_reals: the block the
// SHAPE is chosen for — where the contexts and the slots' blocks are over the cap, fewer environments share a wavefront.
// 0 is for a plan that ts_plan has shaped already (tangent_plan, frame_jacobian_plan): that plan's contexts fit the cap or its lanes are all 64, so
// the loop below leaves them and the grid comes out as ts_plan's.  own_reals: the block of this launch.  The plan's grid is that of the shape, its LDS the contexts' (ctx_lds: where the blocks begin) and the
// launch's own blocks behind them
struct SlotPlan { TsPlan plan; size_t ctx_lds; };
static SlotPlan slot_block_plan(const tsim_batch* b, TsPlan p, int shape_reals, int own_reals) {
  while (p.lpe < TS_WAVE && lds_bytes_for(b, TS_WAVE / p.lpe) + (TS_WAVE / p.lpe) * ((size_t)shape_reals * b->esz) > TS_TAN_LDS_CAP) p.lpe *= 2;
  const int ns = TS_WAVE / p.lpe;
  p.grid = (unsigned)((b->B + ns - 1) / ns);
  const size_t ctx_lds = lds_bytes_for(b, ns);
  p.lds = ctx_lds + (((size_t)ns * own_reals * b->esz + 15) / 16) * 16;
  return {p, ctx_lds};
}
static TsPlan ts_plan(const tsim_batch* b, int kernel, bool policy, int lpe) {
  int forced = lpe ? lpe : b->lpe_forced;
  if (kernel == TS_K_DEBUG_EVAL && !forced) forced = TS_WAVE;      // the debug kernel: one environment per wavefront unless a shape is forced
  const LaunchShape L = launch_shape(b, forced);
  TsPlan p;
  p.kernel = kernel; p.policy = policy; p.lpe = L.lpe; p.grid = L.grid; p.lds = L.lds;
  p.expj = b->has_exp; p.nrm = b->has_exp || b->nr > 8 ? 16 : 8;      // rows of the register solve (a rotation-vector joint: 16, at 64 lanes: launch_shape)
  const bool adjoint = kernel == TS_K_BACKWARD || kernel == TS_K_BACKWARD_Z || kernel == TS_K_CLOSED_BACKWARD_Z;
  p.variant = kernel == TS_K_PARAM_GRAD || kernel == TS_K_PARAM_GRAD_BODY || kernel == TS_K_TANGENT || kernel == TS_K_TANGENT_BODY || kernel == TS_K_CLOSED_TANGENT || kernel == TS_K_FRAME_JACOBIAN || kernel == TS_K_TACTILE_JACOBIAN || kernel == TS_K_PARAM_JACOBIAN || kernel == TS_K_TACTILE_NORMAL || (adjoint && !b->tape_k_ok) ? TS_KM_GENERIC : kernel_mode(b, forced);
  if (p.variant != TS_KM_GENERIC && !pusher_instantiated(b, kernel, policy, false, p.lpe)) p.variant = TS_KM_GENERIC;
  p.default_opts = p.variant != TS_KM_GENERIC && default_options(b) && pusher_instantiated(b, kernel, policy, true, p.lpe);
  p.fused = p.variant == TS_KM_STATIC ? ts_static_fused<TsStaticPusher, float>() : p.variant == TS_KM_PARAM && ts_static_fused<TsParamPusher, float>();
  if (kernel == TS_K_TANGENT || kernel == TS_K_CLOSED_TANGENT) {
    // the tangent pass (and its closed-loop twin, whose policy scratch is the contexts' own pair-staging records): every slot holds its tangent block behind the contexts (tsim_tangent.h).  The lanes are chosen for TSIM_TANGENT_MAX_DIR
    // directions with parameters, whatever the launch asks for — the shape must not depend on ndir or on which inputs are given —: where the
    // block's LDS does not hold that, fewer environments share a wavefront.  grid and lds are those of the contexts; launch_tangent adds the
    // launch's own tangent blocks
    return slot_block_plan(b, p, ts_tan_slot_reals(b->nr, b->nu, ts_pg_count(b->I[TSIM_IH_NPAIR], b->I[TSIM_IH_NSENSOR], b->nr), 4, TS_TAN_MAX_DIR), 0).plan;
  }
  // the frame Jacobians: every slot holds its 2 nr + nu columns behind the contexts (tsim_frame_jacobian.h), whichever outputs are asked for; where
  // the block's LDS does not hold that, fewer environments share a wavefront.  lds is the contexts'; frame_jacobian_plan adds the blocks,
  // launch_frame_jacobians multiplies the grid by the frames
  if (kernel == TS_K_FRAME_JACOBIAN) return slot_block_plan(b, p, ts_fj_slot_reals(b->nr, b->nu), 0).plan;
  // the tactile Jacobians likewise: every slot holds a pair's per-dof records behind the contexts (tsim_tactile_jacobian.h)
  if (kernel == TS_K_TACTILE_JACOBIAN) return slot_block_plan(b, p, ts_tj_slot_reals(b->nr), 0).plan;
  // the parameter Jacobians likewise: every slot holds TS_PJ_MAX_COLS columns behind the contexts (tsim_param_jacobian.h), whatever the launch selects
  if (kernel == TS_K_PARAM_JACOBIAN) return slot_block_plan(b, p, ts_pj_slot_reals(b->nr), 0).plan;
  // (the tactile normal equations, TS_K_TACTILE_NORMAL: the batch's shape here; their block depends on the call's with_params and on the taxels per
  // trip, so tactile_normal_plan widens the lanes and sizes the block)
  return p;
}
// the kernel arguments that come from the batch; each launch sets its own
template <class R> static FwdArgs<R> fwd_args(const tsim_batch* b) {
  FwdArgs<R> a{};
  a.I = b->dI; a.F = (const R*)b->dF; a.Fenv = (const R*)b->dFenv; a.fstride = b->nfrec; a.B = b->B; a.record = b->record; a.t0 = b->t_cur;
  a.tape = (R*)b->tape; a.evals = b->evals; a.prev = (double*)b->prev; a.has_prev = b->has_prev; a.stage_cpt = b->stage_cpt;
  a.cross_kinks = b->cross_kinks; a.eval_budget = b->eval_budget; a.gnorm = b->gnorm; a.cull = b->pair_cull; a.vo_ls = b->value_trials;
  a.default_opts = default_options(b) ? 1 : 0; a.tk = b->tape_k;
  return a;
}
template <class R> static BwdArgs<R> bwd_args(const tsim_batch* b) {
  BwdArgs<R> a{};
  a.I = b->dI; a.F = (const R*)b->dF; a.Fenv = (const R*)b->dFenv; a.fstride = b->nfrec; a.B = b->B; a.t_end = b->t_cur;
  a.tape = (const R*)b->tape; a.lamq = (R*)b->lamq; a.lamv = (R*)b->lamv; a.stage_cpt = b->stage_cpt; a.cull = b->pair_cull; a.tk = b->tape_k;
  return a;
}

// Pads too large for the in-kernel read-out (lanes of one environment over its taxels) are read on demand by tsim_readout; for those
// the forward launch leaves the pose records of its final state (k_forward, end of the launch).  Not under stream capture: a graph
// replay changes the state without the host seeing it, so a batch that was ever captured always recomputes the kinematics.
enum { TS_POSE_EMIT_MIN_TAXELS = 4096 };
static bool pose_emit(tsim_batch* b, hipStream_t st) {
  pose_invalidate(b, st);
  return !b->pose_off && b->nspt > 0 && b->poseR && b->ntax >= TS_POSE_EMIT_MIN_TAXELS;
}

// k_taxels over the pose records [frames][B][nspt]: frame f -> slot tac_slot[f] (device array; null: slot f) of tac_out.
// Taxels per block.  A block's prologue (staging the pose records and the model tables of its environment, two barriers)
// is a chain of dependent global loads, ~3 us whatever the slice; with many short blocks per SIMD slot the kernel WAS that prologue
// (8192 blocks of 5 taxels per thread: 4.6 rounds of ~7 us for 256 x 40 000 taxels).  So: ONE round — as many blocks as the device
// holds at once (occupancy x CUs), each with a slice long enough to cover the batch; never less than 256 taxels per block, so the
// single environment of test_sim_speed.py still spreads its 40 000 taxels over 157 blocks.
static bool taxels_supported(const tsim_batch* b) { return b->ntax > 0 && b->nspt > 0 && b->nspt <= TX_MAXK && b->I[TSIM_IH_NSENSOR] <= TX_MAXS; }
// the launch is k_taxels_small's: many records of a small pad
static bool taxels_small(const tsim_batch* b, long long nrec) {
  return nrec >= 4 * TXS_RPB && b->ntax <= TXS_MAX_TAXELS && b->nspt <= TXS_MAXK && b->I[TSIM_IH_NSENSOR] <= TXS_MAXS && !b->ab_taxels_per_record;
}
// sub: the environments the launch covers (k_taxels_small only; null: all of them)
template <class R>
static int launch_taxels(tsim_batch* b, const void* poseR, const double* poseD, int frames, const int32_t* tac_slot, void* tac_out, hipStream_t st, const TsSubRange* sub = nullptr) {
  if (b->tax_slots == 0) {
    int per_cu = 0;
    const hipError_t e_ = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_taxels<R>, 256, 0);
    b->tax_slots = (e_ == hipSuccess && per_cu > 0 ? per_cu : 4) * (b->n_simd / 4);
  }
  const TsSubRange all{nullptr, 0, b->B};
  const long long nrec = (long long)frames * (sub ? sub->n : b->B);
  if (taxels_small(b, nrec)) {
    TaxArgs<R> t{b->dI, (const R*)b->dF, (const R*)b->dFenv, b->nfrec, (const R*)poseR, poseD, b->nspt, (R*)tac_out, 0, b->B, tac_slot,
                 b->ntax, b->I[TSIM_IH_NSENSOR], b->I[TSIM_IH_FOFF_SENSOR], b->I[TSIM_IH_FOFF_PAIR], b->I[TSIM_IH_FOFF_TAXEL], b->tt_off};
    hipLaunchKernelGGL(k_taxels_small<R>, dim3((unsigned)((nrec + TXS_RPB - 1) / TXS_RPB)), dim3(256), 0, st, t, (int)nrec, sub ? *sub : all);
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (sub) return fail("launch_taxels: a sub-range of the environments is k_taxels_small's");
  const int per_env = (int)std::max<long long>(1, std::min<long long>(b->tax_slots / nrec, (b->ntax + 255) / 256));
  const int slice = ((b->ntax + per_env - 1) / per_env + 255) / 256 * 256;
  const dim3 tgrid((unsigned)nrec, (b->ntax + slice - 1) / slice);
  TaxArgs<R> t{b->dI, (const R*)b->dF, (const R*)b->dFenv, b->nfrec, (const R*)poseR, poseD, b->nspt, (R*)tac_out, slice, b->B, tac_slot,
               b->ntax, b->I[TSIM_IH_NSENSOR], b->I[TSIM_IH_FOFF_SENSOR], b->I[TSIM_IH_FOFF_PAIR], b->I[TSIM_IH_FOFF_TAXEL], b->tt_off};
  hipLaunchKernelGGL(k_taxels<R>, tgrid, dim3(256), 0, st, t);
  HIPCHK(hipGetLastError());
  return 0;
}

template <class R>
static int launch_forward(tsim_batch* b, const void* u, int nframes, const int32_t* tac_slot, int nsub, void* q_out, void* qd_out, void* var_out, void* tac_out, int32_t* status, hipStream_t st) {
  FwdArgs<R> a = fwd_args<R>(b);
  a.nsub = nsub; a.nframes = nframes; a.tac_slot = tac_slot; a.u = (const R*)u;
  a.q_out = (R*)q_out; a.qd_out = (R*)qd_out; a.var_out = (R*)var_out; a.tac_out = (R*)tac_out; a.status = status;
  a.order = (b->B >= 256 && nframes == 1 && b->order_valid) ? (const int*)b->order : (b->B >= 256 && nframes > 1 && b->order_ep_n == nframes * nsub && !b->ab_no_episode_lpt) ? (const int*)b->order_ep : nullptr;
  a.vo_first = b->value_first; a.helpers = b->trial_helpers; a.helped = b->helped;
  a.pred_helpers = b->trial_helpers && b->pred_helpers;      // (only where the trial helpers are; the kernel: only in free-running launches that record a tape, k_forward)
  const bool emit = pose_emit(b, st);
  a.nspt = b->nspt;
  if (emit) { a.poseR = (R*)b->poseR; a.poseD = b->poseD; }
  // The tactile frames of the launch: by k_taxels afterwards, from the pose records the launch leaves per frame — which is what lets the
  // slots of a wavefront run their frames independently (k_forward, main loop).  TSIM_INKERNEL_READOUT=1 / TSIM_NO_FREE_RUN=1: A/B.
  // (not when the per-frame pose records would take more than 1 GiB — 180-frame grasp episodes with 22 (sensor, primitive) combinations —: those
  // launches keep the in-kernel read-out)
  const size_t fpose_bytes = (size_t)nframes * b->B * (size_t)std::max(b->nspt, 1) * (TP_R_SIZE * b->esz + TP_D_SIZE * sizeof(double));
  bool defer = tac_out && taxels_supported(b) && fpose_bytes <= ((size_t)1 << 30) && !b->ab_inkernel_readout;
  if (defer && b->fpose_frames < nframes) {
    if (capturing(st)) defer = false;      // no allocation inside a capture: the in-kernel read-out
    else {
      // (a graph captured from ANY launch of this batch, pose_off, may name the old records)
      const size_t nrec = (size_t)nframes * b->B * b->nspt;
      const int rc = grow_buffers(b, st, b->pose_off != 0, {{b->fposeR, nrec * TP_R_SIZE * b->esz}, {b->fposeD, nrec * TP_D_SIZE * sizeof(double)}});
      if (rc > 0) return rc;
      b->fpose_frames = rc ? 0 : nframes;
      if (rc) defer = false;      // no memory for them: the in-kernel read-out
    }
  }
  if (defer) { a.fposeR = (R*)b->fposeR; a.fposeD = b->fposeD; }
  a.free_run = (defer || !tac_out || b->ntax == 0) && !b->ab_no_free_run;
  a.lockstep = b->ab_lockstep ? 1 : 0;
  if (a.lockstep) a.free_run = 0;
  TsPlan plan = ts_plan(b, TS_K_FORWARD, false, 0);
  if (b->record && !plan.fused) b->tape_k_ok = 0;      // records without K from here on
  // Episode launches of a fused compiled-in model that record a tape, run free and defer the tactile read-out end no frame inside k_forward: a frame's
  // final state is on the tape, and k_frame_records writes q, qd, the variables and the frame's pose records from it afterwards, on every SIMD, instead
  // of the launch's slowest wavefront doing it once per slot and frame (k_forward, end of a frame).  The same bits (ts_frame_outputs).  With every
  // option at its default the forward kernel is k_forward_fr, which has the switch as a constant (TsFrameRecords<>, tsim_static.h: k_forward 2.95 -> 2.57 ms
  // per 20-step launch, against 2.71 ms with the run-time switch; the pass itself 0.07 ms; profiles/r14_frame_records.md).
  // TSIM_INKERNEL_FRAME_OUT=1 at creation keeps the in-kernel frame end: A/B, and what tests/test_gpu_frame_records.py compares with.
  const TsPlan fr_plan = ts_plan(b, TS_K_FRAME_RECORDS, false, 0);
  // (not in a launch that leaves the pose records of its FINAL state, `emit`: those are taken from the link records the last frame end left in LDS)
  const bool frame_rec = defer && a.free_run && b->record && nframes > 1 && plan.fused && !emit && !b->ab_inkernel_frame_out &&
                         fr_plan.variant == plan.variant && fr_plan.lpe == plan.lpe;
  a.frame_rec = frame_rec ? 1 : 0;
  plan.frame_rec = frame_rec;
  b->last_frame_rec = !frame_rec ? 0 : (plan.frame_rec && plan.default_opts) ? 2 : 1;
  // k_frame_records over the environments of sub, on stream s — about one block per SIMD: the blocks of a chunk cover the environments, the chunks the frames
  const int ns_ = TS_WAVE / plan.lpe;
  auto frame_records = [&](hipStream_t s, const TsSubRange& sub) {
    TsPlan p = fr_plan;
    const int nblk = (sub.n + ns_ - 1) / ns_, chunks = std::max(1, std::min(nframes, b->n_simd / std::max(nblk, 1))), fpc = (nframes + chunks - 1) / chunks;
    p.grid = (unsigned)(nblk * ((nframes + fpc - 1) / fpc));
    return ts_launch<false, R>(p, s, a, fpc, sub);
  };
  // The launch split by LPT rank.  Every wavefront of such a launch is resident at once, one per SIMD, and the launch lasts as long as its heaviest
  // environment's chain of evaluations — while most SIMDs have run out of work long before (profiles/r27_forward_split.md).  The read-out side needs
  // only the tape records of the environments it reads, so the launch goes out as two: the wavefronts [0, wh) — under the episode order's deal wavefront
  // w holds the w-th heaviest environment (k_order_by_evals) — on the caller's stream, the others on the batch's side stream, each followed by the
  // read-out of ITS environments; the light group's read-out then runs on the SIMDs its forward kernel has left, under the heavy group's tail.  The
  // same kernels on the same inputs, environment by environment: the same bits.  The caller's stream waits for the side stream before anything else
  // is put on it (the next order is computed from both groups' evaluation counts), so the caller sees one stream as ever.
  // Not inside a capture (no parallel branches in a captured graph), nor without the episode order, nor where the wavefronts are not all resident.
  const int nblk_f = (int)plan.grid, wh = std::max(1, nblk_f / 8);
  const bool split = frame_rec && b->split_st && a.order && a.order == (const int*)b->order_ep && b->B % ns_ == 0 && nblk_f <= b->n_simd && nblk_f >= 64 &&
                     taxels_small(b, (long long)nframes * wh * ns_) && !capturing(st);
  b->last_fwd_split = split ? 1 : 0;
  if (split) {
    const TsSubRange heavy{a.order, 0, wh * ns_}, light{a.order, wh * ns_, b->B - wh * ns_};
    auto forward = [&](hipStream_t s, unsigned grid, const FwdArgs<R>& fa) -> int {
      TsPlan p = plan; p.grid = grid;
      if (!ts_launch<false, R>(p, s, fa)) return fail("no k_forward instantiation for the launch plan");
      HIPCHK(hipGetLastError());
      return 0;
    };
    auto read_out = [&](hipStream_t s, const TsSubRange& sub) -> int {      // one group's frames, on the stream of its forward kernel
      if (!frame_records(s, sub)) return fail("no k_frame_records instantiation for the launch plan");
      HIPCHK(hipGetLastError());
      return launch_taxels<R>(b, b->fposeR, b->fposeD, nframes, tac_slot, tac_out, s, &sub);
    };
    int rc;
    {
      KtScope kt_(b, TSIM_KT_FORWARD, st);
      HIPCHK(hipEventRecord(b->split_fork, st));      // (nothing is on the side stream yet: the fork may leave directly)
      HIPCHK(hipStreamWaitEvent(b->split_st, b->split_fork, 0));
      rc = forward(st, (unsigned)wh, a);
    }
    // From the side stream's first launch on the join is never skipped: whatever fails below, the caller's stream waits for what did get onto the
    // side stream before the error is returned
    if (!rc) {
      FwdArgs<R> al = a; al.order = a.order + light.e0;      // (a.B stays the stride of the tape and of the outputs)
      rc = forward(b->split_st, (unsigned)(nblk_f - wh), al);
    }
    if (!rc) rc = read_out(b->split_st, light);
    const hipError_t e_rec = hipEventRecord(b->split_join, b->split_st);
    hipError_t e_wait;
    {
      KtScope kt_(b, TSIM_KT_TAXELS, st);
      if (!rc) rc = read_out(st, heavy);
      e_wait = e_rec == hipSuccess ? hipStreamWaitEvent(st, b->split_join, 0) : hipStreamSynchronize(b->split_st);
    }
    if (rc) return rc;
    HIPCHK(e_rec);
    HIPCHK(e_wait);
  } else {
    { KtScope kt_(b, TSIM_KT_FORWARD, st); if (!ts_launch<false, R>(plan, st, a)) return fail("no k_forward instantiation for the launch plan"); }
    HIPCHK(hipGetLastError());
    if (defer) {
      KtScope kt_(b, TSIM_KT_TAXELS, st);
      if (frame_rec) {
        if (!frame_records(st, TsSubRange{nullptr, 0, b->B})) return fail("no k_frame_records instantiation for the launch plan");
        HIPCHK(hipGetLastError());
      }
      if (launch_taxels<R>(b, b->fposeR, b->fposeD, nframes, tac_slot, tac_out, st)) return 1;
    }
  }
  b->pose_valid = emit ? 1 : 0;
  if (b->B >= 256) {
    const int ns = TS_WAVE / plan.lpe, nsv = (b->B % ns == 0) ? ns : 1;
    if (nframes > 1) {          // episode totals: the order of the next episode launch of this length (kept across resets)
      const int n = nframes * nsub;
      hipLaunchKernelGGL(k_order_by_evals, dim3(1), dim3(1024), 0, st, (const int*)b->evals, b->order_ep, b->B, nsv, 2 * n, std::max(1, 5 * n / 2), b->ab_lpt_deal);
      b->order_ep_n = n; b->order_valid = 0;
    } else {
      hipLaunchKernelGGL(k_order_by_evals, dim3(1), dim3(1024), 0, st, (const int*)b->evals, b->order, b->B, nsv, 0, 64, b->ab_lpt_deal);
      b->order_valid = 1;
    }
    HIPCHK(hipGetLastError());
  } else if (nframes > 1) b->order_valid = 0;
  return 0;
}

// The parameter passes' slots.  Chunks of sub-steps per environment: enough (environment, chunk) slots for about four wavefronts per SIMD at four
// environments per wavefront, at most one chunk per sub-step (most), then chunks of equal length and none of them empty (nchunk x chunk_len).
// most is a function of the batch alone for n = the tape's capacity, so that the partial-sum buffers are sized once (pg_alloc).
struct PgLayout { int nchunk, chunk_len, most; };
static PgLayout pg_layout(const tsim_batch* b, int n) {
  const int want = (int)std::max<long long>(1, (16LL * b->n_simd + b->B - 1) / b->B);
  const int most = std::max(1, std::min(n, want)), chunk_len = (n + most - 1) / most;
  return {(n + chunk_len - 1) / chunk_len, chunk_len, most};
}
// what every pass over (environment, chunk of sub-steps) slots takes from the batch: its view of the model, the window of n sub-steps that ends
// at the tape's newest record, and the chunk layout
template <class R> static void pg_common(const tsim_batch* b, PgCommon<R>& p, int n, int nchunk, int chunk_len) {
  p.I = b->dI; p.F = (const R*)b->dF; p.Fenv = (const R*)b->dFenv; p.fstride = b->nfrec; p.B = b->B; p.n = n; p.t_end = b->t_cur;
  p.tape = (const R*)b->tape; p.nchunk = nchunk; p.chunk_len = chunk_len; p.stage_cpt = b->stage_cpt; p.tk = b->tape_k;
}
// A parameter pass of an adjoint launch (tsim_set_param_grad): the pass's kernel (TsLaunch::run picks it by the type of p, whose own fields the
// caller has set) over the sub-steps the launch just undid, then the fixed-order reduction of its partial sums into the caller's buffer
template <class R, class Args>
static int launch_param_pass(tsim_batch* b, TsKernel kernel, const char* name, const char* no_part, Args& p, int n, void* part, const PgSeg (&seg)[3], hipStream_t st) {
  const PgLayout lay = pg_layout(b, n);
  pg_common<R>(b, p, n, lay.nchunk, lay.chunk_len);
  p.z = (const R*)b->zbuf; p.P = seg[0].count + seg[1].count + seg[2].count; p.part = (R*)part;
  if (!part || p.nchunk > b->pg_chunks) return fail(no_part);
  TsPlan plan = ts_plan(b, kernel, false, 0);
  plan.grid *= p.nchunk;
  if (!TsLaunch<void, false, R>::run(plan, st, p)) return fail(std::string("no ") + name + " instantiation for the launch plan");
  HIPCHK(hipGetLastError());
  ts_param_reduce_launch(PgReduceArgs<R>{(const R*)part, p.nchunk, b->B, p.P, (R*)b->dLdp, b->nfrec, {seg[0], seg[1], seg[2]}}, st);
  HIPCHK(hipGetLastError());
  return 0;
}
// the contact groups: [pair kn kt mu kd], [sensor kn kt mu kd], [dof damping] (ts_pg_count)
template <class R>
static int launch_param_grad(tsim_batch* b, int n, int seed_stride, int frames, const int32_t* tac_slot, const void* df_dtac, hipStream_t st) {
  PgArgs<R> p;
  p.seed_stride = seed_stride; p.frames = frames; p.tac_slot = tac_slot; p.df_dtac = (const R*)df_dtac;
  const PgSeg seg[3] = {{4 * b->I[TSIM_IH_NPAIR], 4, TSIM_PF_SIZE, b->I[TSIM_IH_FOFF_PAIR] + TSIM_PF_KN, 1},
                        {4 * b->I[TSIM_IH_NSENSOR], 4, TSIM_SF_SIZE, b->I[TSIM_IH_FOFF_SENSOR] + TSIM_SF_KN, 1},
                        {b->nr, 1, TSIM_DF_SIZE, b->I[TSIM_IH_FOFF_DOF] + TSIM_DF_DAMPING, 1}};
  return launch_param_pass<R>(b, TS_K_PARAM_GRAD, "k_param_grad", "param_grad: partial-sum buffer too small", p, n, b->pgpart, seg, st);
}
// ... and the body groups (tsim_set_param_grad_groups): [link mass com inertia], [motor lo hi P D], [dof lim_lo lim_hi lim_k] (ts_pgb_count);
// only the groups that are on are evaluated and added
template <class R>
static int launch_param_grad_body(tsim_batch* b, int n, hipStream_t st) {
  PgBodyArgs<R> p;
  p.groups = b->pg_groups;
  const PgSeg seg[3] = {{10 * b->I[TSIM_IH_NL], 10, TSIM_LF_SIZE, b->I[TSIM_IH_FOFF_LINK] + TSIM_LF_MASS, b->pg_groups & TS_PG_INERTIAL},
                        {4 * b->nu, 4, 4, b->I[TSIM_IH_FOFF_MOTOR], b->pg_groups & TS_PG_MOTOR},      // TSIM_MF_SIZE = 4: lo hi P D
                        {3 * b->nr, 3, TSIM_DF_SIZE, b->I[TSIM_IH_FOFF_DOF] + TSIM_DF_LIM_LO, b->pg_groups & TS_PG_LIMIT}};
  return launch_param_pass<R>(b, TS_K_PARAM_GRAD_BODY, "k_param_grad_body", "param_grad: the body groups' partial-sum buffer is missing or too small", p, n,
                              b->pgbpart, seg, st);
}

// The passes behind an adjoint launch that saved z (b->dLdp set; nothing otherwise): the contact pass with the launch's seed layout, then the body
// groups' pass, each only where its groups are on
template <class R>
static int launch_param_passes(tsim_batch* b, int n, int seed_stride, int frames, const int32_t* tac_slot, const void* df_dtac, hipStream_t st) {
  b->adj_passes = 0;
  if (!b->dLdp) return 0;
  if (b->pg_groups & TS_PG_CONTACT) {
    if (launch_param_grad<R>(b, n, seed_stride, frames, tac_slot, df_dtac, st)) return 1;
    b->adj_passes |= 1;
  }
  if (b->pg_groups & ~TS_PG_CONTACT) {
    if (launch_param_grad_body<R>(b, n, st)) return 1;
    b->adj_passes |= 2;
  }
  return 0;
}

template <class R>
static int launch_backward(tsim_batch* b, int n, int seed_stride, int frames, const int32_t* tac_slot, const void* df_dq, const void* df_dvar, const void* df_dtac, void* df_du, hipStream_t st) {
  BwdArgs<R> a = bwd_args<R>(b);
  a.n = n; a.seed_stride = seed_stride; a.frames = frames; a.tac_slot = tac_slot;
  a.df_dq = (const R*)df_dq; a.df_dvar = (const R*)df_dvar; a.df_dtac = (const R*)df_dtac; a.df_du = (R*)df_du; a.cyc = b->bwd_stamps;
  {
    KtScope kt_(b, TSIM_KT_BACKWARD, st);
    // with the parameter pass: the same variant's SAVEZ twin (z of every sub-step).  TSIM_BWD_LPE at creation (A/B): another launch shape for
    // the adjoint kernel (the tape does not depend on it)
    const TsPlan plan = ts_plan(b, b->dLdp ? TS_K_BACKWARD_Z : TS_K_BACKWARD, false, b->ab_bwd_lpe);
    // An episode launch of a fused compiled-in view (fp32, 16 lanes, BDF1; no parameter gradient): the frames' seed partials by k_adjoint_seeds, then
    // k_backward_pre, which reads them (tsim_adjoint_pre.h) — both on this stream and inside this timing scope: k_backward's time stays the whole adjoint side
    b->adj_pre_ran = 0;
    if constexpr (std::is_same<R, float>::value) {
      if (b->adj_pre && b->sseed && frames == 1 && !b->dLdp && plan.fused && plan.lpe == 16 && b->I[TSIM_IH_INTEGRATOR] != 2 &&
          ts_adjoint_pre_launch(plan, st, a, (float*)b->sseed, b->nfrec)) b->adj_pre_ran = 1;
    }
    if (!b->adj_pre_ran && !ts_launch<false, R>(plan, st, a, (R*)b->zbuf)) return fail("no k_backward instantiation for the launch plan");
  }
  HIPCHK(hipGetLastError());
  b->adj_kernel = b->dLdp ? TSIM_ADJ_BACKWARD_Z : TSIM_ADJ_BACKWARD;
  return launch_param_passes<R>(b, n, seed_stride, frames, tac_slot, df_dtac, st);
}

// The tangent pass over the newest T x S taped sub-steps (tsim_tangent_episode): one launch of the generic k_tangent, whatever the batch's view (a
// compiled-in model's tape has K in its records: a.tk), on the batch's per-environment rows.  Reads the tape, writes the caller's buffers.
// With a body group on (tsim_set_param_grad_groups) and dtables given, k_tangent_body_src runs first, into the batch's workspace (launch_tangent).
// the plan of a tangent launch of ndir directions: ts_plan's shape, its LDS grown by the launch's own tangent blocks (ctx_lds: the contexts' part,
// where the blocks begin).  launch_tangent and tsim_tangent_launch_info both take it from here
static SlotPlan tangent_plan(const tsim_batch* b, int ndir, bool with_dtab, int kernel = TS_K_TANGENT) {
  const int nhist = b->I[TSIM_IH_INTEGRATOR] == 2 ? 4 : 2, P = with_dtab ? ts_pg_count(b->I[TSIM_IH_NPAIR], b->I[TSIM_IH_NSENSOR], b->nr) : 0;
  return slot_block_plan(b, ts_plan(b, kernel, false, 0), 0, ts_tan_slot_reals(b->nr, b->nu, P, nhist, ndir));
}
// what a tangent launch takes from the batch and the caller (launch_tangent, and the closed-loop launch in tsim_env_push.h)
template <class R>
static void tangent_args(const tsim_batch* b, TanArgs<R>& a, int T, int S, int ndir, const int32_t* tac_slot, const void* du, const void* dq0, const void* dqd0, const void* dtab,
                         void* dq_out, void* dqd_out, void* dvar_out, void* dtac_out) {
  a.I = b->dI; a.F = (const R*)b->dF; a.Fenv = (const R*)b->dFenv; a.fstride = b->nfrec;
  a.B = b->B; a.n = T * S; a.t_end = b->t_cur; a.nsub = S; a.nframes = T; a.ndir = ndir; a.tk = b->tape_k;
  a.stage_cpt = b->stage_cpt; a.cull = b->pair_cull; a.tac_slot = tac_slot; a.tape = (const R*)b->tape;
  a.du = (const R*)du; a.dq0 = (const R*)dq0; a.dqd0 = (const R*)dqd0; a.dtab = (const R*)dtab;
  a.dq_out = (R*)dq_out; a.dqd_out = (R*)dqd_out; a.dvar_out = (R*)dvar_out; a.dtac_out = (R*)dtac_out;
}
// The body-group columns of dtables (a body group on in tsim_set_param_grad_groups): their part of every sub-step's source by k_tangent_body_src,
// over the parameter passes' slots (pg_layout) at the batch's lanes, into the batch's workspace — on this stream, before the tangent kernel, which
// adds it (a.src is set).  Nothing to do without dtables or with the contact group alone.  who: the entry point, for the messages
template <class R>
static int launch_tangent_body_src(tsim_batch* b, TanArgs<R>& a, hipStream_t st, const char* who) {
  if (!a.dtab || !(b->pg_groups & ~TS_PG_CONTACT)) return 0;
  const int ndir = a.ndir;
  const size_t need = (size_t)ndir * a.n * b->B * b->nr;
  const bool cap = capturing(st);
  if (need > b->tan_src_reals) {      // the one allocation of a tangent call: the first that needs the workspace, or needs it larger
    if (cap)
      return fail(std::string(who) + ": the body columns' workspace must grow, which a stream capture cannot do: call once with these sizes before capturing");
    // (a graph captured from a launch below names the workspace in the arguments of k_tangent_body_src and the tangent kernel: tan_src_captured)
    const int rc = grow_buffers(b, st, b->tan_src_captured != 0, {{b->tan_src, need * b->esz}});
    if (rc > 0) return rc;
    b->tan_src_captured = 0;
    b->tan_src_reals = rc ? 0 : need;
    if (rc) return fail(std::string(who) + ": hipMalloc of the body columns' workspace failed");
  }
  const PgLayout lay = pg_layout(b, a.n);
  TanBodyArgs<R> p{};
  pg_common<R>(b, p, a.n, lay.nchunk, lay.chunk_len);
  p.groups = b->pg_groups; p.ndir = ndir; p.dtab = a.dtab; p.src = (R*)b->tan_src;
  if (cap) b->tan_src_captured = 1;      // a graph now names this workspace
  TsPlan bp = ts_plan(b, TS_K_TANGENT_BODY, false, 0);
  bp.grid *= p.nchunk;
  if (!TsLaunch<void, false, R>::run(bp, st, p)) return fail("no k_tangent_body_src instantiation for the launch plan");
  HIPCHK(hipGetLastError());
  a.src = (const R*)b->tan_src;
  return 0;
}
template <class R>
static int launch_tangent(tsim_batch* b, int T, int S, int ndir, const int32_t* tac_slot, const void* du, const void* dq0, const void* dqd0, const void* dtab,
                          void* dq_out, void* dqd_out, void* dvar_out, void* dtac_out, hipStream_t st) {
  TanArgs<R> a{};
  tangent_args<R>(b, a, T, S, ndir, tac_slot, du, dq0, dqd0, dtab, dq_out, dqd_out, dvar_out, dtac_out);
  const auto [plan, ctx_lds] = tangent_plan(b, ndir, dtab != nullptr);
  a.xoff = (int)(ctx_lds / b->esz);
  if (plan.lds > TS_TAN_LDS_CAP) return fail("tangent_episode: the tangent state of " + std::to_string(ndir) + " directions does not fit the block's LDS for this model");
  if (int rc = launch_tangent_body_src<R>(b, a, st, "tangent_episode")) return rc;
  if (!(a.src ? TsLaunch<void, false, R>::run_tangent_src(plan, st, a) : TsLaunch<void, false, R>::run(plan, st, a))) return fail("no k_tangent instantiation for the launch plan");
  HIPCHK(hipGetLastError());
  return 0;
}

// The per-frame transition Jacobians over the newest T x S taped sub-steps (tsim_frame_jacobians): one launch of the generic k_frame_jacobian,
// T x ceil(B / NS) blocks, whatever the batch's view, on the batch's per-environment rows.  Reads the tape, writes the caller's buffers.
// the plan: ts_plan's shape for ONE frame, its LDS grown by the slots' blocks (ctx_lds: the contexts' part, where the blocks begin)
static SlotPlan frame_jacobian_plan(const tsim_batch* b) { return slot_block_plan(b, ts_plan(b, TS_K_FRAME_JACOBIAN, false, 0), 0, ts_fj_slot_reals(b->nr, b->nu)); }
template <class R>
static int launch_frame_jacobians(tsim_batch* b, int T, int S, void* A_out, void* B_out, void* Jvar_out, hipStream_t st) {
  auto [plan, ctx_lds] = frame_jacobian_plan(b);
  if (plan.lds > TS_TAN_LDS_CAP) return fail("frame_jacobians: the " + std::to_string(ts_fj_ncol(b->nr, b->nu)) + " columns of an environment do not fit the block's LDS for this model");
  if ((unsigned long long)plan.grid * (unsigned)T > 0x7fffffffull) return fail("frame_jacobians: too many blocks");
  FjArgs<R> a{};
  pg_common<R>(b, a, T * S, T, S);      // a chunk is a frame
  a.cull = b->pair_cull; a.xoff = (int)(ctx_lds / b->esz);
  a.A_out = (R*)A_out; a.B_out = (R*)B_out; a.Jvar_out = (R*)Jvar_out;
  plan.grid *= (unsigned)T;
  if (!TsLaunch<void, false, R>::run(plan, st, a)) return fail("no k_frame_jacobian instantiation for the launch plan");
  HIPCHK(hipGetLastError());
  return 0;
}

// The per-frame tactile Jacobians of the masked frames of the newest T x S taped sub-steps (tsim_tactile_jacobians): one launch of the generic
// k_tactile_jacobian, T x ceil(B / NS) blocks (a block of a frame that is not masked returns at once), whatever the batch's view, on the batch's
// per-environment rows.  Reads the tape, writes the caller's buffer.  The plan: as frame_jacobian_plan
static SlotPlan tactile_jacobian_plan(const tsim_batch* b) { return slot_block_plan(b, ts_plan(b, TS_K_TACTILE_JACOBIAN, false, 0), 0, ts_tj_slot_reals(b->nr)); }
template <class R>
static int launch_tactile_jacobians(tsim_batch* b, int T, int S, const int32_t* tac_slot, void* Ct_out, hipStream_t st) {
  auto [plan, ctx_lds] = tactile_jacobian_plan(b);
  if (plan.lds > TS_TAN_LDS_CAP) return fail("tactile_jacobians: a pair's per-dof records do not fit the block's LDS next to the context for this model");
  if ((unsigned long long)plan.grid * (unsigned)T > 0x7fffffffull) return fail("tactile_jacobians: too many blocks");
  TjArgs<R> a{};
  pg_common<R>(b, a, T * S, T, S);      // a chunk is a frame
  a.cull = b->pair_cull; a.xoff = (int)(ctx_lds / b->esz);
  a.tac_slot = tac_slot; a.Ct_out = (R*)Ct_out;
  plan.grid *= (unsigned)T;
  if (!TsLaunch<void, false, R>::run(plan, st, a)) return fail("no k_tactile_jacobian instantiation for the launch plan");
  HIPCHK(hipGetLastError());
  return 0;
}

// The tactile normal equations of the masked frames of the newest T x S taped sub-steps (tsim_tactile_normal_equations): one launch of the generic
// k_tactile_normal, T x ceil(B / NS) blocks (a block of a frame that is not masked returns at once), whatever the batch's view, on the batch's
// per-environment rows.  Reads the tape, writes the caller's buffers.  The plan: the batch's shape; the lanes double while the contexts, the slots'
// blocks (tsim_tactile_normal.h, a tile row per lane) and the entry table are over the cap; at 64 lanes the taxels per trip halve instead, down
// to TS_TN_MIN_ROWS.  It depends on with_params and on nothing else of the call
struct TnPlan { TsPlan plan; size_t ctx_lds, toff; int rows; };
static TnPlan tactile_normal_plan(const tsim_batch* b, int with_params) {
  TsPlan p = ts_plan(b, TS_K_TACTILE_NORMAL, false, 0);
  const int wp = with_params ? 1 : 0;
  auto blocks = [&](int lpe, int rows) { return (((size_t)(TS_WAVE / lpe) * ts_tn_slot_reals(b->nr, wp, rows) * b->esz + 15) / 16) * 16; };
  auto bytes = [&](int lpe, int rows) { return lds_bytes_for(b, TS_WAVE / lpe) + blocks(lpe, rows) + (size_t)ts_tn_table_bytes(b->nr, wp); };
  while (p.lpe < TS_WAVE && bytes(p.lpe, p.lpe) > TS_TAN_LDS_CAP) p.lpe *= 2;
  int rows = p.lpe;
  while (rows > TS_TN_MIN_ROWS && bytes(p.lpe, rows) > TS_TAN_LDS_CAP) rows /= 2;
  const int ns = TS_WAVE / p.lpe;
  p.grid = (unsigned)((b->B + ns - 1) / ns);
  const size_t ctx_lds = lds_bytes_for(b, ns);
  p.lds = bytes(p.lpe, rows);
  return {p, ctx_lds, ctx_lds + blocks(p.lpe, rows), rows};
}
template <class R>
static int launch_tactile_normal(tsim_batch* b, int T, int S, const int32_t* tac_slot, int with_params, const void* weight, const void* resid, void* N_out, void* n_out, hipStream_t st) {
  auto [plan, ctx_lds, toff, rows] = tactile_normal_plan(b, with_params);
  if (plan.lds > TS_TAN_LDS_CAP) return fail("tactile_normal_equations: a pair's per-dof records, the sums and a tile of " + std::to_string((int)TS_TN_MIN_ROWS) + " taxels do not fit the block's LDS next to the context for this model");
  if ((unsigned long long)plan.grid * (unsigned)T > 0x7fffffffull) return fail("tactile_normal_equations: too many blocks");
  TnArgs<R> a{};
  pg_common<R>(b, a, T * S, T, S);      // a chunk is a frame
  a.cull = b->pair_cull; a.xoff = (int)(ctx_lds / b->esz); a.toff = (int)toff; a.rows = rows; a.with_params = with_params ? 1 : 0;
  a.tac_slot = tac_slot; a.weight = (const R*)weight; a.resid = (const R*)resid; a.N_out = (R*)N_out; a.n_out = (R*)n_out;
  plan.grid *= (unsigned)T;
  if (!TsLaunch<void, false, R>::run(plan, st, a)) return fail("no k_tactile_normal instantiation for the launch plan");
  HIPCHK(hipGetLastError());
  return 0;
}

// The per-frame parameter Jacobians over the newest T x S taped sub-steps (tsim_param_jacobians): one launch of the generic k_param_jacobian,
// T x ceil(B / NS) blocks, whatever the batch's view, on the batch's per-environment rows.  Reads the tape, writes the caller's buffers.  The
// plan: as frame_jacobian_plan, the slot's block sized for TS_PJ_MAX_COLS columns whatever the launch selects
static SlotPlan param_jacobian_plan(const tsim_batch* b) { return slot_block_plan(b, ts_plan(b, TS_K_PARAM_JACOBIAN, false, 0), 0, ts_pj_slot_reals(b->nr)); }
// cidx: the selected columns as compact indices (ts_pg_count order), ncols of them (0 without E_out); they travel by value in the arguments
template <class R>
static int launch_param_jacobians(tsim_batch* b, int T, int S, int ncols, const int* cidx, const int32_t* tac_slot, void* E_out, void* Ft_out, hipStream_t st) {
  auto [plan, ctx_lds] = param_jacobian_plan(b);
  if (plan.lds > TS_TAN_LDS_CAP) return fail("param_jacobians: the " + std::to_string((int)TS_PJ_MAX_COLS) + " columns of an environment do not fit the block's LDS for this model");
  if ((unsigned long long)plan.grid * (unsigned)T > 0x7fffffffull) return fail("param_jacobians: too many blocks");
  PjArgs<R> a{};
  pg_common<R>(b, a, T * S, T, S);      // a chunk is a frame
  a.cull = b->pair_cull; a.xoff = (int)(ctx_lds / b->esz);
  a.ncols = ncols;
  for (int k = 0; k < ncols; ++k) a.col[k] = cidx[k];
  a.tac_slot = tac_slot; a.E_out = (R*)E_out; a.Ft_out = (R*)Ft_out;
  plan.grid *= (unsigned)T;
  if (!TsLaunch<void, false, R>::run(plan, st, a)) return fail("no k_param_jacobian instantiation for the launch plan");
  HIPCHK(hipGetLastError());
  return 0;
}

// The checks the episode entry points share; who: the entry point, in front of the message.
static int frames_positive(const std::string& who, int num_frames, int num_steps) {
  return num_frames <= 0 || num_steps <= 0 ? fail(who + ": num_frames and num_steps must be positive") : 0;
}
// the window of num_frames x num_steps sub-steps (*n) is on the tape: the newest ones
static int taped_window(const tsim_batch* b, const std::string& who, int num_frames, int num_steps, long long* n) {
  if (int rc = frames_positive(who, num_frames, num_steps)) return rc;
  *n = (long long)num_frames * num_steps;
  return *n > b->t_cur ? fail(who + ": only " + std::to_string(b->t_cur) + " sub-steps on the tape") : 0;
}
// the tangent passes carry nothing across calls: a BDF2 model's window is the whole tape
static int bdf2_window_is_the_tape(const tsim_batch* b, const std::string& who, long long n) {
  if (b->I[TSIM_IH_INTEGRATOR] != 2 || n == b->t_cur) return 0;
  return fail(who + ": a BDF2 model's window must start at tape record 0 (no tangent is carried across calls); the tape holds " + std::to_string(b->t_cur) + " sub-steps");
}

extern "C" {

const char* tsim_last_error(void) { return g_err.c_str(); }

int tsim_batch_create(const int32_t* I, const double* F, int B, int tape_capacity, int dtype, int device, tsim_batch** out) {
  if (!I || !F || !out) return fail("null argument");
  if (I[TSIM_IH_MAGIC] != TSIM_MAGIC || I[TSIM_IH_VERSION] != TSIM_VERSION) return fail("model blob: bad magic/version");
  if (B <= 0 || tape_capacity < 0) return fail("bad batch size / tape capacity");
  if (dtype != TSIM_F32 && dtype != TSIM_F64) return fail("bad dtype");
  if (I[TSIM_IH_INTEGRATOR] != 1 && I[TSIM_IH_INTEGRATOR] != 2) return fail("unknown integrator");
  const int nl = I[TSIM_IH_NL], nr = I[TSIM_IH_NR], nu = I[TSIM_IH_NU];
  int n_exp = 0;
  if (nr > 16 || nr < 1 || nu > 16) return fail("ndof_r must be in 1..16 and ndof_u <= 16");
  for (int i = 1; i <= nl; ++i) {
    int jt = I[I[TSIM_IH_OFF_LINK] + (i - 1) * TSIM_LI_SIZE + TSIM_LI_JTYPE];
    if (jt != TSIM_J_REVOLUTE && jt != TSIM_J_PRISMATIC && jt != TSIM_J_PLANAR && jt != TSIM_J_TRANSLATIONAL && jt != TSIM_J_SPHERICAL_EXP)
      return fail("joint type not supported by the HIP path");
    if (jt == TSIM_J_SPHERICAL_EXP && ++n_exp > 1) return fail("at most one rotation-vector joint per model on the HIP path");
  }
  for (int s = 0; s < I[TSIM_IH_NSENSOR]; ++s)
    if (I[I[TSIM_IH_OFF_SENSOR] + s * TSIM_SI_SIZE + TSIM_SI_NSPRIM] > 16) return fail("too many primitives per sensor");
  DeviceGuard guard_(device);
  if (!guard_.ok) return fail("hipSetDevice(" + std::to_string(device) + ") failed");
  tsim_batch* b = new tsim_batch();
  b->B = B; b->dtype = dtype; b->device = device; b->cap = tape_capacity;
  b->I.assign(I, I + I[TSIM_IH_NI]); b->F.assign(F, F + I[TSIM_IH_NF]);
  b->nl = nl; b->nr = nr; b->nu = nu; b->nvar = I[TSIM_IH_NVAR]; b->ntax = I[TSIM_IH_NTAXEL];
  b->esz = dtype == TSIM_F32 ? 4 : 8;
  b->t_cur = 0; b->record = 0; b->has_exp = n_exp > 0;
  b->nfrec = I[TSIM_IH_FOFF_CPT];
  b->lpe_forced = 0;
  { const std::vector<int32_t> S_ = build_sched(b->I, b->F); b->nsched = (int)S_.size(); b->tt_off = b->I[TSIM_IH_NI] + S_[TS_SCHED_TAXTAB]; }
  b->pair_cull = getenv("TSIM_NO_PAIR_CULL") ? 0 : 1;
  b->no_static = getenv("TSIM_NO_STATIC") != nullptr;
  b->trial_helpers = getenv("TSIM_NO_TRIAL_HELPERS") ? 0 : 1;
  b->pred_helpers = getenv("TSIM_NO_PREDICTOR_HELPERS") ? 0 : 1;
  b->ab_no_episode_lpt = getenv("TSIM_NO_EPISODE_LPT") != nullptr; b->ab_inkernel_readout = getenv("TSIM_INKERNEL_READOUT") != nullptr;
  b->ab_no_free_run = getenv("TSIM_NO_FREE_RUN") != nullptr; b->ab_lockstep = getenv("TSIM_LOCKSTEP") != nullptr; b->ab_no_default_opts = getenv("TSIM_NO_DEFAULT_OPTS") != nullptr;
  if (const char* e = getenv("TSIM_LPT_DEAL")) b->ab_lpt_deal = atoi(e);
  if (const char* e = getenv("TSIM_BWD_LPE")) { const int v = atoi(e); if (v == 16 || v == 32 || v == 64) b->ab_bwd_lpe = v; }
  b->ab_taxels_per_record = getenv("TSIM_TAXELS_PER_RECORD") != nullptr; b->ab_no_envtab_cpt = getenv("TSIM_NO_ENVTAB_CPT") != nullptr;
  b->value_first = getenv("TSIM_NO_VALUE_FIRST") ? 0 : 1;
  b->ab_inkernel_frame_out = getenv("TSIM_INKERNEL_FRAME_OUT") != nullptr;
  if (const char* e = getenv("TSIM_VALUE_TRIALS")) b->value_trials = std::max(0, atoi(e));
  if (const char* e = getenv("TSIM_LPE")) { const int v = atoi(e); if (v == 16 || v == 32 || v == 64) b->lpe_forced = v; }
  b->cross_kinks = dtype == TSIM_F32 ? 1 : 0;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    b->n_simd = 4 * cus;
  }
  b->stage_cpt = 0;
  detect_static_model(b);      // before the staging decision: the launch shape depends on which kernels run
  b->tape_k = kernel_mode(b, b->lpe_forced) != TS_KM_GENERIC ? 1 : 0;
  b->rec = ts_rec(nr, nu, (int)b->esz, b->tape_k);
  if (lds_bytes_for(b, 1) > 64 * 1024) { delete b; return fail("model needs more than 64 KiB of LDS per environment"); }
  decide_stage_cpt(b);
  b->nspt = b->I[TSIM_IH_NSPRIM];
  size_t tape_bytes = (size_t)(tape_capacity + 1) * B * b->rec * b->esz;
  if (hipMalloc(&b->dI, (b->I.size() + b->nsched) * sizeof(int32_t)) != hipSuccess || hipMalloc(&b->dF, b->F.size() * b->esz) != hipSuccess ||
      hipMalloc(&b->tape, tape_bytes) != hipSuccess || hipMalloc(&b->lamq, (size_t)2 * B * nr * b->esz) != hipSuccess ||
      hipMalloc(&b->lamv, (size_t)2 * B * nr * b->esz) != hipSuccess || hipMalloc(&b->evals, (size_t)B * sizeof(int)) != hipSuccess || hipMalloc((void**)&b->helped, (size_t)B * sizeof(int)) != hipSuccess || hipMemset(b->helped, 0, (size_t)B * sizeof(int)) != hipSuccess || hipMalloc((void**)&b->gnorm, (size_t)B * sizeof(float)) != hipSuccess || hipMalloc(&b->order, (size_t)B * sizeof(int)) != hipSuccess || hipMalloc((void**)&b->order_ep, (size_t)B * sizeof(int)) != hipSuccess || hipMalloc(&b->prev, (size_t)B * 2 * nr * sizeof(double)) != hipSuccess ||
      (b->nspt > 0 && (hipMalloc(&b->poseR, (size_t)B * b->nspt * TP_R_SIZE * b->esz) != hipSuccess || hipMalloc((void**)&b->poseD, (size_t)B * b->nspt * TP_D_SIZE * sizeof(double)) != hipSuccess))) {
    tsim_batch_destroy(b);
    return fail("hipMalloc failed (tape bytes = " + std::to_string(tape_bytes) + ")");
  }
  if (hipMemset(b->tape, 0, tape_bytes) != hipSuccess || hipMemset(b->lamq, 0, (size_t)2 * B * nr * b->esz) != hipSuccess ||
      hipMemset(b->lamv, 0, (size_t)2 * B * nr * b->esz) != hipSuccess) { tsim_batch_destroy(b); return fail("hipMemset failed"); }
  if (upload_model(b, nullptr)) { tsim_batch_destroy(b); return 1; }
  // the seed pre-pass's buffer [cap][B][2 nr] (tsim_adjoint_pre.h), for a batch that can take the path: here, never at launch.  A failed allocation
  // is no error: the batch keeps the in-kernel path (TSIM_OPT_ADJOINT_PREPASS reads 0)
  b->adj_pre = getenv("TSIM_NO_ADJOINT_PREPASS") ? 0 : 1;
  if (b->adj_pre && b->tape_k && dtype == TSIM_F32 && tape_capacity > 0 && hipMalloc(&b->sseed, (size_t)tape_capacity * B * 2 * nr * b->esz) != hipSuccess) {
    (void)hipGetLastError();
    b->adj_pre = 0;
  }
  // the side stream of the split forward launch (launch_forward; a split has 64 blocks or more).  Non-blocking: it is ordered against the caller's
  // stream by its two events alone — the caller's may be the null stream, which every blocking stream waits for
  if (B >= 64 && !getenv("TSIM_NO_FORWARD_SPLIT")) {
    if (hipStreamCreateWithFlags(&b->split_st, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&b->split_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&b->split_join, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      split_release(b);
    }
  }
  *out = b;
  return 0;
}

void tsim_batch_destroy(tsim_batch* b) {
  if (!b) return;
  DeviceGuard guard_(b->device);
  for (auto& e : b->cache) (void)hipFree(e.buf);
  for (void* p : b->pool) (void)hipFree(p);
  for (void* p : b->retired) (void)hipFree(p);
  for (auto& k : b->kt) { (void)hipEventDestroy(k.a); (void)hipEventDestroy(k.b); }
  for (hipEvent_t e : b->kt_free) (void)hipEventDestroy(e);
  split_release(b);
  (void)hipFree(b->tape);
  delete b;      // the buffers the batch owns (DevBuf) go with it, on the batch's device: guard_ is still in scope
}

int tsim_ndof_r(const tsim_batch* b) { return b->nr; }
int tsim_ndof_u(const tsim_batch* b) { return b->nu; }
int tsim_ndof_var(const tsim_batch* b) { return 3 * b->nvar; }
int tsim_ndof_tactile(const tsim_batch* b) { return 3 * b->ntax; }
int tsim_batch_size(const tsim_batch* b) { return b->B; }
int tsim_dtype(const tsim_batch* b) { return b->dtype; }
double tsim_timestep(const tsim_batch* b) { return b->F[TSIM_FH_H]; }
int tsim_tape_len(const tsim_batch* b) { return b->record ? b->t_cur : 0; }
int tsim_launch_info(const tsim_batch* b, int32_t* out) { return plan_info(ts_plan(b, TS_K_FORWARD, false, 0), out); }      // (launch_shape at the batch's lanes)
int tsim_tangent_launch_info(const tsim_batch* b, int ndir, int with_dtables, int32_t* out) {
  if (!b || !out) return fail("tangent_launch_info: null argument");
  if (ndir < 1 || ndir > TSIM_TANGENT_MAX_DIR) return fail("tangent_launch_info: ndir must be 1 .. " + std::to_string((int)TSIM_TANGENT_MAX_DIR));
  return plan_info(tangent_plan(b, ndir, with_dtables != 0).plan, out);
}
int tsim_frame_jacobians_launch_info(const tsim_batch* b, int32_t* out) {
  if (!b || !out) return fail("frame_jacobians_launch_info: null argument");
  return plan_info(frame_jacobian_plan(b).plan, out);
}
int tsim_tactile_jacobians_launch_info(const tsim_batch* b, int32_t* out) {
  if (!b || !out) return fail("tactile_jacobians_launch_info: null argument");
  return plan_info(tactile_jacobian_plan(b).plan, out);
}
int tsim_param_jacobians_launch_info(const tsim_batch* b, int32_t* out) {
  if (!b || !out) return fail("param_jacobians_launch_info: null argument");
  return plan_info(param_jacobian_plan(b).plan, out);
}
int tsim_tactile_normal_equations_launch_info(const tsim_batch* b, int with_params, int32_t* out) {
  if (!b || !out) return fail("tactile_normal_equations_launch_info: null argument");
  return plan_info(tactile_normal_plan(b, with_params).plan, out);
}
int tsim_kernel_timing(tsim_batch* b, int enable) { b->kt_on = enable ? 1 : 0; return 0; }
int tsim_kernel_times(tsim_batch* b, double* ms_sum, int32_t* launches) {
  if (!ms_sum || !launches) return fail("kernel_times: null argument");
  TS_DEVICE(b);
  for (int k = 0; k < TSIM_KT_COUNT; ++k) { ms_sum[k] = 0.0; launches[k] = 0; }
  for (auto& p : b->kt) {
    float ms = 0.f;
    HIPCHK(hipEventSynchronize(p.b));
    HIPCHK(hipEventElapsedTime(&ms, p.a, p.b));
    ms_sum[p.kind] += ms; launches[p.kind] += 1;
    b->kt_free.push_back(p.a); b->kt_free.push_back(p.b);
  }
  b->kt.clear();
  return 0;
}
int tsim_set_lanes_per_env(tsim_batch* b, int lanes) {
  if (lanes != 0 && lanes != 16 && lanes != 32 && lanes != 64) return fail("set_lanes_per_env: 0 (automatic), 16, 32 or 64");
  b->lpe_forced = lanes;
  shape_changed(b);
  return 0;
}
int tsim_static_model(const tsim_batch* b) { return kernel_mode(b, b->lpe_forced) != TS_KM_GENERIC ? b->static_id : 0; }
const char* tsim_kernel_variant(const tsim_batch* b) {
  const int km = kernel_mode(b, b->lpe_forced);
  if (km == TS_KM_STATIC) return "static:pusher";
  if (km == TS_KM_PARAM) return "param:pusher";
  return "generic";
}
int tsim_set_static(tsim_batch* b, int allow) {
  b->no_static = allow ? 0 : 1;
  shape_changed(b);      // the launch shape depends on which kernels run
  return 0;
}
int tsim_set_option(tsim_batch* b, int option, int value) {
  if (option == TSIM_OPT_PAIR_CULL) { b->pair_cull = value != 0; return 0; }
  if (option == TSIM_OPT_VALUE_TRIALS) { if (value < 0) return fail("set_option: TSIM_OPT_VALUE_TRIALS >= 0"); b->value_trials = value; return 0; }
  if (option == TSIM_OPT_TRIAL_HELPERS) { b->trial_helpers = value != 0; return 0; }
  if (option == TSIM_OPT_VALUE_FIRST) { b->value_first = value != 0; return 0; }
  if (option == TSIM_OPT_PREDICTOR_HELPERS) { b->pred_helpers = value != 0; return 0; }
  if (option == TSIM_OPT_ADJOINT_PREPASS) { b->adj_pre = value != 0; return 0; }
  return fail("set_option: unknown option " + std::to_string(option));
}
int tsim_get_option(const tsim_batch* b, int option) {
  if (option == TSIM_OPT_PAIR_CULL) return b->pair_cull;
  if (option == TSIM_OPT_VALUE_TRIALS) return b->value_trials;
  if (option == TSIM_OPT_TRIAL_HELPERS) return b->trial_helpers;
  if (option == TSIM_OPT_VALUE_FIRST) return b->value_first;
  if (option == TSIM_OPT_CROSS_KINKS) return b->cross_kinks;
  if (option == TSIM_OPT_EVAL_BUDGET) return b->eval_budget;
  if (option == TSIM_OPT_ALL_DEFAULT) return default_options(b) ? 1 : 0;
  if (option == TSIM_OPT_FRAME_RECORDS) return b->last_frame_rec;
  if (option == TSIM_OPT_FORWARD_SPLIT) return b->last_fwd_split;
  if (option == TSIM_OPT_PREDICTOR_HELPERS) return b->pred_helpers;
  if (option == TSIM_OPT_ADJOINT_PREPASS) return b->adj_pre_ran;
  return -1;
}
int tsim_set_solver_options(tsim_batch* b, int cross_kinks, int eval_budget) {
  if (eval_budget < 0) return fail("set_solver_options: negative evaluation budget");
  b->cross_kinks = cross_kinks != 0;
  b->eval_budget = eval_budget;
  return 0;
}
int tsim_last_gnorm(tsim_batch* b, float* host_out) {
  TS_DEVICE(b);
  if (hipMemcpy(host_out, b->gnorm, (size_t)b->B * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return fail("last_gnorm: copy failed");
  return 0;
}
int tsim_last_helper_trials(tsim_batch* b, int32_t* host_out) {
  TS_DEVICE(b);
  if (hipMemcpy(host_out, b->helped, (size_t)b->B * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail("last_helper_trials: copy failed");
  return 0;
}
int tsim_last_evals(tsim_batch* b, int32_t* host_out) {
  TS_DEVICE(b);
  if (hipMemcpy(host_out, b->evals, (size_t)b->B * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail("last_evals: copy failed");
  return 0;
}

int tsim_update_model(tsim_batch* b, const int32_t* I, const double* F, void* stream) {
  if (I[TSIM_IH_NI] != (int)b->I.size() || I[TSIM_IH_NF] != (int)b->F.size()) return fail("update_model: blob size changed");
  for (int i = 0; i < TSIM_IH_SIZE; ++i) if (I[i] != b->I[i]) return fail("update_model: topology changed");
  TS_DEVICE(b);
  pose_invalidate(b, (hipStream_t)stream);
  b->I.assign(I, I + I[TSIM_IH_NI]); b->F.assign(F, F + I[TSIM_IH_NF]);
  if (b->dFenv) { HIPCHK(hipFree(b->dFenv)); (void)b->dFenv.take(); b->env_struct_ok = 0; }     // per-environment tables refer to the old model
  if (int rc = upload_model(b, (hipStream_t)stream)) return rc;
  shape_changed(b);      // the edit may have moved the batch between the compiled-in and the generic kernels: another launch shape
  return 0;
}

int tsim_set_env_tables(tsim_batch* b, const void* tables, void* stream) {
  TS_DEVICE(b);
  pose_invalidate(b, (hipStream_t)stream);
  if (!tables) { if (b->dFenv) { HIPCHK(hipFree(b->dFenv)); (void)b->dFenv.take(); b->env_struct_ok = 0; decide_stage_cpt(b); } return 0; }      // (the block orders stay: see profiles/r24_host_launch_layer.md)
  size_t bytes = (size_t)b->B * b->nfrec * b->esz;
  const bool fresh = !b->dFenv;
  if (fresh) HIPCHK(hipMalloc(&b->dFenv, bytes));
  HIPCHK(hipMemcpyAsync(b->dFenv, tables, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  // Time step, gravity and Newton tolerance are properties of the batch, not of an environment (the reference's randomisers never touch them, and
  // the kernels cache them per wavefront: a helper slot evaluating another environment's trial point would use its own): the header of every row
  // is overwritten with the shared model's.
  {
    const unsigned nh = (unsigned)((b->B * TSIM_FH_SIZE + 255) / 256);
    by_real(b, [&](auto r) { using R = decltype(r); hipLaunchKernelGGL(k_env_header<R>, dim3(nh), dim3(256), 0, (hipStream_t)stream, (R*)b->dFenv, (const R*)b->dF, b->nfrec, b->B); });
    HIPCHK(hipGetLastError());
  }
  // A batch whose model has a compiled-in structure stays on that instantiation if every environment's table keeps the structural floats
  // (the exact 0 / 1 / -1 entries the instantiation has folded away): checked here, on the device, once per call — one small kernel and a
  // 4-byte read-back (this call synchronises then; inside a stream capture the check is skipped and the batch takes the generic kernels).
  const int ok_before = b->env_struct_ok;
  b->env_struct_ok = 0;
  if (b->static_id != 0 && b->dtype == TSIM_F32 && !capturing((hipStream_t)stream)) {
    if (!b->dKmask) {
      std::vector<unsigned char> km(b->nfrec);
      for (int i = 0; i < b->nfrec; ++i) km[i] = TsParam<TsStaticPusher>::Fk(i) ? 1 : 0;
      HIPCHK(hipMalloc((void**)&b->dKmask, km.size())); HIPCHK(hipMalloc((void**)&b->dFlag, sizeof(int)));
      HIPCHK(hipMemcpy(b->dKmask, km.data(), km.size(), hipMemcpyHostToDevice));
    }
    int flag = 0;
    HIPCHK(hipMemsetAsync(b->dFlag, 0, sizeof(int), (hipStream_t)stream));
    const size_t n = (size_t)b->B * b->nfrec;
    hipLaunchKernelGGL(k_check_structure, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)b->dFenv, (const float*)b->dF, b->dKmask, b->nfrec, n, b->dFlag);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&flag, b->dFlag, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    b->env_struct_ok = flag == 0;
  }
  if (fresh || ok_before != b->env_struct_ok) shape_changed(b);      // the block's LDS layout / the kernels change
  return 0;
}
int tsim_table_size(const tsim_batch* b) { return b->nfrec; }

// What the parameter passes need on the device, once a gradient buffer is asked for: z of every taped sub-step and the contact pass's partial sums,
// and, once a body group is on as well, the body pass's partial sums (the default mask never allocates those).  What is there already stays.
static int pg_alloc(tsim_batch* b) {
  const bool body = (b->pg_groups & ~TS_PG_CONTACT) != 0;
  if (b->zbuf && b->pgpart && b->pg_slots && (b->pgbpart || !body)) return 0;
  TS_DEVICE(b);
  const int chunks = pg_layout(b, b->cap).most;
  auto get = [&](void** p, size_t reals) {
    if (*p || hipMalloc(p, std::max<size_t>(reals * b->B * b->esz, 8)) == hipSuccess) return true;
    (void)hipGetLastError(); *p = nullptr;
    return false;
  };
  if (body && !get(&b->pgbpart, (size_t)chunks * ts_pgb_count(b->I[TSIM_IH_NL], b->nu, b->nr))) return fail("set_param_grad_groups: hipMalloc failed");
  if (!get(&b->zbuf, (size_t)b->cap * b->nr) || !get(&b->pgpart, (size_t)chunks * ts_pg_count(b->I[TSIM_IH_NPAIR], b->I[TSIM_IH_NSENSOR], b->nr))) {
    b->zbuf.release(); b->pgpart.release();
    return fail("set_param_grad: hipMalloc failed");
  }
  b->pg_chunks = chunks;
  // ... and the closed-loop adjoint's frame -> seed row table: at most one frame per taped sub-step
  if (!b->pg_slots && hipMalloc((void**)&b->pg_slots, std::max<size_t>((size_t)b->cap * sizeof(int32_t), 8)) != hipSuccess) {
    (void)hipGetLastError(); (void)b->pg_slots.take();
    return fail("set_param_grad: hipMalloc failed");
  }
  return 0;
}

int tsim_set_param_grad_groups(tsim_batch* b, int mask) {
  if (!b) return fail("set_param_grad_groups: null batch");
  if (mask < 0 || (mask & ~(TS_PG_CONTACT | TS_PG_INERTIAL | TS_PG_MOTOR | TS_PG_LIMIT))) return fail("set_param_grad_groups: unknown group in mask " + std::to_string(mask));
  const int before = b->pg_groups;
  b->pg_groups = mask;
  if (b->dLdp && pg_alloc(b)) { b->pg_groups = before; return 1; }
  return 0;
}
int tsim_get_param_grad_groups(const tsim_batch* b) { return b ? b->pg_groups : -1; }
int tsim_last_adjoint_launch(const tsim_batch* b, int32_t* out) {
  if (!b || !out) return fail("last_adjoint_launch: null argument");
  out[0] = b->adj_kernel; out[1] = b->adj_passes;
  return 0;
}

int tsim_set_param_grad(tsim_batch* b, void* dL_dtables) {
  if (dL_dtables && pg_alloc(b)) return 1;
  b->dLdp = dL_dtables;
  return 0;
}

int tsim_reset(tsim_batch* b, const void* q0, const void* qd0, int backward_flag, void* stream) {
  if (!q0) return fail("reset: q0 is null");
  TS_DEVICE(b);
  hipStream_t st = (hipStream_t)stream;
  int n = b->B * b->nr, blk = 256, grd = (n + blk - 1) / blk;
  by_real(b, [&](auto r) { using R = decltype(r); hipLaunchKernelGGL(k_set_state<R>, dim3(grd), dim3(blk), 0, st, (R*)b->tape, (const R*)q0, (const R*)qd0, b->B, b->nr, b->rec); });
  HIPCHK(hipGetLastError());
  if (zero_async(b->lamq, (size_t)2 * b->B * b->nr * b->esz, st) || zero_async(b->lamv, (size_t)2 * b->B * b->nr * b->esz, st)) return 1;
  b->t_cur = 0; b->record = backward_flag ? 1 : 0; b->order_valid = 0; b->has_prev = 0; b->tape_k_ok = b->tape_k;
  pose_invalidate(b, st);
  return 0;
}

int tsim_reset_masked(tsim_batch* b, const void* q0, const void* qd0, const int32_t* mask, void* stream) {
  if (!q0 || !mask) return fail("reset_masked: q0 / mask is null");
  if (b->record) return fail("reset_masked: not while recording (the tape is shared by the batch): use reset");
  TS_DEVICE(b);
  hipStream_t st = (hipStream_t)stream;
  pose_invalidate(b, st);
  int n = b->B * b->nr, blk = 256, grd = (n + blk - 1) / blk;
  size_t off = (size_t)b->t_cur * b->B * b->rec;
  // BDF2 models: the environment restarts with a constant-velocity history (q_-1 = q0 - h qd0, qd_-1 = qd0) [CHOICE]
  double* prev = (b->I[TSIM_IH_INTEGRATOR] == 2 && b->has_prev) ? (double*)b->prev : nullptr;
  by_real(b, [&](auto r) {
    using R = decltype(r);
    hipLaunchKernelGGL(k_set_state_masked<R>, dim3(grd), dim3(blk), 0, st, (R*)b->tape + off, (const R*)q0, (const R*)qd0, mask, prev, (R)b->F[TSIM_FH_H], b->B, b->nr, b->rec);
  });
  HIPCHK(hipGetLastError());
  return 0;
}

int tsim_step(tsim_batch* b, const void* u, int num_steps, void* q_out, void* qd_out, void* var_out, void* tac_out, int32_t* status, void* stream) {
  if (num_steps <= 0) return fail("step: num_steps must be positive");
  if (!u && b->nu > 0) return fail("step: u is null");
  if (b->record && b->t_cur + num_steps > b->cap) return fail("step: tape capacity exceeded (" + std::to_string(b->cap) + " sub-steps)");
  TS_DEVICE(b);
  if (int rc = by_real(b, [&](auto r) { return launch_forward<decltype(r)>(b, u, 1, nullptr, num_steps, q_out, qd_out, var_out, tac_out, status, (hipStream_t)stream); })) return rc;
  if (b->record) b->t_cur += num_steps;
  b->has_prev = 1;
  return 0;
}

int tsim_get_state(tsim_batch* b, void* q_out, void* qd_out, void* stream) {
  TS_DEVICE(b);
  int n = b->B * b->nr, blk = 256, grd = (n + blk - 1) / blk;
  size_t off = (size_t)b->t_cur * b->B * b->rec;
  by_real(b, [&](auto r) { using R = decltype(r); hipLaunchKernelGGL(k_get_state<R>, dim3(grd), dim3(blk), 0, (hipStream_t)stream, (const R*)b->tape + off, (R*)q_out, (R*)qd_out, b->B, b->nr, b->rec); });
  HIPCHK(hipGetLastError());
  return 0;
}

int tsim_readout(tsim_batch* b, void* var_out, void* tac_out, void* stream) {
  TS_DEVICE(b);
  hipStream_t st = (hipStream_t)stream;
  const bool tac = tac_out && b->ntax > 0 && b->nspt > 0;
  // taxels that are paired with no primitive (a sensor body without a general_primitive_contact) read zero, as in k_forward's read-out
  if (tac_out && b->ntax > 0 && b->nspt == 0 && zero_async(tac_out, (size_t)b->B * 3 * b->ntax * b->esz, st)) return 1;
  if (tac && (b->nspt > TX_MAXK || b->I[TSIM_IH_NSENSOR] > TX_MAXS)) return fail("readout: more than " + std::to_string((int)TX_MAXK) + " (sensor, primitive) combinations or " + std::to_string((int)TX_MAXS) + " sensors (k_taxels staging)");
  if (capturing(st)) { b->pose_off = 1; b->pose_valid = 0; }
  const bool fk = var_out || !tac || !b->pose_valid;      // the forward launch left the pose records of this state: k_taxels alone
  const int rc = by_real(b, [&](auto r) {
    using R = decltype(r);
    ReadArgs<R> a{b->dI, (const R*)b->dF, (const R*)b->dFenv, b->nfrec, b->B, b->t_cur, (const R*)b->tape, (R*)var_out, tac ? (R*)b->poseR : nullptr, b->poseD, b->nspt, b->stage_cpt, b->tape_k};
    if (fk) hipLaunchKernelGGL(k_readout<R>, dim3(b->B), dim3(TS_WAVE), lds_bytes_for(b, 1), st, a);
    if (!tac) return 0;
    KtScope kt_(b, TSIM_KT_TAXELS, st);
    return launch_taxels<R>(b, b->poseR, b->poseD, 1, nullptr, tac_out, st);
  });
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return 0;
}

int tsim_backward_steps(tsim_batch* b, int n, int seed_mode, const void* df_dq, const void* df_dvar, const void* df_dtac, void* df_du, void* stream) {
  if (!b->record) return fail("backward_steps: reset(backward_flag=True) was not called");
  if (n <= 0 || n > b->t_cur) return fail("backward_steps: only " + std::to_string(b->t_cur) + " sub-steps on the tape");
  if (!df_du && b->nu > 0) return fail("backward_steps: df_du is null");
  if (seed_mode != 0 && seed_mode != 1) return fail("backward_steps: bad seed_mode");
  TS_DEVICE(b);
  const int stride = seed_mode == 1 ? 1 : n;
  if (int rc = by_real(b, [&](auto r) { return launch_backward<decltype(r)>(b, n, stride, 0, nullptr, df_dq, df_dvar, df_dtac, df_du, (hipStream_t)stream); })) return rc;
  b->t_cur -= n;
  pose_invalidate(b, (hipStream_t)stream);      // the pose records a forward launch left are those of the state before the roll-back
  return 0;
}

int tsim_rollout(tsim_batch* b, const void* u, int num_frames, int num_steps, const int32_t* tactile_slot, void* q_out, void* qd_out, void* var_out, void* tac_out, int32_t* status, void* stream) {
  if (int rc = frames_positive("rollout", num_frames, num_steps)) return rc;
  if (!u && b->nu > 0) return fail("rollout: u is null");
  if (b->record && b->t_cur + (long long)num_frames * num_steps > b->cap) return fail("rollout: tape capacity exceeded (" + std::to_string(b->cap) + " sub-steps)");
  TS_DEVICE(b);
  if (int rc = by_real(b, [&](auto r) { return launch_forward<decltype(r)>(b, u, num_frames, tactile_slot, num_steps, q_out, qd_out, var_out, tac_out, status, (hipStream_t)stream); })) return rc;
  if (b->record) b->t_cur += num_frames * num_steps;
  b->has_prev = 1;
  return 0;
}

int tsim_backward_episode(tsim_batch* b, int num_frames, int num_steps, const int32_t* tactile_slot, const void* df_dq, const void* df_dvar, const void* df_dtac, void* df_du, void* stream) {
  if (!b->record) return fail("backward_episode: reset(backward_flag=True) was not called");
  long long n;
  if (int rc = taped_window(b, "backward_episode", num_frames, num_steps, &n)) return rc;
  if (!df_du && b->nu > 0) return fail("backward_episode: df_du is null");
  TS_DEVICE(b);
  if (int rc = by_real(b, [&](auto r) { return launch_backward<decltype(r)>(b, (int)n, num_steps, 1, tactile_slot, df_dq, df_dvar, df_dtac, df_du, (hipStream_t)stream); })) return rc;
  b->t_cur -= (int)n;
  pose_invalidate(b, (hipStream_t)stream);
  return 0;
}

int tsim_tangent_episode(tsim_batch* b, int num_frames, int num_steps, int ndir, const int32_t* tactile_slot, const void* du, const void* dq0, const void* dqd0,
                         const void* dtables, void* dq_out, void* dqd_out, void* dvar_out, void* dtac_out, void* stream) {
  if (!b) return fail("tangent_episode: null batch");
  if (ndir < 1 || ndir > TSIM_TANGENT_MAX_DIR) return fail("tangent_episode: ndir must be 1 .. " + std::to_string((int)TSIM_TANGENT_MAX_DIR) + ", got " + std::to_string(ndir));
  if (!b->record || b->t_cur <= 0) return fail("tangent_episode: no tape recorded (reset(backward_flag=True), then a roll-out)");
  long long n;
  if (int rc = taped_window(b, "tangent_episode", num_frames, num_steps, &n)) return rc;
  if (int rc = bdf2_window_is_the_tape(b, "tangent_episode", n)) return rc;
  TS_DEVICE(b);
  return by_real(b, [&](auto r) { return launch_tangent<decltype(r)>(b, num_frames, num_steps, ndir, tactile_slot, du, dq0, dqd0, dtables, dq_out, dqd_out, dvar_out, dtac_out, (hipStream_t)stream); });
}

int tsim_frame_jacobians(tsim_batch* b, int num_frames, int num_steps, void* A_out, void* B_out, void* Jvar_out, void* stream) {
  if (!b) return fail("frame_jacobians: null batch");
  if (!b->record || b->t_cur <= 0) return fail("frame_jacobians: no tape recorded (reset(backward_flag=True), then a roll-out)");
  long long n;
  if (int rc = taped_window(b, "frame_jacobians", num_frames, num_steps, &n)) return rc;
  if (b->I[TSIM_IH_INTEGRATOR] == 2) return fail("frame_jacobians: a BDF2 model's transition acts on two states of history, which is out of scope");
  if (!A_out && !B_out && !Jvar_out) return 0;
  TS_DEVICE(b);
  return by_real(b, [&](auto r) { return launch_frame_jacobians<decltype(r)>(b, num_frames, num_steps, A_out, B_out, Jvar_out, (hipStream_t)stream); });
}

int tsim_tactile_jacobians(tsim_batch* b, int num_frames, int num_steps, const int32_t* tactile_slot, void* Ct_out, void* stream) {
  if (!b) return fail("tactile_jacobians: null batch");
  if (b->ntax <= 0) return fail("tactile_jacobians: the model has no taxels");
  if (!Ct_out) return fail("tactile_jacobians: null Ct_out");
  if (!b->record || b->t_cur <= 0) return fail("tactile_jacobians: no tape recorded (reset(backward_flag=True), then a roll-out)");
  long long n;
  if (int rc = taped_window(b, "tactile_jacobians", num_frames, num_steps, &n)) return rc;
  TS_DEVICE(b);
  return by_real(b, [&](auto r) { return launch_tactile_jacobians<decltype(r)>(b, num_frames, num_steps, tactile_slot, Ct_out, (hipStream_t)stream); });
}

int tsim_tactile_normal_equations(tsim_batch* b, int num_frames, int num_steps, const int32_t* tactile_slot, int with_params, const void* weight, const void* resid,
                                  void* N_out, void* n_out, void* stream) {
  if (!b) return fail("tactile_normal_equations: null batch");
  if (b->ntax <= 0) return fail("tactile_normal_equations: the model has no taxels");
  if (!N_out) return fail("tactile_normal_equations: null N_out");
  if ((resid != nullptr) != (n_out != nullptr)) return fail("tactile_normal_equations: resid and n_out go together (one of them is null)");
  if (!b->record || b->t_cur <= 0) return fail("tactile_normal_equations: no tape recorded (reset(backward_flag=True), then a roll-out)");
  long long n;
  if (int rc = taped_window(b, "tactile_normal_equations", num_frames, num_steps, &n)) return rc;
  TS_DEVICE(b);
  return by_real(b, [&](auto r) { return launch_tactile_normal<decltype(r)>(b, num_frames, num_steps, tactile_slot, with_params, weight, resid, N_out, n_out, (hipStream_t)stream); });
}

// table column -> compact index in ts_pg_count order ([pair kn kt mu kd], [sensor kn kt mu kd], [dof damping]: launch_param_grad's segments), or -1
static_assert((int)TS_PJ_MAX_COLS == (int)TSIM_PARAM_JACOBIAN_MAX_COLS, "tsim_param_jacobian.h and include/tsim.h disagree");
static int contact_column_index(const tsim_batch* b, int col) {
  const int npair = b->I[TSIM_IH_NPAIR], nsensor = b->I[TSIM_IH_NSENSOR];
  const struct { int count, per, rec, col0, base; } seg[3] = {{npair, 4, TSIM_PF_SIZE, b->I[TSIM_IH_FOFF_PAIR] + TSIM_PF_KN, 0},
                                                               {nsensor, 4, TSIM_SF_SIZE, b->I[TSIM_IH_FOFF_SENSOR] + TSIM_SF_KN, 4 * npair},
                                                               {b->nr, 1, TSIM_DF_SIZE, b->I[TSIM_IH_FOFF_DOF] + TSIM_DF_DAMPING, 4 * npair + 4 * nsensor}};
  for (const auto& s : seg) {
    const int rel = col - s.col0;
    if (rel < 0 || rel >= s.count * s.rec) continue;
    if (rel % s.rec < s.per) return s.base + (rel / s.rec) * s.per + rel % s.rec;
  }
  return -1;
}

int tsim_param_jacobians(tsim_batch* b, int num_frames, int num_steps, int ncols, const int32_t* cols, const int32_t* tactile_slot, void* E_out, void* Ft_out, void* stream) {
  if (!b) return fail("param_jacobians: null batch");
  if (!E_out && !Ft_out) return fail("param_jacobians: E_out and Ft_out are both null");
  int cidx[TS_PJ_MAX_COLS];
  if (E_out) {
    if (ncols < 1 || ncols > TSIM_PARAM_JACOBIAN_MAX_COLS) return fail("param_jacobians: ncols must be 1 .. " + std::to_string((int)TSIM_PARAM_JACOBIAN_MAX_COLS) + ", got " + std::to_string(ncols));
    if (!cols) return fail("param_jacobians: null cols");
    for (int k = 0; k < ncols; ++k) {
      cidx[k] = contact_column_index(b, cols[k]);
      if (cidx[k] < 0) return fail("param_jacobians: table column " + std::to_string(cols[k]) + " is not a contact-group parameter (pair or sensor kn kt mu damping, dof damping)");
      for (int i = 0; i < k; ++i)
        if (cidx[i] == cidx[k]) return fail("param_jacobians: table column " + std::to_string(cols[k]) + " is listed twice");
    }
  }
  if (Ft_out && b->ntax <= 0) return fail("param_jacobians: Ft_out on a model without taxels");
  if (!b->record || b->t_cur <= 0) return fail("param_jacobians: no tape recorded (reset(backward_flag=True), then a roll-out)");
  long long n;
  if (int rc = taped_window(b, "param_jacobians", num_frames, num_steps, &n)) return rc;
  if (E_out && b->I[TSIM_IH_INTEGRATOR] == 2) return fail("param_jacobians: E_out on a BDF2 model (its transition acts on two states of history), which is out of scope");
  TS_DEVICE(b);
  return by_real(b, [&](auto r) { return launch_param_jacobians<decltype(r)>(b, num_frames, num_steps, E_out ? ncols : 0, cidx, tactile_slot, E_out, Ft_out, (hipStream_t)stream); });
}

int tsim_get_adjoint(tsim_batch* b, void* df_dq0, void* df_dqd0, void* stream) {
  TS_DEVICE(b);
  size_t bytes = (size_t)b->B * b->nr * b->esz;
  if (df_dq0) HIPCHK(hipMemcpyAsync(df_dq0, b->lamq, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (df_dqd0) HIPCHK(hipMemcpyAsync(df_dqd0, b->lamv, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// Backward cache = LIFO of tape BUFFERS swapped by pointer (no tape copy): save parks the live tape on the stack and takes a
// spare buffer from the pool (allocated on first use, or ahead of time by tsim_cache_reserve), pop swaps back.  After
// warm-up neither allocates nor synchronises, so both can sit inside a captured HIP graph region's host code path.
static size_t tape_bytes_of(const tsim_batch* b) { return (size_t)(b->cap + 1) * b->B * b->rec * b->esz; }
int tsim_cache_reserve(tsim_batch* b, int depth) {
  TS_DEVICE(b);
  while ((int)(b->pool.size() + b->cache.size()) < depth) {
    void* p = nullptr;
    if (hipMalloc(&p, tape_bytes_of(b)) != hipSuccess) return fail("cache_reserve: hipMalloc of a " + std::to_string(tape_bytes_of(b)) + " byte tape failed");
    b->pool.push_back(p);
  }
  return 0;
}
int tsim_cache_save(tsim_batch* b, void* stream) {
  TS_DEVICE(b);
  if (b->pool.empty()) { int rc = tsim_cache_reserve(b, (int)b->cache.size() + 1); if (rc) return rc; }
  void* spare = b->pool.back(); b->pool.pop_back();
  // the simulation goes on from its current state: carry the newest record (q, qd of all environments) over
  const size_t rec_bytes = (size_t)b->B * b->rec * b->esz, off = (size_t)b->t_cur * rec_bytes;
  HIPCHK(hipMemcpyAsync((char*)spare + off, (char*)b->tape + off, rec_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  // ... and, for BDF2 models, the record before it: while recording, k_forward takes the state before the previous sub-step from tape
  // record t0 - 1, so a forward launch that continues on the spare buffer must find it there
  if (b->I[TSIM_IH_INTEGRATOR] == 2 && b->t_cur >= 1)
    HIPCHK(hipMemcpyAsync((char*)spare + off - rec_bytes, (char*)b->tape + off - rec_bytes, rec_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  CacheEntry e; e.buf = b->tape; e.len = b->t_cur; e.record = b->record; e.tape_k_ok = b->tape_k_ok;
  b->cache.push_back(e);
  b->tape = spare;
  return 0;
}
int tsim_cache_pop(tsim_batch* b, void* stream) {
  if (b->cache.empty()) return fail("popBackwardCache: cache is empty");
  TS_DEVICE(b);
  CacheEntry e = b->cache.back(); b->cache.pop_back();
  b->pool.push_back(b->tape);                 // stream order keeps earlier kernels on the old buffer safe: it is only
  b->tape = e.buf;                            // handed out again by a later save on the same stream
  b->t_cur = e.len; b->record = e.record; b->tape_k_ok = e.tape_k_ok; b->has_prev = 0; b->order_valid = 0;
  pose_invalidate(b, (hipStream_t)stream);
  if (zero_async(b->lamq, (size_t)2 * b->B * b->nr * b->esz, (hipStream_t)stream) || zero_async(b->lamv, (size_t)2 * b->B * b->nr * b->esz, (hipStream_t)stream)) return 1;
  return 0;
}
int tsim_cache_clear(tsim_batch* b) {
  DeviceGuard guard_(b->device);
  for (auto& e : b->cache) b->pool.push_back(e.buf);
  b->cache.clear();
  while (b->pool.size() > 2) { (void)hipFree(b->pool.back()); b->pool.pop_back(); }     // keep two spares warm
  return 0;
}
int tsim_cache_depth(const tsim_batch* b) { return (int)b->cache.size(); }

int tsim_debug_signature(tsim_batch* b, int t_first, int n, uint32_t* out, void* stream) {
  if (!b->record) return fail("debug_signature: reset(backward_flag=True) was not called (the signature is taken from the tape)");
  if (t_first < 0 || n <= 0 || t_first + n > b->t_cur) return fail("debug_signature: sub-steps " + std::to_string(t_first) + "+" + std::to_string(n) + " are not on the tape (" + std::to_string(b->t_cur) + ")");
  if (!out) return fail("debug_signature: out is null");
  TS_DEVICE(b);
  by_real(b, [&](auto r) {
    using R = decltype(r);
    SigArgs<R> a{b->dI, (const R*)b->dF, (const R*)b->dFenv, b->nfrec, b->B, t_first, n, (const R*)b->tape, out, b->stage_cpt, b->tape_k};
    hipLaunchKernelGGL(k_signature<R>, dim3(b->B), dim3(TS_WAVE), lds_bytes_for(b, 1), (hipStream_t)stream, a);
  });
  HIPCHK(hipGetLastError());
  return 0;
}

int tsim_debug_stamps(tsim_batch* b, long long* cycles) { b->bwd_stamps = cycles; return 0; }

int tsim_debug_eval(tsim_batch* b, const void* q1, const void* q0, const void* qd0, const void* u, void* g_out, void* H_out, long long* cycles, void* stream) {
  TS_DEVICE(b);
  // the stamped variant of an nr > 8 model: one environment per wavefront whatever the batch's shape (ts_plan: the debug kernel's shape)
  const TsPlan plan = ts_plan(b, TS_K_DEBUG_EVAL, false, cycles && b->nr > 8 ? TS_WAVE : 0);
  const bool ok = by_real(b, [&](auto r) {
    using R = decltype(r);
    DbgArgs<R> a{b->dI, (const R*)b->dF, (const R*)b->dFenv, b->nfrec, b->B, (const R*)q1, (const R*)q0, (const R*)qd0, (const R*)u, (R*)g_out, (R*)H_out, cycles, b->stage_cpt, b->pair_cull};
    return ts_launch<false, R>(plan, (hipStream_t)stream, a);
  });
  if (!ok) return fail("no k_debug_eval instantiation for the launch plan");
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"

// ================================================================================================ TactilePush per-step formulas
#include "../../include/tsim_env.h"
#include "tsim_env_push.h"
