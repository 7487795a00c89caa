// tsim_batch.h — the host side's plumbing: the batch (tsim_batch), what every entry point does before it launches (the error text, the device
// guard, the precision dispatch, "is this stream capturing?"), and the ownership of the batch's device buffers.  Host only: no kernel, no device
// code.  Included by tsim_hip.hip alone, which defines the entry points on top of it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/tsim.h"
#include "tsim_launch.h"

static thread_local std::string g_err;
static int fail(const std::string& m) { g_err = m; return 1; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

// Every entry point runs on the batch's device and leaves the calling thread's current device as it found it (a process
// may drive several GPUs, and torch's current device / current_stream() follow the thread's HIP device).
struct DeviceGuard {
  int prev = -1; bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess; else prev = -1;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define TS_DEVICE(b) DeviceGuard guard_((b)->device); if (!guard_.ok) return fail("hipSetDevice(" + std::to_string((b)->device) + ") failed")

// Is the stream being captured into a graph?  A query that fails counts as yes: every caller then takes its careful side (no events, no
// allocation, no read-back, no reuse of what a replay would change behind the host's back).
static bool capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
}

// The precision of a launch as a type: f(R()) with R = float or double, so that a templated call and its arguments are written once.
template <class F> static auto by_dtype(int dtype, F&& f) { return dtype == TSIM_F32 ? f(float()) : f(double()); }

// A device buffer the batch owns: null until allocated, freed when the batch goes (tsim_batch_destroy, on the batch's device), never copied.
// It converts to the pointer type its use names, as a void* member does under a cast; & is hipMalloc's out-parameter, for an EMPTY buffer.
struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { (void)hipFree(p); }
  template <class U> operator U*() const { return static_cast<U*>(p); }
  explicit operator bool() const { return p != nullptr; }
  void** operator&() { return &p; }
  void* take() { void* q = p; p = nullptr; return q; }      // the caller owns it now
  void release() { (void)hipFree(take()); }
};

struct CacheEntry { void* buf; int len; int record, tape_k_ok; };
struct KtPair { hipEvent_t a, b; int kind; };
struct tsim_batch {
  int B, dtype, device, cap;
  std::vector<int32_t> I; std::vector<double> F;
  int nl, nr, nu, nvar, ntax, rec;
  // The tape records of a batch created with a compiled-in model (kernel_mode: the fused static instantiations) hold K next to H (ts_rec: tape_k).
  // tape_k_ok: every record since the last reset was written by such an instantiation, which the fused adjoint kernels need (launch_backward)
  int tape_k = 0, tape_k_ok = 0;
  DevBuf dI, dF;                 // model on device (int32; dF in the batch's real type)
  DevBuf dFenv; int nfrec;       // optional per-environment float tables [B][nfrec] (domain randomisation)
  void* tape = nullptr;          // [(cap+1)][B][rec]; not a DevBuf: the backward cache swaps it with the pool's buffers (tsim_cache_save / _pop)
  DevBuf lamq, lamv;             // carried adjoint [2][B][nr]: of the state the next adjoint sub-step starts from, and (BDF2) what later
                                 // sub-steps already contributed to the state one step further back
  DevBuf evals;                  // int: residual evaluations of the last forward launch, per env
  DevBuf helped;                 // int: ... and how many of its line-search trials a helper slot evaluated (k_forward; tsim_last_helper_trials)
  DevBuf gnorm;                  // float: largest ||g|| a sub-step of the last forward launch ended with, per env
  int cross_kinks = 0, eval_budget = 0;     // tsim_set_solver_options
  DevBuf order; int order_valid = 0; // int: block -> env map for the next forward launch (LPT scheduling)
  DevBuf order_ep; int order_ep_n = 0;   // ... for the next EPISODE launch of order_ep_n sub-steps (from the previous one's totals; survives reset)
  DevBuf prev; int has_prev = 0; // double: BDF2: state before the previous sub-step [B][2 nr]
  DevBuf poseR, poseD; int nspt; // tsim_readout: pose records [B][nspt] of the (sensor, primitive) combinations (k_readout -> k_taxels); real, double
  int has_exp;                   // model contains a rotation-vector joint
  int t_cur, record;
  int lpe_forced;                // lanes per environment forced by TSIM_LPE (0 = choose from the batch size)
  int nsched;                    // ints of the sweep schedule appended to dI
  int stage_cpt;                 // the contact-point arrays are staged in LDS with the shared tables
  int n_simd;                    // SIMDs of the device (CUs x 4)
  int last_frame_rec = 0;        // the newest forward launch left its frames' outputs to k_frame_records (1; 2: and ran k_forward_fr; tsim_get_option TSIM_OPT_FRAME_RECORDS)
  // The forward launch split by LPT rank (launch_forward); all three null with TSIM_NO_FORWARD_SPLIT=1 at creation (or where they could not be
  // created): one launch everywhere
  hipStream_t split_st = nullptr;    // the side stream that carries the light wavefronts and their read-out
  hipEvent_t split_fork = nullptr;   // recorded on the caller's stream before the heavy launch: the side stream waits for it
  hipEvent_t split_join = nullptr;   // recorded on the side stream behind its last kernel: the caller's stream waits for it
  int last_fwd_split = 0;        // the newest forward launch went out split (tsim_get_option TSIM_OPT_FORWARD_SPLIT)
  int value_trials = 2;          // line-search trials after this many rejected ones evaluate the residual only (0: off; tsim_set_option TSIM_OPT_VALUE_TRIALS; TSIM_VALUE_TRIALS=n at creation)
  int pred_helpers = 1;         // ... and the predictor of the next sub-step of a slot whose evaluation may end its current one (tsim_set_option TSIM_OPT_PREDICTOR_HELPERS; TSIM_NO_PREDICTOR_HELPERS=1 at creation: off; nothing without trial_helpers)
  int trial_helpers = 1;        // finished slots of a wavefront evaluate the next line-search trials of a slot that is still in one (tsim_set_option TSIM_OPT_TRIAL_HELPERS; TSIM_NO_TRIAL_HELPERS=1 at creation: off)
  int value_first = 1;           // launches without a tape: the first trial after a Newton step evaluates the residual only where the previous sub-step converged in one step (tsim_set_option TSIM_OPT_VALUE_FIRST; TSIM_NO_VALUE_FIRST=1 at creation: off)
  // A/B switches of the environment, read ONCE at creation (launches are on the host-bound path of the per-step collectors):
  // TSIM_NO_EPISODE_LPT, TSIM_INKERNEL_READOUT, TSIM_NO_FREE_RUN, TSIM_LOCKSTEP, TSIM_TAXELS_PER_RECORD, TSIM_NO_ENVTAB_CPT
  bool ab_no_episode_lpt = false, ab_inkernel_readout = false, ab_no_free_run = false, ab_lockstep = false, ab_taxels_per_record = false, ab_no_envtab_cpt = false, ab_no_default_opts = false, ab_inkernel_frame_out = false; int ab_bwd_lpe = 0, ab_lpt_deal = 2;
  int pair_cull = 1;             // phase 2 skips contact pairs out of reach of their primitive (tsim_set_option TSIM_OPT_PAIR_CULL; TSIM_NO_PAIR_CULL=1 at creation: off)
  // Compiled-in models (csrc/tsim_static.h).  static_id: the model whose STRUCTURE the batch's blob has (ints + the structural floats: 1 TactilePush);
  // static_exact: every float record equals the compiled asset's bit for bit as well (the fully static instantiation); env_struct_ok: the
  // per-environment tables keep the structural floats (checked on the device by tsim_set_env_tables).  TSIM_NO_STATIC=1 at creation /
  // tsim_set_static(0) keep the generic kernels.
  int static_id = 0, static_exact = 0, env_struct_ok = 0, no_static = 0;
  DevBuf dKmask, dFlag;          // structural-float mask of static_id on the device (bytes), one-int result of the table check
  DevBuf fposeR, fposeD; int fpose_frames = 0;   // pose records per frame [fpose_frames][B][nspt] of episode launches with a deferred read-out; real, double
  int pose_valid = 0;            // the pose records are those of the current state (left by the last forward launch)
  int pose_off = 0;              // a launch of this batch was captured in a HIP graph: replays change the state behind the host's back, no reuse
  int tt_off = 0;                // offset of the taxel staging table in the device int blob (I[NI] + S[TS_SCHED_TAXTAB])
  int tax_slots = 0;             // blocks of k_taxels the device holds at once (occupancy x CUs), queried on first use
  size_t esz;
  std::vector<CacheEntry> cache;   // saved tapes, newest last
  std::vector<void*> pool;          // spare tape buffers
  std::vector<void*> retired;       // grow-only buffers replaced by larger ones while a captured graph may still name them (grow_buffers)
  long long* bwd_stamps = nullptr;  // diagnostics (tsim_debug_stamps): the caller's buffer
  // tsim_set_param_grad: the caller's table gradient [B][nfrec] (null: off; the caller's buffer), the adjoint solutions z [cap][B][nr] the adjoint launch saves for the
  // parameter passes, and the contact pass's partial sums [pg_chunks][B][ts_pg_count] (pg_alloc: both when the gradient is first asked for)
  void* dLdp = nullptr; DevBuf zbuf, pgpart; int pg_chunks = 0;
  // tsim_set_param_grad_groups: which groups of columns a launch adds to (TSIM_PG_*), and the body pass's partial sums
  // [pg_chunks][B][ts_pgb_count] (pg_alloc: once a body group is on and the gradient is asked for)
  int pg_groups = TS_PG_CONTACT; DevBuf pgbpart;
  // tsim_tangent_episode with a body group on: the body columns' part of every sub-step's source, [ndir][n][B][nr] (k_tangent_body_src writes it,
  // k_tangent reads it).  Grows only: allocated by the first call that needs it or needs it larger (launch_tangent_body_src), tan_src_reals its size
  // tan_src_captured: a launch that names the current workspace was issued under stream capture, so growth retires it instead of freeing it
  DevBuf tan_src; size_t tan_src_reals = 0; int tan_src_captured = 0;
  // the closed-loop adjoint with the buffer set (tsim_push_closed_backward): frame -> seed row of the contact pass, int32 [cap] (pg_alloc; written on the
  // launch's stream by ts_closed_slots_launch)
  DevBuf pg_slots;
  // diagnostics (tsim_last_adjoint_launch): the kernel of the most recent adjoint launch (TSIM_ADJ_*, -1: none yet) and the parameter passes behind it
  int adj_kernel = -1, adj_passes = 0;
  // the seed pre-pass of the fused episode adjoint (tsim_adjoint_pre.h; tsim_set_option TSIM_OPT_ADJOINT_PREPASS, TSIM_NO_ADJOINT_PREPASS=1 at creation: off):
  // its result [cap][B][2 nr], allocated with the tape (a batch whose allocation failed keeps the in-kernel path), and whether the last adjoint launch took the path
  int adj_pre = 1, adj_pre_ran = 0; DevBuf sseed;
  // tsim_kernel_timing: HIP events around every launch of the simulation kernels, on the stream they are launched on
  int kt_on = 0;
  std::vector<KtPair> kt;           // pairs recorded since the last tsim_kernel_times
  std::vector<hipEvent_t> kt_free;  // events to reuse
};
template <class F> static auto by_real(const tsim_batch* b, F&& f) { return by_dtype(b->dtype, f); }
// the side stream and the events of the split forward launch go (on the batch's device; destroying a stream lets its work finish first)
static void split_release(tsim_batch* b) {
  if (b->split_st) (void)hipStreamDestroy(b->split_st);
  if (b->split_fork) (void)hipEventDestroy(b->split_fork);
  if (b->split_join) (void)hipEventDestroy(b->split_join);
  b->split_st = nullptr; b->split_fork = b->split_join = nullptr;
}

// One timed launch: start event in the constructor, stop event in the destructor (nothing under stream capture: no events inside a graph).
struct KtScope {
  tsim_batch* b; hipStream_t st; KtPair p; bool on = false;
  KtScope(tsim_batch* b_, int kind, hipStream_t st_) : b(b_), st(st_) {
    if (!b->kt_on || b->kt.size() >= (size_t)1 << 16) return;      // (a caller that never reads the times back does not grow the list without bound)
    if (capturing(st)) return;
    hipEvent_t e[2];
    for (int i = 0; i < 2; ++i) {
      if (!b->kt_free.empty()) { e[i] = b->kt_free.back(); b->kt_free.pop_back(); }
      else if (hipEventCreate(&e[i]) != hipSuccess) { (void)hipGetLastError(); if (i) b->kt_free.push_back(e[0]); return; }
    }
    p.a = e[0]; p.b = e[1]; p.kind = kind;
    on = hipEventRecord(p.a, st) == hipSuccess;
    if (!on) { b->kt_free.push_back(e[0]); b->kt_free.push_back(e[1]); }
  }
  ~KtScope() { if (on) { (void)hipEventRecord(p.b, st); b->kt.push_back(p); } }
};

// Grow-only device buffers (the per-frame pose records, the tangent workspace): replace each by one of the size wanted.  The caller has made sure
// the stream is not capturing (no allocation inside a capture).  The stream is synchronised first: an earlier launch may still use the old
// buffers.  named: a captured graph may hold the OLD buffers' addresses in its kernel arguments (each caller's own condition) — a replay after
// this point would write freed memory: such buffers are retired (freed with the batch), not freed.
// 0: grown; 1: failed, the message is set; -1: no memory — every buffer is empty, and what follows from that is the caller's
struct GrowWant { DevBuf& buf; size_t bytes; };
static int grow_buffers(tsim_batch* b, hipStream_t st, bool named, std::initializer_list<GrowWant> want) {
  HIPCHK(hipStreamSynchronize(st));
  for (const GrowWant& w : want) {
    if (!named) w.buf.release();
    else if (w.buf) b->retired.push_back(w.buf.take());
  }
  for (const GrowWant& w : want)
    if (hipMalloc(&w.buf, w.bytes) != hipSuccess) {      // (which leaves null in w.buf)
      (void)hipGetLastError();
      for (const GrowWant& v : want) v.buf.release();
      return -1;
    }
  return 0;
}

// the four ints a *_launch_info entry point reports of a plan
static int plan_info(const TsPlan& p, int32_t* out) {
  out[0] = (int32_t)p.lds; out[1] = TS_WAVE; out[2] = (int32_t)p.grid; out[3] = p.lpe;
  return 0;
}
