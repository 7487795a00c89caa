"""The body groups of the kernels' table gradient (tsim_set_param_grad_groups: k_backward_z -> k_param_grad_body -> k_param_reduce; link mass,
com, inertia; motor lo hi P D; limit lo hi k) against the fp64 CPU oracle's exact body adjoint (OracleSim.set_param_grad_groups, pinned to the
oracle's own finite differences by tests/test_oracle_body_param_grad.py).

Built like tests/test_gpu_param_grad_oracle.py: every environment is compared with an oracle run of the model with that environment's table row
in place, on the same trajectory, EVERY body column of it.  Compared: the environments whose kernel branch signature equals the oracle's at every
sub-step and that converged on both sides.  fp64 kernels and oracle take the same Newton iterates (tol 1e-13, or the asset's own for
static:pusher), so the Newton tolerance does not enter the comparison.  fp32 kernels run at the model's tol, the oracle there with max_iter >= 100.

What the finite-difference file (tests/test_gpu_body_param_grad.py, B = 1 throughout) cannot see and this one is for: more than one sub-step per
chunk of k_param_grad_body (its accumulators over the loop, the t - 1 / t - 2 records read across a chunk boundary), all four chunk layouts, slots
> 0 with distinct environments at 16 / 32 lanes, the invalid slots of a ragged batch, and windows that continue a buffer.
Too little compared fails, it does not skip.  TSIM_PG_STATS=<dir>: the error distributions are written there (profiles/r12_body_param_grad_oracle.md)."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
from param_grad_util import (ALL, BODY_KINDS as KINDS, LIMIT_CHAIN, MODELS, body_case, gpu_episode, kind_of, layout_kind, loss_weights,      # noqa: E402
                             make_sim as _sim, oracle_cached, pg_layout, pusher_case, row_model, table_rows)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATS = os.environ.get("TSIM_PG_STATS")
# fp64, per (environment, column): |g - g_oracle| / max(|g_oracle|, F64_FLOOR x the row's largest oracle entry of the same kind).  Measured on
# MI355X over every group of this file (profiles/r12_body_param_grad_oracle.md): max 7.3e-6 (generic, all three launch shapes alike), 99 % 4e-7;
# every other group <= 1.7e-6.  The bound is 10x the measured maximum.
F64_FLOOR, F64_BOUND = 1e-7, 7.3e-5
F64_SHARE = 1e-6        # and >= 99 % within 1e-6 of the row-kind scale (the project's fp64 expectation; measured 99.92 % generic, 100 % elsewhere)
# fp32, the project's rule against the oracle value: >= 99 % within 1e-4 S_kind, none above 1e-2 (S_kind: the row's largest oracle entry of the kind)
F32_99, F32_MAX = 1e-4, 1e-2
ABOVE = 1e-3            # "above the floor" in the coverage counts: |g_oracle| >= 1e-3 S_kind
LIMIT_KINDS = ("limit lo", "limit hi", "limit k")
PUSHER_KINDS = ("mass", "com", "inertia", "motor lo", "motor hi")      # TactilePush: force motors, no limits


class Tally:
    """errors and coverage of one group of this file"""

    def __init__(self, fp64):
        self.fp64, self.envs, self.compared = fp64, 0, 0
        self.rel, self.over_s, self.worst = [], [], []
        self.above = {k: 0 for k in KINDS}
        self.models = {k: set() for k in KINDS}
        self.lanes, self.layouts, self.reached = set(), set(), set()

    def add(self, m, g, go, name, tag):
        bcols = m.body_param_columns()
        kinds = [kind_of(bc) for bc in bcols]
        S = {k: max([abs(go[bc[3]]) for bc, kk in zip(bcols, kinds) if kk == k], default=0.0) for k in set(kinds)}
        self.compared += 1
        for bc, k in zip(bcols, kinds):
            c, s = bc[3], S[k]
            d = abs(g[c] - go[c])
            if s == 0:                                     # the loss does not see this kind on this row: the kernels' entries are exactly 0 too
                assert d == 0, (tag, bc, g[c])
                continue
            self.rel.append(d / max(abs(go[c]), F64_FLOOR * s))
            self.over_s.append(d / s)
            self.worst.append((float(self.rel[-1] if self.fp64 else self.over_s[-1]), str(tag), k))
            if abs(go[c]) >= ABOVE * s:
                self.above[k] += 1
                self.models[k].add(name)

    def check(self, what, kinds, min_share=0.5, min_count=3, limit_models=False, share=True):
        rel, ov = np.array(self.rel), np.array(self.over_s)
        q = lambda x: [float(v) for v in np.quantile(x, [0.5, 0.9, 0.99, 1.0])] if x.size else None      # noqa: E731
        st = {"envs": self.envs, "compared": self.compared, "entries": int(rel.size), "lanes": sorted(self.lanes), "layouts": sorted(self.layouts),
              "reached": sorted(self.reached), "above_floor": self.above, "limit_models": {k: sorted(self.models[k]) for k in LIMIT_KINDS},
              "rel_q": q(rel), "over_S_q": q(ov), "share_within_1e-6_S": float(np.mean(ov <= F64_SHARE)) if ov.size else None,
              "share_within_1e-4_S": float(np.mean(ov <= F32_99)) if ov.size else None, "worst": sorted(self.worst, reverse=True)[:6]}
        print(what, json.dumps(st))
        if STATS:
            os.makedirs(STATS, exist_ok=True)
            with open(os.path.join(STATS, "bpg_oracle_%s.json" % what), "w") as f:
                json.dump(st, f, indent=0)
        assert self.compared >= min_share * self.envs and self.compared > 0, (what, st)
        for k in kinds:
            assert self.above[k] >= min_count, (what, k, st)
        if limit_models:                           # every limit kind from limit_push and from one other model
            for k in LIMIT_KINDS:
                assert "limit_push" in self.models[k] and len(self.models[k]) >= 2, (what, k, st)
        if self.fp64:
            assert rel.max() <= F64_BOUND, (what, st)
            assert np.mean(ov <= F64_SHARE) >= 0.99, (what, st)
        else:
            assert (np.mean(ov <= F32_99) >= 0.99 or not share) and ov.max() <= F32_MAX, (what, st)
        return st


def _compare_batch(tally, name, m, sim, rows, q0, qd0, u, S, w, envs, mode="episode", max_iter=None):
    """run the batch with every group on, then the oracle on the environments `envs` with their own rows; adds to tally"""
    if sim.dtype == torch.float32:                         # both sides start from the values the fp32 batch holds
        q0, qd0, u = (x.astype(np.float32).astype(np.float64) for x in (q0, qd0, u))
    tab = None if rows is None else torch.tensor(rows, device=DEV, dtype=sim.dtype)
    g, sig, status = gpu_episode(sim, tab, q0, qd0, u, S, w, groups=ALL, mode=mode)[:3]
    g, sig, status = g.double().cpu().numpy(), sig.cpu().numpy(), status.cpu().numpy()
    n = u.shape[1] * S
    tally.layouts.add(layout_kind(sim.B, n if mode == "episode" else S if mode == "steps" else (u.shape[1] - u.shape[1] // 2) * S))
    other = np.setdiff1d(np.arange(g.shape[1]), [c for (_, _, _, c) in m.param_columns() + m.body_param_columns()])
    assert np.all(g[:, other] == 0), name
    for e in envs:
        tally.envs += 1
        om = m if rows is None else row_model(m, rows[e].astype(np.float64))
        if max_iter:
            om = copy.copy(om)
            om.I = om.I.copy()
            om.I[Bl.TSIM_IH_MAX_ITER] = max(int(om.I[Bl.TSIM_IH_MAX_ITER]), max_iter)
        go, osig, obad, _ = oracle_cached(om, q0[e], qd0[e], u[e], S, w, groups=ALL)[1]
        if obad or status[e] != 0 or not np.array_equal(sig[:, e], osig):
            continue
        tally.add(m, g[e], go, name, (name, int(e)))


def _tol(m, fp64):
    m = copy.deepcopy(m)
    if fp64:
        m.F[Bl.TSIM_FH_TOL] = 1e-13
    return m


DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])


# ---------------------------------------------------------------------------------------------------- 1. generic kernels, every model
@DTYPES
@pytest.mark.parametrize("lanes", [16, 32, 64])
def test_generic_body_gradient_against_the_oracle(lanes, dtype):
    """the 17 models of the finite-difference yardstick and limit_chain (a second contact-free model with a dof below its lower and one above its
    upper limit: of the 17, the ones with a dof below its lower limit — large:L7, small:11 — do not keep the oracle's contact branches in fp32),
    B = 4, every environment with its own tables (every contact and body column scaled), every group on; a rotation-vector model has only the
    64-lane instantiation"""
    import random_corpus as RC
    fp64 = dtype == torch.float64
    tally, B, exp_seen = Tally(fp64), 4, False
    for name, T in MODELS + [LIMIT_CHAIN]:
        m, q0, qd0, u, S = body_case(name, B, T)
        m = _tol(m, fp64)
        exp_seen |= RC.has_exp_joint(m)
        sim = _sim(m, B, dtype, u.shape[1] * S, lanes, tally=tally)
        info = sim.launch_info()
        assert info["lanes_per_env"] == (64 if RC.has_exp_joint(m) else lanes) or (info["lanes_per_env"] > lanes and info["lds_bytes"] <= 64 * 1024), (name, info)
        assert sim.kernel_variant() == "generic" or name == "pusher"
        _compare_batch(tally, name, m, sim, table_rows(m, B, not fp64, 17), q0, qd0, u, S, loss_weights(m, u.shape[1]), range(B), max_iter=None if fp64 else 100)
    assert exp_seen and lanes in tally.lanes, tally.lanes
    tally.check("generic_%s_lpe%d" % ("fp64" if fp64 else "fp32", lanes), KINDS, limit_models=True)


# ---------------------------------------------------------------------------------------------------- 2. ragged batches
def _limit_push_case(B, T, seed):
    """limit_push with per-environment start states and controls around the case's own (both dofs stay in their limits)"""
    m, q0, qd0, u, S = body_case("limit_push", 1, 4)
    rng = np.random.default_rng(seed)
    q0 = np.tile(q0, (B, 1)) + 0.003 * rng.normal(size=(B, q0.shape[1]))
    u = np.tile(np.resize(u, (1, T, u.shape[2])), (B, 1, 1)) + 0.05 * rng.normal(size=(B, T, u.shape[2]))
    return m, q0, np.zeros_like(q0), np.clip(u, -0.98, 0.98), S


@DTYPES
@pytest.mark.parametrize("B,lanes", [(5, 16), (3, 32)])
def test_ragged_batches(B, lanes, dtype):
    """B is no multiple of the environments per wavefront: the last block's invalid slots run the loop on the last environment's records and store
    nothing.  limit_push (2 dofs: 4 / 2 slots per block) and ball_push (a rotation-vector joint: 64 lanes, one slot)"""
    fp64 = dtype == torch.float64
    tally = Tally(fp64)
    m, q0, qd0, u, S = _limit_push_case(B, 4, 7)
    m = _tol(m, fp64)
    sim = _sim(m, B, dtype, u.shape[1] * S, lanes, tally=tally)
    assert sim.launch_info()["lanes_per_env"] == lanes and B % (64 // lanes) != 0
    _compare_batch(tally, "limit_push", m, sim, table_rows(m, B, not fp64, 23), q0, qd0, u, S, loss_weights(m, u.shape[1]), range(B), max_iter=None if fp64 else 100)
    m, q0, qd0, u, S = body_case("ball_push", B, 4)
    m = _tol(m, fp64)
    sim = _sim(m, B, dtype, u.shape[1] * S, lanes, tally=tally)
    _compare_batch(tally, "ball_push", m, sim, table_rows(m, B, not fp64, 29), q0, qd0, u, S, loss_weights(m, u.shape[1]), range(B), max_iter=None if fp64 else 100)
    tally.reached.add("ragged B=%d lanes=%d" % (B, lanes))
    tally.check("ragged_B%d_lpe%d_%s" % (B, lanes, "fp64" if fp64 else "fp32"), KINDS)


# ---------------------------------------------------------------------------------------------------- 3. chunk layouts
def _batch_for(kind, n):
    """the smallest batch (4, or a multiple of 256) whose body pass over n sub-steps has the chunk layout `kind` on this device"""
    for B in [4] + list(range(256, 65536 + 1, 256)):
        if layout_kind(B, n) == kind:
            return B
    raise AssertionError("no batch size gives the %s layout for %d sub-steps on this device" % (kind, n))


def _sample(B, k, seed, last_block):
    """a seeded sample of k environments with the first, the last and others of the last block"""
    rng = np.random.default_rng(seed)
    fixed = {0, B - 1} | set(range(max(0, B - last_block), B))
    rest = [int(e) for e in rng.permutation(B) if e not in fixed]
    return np.array(sorted(fixed | set(rest[:max(0, k - len(fixed))])))


@DTYPES
@pytest.mark.parametrize("kind", ["single", "len1", "len1:256", "even", "ragged"])
def test_chunk_layouts_of_the_body_pass(kind, dtype):
    """limit_push (2 dofs, 2 links, a force and a position motor, both limits active), 8 frames x 2 sub-steps, per-environment states, controls and
    tables: one chunk; one sub-step per chunk; several sub-steps per chunk, all chunks full; a shorter last chunk.  With more than one sub-step
    per chunk the accumulators of k_param_grad_body run over the loop and the t - 1 record of a chunk's first sub-step belongs to the chunk before.
    Each layout at the smallest batch that has it (len1: B = 4).  The fp32 rule's 99 % is a share of a population, and 4 environments are 136
    entries, one environment 1.5 % of them (measured there: two entries of one environment at 2.7e-4 S_kind, 98.5 %): at B = 4 fp32 is held to
    the rule's maximum alone, and len1 runs a second time at B = 256 with 32 sampled environments like the other layouts, under the whole rule."""
    fp64 = dtype == torch.float64
    T, lanes = 8, 16
    tally = Tally(fp64)
    kind, _, forced = kind.partition(":")
    B = int(forced) if forced else _batch_for(kind, T * 2)
    m, q0, qd0, u, S = _limit_push_case(B, T, 41)
    assert S == 2 and layout_kind(B, T * S) == kind
    m = _tol(m, fp64)
    sim = _sim(m, B, dtype, T * S, lanes, tally=tally)
    envs = _sample(B, 32, B, 64 // lanes) if B > 32 else range(B)
    _compare_batch(tally, "limit_push", m, sim, table_rows(m, B, not fp64, 31), q0, qd0, u, S, loss_weights(m, T), envs, max_iter=None if fp64 else 100)
    assert tally.layouts == {kind}, tally.layouts
    nchunk, cl = pg_layout(B, T * S)
    tally.reached.add("layout %s: B=%d nchunk=%d chunk_len=%d" % (kind, B, nchunk, cl))
    tally.check("layout_%s_B%d_%s" % (kind, B, "fp64" if fp64 else "fp32"), KINDS, share=fp64 or B >= 32)


@pytest.mark.parametrize("B", [4096, 16384])
def test_chunk_layouts_on_the_headline_shape(B):
    """the inertial case on the headline instantiation: fp32 param:pusher, 16 lanes, 10 frames x 5 sub-steps, per-environment tables — the shapes of
    the contact pass's layout test (B = 4096: 4 chunks of 13, the last one short; B = 16384: one chunk); 40 sampled environments go to the oracle"""
    T = 10
    m, q0, qd0, u, S = pusher_case(B, T, seed=11)
    tally = Tally(False)
    sim = _sim(m, B, torch.float32, T * S, 16, static=True, tally=tally)
    rows = table_rows(m, B, True, 0)
    sim.set_env_tables(torch.tensor(rows, device=DEV))
    assert sim.kernel_variant() == "param:pusher"
    want = {4096: "ragged", 16384: "single"}[B]
    assert layout_kind(B, T * S) == want
    _compare_batch(tally, "pusher", m, sim, rows, q0, qd0, u, S, loss_weights(m, T), _sample(B, 40, B, 4), max_iter=100)
    assert sim.kernel_variant() == "param:pusher" and tally.layouts == {want} and tally.lanes == {16}
    tally.reached.add("headline B=%d %s" % (B, want))
    tally.check("headline_B%d" % B, PUSHER_KINDS)


# ---------------------------------------------------------------------------------------------------- 4. windows
@DTYPES
@pytest.mark.parametrize("mode", ["episode", "steps", "halves"])
def test_windows(mode, dtype):
    """the episode in one launch, frame by frame, and as two half-episodes into one buffer, on a BDF1 model and on bdf2:ball_push: the second
    half's first sub-step reads the t - 1 and t - 2 records the first half wrote"""
    fp64 = dtype == torch.float64
    tally = Tally(fp64)
    for name, T in (("limit_push", 4), ("ball_push", 4), ("bdf2:ball_push", 3)):
        m, q0, qd0, u, S = body_case(name, 4, T)
        m = _tol(m, fp64)
        if name.startswith("bdf2:"):
            assert int(m.I[Bl.TSIM_IH_INTEGRATOR]) == 2 and (T - T // 2) * S >= 2 and (T // 2) * S >= 2
        sim = _sim(m, 4, dtype, u.shape[1] * S, 32, tally=tally)
        _compare_batch(tally, name, m, sim, table_rows(m, 4, not fp64, 37), q0, qd0, u, S, loss_weights(m, u.shape[1]), range(4), mode=mode,
                       max_iter=None if fp64 else 100)
    tally.reached.add("window %s" % mode)
    tally.check("window_%s_%s" % (mode, "fp64" if fp64 else "fp32"), KINDS)


# ---------------------------------------------------------------------------------------------------- 5. compiled-in
@pytest.mark.parametrize("variant,dtype", [("static", torch.float64), ("static", torch.float32), ("param_edited", torch.float64)])
def test_compiled_in_body_gradient_against_the_oracle(variant, dtype):
    """static:pusher on the asset as shipped, against the oracle at the asset's own Newton tolerance (the exact adjoint is taken at the iterate
    the solve stopped at, so the tolerance does not enter); param:pusher fp64 on an edited model"""
    fp64 = dtype == torch.float64
    tally = Tally(fp64)
    B, T = 8, 4
    m, q0, qd0, u, S = pusher_case(B, T)
    if variant == "param_edited":
        m = copy.deepcopy(m)
        m.F[m.I[Bl.TSIM_IH_FOFF_PAIR] + Bl.TSIM_PF_KN] *= 1.5
        m.F[m.I[Bl.TSIM_IH_FOFF_DOF] + Bl.TSIM_DF_DAMPING] = 0.7
        m.F[m.I[Bl.TSIM_IH_FOFF_LINK] + (int(m.I[Bl.TSIM_IH_NL]) - 1) * Bl.TSIM_LF_SIZE + Bl.TSIM_LF_MASS] *= 1.3      # the last link: the box
        m.F[Bl.TSIM_FH_TOL] = 1e-13
    want = {"static": "static:pusher", "param_edited": "param:pusher"}[variant]
    sim = _sim(m, B, dtype, T * S, 32, static=True, tally=tally)
    assert sim.kernel_variant() == want, (sim.kernel_variant(), want)
    _compare_batch(tally, "pusher", m, sim, None, q0, qd0, u, S, loss_weights(m, T), range(B), max_iter=None if fp64 else 100)
    assert sim.kernel_variant() == want
    tally.check("%s_%s" % (variant, "fp64" if fp64 else "fp32"), PUSHER_KINDS)
