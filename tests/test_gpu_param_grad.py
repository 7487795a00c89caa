"""Gradients w.r.t. the contact, tactile and damping parameters of the numeric tables (include/tsim.h tsim_set_param_grad, BatchSim.set_param_grad,
functions.BatchedEpisodicParamSimFunction).

The reference's boundary has the slot (backward_info.set_flags(flag_p=...) / backward_results.df_dp, envs/redmax_torch_functions.py:83,151); here it is
batched: every environment's gradient w.r.t. its own row of the per-environment tables.  The values are held against central finite differences of
the kernels themselves (one batch: row 0 the base, rows 2k+1 / 2k+2 the base with column k moved by +-h), against finite differences of the fp64
CPU oracle on edited blobs, and against one-environment batches of separately edited models.  The stick / slip switch of the friction law is a kink,
so a finite difference is compared only where the branch signature (tsim_debug_signature) of the base and of both moved rows is the same.
The rest: nothing existing changes while the gradient is asked for (bit for bit), bookkeeping (episode vs steps, accumulation, determinism, the
backward cache), fp32 against fp64, the torch surface and a short parameter identification."""
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
from tactilesimulation_amd.model.compiler import load_model      # noqa: E402
from tactilesimulation_amd.workloads import asset, push_workload      # noqa: E402
from param_grad_util import bdf2_case, fixed_case as _case, gpu_episode      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATS = os.environ.get("TSIM_PG_STATS")      # a directory: the finite-difference error distributions are written there as JSON (profiles/)


def _sim(m, B, dtype=torch.float64, cap=64, static=False, lanes=0):
    from tactilesimulation_amd.host.batch import BatchSim
    sim = BatchSim(m, B, device=DEV, dtype=dtype, tape_capacity=cap)
    sim.set_static(static)
    if lanes:
        sim.set_lanes_per_env(lanes)
    return sim


def _loss_weights(m, T, nm, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(T, m.ndof_r)), rng.normal(size=(T, m.ndof_var)), rng.normal(size=(nm, m.ndof_tactile)))


def _run(sim, tab, q0, u, S, w, grad=True, episode=True):
    """forward of the episode + its adjoint with the table gradient: (loss per env, table gradient, signatures, status, outputs, df_du, adjoint)"""
    g, sig, status, out, du, adj = gpu_episode(sim, tab, q0, None, u, S, w, mode="episode" if episode else "steps", grad=grad)
    wq, wv, wt = (torch.tensor(x, device=DEV, dtype=sim.dtype).unsqueeze(1) for x in w)
    L = (out["q"].double() * wq.double()).sum((0, 2))
    if sim.ndof_var:
        L = L + (out["var"].double() * wv.double()).sum((0, 2))
    if sim.ndof_tactile:
        L = L + (out["tactile"].double() * wt.double()).sum((0, 2))
    return L, g, sig, status, out, du, adj


FD_MODELS = ["pusher", "tactile_insertion", "stable_grasp", "dclaw_position_control", "tactile_pad", "box_slide", "pad_press", "sphere_rest",
             "slider_push", "ball_push"] + ["random%d" % k for k in range(20)]


def _fd_compare(m, q0, u, S, nbase=2, hrel=1e-4, tol=1e-13, detail=None):
    """Central differences at steps h and h / 2, Richardson-extrapolated ((4 D(h/2) - D(h)) / 3: no h^2 term), of the kernels' own episode loss, in
    ONE batch: per base environment the base row and four moved rows per column.  h = hrel max(|p|, 1): a damping of 0 is moved by 1e-4, not by
    nothing (the converged solves' residual noise over 2h must stay far below the difference)."""
    m = copy.deepcopy(m)
    m.F[Bl.TSIM_FH_TOL] = tol
    pcols = m.param_columns()
    cols = [c for (_, _, _, c) in pcols]
    K = len(cols)
    R = 1 + 4 * K
    sim = _sim(m, nbase * R, cap=u.shape[1] * S)
    tab = sim.base_tables()
    n = tab.shape[1]
    base = tab[0].clone()
    hs = []
    for k, c in enumerate(cols):
        p = float(base[c])
        h = hrel * max(abs(p), 1.0)
        hs.append(h)
        for b_ in range(nbase):
            r = b_ * R + 1 + 4 * k
            tab[r, c], tab[r + 1, c], tab[r + 2, c], tab[r + 3, c] = p + h, p - h, p + h / 2, p - h / 2
    q0b = np.repeat(q0[:nbase], R, axis=0)
    ub = np.repeat(u[:nbase], R, axis=0)
    w = _loss_weights(m, u.shape[1], u.shape[1], seed=1)
    L, g, sig, status, _, _, _ = _run(sim, tab, q0b, ub, S, w)
    L, g, sig, status = L.cpu().numpy(), g.double().cpu().numpy(), sig.cpu().numpy(), status.cpu().numpy()
    errs = []
    for b_ in range(nbase):
        r0 = b_ * R
        scale = np.abs(g[r0, cols]).max()
        if scale == 0:
            continue
        for k, c in enumerate(cols):
            rows = [r0] + [r0 + 1 + 4 * k + i for i in range(4)]
            if any(status[r] != 0 for r in rows) or not all(np.array_equal(sig[:, r0], sig[:, r]) for r in rows[1:]):
                continue
            d1 = (L[rows[1]] - L[rows[2]]) / (2 * hs[k])
            d2 = (L[rows[3]] - L[rows[4]]) / hs[k]
            fd = (4 * d2 - d1) / 3
            errs.append(abs(fd - g[r0, c]) / scale)
            if detail is not None:
                detail.append({"base": b_, "column": "%s %s %s" % pcols[k][:3], "p": float(base[c]), "h": hs[k], "fd": float(fd), "fd_h": float(d1),
                               "grad": float(g[r0, c]), "scale": float(scale), "err": float(errs[-1])})
    # entries outside the parameter columns stay exactly zero
    other = np.setdiff1d(np.arange(n), cols)
    assert np.all(g[:, other] == 0)
    return np.array(errs), nbase * K


@pytest.mark.parametrize("name", FD_MODELS)
def test_table_gradient_equals_finite_differences_fp64(name):
    m, q0, u, S = _case(name, 2)
    detail = []
    errs, total = _fd_compare(m, q0, u, S, detail=detail)
    if STATS:
        os.makedirs(STATS, exist_ok=True)
        with open(os.path.join(STATS, "fd_%s.json" % name), "w") as f:
            json.dump({"model": name, "pairs": total, "compared": int(errs.size), "errors": sorted(float(e) for e in errs),
                       "worst": sorted(detail, key=lambda d: -d["err"])[:5]}, f, indent=0)
    if errs.size == 0:
        pytest.skip("no (env, column) pair with an unchanged branch signature")
    assert np.mean(errs <= 1e-6) >= 0.99 and errs.max() <= 1e-3, (name, errs.size, np.quantile(errs, [0.5, 0.99]), errs.max())


def test_pusher_gradient_against_oracle_finite_differences():
    """No GPU arithmetic in the reference value: central differences of the fp64 CPU oracle on blobs edited at table_offset, all 19 columns."""
    from oracle.oracle import OracleSim
    m, q0, u, S = _case("pusher", 1)
    m = copy.deepcopy(m)
    m.F[Bl.TSIM_FH_TOL] = 1e-13
    T = 6
    u = u[:, :T]
    cols = m.param_columns()
    w = _loss_weights(m, T, T, seed=2)
    sim = _sim(m, 1, cap=T * S)
    _, g, _, status, _, _, _ = _run(sim, None, q0, u, S, w)
    assert int(status[0]) == 0
    g = g.double().cpu().numpy()[0]

    def oracle_loss(mm):
        o = OracleSim(mm)
        o.reset(q0[0], record=False)
        L = 0.0
        for t in range(T):
            o.forward(u[0, t], S)
            q, _ = o.state()
            var, tac = o.outputs()
            L += float(w[0][t] @ q) + float(w[1][t] @ var) + float(w[2][t] @ tac)
        return L
    scale = max(abs(g[c]) for (_, _, _, c) in cols)
    errs = []
    for (_, _, _, c) in cols:
        p = m.F[c]
        h = 1e-6 * abs(p) if p != 0 else 1e-6
        mp, mm_ = copy.deepcopy(m), copy.deepcopy(m)
        mp.F[c] = p + h
        mm_.F[c] = p - h
        fd = (oracle_loss(mp) - oracle_loss(mm_)) / (2 * h)
        errs.append(abs(fd - g[c]) / scale)
    errs = np.array(errs)
    if STATS:
        with open(os.path.join(STATS, "oracle_fd_pusher.json"), "w") as f:
            json.dump({"errors": [float(e) for e in errs]}, f)
    assert np.mean(errs <= 1e-6) >= 0.99 and errs.max() <= 1e-3, errs


VARIANTS = [("generic", torch.float64, 0), ("generic", torch.float64, 32), ("generic", torch.float64, 16), ("generic", torch.float32, 0),
            ("generic", torch.float32, 32), ("generic", torch.float32, 64), ("static", torch.float32, 16), ("static", torch.float64, 0),
            ("param", torch.float32, 16), ("param", torch.float32, 32)]      # (param:pusher is fp32 only: fp64 batches with tables stay generic)


@pytest.mark.parametrize("episode", [True, False])
@pytest.mark.parametrize("variant,dtype,lanes", VARIANTS)
def test_nothing_existing_changes_with_the_gradient_on(variant, dtype, lanes, episode):
    """With the buffer set vs unset: forward outputs, df_du, dL/dq0, dL/dqd0 bit-identical (the adjoint launch is the SAVEZ twin of the same variant)"""
    m, q0, u, S = _case("pusher", 8)
    u = u[:, :6]
    sim = _sim(m, 8, dtype=dtype, cap=6 * S, static=variant != "generic", lanes=lanes)
    tab = None
    if variant == "param":
        tab = sim.base_tables()
        tab[:, m.table_offset("pair", ("tactile_pad_left", "box"), "kn")] *= torch.linspace(0.8, 1.2, 8, device=DEV, dtype=dtype)
    want = {"generic": "generic", "static": "static:pusher", "param": "param:pusher"}[variant]
    if variant == "static" and dtype == torch.float64 and os.environ.get("TSIM_LPE") == "16":
        want = "generic"      # (an fp64 batch forced to 16 lanes per environment has no compiled-in instantiation: include/tsim.h)
    if tab is not None:
        sim.set_env_tables(tab)
    assert sim.kernel_variant() == want
    w = _loss_weights(m, 6, 6)
    a = _run(sim, tab, q0, u, S, w, grad=False, episode=episode)
    b = _run(sim, tab, q0, u, S, w, grad=True, episode=episode)
    for k in ("q", "qd", "var", "tactile", "status"):
        assert torch.equal(a[4][k], b[4][k]), k
    assert torch.equal(a[5], b[5]) and torch.equal(a[6][0], b[6][0]) and torch.equal(a[6][1], b[6][1])
    assert torch.isfinite(b[1]).all() and b[1].abs().sum() > 0


@pytest.mark.parametrize("name", ["tactile_pad", "ball_push"])
def test_nothing_existing_changes_on_bdf2(name):
    m, q0, u, S = bdf2_case(name)
    for dtype in (torch.float64, torch.float32):
        sim = _sim(m, q0.shape[0], dtype=dtype, cap=u.shape[1] * S)
        w = _loss_weights(m, u.shape[1], u.shape[1])
        a = _run(sim, None, q0, u, S, w, grad=False)
        b = _run(sim, None, q0, u, S, w, grad=True)
        assert torch.equal(a[5], b[5]) and torch.equal(a[6][0], b[6][0]) and torch.equal(a[6][1], b[6][1])


def test_bdf2_gradient_equals_finite_differences():
    m, q0, u, S = bdf2_case("ball_push")
    errs, total = _fd_compare(m, q0, u[:, :6], S, nbase=1)
    assert errs.size > 0 and np.mean(errs <= 1e-6) >= 0.99 and errs.max() <= 1e-3, errs


def test_bookkeeping_episode_steps_halves_determinism_sentinel():
    m, q0, u, S = _case("pusher", 4)
    T = 8
    u = u[:, :T]
    w = _loss_weights(m, T, T)
    sim = _sim(m, 4, cap=T * S)
    g1 = _run(sim, None, q0, u, S, w)[1]
    g2 = _run(sim, None, q0, u, S, w, episode=False)[1]
    assert torch.allclose(g1, g2, rtol=1e-12, atol=1e-12 * float(g1.abs().max()))
    g3 = _run(sim, None, q0, u, S, w)[1]
    assert torch.equal(g1, g3)                                            # bit-identical from run to run
    # two half-episodes accumulating into one buffer
    sim.reset(torch.tensor(q0, device=DEV, dtype=torch.float64), None, backward_flag=True)
    ut = torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device=DEV, dtype=torch.float64)
    sim.rollout(ut, S)
    wq, wv, wt = (torch.tensor(x, device=DEV, dtype=torch.float64).unsqueeze(1).expand(-1, 4, -1).contiguous() for x in w)
    cols = [c for (_, _, _, c) in m.param_columns()]
    n = g1.shape[1]
    buf = torch.full((4, n), float("nan"), device=DEV, dtype=torch.float64)
    buf[:, cols] = 1.0
    sim.set_param_grad(buf)
    h = T // 2
    sim.backward_episode(T - h, S, wq[h:], wv[h:], wt[h:])
    sim.backward_episode(h, S, wq[:h], wv[:h], wt[:h])
    sim.set_param_grad(None)
    torch.cuda.synchronize()
    other = [c for c in range(n) if c not in cols]
    assert torch.isnan(buf[:, other]).all()                               # untouched
    assert torch.allclose(buf[:, cols] - 1.0, g1[:, cols], rtol=1e-12, atol=1e-12 * float(g1.abs().max()))


def test_backward_cache_gives_each_episode_its_own_gradient():
    m, q0, u, S = _case("pusher", 4)
    T = 6
    w = _loss_weights(m, T, T)
    sim = _sim(m, 4, cap=T * S)
    gA = _run(sim, None, q0, u[:, :T], S, w)[1]
    gB = _run(sim, None, q0, u[:, T:2 * T], S, w)[1]
    wq, wv, wt = (torch.tensor(x, device=DEV, dtype=torch.float64).unsqueeze(1).expand(-1, 4, -1).contiguous() for x in w)
    sim.cache_reserve(2)
    for uu in (u[:, :T], u[:, T:2 * T]):
        sim.reset(torch.tensor(q0, device=DEV, dtype=torch.float64), None, backward_flag=True)
        sim.rollout(torch.tensor(np.ascontiguousarray(uu.transpose(1, 0, 2)), device=DEV, dtype=torch.float64), S)
        sim.cache_save()
    for want in (gB, gA):
        sim.cache_pop()
        g = torch.zeros_like(want)
        sim.set_param_grad(g)
        sim.backward_episode(T, S, wq, wv, wt)
        sim.set_param_grad(None)
        torch.cuda.synchronize()
        assert torch.equal(g, want)


def test_per_environment_rows_equal_separately_edited_models():
    name = "tactile_insertion"
    m, q0, u, S = _case(name, 4)
    u = u[:, :8]
    T = u.shape[1]
    rng = np.random.default_rng(4)
    sim = _sim(m, 4, cap=T * S)
    tab = sim.base_tables()
    cols = [c for (_, _, _, c) in m.param_columns()]
    tab[:, cols] *= torch.tensor(rng.uniform(0.8, 1.25, size=(4, len(cols))), device=DEV, dtype=torch.float64)
    w = _loss_weights(m, T, T)
    g = _run(sim, tab, q0, u, S, w)[1].cpu().numpy()
    rows = tab.cpu().numpy()
    n = rows.shape[1]
    for e in range(4):
        me = copy.deepcopy(m)
        me.F[:n] = rows[e]
        one = _sim(me, 1, cap=T * S)
        g1 = _run(one, None, q0[e:e + 1], u[e:e + 1], S, w)[1].cpu().numpy()[0]
        assert np.allclose(g[e], g1, rtol=1e-12, atol=1e-12 * np.abs(g1).max()), e


def test_fp32_headline_config_against_fp64():
    """pusher, B = 4096, param:pusher with tables: on the environments whose fp32 and fp64 branch signatures are equal, >= 99 % of the entries
    within 1e-4 of the env's fp64 gradient scale"""
    B = 4096
    m = load_model(asset("pusher"))
    q0, u, _ = push_workload(B, 10, seed=11)
    S = 5
    rng = np.random.default_rng(0)
    cols = [c for (_, _, _, c) in m.param_columns()]
    res = {}
    for dt in (torch.float32, torch.float64):
        sim = _sim(m, B, dtype=dt, cap=10 * S, static=True)
        tab = sim.base_tables().double()
        tab[:, cols] *= torch.tensor(np.random.default_rng(0).uniform(0.8, 1.25, size=(B, len(cols))), device=DEV)
        tab = tab.to(dt)
        sim.set_env_tables(tab)
        if dt == torch.float32:
            assert sim.kernel_variant() == "param:pusher"
        res[dt] = _run(sim, tab, q0, u, S, _loss_weights(m, 10, 10))
    g32, g64 = res[torch.float32][1].double().cpu().numpy()[:, cols], res[torch.float64][1].cpu().numpy()[:, cols]
    same = (res[torch.float32][2] == res[torch.float64][2]).all(2).all(0).cpu().numpy()
    same &= (res[torch.float32][3] == 0).cpu().numpy() & (res[torch.float64][3] == 0).cpu().numpy()
    scale = np.abs(g64).max(1, keepdims=True) + 1e-300
    err = (np.abs(g32 - g64) / scale)[same]
    if STATS:
        with open(os.path.join(STATS, "fp32_headline.json"), "w") as f:
            json.dump({"envs_same_signature": int(same.sum()), "quantiles": [float(x) for x in np.quantile(err, [0.5, 0.9, 0.99, 1.0])]}, f)
    assert same.mean() > 0.5 and np.mean(err <= 1e-4) >= 0.99, (same.mean(), np.quantile(err, [0.5, 0.99, 1.0]))


LARGE_PG = ["large:L26", "large:L7", "large:L16", "large:L3", "large:L5", "large:L11"]      # ndof_r 13, 14, 15, 16, 16, 16


@pytest.mark.parametrize("lanes", [16, 32, 64])
def test_fp32_table_gradient_against_fp64_on_many_models(lanes):
    """k_param_grad<float> on the generic kernels against the fp64 kernels' table gradient (held to finite differences above) on the same inputs:
    every model of FD_MODELS and six of the large random corpus, 16 environments each with their own random scaling (0.8 - 1.25) of every
    parameter column.  Environments whose fp32 and fp64 branch signatures are equal and that both converged; per environment, relative to the
    largest fp64 entry of its row: >= 99 % within 1e-4, none above 1e-2; entries outside param_columns() exactly 0 in fp32 as well."""
    B = 16
    errs, worst, total = [], [], 0
    for name in FD_MODELS + LARGE_PG:
        m, q0, u, S = _case(name, B)
        cols = [c for (_, _, _, c) in m.param_columns()]
        if not cols:
            continue
        T = u.shape[1]
        fac = np.random.default_rng(17).uniform(0.8, 1.25, size=(B, len(cols)))
        res = {}
        for dt in (torch.float32, torch.float64):
            sim = _sim(m, B, dtype=dt, cap=T * S, lanes=lanes)
            tab = sim.base_tables().double()
            tab[:, cols] *= torch.tensor(fac, device=DEV)
            tab = tab.to(dt)
            res[dt] = _run(sim, tab, q0, u, S, _loss_weights(m, T, T))
        g32, g64 = res[torch.float32][1].double().cpu().numpy(), res[torch.float64][1].cpu().numpy()
        assert np.all(g32[:, np.setdiff1d(np.arange(g32.shape[1]), cols)] == 0), name
        g32, g64 = g32[:, cols], g64[:, cols]
        same = (res[torch.float32][2] == res[torch.float64][2]).all(2).all(0).cpu().numpy()
        same &= (res[torch.float32][3] == 0).cpu().numpy() & (res[torch.float64][3] == 0).cpu().numpy()
        scale = np.abs(g64).max(1)
        ok = same & (scale > 0)
        total += B
        e = np.abs(g32 - g64).max(1)[ok] / scale[ok]
        errs += list(e)
        worst += [(float(x), name, int(i)) for x, i in zip(e, np.nonzero(ok)[0])]
    errs = np.array(errs)
    worst.sort(reverse=True)
    if STATS:
        with open(os.path.join(STATS, "fp32_many_models_lpe%d.json" % lanes), "w") as f:
            json.dump({"envs": total, "compared": len(errs), "quantiles": [float(x) for x in np.quantile(errs, [0.5, 0.9, 0.99, 1.0])], "worst": worst[:10]}, f)
    assert len(errs) >= 0.6 * total and np.mean(errs <= 1e-4) >= 0.99 and errs.max() <= 1e-2, (len(errs), total, np.quantile(errs, [0.5, 0.99, 1.0]), worst[:5])


def test_torch_function_surface():
    from tactilesimulation_amd.functions import BatchedEpisodicSimFunction, BatchedEpisodicParamSimFunction
    m, q0, u, S = _case("pusher", 4)
    T = 6
    u = u[:, :T]
    sim = _sim(m, 4, cap=T * S)
    w = _loss_weights(m, T, T)
    wq, wv, wt = (torch.tensor(x, device=DEV, dtype=torch.float64).unsqueeze(1).expand(-1, 4, -1) for x in w)
    mask = torch.ones(T, dtype=torch.bool)

    def inputs():
        a = torch.tensor(q0, device=DEV, dtype=torch.float64, requires_grad=True)
        b = torch.zeros_like(a, requires_grad=True)
        c = torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device=DEV, dtype=torch.float64, requires_grad=True)
        return a, b, c
    tab = sim.base_tables()
    a1, b1, c1 = inputs()
    sim.set_env_tables(tab)
    qs, vs, ts = BatchedEpisodicSimFunction.apply(a1, b1, c1, mask, sim, True, S)
    ((qs * wq).sum() + (vs * wv).sum() + (ts * wt).sum()).backward()
    a2, b2, c2 = inputs()
    t2 = tab.clone().requires_grad_(True)
    qs, vs, ts = BatchedEpisodicParamSimFunction.apply(a2, b2, c2, t2, mask, sim, True, S)
    ((qs * wq).sum() + (vs * wv).sum() + (ts * wt).sum()).backward()
    assert torch.equal(a1.grad, a2.grad) and torch.equal(b1.grad, b2.grad) and torch.equal(c1.grad, c2.grad)
    g = _run(sim, tab, q0, u, S, w)[1]
    assert torch.equal(t2.grad, g)
    # the shared-parameter gradient through autograd's sum
    cols = [c for (_, _, _, c) in m.param_columns()]
    base = tab[0].clone().requires_grad_(True)
    qs, vs, ts = BatchedEpisodicParamSimFunction.apply(*inputs(), base.expand(4, -1), mask, sim, True, S)
    ((qs * wq).sum() + (vs * wv).sum() + (ts * wt).sum()).backward()
    assert torch.allclose(base.grad, g.sum(0), rtol=1e-12, atol=1e-12 * float(g.abs().max()))
    # a map from a few parameters (log scale of the pad's kn, kt and damping) into the tables: gradcheck
    idx = [m.table_offset("pair", ("tactile_pad_left", "box"), f) for f in ("kn", "kt", "damping")]
    T2 = 3

    def f(logs):
        tb = tab[:2].clone()
        tb[:, idx] = tb[:, idx] * torch.exp(logs)
        a = torch.tensor(q0[:2], device=DEV, dtype=torch.float64)
        c = torch.tensor(np.ascontiguousarray(u[:2, :T2].transpose(1, 0, 2)), device=DEV, dtype=torch.float64)
        qs, vs, ts = BatchedEpisodicParamSimFunction.apply(a, torch.zeros_like(a), c, tb, torch.ones(T2, dtype=torch.bool), sim2, True, S)
        return (qs * wq[:T2, :2]).sum() + (vs * wv[:T2, :2]).sum() + (ts * wt[:T2, :2]).sum()
    mm = copy.deepcopy(m)
    mm.F[Bl.TSIM_FH_TOL] = 1e-13
    sim2 = _sim(mm, 2, cap=T2 * S)
    # (torch.autograd.gradcheck's own numerical part, by hand: its re-entrancy probe runs backward twice on one forward, and an episodic function
    # pops its tape in backward — once per forward, like the reference's popBackwardCache)
    logs = torch.zeros(2, 3, device=DEV, dtype=torch.float64, requires_grad=True)
    f(logs).backward()
    ana = logs.grad.clone()
    num = torch.zeros_like(ana)
    with torch.no_grad():
        for i in range(2):
            for j in range(3):
                d = torch.zeros_like(logs); d[i, j] = 1e-6
                num[i, j] = (f(logs + d) - f(logs - d)) / 2e-6
    assert torch.allclose(ana, num, rtol=1e-4, atol=1e-5 * float(num.abs().max())), (ana, num)


def test_captured_backward_replays_to_eager():
    m, q0, u, S = _case("pusher", 8)
    T = 4
    u = u[:, :T]
    sim = _sim(m, 8, dtype=torch.float32, cap=T * S, static=True)
    w = _loss_weights(m, T, T)
    wq, wv, wt = (torch.tensor(x, device=DEV, dtype=torch.float32).unsqueeze(1).expand(-1, 8, -1).contiguous() for x in w)
    q0t = torch.tensor(q0, device=DEV, dtype=torch.float32)
    ut = torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device=DEV, dtype=torch.float32)
    n = sim.base_tables().shape[1]
    g = torch.zeros(8, n, device=DEV, dtype=torch.float32)

    def body():
        sim.reset(q0t, None, backward_flag=True)
        sim.rollout(ut, S)
        g.zero_()
        sim.set_param_grad(g)
        sim.backward_episode(T, S, wq, wv, wt)
        sim.set_param_grad(None)
    body()
    torch.cuda.synchronize()
    eager = g.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    g.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g, eager)


def test_identification_recovers_contact_parameters():
    """Short form of examples/identify_contact_params.py: tactile frames recorded at per-environment true parameters, fitted from mid-range values by
    Adam on log-parameters through BatchedEpisodicParamSimFunction."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
    import identify_contact_params as ic
    r = ic.identify(B=8, iters=400, device=DEV, verbose=False)
    if STATS:
        with open(os.path.join(STATS, "identification.json"), "w") as f:
            tl = lambda v: {k: tl(x) for k, x in v.items()} if isinstance(v, dict) else (v.tolist() if hasattr(v, "tolist") else v)
            json.dump(tl(r), f)
    assert r["loss"][-1] <= r["loss"][0] / 100, (r["loss"][0], r["loss"][-1])
    ok = r["stable"]
    assert ok.sum() >= 4, ok
    for f in ("kn", "kt"):
        assert np.all(r["rel_err"][f][ok] <= 0.02), (f, r["rel_err"][f][ok])
    # The sensor's damping and mu are NOT asserted: measured (profiles/r07_param_grad.md), the pressed taxels' normal velocity is so small in these
    # frames that kd dd d is below the fit's resolution (errors 8 % - 400 %), and mu shows only on the few slipping taxels.
