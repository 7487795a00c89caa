"""Kernels against the fp64 oracle on RANDOM models: kinematic forests with every joint and primitive body kind, random joint and body frames,
ground and general-primitive contacts, force and position motors, rect_array sensors, end-effectors, BDF1 / BDF2 (the generator of
tests/test_native_model_loader.py, which holds the two model compilers against each other on the same models).  The fixed models of the other GPU
tests cover the structures the reference's assets have; this covers the ones they do not (a planar joint under a tilted revolute, prismatic chains,
several sensors on one link ...).  fp64 generic kernels, a few env-steps from rest under random controls: state, variables, tactile frame and the
adjoint of a random functional, to the oracle.  (fp32 kernels: with the models' random scales a third of them cannot reach the drawn `tol` in
single precision and flag the sub-step — the last test of the file runs them with `tol` 1e-5 and bounds the error distribution; the fp32 envelope
proper is the reference's assets, tests/test_gpu_parity.py.)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tactilesimulation_amd", "compat"))      # `import redmax_py`
import random_corpus as RC      # noqa: E402
from random_corpus import N_MODELS, SEED0      # noqa: E402,F401

pytestmark = pytest.mark.gpu
B_, T, S = 3, 3, 2
LARGE = RC.LARGE + ["chain16"]      # ndof_r 13 .. 16 (tests/random_corpus.py)


def _case(case, tmp_path, files=False):
    """(model, rng) of a corpus case: an int of the small corpus (seed SEED0 + case), a large-corpus id or "chain16" (tests/random_corpus.py)"""
    r = RC.draw(case, tmp_path, files)
    if r is None:
        pytest.skip("no model within the kernels' sizes")
    return r


@pytest.mark.parametrize("lanes,dtype,files", [(0, torch.float64, False), (32, torch.float64, False), (16, torch.float64, False), (0, torch.float64, True), (32, torch.float64, True)])
@pytest.mark.parametrize("seed", list(range(N_MODELS)) + LARGE)
def test_random_model_follows_the_oracle(seed, lanes, dtype, files, tmp_path):
    """files: abstract bodies with contact-point files as general bodies, abstract taxel files as sensors (the D'Claw vocabulary)"""
    from oracle.oracle import OracleSim
    from tactilesimulation_amd.host.batch import BatchSim
    m, rng = _case(seed, tmp_path, files)
    nr, nu, nv, nt = m.ndof_r, m.ndof_u, m.ndof_var, m.ndof_tactile
    q0 = 0.02 * rng.normal(size=(B_, nr))
    u = rng.uniform(-1, 1, size=(B_, T, max(nu, 1)))[:, :, :nu]
    wq, wv, wt = rng.normal(size=(B_, nr)), rng.normal(size=(B_, nv)), rng.normal(size=(B_, nt))
    dev, dt = "cuda:0", dtype
    f32 = dtype == torch.float32
    tq, tg = (2e-4, 2e-3) if f32 else (1e-8, 1e-7)      # state / gradient tolerance relative to the scale of the quantity (fp32: the BASELINE 1e-4 with a margin for models nobody tuned)
    sim = BatchSim(m, B_, dtype=dt, tape_capacity=T * S)
    if lanes:      # two / four environments per wavefront where the model's LDS footprint allows it (the library falls back otherwise)
        RC.force_lanes(sim, m, lanes)
    sim.reset(torch.tensor(q0, device=dev, dtype=dt), None, backward_flag=True)
    outs = [sim.step(torch.tensor(u[:, t], device=dev, dtype=dt).reshape(B_, nu), S, want_qd=True) for t in range(T)]
    if nv or nt:      # the on-demand read-out (tsim_readout: k_readout + k_taxels) of the final state == what the last step returned, bit for bit
        rv, rt = sim.readout(want_var=bool(nv), want_tactile=bool(nt))
        assert (not nv or torch.equal(rv, outs[-1]["var"])) and (not nt or torch.equal(rt, outs[-1]["tactile"])), seed
    outs = [{k: (v.double() if v.is_floating_point() else v).cpu().numpy() for k, v in o.items()} for o in outs]
    kw = {"df_dq": torch.tensor(wq, device=dev, dtype=dt)}
    if nv:
        kw["df_dvar"] = torch.tensor(wv, device=dev, dtype=dt)
    if nt:
        kw["df_dtactile"] = torch.tensor(wt, device=dev, dtype=dt)
    du = sim.backward_steps(T * S, **kw).double().cpu().numpy()
    lam_q, lam_v = (x.double().cpu().numpy() for x in sim.get_adjoint())      # dL/dq0, dL/dqdot0 (backward() + backward_results.df_dq0 / df_dqdot0)
    o = OracleSim(m)
    compared = 0
    for e in range(B_):
        o.reset(q0[e], record=True)
        clean = True
        for t in range(T):
            it0 = o.stats()["newton_iters"]
            bad = o.forward(u[e, t], S)
            iters = o.stats()["newton_iters"] - it0
            q, qd = o.state()
            var, tac = o.outputs()
            kbad = outs[t]["status"][e] != 0
            if bad != 0 or kbad or not np.all(np.isfinite(q)):
                # A sub-step that exhausts max_iter ends on its last iterate, and a stagnating Newton iteration amplifies round-off by 2 - 3 x per
                # iteration (tools/random_model_iters.py: kernels and oracle take the SAME line-search decisions for 25 - 30 iterations while their
                # iterates drift apart from 1e-15 to 1e-3; then one of them may leave the plateau and converge where the other does not).  Both
                # flag the sub-step, or the one that converged needed a stagnation's worth of iterations for it; nothing after it is comparable.
                assert (bad != 0) == bool(kbad) or iters >= 6 * S, (seed, e, t, bad, int(outs[t]["status"][e]), iters)
                clean = False
                break
            scale = 1.0 + np.abs(q).max()
            assert np.allclose(outs[t]["q"][e], q, rtol=0, atol=tq * scale), (seed, e, t, np.abs(outs[t]["q"][e] - q).max())
            assert np.allclose(outs[t]["qd"][e], qd, rtol=0, atol=100 * tq * (1.0 + np.abs(qd).max())), (seed, e, t, np.abs(outs[t]["qd"][e] - qd).max())
            if nv:
                assert np.allclose(outs[t]["var"][e], var, rtol=0, atol=tq * scale), (seed, e, t)
            if nt:
                assert np.allclose(outs[t]["tactile"][e], tac, rtol=0, atol=10 * tq * (1.0 + np.abs(tac).max())), (seed, e, t, np.abs(outs[t]["tactile"][e] - tac).max())
            compared += 1
        if nu and clean:
            g = o.backward_steps(T * S, df_dq=np.concatenate([np.zeros((T * S - 1) * nr), wq[e]]), df_dvar=np.concatenate([np.zeros((T * S - 1) * nv), wv[e]]) if nv else None,
                                 df_dtac=np.concatenate([np.zeros((T * S - 1) * nt), wt[e]]) if nt else None)
            gs = 1.0 + np.abs(g).max()
            assert np.allclose(du[e].reshape(T * S, nu), g, rtol=0, atol=tg * gs), (seed, e, np.abs(du[e].reshape(T * S, nu) - g).max(), gs)
        if clean:
            if not nu:
                o.backward_steps(T * S, df_dq=np.concatenate([np.zeros((T * S - 1) * nr), wq[e]]), df_dvar=np.concatenate([np.zeros((T * S - 1) * nv), wv[e]]) if nv else None,
                                 df_dtac=np.concatenate([np.zeros((T * S - 1) * nt), wt[e]]) if nt else None)
            aq, av = o.adjoint()
            for mine, ref in ((lam_q[e], aq), (lam_v[e], av)):
                assert np.allclose(mine, ref, rtol=0, atol=tg * (1.0 + np.abs(ref).max())), (seed, e, np.abs(mine - ref).max(), np.abs(ref).max())
    if compared == 0:
        pytest.skip("every environment of this model hits max_iter in its first env-step")


@pytest.mark.parametrize("lanes,dtype", [(0, torch.float64), (32, torch.float64), (16, torch.float32), (32, torch.float32)])
@pytest.mark.parametrize("seed", list(range(0, N_MODELS, 3)) + LARGE)
def test_episode_launches_equal_the_step_loop_on_random_models(seed, lanes, dtype, tmp_path):
    """tsim_rollout + tsim_backward_episode (one launch each way per episode: free-running slots, helper slots, LPT order, deferred read-out)
    against T x tsim_step + tsim_backward_steps on the same random models — bit for bit, both precisions, ragged batch (11 environments, so that
    wavefronts carry 1 - 4 of them and the last one is partly empty), a tactile mask, per-frame seeds."""
    from tactilesimulation_amd.host.batch import BatchSim
    m, rng = _case(seed, tmp_path)
    nr, nu, nv, nt = m.ndof_r, m.ndof_u, m.ndof_var, m.ndof_tactile
    B2, T2, S2 = 11, 4, 3
    dev = "cuda:0"
    q0 = torch.tensor(0.02 * rng.normal(size=(B2, nr)), device=dev, dtype=dtype)
    u = torch.tensor(rng.uniform(-1, 1, size=(T2, B2, max(nu, 1)))[:, :, :nu], device=dev, dtype=dtype).contiguous()
    mask = torch.tensor([True, False, True, True])
    wq = torch.tensor(rng.normal(size=(T2, B2, nr)), device=dev, dtype=dtype)
    wv = torch.tensor(rng.normal(size=(T2, B2, nv)), device=dev, dtype=dtype) if nv else None
    wt = torch.tensor(rng.normal(size=(int(mask.sum()), B2, nt)), device=dev, dtype=dtype) if nt else None
    a, b = (BatchSim(m, B2, dtype=dtype, tape_capacity=T2 * S2) for _ in range(2))
    for sim in (a, b):
        if lanes:
            RC.force_lanes(sim, m, lanes)
        sim.reset(q0, None, backward_flag=True)
    ro = a.rollout(u, S2, want_qd=True, tactile_mask=mask)
    steps = [b.step(u[t], S2, want_qd=True) for t in range(T2)]
    for k in ("q", "qd") + (("var",) if nv else ()):
        assert torch.equal(ro[k], torch.stack([s_[k] for s_ in steps])), (seed, k)
    if nt:
        assert torch.equal(ro["tactile"], torch.stack([steps[t]["tactile"] for t in range(T2) if mask[t]])), seed
    bad = torch.stack([s_["status"] for s_ in steps]).ne(0).any(0)
    assert torch.equal(ro["status"].ne(0), bad), seed
    if nu == 0:
        return
    ga = a.backward_episode(T2, S2, df_dq=wq, df_dvar=wv, df_dtactile=wt, tactile_mask=mask)             # [T, B, nu]: dL/du of every env-step
    # the same seeds for tsim_backward_steps: [B, n, dim] per SUB-step, an env-step's outputs on its last sub-step
    def per_substep(w, dim, frames):
        full = torch.zeros(B2, T2 * S2, dim, device=dev, dtype=dtype)
        for j, t in enumerate(frames):
            full[:, t * S2 + S2 - 1] = w[j]
        return full
    kw = {"df_dq": per_substep(wq, nr, range(T2))}
    if nv:
        kw["df_dvar"] = per_substep(wv, nv, range(T2))
    if nt:
        kw["df_dtactile"] = per_substep(wt, nt, [t for t in range(T2) if mask[t]])
    gb = b.backward_steps(T2 * S2, all_steps=True, **kw)                                                     # [B, T*S, nu] per sub-step
    gb = gb.reshape(B2, T2, S2, nu).sum(2).transpose(0, 1)
    ok = ~bad
    if dtype == torch.float64:
        assert torch.allclose(ga[:, ok], gb[:, ok], rtol=1e-9, atol=1e-9 * (1.0 + float(gb[:, ok].abs().max()) if ok.any() else 1.0)), seed
    else:
        assert torch.allclose(ga[:, ok], gb[:, ok], rtol=1e-3, atol=1e-3 * (1.0 + float(gb[:, ok].abs().max()) if ok.any() else 1.0)), seed


@pytest.mark.parametrize("lanes", [0, 32])
@pytest.mark.parametrize("seed", range(1, N_MODELS, 3))
def test_per_environment_tables_equal_separately_edited_models_on_random_models(seed, lanes, tmp_path):
    """tsim_set_env_tables on the generic kernels: every environment of a batch with its own numeric tables (contact / tactile parameters AND primitive
    shapes, joint damping and limits, link masses and inertias, motor gains — what the update_* randomisers of the reference's envs touch, all at once)
    runs what a batch of the model edited to that row runs — state, tactile frame, adjoint.  (The pair cull and the sweep schedule are built by the
    host from the SHARED model: an environment whose primitive is larger than the shared one must not lose contacts to them.)"""
    import copy
    import tactilesimulation_amd.model.blob as BL
    from tactilesimulation_amd.host.batch import BatchSim
    m, rng = _case(seed, tmp_path)
    nr, nu, nv, nt = m.ndof_r, m.ndof_u, m.ndof_var, m.ndof_tactile
    Bt, Tt, St = 5, 3, 2
    dev, dt = "cuda:0", torch.float64
    sim = BatchSim(m, Bt, dtype=dt, tape_capacity=Tt * St)
    if lanes:
        sim.set_lanes_per_env(lanes)
    tab = sim.base_tables()
    n = tab.shape[1]
    I = m.I
    cols = []
    for p_ in range(int(I[BL.TSIM_IH_NPAIR])):
        o_ = int(I[BL.TSIM_IH_FOFF_PAIR]) + p_ * BL.TSIM_PF_SIZE
        cols += [o_ + BL.TSIM_PF_SHAPE + k for k in range(4)] + [o_ + BL.TSIM_PF_KN + k for k in range(4)]
    for s_ in range(int(I[BL.TSIM_IH_NSENSOR])):
        cols += [int(I[BL.TSIM_IH_FOFF_SENSOR]) + s_ * BL.TSIM_SF_SIZE + k for k in range(4)]
    for d in range(nr):
        cols += [int(I[BL.TSIM_IH_FOFF_DOF]) + d * BL.TSIM_DF_SIZE + k for k in (BL.TSIM_DF_DAMPING, BL.TSIM_DF_LIM_K)]
    for l_ in range(int(I[BL.TSIM_IH_NL])):
        o_ = int(I[BL.TSIM_IH_FOFF_LINK]) + l_ * BL.TSIM_LF_SIZE
        cols += [o_ + BL.TSIM_LF_MASS] + [o_ + BL.TSIM_LF_INERTIA + k for k in range(6)]
    for k in range(nu):
        cols += [int(I[BL.TSIM_IH_FOFF_MOTOR]) + k * BL.TSIM_MF_SIZE + j for j in (BL.TSIM_MF_P, BL.TSIM_MF_D)]
    cols = [c for c in cols if c < n]
    scale = torch.tensor(rng.uniform(0.7, 1.4, size=(Bt, len(cols))), device=dev, dtype=dt)
    # (a link's mass and inertia scale together, so that the inertia stays one of a body: one factor per link and environment)
    tab[:, cols] = tab[:, cols] * scale
    for l_ in range(int(I[BL.TSIM_IH_NL])):
        o_ = int(I[BL.TSIM_IH_FOFF_LINK]) + l_ * BL.TSIM_LF_SIZE
        fac = torch.tensor(rng.uniform(0.7, 1.4, size=(Bt, 1)), device=dev, dtype=dt)
        base = torch.tensor(m.F[o_ + BL.TSIM_LF_MASS:o_ + BL.TSIM_LF_INERTIA + 6], device=dev, dtype=dt)
        tab[:, o_ + BL.TSIM_LF_MASS] = base[0] * fac[:, 0]
        tab[:, o_ + BL.TSIM_LF_INERTIA:o_ + BL.TSIM_LF_INERTIA + 6] = base[BL.TSIM_LF_INERTIA - BL.TSIM_LF_MASS:] * fac
    sim.set_env_tables(tab)
    q0 = torch.tensor(0.02 * rng.normal(size=(Bt, nr)), device=dev, dtype=dt)
    u = torch.tensor(rng.uniform(-1, 1, size=(Tt, Bt, max(nu, 1)))[:, :, :nu], device=dev, dtype=dt).contiguous()
    wq = torch.tensor(rng.normal(size=(Bt, nr)), device=dev, dtype=dt)
    sim.reset(q0, None, backward_flag=True)
    outs = [sim.step(u[t], St, want_qd=True) for t in range(Tt)]
    du = sim.backward_steps(Tt * St, df_dq=wq)
    rows = tab.cpu().numpy()
    for e in range(Bt):
        me = copy.deepcopy(m)
        me.F[:n] = rows[e]
        one = BatchSim(me, 1, dtype=dt, tape_capacity=Tt * St)
        one.reset(q0[e:e + 1], None, backward_flag=True)
        clean = True
        for t in range(Tt):
            o1 = one.step(u[t, e:e + 1], St, want_qd=True)
            assert int(o1["status"][0] != 0) == int(outs[t]["status"][e] != 0), (seed, e, t)
            if o1["status"][0] != 0:
                clean = False
                break      # (a sub-step at max_iter: see the first test of this file)
            for k in ("q", "qd") + (("var",) if nv else ()) + (("tactile",) if nt else ()):
                a_, b_ = outs[t][k][e], o1[k][0]
                assert torch.allclose(a_, b_, rtol=0, atol=1e-7 * (1.0 + float(b_.abs().max()))), (seed, e, t, k, float((a_ - b_).abs().max()))      # (two launch shapes: other reduction orders, amplified by the stiffer of these models)
        if clean and nu:
            d1 = one.backward_steps(Tt * St, df_dq=wq[e:e + 1])
            assert torch.allclose(du[e], d1[0], rtol=0, atol=1e-6 * (1.0 + float(d1.abs().max()))), (seed, e, float((du[e] - d1[0]).abs().max()))


@pytest.mark.parametrize("seed", range(2, N_MODELS, 6))
def test_reference_call_sequence_on_random_model_files(seed, tmp_path):
    """The drop-in surface end to end on models nobody wrote by hand: `redmax_py.Simulation(xml_path)` (compat/redmax_py.py: what
    envs/redmax_torch_env.py:33 constructs) stepped and differentiated through StepSimFunction exactly as envs/redmax_torch_functions.py:115-174
    does, with contact-point and taxel files next to the XML — loss and every action's gradient against the oracle."""
    import redmax_py as redmax
    from oracle.oracle import OracleSim
    from tactilesimulation_amd.functions import StepSimFunction
    m, rng = _case(seed, tmp_path, files=True)
    nr, nu, nv, nt = m.ndof_r, m.ndof_u, m.ndof_var, m.ndof_tactile
    if nu == 0:
        pytest.skip("no motor in this model")
    sim = redmax.Simulation(str(tmp_path / ("m%d.xml" % (SEED0 + seed))))
    assert (sim.ndof_r, sim.ndof_u, sim.ndof_var, sim.ndof_tactile) == (nr, nu, nv, nt) and sim.options.h == m.h
    q0 = 0.02 * rng.normal(size=nr)
    Tn, Sn = 3, 2
    u = rng.uniform(-1, 1, size=(Tn, nu))
    cq, cv, ct = rng.normal(size=nr), rng.normal(size=nv), rng.normal(size=nt)
    sim.set_state_init(q0, np.zeros(nr))
    sim.reset(backward_flag=True)
    acts = [torch.tensor(u[t], dtype=torch.float64, requires_grad=True) for t in range(Tn)]
    L = 0.0
    for a in acts:
        q, var, tac = StepSimFunction.apply(a, Sn, sim, True)
        L = L + (q * torch.tensor(cq)).sum() + ((var * torch.tensor(cv)).sum() if nv else 0.0) + ((tac * torch.tensor(ct)).sum() if nt else 0.0)
    L.backward()
    o = OracleSim(m)
    o.reset(q0, record=True)
    Lo = 0.0
    for t in range(Tn):
        if o.forward(u[t], Sn) != 0:
            pytest.skip("a sub-step at max_iter (see the first test of this file)")
        q, _ = o.state()
        v, tc = o.outputs()
        Lo += cq @ q + (cv @ v if nv else 0.0) + (ct @ tc if nt else 0.0)
    assert abs(float(L.detach()) - Lo) < 1e-8 * max(abs(Lo), 1.0)
    for t in reversed(range(Tn)):
        z = lambda c, d: np.concatenate([np.zeros((Sn - 1) * d), c]) if d else None
        go = o.backward_steps(Sn, z(cq, nr), z(cv, nv), z(ct, nt)).sum(0)
        assert np.abs(acts[t].grad.numpy() - go).max() < 1e-6 * max(np.abs(go).max(), 1e-3), (seed, t)


def test_fp32_kernels_on_the_random_models_in_distribution(tmp_path):
    """The fp32 generic kernels against the fp64 oracle on all 120 random models, with `tol` relaxed to 1e-5 (what single precision can reach on models
    of arbitrary scale: with the drawn 1e-9 a third of them flag their sub-steps, which is why the per-model tests above are fp64).  A distribution,
    not a per-model bound — a loose root of an ill-conditioned model is the root to 1e-3 only: measured (tools/random_model_fp32_probe.py) relative
    state error median 9e-9, 90 % 8e-8, 99 % 1e-5, max 4e-3 over 1029 env-steps; tactile frames to 7e-7; 4 of 1046 env-steps flagged by one side only.
    Over 1500 more models (13 272 env-steps: the same quantiles) two environments land on ANOTHER root of their first sub-step — one through the fp32
    default's kink crossing (the one solver option the reference does not have: with it off the kernel is on the oracle's root), one after a 476-evaluation
    struggle in single precision (tools/random_model_fp32_case.py) — hence a bound on the share of such env-steps, not on the maximum."""
    import tactilesimulation_amd.model.blob as BL
    from oracle.oracle import OracleSim
    from tactilesimulation_amd.host.batch import BatchSim
    dq, dtac, one_sided, total = [], [], 0, 0
    for seed in range(N_MODELS):
        try:
            m, rng = _case(seed, tmp_path)
        except BaseException:      # (pytest.skip inside _case)
            continue
        m.F[BL.TSIM_FH_TOL] = 1e-5
        nr, nu = m.ndof_r, m.ndof_u
        q0 = 0.02 * rng.normal(size=(B_, nr))
        u = rng.uniform(-1, 1, size=(B_, T, max(nu, 1)))[:, :, :nu]
        sim = BatchSim(m, B_, dtype=torch.float32, tape_capacity=T * S)
        sim.reset(torch.tensor(q0, device="cuda:0", dtype=torch.float32), None, backward_flag=False)
        outs = [sim.step(torch.tensor(u[:, t], device="cuda:0", dtype=torch.float32).reshape(B_, nu), S) for t in range(T)]
        o = OracleSim(m)
        for e in range(B_):
            o.reset(q0[e])
            for t in range(T):
                bad = o.forward(u[e, t], S) != 0
                kbad = int(outs[t]["status"][e]) != 0
                q, _ = o.state()
                total += 1
                if bad or kbad or not np.all(np.isfinite(q)):
                    one_sided += bad != kbad
                    break
                dq.append(np.abs(outs[t]["q"][e].double().cpu().numpy() - q).max() / (1.0 + np.abs(q).max()))
                if m.ndof_tactile:
                    tac = o.outputs()[1]
                    dtac.append(np.abs(outs[t]["tactile"][e].double().cpu().numpy() - tac).max() / (1.0 + np.abs(tac).max()))
    dq, dtac = np.array(dq), np.array(dtac)
    assert len(dq) >= 950 and one_sided <= 0.02 * total, (len(dq), one_sided, total)
    assert np.quantile(dq, 0.5) < 1e-6 and np.quantile(dq, 0.9) < 1e-5 and np.quantile(dq, 0.99) < 1e-3 and (dq > 1e-2).mean() <= 2e-3, [float(np.quantile(dq, x)) for x in (0.5, 0.9, 0.99, 1.0)]
    assert len(dtac) > 100 and np.quantile(dtac, 0.99) < 1e-4 and dtac.max() < 1e-2, [float(np.quantile(dtac, x)) for x in (0.5, 0.99, 1.0)]


# minimum numbers of compared contact states per coverage key (tests/random_corpus.py state_keys) whose contact part of H is far above the tolerance:
# about 3/4 of what the seeded sampler finds on both corpora and chain16 (537 states; profiles/r08_fp32_random_models.md)
GH_MIN = {("prim", "plane"): 350, ("prim", "cuboid"): 16, ("prim", "sphere"): 38, ("prim", "cylinder"): 24, ("sphere_plane",): 180,
          ("stick", "plane"): 340, ("slip", "plane"): 70, ("stick", "cuboid"): 14, ("slip", "cuboid"): 8, ("stick", "sphere"): 30,
          ("slip", "sphere"): 18, ("stick", "cylinder"): 20, ("slip", "cylinder"): 8}
STATS = os.environ.get("TSIM_RM_STATS")      # a directory: the error distributions of the fp32 tests below are written there as JSON (profiles/)


def _stats(name, d):
    if STATS:
        import json
        with open(os.path.join(STATS, name + ".json"), "w") as f:
            json.dump(d, f)


def _q(x):
    x = np.asarray(x)
    return [float(np.quantile(x, p)) for p in (0.5, 0.9, 0.99, 1.0)] if len(x) else []


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-3), (torch.float64, 1e-9)])
def test_residual_and_newton_matrix_on_random_structures(dtype, tol, tmp_path):
    """g and H = dg/dq1 of one evaluation (tsim_debug_eval) on the generic kernels against the oracle's dual-number Jacobian, on every model of both
    corpora and chain16, at contact states of a seeded rejection sampler (random_corpus.contact_states), at 64 / 32 / 16 lanes per environment, pair
    cull on and off.  fp32 builds the contact part of H with its own accumulated 6 x 12 matrix (pair_contacts_matrix) and culls points with an fp32
    distance first: a Newton matrix that is wrong there still converges to the same root, so only this comparison sees it.  H per ROW, relative to
    that row's largest oracle entry (a stiff contact row cannot hide an error in another); the bound of tests/test_gpu_parity.py's pusher states.
    Non-vacuity: the contact part of the oracle's H (H minus H of the model with kn = kt = 0 on the touching pairs) is above 10 x the tolerance in
    the states counted per primitive type and friction branch."""
    from oracle.oracle import OracleSim
    from tactilesimulation_amd.host.batch import BatchSim
    dev = "cuda:0"
    counts = {k: 0 for k in GH_MIN}
    eg, eh, nstates, shapes = [], [], 0, set()
    for case in list(range(N_MODELS)) + LARGE:
        r = RC.draw(case, tmp_path)
        if r is None or not RC.pair_info(r[0]):
            continue
        m = r[0]
        states = RC.contact_states(m, RC.state_seed(case))
        if not states:
            continue
        o = OracleSim(m)
        ref = []
        for q1, q0, qd0, u, c in states:
            go, Ho = o.residual(q1, q0, qd0, u, which=0)
            _, H0 = OracleSim(RC.without_contact(m, {p for p, *_ in c})).residual(q1, q0, qd0, u, which=0)
            ref.append((go, Ho))
            if (np.abs(Ho - H0).max(1) / np.abs(Ho).max(1)).max() > 10 * tol:
                for k in RC.state_keys(m, c):
                    if k in counts:
                        counts[k] += 1
        nstates += len(states)
        B = len(states)
        sim = BatchSim(m, B, dtype=dtype, tape_capacity=1)
        assert sim.kernel_variant() == "generic"
        args = [torch.tensor(np.stack([s_[j] for s_ in states]).reshape(B, d), device=dev, dtype=dtype) for j, d in enumerate([m.ndof_r] * 3 + [m.ndof_u])]
        for lanes in (64, 32, 16):
            got = RC.force_lanes(sim, m, lanes)
            shapes.add((m.ndof_r, lanes, got))
            for cull in (False, True):
                sim.set_option(BatchSim.OPT_PAIR_CULL, cull)
                g, H = sim.debug_eval(*args)
                g, H = g.double().cpu().numpy(), H.double().cpu().numpy()
                for e, (go, Ho) in enumerate(ref):
                    # g relative to the larger of itself and the size of its inertial / stiffness part H (q1 - q0): at a random state g can be a small
                    # difference of large terms, whose rounding is relative to the terms
                    rg = np.abs(g[e] - go).max() / max(np.abs(go).max(), np.abs(Ho @ (states[e][0] - states[e][1])).max(), 1e-6)
                    rh = (np.abs(H[e] - Ho).max(1) / np.abs(Ho).max(1)).max()
                    eg.append(rg)
                    eh.append(rh)
                    assert np.isfinite(rg) and np.isfinite(rh) and rg <= tol and rh <= tol, (case, lanes, got, cull, e, rg, rh, m.ndof_r)
    _stats("gh_%s" % str(dtype)[-7:], {"states": nstates, "counts": {"/".join(k): v for k, v in counts.items()}, "g": _q(eg), "H_row": _q(eh),
                                        "shapes": sorted(shapes)})
    assert nstates >= 450, nstates
    assert all(counts[k] >= GH_MIN[k] for k in GH_MIN), {"/".join(k): (counts[k], GH_MIN[k]) for k in GH_MIN}


def test_fp32_adjoint_on_the_random_models_in_distribution(tmp_path):
    """The fp32 generic kernels' adjoint — dL/du of every sub-step, dL/dq0, dL/dqdot0 — against the fp64 oracle on both corpora and chain16, 8
    environments per model, the kernels at `tol` 1e-5 (see the test above), the oracle at the same `tol` and max_iter >= 100 — the same Newton loop,
    so that what is measured is the kernels' arithmetic: against an oracle at `tol` 1e-12 the distribution is that of the 1e-5 root itself, and the
    fp64 kernels at `tol` 1e-5 show the same one (median 1e-5, 99 % 8e-3, max 5e-2; profiles/r08_fp32_random_models.md).
    Compared: environments whose branch signature of every sub-step (tsim_debug_signature) is the oracle's (forward_sig) and that both sides
    converged — a gradient across a contact / friction kink is not comparable.  Per environment and quantity, relative to the quantity's largest
    oracle entry.  >= 300 environments; >= 99 % within 1e-4; none above 1e-2 (an environment on the oracle's branches with a wrong gradient is a bug)."""
    import tactilesimulation_amd.model.blob as BL
    from oracle.oracle import OracleSim
    from tactilesimulation_amd.host.batch import BatchSim
    B8, T8, S8 = 8, 3, 2
    n = T8 * S8
    dev, dt = "cuda:0", torch.float32
    errs, worst, excluded = [], [], 0
    for case in list(range(N_MODELS)) + LARGE:
        r = RC.draw(case, tmp_path)
        if r is None:
            continue
        m, rng = r
        m.F[BL.TSIM_FH_TOL] = 1e-5
        m.I[BL.TSIM_IH_MAX_ITER] = max(int(m.I[BL.TSIM_IH_MAX_ITER]), 100)
        nr, nu, nv, nt = m.ndof_r, m.ndof_u, m.ndof_var, m.ndof_tactile
        q0 = 0.02 * rng.normal(size=(B8, nr))
        u = rng.uniform(-1, 1, size=(B8, T8, max(nu, 1)))[:, :, :nu]
        wq, wv, wt = rng.normal(size=(B8, nr)), rng.normal(size=(B8, nv)), rng.normal(size=(B8, nt))
        sim = BatchSim(m, B8, dtype=dt, tape_capacity=n)
        sim.reset(torch.tensor(q0, device=dev, dtype=dt), None, backward_flag=True)
        st = np.stack([sim.step(torch.tensor(u[:, t], device=dev, dtype=dt).reshape(B8, nu), S8)["status"].cpu().numpy() for t in range(T8)])
        sig = sim.branch_signature().cpu().numpy()
        kw = {"df_dq": torch.tensor(wq, device=dev, dtype=dt)}
        if nv:
            kw["df_dvar"] = torch.tensor(wv, device=dev, dtype=dt)
        if nt:
            kw["df_dtactile"] = torch.tensor(wt, device=dev, dtype=dt)
        du = sim.backward_steps(n, **kw).double().cpu().numpy().reshape(B8, n, nu)
        lam_q, lam_v = (x.double().cpu().numpy() for x in sim.get_adjoint())
        o = OracleSim(m)
        for e in range(B8):
            o.reset(q0[e], record=True)
            so, bad = np.zeros((n, 2), dtype=np.int64), 0
            for t in range(T8):
                b_, so[t * S8:(t + 1) * S8] = o.forward_sig(u[e, t], S8)
                bad |= b_ != 0
            if bad or (st[:, e] != 0).any() or not np.array_equal(so, sig[:, e]):
                excluded += 1
                continue
            z = lambda w, d: np.concatenate([np.zeros((n - 1) * d), w]) if d else None
            g = o.backward_steps(n, df_dq=z(wq[e], nr), df_dvar=z(wv[e], nv) if nv else None, df_dtac=z(wt[e], nt) if nt else None)
            aq, av = o.adjoint()
            pairs = [(du[e], g)] if nu else []
            pairs += [(lam_q[e], aq), (lam_v[e], av)]
            top = max(np.abs(y).max() for _, y in pairs)
            err = max(np.abs(x - y).max() / max(np.abs(y).max(), 1e-6 * top, 1e-30) for x, y in pairs)
            errs.append(err)
            worst.append((err, str(case), e))
    errs = np.array(errs)
    worst.sort(reverse=True)
    _stats("adjoint_fp32", {"compared": len(errs), "excluded": excluded, "quantiles": _q(errs), "worst": worst[:10]})
    assert len(errs) >= 300 and np.mean(errs <= 1e-4) >= 0.99 and errs.max() <= 1e-2, (len(errs), excluded, _q(errs), worst[:5])
