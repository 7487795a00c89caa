"""Every generic kernel instantiation of the 16-row register solve with SEVERAL environments per wavefront, against the fp64 oracle.

The launch plan (csrc/tsim_hip.hip ts_plan) picks an instantiation from the precision, the rows of the register solve (NRM 16 for more than 8
dofs), a rotation-vector joint (EXPJ) and the lanes per environment, the widest packing whose block fits 64 KB of LDS.  The fixed models of the
suite that have more than 8 dofs carry them on many links, whose contexts do not fit two or four to a block, and the tests that force 16 or 32
lanes accept a wider shape without recording which model got which: only a drawn model of the table-gradient tests ("random16", 9 - 10 dofs)
happens to run k_forward, k_backward_z and k_param_grad at NRM 16 and 16 lanes in fp32 (profiles/r20_wide_models.md: the mutation run), and
nothing ran k_backward, k_debug_eval's rows 8 and above or the tangent kernels there.  tests/models/wide9.xml and wide10.xml (tests/wide_models.py) carry
9 / 10 dofs on 4 / 5 links: NRM 16 at 16 lanes in fp32 — every lane of a slot owns a row of the solve — and at 32 lanes in both precisions, for
every kernel, with the shape asserted.

Each test runs both models in both precisions with the lanes forced to 16, 32 and 64, B = 5 (ragged at 4 and at 2 environments per wavefront),
3 frames of 2 sub-steps, per-environment rows, and asserts the exact shape it ran at (launch_info, tangent_launch_info(8, True)), the generic
kernels, and that the block's LDS is what tests/wide_models.py computes.  Expected lanes per environment:

    forced             16   32   64
    fp32               16   32   64      (k_tangent of wide10: 32 32 64 — four contexts AND four tangent blocks of eight directions exceed 64 KB)
    fp64               32   32   64      (four fp64 contexts of a model of 9 or more dofs never fit: tests/test_wide_models.py proves it)

Every bound is the one of the test it mirrors: test_gpu_random_models.py (state, tactile frame, adjoint; residual and Newton matrix),
test_gpu_literal.py (per-sub-step iterates), test_gpu_param_grad_oracle.py and test_gpu_body_param_grad_oracle.py (table gradient: their Tally
and bounds), test_gpu_tangent.py (identity and contraction with the oracle's adjoint rows).  Measured: profiles/r20_wide_models.md.

REACHED_BY / UNREACHABLE at the end are the census of the generic instantiations: which test of the suite runs each, and why the rest cannot be
run by any model."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
import param_grad_util as PU      # noqa: E402
import random_corpus as RC      # noqa: E402
import wide_models as W      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = PU.DEV
F64, F32 = torch.float64, torch.float32
B, T, S = W.B_ENVS, W.T_FRAMES, W.SUBSTEPS
ROWS_SEED = 11
# lanes per environment reached when 16 / 32 / 64 are forced: (batch, k_tangent with eight directions and dtables)
SHAPES = {("wide9", F32): ((16, 32, 64), (16, 32, 64)), ("wide9", F64): ((32, 32, 64), (32, 32, 64)),
          ("wide10", F32): ((16, 32, 64), (32, 32, 64)), ("wide10", F64): ((32, 32, 64), (32, 32, 64))}
STATS = os.environ.get("TSIM_WIDE_STATS")      # a file: the measured figures are appended to it (profiles/r20_wide_models.md)
GRID = [pytest.param(n, dt, l, id="%s-%s-lanes%d" % (n, "fp64" if dt == F64 else "fp32", l)) for n in W.WIDE for dt in (F64, F32) for l in (16, 32, 64)]


def _note(what, name, dtype, lanes, **figures):
    line = "%s %s %s lanes %d: %s" % (what, name, "fp64" if dtype == F64 else "fp32", lanes, " ".join("%s %.3e" % kv for kv in figures.items()))
    print(line)
    if STATS:
        with open(STATS, "a") as f:
            f.write(line + "\n")


def _t(x, dt):
    return torch.tensor(np.ascontiguousarray(x), device=DEV, dtype=dt)


def _expect(name, dtype, lanes):
    return tuple(s[(16, 32, 64).index(lanes)] for s in SHAPES[name, dtype])


def _assert_shape(sim, m, name, dtype, lanes, rows):
    """the exact shape: the batch's, k_tangent's, the generic kernels, and the block's LDS as tests/wide_models.py restates it"""
    want, want_tan = _expect(name, dtype, lanes)
    info, tan = sim.launch_info(), sim.tangent_launch_info(8, True)
    esz = 8 if dtype == F64 else 4
    assert sim.kernel_variant() == "generic"
    assert info["lanes_per_env"] == want and info["blocks"] == -(-sim.B // (64 // want)), (name, dtype, lanes, info)
    assert info["lds_bytes"] == W.forced_shape(m, lanes, esz, env_tables=rows)[1] and want == W.forced_shape(m, lanes, esz, rows)[0], (name, dtype, lanes, info)
    if rows:      # (SHAPES' second entry is k_tangent's shape with per-environment rows, as the tangent tests run it)
        assert tan["lanes_per_env"] == want_tan == W.tangent_shape(m, lanes, esz) and tan["lds_bytes"] <= W.LDS_CAP, (name, dtype, lanes, tan)


def _batch(name, dtype, lanes, rows=True, tol=None):
    """(batch forced to `lanes` at the shape asserted, model, q0, qd0, u, per-environment rows or None)"""
    m, q0, qd0, u, _ = W.wide_case(name)
    m = copy.deepcopy(m)
    if tol is not None:
        m.F[Bl.TSIM_FH_TOL] = tol
    sim = PU.make_sim(m, B, dtype, T * S, lanes=lanes)
    tab = PU.table_rows(m, B, dtype == F32, ROWS_SEED) if rows else None
    if rows:
        sim.set_env_tables(_t(tab, dtype))
    _assert_shape(sim, m, name, dtype, lanes, rows)
    return sim, m, q0, qd0, u, tab


# ---------------------------------------------------------------------------------------------------- 1. state, tactile frame, adjoint
def _follow(sim, m, q0, qd0, u, tab, dtype, tag, S=S):
    """tests/test_gpu_random_models.py test_random_model_follows_the_oracle, its code and bounds, on one sub-step per launch and on one episode
    launch; in fp64 also tests/test_gpu_literal.py's per-sub-step iterate check at its bound"""
    from literal_util import compare_with_literal
    from oracle.oracle import OracleSim
    nr, nu, nv, nt = m.ndof_r, m.ndof_u, m.ndof_var, m.ndof_tactile
    nB = q0.shape[0]
    f32 = dtype == F32
    tq, tg = (2e-4, 2e-3) if f32 else (1e-8, 1e-7)
    rng = np.random.default_rng(5)
    wq, wv, wt = rng.normal(size=(nB, nr)), rng.normal(size=(nB, nv)), rng.normal(size=(nB, nt))
    ut = _t(u.transpose(1, 0, 2), dtype)
    kw = {"df_dq": _t(wq, dtype)}
    if nv:
        kw["df_dvar"] = _t(wv, dtype)
    if nt:
        kw["df_dtactile"] = _t(wt, dtype)
    # one sub-step per launch
    sim.reset(_t(q0, dtype), _t(qd0, dtype), backward_flag=True)
    subs = [sim.step(ut[t], 1, want_qd=True) for t in range(T) for _ in range(S)]
    assert all(int((o["status"] != 0).sum()) == 0 for o in subs), tag
    outs = [{k: (v.double() if v.is_floating_point() else v).cpu().numpy() for k, v in subs[t * S + S - 1].items()} for t in range(T)]
    traj_q = np.stack([q0] + [o["q"].double().cpu().numpy() for o in subs], 1)
    traj_qd = np.stack([qd0] + [o["qd"].double().cpu().numpy() for o in subs], 1)
    du = sim.backward_steps(T * S, **kw).double().cpu().numpy().reshape(nB, T * S, nu)
    lam = [x.double().cpu().numpy() for x in sim.get_adjoint()]
    # one launch each way
    sim.reset(_t(q0, dtype), _t(qd0, dtype), backward_flag=True)
    ro = sim.rollout(ut, S, want_qd=True)
    assert int((ro["status"] != 0).sum()) == 0, tag
    last = lambda w: torch.cat([torch.zeros((T - 1,) + tuple(w.shape), device=DEV, dtype=dtype), w.unsqueeze(0)], 0).contiguous()      # noqa: E731
    du_ep = sim.backward_episode(T, S, last(kw["df_dq"]), last(kw["df_dvar"]) if nv else None, last(kw["df_dtactile"]) if nt else None).double().cpu().numpy()
    lam_ep = [x.double().cpu().numpy() for x in sim.get_adjoint()]
    ro = {k: v.double().cpu().numpy() for k, v in ro.items() if v.is_floating_point()}
    worst = {"q": 0.0, "qd": 0.0, "var": 0.0, "tactile": 0.0, "du": 0.0, "adjoint": 0.0, "substep": 0.0}
    seen = lambda k, x, scale: worst.__setitem__(k, max(worst[k], float(np.abs(x).max()) / scale))      # noqa: E731
    for e in range(nB):
        me = m if tab is None else PU.row_model(m, np.asarray(tab[e], dtype=np.float64))
        o = OracleSim(me)
        o.reset(q0[e], qd0[e], record=True)
        for t in range(T):
            assert o.forward(u[e, t], S) == 0, (tag, e, t)
            q, qd = o.state()
            var, tac = o.outputs()
            scale = 1.0 + np.abs(q).max()
            for got in (outs[t], {k: v[t] for k, v in ro.items()}):
                seen("q", got["q"][e] - q, scale); seen("qd", got["qd"][e] - qd, 1.0 + np.abs(qd).max())
                assert np.allclose(got["q"][e], q, rtol=0, atol=tq * scale), (tag, e, t, np.abs(got["q"][e] - q).max())
                assert np.allclose(got["qd"][e], qd, rtol=0, atol=100 * tq * (1.0 + np.abs(qd).max())), (tag, e, t, np.abs(got["qd"][e] - qd).max())
                if nv:
                    seen("var", got["var"][e] - var[:nv], scale)
                    assert np.allclose(got["var"][e], var[:nv], rtol=0, atol=tq * scale), (tag, e, t)
                if nt:
                    seen("tactile", got["tactile"][e] - tac[:nt], 1.0 + np.abs(tac).max())
                    assert np.allclose(got["tactile"][e], tac[:nt], rtol=0, atol=10 * tq * (1.0 + np.abs(tac).max())), (tag, e, t, np.abs(got["tactile"][e] - tac[:nt]).max())
        z = lambda w_, d: np.concatenate([np.zeros((T * S - 1) * d), w_]) if d else None      # noqa: E731
        g = np.asarray(o.backward_steps(T * S, df_dq=z(wq[e], nr), df_dvar=z(wv[e], nv), df_dtac=z(wt[e], nt))).reshape(T * S, nu)
        gs = 1.0 + np.abs(g).max()
        seen("du", du[e] - g, gs); seen("du", du_ep[:, e] - g.reshape(T, S, nu).sum(1), gs)
        assert np.allclose(du[e], g, rtol=0, atol=tg * gs), (tag, e, np.abs(du[e] - g).max(), gs)
        assert np.allclose(du_ep[:, e], g.reshape(T, S, nu).sum(1), rtol=0, atol=tg * gs), (tag, e, np.abs(du_ep[:, e] - g.reshape(T, S, nu).sum(1)).max(), gs)
        for mine in (lam, lam_ep):
            for x, ref in zip(mine, o.adjoint()):
                seen("adjoint", x[e] - ref, 1.0 + np.abs(ref).max())
                assert np.allclose(x[e], ref, rtol=0, atol=tg * (1.0 + np.abs(ref).max())), (tag, e, np.abs(x[e] - ref).max(), np.abs(ref).max())
        if not f32:      # every sub-step repeated by the literal solver from the kernels' own state before it: the same root, to 1e-9
            dq, ok, _ = compare_with_literal(me, traj_q[e:e + 1], traj_qd[e:e + 1], u[e:e + 1], S)
            worst["substep"] = max(worst["substep"], float(dq.max()))
            assert ok.all() and dq.max() <= 1e-9, (tag, e, dq)
    return worst


@pytest.mark.parametrize("name,dtype,lanes", GRID)
def test_state_tactile_frame_and_adjoint_follow_the_oracle(name, dtype, lanes):
    sim, m, q0, qd0, u, tab = _batch(name, dtype, lanes)
    _note("follow", name, dtype, lanes, **_follow(sim, m, q0, qd0, u, tab, dtype, (name, str(dtype), lanes)))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("lanes", [16, 32, 64])
def test_three_dofs_follow_the_oracle_at_every_shape(lanes, dtype):
    """box_slide (3 dofs: the 8-row solve), which has every shape in both precisions, through the same comparison: the census' k_forward and
    k_backward rows of NRM 8 (no table-gradient buffer is set here, so the adjoint is k_backward and not its twin k_backward_z)"""
    m, q0, qd0, u, S_ = PU.body_case("box_slide", B, T)      # (4 sub-steps per frame)
    if dtype == F32:      # (the model's tol of 1e-12 is out of single precision's reach: 1e-5, as the fp32 tests of test_gpu_random_models.py set it)
        m = copy.deepcopy(m)
        m.F[Bl.TSIM_FH_TOL] = 1e-5
    sim = PU.make_sim(m, B, dtype, T * S_, lanes=lanes)
    tab = PU.table_rows(m, B, dtype == F32, ROWS_SEED)
    sim.set_env_tables(_t(tab, dtype))
    assert sim.launch_info()["lanes_per_env"] == lanes and sim.kernel_variant() == "generic"
    _note("follow", "box_slide", dtype, lanes, **_follow(sim, m, q0, qd0, u, tab, dtype, ("box_slide", str(dtype), lanes), S_))


# ---------------------------------------------------------------------------------------------------- 2. g and H of one evaluation
def _residual_and_matrix(name, m, dtype, lanes):
    """tests/test_gpu_random_models.py test_residual_and_newton_matrix_on_random_structures on one model and one shape: its sampler, its error
    measures, its tolerances, pair cull on and off.  Returns (states whose contact part of H is above 10 x the tolerance, worst g, worst H row)"""
    from oracle.oracle import OracleSim
    from tactilesimulation_amd.host.batch import BatchSim
    tol = 2e-3 if dtype == F32 else 1e-9
    states = RC.contact_states(m, 77, k=5)
    assert len(states) >= 3, name
    o = OracleSim(m)
    ref, loaded = [], 0
    for q1, q0, qd0, u, c in states:
        go, Ho = o.residual(q1, q0, qd0, u, which=0)
        _, H0 = OracleSim(RC.without_contact(m, {p for p, *_ in c})).residual(q1, q0, qd0, u, which=0)
        ref.append((go, Ho))
        loaded += (np.abs(Ho - H0).max(1) / np.abs(Ho).max(1)).max() > 10 * tol
    n = len(states)
    sim = BatchSim(m, n, dtype=dtype, tape_capacity=1)
    RC.force_lanes(sim, m, lanes)
    if name in W.WIDE:
        _assert_shape(sim, m, name, dtype, lanes, False)
    else:
        assert sim.launch_info()["lanes_per_env"] == lanes and sim.kernel_variant() == "generic"
    args = [_t(np.stack([s_[j] for s_ in states]).reshape(n, d), dtype) for j, d in enumerate([m.ndof_r] * 3 + [m.ndof_u])]
    wg = wh = 0.0
    for cull in (False, True):
        sim.set_option(BatchSim.OPT_PAIR_CULL, cull)
        g, H = sim.debug_eval(*args)
        g, H = g.double().cpu().numpy(), H.double().cpu().numpy()
        for e, (go, Ho) in enumerate(ref):
            rg = np.abs(g[e] - go).max() / max(np.abs(go).max(), np.abs(Ho @ (states[e][0] - states[e][1])).max(), 1e-6)
            rh = (np.abs(H[e] - Ho).max(1) / np.abs(Ho).max(1)).max()
            wg, wh = max(wg, rg), max(wh, rh)
            assert np.isfinite(rg) and np.isfinite(rh) and rg <= tol and rh <= tol, (name, lanes, cull, e, rg, rh)
            if m.ndof_r > 9:      # the rows of index 9 and above by themselves, and their coupling with the dofs below is there to be compared
                assert np.abs(Ho[9:, :9]).max() > 0 and (np.abs(H[e] - Ho)[9:].max(1) / np.abs(Ho)[9:].max(1)).max() <= tol, (name, lanes, e)
    return loaded, wg, wh


@pytest.mark.parametrize("name,dtype,lanes", GRID)
def test_residual_and_newton_matrix_follow_the_oracle(name, dtype, lanes):
    """tsim_debug_eval against the oracle's dual-number Jacobian, every row of H relative to its own largest entry: the direct check of the rows
    8 and above of the 16-row solve's matrix (the shared model, no per-environment rows)"""
    m = W.wide_model(name)
    loaded, wg, wh = _residual_and_matrix(name, m, dtype, lanes)
    assert loaded >= 2, (name, loaded)      # the contact part of H is far above the tolerance
    _note("g_H", name, dtype, lanes, g=wg, H_row=wh, loaded=loaded)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("lanes", [16, 32, 64])
def test_residual_and_newton_matrix_of_three_dofs_at_every_shape(lanes, dtype):
    """box_slide: the census' k_debug_eval rows that no model of more than 8 dofs reaches (fp64 at 16 lanes)"""
    m = PU.body_case("box_slide", 1, T)[0]
    loaded, wg, wh = _residual_and_matrix("box_slide", m, dtype, lanes)
    assert loaded >= 1
    _note("g_H", "box_slide", dtype, lanes, g=wg, H_row=wh, loaded=loaded)


# ---------------------------------------------------------------------------------------------------- 3. table gradient, all four groups
@pytest.mark.parametrize("name,dtype,lanes", GRID)
def test_table_gradient_against_the_oracle(name, dtype, lanes):
    """the contact columns (tsim_set_param_grad: k_backward_z -> k_param_grad) and every group (tsim_set_param_grad_groups: k_param_grad_body)
    against the oracle's exact parameter and body adjoints, with the Tally and the bounds of tests/test_gpu_param_grad_oracle.py and
    tests/test_gpu_body_param_grad_oracle.py, unchanged; too little compared fails.  The kinds a tally must hold above its floor are the ones the
    oracle has there (wide_models.CONTACT_KINDS / BODY_KINDS, asserted on the CPU by tests/test_wide_models.py)."""
    import test_gpu_body_param_grad_oracle as BPGO
    import test_gpu_param_grad_oracle as PGO
    fp64 = dtype == F64
    sim, m, q0, qd0, u, tab = _batch(name, dtype, lanes, tol=1e-13 if fp64 else None)
    w = PU.loss_weights(m, T)
    what = "wide_%s_%s_lpe%d" % (name, "fp64" if fp64 else "fp32", lanes)
    tc = PGO.Tally(fp64)
    PGO._compare_batch(tc, ("wide", name), m, sim, _t(tab, dtype), q0, qd0, u, S, w, range(B), max_iter=None if fp64 else 100)
    st = tc.check("contact_" + what, kinds=W.CONTACT_KINDS[name, fp64])
    tb = BPGO.Tally(fp64)
    BPGO._compare_batch(tb, name, m, sim, tab, q0, qd0, u, S, w, range(B), max_iter=None if fp64 else 100)
    sb = tb.check("body_" + what, W.BODY_KINDS[name])
    assert sim.launch_info()["lanes_per_env"] == _expect(name, dtype, lanes)[0]
    _note("table_gradient", name, dtype, lanes, contact_col_max=st["col_q"][2], contact_row_max=st["row_q"][2], body_rel_max=sb["rel_q"][3], body_over_S_max=sb["over_S_q"][3])


# ---------------------------------------------------------------------------------------------------- 4. tangent
@pytest.mark.parametrize("name,dtype,lanes", GRID)
def test_tangent_identity_with_eight_directions(name, dtype, lanes):
    """<w, J v> = <J^T w, v> with nd = 8 and every group on: the directions cover du, dq0, dqd0, the contact columns and the body columns
    (k_tangent_body_src -> k_tangent_src; tests/test_gpu_tangent_body.py _identity), held to tests/test_gpu_tangent.py's IDENT_BOUND"""
    import test_gpu_tangent as TG
    import test_gpu_tangent_body as TGB
    m = W.wide_model(name)
    err, info = TGB._identity(name, dtype, lanes=lanes, groups=PU.ALL, nd=8, B=B, case=W.wide_case(name))
    esz = 8 if dtype == F64 else 4
    assert info["variant"] == "generic" and (info["batch_lanes"], info["lanes_per_env"]) == _expect(name, dtype, lanes), (name, dtype, lanes, info)
    assert (info["batch_lanes"], info["batch_lds_bytes"]) == W.forced_shape(m, lanes, esz) and info["lanes_per_env"] == W.tangent_shape(m, lanes, esz)
    # the launch's own LDS: the contexts of its slots and their tangent blocks of eight directions with dtables (BDF1: two history states)
    ns = 64 // info["lanes_per_env"]
    assert info["lds_bytes"] == W.block_bytes(m, ns, esz, stage_cpt=W.stages_cpt(m, lanes, esz)) + (ns * W.tangent_slot_bytes(m, esz, nhist=2) + 15) // 16 * 16 <= W.LDS_CAP, info
    _note("identity", name, dtype, lanes, max=err.max(), median=float(np.median(err)))
    assert err.max() <= TG.IDENT_BOUND[dtype], (name, err)


@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("name", W.WIDE)
def test_tangent_against_the_oracle_adjoint_per_component(name, lanes):
    """tests/test_gpu_tangent.py test_tangent_against_the_oracle_adjoint_per_component on the wide models: fp64, Newton tol 1e-13, J v of
    k_tangent (eight directions on du, dq0, dqd0 and the contact columns) contracted with the oracle's seeds against the oracle's J^T w
    contracted with v, within 1e-7 of the row's scale (floor 1e-9)"""
    import test_gpu_tangent as TG
    sim, m, q0, qd0, u, tab = _batch(name, F64, lanes, tol=1e-13)
    wtac = np.random.default_rng(31).normal(size=(4, T, m.ndof_tactile))
    seeds, rows = TG._oracle_rows("wide:" + name, m, tab, q0, qd0, u, S, wtac)
    TG._roll(sim, tab, q0, qd0, u, S)
    nd = 8
    v = TG._directions(sim, m, T, nd, 23, tab)
    o = {k: x.cpu().numpy() for k, x in sim.tangent_episode(T, S, **v).items()}
    vn = {k: x.cpu().numpy() for k, x in v.items()}
    worst = 0.0
    for e in range(B):
        for (kind, i), (du, lq, lv, g) in zip(seeds, rows[e]):
            for d in range(nd):
                if kind == "q":
                    lhs = o["dq"][d, T - 1, e, i]
                elif kind == "var":
                    lhs = o["dvar"][d, T - 1, e, i]
                else:
                    lhs = float((o["dtactile"][d, :, e] * wtac[i]).sum())
                parts = [du * vn["du"][d, :, e], lq * vn["dq0"][d, e], lv * vn["dqd0"][d, e], g * vn["dtables"][d, e]]
                rhs, scale = sum(p.sum() for p in parts), max(sum(np.abs(p).sum() for p in parts), 1e-9)
                worst = max(worst, abs(lhs - rhs) / scale)
                assert abs(lhs - rhs) <= 1e-7 * scale, (name, lanes, e, kind, i, d, lhs, rhs, scale)
    _note("oracle_rows", name, F64, lanes, worst=worst)


# ---------------------------------------------------------------------------------------------------- 5. k_tangent itself
@pytest.mark.parametrize("name,dtype,lanes", GRID)
def test_tangent_identity_with_the_contact_group_alone(name, dtype, lanes):
    """the body groups off: no pre-pass and no source term, so the launch is k_tangent itself and not k_tangent_src — tests/test_gpu_tangent.py's
    identity check with eight directions on du, dq0, dqd0 and the contact columns, at its bound and at the shape asserted"""
    import test_gpu_tangent as TG
    sim, m, q0, qd0, u, tab = _batch(name, dtype, lanes)
    TG._roll(sim, tab, q0, qd0, u, S)
    v = TG._directions(sim, m, T, 8, 21, tab)
    o = sim.tangent_episode(T, S, want_qd=True, **v)
    w = TG._seeds(sim, T, T, 22)
    err = TG._identity_errors(o, v, w, TG._adjoint(sim, T, S, w))
    _note("identity_contact_only", name, dtype, lanes, max=err.max(), median=float(np.median(err)))
    assert err.max() <= TG.IDENT_BOUND[dtype], (name, err)


# ---------------------------------------------------------------------------------------------------- 6. the census
# An instantiation: (kernel, real "f" / "d", NRM — None where the kernel has no such parameter —, EXPJ, LPE).  REACHED_BY maps every generic
# instantiation of the ten kernels to (case, forced lanes (0: the library's choice), per-environment rows, the test that runs it there); the
# precision is the instantiation's.  Cases: the wide models (NRM 16 below 64 lanes, and at 64), "box_slide" (3 dofs: NRM 8, every shape in both
# precisions) and "bdf2:tactile_pad" (a rotation-vector joint: EXPJ, 64 lanes whatever is asked for).  UNREACHABLE: the rest, with the arithmetic.
# What ties an entry to its test: tests/test_wide_models.py reads the named test's parametrize marks and body for the case and the lanes, and the
# plan test below asks the library for the shape of (case, lanes).  Neither executes the named test: a case it skipped at run time would not show.
WITH_NRM = ("k_forward", "k_backward", "k_backward_z", "k_tangent", "k_tangent_src", "k_frame_jacobian")
WITHOUT_NRM = ("k_debug_eval", "k_param_grad", "k_param_grad_body", "k_tangent_body_src")
_HERE = "test_gpu_wide_models.py::"
_BODY = "test_gpu_body_param_grad_oracle.py::test_generic_body_gradient_against_the_oracle"
_FJ = "test_gpu_frame_jacobians.py::"
_TEST_OF = {      # kernel: the test that runs it on (the wide models, box_slide, bdf2:tactile_pad)
    "k_forward": (_HERE + "test_state_tactile_frame_and_adjoint_follow_the_oracle", _HERE + "test_three_dofs_follow_the_oracle_at_every_shape", _BODY),
    # (no table-gradient buffer: k_backward; with one: its twin k_backward_z, then the parameter passes)
    "k_backward": (_HERE + "test_state_tactile_frame_and_adjoint_follow_the_oracle", _HERE + "test_three_dofs_follow_the_oracle_at_every_shape",
                   "test_gpu_bdf2_adjoint.py::test_bdf2_adjoint_matches_the_oracle"),
    "k_backward_z": (_HERE + "test_table_gradient_against_the_oracle", _BODY, _BODY),
    "k_param_grad": (_HERE + "test_table_gradient_against_the_oracle", _BODY, _BODY),
    "k_param_grad_body": (_HERE + "test_table_gradient_against_the_oracle", _BODY, _BODY),
    "k_debug_eval": (_HERE + "test_residual_and_newton_matrix_follow_the_oracle", _HERE + "test_residual_and_newton_matrix_of_three_dofs_at_every_shape", None),
    # (the body groups off: k_tangent; on, with dtables: k_tangent_body_src, then k_tangent_src)
    "k_tangent": (_HERE + "test_tangent_identity_with_the_contact_group_alone", "test_gpu_tangent.py::test_identity_at_every_launch_shape",
                  "test_gpu_tangent.py::test_identity_against_the_adjoint"),
    "k_tangent_src": (_HERE + "test_tangent_identity_with_eight_directions", "test_gpu_tangent_body.py::test_identity_at_every_launch_shape",
                      "test_gpu_tangent_body.py::test_identity_with_body_directions"),
    "k_tangent_body_src": (_HERE + "test_tangent_identity_with_eight_directions", "test_gpu_tangent_body.py::test_identity_at_every_launch_shape",
                           "test_gpu_tangent_body.py::test_identity_with_body_directions"),
    # (BDF1 models only: its rotation-vector case is param_grad_util's "tactile_pad" run as a BDF1 model, not the BDF2 file's)
    "k_frame_jacobian": (_FJ + "test_columns_on_the_wide_models", _FJ + "test_columns_at_every_launch_shape", _FJ + "test_columns_with_a_rotation_vector_joint")}
TANGENT_SHAPED = ("k_tangent", "k_tangent_src")      # their lanes are tsim_tangent_launch_info's; every other kernel runs at the batch's ...
FRAME_JACOBIAN_SHAPED = ("k_frame_jacobian",)        # ... but this one: tsim_frame_jacobians_launch_info's (wide_models.frame_jacobian_shape)


def _census():
    reached, unreachable = {}, {}
    why = ("four fp64 contexts of a model of 9 or more dofs take at least 4 x %d bytes > 64 KB (tests/test_wide_models.py "
           "test_no_model_of_nine_or_more_dofs_fits_four_fp64_environments)" % W.env_bytes_lower_bound(9, 8))
    for k, (t_wide, t_box, t_exp) in _TEST_OF.items():
        rows = k != "k_debug_eval"      # the debug kernel's tests run the shared model
        for r in "fd":
            for lpe in (16, 32, 64):
                # more than 8 dofs at lpe lanes: wide10 forced to lpe — but k_tangent in fp32 at 16 lanes only wide9 (SHAPES), and nothing in fp64 at 16
                # (and k_frame_jacobian: four column blocks of wide10 next to four fp32 contexts exceed 64 KB too)
                wide = None if (r, lpe) == ("d", 16) else "wide9" if k in TANGENT_SHAPED + FRAME_JACOBIAN_SHAPED and (r, lpe) == ("f", 16) else "wide10"
                if k in WITH_NRM:
                    reached[k, r, 8, False, lpe] = ("box_slide", lpe, rows, t_box)
                    if wide:
                        reached[k, r, 16, False, lpe] = (wide, lpe, rows, t_wide)
                    else:
                        unreachable[k, r, 16, False, lpe] = why
                else:      # one instantiation for every number of dofs: the wide models where they reach the shape
                    reached[k, r, None, False, lpe] = (wide, lpe, rows, t_wide) if wide else ("box_slide", lpe, rows, t_box)
            if t_exp:
                reached[k, r, 16 if k in WITH_NRM else None, True, 64] = ("tactile_pad" if k in FRAME_JACOBIAN_SHAPED else "bdf2:tactile_pad", 0, True, t_exp)
    return reached, unreachable


REACHED_BY, UNREACHABLE = _census()


def census_model(case):
    return W.wide_model(case) if case in W.WIDE else PU.body_case(case, 1, T)[0]


@pytest.mark.parametrize("inst", sorted(REACHED_BY, key=str), ids=lambda i: "%s-%s-nrm%s-exp%d-lpe%d" % i)
def test_the_plan_reaches_every_census_entry(inst):
    """the batch of the entry's case, created and forced as its test does, not simulated: the launch plan reports the entry's lanes per
    environment (k_tangent, k_tangent_src: tsim_tangent_launch_info; k_frame_jacobian: tsim_frame_jacobians_launch_info; the others:
    tsim_launch_info, the shape of the parameter passes and of the pre-pass too) and the generic kernels, and the entry's NRM and EXPJ are the plan's rule for the model — NRM = 16 iff ndof_r > 8 or a
    rotation-vector joint (csrc/tsim_hip.hip ts_plan; the library reports no NRM, so the rule is restated here)"""
    kernel, r, nrm, expj, lpe = inst
    case, lanes, rows, test = REACHED_BY[inst]
    dtype = F64 if r == "d" else F32
    m = census_model(case)
    sim = PU.make_sim(m, B, dtype, T * S, lanes=lanes)
    if rows:
        sim.set_env_tables(_t(PU.table_rows(m, B, dtype == F32, ROWS_SEED), dtype))
    info = sim.tangent_launch_info(8, True) if kernel in TANGENT_SHAPED else sim.frame_jacobians_launch_info() if kernel in FRAME_JACOBIAN_SHAPED else sim.launch_info()
    assert info["lanes_per_env"] == lpe and info["lds_bytes"] <= W.LDS_CAP, (inst, REACHED_BY[inst], info)
    assert sim.kernel_variant() == "generic" and RC.has_exp_joint(m) == expj
    assert nrm is None or nrm == (16 if m.ndof_r > 8 or RC.has_exp_joint(m) else 8), (inst, m.ndof_r)
