"""The contact-pair and branch loops of the evaluation (csrc/tsim_eval.h phase2, pair_points_matrix, pair_contacts_per_direction, phase3; the
point loops of csrc/tsim_param_grad.hip and csrc/tsim_tangent_kernel.h; csrc/tsim_hip.hip decide_stage_cpt) against the fp64 oracle at the edges
of their shapes, on the models of tests/contact_shape_models.py (tests/test_contact_shape_models.py checks the models and the states on the CPU):

    P1  pairs in groups of four: npair 1, 4, 5, 8, 9                      P4  act / hit masks OR-ed over the slots of a wavefront
    P2  lanes = (pair, direction): np nr = LPE - 1, LPE, LPE + 4          P5  contact points staged in LDS: ncpt 341 | 342 (fp64), 682 | 683 (fp32)
    P3  lanes = points: npt 1, 15 .. 17, 31 .. 33, 63 .. 65, 129           P6  lanes = (branch, direction): nb nr = 15, 16, 20, 32, 36, 64, 81

Generic kernels, fp64 and fp32, forced to 16, 32 and 64 lanes; every test asserts the shape the library reports (lanes per environment and the
block's LDS) against what the case was designed for (contact_shape_models.SHAPES, tests/wide_models.py's arithmetic) and prints the trip counts
of the three loops.  k_tangent has a shape of its own (eight directions' tangent state per slot): asserted against contact_shape_models.TAN_SHAPES,
and the t* models are the 16-lane edges shrunk until k_tangent<double> runs them at 16 lanes too.  No tolerance is chosen here: debug_eval 1e-9 / 2e-3 and its error measures are tests/test_gpu_random_models.py
test_residual_and_newton_matrix_on_random_structures'; the episode comparison is tests/test_gpu_wide_models.py _follow itself; the table
gradient uses the Tally and the bounds of tests/test_gpu_param_grad_oracle.py; the identity is held to tests/test_gpu_tangent.py IDENT_BOUND.
Measured: profiles/r21_contact_pair_shapes.md (TSIM_CONTACT_SHAPE_STATS=<file> appends every figure to it)."""
import copy
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
import contact_shape_models as CS      # noqa: E402
import param_grad_util as PU      # noqa: E402
import wide_models as W      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = PU.DEV
F64, F32 = torch.float64, torch.float32
B, T, S = CS.B_ENVS, CS.T_FRAMES, CS.SUBSTEPS
ROWS_SEED = 11
STATS = os.environ.get("TSIM_CONTACT_SHAPE_STATS")
_TMP = []


def _dir():
    """where the models' XML and point files go: created when the first test needs it, not at import"""
    if not _TMP:
        _TMP.append(tempfile.mkdtemp(prefix="tsim_contact_shapes_"))
    return _TMP[0]


def _grid(names, rows=(False,)):
    return [pytest.param(n, dt, l, r, id="%s-%s-lanes%d-%s" % (n, "fp64" if dt == F64 else "fp32", l, "rows" if r else "shared"))
            for n in names for dt in (F64, F32) for l in (16, 32, 64) for r in (rows if n not in CS.P5 else (False, True))]


def _t(x, dt):
    return torch.tensor(np.ascontiguousarray(x), device=DEV, dtype=dt)


def _note(what, name, dtype, got, s, **figures):
    p2, p3, p6 = CS.trips(s, got)
    line = "%s %s %s lanes %d trips phase2 %s points %s phase3 %d: %s" % (what, name, "fp64" if dtype == F64 else "fp32", got, p2, p3, p6,
                                                                          " ".join("%s %.3e" % kv for kv in figures.items()))
    print(line)
    if STATS:
        with open(STATS, "a") as f:
            f.write(line + "\n")


def _assert_shape(sim, m, name, dtype, lanes, rows):
    """the exact shape: the lanes the case was designed for, the generic kernels, the block's LDS as tests/wide_models.py restates it — and with
    it whether the contact points are staged"""
    esz = 8 if dtype == F64 else 4
    want = CS.SHAPES[name][esz, rows][(16, 32, 64).index(lanes)]
    info = sim.launch_info()
    assert sim.kernel_variant() == "generic"
    assert info["lanes_per_env"] == want == W.forced_shape(m, lanes, esz, rows)[0], (name, dtype, lanes, rows, info)
    assert info["lds_bytes"] == W.forced_shape(m, lanes, esz, rows)[1] and info["blocks"] == -(-sim.B // (64 // want)), (name, dtype, lanes, rows, info)
    ncpt = int(m.I[Bl.TSIM_IH_NCPT])
    staged = W.stages_cpt(m, lanes, esz, rows)
    assert info["lds_bytes"] == W.block_bytes(m, 64 // want, esz, rows, staged) != W.block_bytes(m, 64 // want, esz, rows, not staged)
    if name in CS.P5:      # both sides of both thresholds
        assert staged == (3 * ncpt * esz <= W.CPT_LDS_BYTES) == {(341, 4): True, (342, 4): True, (682, 4): True, (683, 4): False,
                                                                 (341, 8): True, (342, 8): False, (682, 8): False, (683, 8): False}[ncpt, esz]
    return want


def _sim(name, dtype, lanes, rows, nenv, cap, tol=None):
    from tactilesimulation_amd.host.batch import BatchSim
    m, s = CS.table_model(name, _dir())
    m = copy.deepcopy(m)
    if tol is not None:
        m.F[Bl.TSIM_FH_TOL] = tol
    sim = BatchSim(m, nenv, device=DEV, dtype=dtype, tape_capacity=cap)
    sim.set_static(False)
    sim.set_lanes_per_env(lanes)
    tab = PU.table_rows(m, nenv, dtype == F32, ROWS_SEED) if rows else None
    if rows:
        sim.set_env_tables(_t(tab, dtype))
    got = _assert_shape(sim, m, name, dtype, lanes, rows)
    return sim, m, s, tab, got


# ---------------------------------------------------------------------------------------------------- a. g and H of one evaluation
_REF = {}


def _eval_reference(name, m, s, tab, fp32):
    """(names, states, [(g, H)] of the oracle, states with contact) of contact_shape_models.eval_batch — computed once per (model, rows)"""
    from oracle.oracle import OracleSim
    key = (name, None if tab is None else fp32)
    if key not in _REF:
        names, states = CS.eval_batch(s, m)
        ref = []
        for e, (q1, q0, qd0, u) in enumerate(states):
            me = m if tab is None else PU.row_model(m, np.asarray(tab[e], dtype=np.float64))
            ref.append(OracleSim(me).residual(q1, q0, qd0, u, which=0))
        _REF[key] = (names, states, ref)
    return _REF[key]


@pytest.mark.parametrize("name,dtype,lanes,rows", _grid(list(CS.TABLE)))
def test_residual_and_newton_matrix_follow_the_oracle(name, dtype, lanes, rows):
    """tsim_debug_eval on a batch whose slots differ: environment e touches pair e mod npair alone (deep: every near point), then one that
    touches nothing (everything far), one that touches everything, one whose pairs' bounding spheres reach their primitives while no point
    penetrates, then every pair alone grazing (its low point only); B is no multiple of 4.  The error measures and tolerances of
    tests/test_gpu_random_models.py test_residual_and_newton_matrix_on_random_structures; pair cull on and off agree bit for bit.  The P5 models also
    with per-environment tables"""
    from tactilesimulation_amd.host.batch import BatchSim
    m0, s0 = CS.table_model(name, _dir())
    n = len(CS.eval_batch(s0, m0)[0])
    assert n % 4 and n >= len(s0.pairs) + 3
    sim, m, s, tab, got = _sim(name, dtype, lanes, rows, n, 1)
    names, states, ref = _eval_reference(name, m, s, tab, dtype == F32)
    tol = 2e-3 if dtype == F32 else 1e-9
    args = [_t(np.stack([st[j] for st in states]).reshape(n, d), dtype) for j, d in enumerate([m.ndof_r] * 3 + [m.ndof_u])]
    out, wg, wh = [], 0.0, 0.0
    for cull in (False, True):
        sim.set_option(BatchSim.OPT_PAIR_CULL, cull)
        g, H = sim.debug_eval(*args)
        out.append((g.clone(), H.clone()))
        g, H = g.double().cpu().numpy(), H.double().cpu().numpy()
        for e, (go, Ho) in enumerate(ref):
            rg = np.abs(g[e] - go).max() / max(np.abs(go).max(), np.abs(Ho @ (states[e][0] - states[e][1])).max(), 1e-6)
            rh = (np.abs(H[e] - Ho).max(1) / np.abs(Ho).max(1)).max()
            wg, wh = max(wg, rg), max(wh, rh)
            print("  %s env %d %s cull %d: g %.3e H row %.3e" % (name, e, names[e], cull, rg, rh))
            assert np.isfinite(rg) and np.isfinite(rh) and rg <= tol and rh <= tol, (name, lanes, cull, e, names[e], rg, rh)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), (name, lanes, "pair cull changes the result")
    _note("g_H", name, dtype, got, s, g=wg, H_row=wh, envs=n)


# ---------------------------------------------------------------------------------------------------- b. a short episode
@pytest.mark.parametrize("name,dtype,lanes,rows", _grid(CS.EPISODE_MODELS, rows=(True,)))
def test_short_episode_follows_the_oracle(name, dtype, lanes, rows):
    """three frames of two sub-steps from a pressed state (every pair grazing), five environments: one sub-step per launch and one episode
    launch; state, end-effector variable, dL/du, dL/dq0 and dL/dqd0 by tests/test_gpu_wide_models.py _follow, its code and bounds; the kernels'
    branch signatures are the oracle's in all five environments"""
    import test_gpu_wide_models as G
    from oracle.oracle import OracleSim
    sim, m, s, tab, got = _sim(name, dtype, lanes, rows, B, T * S)
    q0, qd0, u, S_ = CS.episode_case(s, m)
    assert S_ == S and (G.T, G.S) == (T, S)
    worst = G._follow(sim, m, q0, qd0, u, tab, dtype, (name, str(dtype), lanes, rows), S)
    sim.reset(_t(q0, dtype), _t(qd0, dtype), backward_flag=True)
    sim.rollout(_t(u.transpose(1, 0, 2), dtype), S)
    sig = sim.branch_signature().cpu().numpy()
    for e in range(B):
        o = OracleSim(m if tab is None else PU.row_model(m, np.asarray(tab[e], dtype=np.float64)))
        o.reset(q0[e], qd0[e])
        osig = np.concatenate([o.forward_sig(u[e, t], S)[1] for t in range(T)], 0)
        assert osig[:, 0].max() >= 1 and np.array_equal(sig[:, e], osig), (name, dtype, lanes, e, sig[:, e], osig)
    assert sim.launch_info()["lanes_per_env"] == got
    _note("follow", name, dtype, got, s, **worst)


# ---------------------------------------------------------------------------------------------------- c. the contact columns' gradient
def _touched_pairs(om, q0, qd0, u):
    from oracle.oracle import OracleSim
    o = OracleSim(om)
    o.reset(q0, qd0)
    touched = set()
    for t in range(u.shape[0]):
        for _ in range(S):
            o.forward(u[t], 1)
            touched |= {r[0] for r in o.contact_list(*o.state(), max_rows=1024)}
    return touched


@pytest.mark.parametrize("name,dtype,lanes,rows", _grid(CS.GRADIENT_MODELS, rows=(True,)))
def test_contact_columns_gradient_against_the_oracle(name, dtype, lanes, rows):
    """tsim_set_param_grad (k_backward_z -> k_param_grad) against the oracle's parameter adjoint, with the Tally and the bounds of
    tests/test_gpu_param_grad_oracle.py, over every column of the row and once more over the pair columns alone (its coverage asserts ask for
    tactile sensors, which these models do not have: every environment must be compared and the pair kn column must be above the floor in
    three of them instead).  Environment e presses pair e mod npair alone, the
    other branches are far above, and B = max(5, npair + 1), so that every pair — the second group and the trailing group of the npair 8 and 9 models
    too — is the lone touching pair of some environment: the columns of a pair the oracle never sees in contact are EXACTLY zero on both sides, the
    others are the oracle's — a pair index that is off by one fails both"""
    import test_gpu_param_grad_oracle as PGO
    fp64 = dtype == F64
    nB = CS.gradient_batch(name)      # five, or npair + 1: every pair of the npair 8 and 9 models is the lone touching pair of an environment
    sim, m, s, tab, got = _sim(name, dtype, lanes, rows, nB, T * S, tol=1e-13 if fp64 else None)
    q0, qd0, u, _ = CS.episode_case(s, m, B=nB, only=True)
    w = PU.loss_weights(m, T)
    g, sig, status = PU.gpu_episode(sim, None if tab is None else _t(tab, dtype), q0, qd0, u, S, w, want_qd=False)[:3]
    g, sig, status = g.double().cpu().numpy(), sig.cpu().numpy(), status.cpu().numpy()
    pcols = m.param_columns()
    assert np.all(g[:, np.setdiff1d(np.arange(g.shape[1]), [c for (_, _, _, c) in pcols])] == 0)
    keys = [tuple(k) for k in m.meta["pair_keys"]]
    tally, pairs_only = PGO.Tally(fp64), PGO.Tally(fp64)
    zero_cols = live_cols = 0
    # the rows the kernels read (tests/test_gpu_param_grad_oracle.py _compare_batch): the per-environment tables, or the shared model rounded to the batch's type
    table = (sim.base_tables().double().cpu().numpy() if tab is None else np.asarray(tab, dtype=np.float64))
    lone = set()
    for e in range(nB):
        tally.envs += 1
        om = PU.row_model(m, table[e])
        lone.add(e % len(s.pairs))
        if not fp64:
            om.I = om.I.copy()
            om.I[Bl.TSIM_IH_MAX_ITER] = max(int(om.I[Bl.TSIM_IH_MAX_ITER]), 100)
        _, (go, osig, obad, ost) = PU.oracle_cached(om, q0[e], qd0[e], u[e], S, w)
        assert obad == 0 and status[e] == 0 and np.array_equal(sig[:, e], osig), (name, dtype, lanes, e, sig[:, e], osig)
        touched = _touched_pairs(om, q0[e], qd0[e], u[e])
        assert touched >= CS.touching_of_env(s, e, True)
        for kind, key, f, c in pcols:
            if kind == "pair":
                j = keys.index(tuple(key))
                if j not in touched:
                    zero_cols += 1
                    assert g[e, c] == 0.0 and go[c] == 0.0, (name, dtype, lanes, e, j, f, g[e, c], go[c])
                else:
                    live_cols += go[c] != 0.0
        flags = PGO._states_flags(ost, m, om, np.ones(T, bool))
        tally.add(m, g[e], go, pcols, *flags, tag=(name, e))
        # the row's largest entry is a dof's damping column (a falling branch), and the fp32 floor of 1e-3 of it hides the pair columns: the same
        # Tally once more over the pair columns alone, each held against the largest PAIR column of its row
        pairs_only.envs += 1
        pairs_only.add(m, g[e], go, [pc for pc in pcols if pc[0] == "pair"], *flags, tag=(name, e))
    worst = {}
    for what, t in (("row", tally), ("pairs", pairs_only)):
        ce, re_ = np.array(t.col_err), np.array(t.row_err)
        print("  %s %s: zero columns %d, live %d, col max %.3e row max %.3e above %s" % (name, what, zero_cols, live_cols, ce.max(), re_.max(), t.above))
        assert t.compared == t.envs == nB, (name, what, t.compared)
        if fp64:      # tests/test_gpu_param_grad_oracle.py Tally.check, its bounds
            assert ce.max() <= PGO.F64_BOUND, (name, lanes, what, ce.max())
        else:
            assert np.mean(re_ <= PGO.F32_ROW99) >= 0.99 and re_.max() <= PGO.F32_ROWMAX, (name, lanes, what, re_)
            # (the per-column share is a criterion for the whole row's hundred entries: of the 80 pair entries ONE is 1.25 %, and a column at the
            # floor carries the row's error divided by 1e-3 — the pair columns alone are held by the row bounds above)
            assert what == "pairs" or np.mean(ce <= PGO.F32_COL99) >= 0.99, (name, lanes, what, np.sort(ce)[-5:])
        worst[what + "_col_max"], worst[what + "_row_max"] = ce.max(), re_.max()
    assert lone == set(range(len(s.pairs)))
    assert pairs_only.above["pair kn"] >= 3 and live_cols >= 3 and (zero_cols >= 4 or len(s.pairs) < 3), (name, pairs_only.above, live_cols, zero_cols)
    assert sim.launch_info()["lanes_per_env"] == got
    _note("table_gradient", name, dtype, got, s, zero_columns=zero_cols, **worst)


# ---------------------------------------------------------------------------------------------------- d. the tangent identity
@pytest.mark.parametrize("name,dtype,lanes,rows", _grid(CS.TANGENT_MODELS, rows=(True,)))
def test_tangent_identity_with_eight_directions(name, dtype, lanes, rows):
    """<w, J v> = <J^T w, v>, eight directions on du, dq0, dqd0 and the contact columns: tests/test_gpu_tangent.py's helpers and IDENT_BOUND; the
    shape of k_tangent is the one tests/wide_models.py computes (never narrower than the batch's)"""
    import test_gpu_tangent as TG
    sim, m, s, tab, got = _sim(name, dtype, lanes, rows, B, T * S)
    q0, qd0, u, _ = CS.episode_case(s, m)
    TG._roll(sim, tab, q0, qd0, u, S)
    tl = sim.tangent_launch_info(8, True)
    esz = 8 if dtype == F64 else 4
    want = CS.TAN_SHAPES[name][esz][(16, 32, 64).index(lanes)]      # the designed lanes of k_tangent: a 16-lane edge of a SMALL model runs at 16 lanes
    assert tl["lanes_per_env"] == want == W.tangent_shape(m, lanes, esz) >= got and tl["lds_bytes"] <= W.LDS_CAP, (name, dtype, lanes, tl)
    assert name not in CS.SMALL or want == lanes
    v = TG._directions(sim, m, T, 8, 21, tab)
    o = sim.tangent_episode(T, S, want_qd=True, **v)
    w = TG._seeds(sim, T, T, 22)
    err = TG._identity_errors(o, v, w, TG._adjoint(sim, T, S, w))
    _note("identity", name, dtype, tl["lanes_per_env"], s, max=err.max(), median=float(np.median(err)), batch_lanes=got)
    assert err.max() <= TG.IDENT_BOUND[dtype], (name, err)
