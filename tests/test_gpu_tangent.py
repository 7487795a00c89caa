"""The forward-mode tangent pass over the taped episode (include/tsim.h tsim_tangent_episode, BatchSim.tangent_episode, functions.episode_jacobian).

It is the transpose of the adjoint launches, so it is held to them by the inner-product identity <w, J v> = <J^T w, v>: random directions
v = (du, dq0, dqd0, dtables on the contact columns) through tangent_episode against random seeds w = (wq, wv, wt) on every frame through
backward_episode + get_adjoint + the set_param_grad buffer, per environment, none left out (the identity holds at any iterate).  The error is
    |<w, J v> - <J^T w, v>| / (sum_i |w_i (J v)_i| + sum_j |(J^T w)_j v_j|)
and its bound is 10 x the largest value measured over every case of the identity test (profiles/r17_tangent.md): fp64 6.7e-15 measured (it must
stay below 1e-10: both sides use the same taped H and the same evaluation, only the order of the sums differs), fp32 1.1e-6 measured (below 1e-4,
the project's fp32 gradient tolerance).
The adjoint itself is pinned to the fp64 oracle elsewhere; here the tangent's outputs are also contracted with the oracle's own adjoint rows,
component by component (1e-7 of the row's scale at Newton tol 1e-13: the setting and bound of tests/test_gpu_parity.py's fp64 adjoint).
tests/test_tangent_yardstick.py checks, on the CPU, that the oracle's adjoint is the derivative of its forward pass along such directions and that
every case here converges on the oracle.  The rest: directions are independent of each other and of ndir (bit for bit), the launch changes nothing
that exists, the refusals, the Jacobian helper and the Levenberg-Marquardt example.  Every identity case asserts the shape k_tangent ran at
(tsim_tangent_launch_info) and prints it.
Cases: the inputs of tests/param_grad_util.py, B = 5 (ragged at 4 and 2 environments per wavefront), T = 3 frames of 2 sub-steps (pusher: 5)."""
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
from test_tangent_yardstick import TANGENT_CASES, T_FRAMES, tangent_case      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = PU.DEV
F64, F32 = torch.float64, torch.float32
# 10 x the measured maxima (module docstring)
IDENT_BOUND = {F64: 6.7e-14, F32: 1.1e-5}
STATS = os.environ.get("TSIM_TANGENT_STATS")      # a file: every identity error is appended to it (profiles/r17_tangent.md)


def _t(x, dt):
    return torch.tensor(np.ascontiguousarray(x), device=DEV, dtype=dt)


def _directions(sim, m, T, nd, seed, tab=None, table_dirs=True):
    """random directions: du [nd, T, B, nu], dq0, dqd0 [nd, B, nr], dtables [nd, B, table_size] on the contact columns (of the size of the entry)"""
    rng = np.random.default_rng(seed)
    B, dt = sim.B, sim.dtype
    base = sim.base_tables().double().cpu().numpy() if tab is None else np.asarray(tab, dtype=np.float64)
    cols = [c for (_, _, _, c) in m.param_columns()]
    dtab = np.zeros((nd,) + base.shape)
    dtab[:, :, cols] = rng.normal(size=(nd, B, len(cols))) * (np.abs(base[:, cols]) + 0.1)
    v = {"du": _t(rng.normal(size=(nd, T, B, sim.ndof_u)), dt), "dq0": _t(rng.normal(size=(nd, B, sim.ndof_r)), dt),
         "dqd0": _t(rng.normal(size=(nd, B, sim.ndof_r)), dt), "dtables": _t(dtab, dt) if table_dirs else None}
    return v


def _seeds(sim, T, nm, seed):
    rng = np.random.default_rng(seed)
    dt = sim.dtype
    return (_t(rng.normal(size=(T, sim.B, sim.ndof_r)), dt), _t(rng.normal(size=(T, sim.B, sim.ndof_var)), dt) if sim.ndof_var else None,
            _t(rng.normal(size=(nm, sim.B, sim.ndof_tactile)), dt) if sim.ndof_tactile and nm else None)


def _roll(sim, tab, q0, qd0, u, S, mask=None):
    dt = sim.dtype
    if tab is not None:
        sim.set_env_tables(_t(tab, dt))
    sim.reset(_t(q0, dt), _t(qd0, dt), backward_flag=True)
    return sim.rollout(_t(u.transpose(1, 0, 2), dt), S, want_qd=True, tactile_mask=mask)


def _adjoint(sim, T, S, w, mask=None):
    """backward_episode with the table gradient into a zeroed buffer: (dL/du [T, B, nu], dL/dq0, dL/dqd0, table gradient)"""
    g = torch.zeros_like(sim.base_tables())
    sim.set_param_grad(g)
    try:
        du = sim.backward_episode(T, S, w[0], w[1], w[2], tactile_mask=mask)
    finally:
        sim.set_param_grad(None)
    lq, lv = sim.get_adjoint()
    return du, lq, lv, g


def _identity_errors(o, v, w, adj):
    """[nd, B] identity errors, in double on the host"""
    d = lambda x: x.double()
    du, lq, lv, g = adj
    lhs = d(o["dq"]) * d(w[0]).unsqueeze(0)
    terms_l = [lhs.sum((1, 3)), lhs.abs().sum((1, 3))]
    for k, ws in (("dvar", w[1]), ("dtactile", w[2])):
        if ws is not None:
            x = d(o[k]) * d(ws).unsqueeze(0)
            terms_l[0] = terms_l[0] + x.sum((1, 3)); terms_l[1] = terms_l[1] + x.abs().sum((1, 3))
    x = d(v["du"]) * d(du).unsqueeze(0)
    r, ra = x.sum((1, 3)), x.abs().sum((1, 3))
    for a, b in ((v["dq0"], lq), (v["dqd0"], lv), (v["dtables"], g)):
        if a is not None:
            x = d(a) * d(b).unsqueeze(0)
            r, ra = r + x.sum(2), ra + x.abs().sum(2)
    err = ((terms_l[0] - r).abs() / (terms_l[1] + ra)).cpu().numpy()
    assert np.all(np.isfinite(err)) and float((terms_l[1] + ra).min()) > 0
    return err


def _check_identity(name, dtype, lanes=0, static=False, rows=True, mask=None, nd=3, expect_variant=None, edit=False, expect_lanes=None):
    B = 5
    m, q0, qd0, u, S = tangent_case(name, B)
    if edit:                                                                  # another model of the same structure: its contact parameters scaled
        m = copy.deepcopy(m)
        m.F[[c for (_, _, _, c) in m.param_columns()]] *= 1.1
    T = T_FRAMES
    sim = PU.make_sim(m, B, dtype, T * S, lanes=lanes, static=static)
    tab = PU.table_rows(m, B, dtype == F32, 11) if rows else None
    _roll(sim, tab, q0, qd0, u, S, mask)
    if expect_variant:
        assert sim.kernel_variant() == expect_variant
    nm = T if mask is None else int(np.sum(mask))
    # the shape k_tangent runs at: the batch's lanes, or wider where a block would not hold eight directions' tangent state (never narrower)
    bl, tl = sim.launch_info()["lanes_per_env"], sim.tangent_launch_info(nd, True)
    assert tl["lanes_per_env"] >= bl and tl["lds_bytes"] <= 64 * 1024 and tl["lanes_per_env"] == sim.tangent_launch_info(8, True)["lanes_per_env"]
    if expect_lanes is not None:
        assert tl["lanes_per_env"] == expect_lanes, (name, dtype, lanes, bl, tl)
    v = _directions(sim, m, T, nd, 21, tab)
    o = sim.tangent_episode(T, S, tactile_mask=mask, want_qd=True, **v)
    assert sim.tape_len() == T * S
    w = _seeds(sim, T, nm, 22)
    err = _identity_errors(o, v, w, _adjoint(sim, T, S, w, mask))
    print("identity %-24s %s lanes %2d (k_tangent at %2d, NRM %2d) static %d rows %d mask %d: max %.3e median %.3e" % (
        name, "f64" if dtype == F64 else "f32", lanes, tl["lanes_per_env"], 16 if sim.ndof_r > 8 or "tactile_pad" in name else 8, static, rows, mask is not None,
        err.max(), np.median(err)))
    if STATS:
        with open(STATS, "a") as f:
            f.write("%s %s %d/%d %d %d %d %s\n" % (name, "f64" if dtype == F64 else "f32", lanes, tl["lanes_per_env"], static, rows, mask is not None,
                                                    " ".join("%.4e" % e for e in err.ravel())))
    assert err.max() <= IDENT_BOUND[dtype], (name, err)


# ---------------------------------------------------------------------------------------------------- 2. identity against the kernels' own adjoint
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", TANGENT_CASES)
def test_identity_against_the_adjoint(name, dtype):
    """every case, per-environment rows, the library's launch shape"""
    _check_identity(name, dtype)


# lanes per environment k_tangent runs at when 16 / 32 / 64 are asked for: a block's LDS holds at most 64 KB, so fp64 TactilePush has no 16-lane
# shape (four contexts), D'Claw (10 dofs, NRM 16) none below 32 lanes in fp32 and 64 in fp64; box_slide (3 dofs) has every shape in both precisions.
# Reached here: NRM 8 at 16 / 32 / 64 lanes in both precisions, NRM 16 at 32 (fp32) and 64 lanes (both).  k_tangent<float, 16, false, 16> and
# <double, 16, false, 32> are run by tests/test_gpu_wide_models.py on models of 9 / 10 dofs on few links; <double, 16, false, 16> cannot be
# reached by any model — four fp64 contexts of 9 or more dofs exceed a block's 64 KB (the census there, tests/test_wide_models.py,
# profiles/r20_wide_models.md).
SHAPES = {("pusher", F64): (32, 32, 64), ("pusher", F32): (16, 32, 64), ("dclaw_position_control", F64): (64, 64, 64),
          ("dclaw_position_control", F32): (32, 32, 64), ("box_slide", F64): (16, 32, 64), ("box_slide", F32): (16, 32, 64)}


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("name", ["pusher", "dclaw_position_control", "box_slide"])
def test_identity_at_every_launch_shape(name, lanes, dtype):
    _check_identity(name, dtype, lanes=lanes, expect_lanes=SHAPES[name, dtype][(16, 32, 64).index(lanes)])


@pytest.mark.parametrize("dtype", [F64, F32])
def test_identity_on_the_shared_model_and_with_a_tactile_mask(dtype):
    _check_identity("pusher", dtype, rows=False)
    _check_identity("pusher", dtype, mask=[True, False, True])
    _check_identity("pad_press", dtype, rows=False, nd=8)


@pytest.mark.parametrize("dtype,rows,edit,variant", [(F32, False, False, "static:pusher"), (F32, True, False, "param:pusher"),
                                                     (F64, False, False, "static:pusher"), (F64, False, True, "param:pusher")])
def test_identity_on_a_compiled_in_model_batch(dtype, rows, edit, variant):
    """the generic k_tangent over the tape a static:pusher / param:pusher batch recorded (K in its records), against that batch's fused adjoint.
    param:pusher: per-environment rows in fp32, an edited model in fp64 (fp64 batches with per-environment tables run the generic kernels, and so
    does an fp64 batch forced to 16 lanes: the compiled-in model has no fp64 instantiation there)"""
    if dtype == F64 and os.environ.get("TSIM_LPE") == "16":
        variant = "generic"
    _check_identity("pusher", dtype, static=True, rows=rows, edit=edit, expect_variant=variant)


# ---------------------------------------------------------------------------------------------------- 3. against the oracle, per output component
_ORACLE_ROWS = {}


def _oracle_rows(name, m, tab, q0, qd0, u, S, wtac):
    """per environment: rows of J^T from the oracle's own adjoint — a unit seed on every component of the last frame's q and var, and the tactile
    seeds wtac [4, T, ntac] over all frames: (dL/du [T, nu], dL/dq0, dL/dqd0, table gradient) each.  Computed once per case."""
    if name in _ORACLE_ROWS:
        return _ORACLE_ROWS[name]
    from oracle.oracle import OracleSim
    T, nr, nv, ntc = u.shape[1], m.ndof_r, m.ndof_var, m.ndof_tactile
    seeds = [("q", i) for i in range(nr)] + [("var", i) for i in range(nv)] + [("tac", k) for k in range(len(wtac) if ntc else 0)]
    out = []
    for e in range(tab.shape[0]):
        o = OracleSim(PU.row_model(m, tab[e]))
        rows = []
        for kind, i in seeds:
            o.reset(q0[e], qd0[e], record=True)
            o.clear_adjoint()
            bad = sum(o.forward(u[e, t], S) for t in range(T))
            assert bad == 0
            g = np.zeros(o._L.orc_table_size(o._h))
            o.set_param_grad(g)
            du = np.zeros((T, m.ndof_u))
            for t in reversed(range(T)):
                dq, dv, dt = np.zeros((S, nr)), np.zeros((S, nv)), np.zeros((S, ntc))
                if kind == "q" and t == T - 1:
                    dq[-1, i] = 1.0
                if kind == "var" and t == T - 1:
                    dv[-1, i] = 1.0
                if kind == "tac":
                    dt[-1] = wtac[i][t]
                du[t] = np.asarray(o.backward_steps(S, dq, dv if nv else None, dt if ntc else None)).reshape(S, -1).sum(0)
            o.set_param_grad(None)
            lq, lv = o.adjoint()
            rows.append((du, lq, lv, g))
        out.append(rows)
    _ORACLE_ROWS[name] = (seeds, out)
    return _ORACLE_ROWS[name]


@pytest.mark.parametrize("name", ["pusher", "pad_press"])
def test_tangent_against_the_oracle_adjoint_per_component(name):
    """fp64, four environments with rows of their own, Newton tol 1e-13: J v of the kernels contracted with the oracle's seeds against the oracle's
    J^T w contracted with v, within 1e-7 of the row's scale sum_j |(J^T w)_j v_j| (floor 1e-9, as tests/test_gpu_parity.py floors its scales)"""
    B, T = 4, T_FRAMES
    m, q0, qd0, u, S = tangent_case(name, B)
    m = copy.deepcopy(m)
    m.F[Bl.TSIM_FH_TOL] = 1e-13
    tab = PU.table_rows(m, B, False, 12)
    wtac = np.random.default_rng(31).normal(size=(4, T, m.ndof_tactile))
    seeds, rows = _oracle_rows(name, m, tab, q0, qd0, u, S, wtac)
    sim = PU.make_sim(m, B, F64, T * S)
    _roll(sim, tab, q0, qd0, u, S)
    nd = 3
    v = _directions(sim, m, T, nd, 23, tab)
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
                assert abs(lhs - rhs) <= 1e-7 * scale, (name, e, kind, i, d, lhs, rhs, scale)
    print("oracle rows %s: worst |J v . w - J^T w . v| / scale = %.3e" % (name, worst))


# ---------------------------------------------------------------------------------------------------- 4. directions are independent
@pytest.mark.parametrize("dtype", [F64, F32])
def test_directions_are_independent(dtype):
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    sim = PU.make_sim(m, B, dtype, T * S)
    tab = PU.table_rows(m, B, dtype == F32, 11)
    _roll(sim, tab, q0, qd0, u, S)
    v = _directions(sim, m, T, 8, 41, tab)
    for k in v:
        v[k][3] = 0                                                           # a zero direction among the others
    all8 = sim.tangent_episode(T, S, want_qd=True, **v)
    for d in range(8):                                                        # ndir = 8 in one launch = eight launches of one, bit for bit
        one = sim.tangent_episode(T, S, want_qd=True, **{k: x[d:d + 1] for k, x in v.items()})
        for k in all8:
            assert torch.equal(all8[k][d], one[k][0]), (d, k)
    assert all(bool((all8[k][3] == 0).all()) for k in all8)                   # ... and the zero direction returns exact zeros
    assert any(bool((all8[k][2] != 0).any()) for k in all8)
    # NULL inputs = zero-filled ones
    for drop in ("du", "dq0", "dqd0", "dtables"):
        vz = {k: (torch.zeros_like(x) if k == drop else x) for k, x in v.items()}
        a = sim.tangent_episode(T, S, want_qd=True, **vz)
        b = sim.tangent_episode(T, S, want_qd=True, **{k: (None if k == drop else x) for k, x in vz.items()})
        assert all(torch.equal(a[k], b[k]) for k in a), drop
    # a direction on a column outside model.param_columns() changes no output bit
    cols = [c for (_, _, _, c) in m.param_columns()]
    other = np.setdiff1d(np.arange(v["dtables"].shape[2]), cols)
    vo = dict(v)
    vo["dtables"] = v["dtables"].clone()
    vo["dtables"][:, :, torch.tensor(other, device=DEV)] = 7.0
    c = sim.tangent_episode(T, S, want_qd=True, **vo)
    assert all(torch.equal(all8[k], c[k]) for k in all8)


# ---------------------------------------------------------------------------------------------------- 5. nothing existing changes
@pytest.mark.parametrize("static,rows,variant", [(False, True, "generic"), (True, False, "static:pusher"), (True, True, "param:pusher")])
def test_tangent_launches_change_nothing(static, rows, variant):
    """roll-out -> 0, 1 or 3 tangent launches -> the adjoint with the parameter buffer, bit for bit: on a generic batch, on a static:pusher batch
    (the shared model: the fully compiled-in forward and fused adjoint) and on a param:pusher one (per-environment rows)"""
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    res = []
    for ntan in (0, 1, 3):
        sim = PU.make_sim(m, B, F32, T * S, static=static)
        tab = PU.table_rows(m, B, True, 11) if rows else None
        out = _roll(sim, tab, q0, qd0, u, S)
        assert sim.kernel_variant() == variant
        v = _directions(sim, m, T, 3, 51, tab)
        for _ in range(ntan):
            sim.tangent_episode(T, S, **v)
        before = sim.last_adjoint_launch()
        assert before["kernel"] is None                                       # the tangent launch is no adjoint launch
        tl, st = sim.tape_len(), sim.get_state()
        w = _seeds(sim, T, T, 52)
        adj = _adjoint(sim, T, S, w)
        res.append([out["q"], out["qd"], out["var"], out["tactile"], out["status"], torch.tensor(tl), st[0], st[1]] + list(adj)
                   + [torch.tensor(sorted(sim.last_adjoint_launch().items()) == sorted({"kernel": "k_backward_z", "param_passes": ("k_param_grad",)}.items()))])
        assert sim.tape_len() == 0 and sim.kernel_variant() == variant
        assert sim.last_adjoint_launch() == {"kernel": "k_backward_z", "param_passes": ("k_param_grad",)}
    for r in res[1:]:
        assert all(torch.equal(a, b) for a, b in zip(res[0], r))


@pytest.mark.parametrize("dtype", [F64, F32])
def test_half_window_continues_the_whole_episode(dtype):
    """the newest half of the episode (BDF1), started from the whole-episode tangent's mid-frame dq, dqd, gives the whole launch's last frames"""
    B, T = 5, 4
    m, q0, qd0, u, S = PU.body_case("pusher", B, T)
    sim = PU.make_sim(m, B, dtype, T * S)
    tab = PU.table_rows(m, B, dtype == F32, 11)
    _roll(sim, tab, q0, qd0, u, S)
    v = _directions(sim, m, T, 3, 61, tab)
    whole = sim.tangent_episode(T, S, want_qd=True, **v)
    h = T // 2
    half = sim.tangent_episode(T - h, S, du=v["du"][:, h:], dq0=whole["dq"][:, h - 1], dqd0=whole["dqd"][:, h - 1], dtables=v["dtables"], want_qd=True)
    for k in whole:
        a, b = whole[k][:, h:].double(), half[k].double()
        assert (a - b).abs().max() <= IDENT_BOUND[dtype] * max(float(a.abs().max()), 1e-30), k
        assert torch.equal(whole[k][:, h:], half[k]), k                       # the two launches sum in the same order


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals():
    from tactilesimulation_amd.host import capi
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    sim = PU.make_sim(m, B, F64, T * S)
    L = capi.lib()
    n = None
    args = lambda h, nf, ns, nd: (h, nf, ns, nd, n, n, n, n, n, n, n, n, n, n)
    assert L.tsim_tangent_episode(*args(None, T, S, 1)) != 0 and b"null batch" in L.tsim_last_error()
    sim.reset(_t(q0, F64), None, backward_flag=True)
    assert L.tsim_tangent_episode(*args(sim._h, T, S, 1)) != 0 and b"no tape" in L.tsim_last_error()
    _roll(sim, None, q0, qd0, u, S)
    for nd in (0, 9, -1):
        assert L.tsim_tangent_episode(*args(sim._h, T, S, nd)) != 0 and b"ndir" in L.tsim_last_error()
    assert L.tsim_tangent_episode(*args(sim._h, T + 1, S, 1)) != 0 and b"sub-steps on the tape" in L.tsim_last_error()
    with pytest.raises(ValueError):
        sim.tangent_episode(T, S, du=torch.zeros((2, T, B, sim.ndof_u)), dq0=torch.zeros((3, B, sim.ndof_r)))
    with pytest.raises(ValueError):
        sim.tangent_episode(T, S, dq0=torch.zeros((B, sim.ndof_r)))
    # a BDF2 model: a window that does not start at tape record 0
    mb, q0b, qd0b, ub, Sb = tangent_case("bdf2:ball_push", B)
    simb = PU.make_sim(mb, B, F64, T * Sb)
    _roll(simb, None, q0b, qd0b, ub, Sb)
    assert L.tsim_tangent_episode(*args(simb._h, T - 1, Sb, 1)) != 0 and b"BDF2" in L.tsim_last_error()
    # ... and a valid launch after the refusals still gives the right answer
    for s_, m_, S_ in ((sim, m, S), (simb, mb, Sb)):
        v = _directions(s_, m_, T, 2, 71)
        o = s_.tangent_episode(T, S_, want_qd=True, **v)
        w = _seeds(s_, T, T, 72)
        assert _identity_errors(o, v, w, _adjoint(s_, T, S_, w)).max() <= IDENT_BOUND[F64]


# ---------------------------------------------------------------------------------------------------- 7. the Jacobian helper and the LM example
def test_episode_jacobian_columns_are_single_direction_tangents():
    from tactilesimulation_amd.functions import episode_jacobian
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    sim = PU.make_sim(m, B, F64, T * S)
    tab = PU.table_rows(m, B, False, 11)
    mask = [True, False, True]
    _roll(sim, tab, q0, qd0, u, S, mask)
    pcols = m.param_columns()
    rng = np.random.default_rng(81)
    pick = [pcols[i] for i in rng.permutation(len(pcols))[:11]]              # more than one launch of eight
    J = episode_jacobian(sim, T, S, pick, tactile_mask=mask)
    nq, nv, nt = T * sim.ndof_r, T * sim.ndof_var, 2 * sim.ndof_tactile
    assert tuple(J.shape) == (B, nq + nv + nt, len(pick))
    for k, pc in enumerate(pick):
        dt = torch.zeros((1, B, tab.shape[1]), device=DEV, dtype=F64)
        dt[0, :, pc[3]] = 1.0
        o = sim.tangent_episode(T, S, dtables=dt, tactile_mask=mask)
        col = torch.cat([o[x][0].permute(1, 0, 2).reshape(B, -1) for x in ("dq", "dvar", "dtactile")], 1)
        assert torch.equal(J[:, :, k], col), pc
    assert bool((J != 0).any())
    with pytest.raises(ValueError):
        episode_jacobian(sim, T, S, [0])


# twice the measured iteration count (every environment, stable or not, is within 2 % after at most 4 iterations: profiles/r17_tangent.md); the
# issue's cap is 40, a tenth of the 400 Adam iterations of test_identification_recovers_contact_parameters
LM_BUDGET = 8


def test_levenberg_marquardt_identification_recovers_contact_parameters():
    """examples/identify_contact_params_lm.py: the assertion of tests/test_gpu_param_grad.py::test_identification_recovers_contact_parameters (kn, kt
    within 2 % on every environment on the true parameters' branches), within LM_BUDGET iterations"""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
    import identify_contact_params_lm as lm
    r = lm.identify(B=8, iters=LM_BUDGET, device=DEV, verbose=False)
    ok = r["stable"]
    print("LM identification: stable %s reached %s kn %s kt %s" % (ok.tolist(), r["reached"].tolist(), r["rel_err"]["kn"].tolist(), r["rel_err"]["kt"].tolist()))
    assert ok.sum() >= 4, ok
    for f in ("kn", "kt"):
        assert np.all(r["rel_err"][f][ok] <= 0.02), (f, r["rel_err"][f][ok])
    assert np.all(r["reached"][ok] >= 1) and np.all(r["reached"][ok] <= LM_BUDGET), r["reached"]
