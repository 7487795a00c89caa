"""The body-group columns of dtables as directions of the tangent pass (include/tsim.h tsim_tangent_episode with tsim_set_param_grad_groups'
TSIM_PG_INERTIAL / MOTOR / LIMIT on: k_tangent_body_src -> k_tangent; link mass, centre of mass, inertia; motor lo hi P D; limit lo hi k).

k_tangent_body_src is k_param_grad_body read forwards, so the pass is held to the kernels' own adjoint by the inner-product identity
<w, J v> = <J^T w, v> of tests/test_gpu_tangent.py (its error measure, _identity_errors), with every group on on both sides and random directions on
du, dq0, dqd0, the contact columns AND the body columns, per environment, none left out.  The conditions are the existing identity test's — below
1e-10 in fp64, below 1e-4 in fp32 — and the asserted bound is 10 x the largest value measured over every case of test 1 on the MI355X
(profiles/r18_tangent_body.md), per precision, the rule of test_gpu_tangent.py's IDENT_BOUND.  The fp32 identity holds only because the pre-pass forms
the sub-step's discrete acceleration as k_param_grad_body does, from the taped double positions.
Then: each group alone (a direction on a group that is off changes no bit); unit body directions move something, and the columns that must give
exact zeros do; J v against the fp64 oracle's exact body adjoint (1e-7 of sum |g_j v_j|, floor 1e-9, Newton tol 1e-13: the setting and bound of
test_gpu_tangent.py's oracle test; tests/test_tangent_body_yardstick.py pins bad == 0 and the oracle's body gradient to its finite differences, on
the CPU); the launch shapes; the pre-pass's chunk layouts; bit-exactness (directions independent of ndir, nothing existing changes, the workspace
is allocated once: two calls under torch.cuda.graph capture after a warm-up call — a call that had to allocate is refused under capture); the
Jacobian helper; the Levenberg-Marquardt mass identification."""
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
import test_gpu_tangent as TG      # noqa: E402
from test_tangent_body_yardstick import BODY_CASES, ORACLE_CASES, body_tangent_case, body_direction      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = PU.DEV
F64, F32 = torch.float64, torch.float32
# the conditions (the existing identity test's) and 10 x the maxima measured on the MI355X over every case of test 1 (profiles/r18_tangent_body.md):
# fp64 2.42e-15, fp32 1.55e-6, both on tactile_insertion (six massless intermediate links, 64 lanes); every other case <= 2.4e-16 / 1.7e-7
IDENT_CONDITION = {F64: 1e-10, F32: 1e-4}
IDENT_BOUND = {F64: 2.5e-14, F32: 1.6e-5}
STATS = os.environ.get("TSIM_TANGENT_BODY_STATS")      # a file: every identity error is appended to it (profiles/r18_tangent_body.md)
GROUP_OF = {"link": "inertial", "motor": "motor", "limit": "limit"}


def _body_cols(m, groups):
    return [c for (kind, _, _, c) in m.body_param_columns() if GROUP_OF[kind] in groups]


def _directions(sim, m, T, nd, seed, tab, groups=PU.BODY, contact=True, state=True):
    """test_gpu_tangent's random directions, and on the body columns of `groups` random entries of the size of the entry (|entry| + 0.1)"""
    v = TG._directions(sim, m, T, nd, seed, tab)
    base = sim.base_tables().double().cpu().numpy() if tab is None else np.asarray(tab, dtype=np.float64)
    dtab = v["dtables"].double().cpu().numpy() if contact else np.zeros((nd,) + base.shape)
    cols = _body_cols(m, groups)
    dtab[:, :, cols] = body_direction(seed, (nd, sim.B, len(cols)), base[:, cols])
    v["dtables"] = TG._t(dtab, sim.dtype)
    if not state:
        v["du"] = v["dq0"] = v["dqd0"] = None
    return v


def _identity(name, dtype, lanes=0, groups=PU.ALL, nd=3, B=5, case=None, envs=None, static=False):
    """roll the case out, tangent and adjoint with `groups` on, the mask restored afterwards: [nd, B] identity errors (of `envs`)"""
    m, q0, qd0, u, S = case or body_tangent_case(name, B)
    T = u.shape[1]
    sim = PU.make_sim(m, B, dtype, T * S, lanes=lanes, static=static)
    tab = PU.table_rows(m, B, dtype == F32, 11)
    TG._roll(sim, tab, q0, qd0, u, S)
    info = sim.tangent_launch_info(nd, True)
    batch = sim.launch_info()                                             # the shape of the parameter passes, the pre-pass among them
    batch_lanes, variant = batch["lanes_per_env"], sim.kernel_variant()
    sim.set_param_grad_groups(groups)
    try:
        assert sim.tangent_launch_info(nd, True) == info                 # the launch shape does not depend on the mask
        v = _directions(sim, m, T, nd, 21, tab, groups=[g for g in groups if g != "contact"])
        o = sim.tangent_episode(T, S, want_qd=True, **v)
        assert sim.tape_len() == T * S
        w = TG._seeds(sim, T, T, 22)
        adj = TG._adjoint(sim, T, S, w)
    finally:
        sim.set_param_grad_groups(("contact",))
    bcols = _body_cols(m, groups)
    assert bool((adj[3][:, bcols] != 0).any()), name                      # the adjoint side has body entries: the identity is about them
    err = TG._identity_errors(o, v, w, adj)
    if envs is not None:
        err = err[:, envs]
    tag = "%s %s lanes %d B %d groups %s" % (name, "f64" if dtype == F64 else "f32", lanes, B, "+".join(groups))
    print("body identity %-70s (k_tangent at %2d lanes): max %.3e median %.3e" % (tag, info["lanes_per_env"], err.max(), np.median(err)))
    if STATS:
        with open(STATS, "a") as f:
            f.write("%s | %s\n" % (tag, " ".join("%.4e" % e for e in err.ravel())))
    return err, dict(info, batch_lanes=batch_lanes, batch_lds_bytes=batch["lds_bytes"], variant=variant)


# ---------------------------------------------------------------------------------------------------- 1. identity against the kernels' own adjoint
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", BODY_CASES)
def test_identity_with_body_directions(name, dtype):
    """every case, per-environment rows, every group on, every environment compared.  On the parent commit the body columns of dtables are not
    read and the identity misses by the size of the body terms.  Measured maxima: profiles/r18_tangent_body.md"""
    err, _ = _identity(name, dtype)
    assert err.max() < IDENT_CONDITION[dtype] and err.max() <= IDENT_BOUND[dtype], (name, err)


# ---------------------------------------------------------------------------------------------------- 2. each group alone
@pytest.mark.parametrize("group", PU.BODY)
def test_each_group_alone(group):
    err, _ = _identity("limit_push", F64, groups=("contact", group))
    assert err.max() <= IDENT_BOUND[F64], (group, err)
    # a direction supported only on the groups that are off: the bits of a zero direction
    B = 5
    m, q0, qd0, u, S = body_tangent_case("limit_push", B)
    T = u.shape[1]
    sim = PU.make_sim(m, B, F64, T * S)
    tab = PU.table_rows(m, B, False, 11)
    TG._roll(sim, tab, q0, qd0, u, S)
    off = [g for g in PU.BODY if g != group]
    sim.set_param_grad_groups(("contact", group))
    try:
        v = _directions(sim, m, T, 2, 23, tab, groups=off, contact=False, state=False)
        assert bool((v["dtables"] != 0).any())
        a = sim.tangent_episode(T, S, want_qd=True, **v)
        z = sim.tangent_episode(T, S, want_qd=True, dtables=torch.zeros_like(v["dtables"]))
        on = sim.tangent_episode(T, S, want_qd=True, **_directions(sim, m, T, 2, 23, tab, groups=[group], contact=False, state=False))
    finally:
        sim.set_param_grad_groups(("contact",))
    assert all(torch.equal(a[k], z[k]) for k in a) and all(bool((a[k] == 0).all()) for k in a), group
    assert bool((on["dq"] != 0).any()), group


# ---------------------------------------------------------------------------------------------------- 3. body directions move something
def _motor_of(m, col):
    n = (col - int(m.I[Bl.TSIM_IH_FOFF_MOTOR])) // Bl.TSIM_MF_SIZE
    return n, int(m.I[int(m.I[Bl.TSIM_IH_OFF_MOTOR]) + n * Bl.TSIM_MI_SIZE + Bl.TSIM_MI_CTRL])


@pytest.mark.parametrize("name", ["limit_push", "pusher"])
def test_unit_body_directions_move_something(name):
    """a vacuous identity (both sides zero on the body columns) would pass test 1: unit directions on a mass column, on the hi (force control) or P
    (position control) column of a motor and on the limit columns of the dofs that are outside their limits must move q; P of a force motor and lo
    of a position motor must give exact zeros"""
    from body_param_util import active_limit_columns
    B = 2
    m, q0, qd0, u, S = body_tangent_case(name, B)
    T = u.shape[1]
    cols = m.body_param_columns()
    states = PU.oracle_episode(m, q0[0], u[0], S, PU.loss_weights(m, T), grad=False, qd0=qd0[0])[4]
    # (the mass of a link that translates: limit_push's slider, TactilePush's box — the mass of its gripper base, which only turns about an axis
    # through its centre of mass, moves nothing, measured: an exact 0)
    joint = {"limit_push": "slider", "pusher": "box"}[name]
    moving = [next(bc for bc in cols if PU.kind_of(bc) == "mass" and bc[1][0] == joint)]
    zero = []
    for bc in cols:
        if bc[0] == "motor":
            ctrl = _motor_of(m, bc[3])[1]
            if (bc[2], ctrl) in (("hi", 0), ("P", 1)):
                moving.append(bc)
            if (bc[2], ctrl) in (("P", 0), ("lo", 1)):
                zero.append(bc)
    lim = [cols[i] for i in sorted(active_limit_columns(m, cols, states))]
    moving += lim
    if name == "limit_push":
        assert {bc[2] for bc in lim} == {"lo", "hi", "k"} and {bc[2] for bc in zero} == {"P", "lo"}, (lim, zero)
        assert {bc[2] for bc in moving if bc[0] == "motor"} == {"hi", "P"}
    sim = PU.make_sim(m, B, F64, T * S)
    TG._roll(sim, None, q0, qd0, u, S)
    sim.set_param_grad_groups(PU.ALL)
    try:
        for bcs, moves in ((moving, True), (zero, False)):
            for c0 in range(0, len(bcs), 8):
                chunk = bcs[c0:c0 + 8]
                dt = torch.zeros((len(chunk), B, sim.base_tables().shape[1]), device=DEV, dtype=F64)
                for d, bc in enumerate(chunk):
                    dt[d, :, bc[3]] = 1.0
                o = sim.tangent_episode(T, S, want_qd=True, dtables=dt)
                for d, bc in enumerate(chunk):
                    top = float(o["dq"][d].abs().max())
                    print("unit direction %s %s: max |dq| %.3e" % (name, bc[:3], top))
                    assert (top > 0) if moves else all(bool((o[k][d] == 0).all()) for k in o), (name, bc, top)
    finally:
        sim.set_param_grad_groups(("contact",))


# ---------------------------------------------------------------------------------------------------- 4. against the oracle's exact body adjoint
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_body_tangent_against_the_oracle_adjoint(name):
    """fp64, four environments with rows of their own, Newton tol 1e-13: the kernels' J v contracted with the loss weights against the oracle's
    groups = ALL table gradient contracted with dp — three directions on every column, contact and body, and three on the body columns alone
    (the body part by itself) — within 1e-7 of sum_j |g_j v_j| (floor 1e-9)"""
    B = 4
    m, q0, qd0, u, S = body_tangent_case(name, B)
    T = u.shape[1]
    m = copy.deepcopy(m)
    m.F[Bl.TSIM_FH_TOL] = 1e-13
    tab = PU.table_rows(m, B, False, 12)
    w = PU.loss_weights(m, T)
    sim = PU.make_sim(m, B, F64, T * S)
    TG._roll(sim, tab, q0, qd0, u, S)
    sim.set_param_grad_groups(PU.ALL)
    try:
        va = _directions(sim, m, T, 3, 25, tab, state=False)["dtables"]
        vb = _directions(sim, m, T, 3, 26, tab, contact=False, state=False)["dtables"]
        dt = torch.cat([va, vb], 0)
        o = {k: x.cpu().numpy() for k, x in sim.tangent_episode(T, S, dtables=dt).items()}
    finally:
        sim.set_param_grad_groups(("contact",))
    dt = dt.cpu().numpy()
    assert np.any(o["dq"][3:] != 0)
    worst = 0.0
    for e in range(B):
        g, _, bad, _ = PU.oracle_cached(PU.row_model(m, tab[e]), q0[e], qd0[e], u[e], S, w, groups=PU.ALL)[1]
        assert bad == 0, (name, e)
        for d in range(6):
            lhs = float((o["dq"][d, :, e] * w[0]).sum())
            if m.ndof_var:
                lhs += float((o["dvar"][d, :, e] * w[1]).sum())
            if m.ndof_tactile:
                lhs += float((o["dtactile"][d, :, e] * w[2]).sum())
            parts = g * dt[d, e]
            scale = max(float(np.abs(parts).sum()), 1e-9)
            worst = max(worst, abs(lhs - parts.sum()) / scale)
            assert abs(lhs - parts.sum()) <= 1e-7 * scale, (name, e, d, lhs, parts.sum(), scale)
    print("oracle body adjoint %s: worst |J v . w - g . v| / scale = %.3e" % (name, worst))


# ---------------------------------------------------------------------------------------------------- 5. launch shapes
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("name", ["box_slide", "limit_push"])
def test_identity_at_every_launch_shape(name, lanes, dtype):
    """The batch is forced to 16 / 32 / 64 lanes per environment, which both models have in both precisions.  The pre-pass takes the batch's
    shape as k_param_grad_body does (ts_plan with no lanes of its own), and that shape is asserted here through launch_info; the library has no
    diagnostic that reports the pre-pass's own launch, so its width is pinned through the batch's, as the body gradient's tests pin theirs.
    k_tangent runs at its own shape (tangent_launch_info, which the mask does not change: asserted in _identity), here the same"""
    err, info = _identity(name, dtype, lanes=lanes)
    assert info["batch_lanes"] == lanes and info["lanes_per_env"] == lanes, (name, lanes, info)
    assert err.max() <= IDENT_BOUND[dtype], (name, lanes, err)


# ---------------------------------------------------------------------------------------------------- 6. chunk layouts of the pre-pass
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("kind", ["single", "len1", "even", "ragged"])
def test_chunk_layouts_of_the_pre_pass(kind, dtype):
    """limit_push, 8 frames x 2 sub-steps, 16 lanes, per-environment states, controls and tables, each layout at the smallest batch that has it on
    the device: with more than one sub-step per chunk the t - 1 and t - 2 records of a chunk's first sub-step belong to the chunk before.  The
    identity on up to 32 sampled environments with the first, the last and the last block"""
    from test_gpu_body_param_grad_oracle import _batch_for, _limit_push_case, _sample
    T, lanes = 8, 16
    B = _batch_for(kind, T * 2)
    case = _limit_push_case(B, T, 41)
    assert case[4] == 2 and PU.layout_kind(B, T * 2) == kind
    envs = _sample(B, 32, B, 64 // lanes) if B > 32 else np.arange(B)
    err, _ = _identity("limit_push[%s]" % kind, dtype, lanes=lanes, B=B, case=case, envs=envs)
    assert err.max() <= IDENT_BOUND[dtype], (kind, B, err)


# ---------------------------------------------------------------------------------------------------- 7. bit-exactness
def _rolled(name, dtype, B=5, static=False, rows=True):
    m, q0, qd0, u, S = body_tangent_case(name, B)
    T = u.shape[1]
    sim = PU.make_sim(m, B, dtype, T * S, static=static)
    tab = PU.table_rows(m, B, dtype == F32, 11) if rows else None
    out = TG._roll(sim, tab, q0, qd0, u, S)
    return sim, m, tab, T, S, out


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["limit_push", "pusher"])
def test_directions_are_independent_and_the_default_mask_is_unchanged(name, dtype):
    sim, m, tab, T, S, _ = _rolled(name, dtype)
    v = _directions(sim, m, T, 8, 41, tab)
    bcols = torch.tensor(_body_cols(m, PU.BODY), device=DEV)
    vz = dict(v)
    vz["dtables"] = v["dtables"].clone()
    vz["dtables"][:, :, bcols] = 0
    run = lambda x: sim.tangent_episode(T, S, want_qd=True, **x)
    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in a)
    before = run(v)                                                           # the default mask: the body columns are not read
    assert same(before, run(vz))
    sim.set_param_grad_groups(PU.ALL)
    try:
        all8 = run(v)
        for d in range(8):                                                    # ndir = 8 in one launch = eight launches of one, bit for bit
            assert same({k: x[d] for k, x in all8.items()}, {k: x[0] for k, x in run({k: x[d:d + 1] for k, x in v.items()}).items()}), d
        assert not same(all8, before)                                         # (the body directions do something)
        assert same(run(vz), before)                                          # body groups on, zero body columns == the default mask
        nt = {k: (None if k == "dtables" else x) for k, x in v.items()}
        assert same(run(nt), run({k: (torch.zeros_like(x) if k == "dtables" else x) for k, x in v.items()}))      # dtables NULL == zeros
    finally:
        sim.set_param_grad_groups(("contact",))
    assert same(run(v), before)                                               # ... and the default mask after the feature's paths ran


@pytest.mark.parametrize("static,variant", [(False, "generic"), (True, "param:pusher")])
def test_tangent_launches_with_body_directions_change_nothing(static, variant):
    """roll-out -> 0 or 2 tangent launches with body directions -> the adjoint with the parameter buffer and every group on, bit for bit"""
    res = []
    for ntan in (0, 2):
        sim, m, tab, T, S, out = _rolled("pusher", F32, static=static)
        assert sim.kernel_variant() == variant
        sim.set_param_grad_groups(PU.ALL)
        try:
            v = _directions(sim, m, T, 3, 51, tab)
            for _ in range(ntan):
                sim.tangent_episode(T, S, **v)
            tl, st = sim.tape_len(), sim.get_state()
            w = TG._seeds(sim, T, T, 52)
            adj = TG._adjoint(sim, T, S, w)
            assert sim.last_adjoint_launch()["param_passes"] == ("k_param_grad", "k_param_grad_body")
        finally:
            sim.set_param_grad_groups(("contact",))
        res.append([out["q"], out["qd"], out["var"], out["tactile"], out["status"], torch.tensor(tl), st[0], st[1]] + list(adj) + [torch.tensor(sim.tape_len())])
        assert sim.tape_len() == 0 and sim.kernel_variant() == variant
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))


def test_the_workspace_is_allocated_once():
    """hipMalloc is invisible to torch.cuda.memory_allocated, so: a call that has to allocate the body columns' workspace is refused under stream
    capture, and after a warm-up call of the same size two calls are captured and replay to the eager bits"""
    sim, m, tab, T, S, _ = _rolled("limit_push", F32)
    sim.set_param_grad_groups(PU.ALL)
    try:
        v = _directions(sim, m, T, 4, 61, tab)
        small = {k: x[:2].contiguous() for k, x in v.items()}
        eager_small = sim.tangent_episode(T, S, **small)                      # the warm-up of the SMALLER size
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            sim.tangent_episode(T, S, **small)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            with pytest.raises(RuntimeError, match="workspace"):              # four directions need a larger workspace: refused, nothing launched
                sim.tangent_episode(T, S, **v)
            a = sim.tangent_episode(T, S, **small)
            b = sim.tangent_episode(T, S, **small)
        for x in list(a.values()) + list(b.values()):
            x.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a[k], eager_small[k]) and torch.equal(b[k], eager_small[k]) for k in a)
        big = sim.tangent_episode(T, S, **v)                                  # outside a capture the workspace grows
        assert all(torch.equal(big[k][:2], eager_small[k]) for k in big)
        # ... and the captured graph, which names the workspace it was captured with, still replays to the eager bits: that workspace is kept
        # until the batch goes, not freed, and a second growth leaves it alone as well
        torch.cuda.synchronize()
        for grow in (None, 8):
            if grow:
                sim.tangent_episode(T, S, **_directions(sim, m, T, grow, 62, tab))
            for x in list(a.values()) + list(b.values()):
                x.fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a[k], eager_small[k]) and torch.equal(b[k], eager_small[k]) for k in a), grow
            again = sim.tangent_episode(T, S, **small)
            assert all(torch.equal(again[k], eager_small[k]) for k in again), grow
    finally:
        sim.set_param_grad_groups(("contact",))


# ---------------------------------------------------------------------------------------------------- 8. the Jacobian helper
def test_episode_jacobian_takes_body_columns_of_the_groups_that_are_on():
    from tactilesimulation_amd.functions import episode_jacobian
    sim, m, tab, T, S, _ = _rolled("limit_push", F64)
    mass = next(bc for bc in m.body_param_columns() if PU.kind_of(bc) == "mass" and m.F[bc[3]] > 0)
    lim = next(bc for bc in m.body_param_columns() if bc[0] == "limit")
    with pytest.raises(ValueError, match="inertial"):
        episode_jacobian(sim, T, S, [mass])
    sim.set_param_grad_groups(("contact", "inertial"))
    try:
        with pytest.raises(ValueError, match="limit"):
            episode_jacobian(sim, T, S, [mass, lim])
        pick = [mass, m.param_columns()[0]]
        J = episode_jacobian(sim, T, S, pick)
        for k, pc in enumerate(pick):
            dt = torch.zeros((1, sim.B, tab.shape[1]), device=DEV, dtype=F64)
            dt[0, :, pc[3]] = 1.0
            o = sim.tangent_episode(T, S, dtables=dt)
            col = torch.cat([o[x][0].permute(1, 0, 2).reshape(sim.B, -1) for x in ("dq", "dvar", "dtactile") if x in o], 1)
            assert torch.equal(J[:, :, k], col), pc
        assert bool((J[:, :, 0] != 0).any())
    finally:
        sim.set_param_grad_groups(("contact",))


# ---------------------------------------------------------------------------------------------------- 10. the Levenberg-Marquardt mass identification
# twice the measured iteration count — the slowest environment is within 1 % after 10 iterations from 0.5x and after 4 from 2x
# (profiles/r18_tangent_body.md); the cap is 40
LM_BUDGET = 20


def test_levenberg_marquardt_recovers_the_box_mass():
    """examples/identify_box_mass_lm.py: every environment's mass within 1 % from both starts, within LM_BUDGET iterations"""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
    import identify_box_mass_lm as lm
    res = lm.run(B=8, iters=LM_BUDGET, device=DEV, verbose=False)
    for f, r in res.items():
        print("LM mass identification from %sx: reached %s rel. error %s" % (f, r["reached"].tolist(), r["rel_err"].tolist()))
        assert np.all(r["rel_err"] <= 0.01), (f, r["rel_err"])
        assert np.all(r["reached"] >= 1) and np.all(r["reached"] <= LM_BUDGET), (f, r["reached"])
