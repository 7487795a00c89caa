"""The models of tests/contact_shape_models.py, checked on the CPU oracle alone.  No GPU.

tests/test_gpu_contact_pair_shapes.py runs the generic kernels on these models at the edges of the contact-pair and branch loops (P1 - P6 of
profiles/r21_contact_pair_shapes.md).  Here the yardstick and the non-vacuity of every case: the compiled counts are the designed ones and the
native loader agrees; at every named state the oracle reports exactly the designed (pair, point) set and no point is within 1e-5 m of its
primitive's surface, so the fp32 kernels and the fp64 oracle agree on the contact set and the GPU comparisons leave nothing out; the contact
part of the oracle's H is far above the fp32 tolerance, and so is what a dropped last point or last pair would change; the oracle's Jacobian is
the derivative of its residual; every episode converges and takes the same branches on the shared model and on the rows of both roundings; the
launch arithmetic of tests/wide_models.py predicts the shapes the cases are designed for and the staging of the contact points at both thresholds."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
import contact_shape_models as CS      # noqa: E402
import param_grad_util as PU      # noqa: E402
import random_corpus as RC      # noqa: E402
import wide_models as W      # noqa: E402

F32_TOL = 2e-3      # tests/test_gpu_random_models.py test_residual_and_newton_matrix_on_random_structures, fp32
ROWS_SEED = 11      # tests/test_gpu_contact_pair_shapes.py ROWS_SEED
NAMES = list(CS.TABLE)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("contact_shapes")
    return lambda name: CS.table_model(name, d) + (os.path.join(str(d), name, "model.xml"),)


# ---------------------------------------------------------------------------------------------------- the counts
@pytest.mark.parametrize("name", NAMES)
def test_compiled_counts_are_the_designed_ones_and_the_native_loader_agrees(models, name):
    from test_native_model_loader import _native, _same_blob
    m, s, path = models(name)
    nr, nb, pairs, edges = CS.TABLE[name]
    got = CS.counts(m)
    assert got[:5] == (nr, len(pairs), [p["npt"] for p in pairs], sum(p["npt"] for p in pairs), nb), (name, got)
    for (la, lb), p in zip(got[5], s.pairs):      # a world-fixed primitive is merged into the world; one under a branch sits on a moving link
        assert la > 0 and (lb > 0) == (p["prim_on"] is not None), (name, la, lb)
    assert all(int(m.I[int(m.I[Bl.TSIM_IH_OFF_PAIR]) + k * Bl.TSIM_PI_SIZE + Bl.TSIM_PI_FLAGS]) & 1 for k in range(len(pairs)))      # (never reachable otherwise)
    assert [i[1] for i in RC.pair_info(m)] == [p["kind"] == "sphere_plane" for p in pairs]
    assert [RC.PRIM_NAMES[i[0]] for i in RC.pair_info(m)] == [{"ground": "plane", "sphere_plane": "plane"}.get(p["kind"], p["kind"]) for p in pairs]
    nm = _native(path)
    I, F = nm.blob()
    _same_blob(I, F, m)
    assert edges and all(row in ("P1", "P2", "P3", "P3'", "P4", "P5", "P6", "same link", "lb > 0") for row, _, _ in edges)


def test_the_model_list_covers_every_row():
    T = CS.TABLE
    assert sorted(len(T[n][2]) for n in CS.P1) == [1, 4, 5, 8, 9]
    np_nr = {(min(4, len(T[n][2])), T[n][0]) for n in CS.P2}
    assert {(4, 4), (3, 5), (4, 5), (4, 8), (4, 9), (4, 16)} <= np_nr, np_nr
    assert {p["npt"] for n in CS.P3 for p in T[n][2]} >= {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129}
    assert all(p["low"] == p["npt"] - 1 for n in CS.P3 for p in T[n][2][:3])      # "graze": only the tail chunk's last point
    assert [sum(p["npt"] for p in T[n][2]) for n in CS.P5] == [341, 342, 682, 683]
    assert all(sum(p["npt"] - p["nfar"] for p in T[n][2]) == 10 for n in CS.P5)      # all but ten points far from every primitive
    nbnr = [T[n][1] * T[n][0] for n in CS.P6]
    assert (T["p1_9"][0], T["p1_9"][1]) == (9, 9) and nbnr[1] == 16 and 33 <= nbnr[2] <= 36
    for n in CS.P6:      # a contact between two branches, and ground contact
        assert any(p["prim_on"] is not None for p in T[n][2]) and any(p["kind"] == "ground" for p in T[n][2])
    assert any(p["prim_on"] is not None for p in T["p1_5"][2]) and [p["on"] for p in T["p1_5"][2]][:2] == [0, 0]
    rows = {row for n in T for row, _, _ in T[n][3]}
    assert rows >= {"P1", "P2", "P3", "P4", "P5", "P6", "same link", "lb > 0"}
    # low point: point 0, the last point, a point of a middle chunk — each somewhere in the list
    lows = {("first" if p["low"] == 0 else "last" if p["low"] == p["npt"] - 1 else "middle") for n in T for p in T[n][2] if p["npt"] > 2}
    assert lows == {"first", "last", "middle"}


# ---------------------------------------------------------------------------------------------------- the states
def _contact_margin(m, touching, q1, q0, qd0, u, Ho=None):
    """largest row-relative share of the contact part of H: H minus H of the model without contact on the touching pairs"""
    from oracle.oracle import OracleSim
    if Ho is None:
        Ho = OracleSim(m).residual(q1, q0, qd0, u, which=0)[1]
    H0 = OracleSim(RC.without_contact(m, touching)).residual(q1, q0, qd0, u, which=0)[1]
    return (np.abs(Ho - H0).max(1) / np.abs(Ho).max(1)).max()


@pytest.mark.parametrize("name", NAMES)
def test_named_states_touch_exactly_what_they_were_designed_for(models, name):
    from oracle.oracle import OracleSim
    m, s, _ = models(name)
    o = OracleSim(m)
    ns = CS.named_states(s, m)
    assert len(ns) == 3 + 2 * len(s.pairs)
    for n, ((q1, q0, qd0, u), want) in ns.items():
        got = o.contact_list(q1, qd0, max_rows=1024)
        assert {(r[0], r[1]) for r in got} == want and len(got) == len(want), (name, n)
        g = np.concatenate(CS.gaps(s, q1))
        assert np.abs(g).min() >= CS.MARGIN, (name, n, np.abs(g).min())      # nothing within 1e-5 m of a surface, either side
        assert {(j, i) for j, gj in enumerate(CS.gaps(s, q1)) for i in np.flatnonzero(gj < 0)} == want, (name, n)
        assert all(abs(r[3]) >= CS.MARGIN for r in got)
        if want:
            share = _contact_margin(m, {p for p, _ in want}, q1, q0, qd0, u)
            assert share >= 10 * F32_TOL, (name, n, share)
    # "hover": every pair's bounding sphere reaches its primitive, no point penetrates; "none": every pair is out of reach (a quarter of a metre and more against GAP)
    assert all(gj.min() < 2 * CS.GAP + CS.STEP for gj in CS.gaps(s, ns["hover"][0][0])) and all(gj.min() > 0.2 for gj in CS.gaps(s, ns["none"][0][0]))


@pytest.mark.parametrize("name", CS.P3 + CS.P1[1:])
def test_a_dropped_last_point_or_last_pair_would_be_seen(models, name):
    """P3, "only<j>:graze" (only the last point of the tail chunk touches): H of the model with THAT POINT moved a metre up differs from H by 10 x
    the fp32 tolerance in some row.  P1, "only<last>:deep": the same for the model without the last pair, and at "all" too"""
    from oracle.oracle import OracleSim
    m, s, _ = models(name)
    ns = CS.named_states(s, m)
    o = OracleSim(m)
    ncpt, f0 = int(m.I[Bl.TSIM_IH_NCPT]), int(m.I[Bl.TSIM_IH_FOFF_CPT])
    if name in CS.P3:
        pt0 = np.cumsum([0] + [p["npt"] for p in s.pairs])
        for j, p in enumerate(s.pairs):
            (q1, q0, qd0, u), want = ns["only%d:graze" % j]
            assert want == {(j, p["low"])}
            m2 = copy.copy(m)
            m2.F = m.F.copy()
            m2.F[f0 + 2 * ncpt + pt0[j] + p["low"]] += 1.0
            Ho, H2 = o.residual(q1, q0, qd0, u, which=0)[1], OracleSim(m2).residual(q1, q0, qd0, u, which=0)[1]
            assert (np.abs(Ho - H2).max(1) / np.abs(Ho).max(1)).max() >= 10 * F32_TOL, (name, j)
    else:
        last = len(s.pairs) - 1
        for n in ("only%d:deep" % last, "all"):
            (q1, q0, qd0, u), want = ns[n]
            assert any(p == last for p, _ in want)
            assert _contact_margin(m, {last}, q1, q0, qd0, u) >= 10 * F32_TOL, (name, n)


@pytest.mark.parametrize("name", ["p1_5", "p1_9", "p2_4x16", "p3_c", "p5_342"])
def test_oracle_jacobian_is_the_derivative_of_its_residual(models, name):
    """tests/test_oracle_physics.py test_newton_matrix_is_exact: central differences of step 1e-7, within 1e-8 of the largest entry, at three states"""
    from oracle.oracle import OracleSim
    m, s, _ = models(name)
    o = OracleSim(m)
    ns = CS.named_states(s, m)
    for n in ("all", "only0:graze", "only%d:deep" % (len(s.pairs) - 1)):
        (q1, q0, qd0, u), _ = ns[n]
        _, H = o.residual(q1, q0, qd0, u, which=0)
        Hfd = np.zeros_like(H)
        for k in range(m.ndof_r):
            d = np.zeros(m.ndof_r); d[k] = 1e-7
            Hfd[:, k] = (o.residual(q1 + d, q0, qd0, u) - o.residual(q1 - d, q0, qd0, u)) / 2e-7
        assert np.abs(H - Hfd).max() < 1e-8 * np.abs(H).max(), (name, n, np.abs(H - Hfd).max() / np.abs(H).max())


# ---------------------------------------------------------------------------------------------------- the episodes
def _episode_sigs(m, q0, qd0, u, S):
    from oracle.oracle import OracleSim
    o = OracleSim(m)
    o.reset(q0, qd0)
    bad, sigs, touched = 0, [], set()
    for t in range(u.shape[0]):
        for _ in range(S):
            b, sg = o.forward_sig(u[t], 1)
            bad += b
            sigs.append(sg[0])
            touched |= {r[0] for r in o.contact_list(*o.state(), max_rows=1024)}
    return bad, np.stack(sigs), touched


EPISODES = [(n, False) for n in sorted(set(CS.EPISODE_MODELS + CS.P1 + CS.P2 + CS.P3 + CS.TANGENT_MODELS))] + [(n, True) for n in CS.GRADIENT_MODELS]


@pytest.mark.parametrize("name,only", EPISODES, ids=["%s-%s" % (n, "one_pair" if o else "all_pairs") for n, o in EPISODES])
def test_every_episode_converges_and_keeps_one_branch_signature(models, name, only):
    """the episodes of the GPU file (one_pair: the table-gradient test's, environment e presses pair e mod npair alone): bad == 0, and ONE
    signature sequence per environment — the model's Newton tolerance and the 1e-13 of the fp64 comparisons take the same branches at every
    sub-step, and the per-environment rows of both roundings converge; the pressed pairs stay in contact"""
    m, s, _ = models(name)
    nB = CS.gradient_batch(name) if only else CS.B_ENVS      # (one_pair: every pair is the lone touching pair of some environment)
    q0, qd0, u, S = CS.episode_case(s, m, B=nB, only=only)
    assert not only or {e % len(s.pairs) for e in range(nB)} == set(range(len(s.pairs)))
    tight = copy.deepcopy(m)
    tight.F[Bl.TSIM_FH_TOL] = 1e-13
    for e in range(nB):
        bad, sig, touched = _episode_sigs(m, q0[e], qd0[e], u[e], S)
        # (one_pair: a branch that was raised to bring its primitive to the body falls back on its own ground pair — `touched` may hold that pair too)
        assert bad == 0 and touched >= CS.touching_of_env(s, e, only), (name, e, touched)
        assert (sig[:, 0] >= 1).sum() >= 4 and sig[0, 0] >= 1, (name, e, sig)      # in contact at the first sub-step and at four of the six at least
        for mm in (tight, PU.row_model(m, PU.table_rows(m, nB, False, ROWS_SEED)[e].astype(np.float64)),
                   PU.row_model(m, PU.table_rows(m, nB, True, ROWS_SEED)[e].astype(np.float64))):
            b2, s2, _ = _episode_sigs(mm, q0[e], qd0[e], u[e], S)
            assert b2 == 0, (name, e)
            if mm is tight:
                assert np.array_equal(s2, sig), (name, e, sig, s2)


# ---------------------------------------------------------------------------------------------------- the launch arithmetic
def test_the_edges_run_at_the_lanes_they_were_designed_for(models):
    """CS.TABLE's edges name the lanes per environment an edge needs; tests/wide_models.py's restated launch arithmetic gives that shape when the
    lanes are forced, in fp32 at least (the GPU file asserts the library's launch_info against the same arithmetic, and CS.SHAPES is on record)"""
    for name, (nr, nb, pairs, edges) in CS.TABLE.items():
        m, s, _ = models(name)
        for esz in (4, 8):
            for rows in (False, True):
                got = tuple(W.forced_shape(m, l, esz, rows)[0] for l in (16, 32, 64))
                assert got == CS.SHAPES[name][esz, rows], (name, esz, rows, got)
        for row, lanes, what in edges:
            if lanes:
                assert CS.SHAPES[name][4, False][(16, 32, 64).index(lanes)] == lanes, (name, row, lanes, what)
        if name in CS.TANGENT_MODELS:      # k_tangent with eight directions and dtables: its own, possibly wider, shape
            for esz in (4, 8):
                got = tuple(W.tangent_shape(m, l, esz) for l in (16, 32, 64))
                assert got == CS.TAN_SHAPES[name][esz], (name, esz, got)
        if name in CS.SMALL:      # built so that the 16-lane edges run at 16 lanes in EVERY kernel and both precisions, k_tangent<double> included
            assert CS.TAN_SHAPES[name] == {4: (16, 32, 64), 8: (16, 32, 64)} and all(v == (16, 32, 64) for v in CS.SHAPES[name].values())
    assert {p["npt"] for n in CS.SMALL for p in CS.TABLE[n][2]} >= {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129}
    assert {(min(4, len(CS.TABLE[n][2])), CS.TABLE[n][0]) for n in CS.SMALL} >= {(4, 4), (3, 5), (4, 5)}
    # the figures the issue's list ends with: np nr = 32 and 36 at 32 lanes in BOTH precisions, nb nr = 81 at 64, npt 65 and 129 at 64
    for n in ("p2_4x8", "p2_4x9"):
        assert CS.SHAPES[n][8, False][1] == 32 and CS.SHAPES[n][4, False][1] == 32
    for n in ("p1_4", "p2_3x5", "p1_5"):
        assert CS.SHAPES[n][8, False][0] == 16 and CS.SHAPES[n][4, True][0] == 16


@pytest.mark.parametrize("name", CS.P5)
def test_staging_of_the_contact_points_at_both_thresholds(models, name):
    """csrc/tsim_hip.hip decide_stage_cpt as tests/wide_models.py restates it: staged iff 3 ncpt esz <= 8192 (the shapes of these two-dof models
    do not change with the staging and every block fits), with shared and with per-environment tables, and the block is larger by the staged
    points exactly"""
    m, s, _ = models(name)
    ncpt = int(m.I[Bl.TSIM_IH_NCPT])
    for esz in (4, 8):
        want = 3 * ncpt * esz <= W.CPT_LDS_BYTES
        assert want == {(341, 4): True, (342, 4): True, (682, 4): True, (683, 4): False, (341, 8): True, (342, 8): False, (682, 8): False, (683, 8): False}[ncpt, esz]
        for rows in (False, True):
            for lanes in (16, 32, 64):
                assert W.stages_cpt(m, lanes, esz, rows) == want, (name, esz, rows, lanes)
                assert W.forced_shape(m, lanes, esz, rows)[0] == lanes
                ns = 64 // lanes
                with_, without = W.block_bytes(m, ns, esz, rows, True), W.block_bytes(m, ns, esz, rows, False)
                assert abs(with_ - without - 3 * ncpt * esz) < 32 and with_ <= W.LDS_CAP, (name, esz, rows, lanes, with_, without)      # (the table is rounded to four reals, the block to 16 bytes)
                assert W.forced_shape(m, lanes, esz, rows)[1] == (with_ if want else without)
