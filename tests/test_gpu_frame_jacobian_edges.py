"""k_frame_jacobian where its own loops and its launch plan end: the pivoted solve with eight right-hand sides exchanging rows, the column passes'
tails, the Jvar task loop's trips, n = NRM, the plan's doublings and its refusal.

tests/test_gpu_frame_jacobians.py holds the kernel to k_tangent on models whose taped Newton matrix keeps its pivots on the diagonal (all but
wide10, one swap), so solve_lanes_many ran with mycol == lane, and with ncol mod 8 in {1, 3, 4, 5, 6}.  The cases here are models of the random
corpus (tests/frame_jacobian_cases.py) that tests/test_frame_jacobian_cases.py shows, on the CPU oracle, to pivot off the diagonal in every
environment, unambiguously (16 of the 19; three are there for their sizes alone), and to carry the sizes: ncol mod 8 = 0, 2, 7, n = 8 and n = 16, 36 / 64 / 80 / 91 Jvar tasks.  B = 5, T = 3 frames of
S = 2 sub-steps, per-environment rows; every launch shape is asserted against the restated plan (tests/wide_models.py frame_jacobian_shape) and
against the table of the case file: lanes, LDS bytes, blocks.

Bounds.  The columns against k_tangent: BOUND of tests/test_gpu_frame_jacobians.py (10 x the largest error of that file's cases: fp64 3.9e-13, fp32
1.9e-4 of the row's scale) for every case that stays under it; a case that does not would have an entry in OWN_MEASURED and 10 x it as its bound,
the measured value under CAP (1e-10 / 1e-4) — every case stays under BOUND, so the table is empty.  Measured on an MI355X (profiles/r23_frame_jacobian_edges.md), largest column / Jvar error per type over the new cases:
MEASURED_HERE below.  The oracle's rows in fp64: 1e-7 of the row's scale at Newton tol 1e-13, inherited
(test_frame_jacobians_against_the_oracle_rows of the present file now also runs small:11, small:35, small:52, small:99 and large:L1).  fp32 at n = 16 against the
oracle's rows: 10 x the measured error, F32_ORACLE_MEASURED below."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
import param_grad_util as PU      # noqa: E402
import frame_jacobian_cases as FC      # noqa: E402
import test_gpu_frame_jacobians as G      # noqa: E402
from test_gpu_frame_jacobians import _check_columns, _column_errors, _tangent_columns      # noqa: E402,F401
from test_frame_jacobian_yardstick import oracle_frame_rows      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = PU.DEV
F64, F32 = torch.float64, torch.float32
B, T, S = FC.B_ENVS, FC.T_FRAMES, FC.SUBSTEPS
ESZ = {F64: 8, F32: 4}
TAG = {F64: "fp64", F32: "fp32"}
# the largest (column, Jvar) errors against k_tangent over this file's cases, by type: (value, case)
MEASURED_HERE = {F64: ((7.573e-14, "small:12"), (3.426e-16, "small:111")), F32: ((5.807e-5, "small:12"), (2.384e-7, "large:L3"))}
# cases over the present file's BOUND: (case, type) -> the case's own measured worst error; its bound is 10 x that, under CAP.  cond(H): the profile
OWN_MEASURED = {}
OWN_BOUND = {k: 10 * v for k, v in OWN_MEASURED.items()}
# fp32 [A | B] of the 16-dof models against the oracle's rows at the fp32 states: measured worst |entry - oracle| / row scale; the bound is 10 x
F32_ORACLE_MEASURED = {"large:L2": 1.974e-5, "large:L3": 9.393e-6}

GRID = [pytest.param(n, dt, l, id="%s-%s-lanes%d" % (n, TAG[dt], l)) for n in FC.NAMES for dt in (F64, F32) if (n, ESZ[dt]) not in FC.REFUSED
        for l in (0,) + FC.FORCED.get((n, ESZ[dt]), ())]


def _t(x, dt):
    return torch.tensor(np.ascontiguousarray(x), device=DEV, dtype=dt)


def _table_shape(sim, name, lanes):
    """the launch is the case file's table entry (the restated plan's: _check_columns asserts that too)"""
    fl = sim.frame_jacobians_launch_info()
    want = FC.SHAPES[name, ESZ[sim.dtype]][lanes]
    assert (fl["lanes_per_env"], fl["lds_bytes"], fl["lds_bytes"] <= 64 * 1024) == want, (name, lanes, fl, want)
    assert fl["blocks"] == -(-sim.B // (64 // want[0]))
    return fl


# ---------------------------------------------------------------------------------------------------- 1. against k_tangent, every column
@pytest.mark.parametrize("name,dtype,lanes", GRID)
def test_columns_against_the_tangent_pass(name, dtype, lanes):
    """every entry of A_f, B_f and Jvar_f of every frame and environment, at the library's shape and at the forced shapes the case is there for.
    The Jvar task loop: small:30 at 16 lanes (36 tasks, three trips), large:L26 at 64 (91, two) and at 32 (three), large:L2 (64 tasks = 64 lanes),
    large:L3 (80 tasks at 64 lanes)"""
    sim, fj = _check_columns(name, dtype, lanes=lanes, case=FC.fj_case(name), bound=OWN_BOUND.get((name, dtype)))
    _table_shape(sim, name, lanes)
    nvar, nr = FC.CASES[name][2], FC.CASES[name][0]
    assert ("Jvar" in fj) == (nvar > 0) and (not nvar or tuple(fj["Jvar"].shape) == (T, B, 3 * nvar, nr))


# ---------------------------------------------------------------------------------------------------- 2. fp32 at n = 16 against the oracle
@pytest.mark.parametrize("name", ["large:L2", "large:L3"])
def test_fp32_sixteen_dofs_against_the_oracle_rows(name):
    """fp64 frame Jacobians of these models are refused (below), so fp32 has none to lean on: [A_f | B_f] of the fp32 batch against the oracle's
    adjoint rows of the frame started at the fp32 batch's own (q_f, qd_f), on the fp32 rows and controls, per entry relative to the row's
    largest magnitude.  The batch runs at the models' own Newton tol (1e-9), as every fp32 case of the column tests does: single precision does
    not reach it, so the iteration runs until it stalls and some environments report it (status; printed).  (With the batch at tol 1e-5 the same
    comparison measured 3.1e-3 on large:L2 and 2.6e-2 on large:L3 — presumably the taped Newton matrix, the last iterate's, is then a Newton
    step behind the taped point; not looked into further: profiles/r23_frame_jacobian_edges.md.)  The oracle runs at 1e-13.  The bound is 10 x the measured worst (F32_ORACLE_MEASURED), the project's
    margin for the run-to-run differences of an fp32 trajectory; the measured value is under the project's fp32 figure of 1e-4 of the row's scale"""
    m, q0, qd0, u, S_ = FC.fj_case(name)
    sim = PU.make_sim(m, B, F32, T * S)
    tab = PU.table_rows(m, B, True, FC.ROWS_SEED)
    out = G._roll(sim, tab, q0, qd0, u, S)
    print("fp32 oracle rows %s: status %s" % (name, out["status"].tolist()))
    _table_shape(sim, name, 0)
    fj = sim.frame_jacobians(T, S)
    AB = torch.cat([fj["A"], fj["B"]], 3).double().cpu().numpy()
    q = np.concatenate([np.float32(q0)[None].astype(np.float64), out["q"].double().cpu().numpy()], 0)          # [T + 1, B, nr]: the frames' starts
    qd = np.concatenate([np.float32(qd0)[None].astype(np.float64), out["qd"].double().cpu().numpy()], 0)
    u32 = np.float32(u).astype(np.float64)
    worst = 0.0
    for e in range(B):
        me = PU.row_model(m, tab[e].astype(np.float64))
        me.F[Bl.TSIM_FH_TOL] = 1e-13
        for f in range(T):
            rows = oracle_frame_rows(me, q[f, e], qd[f, e], u32[e, f], S)
            worst = max(worst, float((np.abs(AB[f, e] - rows) / np.abs(rows).max(1, keepdims=True)).max()))
    print("fp32 oracle rows %s: worst |entry - oracle| / row scale = %.3e" % (name, worst))
    if G.STATS:
        with open(G.STATS, "a") as fh:
            fh.write("fp32_oracle_rows %s %.4e\n" % (name, worst))
    assert F32_ORACLE_MEASURED[name] is not None and F32_ORACLE_MEASURED[name] <= 1e-4
    assert worst <= 10 * F32_ORACLE_MEASURED[name], (name, worst)


# ---------------------------------------------------------------------------------------------------- 3. the refusal
@pytest.mark.parametrize("name", ["large:L2", "large:L3"])
def test_a_block_over_the_lds_is_refused_and_changes_nothing(name):
    """fp64, 16 dofs: one context and the environment's column block exceed 64 KB at one environment per wavefront (the case file's bytes), so
    tsim_frame_jacobians refuses, launches nothing and writes nothing; the batch then runs its adjoint to the bits of a batch that never asked"""
    from tactilesimulation_amd.host import capi
    m, q0, qd0, u, S_ = FC.fj_case(name)
    nr, nu, nvar = m.ndof_r, m.ndof_u, FC.nvariables(m)
    rng = np.random.default_rng(17)
    w = [_t(rng.normal(size=(T, B, d)), F64) if d else None for d in (nr, m.ndof_var, m.ndof_tactile)]
    res = []
    for ask in (False, True):
        sim = PU.make_sim(m, B, F64, T * S)
        out = G._roll(sim, PU.table_rows(m, B, False, FC.ROWS_SEED), q0, qd0, u, S)
        if ask:
            fl = _table_shape(sim, name, 0)
            assert fl["lds_bytes"] > 64 * 1024 and fl["lanes_per_env"] == 64 and sim.launch_info()["lds_bytes"] <= 64 * 1024
            L = capi.lib()
            bufs = [torch.full((T, B, r, c), 7.0, device=DEV, dtype=F64) for r, c in ((2 * nr, 2 * nr), (2 * nr, nu), (3 * nvar, nr))]
            sim.kernel_timing(True)
            sim.kernel_times()
            assert L.tsim_frame_jacobians(sim._h, T, S, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), None) != 0
            msg = L.tsim_last_error()
            assert b"do not fit the block's LDS" in msg and (b"the %d columns" % (2 * nr + nu)) in msg, msg
            with pytest.raises(RuntimeError, match="do not fit the block's LDS"):
                sim.frame_jacobians(T, S, want_var=True)
            assert L.tsim_frame_jacobians(sim._h, 1, S, None, None, bufs[2].data_ptr(), None) != 0      # (Jvar alone: the plan is the same)
            torch.cuda.synchronize()
            assert all(n == 0 for _, n in sim.kernel_times().values())
            sim.kernel_timing(False)
            assert all(bool((x == 7).all()) for x in bufs)
            print("refusal %s: %d bytes at %d lanes; %s" % (name, fl["lds_bytes"], fl["lanes_per_env"], msg.decode()))
        assert sim.tape_len() == T * S
        du = sim.backward_episode(T, S, w[0], w[1], w[2])
        res.append([out[k] for k in sorted(out)] + [du] + list(sim.get_adjoint()))
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ---------------------------------------------------------------------------------------------------- 4. Jvar alone
@pytest.mark.parametrize("name,dtype,lanes", [("small:30", F32, 16), ("large:L26", F64, 0), ("large:L26", F32, 32), ("large:L2", F32, 0), ("large:L3", F32, 0),
                                               ("small:11", F64, 16)])
def test_jvar_alone_is_the_full_launch_s(name, dtype, lanes):
    """want_A = want_B = False evaluates the frame's last taped point only; the task loop (one to three trips) writes the full launch's bits"""
    m, q0, qd0, u, S_ = FC.fj_case(name)
    sim = PU.make_sim(m, B, dtype, T * S, lanes=lanes)
    G._roll(sim, PU.table_rows(m, B, dtype == F32, FC.ROWS_SEED), q0, qd0, u, S)
    fl = _table_shape(sim, name, lanes)
    full = sim.frame_jacobians(T, S, want_var=True)
    only = sim.frame_jacobians(T, S, want_A=False, want_B=False, want_var=True)
    assert set(only) == {"Jvar"} and torch.equal(only["Jvar"], full["Jvar"]) and bool((full["Jvar"] != 0).any())
    print("Jvar alone %s %s: %d tasks at %d lanes" % (name, TAG[dtype], FC.CASES[name][2] * m.ndof_r, fl["lanes_per_env"]))


# ---------------------------------------------------------------------------------------------------- 5. sub-step and frame edges
@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("edge", ["S1", "T1", "newest"])
@pytest.mark.parametrize("name", ["small:11", "small:52"])
def test_substep_and_frame_edges(name, edge, dtype):
    """S = 1 (chunk_len 1: a qd-row's history is the frame's start), T = 1 (one frame on the tape), and the newest frame of the three-frame tape,
    each against k_tangent at the present file's bound"""
    m, q0, qd0, u, S_ = FC.fj_case(name)
    t_roll, s, window = {"S1": (T, 1, T), "T1": (1, S, 1), "newest": (T, S, 1)}[edge]
    sim = PU.make_sim(m, B, dtype, t_roll * s)
    G._roll(sim, PU.table_rows(m, B, dtype == F32, FC.ROWS_SEED), q0, qd0, u[:, :t_roll], s)
    fj = sim.frame_jacobians(window, s, want_var=True)
    assert sim.tape_len() == t_roll * s and tuple(fj["A"].shape) == (window, B, 2 * m.ndof_r, 2 * m.ndof_r)
    ecol, evar = _column_errors(sim, window, s, fj)
    print("edge %s %s %s: column error %.3e Jvar error %.3e" % (name, edge, TAG[dtype], ecol, evar))
    if G.STATS:
        with open(G.STATS, "a") as fh:
            fh.write("edge %s %s %s %.4e %.4e\n" % (name, edge, TAG[dtype], ecol, evar))
    assert ecol <= G.BOUND[dtype] and evar <= G.BOUND[dtype], (name, edge, ecol, evar)
    if edge == "newest":      # the window is the last frame of the full launch, bit for bit
        full = sim.frame_jacobians(T, S, want_var=True)
        assert all(torch.equal(fj[k][0], full[k][T - 1]) for k in fj)
