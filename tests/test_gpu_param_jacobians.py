"""The per-frame parameter Jacobians of a taped episode (include/tsim.h tsim_param_jacobians, BatchSim.param_jacobians, functions.episode_parameters).

k_param_jacobian is k_tangent's BDF1 recursion for unit dtables columns, one frame per slot and every column starting at zero, eight columns per
elimination of the taped Newton matrix; its Ft is the parameter term of k_tangent's tactile expression.  So it is held to k_tangent column by
column (test_every_column_against_the_tangent_pass): the error of an entry of E is |difference| / (largest magnitude of the reference column over
the same half, q rows or qd rows — columns carry different units, a row-wise scale would let a kn column hide under a mu column), a reference
column that is identically zero must be exactly zero, and dtactile must equal C_f E_f[:, col] + F_f[:, col] (C_f: tsim_tactile_jacobians) on the
scale sum |terms|.  Bounds: 10 x the largest value measured over every case of that test on the MI355X (MEASURED below,
profiles/r26_param_jacobians.md), which stay under the tangent's caps 1e-10 / 1e-4.  E's measured value is 0 in both types: the kernel forms a
column's source with k_tangent's operations in k_tangent's order (M (h dqd0) by mass_times_z per column), and what the two eliminations leave apart
rounds away — so the bound on E is bit-equality with k_tangent; the tactile identity measures 1.1e-14 (fp64) / 3.8e-6 (fp32).
The oracle (fp64, Newton tol 1e-13, four environments on rows of their own): E against tests/param_jacobian_cases.py oracle_frame_param_rows at
the oracle's own states and F against oracle_tactile_param_rows' sensor columns, each entry within 1e-7 of its column-half scale — the one
yardstick that shares nothing with k_tangent (tests/test_param_jacobian_yardstick.py checks it on the CPU).
Then the chain against a whole-episode tangent with a dtables direction, the column passes and the selection (bits), the launch shapes
(param_jacobian_cases.param_jacobian_shape: lanes, LDS bytes, blocks, exactly) with the census of the 14 instantiations, exact structure,
read-only and capture, the refusals, and the ragged batch."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
import pad_models as P      # noqa: E402
import param_grad_util as PU      # noqa: E402
import param_jacobian_cases as PJ      # noqa: E402
import tactile_jacobian_cases as TC      # noqa: E402
import wide_models as W      # noqa: E402
from frame_jacobian_cases import ORACLE_CASES, as_bdf1      # noqa: E402
from test_tangent_yardstick import TANGENT_CASES, T_FRAMES, tangent_case      # noqa: E402
from test_frame_jacobian_yardstick import oracle_frame_states      # noqa: E402
import test_gpu_frame_jacobians as GF      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = PU.DEV
F64, F32 = torch.float64, torch.float32
CASES = [c for c in TANGENT_CASES if not c.startswith("bdf2:")]      # (the BDF2 draws small:3 and large:L7 run as BDF1 models, as the frame Jacobians' do)
# the largest errors measured over every case of test_every_column_against_the_tangent_pass on the MI355X (profiles/r26_param_jacobians.md); the
# bounds are 10 x
MEASURED = {F64: 0.0, F32: 0.0}                   # E's columns against k_tangent's: bit for bit in every case of the file
MEASURED_TAC = {F64: 1.091e-14, F32: 3.756e-6}    # dtactile against C E + F: both on dclaw_position_control
CAP = {F64: 1e-10, F32: 1e-4}
BOUND = {dt: 10 * MEASURED[dt] for dt in MEASURED}
BOUND_TAC = {dt: 10 * MEASURED_TAC[dt] for dt in MEASURED_TAC}
STATS = os.environ.get("TSIM_PARAM_JACOBIAN_STATS")      # a file: every case's largest errors are appended to it (the profile)
MAXC = PJ.MAX_COLS


@pytest.fixture(scope="module")
def pad_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("pj_pads")


def _case(name, B):
    return as_bdf1(*tangent_case(name, B))


def _t(x, dt):
    return torch.tensor(np.ascontiguousarray(x), device=DEV, dtype=dt)


def _roll(sim, tab, q0, qd0, u, S):
    dt = sim.dtype
    if tab is not None:
        sim.set_env_tables(_t(tab, dt))
    sim.reset(_t(q0, dt), _t(qd0, dt), backward_flag=True)
    return sim.rollout(_t(u.transpose(1, 0, 2), dt), S, want_qd=True)


def _stat(line):
    print(line)
    if STATS:
        with open(STATS, "a") as fh:
            fh.write(line + "\n")


def _cols(m):
    return [c for _, c in PJ.columns(m)]


def _E(sim, T, S, cols):
    """E [T, B, 2 nr, len(cols)] in launches of at most 32 columns"""
    return torch.cat([sim.param_jacobians(T, S, cols[c0:c0 + MAXC])["E"] for c0 in range(0, len(cols), MAXC)], 3)


def _dense_F(m, Ft, cols):
    """[n, B, ntac, len(cols)] from the compact Ft [n, B, 4, ntac]: the test's own scatter (functions.episode_parameters has the library's)"""
    F = torch.zeros((Ft.shape[0], Ft.shape[1], Ft.shape[3], len(cols)), device=Ft.device, dtype=Ft.dtype)
    where = PJ.sensor_column_taxels(m)
    for k, c in enumerate(cols):
        if c in where:
            f, t0, nt = where[c]
            F[:, :, 3 * t0:3 * (t0 + nt), k] = Ft[:, :, f, 3 * t0:3 * (t0 + nt)]
    return F


def _tangent_ndir(sim):
    """directions per tangent_episode launch with dtables: eight, or the most whose tangent state fits the block's LDS for this model"""
    return next(nd for nd in (8, 4, 2, 1) if nd == 1 or sim.tangent_launch_info(nd, True)["lds_bytes"] <= 64 * 1024)


def _tangent_param_columns(sim, T, S, f, cols, tac):
    """(M [B, 2 nr, ncols], dtac [B, ntac, ncols] or None) of frame f by k_tangent: the first output frame of a window over the newest T - f
    frames, dtables = unit columns, zero dq0, dqd0 and du"""
    B, nr, dt = sim.B, sim.ndof_r, sim.dtype
    n, ndir = T - f, _tangent_ndir(sim)
    ntab = sim.base_tables().shape[1]
    M = torch.zeros((B, 2 * nr, len(cols)), device=DEV, dtype=dt)
    D = torch.zeros((B, sim.ndof_tactile, len(cols)), device=DEV, dtype=dt) if tac else None
    mask = torch.zeros(n, dtype=torch.bool)
    mask[0] = True
    for c0 in range(0, len(cols), ndir):
        idx = list(range(c0, min(c0 + ndir, len(cols))))
        dtab = torch.zeros((len(idx), B, ntab), device=DEV, dtype=dt)
        for k, i in enumerate(idx):
            dtab[k, :, cols[i]] = 1
        o = sim.tangent_episode(n, S, dtables=dtab, want_qd=True, want_var=False, want_tactile=tac, tactile_mask=mask if tac else None)
        M[:, :nr, idx] = o["dq"][:, 0].permute(1, 2, 0)
        M[:, nr:, idx] = o["dqd"][:, 0].permute(1, 2, 0)
        if tac:
            D[:, :, idx] = o["dtactile"][:, 0].permute(1, 2, 0)
    return M, D


def _column_error(E, M, nr):
    """largest |E - M| / (largest |M| of the column over the same half) over [B, 2 nr, ncols]; a reference column-half that is identically zero
    must be exactly zero in E"""
    worst = 0.0
    for half in (slice(0, nr), slice(nr, 2 * nr)):
        ref, got = M[:, half].double(), E[:, half].double()
        sc = ref.abs().amax(1, keepdim=True).expand_as(ref)
        assert bool((got[sc == 0] == 0).all()), "a column that is identically zero in the reference is not exactly zero"
        if bool((sc > 0).any()):
            worst = max(worst, float(((got - ref).abs() / sc.clamp_min(1e-300))[sc > 0].max()))
    return worst


def _errors_against_the_tangent(sim, m, T, S, cols, E, Ft):
    """(E's column error, the tactile identity's error, the identity's error with k_tangent's own dq, dqd in place of E — what C and F alone leave)
    over the frames"""
    nr = sim.ndof_r
    tac = Ft is not None
    Ct = sim.tactile_jacobians(T, S).double() if tac else None               # [T, B, 2 nr, ntac]
    F = _dense_F(m, Ft, cols).double() if tac else None
    ecol, etac, eown = 0.0, 0.0, 0.0
    for f in range(T):
        M, D = _tangent_param_columns(sim, T, S, f, cols, tac)
        ecol = max(ecol, _column_error(E[f], M, nr))
        if tac:
            Ef = E[f].double()
            got = torch.einsum("bkt,bkc->btc", Ct[f], Ef) + F[f]
            sc = torch.einsum("bkt,bkc->btc", Ct[f].abs(), Ef.abs()) + F[f].abs()
            diff = (got - D.double()).abs()
            assert bool((diff[sc == 0] == 0).all())
            if bool((sc > 0).any()):
                etac = max(etac, float((diff / sc.clamp_min(1e-300))[sc > 0].max()))
            Mf = M.double()
            sc = torch.einsum("bkt,bkc->btc", Ct[f].abs(), Mf.abs()) + F[f].abs()
            diff = (torch.einsum("bkt,bkc->btc", Ct[f], Mf) + F[f] - D.double()).abs()
            if bool((sc > 0).any()):
                eown = max(eown, float((diff / sc.clamp_min(1e-300))[sc > 0].max()))
    return ecol, etac, eown


def _assert_shape(sim, m, lanes, rows):
    """k_param_jacobian's launch is the restated plan's: lanes per environment, LDS bytes, blocks per frame, exactly"""
    env = int(os.environ.get("TSIM_LPE", "0"))
    forced = lanes or (env if env in (16, 32, 64) else 0)
    n_simd = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    want = PJ.param_jacobian_shape(m, forced, 8 if sim.dtype == F64 else 4, rows, sim.B, n_simd, sim.kernel_variant() != "generic")
    fl = sim.param_jacobians_launch_info()
    assert (fl["lanes_per_env"], fl["lds_bytes"], fl["lds_bytes"] <= 64 * 1024) == want and fl["threads"] == 64, (forced, fl, want)
    assert fl["blocks"] == -(-sim.B // (64 // fl["lanes_per_env"]))
    return fl


def _check(name, case, dtype, lanes=0, static=False, rows=True, expect_variant=None, B=5):
    """one case against k_tangent, every column of param_columns(): shape, finiteness, the bounds; returns (sim, model, cols, E, Ft)"""
    m, q0, qd0, u, S = case
    T = u.shape[1]
    sim = PU.make_sim(m, B, dtype, T * S, lanes=lanes, static=static)
    tab = PU.table_rows(m, B, dtype == F32, 11) if rows else None
    _roll(sim, tab, q0, qd0, u, S)
    if expect_variant:
        assert sim.kernel_variant() == expect_variant
    fl = _assert_shape(sim, m, lanes, rows)
    assert fl["lanes_per_env"] >= sim.launch_info()["lanes_per_env"] and fl["lds_bytes"] <= 64 * 1024, fl
    cols = _cols(m)
    tac = sim.ndof_tactile > 0
    torch.full((T, B, 2 * sim.ndof_r, min(len(cols), MAXC)), float("nan"), device=DEV, dtype=dtype)      # (the allocator's next block of this shape is NaN)
    E = _E(sim, T, S, cols)
    Ft = sim.param_jacobians(T, S, (), want_E=False, want_tactile=True)["Ft"] if tac else None
    assert sim.tape_len() == T * S and tuple(E.shape) == (T, B, 2 * sim.ndof_r, len(cols))
    assert bool(torch.isfinite(E).all()) and (Ft is None or bool(torch.isfinite(Ft).all())), (name, "an entry was not written")
    ecol, etac, eown = _errors_against_the_tangent(sim, m, T, S, cols, E, Ft)
    _stat("tangent %-24s %s lanes %2d (kernel at %2d) static %d rows %d ncols %2d: column error %.3e tactile error %.3e (with k_tangent's dq, dqd: %.3e) nonzero E %d Ft %d" % (
        name, "f64" if dtype == F64 else "f32", lanes, fl["lanes_per_env"], static, rows, len(cols), ecol, etac, eown, int((E != 0).sum()),
        0 if Ft is None else int((Ft != 0).sum())))
    assert ecol <= BOUND[dtype] and etac <= BOUND_TAC[dtype], (name, ecol, etac)
    return sim, m, cols, E, Ft


# ---------------------------------------------------------------------------------------------------- the census
# instantiation (real, NRM, EXPJ, lanes) of k_param_jacobian -> (case, forced lanes, per-environment rows, the test of this file that runs it); the
# shapes are the restated plan's (tests/test_param_jacobian_kernel_table.py checks all of it against the kernel table)
_SH = "test_columns_at_every_launch_shape"
_RV = "test_columns_with_a_rotation_vector_joint"
REACHED_BY = {
    ("f", 8, False, 16): ("pusher", 16, True, _SH), ("f", 8, False, 32): ("pusher", 32, True, _SH), ("f", 8, False, 64): ("pusher", 64, True, _SH),
    ("d", 8, False, 16): ("box_slide", 16, True, _SH), ("d", 8, False, 32): ("pusher", 32, True, _SH), ("d", 8, False, 64): ("pusher", 64, True, _SH),
    ("f", 16, False, 16): ("wide9", 16, True, _SH), ("f", 16, False, 32): ("wide9", 32, True, _SH), ("f", 16, False, 64): ("wide9", 64, True, _SH),
    ("d", 16, False, 32): ("wide9", 32, True, _SH), ("d", 16, False, 64): ("wide9", 64, True, _SH),
    ("f", 16, True, 64): ("tactile_pad", 0, True, _RV), ("d", 16, True, 64): ("tactile_pad", 0, True, _RV),
}
UNREACHABLE = {("d", 16, False, 16)}      # four fp64 contexts of a model of more than 8 dofs are over 64 KB (tests/test_wide_models.py, the same row of every kernel)


def census_model(case):
    return W.wide_model(case) if case in W.WIDE else PU.case("tactile_pad", 1, 1)[0] if case == "tactile_pad" else tangent_case(case, 1)[0]


# ---------------------------------------------------------------------------------------------------- 1. every column against k_tangent
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", CASES)
def test_every_column_against_the_tangent_pass(name, dtype):
    """B = 5 (ragged at 4 and 2 per wavefront), T = 3 frames, per-environment rows, the library's launch shape, all of param_columns() in launches
    of at most 32 (tactile_insertion: 64 columns, two launches; dclaw: 34)"""
    sim, m, cols, E, Ft = _check(name, _case(name, 5), dtype)
    assert bool((E != 0).any())


@pytest.mark.parametrize("dtype", [F64, F32])
def test_the_measured_values_lie_under_the_tangents_caps(dtype):
    """MEASURED and MEASURED_TAC under 1e-10 (fp64) / 1e-4 (fp32).  (With the mass matrix formed once from unit vectors, as k_frame_jacobian forms
    it, E differed from k_tangent's columns by 5.2e-6 of their scale in fp32, and the tactile identity on pusher — whose scale is per entry —
    measured 1.147e-4, over the cap, while 4.1e-7 with k_tangent's own dq, dqd: profiles/r26_param_jacobians.md §1.1.  The kernel now takes
    k_tangent's product per column.)"""
    assert MEASURED[dtype] < CAP[dtype] and MEASURED_TAC[dtype] < CAP[dtype], (MEASURED[dtype], MEASURED_TAC[dtype], CAP[dtype])


# ---------------------------------------------------------------------------------------------------- 2. against the oracle
@pytest.mark.parametrize("name", ["pusher", "box_slide", "dclaw_position_control"] + ORACLE_CASES)
def test_against_the_oracle_rows(name):
    """fp64, four environments with rows of their own, Newton tol 1e-13.  E: every column of param_columns() against the oracle's parameter
    adjoint rows of the frame started at the oracle's own (q_f, qd_f), each entry within 1e-7 of its column-half scale (the largest magnitude of
    the oracle's column over the q rows or the qd rows; a column-half the oracle leaves at zero is exactly zero here).  F (models with taxels,
    the last frame): the sensor columns of the oracle's dtactile / dp rows — where E is zero, so the row is the direct term alone — each entry
    within 1e-7 of the column's largest magnitude (the corpus models' sensors are unloaded in that frame: exact zeros on both sides)"""
    B, T = 4, T_FRAMES
    m, q0, qd0, u, S = _case(name, B)
    m = copy.deepcopy(m)
    m.F[Bl.TSIM_FH_TOL] = 1e-13
    tab = PU.table_rows(m, B, False, 12)
    sim = PU.make_sim(m, B, F64, T * S)
    _roll(sim, tab, q0, qd0, u, S)
    cols = _cols(m)
    nr = sim.ndof_r
    E = _E(sim, T, S, cols).cpu().numpy()
    tac = sim.ndof_tactile > 0
    F = None
    if tac:
        mask = torch.zeros(T, dtype=torch.bool)
        mask[T - 1] = True
        F = _dense_F(m, sim.param_jacobians(T, S, (), want_E=False, want_tactile=True, tactile_mask=mask)["Ft"], cols)[0].cpu().numpy()
    sens = [k for k, c in enumerate(cols) if c in PJ.sensor_column_taxels(m)]
    worst, worst_f, nonzero, loaded = 0.0, 0.0, 0, False
    for e in range(B):
        me = PU.row_model(m, tab[e])
        st = oracle_frame_states(me, q0[e], qd0[e], u[e], S)
        for f in range(T):
            rows = PJ.oracle_frame_param_rows(me, st[f][0], st[f][1], u[e, f], S)[:, cols]
            for half in (slice(0, nr), slice(nr, 2 * nr)):
                scale = np.abs(rows[half]).max(0, keepdims=True)
                diff = np.abs(E[f, e][half] - rows[half])
                assert np.all(diff <= 1e-7 * scale), (name, e, f, float((diff / np.maximum(scale, 1e-300)).max()))
                worst = max(worst, float((diff / np.maximum(scale, 1e-300)).max()))
                nonzero += int((scale > 0).sum())
        if tac:
            rows, ld = PJ.oracle_tactile_param_rows(me, st[T - 1][0], st[T - 1][1], u[e, T - 1], S)
            rows = rows[:, cols][:, sens]
            scale = np.abs(rows).max(0, keepdims=True)
            diff = np.abs(F[e][:, sens] - rows)
            assert np.all(diff <= 1e-7 * scale), (name, e, "F", float((diff / np.maximum(scale, 1e-300)).max()))
            worst_f = max(worst_f, float((diff / np.maximum(scale, 1e-300)).max()))
            loaded |= bool(ld.any() and (scale > 0).any())
    _stat("oracle_rows %s: worst |E - oracle| / column-half scale = %.3e (%d non-zero column halves), F %.3e" % (name, worst, nonzero, worst_f))
    assert nonzero > 0 and (loaded or name not in ("pusher", "dclaw_position_control"))


# ---------------------------------------------------------------------------------------------------- 3. the chain
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["pusher", "dclaw_position_control", "box_slide"])
def test_chain_reproduces_the_episode_tangent(name, dtype):
    """x_{f+1} = A_f x_f + E_f dp (in double on the host, x_0 = 0) against a whole-episode tangent_episode with a random dtables direction dp.
    The scale, propagated as tests/test_gpu_frame_jacobians.py propagates it: every entry of A_f may differ from k_tangent's by that file's
    BOUND x (the largest magnitude of its row).  E_f's columns are k_tangent's bit for bit (BOUND is 0), but k_tangent walks the COMBINED
    direction: it rounds sum_col G_col dp_col, one source and one solution per sub-step where the chain adds up 19 .. 34 columns in double — the
    same kind of difference (one kernel's roundings against another's sums) that GF.BOUND measures between k_tangent and k_frame_jacobian, so that
    is the level allowed per unit of the E term's scale too:
        sa_0 = se_0 = 0 ,  sa_{f+1} = |A_f| sa_f + rowmax(A_f) ||x_f||_1 ,  se_{f+1} = |A_f| se_f + sum_col colhalfmax(E_f) |dp_col|
        |chain - tangent| <= GF.BOUND (sa_f + se_f)   per entry."""
    from tactilesimulation_amd.functions import episode_parameters, episode_transition
    B, T, nd = 5, T_FRAMES, 2
    m, q0, qd0, u, S = _case(name, B)
    sim = PU.make_sim(m, B, dtype, T * S)
    tab = PU.table_rows(m, B, dtype == F32, 11)
    _roll(sim, tab, q0, qd0, u, S)
    cols = _cols(m)
    nr = sim.ndof_r
    rng = np.random.default_rng(93)
    dp = rng.normal(size=(nd, B, len(cols))) * np.abs(tab[None, :, cols])    # (every column moves by a share of its own value)
    dtab = torch.zeros((nd, B, tab.shape[1]), device=DEV, dtype=dtype)
    dtab[:, :, cols] = _t(dp, dtype)
    o = sim.tangent_episode(T, S, dtables=dtab, want_qd=True, want_var=False, want_tactile=False)
    dpd = dtab[:, :, cols].double()
    A = episode_transition(sim, T, S)[0].double()
    E = episode_parameters(sim, T, S, cols)[0].double()
    x = torch.zeros((nd, B, 2 * nr), device=DEV, dtype=F64)
    ref, sa, se = x, torch.zeros_like(x), torch.zeros_like(x)
    worst = 0.0
    for f in range(T):
        rowmax = A[f].abs().amax(2)                                           # [B, 2 nr]
        colmax = torch.cat([E[f][:, :nr].abs().amax(1, keepdim=True).expand(-1, nr, -1), E[f][:, nr:].abs().amax(1, keepdim=True).expand(-1, nr, -1)], 1)
        sa = torch.einsum("bij,dbj->dbi", A[f].abs(), sa) + rowmax.unsqueeze(0) * ref.abs().sum(2).unsqueeze(2)
        se = torch.einsum("bij,dbj->dbi", A[f].abs(), se) + torch.einsum("bic,dbc->dbi", colmax, dpd.abs())
        x = torch.einsum("bij,dbj->dbi", A[f], x) + torch.einsum("bic,dbc->dbi", E[f], dpd)
        ref = torch.cat([o["dq"][:, f], o["dqd"][:, f]], 2).double()
        bound = GF.BOUND[dtype] * (sa + se)
        assert float(se.max()) > 0
        assert bool(((x - ref).abs() <= bound).all()), (name, f, float(((x - ref).abs() / bound.clamp_min(1e-300)).max()))
        worst = max(worst, float(((x - ref).abs() / bound.clamp_min(1e-300)).max()))
    _stat("chain %-24s %s: worst |chain - tangent| / bound = %.3e" % (name, "f64" if dtype == F64 else "f32", worst))
    assert bool((ref != 0).any())


# ---------------------------------------------------------------------------------------------------- 4. column passes and selection
def _dclaw(dtype, B=5):
    m, q0, qd0, u, S = _case("dclaw_position_control", B)
    q0 = q0 + 1e-4 * np.random.default_rng(5).normal(size=q0.shape)         # (environments that differ)
    tab = PU.table_rows(m, B, dtype == F32, 11)
    sim = PU.make_sim(m, B, dtype, T_FRAMES * S)
    _roll(sim, tab, q0, qd0, u, S)
    return sim, m, tab, q0, qd0, u, S


@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_columns_bits_do_not_depend_on_its_position_or_its_companions(dtype):
    """D'Claw (34 columns; 32 of them: the pair and dof-damping columns first).  ncols = 1, 7, 8, 9, 16, 17, 32 — a pass's tail, a full pass, the
    second to fourth pass — each the leading columns of the full launch, bit for bit; a shuffled list; every column alone"""
    sim, m, tab, q0, qd0, u, S = _dclaw(dtype)
    T = T_FRAMES
    kinds = PJ.columns(m)
    cols = [c for k, c in kinds if not k.startswith("sensor")] + [c for k, c in kinds if k.startswith("sensor")]
    cols = cols[:MAXC]
    full = sim.param_jacobians(T, S, cols)["E"]
    assert tuple(full.shape) == (T, 5, 2 * sim.ndof_r, MAXC) and bool((full != 0).any())
    for n in (1, 7, 8, 9, 16, 17, 32):
        assert torch.equal(sim.param_jacobians(T, S, cols[:n])["E"], full[..., :n]), n
        assert torch.equal(sim.param_jacobians(T, S, cols[MAXC - n:])["E"], full[..., MAXC - n:]), n      # (the same columns in other passes and places)
    perm = np.random.default_rng(3).permutation(MAXC)
    assert torch.equal(sim.param_jacobians(T, S, [cols[i] for i in perm])["E"], full[..., torch.tensor(perm, device=DEV)])
    for k in range(MAXC):
        assert torch.equal(sim.param_jacobians(T, S, [cols[k]])["E"][..., 0], full[..., k]), k
    nz = (full != 0).flatten(0, 2).any(0)
    assert int(nz.sum()) >= 20      # (the columns are not trivially equal: zeros)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_e_does_not_depend_on_the_window_the_tactile_output_or_the_batch(dtype):
    sim, m, tab, q0, qd0, u, S = _dclaw(dtype)
    T = T_FRAMES
    cols = _cols(m)[:MAXC]
    full = sim.param_jacobians(T, S, cols)["E"]
    assert torch.equal(sim.param_jacobians(T - 1, S, cols)["E"], full[1:])   # the newest 2 of 3 frames
    both = sim.param_jacobians(T, S, cols, want_tactile=True, tactile_mask=torch.tensor([False, True, False]))
    assert torch.equal(both["E"], full)
    ft = sim.param_jacobians(T, S, (), want_E=False, want_tactile=True)["Ft"]
    assert torch.equal(both["Ft"], ft[1:2]) and bool((ft != 0).any())
    lanes = sim.param_jacobians_launch_info()["lanes_per_env"]
    one = PU.make_sim(m, 1, dtype, T * S, lanes=sim.launch_info()["lanes_per_env"])
    _roll(one, tab[4:], q0[4:], qd0[4:], u[4:], S)
    assert one.param_jacobians_launch_info()["lanes_per_env"] == lanes
    o1 = one.param_jacobians(T, S, cols, want_tactile=True)
    assert torch.equal(o1["E"][:, 0], full[:, 4]) and torch.equal(o1["Ft"][:, 0], ft[:, 4])
    assert bool((full[:, 4] != full[:, 3]).any())


def test_episode_parameters_scatters_ft_and_joins_the_launches():
    """tactile_insertion: 64 columns, two launches; F is Ft's row on the sensor's own taxels and columns, zero elsewhere"""
    from tactilesimulation_amd.functions import episode_parameters
    B, T = 2, T_FRAMES
    m, q0, qd0, u, S = _case("tactile_insertion", B)
    sim = PU.make_sim(m, B, F32, T * S)
    _roll(sim, None, q0, qd0, u, S)
    cols = _cols(m)
    assert len(cols) == 64
    mask = torch.tensor([False, True, True])
    E, F = episode_parameters(sim, T, S, cols, mask)
    assert torch.equal(E, _E(sim, T, S, cols)) and tuple(F.shape) == (2, B, sim.ndof_tactile, 64)
    Ft = sim.param_jacobians(T, S, (), want_E=False, want_tactile=True, tactile_mask=mask)["Ft"]
    assert torch.equal(F, _dense_F(m, Ft, cols)) and bool((F != 0).any())
    E2, F2 = episode_parameters(sim, T, S, cols[40:43], mask)               # no sensor column: F is zero
    assert torch.equal(E2, E[..., 40:43]) and torch.equal(F2, F[..., 40:43])


# ---------------------------------------------------------------------------------------------------- 5. launch shapes
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("name", ["pusher", "dclaw_position_control", "box_slide", "wide9", "wide10"])
def test_columns_at_every_launch_shape(name, lanes, dtype):
    """forced lanes; wide9 / wide10 (tests/wide_models.py): 9 / 10 dofs on few links — NRM 16 with four (fp32) and two environments per wavefront"""
    _check(name, as_bdf1(*W.wide_case(name, 5, T_FRAMES)) if name in W.WIDE else _case(name, 5), dtype, lanes=lanes)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_columns_with_a_rotation_vector_joint(dtype):
    """the EXPJ instantiations (NRM 16, 64 lanes): the tactile pad pressed on the ball — param_grad_util's case, whose model integrates with
    BDF2, run as a BDF1 model; B = 2, T = 1 (40 000 taxels)"""
    _check("tactile_pad", as_bdf1(*PU.case("tactile_pad", 2, 1)), dtype, B=2)


@pytest.mark.parametrize("dtype,rows,variant", [(F32, False, "static:pusher"), (F32, True, "param:pusher"), (F64, False, "static:pusher")])
def test_on_a_compiled_in_model_batch(dtype, rows, variant):
    """the generic k_param_jacobian over the tape a static:pusher / param:pusher batch recorded (K in its records), held to k_tangent on that tape"""
    if dtype == F64 and os.environ.get("TSIM_LPE") == "16":
        variant = "generic"
    _check("pusher", _case("pusher", 5), dtype, static=True, rows=rows, expect_variant=variant)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [0, 16, 32, 64])
@pytest.mark.parametrize("name", ["pusher", "pad_press", "dclaw_position_control", "tactile_insertion", "wide9", "wide10", "large:L7"])
def test_the_launch_shape_is_the_restated_plan(name, lanes, dtype):
    m = W.wide_model(name) if name in W.WIDE else tangent_case(name, 1)[0]
    for B, rows in ((5, True), (3, False)):
        sim = PU.make_sim(m, B, dtype, 2, lanes=lanes)
        if rows:
            sim.set_env_tables(_t(PU.table_rows(m, B, dtype == F32, 11), dtype))
        _assert_shape(sim, m, lanes, rows)


# ---------------------------------------------------------------------------------------------------- 6. structure
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["pusher", "dclaw_position_control", "tactile_insertion"])
def test_sensor_columns_and_sensing_only_pairs_are_exactly_zero(name, dtype):
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = _case(name, B)
    sim = PU.make_sim(m, B, dtype, T * S)
    _roll(sim, PU.table_rows(m, B, dtype == F32, 11), q0, qd0, u, S)
    zero = list(PJ.sensor_column_taxels(m)) + PJ.sensing_only_pair_columns(m)
    assert len(PJ.sensor_column_taxels(m)) >= 4
    E = _E(sim, T, S, zero)
    assert bool((E == 0).all())
    assert bool((_E(sim, T, S, [c for c in _cols(m) if c not in zero]) != 0).any())


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("dtype", [F64, F32])
def test_free_flight_damping_is_the_damped_double_integrator(dtype, S):
    """tests/models/point_fall.xml: a cube on three translational dofs, no contact pair, gravity and a force motor; per-environment damping d on
    every dof.  A BDF1 sub-step is m (v1 - v0) / h = f - d v1 and q1 = q0 + h v1, so with a = m / (m + h d), per dof and sub-step
        dv1/dd = a dv0/dd - h v1 / (m + h d) ,   dq1/dd = dq0/dd + h dv1/dd ,   both zero at the frame's start;
    a dof's column is zero on the other dofs, exactly.  The bound: S sub-steps of a few roundings each on a sum of S like-signed terms — 16 S eps"""
    from tactilesimulation_amd.model.compiler import load_model
    m = load_model(os.path.join(HERE, "models", "point_fall.xml"))
    B, T, nr, h = 3, 2, 3, m.h
    cols = _cols(m)
    assert [k for k, _ in PJ.columns(m)] == ["dof damping"] * 3
    mass = float(m.F[[c[3] for c in m.body_param_columns() if c[2] == "mass"][0]])
    tab = np.tile(m.F[:PJ.table_size(m)], (B, 1))
    d = np.array([[0.5, 2.0, 0.0], [3.0, 0.25, 1.0], [0.0, 0.0, 7.0]])
    tab[:, cols] = d
    rng = np.random.default_rng(17)
    q0, qd0, u = 0.1 * rng.normal(size=(B, nr)), rng.normal(size=(B, nr)), rng.uniform(-1, 1, size=(B, T, 3))
    sim = PU.make_sim(m, B, dtype, T * S)
    out = _roll(sim, tab, q0, qd0, u, S)
    E = sim.param_jacobians(T, S, cols)["E"].double().cpu().numpy()         # [T, B, 6, 3]
    # the sub-steps' end velocities from the roll-out's own frames: within a frame f, gravity and motor are constant, v_{k+1} = a v_k + c
    qd = np.concatenate([qd0[None], out["qd"].double().cpu().numpy()], 0)    # [T + 1, B, 3]
    a = mass / (mass + h * d)
    eps = 2.3e-16 if dtype == F64 else 1.2e-7
    for f in range(T):
        geo = sum(a ** k for k in range(S))
        c = (qd[f + 1] - a ** S * qd[f]) / geo                               # v_S = a^S v_0 + c (1 + a + ... + a^{S-1})
        v, dv, dq = qd[f].copy(), np.zeros((B, nr)), np.zeros((B, nr))
        sdv, sdq = np.zeros((B, nr)), np.zeros((B, nr))
        for _ in range(S):
            v = a * v + c
            dv = a * dv - h * v / (mass + h * d)
            dq = dq + h * dv
            sdv = a * sdv + np.abs(h * v / (mass + h * d))
            sdq = sdq + h * sdv
        for j in range(nr):
            others = [i for i in range(2 * nr) if i % nr != j]
            assert np.all(E[f][:, others, j] == 0), (f, j)
            assert np.all(np.abs(E[f][:, j, j] - dq[:, j]) <= 16 * S * eps * sdq[:, j] + 1e-300), (f, j, E[f][:, j, j], dq[:, j])
            assert np.all(np.abs(E[f][:, nr + j, j] - dv[:, j]) <= 16 * S * eps * sdv[:, j] + 1e-300), (f, j, E[f][:, nr + j, j], dv[:, j])
        assert np.any(dq != 0)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_pair_columns_are_exactly_zero_in_free_flight(dtype):
    """box_slide lifted a metre off the ground: its pair is never near, its four columns are exactly zero; the dofs' damping columns are not"""
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = _case("box_slide", B)
    anchor = _E_case(m, q0, qd0, u, S, dtype)
    assert bool((anchor[0] != 0).any()), "on the ground the pair columns are not zero: the lifted case compares something"
    kinds = PJ.columns(m)
    lift = None
    for i in range(m.ndof_r):      # the dof that lifts the box: the one whose +1 leaves every pair column exactly zero and moves no other
        q1 = q0.copy()
        q1[:, i] += 1.0
        pair, damp = _E_case(m, q1, qd0, u, S, dtype)
        if bool((pair == 0).all()):
            lift = i
            assert bool((damp != 0).any())
    assert lift is not None and [k for k, _ in kinds].count("pair kn") == 1


def _E_case(m, q0, qd0, u, S, dtype):
    """(E's pair columns, E's dof-damping columns) of a case on per-environment rows"""
    B, T = u.shape[0], u.shape[1]
    sim = PU.make_sim(m, B, dtype, T * S)
    _roll(sim, PU.table_rows(m, B, dtype == F32, 11), q0, qd0, u, S)
    kinds = PJ.columns(m)
    E = _E(sim, T, S, [c for _, c in kinds])
    pair = torch.tensor([k.startswith("pair") for k, _ in kinds], device=DEV)
    damp = torch.tensor([k == "dof damping" for k, _ in kinds], device=DEV)
    return E[..., pair], E[..., damp]


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["small_130_4x2", "adj_129"])
def test_ft_is_exactly_zero_on_unloaded_taxels_and_not_on_loaded_ones(name, dtype, pad_dir):
    """against the oracle's taxel_list at the frame's end (the borderline taxels left out), as the tactile Jacobians' rows are: the kn row of a
    loaded taxel is not zero (dF/dkn = -d n with d < 0)"""
    m, q0, qd0, u, S = TC.pad_case(name, pad_dir, 4)
    sim = PU.make_sim(m, 4, dtype, S)
    _roll(sim, None, q0, qd0, u, S)
    Ft = sim.param_jacobians(1, S, (), want_E=False, want_tactile=True)["Ft"][0].reshape(4, 4, -1, 3)
    any_loaded = False
    for e in range(4):
        q1, qd1 = oracle_frame_states(m, q0[e], qd0[e], u[e], S)[1]
        ld, keep = TC.pad_keep(m, q1, qd1)
        nz = (Ft[e] != 0).any(0).any(-1).cpu().numpy()
        nz_kn = (Ft[e, 0] != 0).any(-1).cpu().numpy()
        assert np.array_equal(nz[keep], ld[keep]) and np.array_equal(nz_kn[keep], ld[keep]), (name, e)
        any_loaded |= bool(ld[keep].any())
    assert any_loaded


@pytest.mark.parametrize("dtype", [F64, F32])
def test_ft_kn_row_is_tactile_over_kn_on_a_frictionless_normal_load(dtype, pad_dir):
    """pad_models' small_130_1x1 (one sensor of 130 taxels over the slab) with the sensor's mu and damping set to zero in every environment's
    row and kn different per environment: the law is then F = -kn d n, linear in kn, so Ft's kn row is the tactile frame / kn.  Both sides
    rotate and project the same vector with a few roundings each: 64 eps of the taxel's largest component"""
    name = "small_130_1x1"
    m, q0, qd0, u, S = TC.pad_case(name, pad_dir, 4)
    where = PJ.sensor_column_taxels(m)
    col = {f: c for c, (f, _, _) in where.items()}
    assert len(where) == 4
    tab = np.tile(m.F[:PJ.table_size(m)], (4, 1))
    tab[:, col[2]] = 0.0
    tab[:, col[3]] = 0.0
    tab[:, col[0]] *= np.array([1.0, 0.5, 2.0, 1.25])
    sim = PU.make_sim(m, 4, dtype, S)
    tab = _t(tab, dtype).cpu().numpy().astype(np.float64)
    out = _roll(sim, tab, q0, qd0, u, S)
    Ft = sim.param_jacobians(1, S, (), want_E=False, want_tactile=True)["Ft"][0].double()      # [4, 4, ntac]
    tac = out["tactile"][0].double()                                         # [4, ntac]
    want = (tac / _t(tab[:, col[0]], F64)[:, None]).reshape(4, -1, 3)
    got = Ft[:, 0].reshape(4, -1, 3)
    eps = 2.3e-16 if dtype == F64 else 1.2e-7
    scale = want.abs().amax(2, keepdim=True)
    assert bool(((got - want).abs() <= 64 * eps * scale).all()), float(((got - want).abs() / scale.clamp_min(1e-300)).max())
    assert bool((want != 0).any())
    assert bool((Ft[3] == 0).all())                                          # (the lifted environment loads nothing)


# ---------------------------------------------------------------------------------------------------- 7. read-only, capturable
@pytest.mark.parametrize("static,rows,variant", [(False, True, "generic"), (True, False, "static:pusher")])
def test_param_jacobian_launches_change_nothing(static, rows, variant):
    """roll-out -> 0 or 2 param_jacobians launches -> the adjoint, bit for bit"""
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = _case("pusher", B)
    cols = _cols(m)
    res = []
    for npj in (0, 2):
        sim = PU.make_sim(m, B, F32, T * S, static=static)
        out = _roll(sim, PU.table_rows(m, B, True, 11) if rows else None, q0, qd0, u, S)
        assert sim.kernel_variant() == variant
        for i in range(npj):
            sim.param_jacobians(T - i, S, cols, want_tactile=True)
        assert sim.tape_len() == T * S and sim.last_adjoint_launch()["kernel"] is None
        st = sim.get_state()
        rng = np.random.default_rng(52)
        w = [_t(rng.normal(size=(T, B, d)), F32) for d in (sim.ndof_r, sim.ndof_var, sim.ndof_tactile)]
        du = sim.backward_episode(T, S, w[0], w[1], w[2])
        lq, lv = sim.get_adjoint()
        res.append([out["q"], out["qd"], out["var"], out["tactile"], out["status"], st[0], st[1], du, lq, lv])
        assert sim.tape_len() == 0 and sim.kernel_variant() == variant
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))


def test_a_captured_launch_replays_to_the_eager_bits():
    """no allocation, no device copy and no host synchronisation in the call (no mask: building a mask's slot map synchronises in Python); the
    columns travel by value in the kernel's arguments"""
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = _case("pusher", B)
    sim = PU.make_sim(m, B, F32, T * S)
    _roll(sim, PU.table_rows(m, B, True, 11), q0, qd0, u, S)
    cols = _cols(m)
    eager = sim.param_jacobians(T, S, cols, want_tactile=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sim.param_jacobians(T, S, cols, want_tactile=True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a = sim.param_jacobians(T, S, cols, want_tactile=True)
    a["E"].fill_(7.0)
    a["Ft"].fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a["E"], eager["E"]) and torch.equal(a["Ft"], eager["Ft"]) and sim.tape_len() == T * S


# ---------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    from tactilesimulation_amd.host import capi
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = _case("pusher", B)
    sim = PU.make_sim(m, B, F64, T * S)
    L = capi.lib()
    cols = _cols(m)
    nc = len(cols)
    E = torch.full((T + 1, B, 2 * sim.ndof_r, 33), 7.0, device=DEV, dtype=F64)
    Ft = torch.full((T + 1, B, 4, sim.ndof_tactile), 7.0, device=DEV, dtype=F64)
    arr = lambda v: (ctypes.c_int32 * max(len(v), 1))(*v)      # noqa: E731

    def call(h, nf, ns, cl=cols, e=E.data_ptr(), ft=Ft.data_ptr(), n=None):
        return L.tsim_param_jacobians(h, nf, ns, len(cl) if n is None else n, arr(cl) if cl is not None else None, None, e, ft, None)
    sim.kernel_timing(True)
    assert call(None, T, S) != 0 and b"null batch" in L.tsim_last_error()
    sim.reset(_t(q0, F64), None, backward_flag=True)
    assert call(sim._h, T, S) != 0 and b"no tape" in L.tsim_last_error()
    _roll(sim, None, q0, qd0, u, S)
    sim.kernel_times()
    assert call(sim._h, T, S, e=None, ft=None) != 0 and b"both null" in L.tsim_last_error()
    assert call(sim._h, T, S, cl=[]) != 0 and b"ncols must be 1 .. 32" in L.tsim_last_error()
    assert call(sim._h, T, S, cl=cols, n=-1) != 0 and b"ncols must be 1 .. 32" in L.tsim_last_error()
    many = (cols * 2)[:33]
    assert call(sim._h, T, S, cl=many) != 0 and b"ncols must be 1 .. 32" in L.tsim_last_error()
    assert call(sim._h, T, S, cl=None, n=nc) != 0 and b"null cols" in L.tsim_last_error()
    body = [c[3] for c in m.body_param_columns()]
    for bad in (body[0], body[-1], 0, Bl.TSIM_FH_TOL, -1, PJ.table_size(m), PJ.table_size(m) + 5, cols[0] - 1):
        if bad in cols:
            continue
        assert call(sim._h, T, S, cl=cols[:3] + [bad]) != 0 and b"is not a contact-group parameter" in L.tsim_last_error(), bad
    assert call(sim._h, T, S, cl=cols[:4] + [cols[2]]) != 0 and b"listed twice" in L.tsim_last_error()
    for nf, ns in ((0, S), (T, 0), (-1, S)):
        assert call(sim._h, nf, ns) != 0 and b"must be positive" in L.tsim_last_error()
    assert call(sim._h, T + 1, S) != 0 and b"sub-steps on the tape" in L.tsim_last_error()
    with pytest.raises(ValueError, match="no masked frame"):
        sim.param_jacobians(T, S, cols, want_tactile=True, tactile_mask=torch.zeros(T, dtype=torch.bool))
    with pytest.raises(RuntimeError):
        sim.param_jacobians(T, S, cols + [cols[0]])
    mb, q0b, qd0b, ub, Sb = _case("box_slide", B)                            # a model without taxels
    simb = PU.make_sim(mb, B, F64, T * Sb)
    _roll(simb, None, q0b, qd0b, ub, Sb)
    assert L.tsim_param_jacobians(simb._h, T, Sb, 1, arr(_cols(mb)[:1]), None, E.data_ptr(), Ft.data_ptr(), None) != 0 and b"without taxels" in L.tsim_last_error()
    assert L.tsim_param_jacobians_launch_info(None, (ctypes.c_int32 * 4)()) != 0
    torch.cuda.synchronize()
    assert all(n == 0 for _, n in sim.kernel_times().values())               # nothing was launched on the batch's timed kinds ...
    assert bool((E == 7).all()) and bool((Ft == 7).all())                    # ... and nothing was written
    # a valid launch after the refusals still gives the right answer
    Eo = _E(sim, T, S, cols)
    Fo = sim.param_jacobians(T, S, (), want_E=False, want_tactile=True)["Ft"]
    ecol, etac, _ = _errors_against_the_tangent(sim, m, T, S, cols, Eo, Fo)
    assert ecol <= BOUND[F64] and etac <= BOUND_TAC[F64]


@pytest.mark.parametrize("dtype", [F64, F32])
def test_bdf2_refuses_e_and_gives_ft(dtype):
    """bdf2:ball_push (BDF2 with a rotation-vector joint): E_out is refused, nothing written; Ft alone succeeds and is k_tangent's dtactile for
    unit sensor columns (whose dq, dqd are exactly zero: sensors do not enter the dynamics), on the scale |F|"""
    from tactilesimulation_amd.host import capi
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("bdf2:ball_push", B)
    sim = PU.make_sim(m, B, dtype, T * S)
    _roll(sim, PU.table_rows(m, B, dtype == F32, 11), q0, qd0, u, S)
    L = capi.lib()
    cols = _cols(m)
    E = torch.full((T, B, 2 * sim.ndof_r, len(cols)), 7.0, device=DEV, dtype=dtype)
    assert L.tsim_param_jacobians(sim._h, T, S, len(cols), (ctypes.c_int32 * len(cols))(*cols), None, E.data_ptr(), None, None) != 0
    assert b"BDF2" in L.tsim_last_error()
    torch.cuda.synchronize()
    assert bool((E == 7).all())
    Ft = sim.param_jacobians(T, S, (), want_E=False, want_tactile=True)["Ft"]      # [T, B, 4, ntac]
    sens = [c for c in cols if c in PJ.sensor_column_taxels(m)]
    F = _dense_F(m, Ft, sens).double()
    ntab = sim.base_tables().shape[1]
    dtab = torch.zeros((len(sens), B, ntab), device=DEV, dtype=dtype)
    for k, c in enumerate(sens):
        dtab[k, :, c] = 1
    assert len(sens) <= 8
    o = sim.tangent_episode(T, S, dtables=dtab, want_qd=True, want_var=False, want_tactile=True)
    worst = 0.0
    for f in range(T):
        dx = torch.cat([o["dq"][:, f], o["dqd"][:, f]], 2).double()          # [ncol, B, 2 nr]: zero — sensors do not enter the dynamics
        assert bool((dx == 0).all())
        ref = o["dtactile"][:, f].double().permute(1, 2, 0)                  # [B, ntac, ncol]
        sc = F[f].abs()
        diff = (F[f] - ref).abs()
        assert bool((diff[sc == 0] == 0).all())
        if bool((sc > 0).any()):
            worst = max(worst, float((diff / sc.clamp_min(1e-300))[sc > 0].max()))
    _stat("bdf2 Ft %s: worst |F - dtactile| / |F| = %.3e" % ("f64" if dtype == F64 else "f32", worst))
    assert bool((F != 0).any()) and worst <= BOUND_TAC[dtype]


def test_the_lds_refusal_on_a_16_dof_model():
    """large:L2 in fp64 (16 dofs: a context of 59 KB and a column block of 9.2 KB at one environment per wavefront): refused, nothing launched,
    nothing written; in fp32 the same model runs"""
    from tactilesimulation_amd.host import capi
    import frame_jacobian_cases as FC
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = FC.fj_case("large:L2")
    L = capi.lib()
    for dtype, fits in ((F64, False), (F32, True)):
        sim = PU.make_sim(m, B, dtype, T * S)
        _roll(sim, PU.table_rows(m, B, dtype == F32, 11), q0, qd0, u, S)
        fl = _assert_shape(sim, m, 0, True)
        assert (fl["lds_bytes"] <= 64 * 1024) == fits
        cols = _cols(m)[:MAXC]
        E = torch.full((T, B, 2 * sim.ndof_r, len(cols)), 7.0, device=DEV, dtype=dtype)
        rc = L.tsim_param_jacobians(sim._h, T, S, len(cols), (ctypes.c_int32 * len(cols))(*cols), None, E.data_ptr(), None, None)
        torch.cuda.synchronize()
        if fits:
            assert rc == 0 and bool((E != 7).all())
        else:
            assert rc != 0 and b"do not fit the block's LDS" in L.tsim_last_error() and bool((E == 7).all())
            with pytest.raises(RuntimeError, match="do not fit"):
                sim.param_jacobians(T, S, cols)


# ---------------------------------------------------------------------------------------------------- 9. ragged batch
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("B", [5, 3, 1])
def test_the_last_environment_of_a_ragged_batch(B, dtype):
    """pusher at 16 lanes (fp32: four environments per wavefront; fp64: two): the last block's idle slots repeat the last environment and store
    nothing — the buffers' guard rows behind the last environment keep their fill, and environment e is the same whatever the batch's size"""
    T = T_FRAMES
    m, q0, qd0, u, S = _case("pusher", 5)
    q0 = q0 + 1e-4 * np.random.default_rng(5).normal(size=q0.shape)
    tab = PU.table_rows(m, 5, dtype == F32, 11)
    cols = _cols(m)
    sim5 = PU.make_sim(m, 5, dtype, T * S, lanes=16)
    _roll(sim5, tab, q0, qd0, u, S)
    ref = sim5.param_jacobians(T, S, cols, want_tactile=True)
    sim = PU.make_sim(m, B, dtype, T * S, lanes=16)
    _roll(sim, tab[:B], q0[:B], qd0[:B], u[:B], S)
    got = sim.param_jacobians(T, S, cols, want_tactile=True)
    assert torch.equal(got["E"], ref["E"][:, :B]) and torch.equal(got["Ft"], ref["Ft"][:, :B])
    assert bool(torch.isfinite(got["E"]).all()) and bool((got["E"][:, B - 1] != 0).any()) and bool((got["Ft"][:, B - 1] != 0).any())
