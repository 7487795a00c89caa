"""The per-frame transition Jacobians of a taped episode (include/tsim.h tsim_frame_jacobians, BatchSim.frame_jacobians, functions.episode_transition).

k_frame_jacobian is k_tangent's BDF1 recursion seeded with the identity, one frame per slot, eight columns per elimination of the taped Newton
matrix.  So it is held, column by column, to k_tangent itself: for every frame f a tangent_episode over the newest T - f frames with identity dq0 /
dqd0 and a unit du on its first frame, in chunks of eight, whose FIRST output frame is the columns of [A_f | B_f].  The error of an entry is
    |difference| / (largest magnitude in the same row of [A_f | B_f])
and its bound is 10 x the largest value measured over every case of the column test (profiles/r22_frame_jacobians.md): fp64 3.9e-14, fp32
1.9e-5 (MEASURED below) — they must stay under the tangent's caps, 1e-10 and 1e-4 (both kernels use the same taped H and the same evaluation of the taped
point; the elimination's multipliers are the same in fp64, where both pivot, and differ in fp32, where k_tangent tries the pivot-free form first).
Jvar is held to tangent_episode's dvar = Jvar dq, entry by entry against sum_k |Jvar_ik dq_k|; the chain x_{f+1} = A_f x_f + B_f du_f to the tangent
of the whole episode against the scale the column test itself leaves open, propagated over the frames (test_chain_...).  The oracle: rows of tests/test_frame_jacobian_yardstick.py's
builder, 1e-7 of the row's scale at Newton tol 1e-13 (the setting of tests/test_gpu_tangent.py's oracle test).
The rest: the launch shapes, compiled-in model batches, exact zeros and the free-flight structure, that the launch changes nothing that exists, that
the outputs are independent of each other and of the window, the refusals, the ragged batch, a captured launch.
The refusal for a block that does not fit the LDS is not run here: none of this file's models reaches it.  The 16-dof models of the random corpus do
in fp64 (large:L2: a context of 59 KB and a column block of 12.6 KB at one environment per wavefront) — tests/test_gpu_frame_jacobian_edges.py runs it.
The launch shape is held to tests/wide_models.py frame_jacobian_shape, the restated plan: lanes, LDS bytes and blocks, exactly.
Cases: TANGENT_CASES without the two bdf2: ones (small:3 and large:L7 as BDF1 models: _case), B = 5 (ragged at 4 and 2 environments per wavefront), T = 3 frames of 2 sub-steps (pusher: 5)."""
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
import wide_models as W      # noqa: E402
from frame_jacobian_cases import ORACLE_CASES, as_bdf1 as _as_bdf1      # noqa: E402
from test_tangent_yardstick import TANGENT_CASES, T_FRAMES, tangent_case      # noqa: E402
from test_frame_jacobian_yardstick import oracle_frame_rows, oracle_frame_states      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = PU.DEV
F64, F32 = torch.float64, torch.float32
CASES = [c for c in TANGENT_CASES if not c.startswith("bdf2:")]
# the largest column errors measured over every case of this file (profiles/r22_frame_jacobians.md); the bound is 10 x
MEASURED = {F64: 3.901e-14, F32: 1.866e-5}      # both on large:L7 (14 dofs)
CAP = {F64: 1e-10, F32: 1e-4}
BOUND = {dt: 10 * MEASURED[dt] for dt in MEASURED}
STATS = os.environ.get("TSIM_FRAME_JACOBIAN_STATS")      # a file: every case's largest errors are appended to it (the profile)


def _case(name, B):
    """tangent_case, as a BDF1 model.  small:3 (1 dof) and large:L7 (14 dofs, NRM 16) of the random corpus are drawn with integrator BDF2, which
    tsim_frame_jacobians refuses (a BDF2 transition acts on two states of history); they are in the case list for their sizes, so they run here
    with the integrator of the same model set to BDF1 — everything else of the model, the start state and the controls are the case's"""
    return _as_bdf1(*tangent_case(name, B))


def _t(x, dt):
    return torch.tensor(np.ascontiguousarray(x), device=DEV, dtype=dt)


def _roll(sim, tab, q0, qd0, u, S):
    dt = sim.dtype
    if tab is not None:
        sim.set_env_tables(_t(tab, dt))
    sim.reset(_t(q0, dt), _t(qd0, dt), backward_flag=True)
    return sim.rollout(_t(u.transpose(1, 0, 2), dt), S, want_qd=True)


def _tangent_columns(sim, T, S, f, ndir=8):
    """([B, 2 nr, 2 nr + nu], dq [ncol, B, nr], dvar [ncol, B, nvar] or None) of frame f by k_tangent: the first output frame of a window over the
    newest T - f frames, identity dq0 / dqd0 and a unit du on the window's first frame, ndir (eight) directions per launch"""
    B, nr, nu, dt = sim.B, sim.ndof_r, sim.ndof_u, sim.dtype
    ncol, n = 2 * nr + nu, T - f
    M = torch.zeros((B, 2 * nr, ncol), device=DEV, dtype=dt)
    dqs, dvs = [], []
    for c0 in range(0, ncol, ndir):
        cols = list(range(c0, min(c0 + ndir, ncol)))
        dq0 = torch.zeros((len(cols), B, nr), device=DEV, dtype=dt)
        dqd0 = torch.zeros_like(dq0)
        du = torch.zeros((len(cols), n, B, nu), device=DEV, dtype=dt)
        for k, d in enumerate(cols):
            if d < nr:
                dq0[k, :, d] = 1
            elif d < 2 * nr:
                dqd0[k, :, d - nr] = 1
            else:
                du[k, 0, :, d - 2 * nr] = 1
        o = sim.tangent_episode(n, S, du=du, dq0=dq0, dqd0=dqd0, want_qd=True, want_var=True, want_tactile=False)
        M[:, :nr, cols] = o["dq"][:, 0].permute(1, 2, 0)
        M[:, nr:, cols] = o["dqd"][:, 0].permute(1, 2, 0)
        dqs.append(o["dq"][:, 0])
        if "dvar" in o:
            dvs.append(o["dvar"][:, 0])
    return M, torch.cat(dqs, 0), torch.cat(dvs, 0) if dvs else None


def _tangent_ndir(sim):
    """directions per tangent_episode launch: eight, or the most (4, 2, 1) whose tangent state fits the block's LDS for this model"""
    return next(nd for nd in (8, 4, 2, 1) if nd == 1 or sim.tangent_launch_info(nd, False)["lds_bytes"] <= 64 * 1024)


def _column_errors(sim, T, S, fj, ndir=8):
    """(largest column error, largest Jvar error) over the frames, against k_tangent"""
    ecol, evar = 0.0, 0.0
    for f in range(T):
        M, dq, dvar = _tangent_columns(sim, T, S, f, ndir)
        AB = torch.cat([fj["A"][f], fj["B"][f]], 2).double()
        scale = AB.abs().amax(2, keepdim=True)
        assert float(scale.min()) > 0
        ecol = max(ecol, float(((AB - M.double()).abs() / scale).max()))
        if dvar is not None:
            J = fj["Jvar"][f].double()                                        # [B, nvar, nr]
            got = torch.einsum("bik,dbk->dbi", J, dq.double())
            sc = torch.einsum("bik,dbk->dbi", J.abs(), dq.double().abs())
            diff = (got - dvar.double()).abs()
            assert bool((diff[sc == 0] == 0).all())
            evar = max(evar, float((diff / sc.clamp_min(1e-300))[sc > 0].max()) if bool((sc > 0).any()) else 0.0)
    return ecol, evar


def _assert_shape(sim, m, lanes, rows):
    """k_frame_jacobian's launch is the restated plan's (tests/wide_models.py frame_jacobian_shape): lanes per environment, LDS bytes, blocks per
    frame.  lanes: what the batch was forced to (0: nothing, or TSIM_LPE)"""
    env = int(os.environ.get("TSIM_LPE", "0"))
    forced = lanes or (env if env in (16, 32, 64) else 0)
    n_simd = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    want = W.frame_jacobian_shape(m, forced, 8 if sim.dtype == F64 else 4, rows, sim.B, n_simd, sim.kernel_variant() != "generic")
    fl = sim.frame_jacobians_launch_info()
    assert (fl["lanes_per_env"], fl["lds_bytes"], fl["lds_bytes"] <= 64 * 1024) == want and fl["threads"] == 64, (forced, fl, want)
    assert fl["blocks"] == -(-sim.B // (64 // fl["lanes_per_env"]))
    return fl, want


def _check_columns(name, dtype, lanes=0, static=False, rows=True, expect_variant=None, case=None, bound=None):
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = _as_bdf1(*case) if case else _case(name, B)
    sim = PU.make_sim(m, B, dtype, T * S, lanes=lanes, static=static)
    tab = PU.table_rows(m, B, dtype == F32, 11) if rows else None
    _roll(sim, tab, q0, qd0, u, S)
    if expect_variant:
        assert sim.kernel_variant() == expect_variant
    fl, _ = _assert_shape(sim, m, lanes, rows)
    assert fl["lanes_per_env"] >= sim.launch_info()["lanes_per_env"] and fl["lds_bytes"] <= 64 * 1024, fl
    fj = sim.frame_jacobians(T, S, want_var=True)
    assert sim.tape_len() == T * S
    nr, nu = sim.ndof_r, sim.ndof_u
    assert tuple(fj["A"].shape) == (T, B, 2 * nr, 2 * nr) and tuple(fj["B"].shape) == (T, B, 2 * nr, nu)
    assert all(bool(torch.isfinite(x).all()) for x in fj.values())
    ecol, evar = _column_errors(sim, T, S, fj, _tangent_ndir(sim))
    print("columns %-24s %s lanes %2d (k_frame_jacobian at %2d) static %d rows %d: column error %.3e Jvar error %.3e" % (
        name, "f64" if dtype == F64 else "f32", lanes, fl["lanes_per_env"], static, rows, ecol, evar))
    if STATS:
        with open(STATS, "a") as fh:
            fh.write("%s %s %d/%d %d %d %.4e %.4e\n" % (name, "f64" if dtype == F64 else "f32", lanes, fl["lanes_per_env"], static, rows, ecol, evar))
    assert MEASURED[dtype] < CAP[dtype]
    bound = bound or BOUND[dtype]      # (a case of tests/test_gpu_frame_jacobian_edges.py over BOUND: 10 x its own measured worst, which is under CAP)
    assert BOUND[dtype] <= bound < 10 * CAP[dtype]
    assert ecol <= bound and evar <= bound, (name, ecol, evar)
    return sim, fj


# ---------------------------------------------------------------------------------------------------- 1. against k_tangent, every column
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", CASES)
def test_columns_against_the_tangent_pass(name, dtype):
    """every case, per-environment rows, the library's launch shape: every entry of A_f, B_f and Jvar_f of every frame and environment"""
    _check_columns(name, dtype)


# ---------------------------------------------------------------------------------------------------- 2. the chain
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["pusher", "dclaw_position_control", "pad_press"])
def test_chain_reproduces_the_episode_tangent(name, dtype):
    """x_{f+1} = A_f x_f + B_f du_f (in double on the host) against tangent_episode's dq, dqd at every frame, for random (dq0, dqd0, du).
    The scale: the column test lets every entry of [A_f | B_f] differ from k_tangent's by BOUND x (the largest magnitude of its row), so one
    step of the chain may differ by BOUND x rowmax_i x ||(x_f, du_f)||_1 in entry i, and an earlier difference e_f travels on as |A_f| e_f:
        sigma_0 = 0 ,   sigma_{f+1} = |A_f| sigma_f + rowmax(f) ||(x_f, du_f)||_1 ,   |chain - tangent| <= BOUND x sigma_f   per entry
    — sigma_f is a sum of f local terms, which is the factor T of a bound stated per episode."""
    from tactilesimulation_amd.functions import episode_transition
    B, T, nd = 5, T_FRAMES, 3
    m, q0, qd0, u, S = _case(name, B)
    sim = PU.make_sim(m, B, dtype, T * S)
    _roll(sim, PU.table_rows(m, B, dtype == F32, 11), q0, qd0, u, S)
    rng = np.random.default_rng(91)
    nr, nu = sim.ndof_r, sim.ndof_u
    du, dq0, dqd0 = (_t(rng.normal(size=s), dtype) for s in ((nd, T, B, nu), (nd, B, nr), (nd, B, nr)))
    o = sim.tangent_episode(T, S, du=du, dq0=dq0, dqd0=dqd0, want_qd=True, want_var=False, want_tactile=False)
    A, Bm = (x.double() for x in episode_transition(sim, T, S))
    x = torch.cat([dq0, dqd0], 2).double()                                   # [nd, B, 2 nr]
    ref, sig = x, torch.zeros_like(x)
    worst = 0.0
    for f in range(T):
        duf = du[:, f].double()
        rowmax = torch.cat([A[f], Bm[f]], 2).abs().amax(2)                   # [B, 2 nr]
        n1 = ref.abs().sum(2) + duf.abs().sum(2)                              # [nd, B]
        sig = torch.einsum("bij,dbj->dbi", A[f].abs(), sig) + rowmax.unsqueeze(0) * n1.unsqueeze(2)
        x = torch.einsum("bij,dbj->dbi", A[f], x) + torch.einsum("bij,dbj->dbi", Bm[f], duf)
        ref = torch.cat([o["dq"][:, f], o["dqd"][:, f]], 2).double()
        assert float(sig.min()) > 0
        worst = max(worst, float(((x - ref).abs() / sig).max()))
    print("chain %-24s %s: worst %.3e" % (name, "f64" if dtype == F64 else "f32", worst))
    assert worst <= BOUND[dtype], (name, worst)


# ---------------------------------------------------------------------------------------------------- 3. against the oracle
@pytest.mark.parametrize("name", ["pusher", "pad_press"] + ORACLE_CASES)
def test_frame_jacobians_against_the_oracle_rows(name):
    """fp64, four environments with rows of their own, Newton tol 1e-13: every row of [A_f | B_f] against the oracle's adjoint rows of the frame
    started at the oracle's own (q_f, qd_f), each entry within 1e-7 of the row's scale (its largest magnitude).  pusher and pad_press keep their
    pivots on the diagonal; the corpus models of tests/frame_jacobian_cases.py ORACLE_CASES exchange rows, unambiguously, on these very rows
    (tests/test_frame_jacobian_cases.py) — the one yardstick here that shares no taped H, K or point evaluation with k_tangent"""
    B, T = 4, T_FRAMES
    m, q0, qd0, u, S = _case(name, B)
    m = copy.deepcopy(m)
    m.F[Bl.TSIM_FH_TOL] = 1e-13
    tab = PU.table_rows(m, B, False, 12)
    sim = PU.make_sim(m, B, F64, T * S)
    _roll(sim, tab, q0, qd0, u, S)
    fj = sim.frame_jacobians(T, S)
    AB = torch.cat([fj["A"], fj["B"]], 3).cpu().numpy()
    worst = 0.0
    for e in range(B):
        me = PU.row_model(m, tab[e])
        st = oracle_frame_states(me, q0[e], qd0[e], u[e], S)
        for f in range(T):
            rows = oracle_frame_rows(me, st[f][0], st[f][1], u[e, f], S)
            scale = np.abs(rows).max(1, keepdims=True)
            err = np.abs(AB[f, e] - rows) / scale
            worst = max(worst, float(err.max()))
            assert np.all(err <= 1e-7), (name, e, f, float(err.max()))
    print("oracle rows %s: worst |entry - oracle| / row scale = %.3e" % (name, worst))
    if STATS:
        with open(STATS, "a") as fh:
            fh.write("oracle_rows %s %.4e\n" % (name, worst))


# ---------------------------------------------------------------------------------------------------- 4. launch shapes, compiled-in model batches
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("name", ["pusher", "dclaw_position_control", "box_slide"])
def test_columns_at_every_launch_shape(name, lanes, dtype):
    _check_columns(name, dtype, lanes=lanes)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("name", ["wide9", "wide10"])
def test_columns_on_the_wide_models(name, lanes, dtype):
    """tests/wide_models.py: 9 / 10 dofs on few links — NRM 16 with four (fp32) and two environments per wavefront, which no fixed model reaches"""
    import wide_models as W
    _check_columns(name, dtype, lanes=lanes, case=W.wide_case(name, 5, T_FRAMES))


@pytest.mark.parametrize("dtype", [F64, F32])
def test_columns_with_a_rotation_vector_joint(dtype):
    """the EXPJ instantiations (NRM 16, 64 lanes): the tactile pad pressed on the ball, just before the drag — param_grad_util's case, whose model
    integrates with BDF2, run as a BDF1 model like small:3 and large:L7"""
    _check_columns("tactile_pad", dtype, case=PU.case("tactile_pad", 5, T_FRAMES))


@pytest.mark.parametrize("dtype,rows,variant", [(F32, False, "static:pusher"), (F32, True, "param:pusher"), (F64, False, "static:pusher")])
def test_columns_on_a_compiled_in_model_batch(dtype, rows, variant):
    """the generic k_frame_jacobian over the tape a static:pusher / param:pusher batch recorded (K in its records), as k_tangent runs there"""
    if dtype == F64 and os.environ.get("TSIM_LPE") == "16":
        variant = "generic"
    _check_columns("pusher", dtype, static=True, rows=rows, expect_variant=variant)


# ---------------------------------------------------------------------------------------------------- 5. exact zeros and structure
@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_clipped_force_control_has_exactly_zero_columns(dtype):
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("limit_push", B)
    mo = int(m.I[Bl.TSIM_IH_OFF_MOTOR])
    force = [k for k in range(m.ndof_u) if m.I[mo + k * Bl.TSIM_MI_SIZE + Bl.TSIM_MI_CTRL] == 0]
    assert force
    k = force[0]
    u = u.copy()
    u[:, 1, k] = 1.5                                                          # frame 1: outside [-1, 1]
    u[1, 1, k] = -1.25
    sim = PU.make_sim(m, B, dtype, T * S)
    _roll(sim, None, q0, qd0, u, S)
    Bm = sim.frame_jacobians(T, S)["B"]
    assert bool((Bm[1, :, :, k] == 0).all())
    assert bool((Bm[0, :, :, k] != 0).any(1).all()) and bool((Bm[2, :, :, k] != 0).any(1).all())
    other = [j for j in range(m.ndof_u) if j != k]
    assert bool((Bm[1][:, :, other] != 0).any())


@pytest.mark.parametrize("dtype", [F64, F32])
def test_free_flight_is_the_double_integrator(dtype):
    """box_slide lifted off the ground (no contact, no damping, constant mass matrix): A_qq = I, A_qv = h S I, A_vq = 0, A_vv = I to round-off"""
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("box_slide", B)
    q0 = q0.copy()
    q0[:, 2] = 0.05
    sim = PU.make_sim(m, B, dtype, T * S)
    _roll(sim, None, q0, qd0, u, S)
    A = sim.frame_jacobians(T, S)["A"].double()
    nr = sim.ndof_r
    I = torch.eye(nr, device=DEV, dtype=F64).expand(T, B, nr, nr)
    eps = 64 * torch.finfo(dtype).eps
    assert float((A[..., :nr, :nr] - I).abs().max()) <= eps
    assert float((A[..., :nr, nr:] - m.h * S * I).abs().max()) <= eps * m.h * S
    assert float((A[..., nr:, nr:] - I).abs().max()) <= eps
    assert float(A[..., nr:, :nr].abs().max()) <= eps / m.h


# ---------------------------------------------------------------------------------------------------- 6. changes nothing
@pytest.mark.parametrize("static,rows,variant", [(False, True, "generic"), (True, False, "static:pusher"), (True, True, "param:pusher")])
def test_frame_jacobian_launches_change_nothing(static, rows, variant):
    """roll-out -> 0, 1 or 3 frame_jacobians launches -> a tangent launch and the adjoint, bit for bit"""
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    res = []
    for nfj in (0, 1, 3):
        sim = PU.make_sim(m, B, F32, T * S, static=static)
        tab = PU.table_rows(m, B, True, 11) if rows else None
        out = _roll(sim, tab, q0, qd0, u, S)
        assert sim.kernel_variant() == variant
        for i in range(nfj):
            sim.frame_jacobians(T if i != 1 else T - 1, S, want_var=True)
        assert sim.tape_len() == T * S and sim.last_adjoint_launch()["kernel"] is None
        st = sim.get_state()
        rng = np.random.default_rng(52)
        tan = sim.tangent_episode(T, S, du=_t(rng.normal(size=(2, T, B, sim.ndof_u)), F32), dq0=_t(rng.normal(size=(2, B, sim.ndof_r)), F32), want_qd=True)
        w = [_t(rng.normal(size=(T, B, d)), F32) for d in (sim.ndof_r, sim.ndof_var, sim.ndof_tactile)]
        du = sim.backward_episode(T, S, w[0], w[1], w[2])
        lq, lv = sim.get_adjoint()
        res.append([out["q"], out["qd"], out["var"], out["tactile"], out["status"], st[0], st[1], du, lq, lv] + [tan[k] for k in sorted(tan)])
        assert sim.tape_len() == 0 and sim.kernel_variant() == variant
    for r in res[1:]:
        assert all(torch.equal(a, b) for a, b in zip(res[0], r))


# ---------------------------------------------------------------------------------------------------- 7. independence of the outputs
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["pusher", "dclaw_position_control"])
def test_outputs_are_independent_of_each_other_and_of_the_window(name, dtype):
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = _case(name, B)
    sim = PU.make_sim(m, B, dtype, T * S)
    _roll(sim, PU.table_rows(m, B, dtype == F32, 11), q0, qd0, u, S)
    full = sim.frame_jacobians(T, S, want_var=True)
    onlyA = sim.frame_jacobians(T, S, want_A=True, want_B=False, want_var=False)
    onlyB = sim.frame_jacobians(T, S, want_A=False, want_B=True, want_var=False)
    assert set(onlyA) == {"A"} and torch.equal(onlyA["A"], full["A"]) and torch.equal(onlyB["B"], full["B"])
    half = sim.frame_jacobians(T - 1, S, want_var=True)                       # the newest 2 of 3 frames
    for k in full:
        assert torch.equal(half[k], full[k][1:]), k
    # Jvar alone: no solve, the same taped point
    onlyJ = sim.frame_jacobians(T, S, want_A=False, want_B=False, want_var=True)
    assert torch.equal(onlyJ["Jvar"], full["Jvar"])


# ---------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    from tactilesimulation_amd.host import capi
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    sim = PU.make_sim(m, B, F64, T * S)
    L = capi.lib()
    nr, nu = sim.ndof_r, sim.ndof_u
    A = torch.full((T + 1, B, 2 * nr, 2 * nr), 7.0, device=DEV, dtype=F64)
    Bo = torch.full((T + 1, B, 2 * nr, nu), 7.0, device=DEV, dtype=F64)
    call = lambda h, nf, ns: L.tsim_frame_jacobians(h, nf, ns, A.data_ptr(), Bo.data_ptr(), None, None)
    sim.kernel_timing(True)
    assert call(None, T, S) != 0 and b"null batch" in L.tsim_last_error()
    sim.reset(_t(q0, F64), None, backward_flag=True)
    assert call(sim._h, T, S) != 0 and b"no tape" in L.tsim_last_error()
    _roll(sim, None, q0, qd0, u, S)
    sim.kernel_times()
    for nf, ns in ((0, S), (T, 0), (-1, S)):
        assert call(sim._h, nf, ns) != 0 and b"must be positive" in L.tsim_last_error()
    assert call(sim._h, T + 1, S) != 0 and b"sub-steps on the tape" in L.tsim_last_error()
    mb, q0b, qd0b, ub, Sb = tangent_case("bdf2:ball_push", B)
    simb = PU.make_sim(mb, B, F64, T * Sb)
    _roll(simb, None, q0b, qd0b, ub, Sb)
    assert L.tsim_frame_jacobians(simb._h, T, Sb, None, None, None, None) != 0 and b"BDF2" in L.tsim_last_error()
    import ctypes
    assert L.tsim_frame_jacobians_launch_info(None, (ctypes.c_int32 * 4)()) != 0
    torch.cuda.synchronize()
    assert all(n == 0 for _, n in sim.kernel_times().values())               # nothing was launched on the batch's timed kinds ...
    assert bool((A == 7).all()) and bool((Bo == 7).all())                     # ... and nothing was written
    # a valid launch after the refusals still gives the right answer
    fj = sim.frame_jacobians(T, S, want_var=True)
    ecol, evar = _column_errors(sim, T, S, fj)
    assert ecol <= BOUND[F64] and evar <= BOUND[F64]


# ---------------------------------------------------------------------------------------------------- 9. the ragged batch
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["pusher", "box_slide", "small:11"])
def test_the_last_environment_of_a_ragged_batch(name, dtype):
    """B = 5: environment 4 sits alone in the last block; its matrices are those of a B = 1 batch with its inputs, bit for bit (small:11 of the
    random corpus exchanges rows in its solve in every frame: tests/test_frame_jacobian_cases.py)"""
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = _case(name, B)
    rng = np.random.default_rng(5)
    q0 = q0 + 1e-4 * rng.normal(size=q0.shape)                                # (environments that differ)
    tab = PU.table_rows(m, B, dtype == F32, 11)
    sim = PU.make_sim(m, B, dtype, T * S)
    _roll(sim, tab, q0, qd0, u, S)
    lanes = sim.frame_jacobians_launch_info()["lanes_per_env"]
    full = sim.frame_jacobians(T, S, want_var=True)
    one = PU.make_sim(m, 1, dtype, T * S, lanes=sim.launch_info()["lanes_per_env"])
    _roll(one, tab[4:], q0[4:], qd0[4:], u[4:], S)
    assert one.frame_jacobians_launch_info()["lanes_per_env"] == lanes
    solo = one.frame_jacobians(T, S, want_var=True)
    for k in full:
        assert torch.equal(full[k][:, 4], solo[k][:, 0]), k
    assert bool((full["A"][:, 4] != full["A"][:, 3]).any())


# ---------------------------------------------------------------------------------------------------- 10. capturable
def test_a_captured_launch_replays_to_the_eager_bits():
    """no allocation and no host synchronisation in the call: it is captured into a graph, and the replay writes the eager launch's bits"""
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    sim = PU.make_sim(m, B, F32, T * S)
    _roll(sim, PU.table_rows(m, B, True, 11), q0, qd0, u, S)
    eager = sim.frame_jacobians(T, S, want_var=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sim.frame_jacobians(T, S, want_var=True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a = sim.frame_jacobians(T, S, want_var=True)
    for x in a.values():
        x.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a[k], eager[k]) for k in eager)
    assert sim.tape_len() == T * S
