"""The per-frame tactile Jacobians of a taped episode (include/tsim.h tsim_tactile_jacobians, BatchSim.tactile_jacobians, functions.episode_observation).

k_tactile_jacobian is the tactile section of k_tangent for unit directions, one (environment, masked frame) per slot.  So it is held to k_tangent
itself: for 8 random directions (du, dq0, dqd0) every masked frame must satisfy dtactile[d] = sum_k Ct[k] dx_k with dx = (dq, dqd) of the same frame.
The error of an entry is |difference| / sum_k |Ct[k] dx_k| and is exactly 0 where that scale is 0; its bound is 10 x the largest value measured
over every case of this file on the MI355X (MEASURED below, profiles/r25_tactile_jacobians.md), which must stay under the tangent's caps 1e-10 / 1e-4.
The oracle: C [A | B] of the two launches against the adjoint rows of tests/tactile_jacobian_cases.py oracle_tactile_rows (checked on the CPU by
tests/test_tactile_jacobian_yardstick.py), fp64 within 1e-7 of the row's scale at Newton tol 1e-13, fp32 within 10 x the measured value; and C v
against Richardson differences of the oracle's read-out map along the yardstick's pinned draw, at the yardstick's 1e-3.
The rest: the taxel loop's tails, second trips and later-primitive adds on the synthetic pads of tests/pad_models.py at 16 / 32 / 64 forced lanes,
a sensor without primitives, BDF2 and rotation-vector models, exact zeros, per-environment tables, the invariances, that the launch changes
nothing, a captured launch, the refusals and the launch shape (tactile_jacobian_cases.tactile_jacobian_shape: lanes, LDS bytes, blocks, exactly).
The refusal for a block over the LDS cap is not run: no model of the suite reaches it (the 16-dof large:L2 in fp64: 61 600 bytes at one
environment per wavefront) — nor the one for more than 2^31 - 1 blocks, which a tape that long would not fit memory for."""
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
import tactile_jacobian_cases as TC      # noqa: E402
import wide_models as W      # noqa: E402
from test_tangent_yardstick import T_FRAMES, tangent_case      # noqa: E402
from test_frame_jacobian_yardstick import oracle_frame_states      # noqa: E402
from test_tactile_jacobian_yardstick import PAD_CASES, READOUT_DRAW_USED, readout_difference      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = PU.DEV
F64, F32 = torch.float64, torch.float32
# the largest errors measured over every case of this file on the MI355X (profiles/r25_tactile_jacobians.md); the bounds are 10 x
MEASURED = {F64: 2.641e-14, F32: 3.129e-5}        # against k_tangent: both on the pad large_300_blind_725 (1032 taxels, 2 sensors x 3 primitives and a blind one)
MEASURED_ORACLE_F32 = 4.797e-3                      # fp32 C [A | B] against the oracle's rows, of the row's scale: pad_1x8 (pad_4x2: 8.95e-4, pusher: 7.4e-6)
CAP = {F64: 1e-10, F32: 1e-4}
BOUND = {dt: 10 * MEASURED[dt] for dt in MEASURED}
STATS = os.environ.get("TSIM_TACTILE_JACOBIAN_STATS")      # a file: every case's largest errors are appended to it (the profile)
NDIR = 8


@pytest.fixture(scope="module")
def pad_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("tj_pads")


def _t(x, dt):
    return torch.tensor(np.ascontiguousarray(x), device=DEV, dtype=dt)


def _roll(sim, tab, q0, qd0, u, S, mask=None):
    dt = sim.dtype
    if tab is not None:
        sim.set_env_tables(_t(tab, dt))
    sim.reset(_t(q0, dt), _t(qd0, dt), backward_flag=True)
    return sim.rollout(_t(u.transpose(1, 0, 2), dt), S, want_qd=True, tactile_mask=mask)


def _stat(line):
    print(line)
    if STATS:
        with open(STATS, "a") as fh:
            fh.write(line + "\n")


def _tangent_error(sim, T, S, Ct, mask=None, seed=91):
    """largest |dtactile[d] - sum_k Ct[k] dx_k| / sum_k |Ct[k] dx_k| over 8 random directions, the masked frames, environments and entries;
    exactly 0 is asserted where the scale is 0"""
    B, nr, nu, dt = sim.B, sim.ndof_r, sim.ndof_u, sim.dtype
    rng = np.random.default_rng(seed)
    du, dq0, dqd0 = (_t(rng.normal(size=s), dt) for s in ((NDIR, T, B, nu), (NDIR, B, nr), (NDIR, B, nr)))
    o = sim.tangent_episode(T, S, du=du, dq0=dq0, dqd0=dqd0, tactile_mask=mask, want_qd=True, want_var=False)
    frames = [f for f in range(T) if mask is None or bool(mask[f])]
    assert Ct.shape[0] == len(frames) == o["dtactile"].shape[1]
    worst = 0.0
    for i, f in enumerate(frames):
        dx = torch.cat([o["dq"][:, f], o["dqd"][:, f]], 2).double()          # [ndir, B, 2 nr]
        C = Ct[i].double()                                                   # [B, 2 nr, ntac]
        got = torch.einsum("bkt,dbk->dbt", C, dx)
        sc = torch.einsum("bkt,dbk->dbt", C.abs(), dx.abs())
        diff = (got - o["dtactile"][:, i].double()).abs()
        assert bool((diff[sc == 0] == 0).all())
        if bool((sc > 0).any()):
            worst = max(worst, float((diff / sc.clamp_min(1e-300))[sc > 0].max()))
    return worst


def _assert_shape(sim, m, lanes, rows):
    """k_tactile_jacobian's launch is the restated plan's: lanes per environment, LDS bytes, blocks per frame, exactly"""
    env = int(os.environ.get("TSIM_LPE", "0"))
    forced = lanes or (env if env in (16, 32, 64) else 0)
    n_simd = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    want = TC.tactile_jacobian_shape(m, forced, 8 if sim.dtype == F64 else 4, rows, sim.B, n_simd, sim.kernel_variant() != "generic")
    fl = sim.tactile_jacobians_launch_info()
    assert (fl["lanes_per_env"], fl["lds_bytes"], fl["lds_bytes"] <= 64 * 1024) == want and fl["threads"] == 64, (forced, fl, want)
    assert fl["blocks"] == -(-sim.B // (64 // fl["lanes_per_env"]))
    return fl


def _check(name, case, dtype, lanes=0, static=False, rows=True, mask=None, expect_variant=None, want_lanes=None):
    """one case against k_tangent: shape, finiteness, the error bound; returns (sim, Ct, model)"""
    m, q0, qd0, u, S = case
    B, T = u.shape[0], u.shape[1]
    sim = PU.make_sim(m, B, dtype, T * S, lanes=lanes, static=static)
    tab = PU.table_rows(m, B, dtype == F32, 11) if rows else None
    _roll(sim, tab, q0, qd0, u, S, mask)
    if expect_variant:
        assert sim.kernel_variant() == expect_variant
    fl = _assert_shape(sim, m, lanes, rows)
    if want_lanes:
        assert fl["lanes_per_env"] == want_lanes, (fl, want_lanes)
    nm = T if mask is None else int(mask.sum())
    torch.full((nm, B, 2 * sim.ndof_r, sim.ndof_tactile), float("nan"), device=DEV, dtype=dtype)      # (the allocator's next block of this shape is NaN)
    Ct = sim.tactile_jacobians(T, S, mask)
    assert sim.tape_len() == T * S and tuple(Ct.shape) == (nm, B, 2 * sim.ndof_r, sim.ndof_tactile)
    assert bool(torch.isfinite(Ct).all()), (name, "an entry was not written")
    err = _tangent_error(sim, T, S, Ct, mask)
    _stat("tangent %-28s %s lanes %2d (kernel at %2d) static %d rows %d: error %.3e nonzero %d" % (
        name, "f64" if dtype == F64 else "f32", lanes, fl["lanes_per_env"], static, rows, err, int((Ct != 0).sum())))
    assert MEASURED[dtype] < CAP[dtype]
    assert err <= BOUND[dtype], (name, err)
    return sim, Ct, m


# ---------------------------------------------------------------------------------------------------- the census
# instantiation (real, NRM, EXPJ, lanes) of k_tactile_jacobian -> (case, forced lanes, per-environment rows, the test of this file that runs it); the
# shapes are the restated plan's (tests/test_tactile_jacobian_kernel_table.py checks all of it against the kernel table)
_SH = "test_fixed_models_at_every_launch_shape"
_WD = "test_wide_model_at_every_launch_shape"
REACHED_BY = {
    ("f", 8, False, 16): ("pusher", 16, True, _SH), ("f", 8, False, 32): ("pusher", 32, True, _SH), ("f", 8, False, 64): ("pusher", 64, True, _SH),
    ("d", 8, False, 16): ("small_130_1x1", 16, False, "test_four_pad_environments_per_wavefront_on_the_shared_model"),
    ("d", 8, False, 32): ("pusher", 16, True, _SH), ("d", 8, False, 64): ("pusher", 64, True, _SH),
    ("f", 16, False, 16): ("wide9", 16, True, _WD), ("f", 16, False, 32): ("wide9", 32, True, _WD), ("f", 16, False, 64): ("wide9", 64, True, _WD),
    ("d", 16, False, 32): ("wide9", 16, True, _WD), ("d", 16, False, 64): ("wide9", 64, True, _WD),
    ("f", 16, True, 64): ("bdf2:ball_push", 0, True, "test_against_the_tangent_pass"), ("d", 16, True, 64): ("bdf2:ball_push", 0, True, "test_against_the_tangent_pass"),
}
UNREACHABLE = {("d", 16, False, 16)}      # four fp64 contexts of a model of more than 8 dofs are over 64 KB (tests/test_wide_models.py, the same row of every kernel)


def census_model(case, dirpath):
    return W.wide_model(case) if case in W.WIDE else P.table_model(case, dirpath) if case in P.TABLE else tangent_case(case, 1)[0]


# ---------------------------------------------------------------------------------------------------- 1. against k_tangent, the fixed models
FIXED = ["pusher", "dclaw_position_control", "tactile_insertion", "bdf2:ball_push"]      # (pad_press of the tangent cases loads no taxel: it would compare zeros)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", FIXED)
def test_against_the_tangent_pass(name, dtype):
    """B = 5 (ragged at 4 and 2 per wavefront), T = 3 frames, per-environment rows, the library's launch shape; bdf2:ball_push: BDF2 with a
    rotation-vector joint (EXPJ)"""
    sim, Ct, m = _check(name, tangent_case(name, 5), dtype)
    assert bool((Ct != 0).any())


@pytest.mark.parametrize("dtype", [F64, F32])
def test_masked_frames_of_a_ragged_pusher_batch(dtype):
    """pusher, B = 5, T = 3, mask [1, 0, 1]: the output slot follows the mask"""
    mask = torch.tensor([True, False, True])
    sim, Ct, m = _check("pusher mask101", tangent_case("pusher", 5), dtype, mask=mask)
    full = sim.tactile_jacobians(T_FRAMES, 5)
    assert torch.equal(Ct[0], full[0]) and torch.equal(Ct[1], full[2]) and not torch.equal(full[1], full[2])


# ---------------------------------------------------------------------------------------------------- 3. shapes
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("nt", P.ADJ_NT)
def test_taxel_chunks_on_the_pads(nt, lanes, dtype, pad_dir):
    """adj_<nt>: one sensor of nt taxels over the slab — the chunk loop's tails (nt = lanes k - 1, + 1) and second and third trips"""
    name = "adj_%d" % nt
    sim, Ct, m = _check(name, TC.pad_case(name, pad_dir, 4), dtype, lanes=lanes, want_lanes=lanes if dtype == F32 or lanes > 16 else 32)      # (four fp64 contexts of a pad are over the cap)
    assert bool((Ct[0, :3] != 0).any())                                     # a pressed state loads something; the lifted one (environment 3) nothing
    assert bool((Ct[0, 3] == 0).all())


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("combo", P.SMALL_COMBOS)
def test_sensors_and_primitives_on_the_pads(combo, lanes, dtype, pad_dir):
    """small_130_<sensors>x<primitives>: several sensors, and the later primitives' add path"""
    name = "small_130_%dx%d" % combo
    _check(name, TC.pad_case(name, pad_dir, 4), dtype, lanes=lanes, want_lanes=lanes if dtype == F32 or lanes > 16 else 32)      # (four fp64 contexts of a pad are over the cap)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_sensor_without_primitives_gives_exact_zeros(dtype, pad_dir):
    name = "large_300_blind_725"
    sim, Ct, m = _check(name, TC.pad_case(name, pad_dir, 4), dtype)
    blind = ~P.paired_taxels(m)
    assert blind.sum() == 7
    C = Ct.reshape(1, 4, 12, -1, 3)
    assert bool((C[:, :, :, torch.tensor(blind, device=DEV)] == 0).all()) and bool((C != 0).any())


@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_bdf2_pad(dtype, pad_dir):
    m = P.pad_model(os.path.join(str(pad_dir), "bdf2_130_4x2"), P.split(130, 4), 2, integrator="BDF2")
    st = P.states(m, 0, "mixed", 3) + P.states(m, 1, "all_out", 1)
    q0, qd0 = np.stack([s[0] for s in st]), np.stack([s[1] for s in st])
    u = np.tile(TC.PAD_U[None, None], (4, 2, 1))
    _check("bdf2_130_4x2", (m, q0, qd0, u, 2), dtype)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("name", ["pusher"])
def test_fixed_models_at_every_launch_shape(name, lanes, dtype):
    """(pusher in fp64 at 16 forced lanes runs at 32: four contexts are over the cap)"""
    _check(name, tangent_case(name, 5), dtype, lanes=lanes)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [16])
@pytest.mark.parametrize("name", ["small_130_1x1", "small_130_4x2"])
def test_four_pad_environments_per_wavefront_on_the_shared_model(name, lanes, dtype, pad_dir):
    """without per-environment rows four fp64 contexts of a pad fit the block: the only fp64 runs of this file at 16 lanes (NRM 8)"""
    _check(name, TC.pad_case(name, pad_dir, 5), dtype, lanes=lanes, rows=False, want_lanes=16)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("name", ["wide9"])
def test_wide_model_at_every_launch_shape(name, lanes, dtype):
    """tests/wide_models.py: 9 dofs on few links — NRM 16 with four (fp32) and two environments per wavefront"""
    _check(name, W.wide_case(name, 5, T_FRAMES), dtype, lanes=lanes)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_dclaw_three_sensors_on_a_cylinder(dtype):
    """D'Claw: B = 3, T = 1; NRM 16, three sensors on the cylinder primitive.  A finger's dofs move neither body of another finger's pair: those
    columns of that sensor's taxels are exactly zero, and every dof in a sensor's mask has a non-zero column somewhere"""
    m, q0, qd0, u, S = tangent_case("dclaw_position_control", 3)
    sim, Ct, m = _check("dclaw B3 T1", (m, q0, qd0, u[:, :1], S), dtype)
    nr = m.ndof_r
    C = Ct[0].reshape(3, 2, nr, -1, 3)
    for t0, nt, mask in TC.sensor_dof_masks(m):
        out = [k for k in range(nr) if not (mask >> k) & 1]
        assert out and bool((C[:, :, out, t0:t0 + nt] == 0).all())
    assert bool((C != 0).any())


@pytest.mark.parametrize("dtype", [F64, F32])
def test_tactile_insertion_two_pads(dtype):
    """12 dofs, two pads, B = 3"""
    m, q0, qd0, u, S = tangent_case("tactile_insertion", 3)
    sim, Ct, m = _check("tactile_insertion B3", (m, q0, qd0, u[:, :2], S), dtype)
    nr = m.ndof_r
    C = Ct.reshape(2, 3, 2, nr, -1, 3)
    for t0, nt, mask in TC.sensor_dof_masks(m):
        out = [k for k in range(nr) if not (mask >> k) & 1]
        assert out and bool((C[:, :, :, out, t0:t0 + nt] == 0).all())


@pytest.mark.parametrize("dtype", [F64, F32])
def test_the_tactile_pad_of_120000_values(dtype):
    """assets' tactile_pad: B = 2, T = 1 — the EXPJ instantiation, BDF2, 40 000 taxels: 625 trips of the chunk loop, 2.16 M values per environment"""
    m, q0, qd0, u, S = PU.case("tactile_pad", 2, 1)
    sim, Ct, m = _check("tactile_pad B2 T1", (m, q0, qd0, u, S), dtype)
    assert Ct.shape[-1] == 120000 and bool((Ct != 0).any())


@pytest.mark.parametrize("dtype,rows,variant", [(F32, False, "static:pusher"), (F32, True, "param:pusher"), (F64, False, "static:pusher")])
def test_on_a_compiled_in_model_batch(dtype, rows, variant):
    """the generic k_tactile_jacobian over the tape a static:pusher / param:pusher batch recorded (K in its records), held to k_tangent on that
    very tape — the same states — to the bound of the tangent test.  (A generic batch records its own tape, which differs from this one by the
    forward kernels' round-off: its result is not comparable entry by entry at a round-off bound.)"""
    if dtype == F64 and os.environ.get("TSIM_LPE") == "16":
        variant = "generic"
    case = tangent_case("pusher", 5)
    _check("pusher", case, dtype, static=True, rows=rows, expect_variant=variant)


# ---------------------------------------------------------------------------------------------------- 2. against the oracle
def _oracle_case(name, pad_dir, B):
    """model at Newton tol 1e-13, q0, qd0, u [B, T, nu], S, and whether pad_models.borderline applies"""
    if name in PAD_CASES:
        m, q0, qd0, u, S = TC.pad_case(PAD_CASES[name], pad_dir, B)
        pad = True
    else:
        m, q0, qd0, u, S = tangent_case(name, B)
        pad = False
    m = copy.deepcopy(m)
    m.F[Bl.TSIM_FH_TOL] = 1e-13
    return m, q0, qd0, u, S, pad


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["pusher", "pad_4x2", "pad_1x8"])
def test_against_the_oracle_rows(name, dtype, pad_dir):
    """C [A | B] of the two launches against the oracle's adjoint rows of the LAST frame started at the oracle's own (q_f, qd_f): fp64 each entry
    within 1e-7 of the row's scale (its largest magnitude), fp32 within 10 x the measured value.  The rows the oracle leaves at zero (unloaded
    taxels) are exactly zero here too, except on borderline taxels of the pads, which are left out (at most 1 %)"""
    B = 3
    m, q0, qd0, u, S, pad = _oracle_case(name, pad_dir, B)
    T = u.shape[1]
    sim = PU.make_sim(m, B, dtype, T * S)
    _roll(sim, None, q0, qd0, u, S)
    mask = torch.zeros(T, dtype=torch.bool)
    mask[T - 1] = True
    Ct = sim.tactile_jacobians(T, S, mask)[0].double()                       # [B, 2 nr, ntac]
    fj = sim.frame_jacobians(T, S)
    AB = torch.cat([fj["A"][T - 1], fj["B"][T - 1]], 2).double()             # [B, 2 nr, 2 nr + nu]
    CAB = torch.einsum("bkt,bkj->btj", Ct, AB).cpu().numpy()
    worst = 0.0
    for e in range(B):
        st = oracle_frame_states(m, q0[e], qd0[e], u[e], S)
        rows, ld = TC.oracle_tactile_rows(m, st[T - 1][0], st[T - 1][1], u[e, T - 1], S)
        keep = TC.pad_keep(m, *st[T])[1] if pad else np.ones_like(ld)
        k3 = np.repeat(keep, 3)
        scale = np.abs(rows).max(1, keepdims=True)
        diff = np.abs(CAB[e] - rows)
        assert np.all(diff[k3 & (scale[:, 0] == 0)] == 0), (name, e, "an unloaded taxel has a row")
        ok = k3 & (scale[:, 0] > 0)
        if ok.any():
            worst = max(worst, float((diff[ok] / scale[ok]).max()))
    _stat("oracle_rows %s %s: worst |entry - oracle| / row scale = %.3e" % (name, "f64" if dtype == F64 else "f32", worst))
    assert worst > 0
    assert worst <= (1e-7 if dtype == F64 else 10 * MEASURED_ORACLE_F32), (name, worst)


@pytest.mark.parametrize("name", list(READOUT_DRAW_USED))
def test_c_times_v_against_differences_of_the_read_out_map(name, pad_dir):
    """the check that does not pass through A: C v (fp64) against the Richardson differences of the oracle's reset(q, qd); outputs() at the last
    frame's end state along the yardstick's pinned draw, at the yardstick's 1e-3"""
    m, q0, qd0, u, S, pad = _oracle_case(name, pad_dir, 1)
    T = u.shape[1]
    sim = PU.make_sim(m, 1, F64, T * S)
    _roll(sim, None, q0, qd0, u, S)
    mask = torch.zeros(T, dtype=torch.bool)
    mask[T - 1] = True
    Ct = sim.tactile_jacobians(T, S, mask)[0, 0].double().cpu().numpy()     # [2 nr, ntac]
    q1, qd1 = oracle_frame_states(m, q0[0], qd0[0], u[0], S)[T]
    fd, v, used = readout_difference(m, q1, qd1, name)
    assert used == READOUT_DRAW_USED[name]
    keep = np.repeat(TC.pad_keep(m, q1, qd1)[1] if pad else np.ones(m.ndof_tactile // 3, bool), 3)
    ad, scale = v @ Ct, np.abs(v) @ np.abs(Ct)
    worst = float(np.max((np.abs(ad - fd) / np.maximum(np.abs(fd), np.maximum(1e-5 * scale, 1e-300)))[keep]))
    _stat("readout_fd %s: worst |C v - fd| / max(|fd|, 1e-5 scale) = %.3e" % (name, worst))
    assert np.any(fd != 0) and np.all((np.abs(ad - fd) <= 1e-3 * np.maximum(np.abs(fd), 1e-5 * scale))[keep]), (name, worst)


# ---------------------------------------------------------------------------------------------------- 4. exact structure
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["small_130_4x2", "small_130_1x8", "adj_129"])
def test_unloaded_taxels_have_exactly_zero_rows_and_loaded_ones_do_not(name, dtype, pad_dir):
    """against the oracle's taxel_list at the frame's end on the oracle (the pad is a free body: an fp32 batch follows it to ~1e-9 m), the
    borderline taxels left out"""
    m, q0, qd0, u, S = TC.pad_case(name, pad_dir, 4)
    sim = PU.make_sim(m, 4, dtype, S)
    _roll(sim, None, q0, qd0, u, S)
    Ct = sim.tactile_jacobians(1, S)[0].reshape(4, 12, -1, 3)
    any_loaded = False
    for e in range(4):
        q1, qd1 = oracle_frame_states(m, q0[e], qd0[e], u[e], S)[1]
        ld, keep = TC.pad_keep(m, q1, qd1)
        nz = (Ct[e] != 0).any(0).any(-1).cpu().numpy()                       # [ntax]: the taxel's row of C has a non-zero entry
        assert np.array_equal(nz[keep], ld[keep]), (name, e, np.nonzero(nz != ld)[0][:5])
        any_loaded |= bool(ld[keep].any())
    assert any_loaded


# ---------------------------------------------------------------------------------------------------- 5. per-environment tables
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["pusher", "small_130_4x2"])
def test_an_environment_of_a_table_batch_is_the_shared_model_of_its_row(name, dtype, pad_dir):
    B = 3
    m, q0, qd0, u, S = tangent_case(name, B) if name == "pusher" else TC.pad_case(name, pad_dir, B)
    T = u.shape[1]
    tab = PU.table_rows(m, B, dtype == F32, 11)
    sim = PU.make_sim(m, B, dtype, T * S)
    _roll(sim, tab, q0, qd0, u, S)
    lanes = sim.launch_info()["lanes_per_env"]
    Ct = sim.tactile_jacobians(T, S)
    for e in range(B):
        one = PU.make_sim(PU.row_model(m, tab[e].astype(np.float64)), B, dtype, T * S, lanes=lanes)
        _roll(one, None, q0, qd0, u, S)
        assert torch.equal(one.tactile_jacobians(T, S)[:, e], Ct[:, e]), (name, e)
    assert not torch.equal(Ct[:, 0], Ct[:, 1])


# ---------------------------------------------------------------------------------------------------- 6. invariances
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["pusher", "dclaw_position_control"])
def test_a_frames_bits_do_not_depend_on_the_window_the_mask_or_the_batch(name, dtype):
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case(name, B)
    q0 = q0 + 1e-4 * np.random.default_rng(5).normal(size=q0.shape)         # (environments that differ)
    tab = PU.table_rows(m, B, dtype == F32, 11)
    sim = PU.make_sim(m, B, dtype, T * S)
    _roll(sim, tab, q0, qd0, u, S)
    full = sim.tactile_jacobians(T, S)
    assert torch.equal(sim.tactile_jacobians(T - 1, S), full[1:])           # the newest 2 of 3 frames
    assert torch.equal(sim.tactile_jacobians(T, S, torch.tensor([False, True, False])), full[1:2])
    assert torch.equal(sim.tactile_jacobians(T, S, torch.tensor([True, False, True])), full[[0, 2]])
    lanes = sim.tactile_jacobians_launch_info()["lanes_per_env"]
    one = PU.make_sim(m, 1, dtype, T * S, lanes=sim.launch_info()["lanes_per_env"])
    _roll(one, tab[4:], q0[4:], qd0[4:], u[4:], S)
    assert one.tactile_jacobians_launch_info()["lanes_per_env"] == lanes
    assert torch.equal(one.tactile_jacobians(T, S)[:, 0], full[:, 4])
    assert bool((full[:, 4] != full[:, 3]).any())


def test_episode_observation_is_the_transposed_view():
    from tactilesimulation_amd.functions import episode_observation
    B, T = 2, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    sim = PU.make_sim(m, B, F32, T * S)
    _roll(sim, None, q0, qd0, u, S)
    mask = torch.tensor([False, True, True])
    C = episode_observation(sim, T, S, mask)
    Ct = sim.tactile_jacobians(T, S, mask)
    assert tuple(C.shape) == (2, B, sim.ndof_tactile, 2 * sim.ndof_r) and C.transpose(-1, -2).is_contiguous()
    assert torch.equal(C.transpose(-1, -2), Ct)


# ---------------------------------------------------------------------------------------------------- 7. read-only, capturable
@pytest.mark.parametrize("static,rows,variant", [(False, True, "generic"), (True, False, "static:pusher")])
def test_tactile_jacobian_launches_change_nothing(static, rows, variant):
    """roll-out -> 0 or 2 tactile_jacobians launches -> the adjoint, bit for bit"""
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    res = []
    for ntj in (0, 2):
        sim = PU.make_sim(m, B, F32, T * S, static=static)
        out = _roll(sim, PU.table_rows(m, B, True, 11) if rows else None, q0, qd0, u, S)
        assert sim.kernel_variant() == variant
        for i in range(ntj):
            sim.tactile_jacobians(T - i, S)
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
    """no allocation and no host synchronisation in the call (no mask: building a mask's slot map synchronises in Python): one kernel node"""
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    sim = PU.make_sim(m, B, F32, T * S)
    _roll(sim, PU.table_rows(m, B, True, 11), q0, qd0, u, S)
    eager = sim.tactile_jacobians(T, S)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sim.tactile_jacobians(T, S)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a = sim.tactile_jacobians(T, S)
    a.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, eager) and sim.tape_len() == T * S


# ---------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    from tactilesimulation_amd.host import capi
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    sim = PU.make_sim(m, B, F64, T * S)
    L = capi.lib()
    Ct = torch.full((T + 1, B, 2 * sim.ndof_r, sim.ndof_tactile), 7.0, device=DEV, dtype=F64)
    call = lambda h, nf, ns, out=Ct.data_ptr(): L.tsim_tactile_jacobians(h, nf, ns, None, out, None)      # noqa: E731
    sim.kernel_timing(True)
    assert call(None, T, S) != 0 and b"null batch" in L.tsim_last_error()
    sim.reset(_t(q0, F64), None, backward_flag=True)
    assert call(sim._h, T, S) != 0 and b"no tape" in L.tsim_last_error()
    _roll(sim, None, q0, qd0, u, S)
    sim.kernel_times()
    assert call(sim._h, T, S, None) != 0 and b"null Ct_out" in L.tsim_last_error()
    for nf, ns in ((0, S), (T, 0), (-1, S)):
        assert call(sim._h, nf, ns) != 0 and b"must be positive" in L.tsim_last_error()
    assert call(sim._h, T + 1, S) != 0 and b"sub-steps on the tape" in L.tsim_last_error()
    with pytest.raises(ValueError, match="no masked frame"):
        sim.tactile_jacobians(T, S, torch.zeros(T, dtype=torch.bool))
    mb, q0b, qd0b, ub, Sb = tangent_case("box_slide", B)                     # a model without taxels
    simb = PU.make_sim(mb, B, F64, T * Sb)
    _roll(simb, None, q0b, qd0b, ub, Sb)
    assert L.tsim_tactile_jacobians(simb._h, T, Sb, None, Ct.data_ptr(), None) != 0 and b"no taxels" in L.tsim_last_error()
    with pytest.raises(RuntimeError):
        simb.tactile_jacobians(T, Sb)
    assert L.tsim_tactile_jacobians_launch_info(None, (ctypes.c_int32 * 4)()) != 0
    torch.cuda.synchronize()
    assert all(n == 0 for _, n in sim.kernel_times().values())               # nothing was launched on the batch's timed kinds ...
    assert bool((Ct == 7).all())                                              # ... and nothing was written
    # a device mask without a masked frame, which the C entry cannot see: every block returns at once, nothing is written
    none = torch.full((T,), -1, device=DEV, dtype=torch.int32)
    assert L.tsim_tactile_jacobians(sim._h, T, S, none.data_ptr(), Ct.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((Ct == 7).all())
    # a valid launch after the refusals still gives the right answer
    assert _tangent_error(sim, T, S, sim.tactile_jacobians(T, S)) <= BOUND[F64]


# ---------------------------------------------------------------------------------------------------- 9. launch shape
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [0, 16, 32, 64])
@pytest.mark.parametrize("name", ["pusher", "pad_press", "dclaw_position_control", "tactile_insertion", "wide9", "wide10"])
def test_the_launch_shape_is_the_restated_plan(name, lanes, dtype):
    m = W.wide_model(name) if name in W.WIDE else tangent_case(name, 1)[0]
    for B, rows in ((5, True), (3, False)):
        sim = PU.make_sim(m, B, dtype, 2, lanes=lanes)
        if rows:
            sim.set_env_tables(_t(PU.table_rows(m, B, dtype == F32, 11), dtype))
        fl = _assert_shape(sim, m, lanes, rows)
        assert fl["lanes_per_env"] >= sim.launch_info()["lanes_per_env"]
