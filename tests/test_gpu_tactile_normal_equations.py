"""The tactile normal equations of a taped episode (include/tsim.h tsim_tactile_normal_equations, BatchSim.tactile_normal_equations,
functions.episode_information): N = H^T W H and n = H^T W r of H = [C_f | F_f] in one launch, without C_f or F_f being stored.

Yardstick A, every case: the product of what the library already ships and pins to the oracle — tactile_jacobians' Ct and param_jacobians' Ft of the
SAME batch and tape, Ft scattered to the dense F, H and the products formed with torch.einsum in float64 (tests/tactile_normal_cases.py).  The error
of an entry is |N_de - ref| / S_de, S_de = sum_i w_i |h_id| |h_ie| (for n: sum_i w_i |h_id| |r_i|); where S is 0 the entry must be exactly 0.  The
bound is 10 x the largest value measured over every case of this file on the MI355X (MEASURED below, profiles/r29_tactile_normal_equations.md), which
must stay under the tangent family's caps 1e-10 / 1e-4.  w is random in [1, 100], r random normal; both outputs are poisoned with NaN before
every launch.  Every case also checks: N bit-symmetric; the state block and n[:2 nr] with and without parameters, N with and without r, bit for bit.
Yardstick B, fp64: v^T N v against sum_i w_i fd_i^2 and v^T n against sum_i w_i fd_i r_i, fd the Richardson differences of the oracle's read-out
map along the pinned draw of tests/test_tactile_jacobian_yardstick.py, at that test's 1e-3.
The rest: chunk tails and the product pass's row tail on the pads at 16 / 32 / 64 forced lanes, several primitives per sensor (the rows are summed
before the product), several sensors (exactly zero blocks between their parameter columns), a blind sensor and a sensor without primitives, BDF2
and rotation-vector models, the 40 000-taxel pad, D'Claw, the insertion, the wide model, per-environment tables, the invariances, that the launch
changes nothing, a captured launch, the memory the call takes, the refusals and the launch shape (tactile_normal_cases.tactile_normal_shape)."""
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
import tactile_normal_cases as TN      # noqa: E402
import wide_models as W      # noqa: E402
from test_tangent_yardstick import T_FRAMES, tangent_case      # noqa: E402
from test_frame_jacobian_yardstick import oracle_frame_states      # noqa: E402
from test_tactile_jacobian_yardstick import PAD_CASES, READOUT_DRAW_USED, readout_difference      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = PU.DEV
F64, F32 = torch.float64, torch.float32
# the largest errors measured over every case of this file on the MI355X (profiles/r29_tactile_normal_equations.md, the table per case); the bounds are 10 x
MEASURED = {F64: 5.071e-16, F32: 5.984e-6}      # fp64: pusher (B = 5, T = 3; 2 ulp of an entry); fp32: tactile_pad (40 000 taxels, the long sum)
MEASURED_FD = 2.336e-12      # yardstick B, the largest of the three cases (bound: 1e-3)
CAP = {F64: 1e-10, F32: 1e-4}
BOUND = {dt: min(CAP[dt], 10 * MEASURED[dt]) for dt in MEASURED}
STATS = os.environ.get("TSIM_TACTILE_NORMAL_STATS")      # a file: every case's largest errors are appended to it (the profile)


@pytest.fixture(scope="module")
def pad_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("tn_pads")


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


def _nsensor(m):
    return int(m.I[Bl.TSIM_IH_NSENSOR])


def _draw(sim, nm, seed=17):
    """w [ntac] in [1, 100] (log-uniform) and r [nm, B, ntac] (normal), in the batch's type"""
    rng = np.random.default_rng(seed)
    w = _t(10.0 ** rng.uniform(0, 2, size=sim.ndof_tactile), sim.dtype)
    r = _t(rng.normal(size=(nm, sim.B, sim.ndof_tactile)), sim.dtype)
    return w, r


def _poison(sim, nm, Z):
    """(the allocator's next blocks of the outputs' shapes are NaN)"""
    torch.full((nm, sim.B, Z, Z), float("nan"), device=DEV, dtype=sim.dtype)
    torch.full((nm, sim.B, Z), float("nan"), device=DEV, dtype=sim.dtype)


def _call(sim, T, S, w, r, wp, mask=None):
    nm = T if mask is None else int(mask.sum())
    Z = 2 * sim.ndof_r + (4 * _nsensor(sim.model) if wp else 0)
    _poison(sim, nm, Z)
    o = sim.tactile_normal_equations(T, S, weight=w, residual=r, with_params=wp, tactile_mask=mask)
    assert tuple(o["N"].shape) == (nm, sim.B, Z, Z) and (("n" in o) == (r is not None))
    assert bool(torch.isfinite(o["N"]).all()), "an entry of N was not written"
    if r is not None:
        assert tuple(o["n"].shape) == (nm, sim.B, Z) and bool(torch.isfinite(o["n"]).all()), "an entry of n was not written"
    assert torch.equal(o["N"], o["N"].transpose(-1, -2)), "N is not bit-symmetric"
    return o


def _reference(sim, m, T, S, w, r, mask=None):
    """yardstick A: (N, S_N, n, S_n) in float64 from tactile_jacobians' Ct and param_jacobians' Ft of the same batch and tape"""
    Ct = sim.tactile_jacobians(T, S, mask)
    Ft = sim.param_jacobians(T, S, (), want_E=False, want_tactile=True, tactile_mask=mask)["Ft"]
    H = torch.cat([Ct.transpose(-1, -2), TN.dense_F(Ft, TN.sensor_ranges(m))], -1).double()
    wd = torch.ones(sim.ndof_tactile, device=DEV, dtype=F64) if w is None else w.double()
    return TN.reference(H, wd, None if r is None else r.double())


def _errors(got, ref, scale):
    """largest |got - ref| / scale; exactly 0 is asserted where the scale is 0"""
    diff = (got.double() - ref).abs()
    assert bool((got[scale == 0] == 0).all()), "an entry whose scale is zero is not exactly zero"
    return float((diff / scale.clamp_min(1e-300))[scale > 0].max()) if bool((scale > 0).any()) else 0.0


def _assert_shape(sim, m, lanes, rows, wp):
    """k_tactile_normal's launch is the restated plan's: lanes per environment, LDS bytes, blocks per frame, exactly"""
    env = int(os.environ.get("TSIM_LPE", "0"))
    forced = lanes or (env if env in (16, 32, 64) else 0)
    n_simd = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    want = TN.tactile_normal_shape(m, forced, 8 if sim.dtype == F64 else 4, wp, rows, sim.B, n_simd, sim.kernel_variant() != "generic")
    fl = sim.tactile_normal_equations_launch_info(wp)
    assert (fl["lanes_per_env"], fl["lds_bytes"], fl["lds_bytes"] <= 64 * 1024) == want[:3] and fl["threads"] == 64, (forced, fl, want)
    assert fl["blocks"] == -(-sim.B // (64 // fl["lanes_per_env"]))
    return fl


def _check(name, case, dtype, lanes=0, static=False, rows=True, mask=None, expect_variant=None, ones=False):
    """one case against yardstick A, with parameters and a residual; then the same frames without parameters and without a residual, bit for bit.
    ones: the weight is None (W = I).  Returns (sim, o, model)"""
    m, q0, qd0, u, S = case
    B, T = u.shape[0], u.shape[1]
    sim = PU.make_sim(m, B, dtype, T * S, lanes=lanes, static=static)
    tab = PU.table_rows(m, B, dtype == F32, 11) if rows else None
    _roll(sim, tab, q0, qd0, u, S, mask)
    if expect_variant:
        assert sim.kernel_variant() == expect_variant
    fl = _assert_shape(sim, m, lanes, rows, True)
    nm = T if mask is None else int(mask.sum())
    w, r = _draw(sim, nm)
    if ones:
        w = None
    o = _call(sim, T, S, w, r, True, mask)
    N, SN, n, Sn = _reference(sim, m, T, S, w, r, mask)
    eN, en = _errors(o["N"], N, SN), _errors(o["n"], n, Sn)
    _stat("A %-28s %s lanes %2d (kernel at %2d) static %d rows %d w %d: N %.3e n %.3e nonzero %d" % (
        name, "f64" if dtype == F64 else "f32", lanes, fl["lanes_per_env"], static, rows, not ones, eN, en, int((o["N"] != 0).sum())))
    assert MEASURED[dtype] < CAP[dtype]
    assert eN <= BOUND[dtype] and en <= BOUND[dtype], (name, eN, en)
    # positive semi-definite to round-off (w > 0)
    Nd = o["N"].double()
    ev = torch.linalg.eigvalsh(Nd.cpu())
    tr = torch.diagonal(Nd, dim1=-2, dim2=-1).sum(-1).cpu()
    assert bool((ev[..., 0] >= -CAP[dtype] * tr).all()), (name, "not positive semi-definite", float(ev.min()))
    # the state block with and without parameters, with and without a residual
    xs = 2 * sim.ndof_r
    a = _call(sim, T, S, w, r, False, mask)
    assert torch.equal(a["N"], o["N"][..., :xs, :xs]) and torch.equal(a["n"], o["n"][..., :xs]), (name, "the state block depends on with_params")
    assert torch.equal(_call(sim, T, S, w, None, True, mask)["N"], o["N"]), (name, "N depends on the residual")
    assert torch.equal(_call(sim, T, S, w, None, False, mask)["N"], a["N"])
    assert sim.tape_len() == T * S
    return sim, o, m


def _param_blocks(o, m, xs):
    """[nm, B, nsensor, nsensor, 4, 4]: the blocks between the sensors' parameter columns"""
    ns = _nsensor(m)
    Pb = o["N"][..., xs:, xs:]
    return Pb.reshape(Pb.shape[0], Pb.shape[1], ns, 4, ns, 4).permute(0, 1, 2, 4, 3, 5)


# ---------------------------------------------------------------------------------------------------- 1. the fixed models
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [0, 16, 32, 64])
def test_pusher_at_every_launch_shape(lanes, dtype):
    """B = 5 (ragged at 4 and 2 per wavefront), T = 3, per-environment rows; the library's shape and 16 / 32 / 64 forced lanes (fp64 at 16 forced
    lanes runs at 32: four contexts are over the cap)"""
    sim, o, m = _check("pusher", tangent_case("pusher", 5), dtype, lanes=lanes)
    assert bool((o["N"] != 0).any()) and bool((o["n"] != 0).any())


@pytest.mark.parametrize("dtype,rows,variant", [(F32, False, "static:pusher"), (F32, True, "param:pusher"), (F64, False, "static:pusher")])
def test_on_a_compiled_in_model_batch(dtype, rows, variant):
    """the generic k_tactile_normal over the tape a static:pusher / param:pusher batch recorded, held to the Jacobians of that very tape"""
    if dtype == F64 and os.environ.get("TSIM_LPE") == "16":
        variant = "generic"
    _check("pusher", tangent_case("pusher", 5), dtype, static=True, rows=rows, expect_variant=variant)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_masked_frames_of_a_ragged_pusher_batch(dtype):
    """pusher, B = 5, T = 3, mask [1, 0, 1]: the output slot follows the mask"""
    mask = torch.tensor([True, False, True])
    sim, o, m = _check("pusher mask101", tangent_case("pusher", 5), dtype, mask=mask)
    w, _ = _draw(sim, 3)
    full = _call(sim, T_FRAMES, 5, w, None, True)["N"]
    assert torch.equal(o["N"][0], full[0]) and torch.equal(o["N"][1], full[2]) and not torch.equal(full[1], full[2])


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["pusher", "small_130_4x2", "dclaw_position_control"])
def test_without_a_weight_w_is_the_identity(name, dtype, pad_dir):
    case = TC.pad_case(name, pad_dir, 4) if name in P.TABLE else tangent_case(name, 3)
    _check(name + " w=None", case, dtype, ones=True)


# ---------------------------------------------------------------------------------------------------- 2. the pads: tails, primitives, sensors
ADJ_NT = (1, 15, 16, 17, 63, 64, 65, 129)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("nt", ADJ_NT)
def test_taxel_chunks_on_the_pads(nt, lanes, dtype, pad_dir):
    """adj_<nt>: one sensor of nt taxels over the slab — the trip loop's tails (nt = lanes k - 1, + 1), its second and third trips, and the
    product pass's row tail; the lifted environment (3) loads nothing: all zeros"""
    name = "adj_%d" % nt
    sim, o, m = _check(name, TC.pad_case(name, pad_dir, 4), dtype, lanes=lanes)
    assert bool((o["N"][0, :3] != 0).any())
    assert bool((o["N"][0, 3] == 0).all()) and bool((o["n"][0, 3] == 0).all())


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("combo", P.SMALL_COMBOS)
def test_sensors_and_primitives_on_the_pads(combo, lanes, dtype, pad_dir):
    """small_130_<sensors>x<primitives>: 1x8 and 2x4 sum a taxel's row over the primitives before the product; with several sensors the blocks
    between two sensors' parameter columns are exactly zero and the diagonal ones are not"""
    name = "small_130_%dx%d" % combo
    sim, o, m = _check(name, TC.pad_case(name, pad_dir, 4), dtype, lanes=lanes)
    blk = _param_blocks(o, m, 2 * sim.ndof_r)
    ns = combo[0]
    for s in range(ns):
        for t in range(ns):
            if s != t:
                assert bool((blk[:, :, s, t] == 0).all()), (name, s, t)
    assert bool((blk[0, :3].diagonal(dim1=1, dim2=2) != 0).any())
    if ns > 1:
        assert sum(bool((blk[0, :3, s, s] != 0).any()) for s in range(ns)) > 1      # more than one sensor is loaded


@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_blind_sensor_and_its_neighbours(dtype, pad_dir):
    """large_300_blind_725: the sensor without primitives has exactly zero parameter rows and columns, its neighbours have not"""
    name = "large_300_blind_725"
    sim, o, m = _check(name, TC.pad_case(name, pad_dir, 4), dtype)
    xs = 2 * sim.ndof_r
    blind = [s for s, (_, _, nsp) in enumerate(TN.sensor_ranges(m)) if nsp == 0]
    seeing = [s for s, (_, _, nsp) in enumerate(TN.sensor_ranges(m)) if nsp > 0]
    assert len(blind) == 1 and int((~P.paired_taxels(m)).sum()) == 7 and len(seeing) >= 2
    N = o["N"]
    for s in blind:
        c = slice(xs + 4 * s, xs + 4 * s + 4)
        assert bool((N[..., c, :] == 0).all()) and bool((N[..., :, c] == 0).all()) and bool((o["n"][..., c] == 0).all())
    for s in seeing:
        c = slice(xs + 4 * s, xs + 4 * s + 4)
        assert bool((N[..., c, c] != 0).any())


@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_bdf2_pad(dtype, pad_dir):
    m = P.pad_model(os.path.join(str(pad_dir), "bdf2_130_4x2"), P.split(130, 4), 2, integrator="BDF2")
    st = P.states(m, 0, "mixed", 3) + P.states(m, 1, "all_out", 1)
    q0, qd0 = np.stack([s[0] for s in st]), np.stack([s[1] for s in st])
    u = np.tile(TC.PAD_U[None, None], (4, 2, 1))
    _check("bdf2_130_4x2", (m, q0, qd0, u, 2), dtype)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["small_130_1x1", "small_130_4x2"])
def test_four_pad_environments_per_wavefront_on_the_shared_model(name, dtype, pad_dir):
    """without per-environment rows four fp64 contexts of a pad fit the block: fp64 at 16 lanes, where the block does"""
    _check(name, TC.pad_case(name, pad_dir, 5), dtype, lanes=16, rows=False)


# ---------------------------------------------------------------------------------------------------- 3. the other models
@pytest.mark.parametrize("dtype", [F64, F32])
def test_bdf2_ball_push_with_a_rotation_vector_joint(dtype):
    sim, o, m = _check("bdf2:ball_push", tangent_case("bdf2:ball_push", 5), dtype)
    assert bool((o["N"] != 0).any())


@pytest.mark.parametrize("dtype", [F64, F32])
def test_the_tactile_pad_of_120000_values(dtype):
    """assets' tactile_pad: B = 2, T = 1 — the EXPJ instantiation, BDF2, 40 000 taxels: 625 trips, the long accumulation"""
    m, q0, qd0, u, S = PU.case("tactile_pad", 2, 1)
    sim, o, m = _check("tactile_pad B2 T1", (m, q0, qd0, u, S), dtype)
    assert sim.ndof_tactile == 120000 and bool((o["N"] != 0).any())


@pytest.mark.parametrize("dtype", [F64, F32])
def test_dclaw_three_sensors(dtype):
    """D'Claw: B = 3, T = 1; Z = 32"""
    m, q0, qd0, u, S = tangent_case("dclaw_position_control", 3)
    sim, o, m = _check("dclaw B3 T1", (m, q0, qd0, u[:, :1], S), dtype)
    assert o["N"].shape[-1] == 32 and bool((o["N"] != 0).any())
    blk = _param_blocks(o, m, 2 * sim.ndof_r)
    for s in range(3):
        for t in range(3):
            if s != t:
                assert bool((blk[:, :, s, t] == 0).all())


@pytest.mark.parametrize("dtype", [F64, F32])
def test_tactile_insertion_two_pads(dtype):
    m, q0, qd0, u, S = tangent_case("tactile_insertion", 3)
    _check("tactile_insertion B3", (m, q0, qd0, u[:, :2], S), dtype)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [16, 32, 64])
def test_wide_model_at_every_launch_shape(lanes, dtype):
    """tests/wide_models.py wide9: 9 dofs on few links — NRM 16"""
    _check("wide9", W.wide_case("wide9", 5, T_FRAMES), dtype, lanes=lanes)


# ---------------------------------------------------------------------------------------------------- 4. yardstick B
@pytest.mark.parametrize("name", list(READOUT_DRAW_USED))
def test_quadratic_forms_against_differences_of_the_read_out_map(name, pad_dir):
    """v^T N v against sum_i w_i fd_i^2 and v^T n against sum_i w_i fd_i r_i (fp64), fd the Richardson differences of the oracle's read-out map
    at the last frame's end state along the yardstick's pinned draw; the pads' borderline taxels get weight 0"""
    import copy
    if name in PAD_CASES:
        m, q0, qd0, u, S = TC.pad_case(PAD_CASES[name], pad_dir, 1)
    else:
        m, q0, qd0, u, S = tangent_case(name, 1)
    m = copy.deepcopy(m)
    m.F[Bl.TSIM_FH_TOL] = 1e-13
    T = u.shape[1]
    sim = PU.make_sim(m, 1, F64, T * S)
    _roll(sim, None, q0, qd0, u, S)
    q1, qd1 = oracle_frame_states(m, q0[0], qd0[0], u[0], S)[T]
    fd, v, used = readout_difference(m, q1, qd1, name)
    assert used == READOUT_DRAW_USED[name] and np.any(fd != 0)
    keep = np.repeat(TC.pad_keep(m, q1, qd1)[1] if name in PAD_CASES else np.ones(m.ndof_tactile // 3, bool), 3)
    rng = np.random.default_rng(23)
    w = 10.0 ** rng.uniform(0, 2, size=m.ndof_tactile) * keep
    r = rng.normal(size=m.ndof_tactile)
    mask = torch.zeros(T, dtype=torch.bool)
    mask[T - 1] = True
    o = _call(sim, T, S, _t(w, F64), _t(r[None, None], F64), False, mask)
    N, n = o["N"][0, 0].cpu().numpy(), o["n"][0, 0].cpu().numpy()
    qN, refN = float(v @ N @ v), float(np.sum(w * fd * fd))
    qn, refn, scn = float(v @ n), float(np.sum(w * fd * r)), float(np.sum(w * np.abs(fd) * np.abs(r)))
    eN, en = abs(qN - refN) / refN, abs(qn - refn) / scn
    _stat("B %s: |v^T N v - sum w fd^2| / sum w fd^2 = %.3e, |v^T n - sum w fd r| / sum w |fd| |r| = %.3e" % (name, eN, en))
    assert refN > 0 and eN <= 1e-3 and en <= 1e-3, (name, eN, en)


# ---------------------------------------------------------------------------------------------------- 5. exact structure
@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_frame_with_no_loaded_taxel_is_all_zeros(dtype):
    """the pusher at rest before contact, no control: on the oracle nothing is loaded at the frame's end — N and n are exactly zero"""
    from oracle.oracle import OracleSim
    m, q0, qd0, u, S = tangent_case("pusher", 2)
    qd0, u = 0 * qd0, 0 * u[:, :1]
    for e in range(2):
        q1, qd1 = oracle_frame_states(m, q0[e], qd0[e], u[e], S)[1]
        assert not TC.loaded_taxels(OracleSim(m), q1, qd1).any()
    sim = PU.make_sim(m, 2, dtype, S)
    _roll(sim, None, q0, qd0, u, S)
    w, r = _draw(sim, 1)
    o = _call(sim, 1, S, w, r, True)
    assert bool((o["N"] == 0).all()) and bool((o["n"] == 0).all())


# ---------------------------------------------------------------------------------------------------- 6. per-environment tables
@pytest.mark.parametrize("dtype", [F64, F32])
def test_two_environments_that_differ_in_one_sensors_kn(dtype, pad_dir):
    """each environment equals the shared-model batch of its row, bit for bit, and the two differ"""
    name, B = "small_130_4x2", 2
    m, q0, qd0, u, S = TC.pad_case(name, pad_dir, B)
    q0, qd0, u = np.repeat(q0[:1], B, 0), np.repeat(qd0[:1], B, 0), np.repeat(u[:1], B, 0)      # the same state: only the table differs
    n = int(m.I[Bl.TSIM_IH_FOFF_CPT])
    tab = np.tile(np.asarray(m.F[:n], dtype=np.float64), (B, 1))
    col = int(m.I[Bl.TSIM_IH_FOFF_SENSOR]) + 1 * Bl.TSIM_SF_SIZE + Bl.TSIM_SF_KN      # sensor 1's kn
    tab[1, col] *= 1.25
    tab = tab.astype(np.float32 if dtype == F32 else np.float64)
    sim = PU.make_sim(m, B, dtype, S)
    _roll(sim, tab, q0, qd0, u, S)
    lanes = sim.launch_info()["lanes_per_env"]
    w, r = _draw(sim, 1)
    o = _call(sim, 1, S, w, r, True)
    for e in range(B):
        one = PU.make_sim(PU.row_model(m, tab[e].astype(np.float64)), B, dtype, S, lanes=lanes)
        _roll(one, None, q0, qd0, u, S)
        oe = _call(one, 1, S, w, r, True)
        assert torch.equal(oe["N"][:, e], o["N"][:, e]) and torch.equal(oe["n"][:, e], o["n"][:, e]), e
    assert not torch.equal(o["N"][:, 0], o["N"][:, 1])


# ---------------------------------------------------------------------------------------------------- 7. invariances
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["pusher", "dclaw_position_control"])
def test_a_frames_bits_do_not_depend_on_the_window_the_mask_or_the_batch(name, dtype):
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case(name, B)
    q0 = q0 + 1e-4 * np.random.default_rng(5).normal(size=q0.shape)         # (environments that differ)
    tab = PU.table_rows(m, B, dtype == F32, 11)
    sim = PU.make_sim(m, B, dtype, T * S)
    _roll(sim, tab, q0, qd0, u, S)
    w, r = _draw(sim, T)
    full = _call(sim, T, S, w, r, True)
    eq = lambda a, N, n: torch.equal(a["N"], N) and torch.equal(a["n"], n)      # noqa: E731
    assert eq(_call(sim, T - 1, S, w, r[1:].contiguous(), True), full["N"][1:], full["n"][1:])           # the newest 2 of 3 frames
    assert eq(_call(sim, T, S, w, r[1:2].contiguous(), True, torch.tensor([False, True, False])), full["N"][1:2], full["n"][1:2])
    assert eq(_call(sim, T, S, w, r[[0, 2]].contiguous(), True, torch.tensor([True, False, True])), full["N"][[0, 2]], full["n"][[0, 2]])
    lanes = sim.tactile_normal_equations_launch_info(True)["lanes_per_env"]
    one = PU.make_sim(m, 1, dtype, T * S, lanes=sim.launch_info()["lanes_per_env"])
    _roll(one, tab[4:], q0[4:], qd0[4:], u[4:], S)
    assert one.tactile_normal_equations_launch_info(True)["lanes_per_env"] == lanes
    o1 = _call(one, T, S, w, r[:, 4:].contiguous(), True)
    assert torch.equal(o1["N"][:, 0], full["N"][:, 4]) and torch.equal(o1["n"][:, 0], full["n"][:, 4])      # B = 1 against position 4 of 5
    assert bool((full["N"][:, 4] != full["N"][:, 3]).any())


# ---------------------------------------------------------------------------------------------------- 8. read-only, capturable, small
@pytest.mark.parametrize("static,rows,variant", [(False, True, "generic"), (True, False, "static:pusher")])
def test_tactile_normal_launches_change_nothing(static, rows, variant):
    """roll-out -> 0 or 2 launches -> the adjoint, bit for bit"""
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    res = []
    for ntn in (0, 2):
        sim = PU.make_sim(m, B, F32, T * S, static=static)
        out = _roll(sim, PU.table_rows(m, B, True, 11) if rows else None, q0, qd0, u, S)
        assert sim.kernel_variant() == variant
        for i in range(ntn):
            w, r = _draw(sim, T - i)
            _call(sim, T - i, S, w, r, True)
        assert sim.tape_len() == T * S and sim.last_adjoint_launch()["kernel"] is None
        st = sim.get_state()
        rng = np.random.default_rng(52)
        ws = [_t(rng.normal(size=(T, B, d)), F32) for d in (sim.ndof_r, sim.ndof_var, sim.ndof_tactile)]
        du = sim.backward_episode(T, S, ws[0], ws[1], ws[2])
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
    w, r = _draw(sim, T)
    eager = _call(sim, T, S, w, r, True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sim.tactile_normal_equations(T, S, w, r, True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a = sim.tactile_normal_equations(T, S, w, r, True)
    a["N"].fill_(7.0)
    a["n"].fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a["N"], eager["N"]) and torch.equal(a["n"], eager["n"]) and sim.tape_len() == T * S


def test_the_call_allocates_its_outputs_and_nothing_else():
    """the point of the feature: the peak over the call rises by the outputs' own bytes (each rounded up to the allocator's 512), not by Ct"""
    B, T = 64, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    sim = PU.make_sim(m, B, F32, T * S)
    _roll(sim, None, q0, qd0, u, S)
    w, r = _draw(sim, T)
    sim.tactile_normal_equations(T, S, w, r, True)      # (warm: the library is loaded, the kernel's code object is on the device)
    torch.cuda.synchronize()
    Z = 2 * sim.ndof_r + 4
    r512 = lambda n: -(-n // 512) * 512      # noqa: E731
    own = r512(T * B * Z * Z * 4) + r512(T * B * Z * 4)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    o = sim.tactile_normal_equations(T, S, w, r, True)
    peak = torch.cuda.max_memory_allocated()
    assert peak - base <= own, (peak - base, own)
    assert own < T * B * 2 * sim.ndof_r * sim.ndof_tactile * 4 // 10      # ... which Ct alone is over ten times
    del o


# ---------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals():
    from tactilesimulation_amd.host import capi
    B, T = 5, T_FRAMES
    m, q0, qd0, u, S = tangent_case("pusher", B)
    sim = PU.make_sim(m, B, F64, T * S)
    L = capi.lib()
    Z = 2 * sim.ndof_r + 4
    N = torch.full((T + 1, B, Z, Z), 7.0, device=DEV, dtype=F64)
    n = torch.full((T + 1, B, Z), 7.0, device=DEV, dtype=F64)
    r = torch.zeros((T + 1, B, sim.ndof_tactile), device=DEV, dtype=F64)

    def call(h, nf, ns, N_=N.data_ptr(), r_=r.data_ptr(), n_=n.data_ptr()):
        return L.tsim_tactile_normal_equations(h, nf, ns, None, 1, None, r_, N_, n_, None)
    sim.kernel_timing(True)
    assert call(None, T, S) != 0 and b"null batch" in L.tsim_last_error()
    sim.reset(_t(q0, F64), None, backward_flag=True)
    assert call(sim._h, T, S) != 0 and b"no tape" in L.tsim_last_error()
    _roll(sim, None, q0, qd0, u, S)
    sim.kernel_times()
    assert call(sim._h, T, S, None) != 0 and b"null N_out" in L.tsim_last_error()
    assert call(sim._h, T, S, r_=None) != 0 and b"go together" in L.tsim_last_error()
    assert call(sim._h, T, S, n_=None) != 0 and b"go together" in L.tsim_last_error()
    for nf, ns in ((0, S), (T, 0), (-1, S)):
        assert call(sim._h, nf, ns) != 0 and b"must be positive" in L.tsim_last_error()
    assert call(sim._h, T + 1, S) != 0 and b"sub-steps on the tape" in L.tsim_last_error()
    # the Python layer, before any call into C
    w = torch.ones(sim.ndof_tactile, device=DEV, dtype=F64)
    rr = r[:T]
    with pytest.raises(ValueError, match="no masked frame"):
        sim.tactile_normal_equations(T, S, tactile_mask=torch.zeros(T, dtype=torch.bool))
    for bad in (w[:-1], w.float(), w.cpu(), w.repeat(2)[::2], w[None]):
        with pytest.raises(ValueError, match="weight"):
            sim.tactile_normal_equations(T, S, weight=bad)
    for bad in (rr[:, :, :-1], rr[:-1], rr.float(), rr.cpu(), torch.zeros((T, B, 2 * sim.ndof_tactile), device=DEV, dtype=F64)[:, :, ::2]):
        with pytest.raises(ValueError, match="residual"):
            sim.tactile_normal_equations(T, S, residual=bad)
    mb, q0b, qd0b, ub, Sb = tangent_case("box_slide", B)                     # a model without taxels
    simb = PU.make_sim(mb, B, F64, T * Sb)
    _roll(simb, None, q0b, qd0b, ub, Sb)
    assert call(simb._h, T, Sb) != 0 and b"no taxels" in L.tsim_last_error()
    with pytest.raises(RuntimeError):
        simb.tactile_normal_equations(T, Sb)
    assert L.tsim_tactile_normal_equations_launch_info(None, 1, (ctypes.c_int32 * 4)()) != 0
    torch.cuda.synchronize()
    assert all(k == 0 for _, k in sim.kernel_times().values())               # nothing was launched on the batch's timed kinds ...
    assert bool((N == 7).all()) and bool((n == 7).all())                      # ... and nothing was written
    # a device mask without a masked frame, which the C entry cannot see: every block returns at once, nothing is written
    none = torch.full((T,), -1, device=DEV, dtype=torch.int32)
    assert L.tsim_tactile_normal_equations(sim._h, T, S, none.data_ptr(), 1, None, r.data_ptr(), N.data_ptr(), n.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((N == 7).all()) and bool((n == 7).all())
    # a valid launch after the refusals still gives the right answer
    wd, rd = _draw(sim, T)
    o = _call(sim, T, S, wd, rd, True)
    Nr, SN, nr_, Sn = _reference(sim, m, T, S, wd, rd)
    assert _errors(o["N"], Nr, SN) <= BOUND[F64] and _errors(o["n"], nr_, Sn) <= BOUND[F64]


# ---------------------------------------------------------------------------------------------------- 10. launch shape
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("lanes", [0, 16, 32, 64])
@pytest.mark.parametrize("name", ["pusher", "pad_press", "dclaw_position_control", "tactile_insertion", "wide9", "wide10"])
def test_the_launch_shape_is_the_restated_plan(name, lanes, dtype):
    m = W.wide_model(name) if name in W.WIDE else tangent_case(name, 1)[0]
    for B, rows in ((5, True), (3, False)):
        sim = PU.make_sim(m, B, dtype, 2, lanes=lanes)
        if rows:
            sim.set_env_tables(_t(PU.table_rows(m, B, dtype == F32, 11), dtype))
        for wp in (False, True):
            fl = _assert_shape(sim, m, lanes, rows, wp)
            assert fl["lanes_per_env"] >= sim.launch_info()["lanes_per_env"] and fl["lds_bytes"] <= 64 * 1024      # none of these is refused


def test_the_16_dof_corpus_model_with_taxels_is_refused_in_fp64_and_runs_in_fp32():
    """large:L3 (16 dofs, 5 taxels): the fp64 block is over the cap — refused, nothing written; large:L2 (no taxels) is refused for that.  In fp32
    L3 launches, at 32 taxels per trip of its 64 lanes"""
    from tactilesimulation_amd.host import capi
    L = capi.lib()
    m, q0, qd0, u, S = PU.case("large:L3", 1)
    B, T = 2, 1
    q0, qd0, u = np.repeat(q0, B, 0), np.repeat(qd0, B, 0), np.repeat(u, B, 0)[:, :T]
    for dtype in (F64, F32):
        sim = PU.make_sim(m, B, dtype, T * S)
        _roll(sim, None, q0, qd0, u, S)
        fl = _assert_shape(sim, m, 0, False, True)
        if dtype == F64:
            assert fl["lds_bytes"] == 68928
            N = torch.full((T, B, 36, 36), 7.0, device=DEV, dtype=F64)
            assert L.tsim_tactile_normal_equations(sim._h, T, S, None, 1, None, None, N.data_ptr(), None, None) != 0 and b"do not fit" in L.tsim_last_error()
            torch.cuda.synchronize()
            assert bool((N == 7).all())
        else:
            _check("large:L3", (m, q0, qd0, u, S), F32, rows=False)


# ---------------------------------------------------------------------------------------------------- 11. functions.episode_information
@pytest.mark.parametrize("name", ["pusher", "small_130_4x2"])
def test_episode_information_gathers_the_callers_columns(name, pad_dir):
    """(N, n) over (x, p[cols]) in the caller's order against the einsum of episode_observation's C and episode_parameters' F of the same columns;
    pair and dof-damping columns: exactly zero rows and columns"""
    from tactilesimulation_amd.functions import episode_information, episode_observation, episode_parameters
    B = 3
    m, q0, qd0, u, S = TC.pad_case(name, pad_dir, B) if name in P.TABLE else tangent_case(name, B)
    T = u.shape[1]
    sim = PU.make_sim(m, B, F64, T * S)
    _roll(sim, None, q0, qd0, u, S)
    pc = m.param_columns()
    sensor = [c for k, _, _, c in pc if k == "sensor"]
    pair = [c for k, _, _, c in pc if k == "pair"]
    dof = [c for k, _, _, c in pc if k == "dof"]
    cols = [sensor[-1], pair[0], sensor[0], dof[0], sensor[1]]      # out of order, mixed kinds
    w, r = _draw(sim, T)
    N, n = episode_information(sim, T, S, weight=w, residual=r, cols=cols)
    xs = 2 * sim.ndof_r
    assert tuple(N.shape) == (T, B, xs + len(cols), xs + len(cols)) and tuple(n.shape) == (T, B, xs + len(cols))
    C = episode_observation(sim, T, S)
    E, F = episode_parameters(sim, T, S, cols)
    assert E.shape[-1] == len(cols)
    H = torch.cat([C, F], -1).double()
    Nr, SN, nr_, Sn = TN.reference(H, w.double(), r.double())
    assert _errors(N, Nr, SN) <= BOUND[F64] and _errors(n, nr_, Sn) <= BOUND[F64]
    assert torch.equal(N, N.transpose(-1, -2))
    for k in (1, 3):      # the pair and the dof-damping column
        assert bool((N[..., xs + k, :] == 0).all()) and bool((N[..., :, xs + k] == 0).all()) and bool((n[..., xs + k] == 0).all())
    assert bool((N[..., xs + 2, xs + 2] != 0).any())
    N0, n0 = episode_information(sim, T, S, weight=w)      # no columns: the state block alone, no n
    assert n0 is None and torch.equal(N0, N[..., :xs, :xs])
    with pytest.raises(ValueError, match="not a contact-group parameter"):
        episode_information(sim, T, S, cols=[0])
