"""The tactile read-out at every pad-shape edge of its four pieces of HIP, against the fp64 oracle and against each other.

Tactile frames come out of the in-kernel readout() (csrc/tsim_kernels.h), k_taxels_small, and the list and the general branch of k_taxels
(csrc/tsim_hip.hip); the host picks one from the pad's shape (launch_taxels, launch_forward, tsim_readout).  The reference models reach a few
of these shapes only; the synthetic pads of tests/pad_models.py (checked on the CPU by tests/test_pad_models.py) reach the rest: chunk tails, full
and empty lists, ragged blocks that span frames and masked slots, per-environment tables, slice and sensor boundaries, and the switches
1024/1025 taxels, 8/9 combinations, 4/5 sensors, 63/64 records, 4095/4096 taxels, 64/65 combinations, 16/17 sensors and primitives.

Every case evaluates the same states through every route that can take them:
  1  reset, then readout() with and without the variables (k_readout + a taxel kernel);
  2  one step, or a rollout of T frames, with the default deferred read-out;
  3  the same on a batch created under TSIM_INKERNEL_READOUT=1;
  4  the same on a batch created under TSIM_TAXELS_PER_RECORD=1 (never k_taxels_small);
and asserts (a) per frame, max |tac - oracle| / max |oracle| over the taxels that are not borderline (tests/pad_models.py: loaded / unloaded changes
within 1e-6 m; at most 1 % of a frame's taxels, or the case fails) within TOL, and the set of loaded taxels equal to the oracle's; (b) bit
equality between the routes through the taxel kernels always, and with the in-kernel route where no sensor has more than TS_PAIR_GROUP = 4
primitives (beyond that the in-kernel route sums projected outputs per staging group: round-off, bounded by TOL; include/tsim.h says so).
Every case restates the host's dispatch from its sizes and asserts that it reached the kernel it is for, with the taxel launches counted
through tsim_kernel_times.  A case that compares only zeros fails.  The adjoint of the tactile outputs (vjp_taxels) at its chunk edges is
at the end of the file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pad_models as P      # noqa: E402
from _report import rep as _rep      # noqa: E402
from param_grad_util import row_model      # noqa: E402
import tactilesimulation_amd.model.blob as Bl      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
# Bounds on max |tac - oracle| / max |oracle| per frame: 10 x the maximum measured over this file on the MI355X, never looser than the project's
# standing rules (1e-8 fp64, 1e-4 fp32).  Measured (profiles/r16_tactile_readout_shapes.md, 110 cases per precision, every route and frame):
# fp64 max 1.12e-13 (the grazing sphere; every other group <= 1.7e-14), median 4.8e-15; fp32 max 4.19e-5 (the cuboid's corner; the other groups
# <= 2.9e-5), 90 % below 2.5e-5, median 1.2e-5 — ten times that is past the standing 1e-4, which therefore is the fp32 bound.
TOL = {F64: 1.2e-12, F32: 1e-4}
# ... and of the tactile adjoint (dL/du and the carried adjoint against OracleSim.backward_steps + adjoint()): tests/test_gpu_bdf2_adjoint.py's.
# Measured maxima: fp64 6.7e-15, fp32 1.2e-5 (carried position adjoint; dL/du 6.1e-6)
TOL_ADJ = {F64: 1e-7, F32: 2e-4}
ENVS = ("TSIM_INKERNEL_READOUT", "TSIM_TAXELS_PER_RECORD", "TSIM_NO_FREE_RUN", "TSIM_LOCKSTEP")


@pytest.fixture(scope="module")
def pad_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("pads")


# ---------------------------------------------------------------------------------------------------- the host's dispatch, restated
def expected_kernel(ntax, nsensor, nspt, nrec, per_record=False, inkernel=False):
    """which piece of HIP writes the tactile frames of a launch with nrec = frames x B records (csrc/tsim_hip.hip launch_forward, launch_taxels)"""
    if inkernel or nspt > 64 or nsensor > 16:
        return "inkernel"
    if nrec >= 64 and ntax <= 1024 and nspt <= 8 and nsensor <= 4 and not per_record:
        return "small"
    return "list" if nsensor == 1 and nspt == 1 else "general"


# ---------------------------------------------------------------------------------------------------- the oracle's frames
_ORACLE = {}


def oracle_frames(key, m, q, qd, U):
    """[(tac [3 ntax], loaded [ntax], borderline [ntax])] at (q, qd) and after each frame of U [T, nu] (one sub-step per frame), cached under key"""
    if key not in _ORACLE:
        from oracle.oracle import OracleSim
        o = OracleSim(m)
        o.reset(q, qd)
        out = []
        for t in range(len(U) + 1):
            if t:
                assert o.forward(U[t - 1], 1) == 0, "the oracle's sub-step did not converge"
            qt, qdt = o.state()
            out.append((o.outputs()[1].copy(), P.loaded(o, qt, qdt), P.borderline(o, qt, qdt)))
        _ORACLE[key] = out
    return _ORACLE[key]


def env_row(m, dtype, seed):
    """[table_size] one environment's tables: the sensors' kn kt mu damping scaled by 0.8 .. 1.25, the primitives' shapes by 0.995 .. 1.005
    (a slab's top moves by up to 0.1 mm), rounded to the batch's type"""
    n = int(m.I[Bl.TSIM_IH_FOFF_CPT])
    rng = np.random.default_rng(seed)
    row = np.asarray(m.F[:n], dtype=np.float64).copy()
    for s in m.meta["sensor_names"]:
        for f in ("kn", "kt", "mu", "damping"):
            row[m.table_offset("sensor", s, f)] *= rng.uniform(0.8, 1.25)
    for key in m.meta["pair_keys"]:
        k = rng.uniform(0.995, 1.005)
        for f in ("shape0", "shape1", "shape2"):
            row[m.table_offset("pair", tuple(key), f)] *= k
    return row.astype(np.float32 if dtype == F32 else np.float64)


def _poison(*shape, dtype):
    """the block the caching allocator hands to the next output of this shape holds NaN: a taxel a kernel skips does not read as a stale result"""
    t = torch.full(shape, float("nan"), device=DEV, dtype=dtype)
    del t


# ---------------------------------------------------------------------------------------------------- one route on the GPU
def run_route(m, dtype, B, q0, qd0, U, mask, tab, env, monkeypatch):
    """reset + readout (twice), the frames (one step, or a rollout with a tactile mask), readout again (twice).  Returns the tensors and the
    number of taxel launches of each phase."""
    from tactilesimulation_amd.host.batch import BatchSim
    for k in ENVS:
        monkeypatch.delenv(k, raising=False)
    for k in env:
        monkeypatch.setenv(k, "1")
    sim = BatchSim(m, B, dtype=dtype, tape_capacity=0)
    assert sim.kernel_variant() == "generic"
    sim.kernel_timing(True)
    if tab is not None:
        sim.set_env_tables(torch.tensor(tab, device=DEV, dtype=dtype))
    T, n3 = U.shape[0], m.ndof_tactile
    sim.reset(torch.tensor(q0, device=DEV, dtype=dtype), torch.tensor(qd0, device=DEV, dtype=dtype))
    out = {"launches": {}}
    sim.kernel_times()
    try:
        _poison(B, n3, dtype=dtype)
        out["reset_var"] = sim.readout(want_var=True)[1]
        _poison(B, n3, dtype=dtype)
        out["reset"] = sim.readout(want_var=False)[1]
        out["launches"]["reset"] = sim.kernel_times()["k_taxels"][1]
    except RuntimeError as e:
        out["readout_error"] = str(e)
    Ud = torch.tensor(U, device=DEV, dtype=dtype)
    if T == 1:
        o = sim.step(Ud[0], 1, out={"tactile": torch.full((B, n3), float("nan"), device=DEV, dtype=dtype)})
        out["frames"] = o["tactile"][None]
    else:
        _poison(T if mask is None else int(mask.sum()), B, n3, dtype=dtype)
        o = sim.rollout(Ud, 1, tactile_mask=mask)
        out["frames"] = o["tactile"]
    out["launches"]["frames"] = sim.kernel_times()["k_taxels"][1]
    if "readout_error" not in out:
        _poison(B, n3, dtype=dtype)
        out["after"] = sim.readout(want_var=False)[1]        # pads of >= 4096 taxels: from the pose records the launch left (tsim_hip.hip pose_emit)
        _poison(B, n3, dtype=dtype)
        out["after_var"] = sim.readout(want_var=True)[1]     # always kinematics again
        out["launches"]["after"] = sim.kernel_times()["k_taxels"][1]
    torch.cuda.synchronize()
    return out


def compare(name, what, got, ref, dtype, stats):
    """got [F, B, 3 ntax] against ref = [frame][env] (tac, loaded, borderline): the loaded sets, the error bound, the borderline cap"""
    F_, B = got.shape[0], got.shape[1]
    ntax = got.shape[2] // 3
    tac = torch.tensor(np.stack([np.stack([ref[f][e][0] for e in range(B)]) for f in range(F_)]), device=DEV).reshape(F_, B, ntax, 3)
    ld = torch.tensor(np.stack([np.stack([ref[f][e][1] for e in range(B)]) for f in range(F_)]), device=DEV)
    bd = torch.tensor(np.stack([np.stack([ref[f][e][2] for e in range(B)]) for f in range(F_)]), device=DEV)
    assert int(bd.sum(-1).max()) <= P.BORDER_CAP * ntax, (name, what, "borderline taxels", int(bd.sum(-1).max()), ntax)
    g = got.double().reshape(F_, B, ntax, 3)
    assert bool(torch.isfinite(g).all()), (name, what, "a taxel was not written")
    keep = ~bd
    gl = (g != 0).any(-1)
    bad = (gl != ld) & keep
    assert not bool(bad.any()), (name, what, "loaded set differs from the oracle's", bad.nonzero()[:5].tolist())
    diff = ((g - tac).abs().amax(-1) * keep).amax(-1)                      # [F, B]
    scale = (tac.abs().amax(-1) * keep).amax(-1)
    err = torch.where(scale > 0, diff / scale.clamp_min(1e-300), diff)     # a frame the oracle leaves at zero has to be zero
    stats["err"] = max(stats.get("err", 0.0), float(err.max()))
    stats["errs"] = stats.get("errs", []) + err.flatten().tolist()
    stats["border"] = max(stats.get("border", 0.0), float(bd.float().mean(-1).max()))
    stats["loaded"] = stats.get("loaded", 0) + int((ld & keep).sum())
    stats["unloaded"] = stats.get("unloaded", 0) + int((~ld & keep).sum())
    assert float(err.max()) <= TOL[dtype], (name, what, float(err.max()))


def run_case(name, dtype, B, T, masked, tables, pad_dir, monkeypatch, group, want):
    """every route of one (model, launch shape), against the oracle and against each other.  want: the kernel the case is for, per route
    ("reset": the read-out after a reset, nrec = B; "default" / "inkernel" / "per_record": the frames)"""
    m = P.table_model(name, pad_dir)
    ntax, nsensor, nspt, most = P.counts(m)
    st = P.table_states(name, m)
    ns = len(st)
    rng = np.random.default_rng(17)
    Ub = rng.normal(size=(T, ns, 6)) * np.array([1e-3] * 3 + [1e-6] * 3)
    assert B >= ns                                                           # every sampled state, the lifted one included, is in the batch
    q0 = np.stack([st[e % ns][0] for e in range(B)]); qd0 = np.stack([st[e % ns][1] for e in range(B)])
    U = np.stack([Ub[:, e % ns] for e in range(B)], 1)                       # [T, B, 6]
    mask = None
    if masked:
        mask = torch.ones(T, dtype=torch.bool); mask[0] = False; mask[T // 2] = False; mask[T - 1] = False
    frames = [t for t in range(T) if mask is None or bool(mask[t])]
    nrec = T * B
    # the oracle: per environment (per distinct state without tables) the reset state and every frame.  An environment's row is drawn again while
    # a frame of its has more borderline taxels than the cap: the cap is a condition on the case, as it is on the sampled states
    ref, rows = [], []
    for e in range(B):
        if not tables:
            ref.append(oracle_frames((name, None, e % ns, T), m, q0[e], qd0[e], U[:, e]))
            continue
        for k in range(20):
            row = env_row(m, dtype, (23, e, k))
            fr = oracle_frames((name, str(dtype), e, k, B, T), row_model(m, row.astype(np.float64)), q0[e], qd0[e], U[:, e])
            if max(int(f[2].sum()) for f in fr) <= P.BORDER_CAP * ntax:
                break
        else:
            raise AssertionError("no table row within the borderline cap for environment %d of %s" % (e, name))
        ref.append(fr); rows.append(row)
    tab = np.stack(rows) if tables else None
    ref_reset = [[ref[e][0] for e in range(B)]]
    ref_frames = [[ref[e][t + 1] for e in range(B)] for t in frames]
    ref_after = [[ref[e][T] for e in range(B)]]
    # the dispatch, restated
    reach = {"reset": expected_kernel(ntax, nsensor, nspt, B), "default": expected_kernel(ntax, nsensor, nspt, nrec),
             "inkernel": "inkernel", "per_record": expected_kernel(ntax, nsensor, nspt, nrec, per_record=True)}
    for k, v in want.items():
        assert reach[k] == v, (name, k, reach[k], "the case does not reach the kernel it is for")
    stats, res = {}, {}
    for route, env in (("default", ()), ("inkernel", ("TSIM_INKERNEL_READOUT",)), ("per_record", ("TSIM_TAXELS_PER_RECORD",))):
        r = res[route] = run_route(m, dtype, B, q0, qd0, U, mask, tab, env, monkeypatch)
        if nspt > 64 or nsensor > 16:        # beyond k_taxels' staging: readout() refuses, the launches read out in-kernel
            assert "more than 64 (sensor, primitive) combinations or 16 sensors" in r["readout_error"]
            assert r["launches"]["frames"] == 0
        else:
            assert r["launches"] == {"reset": 2, "frames": 0 if route == "inkernel" else 1, "after": 2}, (name, route, r["launches"])
            for k, rf in (("reset", ref_reset), ("reset_var", ref_reset), ("after", ref_after), ("after_var", ref_after)):
                compare(name, (route, k), r[k][None], rf, dtype, stats)
            assert torch.equal(r["reset"], r["reset_var"]) and torch.equal(r["after"], r["after_var"]), (name, route)
            if T == 1 or mask is None or bool(mask[T - 1]):
                if route != "inkernel" or most <= 4:
                    assert torch.equal(r["after"], r["frames"][-1]), (name, route, "readout() after the launch is not the launch's last frame")
        compare(name, (route, "frames"), r["frames"], ref_frames, dtype, stats)
    a, b, c = res["default"], res["per_record"], res["inkernel"]
    for k in ("reset", "frames", "after"):
        if k in a:
            assert torch.equal(a[k], b[k]), (name, k, "default against TSIM_TAXELS_PER_RECORD")
            if k != "frames":
                assert torch.equal(a[k], c[k]), (name, k)
    if most <= 4:
        assert torch.equal(a["frames"], c["frames"]), (name, "in-kernel read-out against the taxel kernels")
    assert stats["loaded"] > 0 and (stats["unloaded"] > 0 or name.endswith("_slab")), (name, "nothing but zeros was compared", stats)
    assert float(a["frames"].abs().max()) > 0
    e = np.asarray(stats["errs"])
    _rep("readout_shapes", group=group, name=name, dtype=str(dtype), B=B, T=T, tables=int(tables), reset=reach["reset"], default=reach["default"],
         per_record=reach["per_record"], err_max=stats["err"], err_p50=float(np.quantile(e, 0.5)), err_p90=float(np.quantile(e, 0.9)),
         border=stats["border"], bitwise_inkernel=int(most <= 4))
    print("%s %s B=%d T=%d tables=%d: reset %s, frames %s, per-record %s; max err %.3g, borderline share %.3g"
          % (name, dtype, B, T, tables, reach["reset"], reach["default"], reach["per_record"], stats["err"], stats["border"]))
    return res


DT = [F32, F64]
ids = lambda v: str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None


# ---------------------------------------------------------------------------------------------------- the list branch of k_taxels
@pytest.mark.parametrize("dtype", DT, ids=ids)
@pytest.mark.parametrize("B,T", [(4, 1), (4, 3)])      # (four environments: one per sampled state, the lifted one included)
@pytest.mark.parametrize("prim", ["slab", "sphere"])
@pytest.mark.parametrize("ntax", P.LIST_NTAX)
def test_list_branch(ntax, prim, B, T, dtype, pad_dir, monkeypatch):
    """one sensor against one bounded primitive, nrec < 64: chunks of 2048 taxels dealt over gridDim.y, their tails (ntax = 2048 k and +- 1, one
    taxel), a chunk whose every taxel is listed (the slab), chunks with a few and with none (the sphere; the lifted state), and the 4095 / 4096
    switch of the pose records a launch leaves for readout()"""
    run_case("list_%d_%s" % (ntax, prim), dtype, B, T, False, False, pad_dir, monkeypatch, "list",
             {"reset": "list", "default": "list", "per_record": "list"})


# ---------------------------------------------------------------------------------------------------- k_taxels_small and just past it
SMALL_SHAPES = [(5, 13, True), (67, 1, False), (9, 9, False)]       # nrec 65 (3 of 13 frames masked: blocks span frames and slots < 0), 67, 81


@pytest.mark.parametrize("dtype", DT, ids=ids)
@pytest.mark.parametrize("B,T,masked", SMALL_SHAPES)
@pytest.mark.parametrize("name", [n for n in P.TABLE if n.startswith("small_")])
def test_small_kernel(name, B, T, masked, dtype, pad_dir, monkeypatch):
    """k_taxels_small at its limits (1024 taxels, 8 combinations, 4 sensors), 16 records per block: a ragged last block (nrec 65, 67, 81), blocks
    that span frames and masked frames, per-environment sensor and shape rows on half of the cases"""
    tables = (sorted(P.TABLE).index(name) + B) % 2 == 0
    ntax, nsensor, nspt = P.TABLE[name][3]
    res = run_case(name, dtype, B, T, masked, tables, pad_dir, monkeypatch, "small",
                   {"reset": "small" if B >= 64 else "list" if nspt == 1 else "general", "default": "small", "per_record": "list" if nspt == 1 else "general"})
    assert T * B in (65, 67, 81) and (T * B) % 16 != 0


PAST = [(n, B, T) for n in P.TABLE if n.startswith("past_") for (B, T) in ((67, 1), (9, 9))] + [("small_130_1x1", 63, 1), ("small_130_4x2", 7, 9)]


@pytest.mark.parametrize("dtype", DT, ids=ids)
@pytest.mark.parametrize("name,B,T", PAST)
def test_just_past_the_small_kernel(name, B, T, dtype, pad_dir, monkeypatch):
    """1025 taxels, 9 combinations, 5 sensors, 63 records: the same launches go to k_taxels, and the results do not move (the oracle bound, and bit
    equality with the in-kernel read-out, hold on both sides of every switch)"""
    ntax, nsensor, nspt = P.TABLE[name][3]
    other = "list" if nspt == 1 and nsensor == 1 else "general"
    run_case(name, dtype, B, T, False, name.startswith("past_130"), pad_dir, monkeypatch, "past", {"reset": other, "default": other, "per_record": other})
    assert ntax > 1024 or nspt > 8 or nsensor > 4 or T * B == 63


# ---------------------------------------------------------------------------------------------------- the general branch, large pads
@pytest.mark.parametrize("dtype", DT, ids=ids)
@pytest.mark.parametrize("name,B,T", [("large_300_725", 4, 1), ("large_2000_2097", 4, 1), ("large_64_1_960_3072", 4, 3), ("large_300_blind_725", 4, 3),
                                      ("large_300_725", 256, 9)])
def test_general_branch_large(name, B, T, dtype, pad_dir, monkeypatch):
    """several sensors against three primitives above 1024 taxels: slices that are multiples of 256 (several per environment at B = 4; one per
    environment at 2304 records, more than the device holds blocks), the unroll's tail, sensor boundaries inside a slice (a sensor of ONE
    taxel; one without any primitive between two that have them)"""
    run_case(name, dtype, B, T, False, B == 4 and T == 3, pad_dir, monkeypatch, "large", {"reset": "general", "default": "general", "per_record": "general"})


# ---------------------------------------------------------------------------------------------------- the limits
@pytest.mark.parametrize("dtype", DT, ids=ids)
@pytest.mark.parametrize("name", ["limit_nspt64", "limit_nspt65", "limit_nsensor16", "limit_nsensor17", "limit_prims16"])
def test_limits(name, dtype, pad_dir, monkeypatch):
    """64 combinations, 16 sensors, 16 primitives on one sensor: every route.  65 combinations, 17 sensors: step / rollout still match the oracle
    (in-kernel) and readout() raises with its message.  An error or a correct result, never a wrong number."""
    beyond = name in ("limit_nspt65", "limit_nsensor17")
    k = "inkernel" if beyond else "general"
    run_case(name, dtype, 4, 1, False, False, pad_dir, monkeypatch, "limits", {"reset": k, "default": k, "per_record": k})


def test_seventeen_primitives_on_one_sensor_are_refused(pad_dir):
    from tactilesimulation_amd.host.batch import BatchSim
    with pytest.raises(RuntimeError, match="too many primitives per sensor"):
        BatchSim(P.table_model("limit_prims17", pad_dir), 3, dtype=F32, tape_capacity=0)


# ---------------------------------------------------------------------------------------------------- geometry edges
@pytest.mark.parametrize("dtype", DT, ids=ids)
@pytest.mark.parametrize("name", ["edge_rod", "edge_corner", "edge_graze", "edge_all"])
def test_geometry_edges(name, dtype, pad_dir, monkeypatch):
    """taxels at the end of a long thin cylinder's axis, at a cuboid's corner, on a sphere at grazing depth (tests/test_pad_models.py checks that the
    states are there): the bounding-sphere pre-test of k_taxels and the fp32 far test drop no taxel the oracle loads"""
    k = "general" if name == "edge_all" else "list"
    run_case(name, dtype, 4, 1, False, False, pad_dir, monkeypatch, "edges", {"reset": k, "default": k, "per_record": k})


# ---------------------------------------------------------------------------------------------------- more than four primitives per sensor
@pytest.mark.parametrize("dtype", DT, ids=ids)
@pytest.mark.parametrize("B,T", [(4, 1), (9, 9)])
def test_two_staging_groups_on_one_taxel(B, T, dtype, pad_dir, monkeypatch):
    """one sensor, six primitives, taxels loaded by primitives 0 and 5 (tests/test_pad_models.py): the in-kernel read-out stages the primitives in
    groups of TS_PAIR_GROUP = 4 and adds the PROJECTED outputs group by group, the taxel kernels add the link-frame forces and project once.  Both
    are within TOL of the oracle (run_case) and of each other.  They are not the same bits — measured max |difference| / max: 2.3e-8 and 4.6e-8
    (fp32), 4.3e-17 and 8.5e-17 (fp64) — which is what include/tsim.h states for such sensors."""
    res = run_case("groups6", dtype, B, T, False, False, pad_dir, monkeypatch, "groups", {"default": "small" if T * B >= 64 else "general"})
    a, c = res["default"]["frames"].double(), res["inkernel"]["frames"].double()
    d = float((a - c).abs().max() / a.abs().max())
    _rep("readout_groups", dtype=str(dtype), B=B, T=T, rel=d, equal=int(torch.equal(a, c)))
    print("in-kernel against taxel kernels, 6 primitives on one sensor: max |diff| / max = %.3g, bitwise equal: %s" % (d, torch.equal(a, c)))
    assert d <= TOL[dtype]


# ---------------------------------------------------------------------------------------------------- the tactile adjoint at its chunk edges
@pytest.mark.parametrize("dtype", DT, ids=ids)
@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("name", [n for n in P.TABLE if n.startswith("adj_")])
def test_tactile_adjoint_chunks(name, lanes, dtype, pad_dir):
    """vjp_taxels (csrc/tsim_kernels.h) walks a sensor's taxels in chunks of `lanes` with a one-chunk-ahead prefetch: nt = lanes k and +- 1, one
    taxel, two sensors.  Reset with a tape, two sub-steps, backward_steps(2, df_dtac = w) with both seed modes; dL/du and the carried adjoint
    against the oracle's, for the environments that went through the oracle's branches and converged (fp64: all five; fp32: at least four)."""
    from tactilesimulation_amd.host.batch import BatchSim
    from oracle.oracle import OracleSim
    m0 = P.table_model(name, pad_dir)
    import copy
    m = copy.copy(m0); m.F = m0.F.copy()
    m.F[Bl.TSIM_FH_TOL] = 1e-13 if dtype == F64 else 1e-8                    # as tests/test_gpu_bdf2_adjoint.py: what an fp32 residual can reach
    B, ntax = 5, m.ndof_tactile // 3
    st = P.table_states(name, m0)[:3] + P.states(m0, 7, "all_in" if ntax == 1 else "mixed", 2, ends=False)
    q0, qd0 = np.stack([s[0] for s in st]), np.stack([s[1] for s in st])
    rng = np.random.default_rng(29)
    u = rng.normal(size=(B, 6)) * np.array([1e-3] * 3 + [1e-6] * 3)
    ends_seen = set()
    for all_steps in (False, True):
        # weights of one sign: the seeded loss is a positively weighted sum of the taxel outputs, so its gradient is not the small difference of large
        # terms that zero-mean weights produce by chance — fp32 rounds relative to the terms, the bound is relative to the sum (measured with
        # zero-mean weights: profiles/r16_tactile_readout_shapes.md)
        w = rng.uniform(0.5, 1.5, size=(B, 2 if all_steps else 1, 3 * ntax))
        sim = BatchSim(m, B, dtype=dtype, tape_capacity=2)
        sim.set_lanes_per_env(lanes)
        assert sim.kernel_variant() == "generic"
        sim.reset(torch.tensor(q0, device=DEV, dtype=dtype), torch.tensor(qd0, device=DEV, dtype=dtype), backward_flag=True)
        out = sim.step(torch.tensor(u, device=DEV, dtype=dtype), 2)
        assert sim.launch_info()["lanes_per_env"] == lanes
        sig = sim.branch_signature().cpu().numpy()                            # [2, B, 2]
        du = sim.backward_steps(2, None, None, torch.tensor(w.reshape(B, -1), device=DEV, dtype=dtype), all_steps=all_steps).double().cpu().numpy()
        lq, lv = (x.double().cpu().numpy() for x in sim.get_adjoint())
        status = out["status"].cpu().numpy()
        ok = 0
        for e in range(B):
            o = OracleSim(m)
            o.reset(q0[e], qd0[e], record=True)
            bad, osig = o.forward_sig(u[e], 2)
            assert bad == 0
            wt = np.zeros((2, 3 * ntax)); wt[2 - w.shape[1]:] = w[e]
            duo = o.backward_steps(2, None, None, wt)
            alq, alv = o.adjoint()
            if status[e] != 0 or not np.array_equal(sig[:, e], osig):
                continue
            ok += 1
            q2, qd2 = o.state()
            ends_seen |= {t for t in P.sensor_ends(m0) if P.loaded(o, q2, qd2)[t]}
            rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
            g, a, v = rel(du[e], duo), rel(lq[e], alq), rel(lv[e], alv)
            _rep("readout_adjoint", name=name, lanes=lanes, dtype=str(dtype), all_steps=int(all_steps), env=e, du=g, lq=a, lv=v)
            assert np.abs(duo).max() > 0 and np.abs(alq).max() > 0
            assert max(g, a, v) <= TOL_ADJ[dtype], (name, lanes, all_steps, e, g, a, v)
        assert ok >= (5 if dtype == F64 else 4), (name, lanes, all_steps, ok, status, "environments on the oracle's branches")
    assert ends_seen == set(P.sensor_ends(m0)), (name, "a sensor's first or last taxel was loaded in no compared environment")
