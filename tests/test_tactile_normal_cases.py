"""The helpers of the tactile normal equations' tests (tests/tactile_normal_cases.py) and the Python layer's refusals that need no device.  No GPU.

The dense-F scatter and the reference product on a numpy-made H with known entries; the restated LDS plan's arithmetic against hand-computed figures
and its invariants on the models of the GPU file; the kernel table's instantiations of k_tactile_normal (no VGPR spills outside the EXPJ shapes); the
ValueErrors BatchSim.tactile_normal_equations and functions.episode_information raise before any call into C."""
import json
import os
import re
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pad_models as P      # noqa: E402
import param_grad_util as PU      # noqa: E402
import tactile_jacobian_cases as TC      # noqa: E402
import tactile_normal_cases as TN      # noqa: E402
import wide_models as W      # noqa: E402
from test_tangent_yardstick import tangent_case      # noqa: E402


# ---------------------------------------------------------------------------------------------------- the scatter and the reference
def test_dense_f_scatters_each_sensor_to_its_own_columns():
    sensors = [(0, 2, 1), (2, 1, 0), (3, 3, 2)]      # 6 taxels: 18 tactile values
    rng = np.random.default_rng(0)
    Ft = rng.normal(size=(2, 3, 4, 18))
    F = TN.dense_F(Ft, sensors)
    assert F.shape == (2, 3, 18, 12)
    for s, (t0, nt, _) in enumerate(sensors):
        rows = slice(3 * t0, 3 * (t0 + nt))
        for k in range(4):
            assert np.array_equal(F[..., rows, 4 * s + k], Ft[..., k, rows])
        other = np.ones(18, bool)
        other[rows] = False
        assert np.all(F[..., other, 4 * s:4 * s + 4] == 0)
    assert np.count_nonzero(F) == Ft.size


def test_reference_products_and_scales_on_a_known_h():
    H = np.array([[1.0, -2.0], [0.0, 3.0], [4.0, 0.0]])
    w = np.array([2.0, 1.0, 0.5])
    r = np.array([1.0, -1.0, 2.0])
    N, SN, n, Sn = TN.reference(H, w, r)
    assert np.array_equal(N, [[2 + 8, -4], [-4, 8 + 9]]) and np.array_equal(SN, [[10, 4], [4, 17]])
    assert np.array_equal(n, [2 + 4, -4 - 3]) and np.array_equal(Sn, [6, 7])
    assert np.array_equal(N, H.T @ np.diag(w) @ H) and np.array_equal(N, N.T)
    N2, SN2, n2, Sn2 = TN.reference(np.stack([H, 2 * H]), w)
    assert n2 is None and Sn2 is None and np.array_equal(N2[1], 4 * N) and np.array_equal(N2[0], N)
    # a zero row of H (an unloaded taxel) contributes nothing, whatever its weight and residual
    H0 = np.vstack([H, np.zeros((1, 2))])
    assert all(np.array_equal(a, b) for a, b in zip(TN.reference(H0, np.append(w, 7.0), np.append(r, 9.0)), (N, SN, n, Sn)))


def test_entry_index_is_the_packed_upper_triangle():
    for zc in (1, 2, 15, 19, 37):
        seen = [TN.tn_entry_index(zc, d, e) for d in range(zc) for e in range(d, zc)]
        assert seen == list(range(TN.tn_entries(zc)))


# ---------------------------------------------------------------------------------------------------- the plan's arithmetic
def test_slot_block_arithmetic():
    # TactilePush: nr = 7; with parameters 14 + 4 + 1 = 19 columns, 190 entries, rows of 21 reals
    assert TN.tn_zc(7, True, True) == 19 and TN.tn_zc(7, True, False) == 18 and TN.tn_zc(7, False, False) == 14 and TN.tn_zc(7, False, True) == 15
    assert TN.tn_stride(7, True) == 21 and TN.tn_stride(7, False) == 17 and TN.tn_entries(19) == 190
    assert TN.tn_slot_reals(7, True, 16) == 128 + 192 + 1008 and TN.tn_table_bytes(7, True) == 768
    assert TN.tn_slot_reals(7, False, 64) == 128 + 120 + 3264 and TN.tn_table_bytes(7, False) == 480
    # 16 dofs: 37 columns, 703 entries, rows of 39
    assert TN.tn_stride(16, True) == 39 and TN.tn_entries(37) == 703 and TN.tn_slot_reals(16, True, 4) == 288 + 704 + 468
    for nr in range(1, 17):
        for wp in (False, True):
            assert TN.tn_stride(nr, wp) % 2 == 1 and TN.tn_stride(nr, wp) > TN.tn_zc(nr, wp, True)      # odd, and room for the weight
            assert TN.tn_table_bytes(nr, wp) % 16 == 0 and all(TN.tn_slot_reals(nr, wp, r) % 4 == 0 for r in (4, 8, 16, 32, 64))


@pytest.fixture(scope="module")
def pad_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("tn_pads")


def _models(pad_dir):
    out = {n: tangent_case(n, 1)[0] for n in ("pusher", "dclaw_position_control", "tactile_insertion", "bdf2:ball_push")}
    out["tactile_pad"] = PU.case("tactile_pad", 1, 1)[0]
    out["stable_grasp"] = PU.case("stable_grasp", 1)[0]
    out["wide9"] = W.wide_model("wide9")
    for n in ["adj_%d" % k for k in (1, 15, 16, 17, 63, 64, 65, 129)] + ["small_130_%dx%d" % c for c in P.SMALL_COMBOS] + ["large_300_blind_725"]:
        out[n] = P.table_model(n, pad_dir)
    return out


def test_the_plan_launches_wherever_the_tactile_jacobians_launch(pad_dir):
    """the five reference models, wide9 and the pads of the GPU file, fp32 and fp64, every forced lane count, with and without parameters and
    per-environment rows: not refused, never fewer lanes than the tactile Jacobians' launch, at most as many taxels per trip as lanes"""
    for name, m in _models(pad_dir).items():
        for esz in (4, 8):
            for lanes in (0, 16, 32, 64):
                for rows in (True, False):
                    tj = TC.tactile_jacobian_shape(m, lanes, esz, rows)
                    assert tj[2], name
                    for wp in (False, True):
                        lpe, nbytes, fits, trip = TN.tactile_normal_shape(m, lanes, esz, wp, rows)
                        assert fits and nbytes <= W.LDS_CAP and nbytes % 16 == 0, (name, esz, lanes, wp, nbytes)
                        assert lpe >= tj[0] and lpe in (16, 32, 64) and TN.MIN_ROWS <= trip <= lpe and (trip == lpe or lpe == 64), (name, lpe, trip)


def test_the_16_dof_corpus_models_are_refused_in_fp64_and_launch_in_fp32():
    """large:L2 and large:L3 (16 dofs): one fp64 context with the records, the 703 sums, a tile of four taxels and the entry table is over 64 KB —
    the two models the frame Jacobians refuse in fp64 too (tests/frame_jacobian_cases.py REFUSED)"""
    want = {"large:L2": 73792, "large:L3": 68928}
    for name, nbytes in want.items():
        m = PU.case(name, 1)[0]
        assert m.ndof_r == 16
        assert TN.tactile_normal_shape(m, 0, 8, True) == (64, nbytes, False, TN.MIN_ROWS)
        assert TN.tactile_normal_shape(m, 0, 4, True)[2]
    m = PU.case("large:L26", 1)[0]      # 13 dofs: launches in fp64, at eight taxels per trip
    assert TN.tactile_normal_shape(m, 0, 8, True)[2:] == (True, 8)


# ---------------------------------------------------------------------------------------------------- the kernel table
NAME = re.compile(r"^_Z16k_tactile_normalI([fd])Li(8|16)ELb([01])ELi(16|32|64)EEv6TnArgsIT_E$")


def test_kernel_table_holds_the_instantiations_without_vector_spills():
    from tactilesimulation_amd.host import buildhash
    if not os.path.exists(buildhash.KERNELS_JSON):
        import __graft_entry__
        __graft_entry__.build()
    table = json.load(open(buildhash.KERNELS_JSON))
    got = {}
    for k, rec in table.items():
        if "k_tactile_normal" in k:
            g = NAME.match(k)
            assert g, k
            got[(g[1], int(g[2]), g[3] == "1", int(g[4]))] = rec
    want = {(r, n, False, l) for r in "fd" for n in (8, 16) for l in (16, 32, 64)} | {(r, 16, True, 64) for r in "fd"}
    assert set(got) == want
    for key, rec in got.items():
        assert rec["max_flat_workgroup_size"] == 64 and rec["code_bytes"] > 0
        if not key[2]:
            assert rec["vgpr_spill_count"] == 0 and rec["private_segment_fixed_size"] == 0, (key, rec)


# ---------------------------------------------------------------------------------------------------- the Python layer, before any call into C
def _fake_sim(ntac=12, B=2, nr=3):
    """a BatchSim without a device: the attributes tactile_normal_equations reads before it calls into C (which these tests never reach)"""
    import torch
    from tactilesimulation_amd.host.batch import BatchSim
    sim = BatchSim.__new__(BatchSim)
    sim.device, sim.dtype, sim.B, sim.ndof_r, sim.ndof_tactile = torch.device("cpu"), torch.float32, B, nr, ntac
    sim._h = None
    return sim


def test_python_layer_refuses_bad_weights_residuals_and_masks_without_a_device(monkeypatch):
    import torch
    from tactilesimulation_amd.host import capi
    monkeypatch.setattr(capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("the call reached C")))
    sim = _fake_sim()
    T, S = 3, 2
    with pytest.raises(ValueError, match="no masked frame"):
        sim.tactile_normal_equations(T, S, tactile_mask=torch.zeros(T, dtype=torch.bool))
    with pytest.raises(ValueError, match="tactile_mask"):
        sim.tactile_normal_equations(T, S, tactile_mask=torch.ones(T + 1, dtype=torch.bool))
    w, r = torch.ones(12), torch.zeros(T, 2, 12)
    for bad in (w[:-1], w.double(), w[None], torch.ones(24)[::2], [1.0] * 12, w.to("meta")):
        with pytest.raises(ValueError, match="weight"):
            sim.tactile_normal_equations(T, S, weight=bad)
    for bad in (r[:-1], r[:, :1], r[..., :-1], r.double(), torch.zeros(T, 2, 24)[..., ::2], r.to("meta")):
        with pytest.raises(ValueError, match="residual"):
            sim.tactile_normal_equations(T, S, residual=bad)
    with pytest.raises(ValueError, match="residual"):      # the mask's frames, not the window's
        sim.tactile_normal_equations(T, S, residual=r, tactile_mask=torch.tensor([True, False, True]))


def test_episode_information_refuses_a_column_that_is_no_parameter():
    import torch
    from tactilesimulation_amd.functions import episode_information
    m = tangent_case("pusher", 1)[0]
    sim = types.SimpleNamespace(model=m, ndof_r=m.ndof_r, tactile_normal_equations=lambda *a, **k: {"N": torch.zeros(1, 1, 18, 18), "n": torch.zeros(1, 1, 18)})
    with pytest.raises(ValueError, match="not a contact-group parameter"):
        episode_information(sim, 1, 1, cols=[0])
    pc = m.param_columns()
    sensor = [c for k, _, _, c in pc if k == "sensor"]
    pair = [c for k, _, _, c in pc if k == "pair"]
    N = torch.arange(18.0 * 18).reshape(1, 1, 18, 18)
    sim.tactile_normal_equations = lambda *a, **k: {"N": N, "n": N[..., 0].clone()}
    N2, n2 = episode_information(sim, 1, 1, residual=torch.zeros(1), cols=[sensor[2], pair[0], sensor[0]])
    idx = [*range(14), 16, 14]
    assert tuple(N2.shape) == (1, 1, 17, 17) and torch.equal(N2[0, 0][:, [*range(14), 14, 16]][[*range(14), 14, 16]], N[0, 0][idx][:, idx])
    assert bool((N2[..., 15, :] == 0).all()) and bool((N2[..., :, 15] == 0).all()) and float(n2[0, 0, 15]) == 0 and float(n2[0, 0, 14]) == float(N[0, 0, 16, 0])
