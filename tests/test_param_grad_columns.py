"""The columns a table gradient covers (CompiledModel.param_columns, include/tsim.h tsim_set_param_grad) — no GPU.  They must be exactly the
entries table_offset names for contact pairs, tactile sensors and dofs, in the Python compiler and in the native loader alike, and the library
must export the entry point."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
ASSETS = ["pusher", "tactile_insertion", "stable_grasp", "dclaw_position_control", "tactile_pad"]


def _expected(py):
    """(kind, key, field) -> column from table_offset, the lookup the per-environment tables are edited with"""
    out = {}
    for k in py.meta["pair_keys"]:
        for f in ("kn", "kt", "mu", "damping"):
            out[("pair", tuple(k), f)] = py.table_offset("pair", tuple(k), f)
    for s in py.meta["sensor_names"]:
        for f in ("kn", "kt", "mu", "damping"):
            out[("sensor", s, f)] = py.table_offset("sensor", s, f)
    for j, (d0, nd) in py.meta["dof_of_joint"].items():
        for k in range(nd):
            out[("dof", (j, k), "damping")] = py.table_offset("dof", (j, k), "damping")
    return out


def _check(py, native):
    cols = py.param_columns()
    assert len({c for (_, _, _, c) in cols}) == len(cols)                  # no column twice
    assert {(k, key, f): c for (k, key, f, c) in cols} == _expected(py)
    for kind, key, f, c in cols:
        if kind == "pair":
            assert native.table_offset("pair", key[0], key[1], f) == c
        elif kind == "sensor":
            assert native.table_offset("sensor", key, field=f) == c
        else:
            assert native.table_offset("dof", key[0], field=key[1]) == c
    n = int(py.I[__import__("tactilesimulation_amd.model.blob", fromlist=["x"]).TSIM_IH_FOFF_CPT])
    assert all(0 <= c < n for (_, _, _, c) in cols)                         # inside the per-environment table
    # exactly 4 per pair, 4 per sensor, 1 per dof
    assert len(cols) == 4 * len(py.meta["pair_keys"]) + 4 * len(py.meta["sensor_names"]) + py.ndof_r


@pytest.mark.parametrize("name", ASSETS)
def test_param_columns_of_the_shipped_assets(name):
    """against table_offset and the native loader's recorded lookups of the reference's models (tests/golden/reference_models.npz)"""
    from test_native_model_loader import REF_XMLS, _Recorded
    rel = [r for r in REF_XMLS if os.path.splitext(os.path.basename(r))[0] == name][0]
    rec = _Recorded(rel)
    _check(rec.python(), rec)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(HERE, "models", "*.xml"))), ids=os.path.basename)
def test_param_columns_of_the_test_models(path):
    from tactilesimulation_amd.host.native_model import NativeModel
    from tactilesimulation_amd.model.compiler import compile_spec, parse_xml
    _check(compile_spec(parse_xml(path)), NativeModel(path))


@pytest.mark.parametrize("seed", range(20))
def test_param_columns_of_random_models(seed, tmp_path):
    from test_native_model_loader import _random_model
    from tactilesimulation_amd.host.native_model import NativeModel
    from tactilesimulation_amd.model.compiler import compile_spec, parse_xml
    p = str(tmp_path / "m.xml")
    open(p, "w").write(_random_model(np.random.default_rng(7000 + seed), max_dof=12))
    _check(compile_spec(parse_xml(p)), NativeModel(p))


def test_library_exports_set_param_grad():
    from tactilesimulation_amd.host import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "tsim_set_param_grad")
    assert "tsim_set_param_grad" in capi.EXPORTS
    assert capi.lib().tsim_set_param_grad is not None
