"""k_param_jacobian in the kernel table of the built library, and the census of the tests that run its instantiations.  No GPU.

The table (host/buildhash.py write_kernel_table) must hold the 14 instantiations the launch plan can name — float / double x NRM 8, 16 x 16, 32, 64
lanes per environment, and (NRM 16, rotation-vector joint, 64 lanes) — each with its registers and code bytes, none with spilled vector registers or
static LDS, under a name that none of the older kernels' census patterns match.  Every instantiation is either run by a test of
tests/test_gpu_param_jacobians.py that has the census' case and forced lanes among its parameters, at the shape the restated plan
(param_jacobian_cases.param_jacobian_shape) gives that case, or cannot be reached by any model."""
import importlib
import inspect
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import param_jacobian_cases as PJ      # noqa: E402
import wide_models as W      # noqa: E402

NAME = re.compile(r"^_Z16k_param_jacobianI([fd])Li(8|16)ELb([01])ELi(16|32|64)EEv6PjArgsIT_E$")
# how the older census tests pick their kernels out of the table (tests/test_wide_models.py, tests/test_capi_symbols.py,
# tests/test_tactile_jacobian_kernel_table.py): by a name that begins so, or that contains `tactile_jacobian`
OLDER = re.compile(r"^_Z\d+(k_frame_jacobianI|k_param_gradI|k_param_grad_bodyI|k_tangent\w*I|k_closed_tangentI|k_forward|k_backward|k_closed_backward)")


def _table():
    from tactilesimulation_amd.host import buildhash
    if not os.path.exists(buildhash.KERNELS_JSON):
        import __graft_entry__
        __graft_entry__.build()
    return json.load(open(buildhash.KERNELS_JSON))


def _rows(table):
    out = {}
    for k, rec in table.items():
        g = NAME.match(k)
        if g:
            out[g.group(1), int(g.group(2)), g.group(3) == "1", int(g.group(4))] = rec
    return out


def test_the_kernel_table_holds_the_fourteen_instantiations():
    table = _table()
    rows = _rows(table)
    want = {(r, nrm, False, lpe) for r in "fd" for nrm in (8, 16) for lpe in (16, 32, 64)} | {(r, 16, True, 64) for r in "fd"}
    assert set(rows) == want and len(want) == 14
    assert sum("param_jacobian" in k for k in table) == 14                  # no instantiation under another name
    for key, rec in rows.items():
        assert rec["code_bytes"] and rec["code_bytes"] > 0 and rec["vgpr_count"] > 0 and rec["sgpr_count"] > 0, key
        assert rec["vgpr_spill_count"] == 0 and rec["max_flat_workgroup_size"] == 64 and rec["group_segment_fixed_size"] == 0, (key, rec)
    for k in table:
        if "param_jacobian" in k:
            assert "tactile_jacobian" not in k and not OLDER.match(k), k
    # ... and the patterns do find the older kernels, so the line above tests something
    assert sum(bool(OLDER.match(k)) for k in table) > 100 and sum("tactile_jacobian" in k for k in table) == 14


def _test_runs(path, fn, case, lanes):
    """does the test `fn` of tests/`path` run `case` with `lanes` forced?  Read off the test itself: the case and the lanes (0: none forced) are
    among the values of its parametrize marks"""
    f = getattr(importlib.import_module(path[:-3]), fn)
    vals = []
    for mk in getattr(f, "pytestmark", []):
        if mk.name == "parametrize":
            for v in mk.args[1]:
                v = getattr(v, "values", v)
                vals += list(v) if isinstance(v, (tuple, list)) else [v]
    return (case in vals or '"%s"' % case in inspect.getsource(f)) and (lanes == 0 or lanes in vals)


def test_every_instantiation_is_run_by_a_test_or_cannot_be():
    import test_gpu_param_jacobians as G
    import random_corpus as RC
    got = set(_rows(_table()))
    assert not set(G.REACHED_BY) & G.UNREACHABLE and set(G.REACHED_BY) | G.UNREACHABLE == got
    for inst in G.UNREACHABLE:
        assert inst == ("d", 16, False, 16) and 4 * W.env_bytes_lower_bound(9, 8) > W.LDS_CAP
    for (r, nrm, expj, lpe), (case, lanes, rows, fn) in G.REACHED_BY.items():
        assert _test_runs("test_gpu_param_jacobians.py", fn, case, lanes), (fn, case, lanes)
        m = G.census_model(case)
        assert RC.has_exp_joint(m) == expj and nrm == (16 if m.ndof_r > 8 or expj else 8), (case, r, nrm, expj)
        if expj:
            assert lpe == 64
            continue
        shape = PJ.param_jacobian_shape(m, lanes, 8 if r == "d" else 4, rows)
        assert shape[0] == lpe and shape[2], (case, lanes, r, shape, lpe)


def test_the_restated_plan_refuses_fp64_large_l2_and_no_fp32_batch():
    """the slot's block is sized for 32 columns whatever is selected: [32][2 nr] + [8][nr] reals.  large:L2 (16 dofs) at one environment per
    wavefront is over 64 KB in fp64 (the GPU file runs its refusal) and fits in fp32"""
    import frame_jacobian_cases as FC
    m = FC.fj_case("large:L2")[0]
    assert m.ndof_r == 16 and PJ.pj_slot_reals(16) == 32 * 32 + 128
    assert PJ.param_jacobian_shape(m, 0, 8, True)[1:] == (68512, False) and PJ.param_jacobian_shape(m, 64, 8, True)[2] is False
    assert PJ.param_jacobian_shape(m, 0, 4, True)[2] is True
