"""The kernels behind the table gradient of the fused closed loop (include/tsim_env.h tsim_push_closed_backward with a tsim_set_param_grad buffer
set): k_closed_backward_z, the closed-loop adjoint kernel's twin that also saves z of every sub-step (csrc/tsim_kernels.h).  The built library's
kernel table (host/buildhash.py) must hold it wherever a closed-loop k_backward exists (csrc/tsim_launch.h ts_instantiated) — the generic kernels
in fp32 and fp64 at 16, 32 and 64 lanes, static:pusher and param:pusher in fp32 at 16 lanes — under that name and no other."""
import json
import os
import re

import pytest


def test_kernel_table_holds_exactly_the_eight_closed_loop_twins():
    from tactilesimulation_amd.host import buildhash
    if not os.path.exists(buildhash.KERNELS_JSON):
        pytest.skip("library not built yet (python -c 'import __graft_entry__ as g; g.build()')")
    table = json.load(open(buildhash.KERNELS_JSON))
    combos = [(dt, lanes, "generic") for dt in ("f32", "f64") for lanes in (16, 32, 64)]
    combos += [("f32", 16, v) for v in ("static:pusher", "param:pusher")]
    want = set()
    for dt, lanes, variant in combos:
        mangled, readable = buildhash.kernel_name("k_closed_backward_z", dt, 7, False, lanes, variant, policy=True)
        assert mangled in table, (readable, mangled)
        rec = table[mangled]
        assert rec["vgpr_count"] > 0 and rec["code_bytes"] > 0 and rec["max_flat_workgroup_size"] == 64, (readable, rec)
        want.add(mangled)
    assert len(want) == 8
    # ... and nothing more under that name; the closed loop has no instantiation of the open-loop twin either (k_backward_z with POLICY = true)
    got = {n for n in table if re.match(r"_Z\d+k_closed_backward_zI", n)}
    assert got == want, ("not listed", sorted(got - want), "missing", sorted(want - got))
    assert not [n for n in table if re.match(r"_Z\d+k_backward_zI[fd]Li\d+ELb[01]ELi\d+ELb1E", n)]


def test_each_twin_sits_beside_the_closed_loop_adjoint_it_replaces():
    """same view, same shape: the twin's launch takes the plan of the closed-loop k_backward (LDS and launch bounds are the original's)"""
    from tactilesimulation_amd.host import buildhash
    if not os.path.exists(buildhash.KERNELS_JSON):
        pytest.skip("library not built yet (python -c 'import __graft_entry__ as g; g.build()')")
    table = json.load(open(buildhash.KERNELS_JSON))
    for dt, lanes, variant in [("f32", 16, "generic"), ("f64", 64, "generic"), ("f32", 16, "static:pusher"), ("f32", 16, "param:pusher")]:
        twin = table[buildhash.kernel_name("k_closed_backward_z", dt, 7, False, lanes, variant, policy=True)[0]]
        orig = table[buildhash.kernel_name("k_backward", dt, 7, False, lanes, variant, policy=True)[0]]
        for k in ("group_segment_fixed_size", "max_flat_workgroup_size", "sgpr_count"):
            assert twin.get(k) == orig.get(k), (dt, lanes, variant, k, twin, orig)
