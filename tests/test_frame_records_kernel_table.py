"""The kernel table host/buildhash.py writes at build time has a row for every instantiation of the two kernels of an episode launch that ends no
frame inside the forward kernel (csrc/tsim_launch.h ts_instantiated): k_frame_records wherever a fused compiled-in model has a forward kernel,
k_forward_fr where the TsDefaultOpts<> twin of k_forward is — and no others.  (No GPU: the table comes from the code object's metadata.)"""
import json
import os
import re

import pytest

from tactilesimulation_amd.host import buildhash


def test_kernel_table_names_the_frame_record_kernels():
    if not os.path.exists(buildhash.KERNELS_JSON):
        pytest.skip("library not built yet (python -c 'import __graft_entry__ as g; g.build()')")
    table = json.load(open(buildhash.KERNELS_JSON))
    want = set()
    for v in ("static:pusher", "param:pusher"):
        want |= {buildhash.kernel_name("k_frame_records", "f32", 7, False, l, v) for l in (16, 32, 64)}
        want |= {buildhash.kernel_name("k_frame_records", "f64", 7, False, l, v) for l in (32, 64)}
        want.add(buildhash.kernel_name("k_forward_fr", "f32", 7, False, 16, v))
    assert len(want) == 12
    for mangled, readable in want:
        assert mangled in table, (readable, mangled)
        rec = table[mangled]
        assert rec["vgpr_count"] > 0 and rec["code_bytes"] > 0 and rec["max_flat_workgroup_size"] == 64, (readable, rec)
    got = {n for n in table if re.match(r"_Z\d+(k_frame_records|k_forward_fr)I", n)}
    assert got == {m for m, _ in want}, sorted(got ^ {m for m, _ in want})
    # the forward kernel without the frame ends is the smaller one, and it spills less: what it is there for
    fr = table[buildhash.kernel_name("k_forward_fr", "f32", 7, False, 16, "static:pusher")[0]]
    kf = table[buildhash.kernel_name("k_forward", "f32", 7, False, 16, "static:pusher", default_opts=True)[0]]
    assert fr["code_bytes"] < kf["code_bytes"] and fr["sgpr_spill_count"] < kf["sgpr_spill_count"]
