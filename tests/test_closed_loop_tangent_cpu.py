"""The host side of the closed-loop tangent pass that needs no GPU (include/tsim_env.h tsim_push_closed_tangent, envs/push_closed_loop.py):
policy_direction_sources against torch's own forward-mode derivative of the three linear layers, and the entry points in the ctypes table with
the header's arity."""
import os
import re

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")


def _layers(theta, obs, h1, h2):
    """the three linear layers on the RECORDED inputs: what the sources are the parameter derivative of"""
    W1, b1, W2, b2, W3, b3 = theta
    return obs @ W1.t() + b1, h1 @ W2.t() + b2, h2 @ W3.t() + b3


@pytest.mark.parametrize("nin", [393, 3, 6])
@pytest.mark.parametrize("stacked", [False, True])
def test_policy_direction_sources_is_the_forward_mode_derivative_of_the_linear_layers(nin, stacked):
    from tactilesimulation_amd.envs.push_closed_loop import policy_direction_sources
    g = torch.Generator().manual_seed(7 + nin)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    T, B, nd = 3, 5, 4
    shapes = [(64, nin), (64, 64), (3, 64)]
    theta = tuple(r(*s) for s in (shapes[0], (64,), shapes[1], (64,), shapes[2], (3,)))
    obs, h1, h2 = r(T, B, nin), r(T, B, 64), r(T, B, 64)
    dirs = [tuple(r(*t.shape) for t in theta) for _ in range(nd)]
    dtheta = tuple(torch.stack([d[k] for d in dirs]) for k in range(6)) if stacked else [dict(zip(KEYS, d)) for d in dirs]
    s = policy_direction_sources(shapes, dtheta, obs, h1, h2)
    assert [tuple(x.shape) for x in s] == [(nd, T, B, 64), (nd, T, B, 64), (nd, T, B, 3)]
    for d in range(nd):
        _, ref = torch.autograd.functional.jvp(lambda *th: _layers(th, obs, h1, h2), theta, dirs[d])      # forward-mode, no finite difference
        for got, want in zip(s, ref):
            scale = float(want.abs().max())
            assert float((got[d] - want).abs().max()) <= 1e-13 * scale, (d, float((got[d] - want).abs().max()), scale)


def test_policy_direction_sources_missing_keys_are_zero_and_bad_input_is_refused():
    from tactilesimulation_amd.envs.push_closed_loop import policy_direction_sources
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    shapes = [(64, 6), (64, 64), (3, 64)]
    obs, h1, h2 = r(2, 3, 6), r(2, 3, 64), r(2, 3, 64)
    dW2, db3 = r(64, 64), r(3)
    s1, s2, s3 = policy_direction_sources(shapes, [{"W2": dW2}, {"b3": db3}], obs, h1, h2)
    assert int((s1 != 0).sum()) == 0
    assert torch.equal(s2[1], torch.zeros_like(s2[1])) and torch.allclose(s2[0], h1 @ dW2.t(), rtol=1e-13, atol=0)
    assert torch.equal(s3[0], torch.zeros_like(s3[0])) and torch.equal(s3[1], db3.expand(2, 3, 3))
    with pytest.raises(ValueError):
        policy_direction_sources(shapes, [{"W4": dW2}], obs, h1, h2)
    with pytest.raises(ValueError):
        policy_direction_sources(shapes, [{"W1": r(64, 7)}], obs, h1, h2)
    with pytest.raises(ValueError):
        policy_direction_sources([(64, 5), (64, 64), (3, 64)], [{"W2": dW2}], obs, h1, h2)


def _header_arity(name):
    txt = open(os.path.join(ROOT, "include", "tsim_env.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name + " is not declared in include/tsim_env.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,arity", [("tsim_push_closed_tangent", 24), ("tsim_push_closed_tangent_launch_info", 4)])
def test_the_entry_points_are_in_the_ctypes_table_with_the_headers_arity(name, arity):
    from tactilesimulation_amd.host import capi
    assert name in capi._SIGS, name
    res, args = capi._SIGS[name]
    assert _header_arity(name) == arity == len(args)
    assert hasattr(capi.lib(), name)


def test_the_kernel_table_lists_the_closed_tangent_instantiations_and_no_other_name_matches_the_pinned_patterns():
    """k_closed_tangent<R, 8, false, LPE, SRC>: R in {float, double} x LPE in {16, 32, 64} x SRC in {false, true}, and nothing else by that name"""
    import json
    from tactilesimulation_amd.host import buildhash
    if not os.path.exists(buildhash.KERNELS_JSON):
        import __graft_entry__
        __graft_entry__.build()
    table = json.load(open(buildhash.KERNELS_JSON))
    got = sorted(n for n in table if "k_closed_tangent" in n)
    want = sorted("_Z16k_closed_tangentI%sLi8ELb0ELi%dELb%dEEv13TanClosedArgsIT_E" % (r, l, s) for r in "fd" for l in (16, 32, 64) for s in (0, 1))
    assert got == want, (got, want)
    for n in got:
        assert table[n]["max_flat_workgroup_size"] == 64 and table[n]["code_bytes"] > 0
