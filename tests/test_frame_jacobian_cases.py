"""The frame-Jacobian edge cases of tests/frame_jacobian_cases.py, checked on the CPU against the oracle.  No GPU.

tests/test_gpu_frame_jacobian_edges.py can only catch a wrong row exchange of solve_lanes_many where the taped Newton matrix makes the pivot
rule leave the diagonal, and only tell a wrong pick from a right one where the rule is unambiguous.  Here, for every case, every one of the five
environments and both roundings of its rows: every sub-step converges on the oracle; the rule replayed on the oracle's H (pivot_order) leaves the
diagonal in exactly the frames the case list says — all three for PIVOT_EVERY_FRAME —; the runner-up of every pivot is more than 16 float ulp
away.  Five cases of the issue's list pivot in one frame only (small:88, small:90, small:35, small:51, small:113); the corpus has no model of
the 8-row solve other than small:11 that pivots in every frame (the last test), so they stay for the sizes they carry and the frame they pivot
in, and the claim "cannot hide a wrong row exchange in any frame" is made for PIVOT_EVERY_FRAME alone.
Then the sizes: the residues of ncol mod 8 over the present cases and these, a full last pass at NRM 8 and NRM 16, n = NRM at 8 and 16, the
trips of the Jvar task loop; and the launch plan: wide_models.frame_jacobian_shape gives the table the GPU file asserts against the library."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
import frame_jacobian_cases as FC      # noqa: E402
import random_corpus as RC      # noqa: E402
import wide_models as W      # noqa: E402

T, S = FC.T_FRAMES, FC.SUBSTEPS
TIE_ULP = 16


def _frames_that_pivot(m, q0, qd0, u):
    """(frames with an off-diagonal pivot on some sub-step, the orders of the sub-steps, the smallest runner-up distance in float ulp)"""
    bad, Hs = FC.newton_matrices(m, q0, qd0, u, S)
    assert bad == 0 and len(Hs) == T * S
    po = [FC.pivot_order(H) for H in Hs]
    ident = list(range(m.ndof_r))
    return tuple(f for f in range(T) if any(po[f * S + s][0] != ident for s in range(S))), [o for o, _ in po], min(g for _, g in po)


# ---------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", FC.NAMES)
def test_case_is_what_the_list_says(name):
    """sizes, integrator, and the pivot orders of environment 0 on the shared table, sub-step by sub-step"""
    nr, nu, nvar, bdf2, frames, _ = FC.CASES[name]
    m, q0, qd0, u, S_ = FC.fj_case(name)
    assert (m.ndof_r, m.ndof_u, FC.nvariables(m), S_) == (nr, nu, nvar, S) and (q0.shape, u.shape) == ((FC.B_ENVS, nr), (FC.B_ENVS, T, nu))
    assert int(m.I[Bl.TSIM_IH_INTEGRATOR]) == 1 and (int(FC._MODELS[name][0].I[Bl.TSIM_IH_INTEGRATOR]) == 2) == bdf2
    _, orders, _ = _frames_that_pivot(m, q0[0], qd0[0], u[0])
    seen, which = FC.ORDERS[name]
    print("pivot orders %s: %s at sub-steps %s" % (name, seen, which))
    assert orders == [seen[k] for k in which], (name, orders)


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64-rows", "fp32-rows"])
@pytest.mark.parametrize("name", FC.NAMES)
def test_every_environment_converges_and_pivots_where_the_list_says(name, fp32):
    """on the rows the GPU file sets (table_rows(m, 5, fp32, 11) through row_model): bad == 0, an off-diagonal pivot in the listed frames in EVERY
    environment, the rule unambiguous at every pivot"""
    m, q0, qd0, u, _ = FC.fj_case(name)
    want = FC.CASES[name][4]
    common, gap = set(range(T)), 1 << 31
    for e, me in enumerate(FC.env_models(m, fp32)):
        frames, orders, g = _frames_that_pivot(me, q0[e], qd0[e], u[e])
        common &= set(frames)
        gap = min(gap, g)
        assert set(want) <= set(frames), (name, e, frames)
    print("pivoting %s %s rows: every environment pivots in frames %s; closest runner-up %d float ulp" % (name, "fp32" if fp32 else "fp64", sorted(common), gap))
    assert tuple(sorted(common)) == want, (name, sorted(common))
    assert gap > TIE_ULP, (name, gap)
    if name in FC.PIVOT_EVERY_FRAME:
        assert want == tuple(range(T))


@pytest.mark.parametrize("name", FC.ORACLE_CASES)
def test_the_oracle_test_s_cases_pivot_unambiguously_on_its_own_rows(name):
    """the settings of test_frame_jacobians_against_the_oracle_rows: four environments, rows of seed 12, Newton tol 1e-13"""
    import copy
    m, q0, qd0, u, _ = FC.fj_case(name, FC.ORACLE_ENVS)
    m = copy.deepcopy(m)
    m.F[Bl.TSIM_FH_TOL] = 1e-13
    for e, me in enumerate(FC.env_models(m, False, FC.ORACLE_ENVS, FC.ORACLE_ROWS_SEED)):
        frames, _, gap = _frames_that_pivot(me, q0[e], qd0[e], u[e])
        assert set(FC.CASES[name][4]) <= set(frames) and frames and gap > TIE_ULP, (name, e, frames, gap)


def test_the_cases_left_out_do_not_converge():
    for name in FC.NOT_CONVERGED:
        m, q0, qd0, u, _ = FC.fj_case(name)
        assert name not in FC.NAMES and sum(FC.newton_matrices(me, q0[0], qd0[0], u[0], S)[0] for me in [m] + FC.env_models(m, False)) > 0, name


def test_no_other_model_of_the_8_row_solve_pivots_in_every_frame():
    """the corpus models with at most 8 dofs and no rotation-vector joint (NRM 8): small:11 alone leaves the diagonal in every frame of every
    environment, so the five cases that pivot in one frame have no replacement there.  An 8-dof model of that kind exists (small:102, n = NRM),
    and two with 2 nr + nu = 8 (small:6, and small:70, drawn with BDF2); none of them pivots"""
    every, eight, full = [], [], []
    for k in range(RC.N_MODELS):
        name = "small:%d" % k
        try:
            m, q0, qd0, u, _ = FC.fj_case(name)
        except AssertionError:
            continue
        if m.ndof_r > 8 or RC.has_exp_joint(m):
            continue
        envs = FC.env_models(m, False) + FC.env_models(m, True)
        runs = [FC.newton_matrices(me, q0[0], qd0[0], u[0], S) for me in envs]
        if all(bad == 0 for bad, _ in runs):
            ident = list(range(m.ndof_r))
            if all(all(any(FC.pivot_order(Hs[f * S + s])[0] != ident for s in range(S)) for f in range(T)) for _, Hs in runs):
                every.append(name)
            eight += [name] if m.ndof_r == 8 else []
            full += [name] if (2 * m.ndof_r + m.ndof_u) % 8 == 0 else []
    assert RC.N_MODELS != 120 or (every, eight, full) == (["small:11"], ["small:102"], ["small:6", "small:70"]), (every, eight, full)


# ---------------------------------------------------------------------------------------------------- the sizes
def _nrm(m):
    return 16 if m.ndof_r > 8 or RC.has_exp_joint(m) else 8


def test_sizes_cover_the_column_passes_and_the_task_loop():
    import wide_models
    from test_tangent_yardstick import TANGENT_CASES, tangent_case
    import param_grad_util as PU
    present = [tangent_case(n, 1)[0] for n in TANGENT_CASES if not n.startswith("bdf2:")] + [wide_models.wide_model(n) for n in wide_models.WIDE]
    present.append(PU.case("tactile_pad", 1, T)[0])
    ncol = lambda m: 2 * m.ndof_r + m.ndof_u      # noqa: E731
    assert {ncol(m) % 8 for m in present} == {1, 3, 4, 5, 6}
    new = {n: FC.fj_case(n)[0] for n in FC.NAMES}
    for n, m in new.items():
        assert RC.has_exp_joint(m) == ("EXPJ" in FC.CASES[n][5]), n
    assert {ncol(m) % 8 for m in present} | {ncol(m) % 8 for m in new.values()} == set(range(8))
    # nb = 8 ends the loop at NRM 8 and at NRM 16; nb = 2 and nb = 7 at both
    for nrm in (8, 16):
        assert {ncol(m) % 8 for m in new.values() if _nrm(m) == nrm} >= {0, 2, 7}, nrm
    assert ncol(new["small:6"]) == 8 and _nrm(new["small:6"]) == 8 and ncol(new["small:100"]) == 32 and ncol(new["small:111"]) == 24
    # n = NRM: every row of the register solve in use
    assert (new["small:102"].ndof_r, _nrm(new["small:102"])) == (8, 8) and all(new[n].ndof_r == 16 for n in ("large:L1", "large:L2", "large:L3"))
    # the Jvar task loop `for t0 = 0; t0 < nvar * nr; t0 += LPE` at k_frame_jacobian's lanes: trips per (case, type, forced lanes)
    trips = lambda n, esz, lanes: -(-(FC.nvariables(new[n]) * new[n].ndof_r) // FC.SHAPES[n, esz][lanes][0])      # noqa: E731
    assert trips("small:30", 4, 16) == 3 and trips("large:L26", 8, 0) == 2 and trips("large:L26", 4, 32) == 3 and trips("large:L3", 4, 0) == 2
    assert FC.nvariables(new["large:L2"]) * 16 == 64 == FC.SHAPES["large:L2", 4][0][0] and trips("large:L2", 4, 0) == 1      # nvar * nr == LPE exactly
    assert FC.nvariables(new["small:88"]) == 0 and new["small:88"].ndof_u == 0                                                 # no Jvar, no B


# ---------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("name", FC.NAMES)
def test_the_plan_s_shapes(name):
    """wide_models.frame_jacobian_shape per type and forced lanes against the table; the bytes are on record (profiles/r23_frame_jacobian_edges.md)"""
    m = FC.fj_case(name)[0]
    nl = int(m.I[Bl.TSIM_IH_NL])
    for esz in (4, 8):
        got = {l: W.frame_jacobian_shape(m, l, esz) for l in (0, 16, 32, 64)}
        print("plan %-10s %s: context %5d B, column block %5d B; forced 0 / 16 / 32 / 64 -> %s" % (
            name, "fp32" if esz == 4 else "fp64", W.lds_env_reals(nl, m.ndof_r, m.ndof_u, esz) * esz, W.fj_slot_reals(m.ndof_r, m.ndof_u) * esz,
            " ".join("%d lanes %d B%s" % (g[0], g[1], "" if g[2] else " REFUSED") for g in got.values())))
        assert got == FC.SHAPES[name, esz], (name, esz, got)
        assert all(g[2] == ((name, esz) not in FC.REFUSED) for g in got.values())
        assert all(l in got and l for l in FC.FORCED.get((name, esz), ()))


def test_the_doublings_and_the_refusal():
    """what the cases are in the list for: the plan doubles beyond the batch's shape (fp64 16 -> 32 and 32 -> 64, fp32 16 -> 32 and 16 -> 64), a
    16-dof fp64 block is refused at one environment per wavefront, large:L1's fits"""
    batch = lambda n, esz, l: W._launch_lanes(FC.fj_case(n)[0], l, esz, True, False, FC.B_ENVS, 1024, False)      # noqa: E731
    for n, esz, forced, b, fj in (("small:51", 8, 16, 16, 32), ("small:99", 8, 32, 32, 64), ("small:52", 4, 16, 16, 32), ("large:L2", 4, 16, 32, 64),
                                  ("small:111", 4, 16, 16, 16), ("small:30", 4, 16, 16, 16), ("small:102", 4, 16, 16, 16)):
        assert (batch(n, esz, forced), FC.SHAPES[n, esz][forced][0]) == (b, fj), (n, esz, forced)
    assert FC.SHAPES["small:111", 4][16][1] == 60688 and FC.SHAPES["large:L1", 8][0] == (64, 63072, True)
    assert FC.SHAPES["large:L2", 8][0] == (64, 72160, False) and FC.SHAPES["large:L3", 8][0] == (64, 68864, False)
    # the refused blocks: one context and one column block
    for n in ("large:L2", "large:L3"):
        m = FC.fj_case(n)[0]
        blk = W.fj_slot_reals(16, m.ndof_u) * 8
        ctx = FC.SHAPES[n, 8][0][1] - blk
        assert ctx in (W.block_bytes(m, 1, 8, True, False), W.block_bytes(m, 1, 8, True, True)) and ctx <= W.LDS_CAP < ctx + blk, (n, ctx, blk)
        print("refusal %s fp64: contexts %d B + column block %d B = %d B > %d" % (n, ctx, blk, ctx + blk, W.LDS_CAP))
