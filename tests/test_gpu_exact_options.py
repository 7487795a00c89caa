"""The exact shortcuts of the residual evaluation and of the line search (include/tsim.h tsim_set_option) against the plain evaluation, on every model of
BASELINE.json's configs, in both precisions, generic and compiled-in kernels:

  TSIM_OPT_PAIR_CULL     a contact pair whose points' bounding sphere is out of reach of its primitive in every environment of a wavefront is
                         skipped, and the generic fp32 kernels test a point's fp32 distance before its double-precision one (csrc/tsim_eval.h phase2);
  TSIM_OPT_VALUE_TRIALS  line-search trials deep in a backtracking evaluate the residual without its tangents; a trial that is taken is
                         re-evaluated in full first (csrc/tsim_kernels.h k_forward).

  TSIM_OPT_TRIAL_HELPERS the slots of a wavefront whose environments are finished evaluate the next trial points of a slot that is still in a
                         line search; the owner judges the results in the sequential loop's order with its decision code (k_forward).

What they skip contributes exact zeros / is never read, so a batch with both off — every pair staged, every point through the double-precision
law, every trial a full evaluation — must give the SAME outputs, the same evaluation counts and the same gradients (torch.equal: up to the sign
of a zero).  (Parity of the default configuration with the oracle is what tests/test_gpu_models.py, test_gpu_configs.py and
test_gpu_reference_pins.py assert: both options are on by default there.)"""
import os

import numpy as np
import pytest
import torch

from tactilesimulation_amd.host.batch import BatchSim
from tactilesimulation_amd.model.compiler import load_model
from tactilesimulation_amd.workloads import asset, dclaw_random_workload, insertion_attempt_workload, push_workload

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# random models with general-primitive contact (tests/random_corpus.py: small corpus 9 / 86 / 64 / 93, large corpus, chain16: cuboid, sphere and
# cylinder pairs, ndof_r 9 .. 16; the fp64 batches of the large ones do not fit two environments per wavefront and skip the 32-lane tests), started from the contact sampler's states so that the fp32 far test decides points that are really near
RANDOM = ["random:9", "random:86", "random:64", "random:93", "random:L22", "random:L45", "random:L5", "random:chain16"]


def _random_case(case, B):
    import pathlib
    import sys
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import random_corpus as RC
    case = case if case[0] in "Lc" else int(case)
    m, rng = RC.draw(case, pathlib.Path(tempfile.mkdtemp(prefix="tsim_ex_")))
    states = RC.contact_states(m, RC.state_seed(case))
    assert states and m.ndof_u >= 1, case
    q0 = np.stack([states[e % len(states)][0] for e in range(B)]) + 0.005 * rng.normal(size=(B, m.ndof_r))
    u = rng.uniform(-1, 1, size=(B, 6, m.ndof_u))
    return m, q0, u, 2


def _case(name, B):
    if name.startswith("random:"):
        return _random_case(name[7:], B)
    m = load_model(asset(name))
    if name == "pusher":
        q0, u, _ = push_workload(B, 10, seed=3)
        return m, q0, u, 5
    if name == "dclaw_position_control":
        q0, u = dclaw_random_workload(B, 12, seed=1)
        return m, q0, u, 5
    q0, u = insertion_attempt_workload(B, seed=5)
    return m, q0, u[:, :30], 1


def _run(m, q0, u, S, dtype, cull, trials, static, helpers=False, lanes=0, first=False, record=True):
    B, T = u.shape[0], u.shape[1]
    sim = BatchSim(m, B, dtype=dtype, tape_capacity=T * S)
    sim.set_static(static)
    if lanes:
        sim.set_lanes_per_env(lanes)
    sim.set_option(BatchSim.OPT_PAIR_CULL, cull)
    sim.set_option(BatchSim.OPT_VALUE_TRIALS, trials)
    sim.set_option(BatchSim.OPT_TRIAL_HELPERS, helpers)
    sim.set_option(BatchSim.OPT_VALUE_FIRST, first)
    assert sim.get_option(BatchSim.OPT_PAIR_CULL) == int(cull) and sim.get_option(BatchSim.OPT_VALUE_TRIALS) == trials
    sim.reset(torch.tensor(q0, device=DEV, dtype=dtype), None, backward_flag=record)
    ro = sim.rollout(torch.tensor(u, device=DEV, dtype=dtype).transpose(0, 1).contiguous(), S, want_qd=True)
    ev = sim.last_evals().copy()
    if not record:
        z = torch.zeros(1)
        return ro, ev, z, z, z, sim.kernel_variant(), sim.last_helper_trials().copy(), sim.launch_info()["lanes_per_env"]
    g = torch.Generator().manual_seed(9)
    wq = torch.randn(T, B, m.ndof_r, generator=g, dtype=torch.float64).to(DEV, dtype)
    wv = torch.randn(T, B, m.ndof_var, generator=g, dtype=torch.float64).to(DEV, dtype) if m.ndof_var else None
    wt = torch.randn(T, B, m.ndof_tactile, generator=g, dtype=torch.float64).to(DEV, dtype) if m.ndof_tactile else None
    du = sim.backward_episode(T, S, wq, wv, wt)
    lq, lv = sim.get_adjoint()
    return ro, ev, du, lq, lv, sim.kernel_variant(), sim.last_helper_trials().copy(), sim.launch_info()["lanes_per_env"]


def _same(a, b, tag):
    for k in ("q", "qd", "var", "tactile", "status"):
        if k in a[0] and a[0][k] is not None and a[0][k].numel():
            assert torch.equal(a[0][k], b[0][k]), (tag, k, float((a[0][k].double() - b[0][k].double()).abs().max()))
    assert (a[1] == b[1]).all(), (tag, "evaluation counts", int((a[1] != b[1]).sum()))
    for x, y, k in ((a[2], b[2], "du"), (a[3], b[3], "lamq"), (a[4], b[4], "lamv")):
        assert torch.equal(x, y), (tag, k, float((x.double() - y.double()).abs().max()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", ["pusher", "dclaw_position_control", "tactile_insertion"] + RANDOM)
def test_the_shortcuts_change_no_number_on_the_generic_kernels(name, dtype):
    B = 256
    m, q0, u, S = _case(name, B)
    plain = _run(m, q0, u, S, dtype, False, 0, False)
    assert plain[5] == "generic"
    for cull, trials in ((True, 0), (False, 1), (False, 2), (True, 2)):
        _same(_run(m, q0, u, S, dtype, cull, trials, False), plain, (name, str(dtype), cull, trials))
    assert int(plain[1].max()) > int(np.median(plain[1]))      # environments differ in Newton effort: some went through line searches


def test_the_shortcuts_change_no_number_on_the_compiled_in_kernels(pusher_model):
    """TactilePush on the fully static instantiation (the bench's headline kernels): value-only trials on / off (the fused evaluation has no pair
    cull of its own)."""
    B = 1024
    q0, u, _ = push_workload(B, 12, seed=8)
    plain = _run(pusher_model, q0, u, 5, torch.float32, True, 0, True)
    assert plain[5] == "static:pusher"
    for trials in (1, 2, 3):
        _same(_run(pusher_model, q0, u, 5, torch.float32, True, trials, True), plain, ("static pusher", trials))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name,lanes", [("pusher", 16), ("pusher", 32), ("dclaw_position_control", 32), ("tactile_insertion", 32)] + [(r, 32) for r in RANDOM])
def test_helper_slots_change_no_number_on_the_generic_kernels(name, lanes, dtype):
    """Finished slots evaluating another slot's next line-search trials: same iterates, flags, evaluation counts (trial points judged), taped matrices
    (the gradients come from them) as the loop without helpers, with and without the other two shortcuts — and the helper path did run."""
    B = 256
    m, q0, u, S = _case(name, B)
    plain = _run(m, q0, u, S, dtype, False, 0, False, helpers=False, lanes=lanes)
    assert plain[5] == "generic" and int(plain[6].sum()) == 0
    if plain[7] != lanes:
        pytest.skip("launch shape falls back to %d lanes per environment" % plain[7])
    for cull, trials in ((False, 0), (True, 2)):
        r = _run(m, q0, u, S, dtype, cull, trials, False, helpers=True, lanes=lanes)
        _same(r, plain, (name, str(dtype), lanes, cull, trials, "helpers"))
        assert int(r[6].sum()) > 0 and (r[6] <= r[1]).all(), "no line-search trial was evaluated by a helper slot"


def test_helper_slots_with_per_environment_tables_on_the_generic_kernels():
    """D'Claw (generic kernels, two environments per wavefront) with one parameter table per environment — a helper slot evaluates the
    OWNER's trial point with the owner's table.  The header of a row (time step, gravity, tolerance) is a property of the batch: rows that carry
    another gravity are overwritten with the model's (include/tsim.h tsim_set_env_tables), so helpers — whose world record holds their own slot's
    gravity — and owners cannot disagree.  Helpers on == helpers off, bit for bit; a corrupted header changes nothing."""
    import tactilesimulation_amd.model.blob as BL
    B = 256
    m, q0, u, S = _case("dclaw_position_control", B)
    T, dtype = u.shape[1], torch.float32

    def run(helpers, bad_header):
        sim = BatchSim(m, B, dtype=dtype, tape_capacity=T * S)
        sim.set_lanes_per_env(32)
        tab = sim.base_tables()
        fo = int(m.I[BL.TSIM_IH_FOFF_PAIR])
        g = torch.Generator().manual_seed(4)
        tab[:, fo + BL.TSIM_PF_MU] *= (0.5 + torch.rand(B, generator=g)).to(tab)              # friction of the first contact pair, drawn per environment
        tab[:, fo + BL.TSIM_PF_KN] *= (0.8 + 0.4 * torch.rand(B, generator=g)).to(tab)
        if bad_header:
            tab[::3, BL.TSIM_FH_GZ] = -3.0
            tab[1::3, BL.TSIM_FH_H] *= 2.0
        sim.set_env_tables(tab)
        sim.set_option(BatchSim.OPT_TRIAL_HELPERS, helpers)
        sim.reset(torch.tensor(q0, device=DEV, dtype=dtype), None, backward_flag=True)
        ro = sim.rollout(torch.tensor(u, device=DEV, dtype=dtype).transpose(0, 1).contiguous(), S, want_qd=True)
        ev = sim.last_evals().copy()
        g = torch.Generator().manual_seed(9)
        wq, wv, wt = (torch.randn(T, B, n, generator=g).to(DEV) for n in (m.ndof_r, m.ndof_var, m.ndof_tactile))
        du = sim.backward_episode(T, S, wq, wv, wt)
        lq, lv = sim.get_adjoint()
        return ro, ev, du, lq, lv, sim.kernel_variant(), sim.last_helper_trials().copy(), sim.launch_info()["lanes_per_env"]

    plain, r, rb = run(False, False), run(True, False), run(True, True)
    if plain[7] != 32:
        pytest.skip("launch shape falls back to %d lanes per environment" % plain[7])
    assert plain[5] == "generic" and r[5] == "generic"
    _same(r, plain, ("dclaw, per-environment tables", "helpers"))
    _same(rb, plain, ("dclaw, per-environment tables", "rows with another gravity / time step in their header"))
    assert int(plain[6].sum()) == 0 and int(r[6].sum()) > 0


@pytest.mark.parametrize("tables", [False, True])
def test_the_default_options_instantiation_changes_no_number(pusher_model, tables, monkeypatch):
    """Round 6: with every solver / scheduling option at its default the fp32 forward launch of a compiled-in model at four environments per wavefront
    runs k_forward<..., TsDefaultOpts<MS>> — the options as compile-time constants (csrc/tsim_static.h; ~2 % faster) — and must give what the
    run-time-option kernel gives (TSIM_NO_DEFAULT_OPTS=1 at creation), bit for bit: states, tactile frames, evaluation counts, helper trials, gradients.
    Fully static and structure-static (per-environment tables)."""
    import tactilesimulation_amd.model.blob as BL
    B = 1024
    q0, u, _ = push_workload(B, 12, seed=8)
    T, S, dtype = u.shape[1], 5, torch.float32

    def run(no_default):
        if no_default:
            monkeypatch.setenv("TSIM_NO_DEFAULT_OPTS", "1")
        else:
            monkeypatch.delenv("TSIM_NO_DEFAULT_OPTS", raising=False)
        sim = BatchSim(pusher_model, B, dtype=dtype, tape_capacity=T * S)
        sim.set_lanes_per_env(16)
        assert sim.get_option(BatchSim.OPT_ALL_DEFAULT) == (0 if no_default else 1) and sim.get_option(BatchSim.OPT_CROSS_KINKS) == 1 and sim.get_option(BatchSim.OPT_EVAL_BUDGET) == 0
        if tables:
            tab = sim.base_tables()
            fo = int(pusher_model.I[BL.TSIM_IH_FOFF_DOF])
            tab[:, fo + BL.TSIM_DF_DAMPING] = (0.5 + torch.rand(B, generator=torch.Generator().manual_seed(4))).to(tab)
            sim.set_env_tables(tab)
        sim.reset(torch.tensor(q0, device=DEV, dtype=dtype), None, backward_flag=True)
        ro = sim.rollout(torch.tensor(u, device=DEV, dtype=dtype).transpose(0, 1).contiguous(), S, want_qd=True)
        ev = sim.last_evals().copy()
        g = torch.Generator().manual_seed(9)
        wq, wv, wt = (torch.randn(T, B, n, generator=g).to(DEV) for n in (7, 6, 390))
        du = sim.backward_episode(T, S, wq, wv, wt)
        lq, lv = sim.get_adjoint()
        return ro, ev, du, lq, lv, sim.kernel_variant(), sim.last_helper_trials().copy()

    a, b = run(False), run(True)
    assert a[5] == b[5] == ("param:pusher" if tables else "static:pusher")
    _same(a, b, ("static pusher", tables, "default-options instantiation"))
    assert (a[6] == b[6]).all()
    # a changed option takes the batch off it (and back)
    monkeypatch.delenv("TSIM_NO_DEFAULT_OPTS", raising=False)
    sim = BatchSim(pusher_model, 64, dtype=dtype, tape_capacity=0)
    assert sim.get_option(BatchSim.OPT_ALL_DEFAULT) == 1
    sim.set_solver_options(cross_kinks=True, eval_budget=32)
    assert sim.get_option(BatchSim.OPT_ALL_DEFAULT) == 0 and sim.get_option(BatchSim.OPT_EVAL_BUDGET) == 32
    sim.set_solver_options(cross_kinks=True, eval_budget=0); sim.set_option(BatchSim.OPT_VALUE_TRIALS, 0)
    assert sim.get_option(BatchSim.OPT_ALL_DEFAULT) == 0
    sim.set_option(BatchSim.OPT_VALUE_TRIALS, 2)
    assert sim.get_option(BatchSim.OPT_ALL_DEFAULT) == 1


@pytest.mark.parametrize("lanes", [16, 32])
@pytest.mark.parametrize("tables", [False, True])
def test_helper_slots_change_no_number_on_the_compiled_in_kernels(pusher_model, lanes, tables):
    """... on the static TactilePush instantiations (fully static; structure-static with one parameter table per environment: the helper reads
    the OWNER's table)."""
    import tactilesimulation_amd.model.blob as BL
    B = 1024
    q0, u, _ = push_workload(B, 12, seed=8)
    T, S, dtype = u.shape[1], 5, torch.float32

    def run(helpers):
        sim = BatchSim(pusher_model, B, dtype=dtype, tape_capacity=T * S)
        sim.set_lanes_per_env(lanes)
        if tables:
            tab = sim.base_tables()
            fo = int(pusher_model.I[BL.TSIM_IH_FOFF_DOF])
            g = torch.Generator().manual_seed(4)
            tab[:, fo + BL.TSIM_DF_DAMPING] = (0.5 + torch.rand(B, generator=g)).to(tab)      # joint damping of dof 0, drawn per environment
            sim.set_env_tables(tab)
        sim.set_option(BatchSim.OPT_TRIAL_HELPERS, helpers)
        sim.reset(torch.tensor(q0, device=DEV, dtype=dtype), None, backward_flag=True)
        ro = sim.rollout(torch.tensor(u, device=DEV, dtype=dtype).transpose(0, 1).contiguous(), S, want_qd=True)
        ev = sim.last_evals().copy()
        g = torch.Generator().manual_seed(9)
        wq, wv, wt = (torch.randn(T, B, n, generator=g).to(DEV) for n in (7, 6, 390))
        du = sim.backward_episode(T, S, wq, wv, wt)
        lq, lv = sim.get_adjoint()
        return ro, ev, du, lq, lv, sim.kernel_variant(), sim.last_helper_trials().copy()

    plain, r = run(False), run(True)
    assert r[5] == ("param:pusher" if tables else "static:pusher") and plain[5] == r[5]
    _same(r, plain, ("static pusher", lanes, tables, "helpers"))
    assert int(plain[6].sum()) == 0 and int(r[6].sum()) > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name,lanes,static", [("pusher", 16, False), ("pusher", 32, False), ("pusher", 16, True), ("pusher", 64, True), ("dclaw_position_control", 32, False),
                                               ("tactile_insertion", 32, False), ("tactile_insertion", 64, False)] + [(r, 32, False) for r in RANDOM])
def test_value_first_trials_change_no_number_in_forward_only_launches(name, lanes, static, dtype):
    """TSIM_OPT_VALUE_FIRST on launches that record no tape (roll-out collection): states, outputs, flags and evaluation counts of the loop
    without it — alone, and together with the other three shortcuts."""
    if static and dtype == torch.float64:
        pytest.skip("the compiled-in kernels are fp32")
    B = 256
    m, q0, u, S = _case(name, B)
    plain = _run(m, q0, u, S, dtype, False, 0, static, lanes=lanes, record=False)
    if plain[7] != lanes:
        pytest.skip("launch shape falls back to %d lanes per environment" % plain[7])
    assert plain[5] == ("static:pusher" if static else "generic")
    for cull, trials, helpers in ((False, 0, False), (True, 2, True)):
        r = _run(m, q0, u, S, dtype, cull, trials, static, helpers=helpers, lanes=lanes, first=True, record=False)
        _same(r, plain, (name, str(dtype), lanes, static, cull, trials, helpers, "value-first"))


@pytest.mark.parametrize("record", [True, False])
@pytest.mark.parametrize("name,lanes", [("pusher", 16), ("dclaw_position_control", 32)])
def test_the_shortcuts_under_an_evaluation_budget_on_a_ragged_batch(name, lanes, record):
    """All four options together against none of them where the loop is cut short: an evaluation budget of 3 per sub-step (flagged sub-steps, the
    take-or-reject decisions at the budget's edge) on a batch that does not fill its last wavefront (67 environments: the idle slots of the last
    wavefront are helpers from the first round)."""
    B = 67
    m, q0, u, S = _case(name, B)
    dtype = torch.float32

    def run(on):
        sim = BatchSim(m, B, dtype=dtype, tape_capacity=u.shape[1] * S if record else 0)
        sim.set_static(False)
        sim.set_lanes_per_env(lanes)
        sim.set_solver_options(cross_kinks=True, eval_budget=3)
        for opt, v in ((BatchSim.OPT_PAIR_CULL, on), (BatchSim.OPT_VALUE_TRIALS, 2 if on else 0), (BatchSim.OPT_TRIAL_HELPERS, on), (BatchSim.OPT_VALUE_FIRST, on)):
            sim.set_option(opt, v)
        sim.reset(torch.tensor(q0, device=DEV, dtype=dtype), None, backward_flag=record)
        ro = sim.rollout(torch.tensor(u, device=DEV, dtype=dtype).transpose(0, 1).contiguous(), S, want_qd=True)
        ev = sim.last_evals().copy()
        z = torch.zeros(1)
        du, lq, lv = z, z, z
        if record:
            T = u.shape[1]
            g = torch.Generator().manual_seed(9)
            wq = torch.randn(T, B, m.ndof_r, generator=g).to(DEV)
            wv = torch.randn(T, B, m.ndof_var, generator=g).to(DEV) if m.ndof_var else None
            wt = torch.randn(T, B, m.ndof_tactile, generator=g).to(DEV)
            du = sim.backward_episode(T, S, wq, wv, wt)
            lq, lv = sim.get_adjoint()
        return ro, ev, du, lq, lv, sim.launch_info()["lanes_per_env"], sim.last_helper_trials().copy()
    plain, r = run(False), run(True)
    if plain[5] != lanes:
        pytest.skip("launch shape falls back to %d lanes per environment" % plain[5])
    _same(r, plain, (name, lanes, record, "budget"))
    assert int((plain[0]["status"] != 0).sum()) > 0                                # the budget does cut sub-steps short
