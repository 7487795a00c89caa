"""Predictor helpers (csrc/tsim_kernels.h k_forward; include/tsim.h TSIM_OPT_PREDICTOR_HELPERS): a slot of a wavefront whose own environment is finished
evaluates, in the round in which a live slot evaluates the point that may end its sub-step, the predictor of that slot's NEXT sub-step; if the point
is committed the live slot starts the next sub-step from the helper's evaluation (g, H and K copied from its LDS).  An evaluation is a function of its
inputs only, so everything the launch leaves must be what the loop without the option leaves, bit for bit — that identity is the whole correctness
argument, and what every case below asserts: q, qd, variables, tactile frames, status, evaluation counts, dL/du and the carried adjoint (dL/dq0,
dL/dqd0: through the taped H and K) of the default run against TSIM_NO_PREDICTOR_HELPERS=1.

The switch is read from the environment when a batch is created, so each setting runs in a fresh child process — this file, as a script, runs EVERY
case once and leaves the results in one .npz; the module's fixture starts the children once, the tests compare case by case.  A third child runs with
TSIM_NO_TRIAL_HELPERS=1, under which no slot helps at all.  EVERY LAUNCH OF A CASE IS ANOTHER EPISODE (start states and actions re-seeded by the
launch's index, identically in all children); nothing clears the tape, the counts or the output buffers in between.

The shapes are the smallest at which the option can go wrong: a helper exists only where a finished (or idle) slot shares a wavefront with a live
one — batches below and just above one wavefront of four (fp64: two) environments.  The helper-trial counts (tsim_last_helper_trials) are no part of
the comparison — they are what differs — and are asserted on their own: with the option on they also count the predictors taken over.

Altered libraries, each of which must turn this file red (profiles/r28_predictor_helpers.md records which tests each fails): the helper takes the
owner's current action instead of the next one at a frame boundary; the adoption copies H but not K (case b1_budget1); the predictor is formed from
q0 instead of the evaluated point."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = "cuda:0"
SWITCHES = ("TSIM_NO_PREDICTOR_HELPERS", "TSIM_NO_TRIAL_HELPERS")

# case -> (kernel variant, B, frames, sub-steps per frame)
CASES = {
    "b1": ("static:pusher", 1, 3, 5),            # three idle slots help from round 1
    "b2": ("static:pusher", 2, 3, 5),            # helpers shared between owners: two idle slots, two owners
    "b3": ("static:pusher", 3, 3, 5),            # ... one idle slot, three owners
    "b5": ("static:pusher", 5, 4, 5),            # one full wavefront, and one wavefront with helpers
    "rest4": ("static:pusher", 4, 4, 5),         # one environment pushing into the box, three at rest: the helpers appear mid-launch
    "b3_6x1": ("static:pusher", 3, 6, 1),        # every commit is a frame boundary: the helper needs the NEXT action
    "masked_b3": ("static:pusher", 3, 3, 5),     # tactile mask with the first and the last frame masked out
    "param_b5": ("param:pusher", 5, 3, 5),       # one parameter table per environment: the helper evaluates with the owner's
    "f64_b3": ("static:pusher", 3, 3, 5),        # fp64 at two environments per wavefront: one helper per owner
    # an evaluation budget of ONE per sub-step: every sub-step ends with its first evaluation, so every predictor taken over ENDS its sub-step at once.
    # The lone environment then sits out a round that computes no tangents (no live slot asks for any) and commits the H and K it copied from the
    # helper — the one path on which the tape's K is the copy itself
    "b1_budget1": ("static:pusher", 1, 3, 5),
}
# first episode's seed (the second: + 17).  Eight for the two cases whose tactile frames are few — one sub-step per frame; only the middle frame read out —:
# with it both episodes touch the pad in those frames (found with the CPU oracle), so the tactile comparison is one of forces, not of zeros
SEED = {"b3_6x1": 8, "masked_b3": 8}
OUT_KEYS = ("q", "qd", "var", "tactile", "status", "evals", "du", "lamq", "lamv")
LAUNCHES = 2


# ---------------------------------------------------------------------------------------------------- the child: every case, once
def _seeds(sim, T, B, torch, mask=None):
    g = torch.Generator().manual_seed(9)
    nm = T if mask is None else int(mask.sum())
    return tuple(torch.randn(n_, B, n, generator=g, dtype=torch.float64).to(DEV, sim.dtype) for n_, n in ((T, sim.ndof_r), (T, sim.ndof_var), (nm, sim.ndof_tactile)))


def _episode(sim, q0, u, S, seeds, mask=None, qd0=None):
    sim.reset(q0, qd0, backward_flag=True)
    out = {k: v.cpu().numpy() for k, v in sim.rollout(u, S, want_qd=True, tactile_mask=mask).items()}
    out["frame_records"] = np.array(sim.get_option(sim.OPT_FRAME_RECORDS))
    out["evals"], out["helped"] = sim.last_evals().copy(), sim.last_helper_trials().copy()
    out["du"] = sim.backward_episode(int(u.shape[0]), S, *seeds, tactile_mask=mask).cpu().numpy()
    out["lamq"], out["lamv"] = (x.cpu().numpy() for x in sim.get_adjoint())
    return out


def _child(path):
    import torch
    sys.path.insert(0, ROOT)
    import tactilesimulation_amd.model.blob as BL
    from tactilesimulation_amd.host.batch import BatchSim
    from tactilesimulation_amd.host.graphed import GraphedEpisode
    from tactilesimulation_amd.model.compiler import load_model
    from tactilesimulation_amd.workloads import asset, push_workload
    pusher = load_model(asset("pusher"))
    res = {}

    def inputs_of(B, T, dtype, seed, rest=()):
        q0, u, _ = push_workload(B, T, seed=seed)
        for e in rest:          # an environment at rest: no action, no disturbance
            u[e] = 0.0
        return torch.tensor(q0, device=DEV, dtype=dtype), torch.tensor(u, device=DEV, dtype=dtype).transpose(0, 1).contiguous()

    def run(case, dtype=torch.float32, lanes=16, mask=None, tables=False, rest=(), budget=0, shape=None, option=None):
        _, B, T, S = CASES[shape or case]
        sim = BatchSim(pusher, B, dtype=dtype, tape_capacity=T * S)
        sim.set_lanes_per_env(lanes)
        if tables:
            tab = sim.base_tables()
            g = torch.Generator().manual_seed(4)
            tab[:, int(pusher.I[BL.TSIM_IH_FOFF_DOF]) + BL.TSIM_DF_DAMPING] = (0.5 + torch.rand(B, generator=g)).to(tab)
            tab[:, int(pusher.I[BL.TSIM_IH_FOFF_PAIR]) + BL.TSIM_PF_KN] *= (0.8 + 0.4 * torch.rand(B, generator=g)).to(tab)
            sim.set_env_tables(tab)
        if budget:
            sim.set_solver_options(eval_budget=budget)
        if option is not None:      # the run-time switch, whatever the environment said at creation
            sim.set_option(sim.OPT_PREDICTOR_HELPERS, option)
        seeds = _seeds(sim, T, B, torch, mask)
        res[case + "/variant"] = np.array(sim.kernel_variant())
        res[case + "/option"] = np.array(sim.get_option(sim.OPT_PREDICTOR_HELPERS))
        for i in range(LAUNCHES):
            q0, u = inputs_of(B, T, dtype, SEED.get(case, 5) + 17 * i, rest)
            # (budget: no Newton step is ever taken, the state only follows its predictor — from rest it would not move and every K would be the same matrix)
            qd0 = None if not budget else (0.5 * torch.randn(B, sim.ndof_r, generator=torch.Generator().manual_seed(3 + i), dtype=torch.float64)).to(DEV, dtype)
            for k, v in _episode(sim, q0, u, S, seeds, mask, qd0).items():
                res["%s/%s@%d" % (case, k, i)] = v

    for case in ("b1", "b2", "b3", "b5", "b3_6x1"):
        run(case)
    run("rest4", rest=(1, 2, 3))
    run("masked_b3", mask=torch.tensor([False, True, False]))
    run("param_b5", tables=True)
    run("f64_b3", dtype=torch.float64, lanes=32)
    run("b1_budget1", budget=1)
    run("b1_opt0", shape="b1", option=0)      # case b1 again, the option set at run time (tsim_set_option) in EVERY child
    run("b1_opt1", shape="b1", option=1)
    # a graph captured behind an eager episode (GraphedEpisode's warm-up), replayed on the SECOND episode of case b3, written into its static inputs after
    # the capture: against that case's eager second launch
    _, B, T, S = CASES["b3"]
    sim = BatchSim(pusher, B, dtype=torch.float32, tape_capacity=T * S)
    sim.set_lanes_per_env(16)
    q0s, us = inputs_of(B, T, torch.float32, 5)
    ge = GraphedEpisode(sim, q0s, us, S, seeds=_seeds(sim, T, B, torch))
    q0n, un = inputs_of(B, T, torch.float32, 5 + 17)
    q0s.copy_(q0n); us.copy_(un)
    ro, du, _ = ge.replay()
    torch.cuda.synchronize()
    for k in ("q", "var", "tactile", "status"):
        res["graph/replay_" + k] = ro[k].cpu().numpy()
    res["graph/replay_du"] = du.cpu().numpy()
    res["graph/replay_evals"], res["graph/replay_helped"] = sim.last_evals().copy(), sim.last_helper_trials().copy()
    np.savez(path, **res)


# ---------------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: the child's .npz}: the default path, TSIM_NO_PREDICTOR_HELPERS=1 and TSIM_NO_TRIAL_HELPERS=1, one fresh process each"""
    d = tmp_path_factory.mktemp("predictor_helpers")
    procs = {}
    for setting, switch in (("default", None), ("off", "TSIM_NO_PREDICTOR_HELPERS"), ("no_helpers", "TSIM_NO_TRIAL_HELPERS")):      # side by side: most of a child's time is start-up
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        if switch:
            env[switch] = "1"
        path = str(d / (setting + ".npz"))
        procs[setting] = (path, subprocess.Popen([sys.executable, os.path.abspath(__file__), path], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    out, failed = {}, []
    for setting, (path, p) in procs.items():
        try:
            log = p.communicate(timeout=300)[0]
        except subprocess.TimeoutExpired:
            p.kill()
            log = "timed out\n" + p.communicate()[0]
        if p.returncode != 0:
            failed.append((setting, p.returncode, log[-4000:]))
        else:
            out[setting] = dict(np.load(path))
    assert not failed, failed
    return out


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _case(runs, setting, case):
    return {k[len(case) + 1:]: v for k, v in runs[setting].items() if k.startswith(case + "/")}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_launch_with_predictor_helpers_equals_the_one_without(runs, case):
    variant = CASES[case][0]
    new, old, none = (_case(runs, s, case) for s in ("default", "off", "no_helpers"))
    assert str(new["variant"]) == variant and str(old["variant"]) == variant
    assert int(new["option"]) == 1 and int(old["option"]) == 0
    for i in range(LAUNCHES):
        print(case, "launch", i, "frame records", int(new["frame_records@%d" % i]), "evals", old["evals@%d" % i].tolist(), "helped: on", new["helped@%d" % i].tolist(),
              "off", old["helped@%d" % i].tolist(), "no helpers", none["helped@%d" % i].tolist())
        for k in OUT_KEYS:
            for other, name in ((new, "default"), (none, "no helpers")):
                a, b = other["%s@%d" % (k, i)], old["%s@%d" % (k, i)]
                assert _same_bits(a, b), (case, name, i, k, float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()))
        assert np.isfinite(old["q@%d" % i]).all() and int(old["evals@%d" % i].min()) > 0
        if case == "b1_budget1":      # every sub-step cut short: one evaluation each; and sub-steps did start from a helper's evaluation
            _, B, T, S = CASES[case]
            assert (old["evals@%d" % i] == T * S).all() and (new["helped@%d" % i] > 0).all() and (old["helped@%d" % i] == 0).all()
        else:
            assert np.abs(old["tactile@%d" % i]).max() > 0
        assert (none["helped@%d" % i] == 0).all()
    assert "q@%d" % LAUNCHES not in new


def test_every_launch_of_a_case_is_another_episode(runs):
    r = runs["off"]
    for case in CASES:
        moving = [0] if case == "rest4" else slice(None)      # (the environments at rest stay where they are, launch after launch)
        for k in ("q", "du"):
            d = r["%s/%s@1" % (case, k)] != r["%s/%s@0" % (case, k)]
            print(case, k, "environments that differ", d.any(axis=(0, 2)).tolist())
            assert d.any(axis=(0, 2))[moving].all(), (case, k)


def test_a_lone_environment_is_helped_by_its_three_idle_slots(runs):
    """B = 1: the slots without an environment are finished from the first round.  Off: they evaluate line-search trials only (the code path of the loop
    before the option).  On: one of them takes the predictor, and every sub-step but the first can start from its evaluation — the count also holds the
    predictors taken over, 14 sub-steps could, so it is larger than the trial-only count of the same episode."""
    new, old = _case(runs, "default", "b1"), _case(runs, "off", "b1")
    for i in range(LAUNCHES):
        on, off = int(new["helped@%d" % i][0]), int(old["helped@%d" % i][0])
        print("b1 launch", i, "helped on", on, "off", off, "evals", int(old["evals@%d" % i][0]))
        assert on > 0 and on > off >= 0


def test_the_run_time_switch_is_the_environment_variable(runs):
    """tsim_set_option(TSIM_OPT_PREDICTOR_HELPERS) after creation, in the child that was created with the option on and in the one created with it off:
    set to 0, the launch is the TSIM_NO_PREDICTOR_HELPERS=1 child's — the same outputs and the same helper count, which is the trial-only count —; set to
    1, the default child's.  Without the trial helpers (TSIM_NO_TRIAL_HELPERS=1) the option switches nothing on."""
    ref = {0: _case(runs, "off", "b1"), 1: _case(runs, "default", "b1")}
    for setting in ("default", "off"):
        for v in (0, 1):
            got = _case(runs, setting, "b1_opt%d" % v)
            assert int(got["option"]) == v
            for i in range(LAUNCHES):
                print(setting, "option set to", v, "launch", i, "helped", got["helped@%d" % i].tolist(), "reference", ref[v]["helped@%d" % i].tolist())
                for k in OUT_KEYS + ("helped",):
                    assert _same_bits(got["%s@%d" % (k, i)], ref[v]["%s@%d" % (k, i)]), (setting, v, i, k)
    for v in (0, 1):
        none = _case(runs, "no_helpers", "b1_opt%d" % v)
        for i in range(LAUNCHES):
            assert (none["helped@%d" % i] == 0).all()
            for k in OUT_KEYS:
                assert _same_bits(none["%s@%d" % (k, i)], ref[0]["%s@%d" % (k, i)]), ("no helpers", v, i, k)


def test_helpers_that_appear_mid_launch_are_used(runs):
    """rest4: a full wavefront, so nothing helps until the three environments at rest have finished — they need fewer evaluations than the one pushing
    into the box, which is helped from then on."""
    new, old = _case(runs, "default", "rest4"), _case(runs, "off", "rest4")
    for i in range(LAUNCHES):
        ev = old["evals@%d" % i]
        print("rest4 launch", i, "evals", ev.tolist(), "helped on", new["helped@%d" % i].tolist(), "off", old["helped@%d" % i].tolist())
        assert ev[0] > ev[1:].max()
        assert int(new["helped@%d" % i][0]) > int(old["helped@%d" % i][0])


def test_a_captured_episode_replays_the_eager_results(runs):
    for setting in ("default", "off"):
        r = runs[setting]
        for k in ("q", "var", "tactile", "status", "du", "evals"):
            assert _same_bits(r["graph/replay_" + k], r["b3/%s@1" % k]), (setting, k)
    assert _same_bits(runs["default"]["graph/replay_helped"], runs["default"]["b3/helped@1"])


def test_a_masked_frame_gets_its_state_and_no_tactile_frame(runs):
    r = runs["default"]
    assert r["masked_b3/q@1"].shape[0] == 3 and r["masked_b3/tactile@1"].shape[0] == 1


if __name__ == "__main__":
    _child(sys.argv[1])
