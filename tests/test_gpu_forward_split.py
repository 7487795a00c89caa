"""An episode launch that has the order of the previous one goes out as two (csrc/tsim_hip.hip launch_forward): the heaviest eighth of its wavefronts on
the caller's stream, the others — with the read-out of their environments — on a side stream of the batch, which the caller's stream waits for.
TSIM_NO_FORWARD_SPLIT=1 at batch creation keeps the single launch.  The two must agree bit for bit: every environment is computed by the same kernels
from the same inputs, only the launch that carries it differs.

The switch is read from the environment when a batch is created, so each setting runs in a fresh child process — this file, as a script, runs EVERY
case below once and leaves the results in one .npz; the module's fixture starts the two children once and the tests compare case by case.  What is
compared, for every launch of a case: q, qd, variables, tactile frames, status, evaluation counts, dL/du and the carried adjoint (dL/dq0, dL/dqd0).  Not
the helper-trial counts: they depend on which environments share a wavefront, and the LPT order leaves that open among environments of equal cost
(csrc/tsim_hip.hip k_order_by_evals).  Every case: 3 frames (the masked one 4) of 2 sub-steps.

EVERY LAUNCH OF A CASE IS ANOTHER EPISODE (start states and actions re-seeded by the launch's index, identically in both children; the order is kept
per episode length, so the later launches still go out split).  Nothing clears the tape, the evaluation counts, the pose records or the output
buffers between launches, so with one episode repeated an environment that the split launch never simulated or never read out, and a consumer that
ran before the side stream had finished, would find exactly the bits the launch before left there; with another episode they find another episode's.
The order a launch runs in is the one the episode BEFORE left, which says nothing about the new one: the light group's forward kernel outlasts the
heavy group's as often as not, so the caller's stream really has something to wait for at the join.  (Checked against three altered libraries —
no join wait; the light read-out's range begun one wavefront late; the light forward launch one wavefront short — each of which turns this file red.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = "cuda:0"
S = 2

# case -> (kernel variant, TSIM_OPT_FRAME_RECORDS, TSIM_OPT_FORWARD_SPLIT after each launch of the default run)
CASES = {
    "static_f32_b256": ("static:pusher", 2, (0, 1)),        # 64 blocks: the smallest split; the first launch has no order yet
    "static_f32_b258": ("static:pusher", 2, (0, 0)),        # no multiple of the four environments of a wavefront
    "static_f32_b252": ("static:pusher", 2, (0, 0)),        # 63 blocks
    "param_f32_tables_b256": ("param:pusher", 2, (0, 1)),   # one parameter table per environment: a record of the read-out keeps its environment's
    "masked_b256": ("static:pusher", 2, (0, 1)),            # tactile mask with the first and the last frame masked out (tac_slot < 0)
    "static_f64_b256": ("static:pusher", 1, (0, 1)),        # fp64, two environments per wavefront: 128 blocks, the run-time form of the frame records
    "repeat3_b256": ("static:pusher", 2, (0, 1, 1)),        # reset + roll-out + adjoint of three episodes on one batch: the join, and the next launch's use of the order
    "two_streams_a": ("static:pusher", 2, (0, 1)),          # two batches driven alternately on two caller streams: a side stream per batch
    "two_streams_b": ("static:pusher", 2, (0, 1)),
}
OUT_KEYS = ("q", "qd", "var", "tactile", "status", "evals", "du", "lamq", "lamv")


# ---------------------------------------------------------------------------------------------------- the child: every case, once
def _seeds(sim, T, B, torch, mask=None):
    g = torch.Generator().manual_seed(9)
    nm = T if mask is None else int(mask.sum())
    return tuple(torch.randn(n_, B, n, generator=g, dtype=torch.float64).to(DEV, sim.dtype) for n_, n in ((T, sim.ndof_r), (T, sim.ndof_var), (nm, sim.ndof_tactile)))


def _launch(sim, q0, u, seeds, mask=None):
    """reset + roll-out + adjoint on the current stream: device tensors and the two path flags (host state, known once the calls return)"""
    sim.reset(q0, None, backward_flag=True)
    ro = dict(sim.rollout(u, S, want_qd=True, tactile_mask=mask))
    flags = (sim.get_option(sim.OPT_FRAME_RECORDS), sim.get_option(sim.OPT_FORWARD_SPLIT))
    ro["du"] = sim.backward_episode(int(u.shape[0]), S, *seeds, tactile_mask=mask)
    return ro, flags


def _collect(sim, ro, flags):
    out = {k: v.cpu().numpy() for k, v in ro.items()}
    out["evals"] = sim.last_evals().copy()
    out["lamq"], out["lamv"] = (x.cpu().numpy() for x in sim.get_adjoint())
    out["frame_records"], out["split"] = np.array(flags[0]), np.array(flags[1])
    return out


def _episodes(sim, inputs, torch, mask=None):
    """one episode per (q0, u) of inputs on one batch, each collected before the next"""
    seeds = _seeds(sim, inputs[0][1].shape[0], inputs[0][1].shape[1], torch, mask)
    return [_collect(sim, *_launch(sim, q0, u, seeds, mask)) for q0, u in inputs]


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

    def push(B, T, dtype=torch.float32, lanes=16, seed=5, launches=2):
        """a batch and the (q0, u) of `launches` different episodes for it"""
        sim = BatchSim(pusher, B, dtype=dtype, tape_capacity=T * S)
        sim.set_lanes_per_env(lanes)
        inputs = []
        for i in range(launches):
            q0, u, _ = push_workload(B, T, seed=seed + 17 * i)
            inputs.append((torch.tensor(q0, device=DEV, dtype=dtype), torch.tensor(u, device=DEV, dtype=dtype).transpose(0, 1).contiguous()))
        return sim, inputs

    def put(case, sim, outs):
        res[case + "/variant"] = np.array(sim.kernel_variant())
        res[case + "/blocks"] = np.array(sim.launch_info()["blocks"])
        for i, out in enumerate(outs):
            for k, v in out.items():
                res["%s/%s@%d" % (case, k, i)] = v

    for B in (256, 258, 252):
        sim, inputs = push(B, 3)
        put("static_f32_b%d" % B, sim, _episodes(sim, inputs, torch))
    sim, inputs = push(256, 3)
    tab = sim.base_tables()
    g = torch.Generator().manual_seed(4)
    tab[:, int(pusher.I[BL.TSIM_IH_FOFF_DOF]) + BL.TSIM_DF_DAMPING] = (0.5 + torch.rand(256, generator=g)).to(tab)
    tab[:, int(pusher.I[BL.TSIM_IH_FOFF_PAIR]) + BL.TSIM_PF_KN] *= (0.8 + 0.4 * torch.rand(256, generator=g)).to(tab)
    sim.set_env_tables(tab)
    put("param_f32_tables_b256", sim, _episodes(sim, inputs, torch))
    sim, inputs = push(256, 4)
    put("masked_b256", sim, _episodes(sim, inputs, torch, mask=torch.tensor([False, True, True, False])))
    sim, inputs = push(256, 3, dtype=torch.float64, lanes=32)
    put("static_f64_b256", sim, _episodes(sim, inputs, torch))
    sim, inputs = push(256, 3, seed=6, launches=3)
    put("repeat3_b256", sim, _episodes(sim, inputs, torch))
    # a graph (captured behind one eager episode, so the captured launch HAS the order) replayed on the SECOND episode of static_f32_b256, written
    # into its static inputs after the capture: against that case's eager second launch
    sim, inputs = push(256, 3)
    q0s, us = inputs[0][0].clone(), inputs[0][1].clone()
    ge = GraphedEpisode(sim, q0s, us, S, seeds=_seeds(sim, 3, 256, torch))
    res["graph/split_at_capture"] = np.array(sim.get_option(sim.OPT_FORWARD_SPLIT))
    q0s.copy_(inputs[1][0]); us.copy_(inputs[1][1])
    ro, du, _ = ge.replay()
    torch.cuda.synchronize()
    for k in ("q", "var", "tactile", "status"):
        res["graph/replay_" + k] = ro[k].cpu().numpy()
    res["graph/replay_du"] = du.cpu().numpy()
    # two batches, two caller streams, alternately and without a synchronisation in between; collected at the end of each round (another episode per round)
    sims = [push(256, 3, seed=7), push(256, 3, seed=8)]
    seeds = [_seeds(s[0], 3, 256, torch) for s in sims]
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream(DEV))
    outs = [[], []]
    for r in range(2):
        live = []
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                live.append(_launch(sims[i][0], *sims[i][1][r], seeds[i]))
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                outs[i].append(_collect(sims[i][0], *live[i]))
    put("two_streams_a", sims[0][0], outs[0])
    put("two_streams_b", sims[1][0], outs[1])
    torch.cuda.synchronize()
    np.savez(path, **res)


# ---------------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: the child's .npz} for the default path and for TSIM_NO_FORWARD_SPLIT=1: one fresh process each"""
    d = tmp_path_factory.mktemp("forward_split")
    procs = {}
    for setting in ("default", "single"):      # side by side: most of a child's time is start-up
        env = {k: v for k, v in os.environ.items() if k != "TSIM_NO_FORWARD_SPLIT"}
        if setting == "single":
            env["TSIM_NO_FORWARD_SPLIT"] = "1"
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


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_split_launch_equals_the_single_launch(runs, case):
    variant, frame_records, split = CASES[case]
    new, old = ({k[len(case) + 1:]: v for k, v in runs[s].items() if k.startswith(case + "/")} for s in ("default", "single"))
    assert str(new["variant"]) == variant and str(old["variant"]) == variant
    if case == "static_f32_b252":
        assert int(new["blocks"]) == 63
    elif "b258" not in case:
        assert int(new["blocks"]) == (128 if "f64" in case else 64)
    for i, want in enumerate(split):
        assert int(new["frame_records@%d" % i]) == frame_records and int(old["frame_records@%d" % i]) == frame_records
        assert int(new["split@%d" % i]) == want, "launch %d of the default run: TSIM_OPT_FORWARD_SPLIT" % i
        assert int(old["split@%d" % i]) == 0
        for k in OUT_KEYS:
            a, b = new["%s@%d" % (k, i)], old["%s@%d" % (k, i)]
            assert _same_bits(a, b), (case, i, k, float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()))
        assert np.isfinite(old["q@%d" % i]).all() and int(old["evals@%d" % i].min()) > 0 and np.abs(old["tactile@%d" % i]).max() > 0
    assert "split@%d" % len(split) not in new


def test_every_launch_of_a_case_is_another_episode(runs):
    """what the comparisons above rest on: a launch that left an environment out would find the previous EPISODE's bits there, not its own"""
    r = runs["single"]
    for case, (_, _, split) in CASES.items():
        for i in range(1, len(split)):
            for k in ("q", "du"):      # [frames, B, .]: environments whose values differ from the launch before
                d = r["%s/%s@%d" % (case, k, i)] != r["%s/%s@%d" % (case, k, i - 1)]
                assert d.any(axis=(0, 2)).all(), (case, i, k)


def test_a_captured_episode_is_one_launch_and_replays_the_eager_results(runs):
    for setting in ("default", "single"):
        r = runs[setting]
        assert int(r["graph/split_at_capture"]) == 0
        for k in ("q", "var", "tactile", "status", "du"):
            assert _same_bits(r["graph/replay_" + k], r["static_f32_b256/%s@1" % k]), (setting, k)


def test_a_masked_frame_gets_its_state_and_no_tactile_frame(runs):
    r = runs["default"]
    assert r["masked_b256/q@1"].shape[0] == 4 and r["masked_b256/var@1"].shape[0] == 4 and r["masked_b256/tactile@1"].shape[0] == 2


if __name__ == "__main__":
    _child(sys.argv[1])
