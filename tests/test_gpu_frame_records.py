"""Episode launches of a fused compiled-in model that record a tape end no frame inside k_forward: k_frame_records writes q, qd, the variables and the
frames' pose records afterwards, from the tape (csrc/tsim_kernels.h; csrc/tsim_hip.hip launch_forward).  TSIM_INKERNEL_FRAME_OUT=1 at batch creation
keeps the frame end in the kernel.  The two must agree bit for bit, and the launches out of the new path's scope (no tape; generic kernels) must not
have moved.

The switch is read from the environment when a batch is created, so each setting runs in a fresh child process — this file, as a script, runs EVERY
case below once and leaves the results in one .npz; the module's fixture starts the two children once and the tests compare case by case.  What is
compared: q, qd, variables, tactile frames, status, evaluation counts, and the tape — through the adjoint that is computed from it with
fixed seeds (dL/du and the carried adjoint are functions of every taped q, qd, H, K and u; the library has no call that copies a tape out).  Not the
helper-trial counts: they depend on which environments share a wavefront, and the LPT order leaves that open among environments of equal cost
(csrc/tsim_hip.hip k_order_by_evals)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = "cuda:0"

# case -> (kernel variant, TSIM_OPT_FRAME_RECORDS of the default run: 0 in the kernel, 1 after it, 2 after it and k_forward_fr)
CASES = {
    "static_f32_b5": ("static:pusher", 2),        # B = 5 at four environments per wavefront: the second wavefront has three idle slots
    "static_f32_b260_lpt": ("static:pusher", 2),   # B >= 256, launched twice: the second launch runs in the LPT order (slot <-> environment is a permutation)
    "static_f32_options": ("static:pusher", 1),   # an option off its default: the run-time switch (FwdArgs::frame_rec) of the run-time-option kernel
    "static_f64_b6": ("static:pusher", 1),        # fp64, two environments per wavefront
    "param_f32_tables_b8": ("param:pusher", 2),   # one parameter table per environment: a slot of k_frame_records keeps its environment's
    "masked_b8": ("static:pusher", 2),            # tactile mask with the first and the last frame masked out (tac_slot < 0)
    "graph_b8": ("static:pusher", 2),             # one HIP-graph replay against the eager calls
    "forward_only_b8": ("static:pusher", 0),      # no tape: out of scope, in-kernel as before
    "generic_ball_push": ("generic", 0),          # generic kernels: out of scope
}


# ---------------------------------------------------------------------------------------------------- the child: every case, once
def _episode(sim, q0, u, S, torch, record=True, mask=None, launches=1):
    """reset + roll-out (+ adjoint with fixed seeds), `launches` times; the last launch's results as numpy arrays"""
    T, B = u.shape[0], u.shape[1]
    g = torch.Generator().manual_seed(9)
    nm = T if mask is None else int(mask.sum())
    wq = torch.randn(T, B, sim.ndof_r, generator=g, dtype=torch.float64).to(DEV, sim.dtype)
    wv = torch.randn(T, B, sim.ndof_var, generator=g, dtype=torch.float64).to(DEV, sim.dtype) if sim.ndof_var else None
    wt = torch.randn(nm, B, sim.ndof_tactile, generator=g, dtype=torch.float64).to(DEV, sim.dtype) if sim.ndof_tactile else None
    for _ in range(launches):
        sim.reset(q0, None, backward_flag=record)
        ro = sim.rollout(u, S, want_qd=True, tactile_mask=mask)
        out = {k: v.cpu().numpy() for k, v in ro.items()}
        out["frame_records"] = np.array(sim.get_option(sim.OPT_FRAME_RECORDS))
        out["evals"] = sim.last_evals().copy()
        if record:
            assert sim.tape_len() == T * S
            out["du"] = sim.backward_episode(T, S, wq, wv, wt, tactile_mask=mask).cpu().numpy()
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

    def push(B, T, S, dtype=torch.float32, lanes=16, seed=5, **kw):
        q0, u, _ = push_workload(B, T, seed=seed)
        sim = BatchSim(pusher, B, dtype=dtype, tape_capacity=T * S if kw.get("record", True) else 0)
        sim.set_lanes_per_env(lanes)
        return sim, torch.tensor(q0, device=DEV, dtype=dtype), torch.tensor(u, device=DEV, dtype=dtype).transpose(0, 1).contiguous()

    def put(case, sim, out):
        out["variant"] = np.array(sim.kernel_variant())
        for k, v in out.items():
            res[case + "/" + k] = v

    sim, q0, u = push(5, 3, 2)
    put("static_f32_b5", sim, _episode(sim, q0, u, 2, torch))
    sim, q0, u = push(260, 2, 5)
    put("static_f32_b260_lpt", sim, _episode(sim, q0, u, 5, torch, launches=2))
    sim, q0, u = push(9, 3, 2)
    sim.set_option(sim.OPT_VALUE_TRIALS, 1)
    put("static_f32_options", sim, _episode(sim, q0, u, 2, torch))
    sim, q0, u = push(6, 3, 2, dtype=torch.float64, lanes=32)
    put("static_f64_b6", sim, _episode(sim, q0, u, 2, torch))
    sim, q0, u = push(8, 3, 2)
    tab = sim.base_tables()
    g = torch.Generator().manual_seed(4)
    tab[:, int(pusher.I[BL.TSIM_IH_FOFF_DOF]) + BL.TSIM_DF_DAMPING] = (0.5 + torch.rand(8, generator=g)).to(tab)
    tab[:, int(pusher.I[BL.TSIM_IH_FOFF_PAIR]) + BL.TSIM_PF_KN] *= (0.8 + 0.4 * torch.rand(8, generator=g)).to(tab)
    sim.set_env_tables(tab)
    put("param_f32_tables_b8", sim, _episode(sim, q0, u, 2, torch))
    sim, q0, u = push(8, 4, 2)
    put("masked_b8", sim, _episode(sim, q0, u, 2, torch, mask=torch.tensor([False, True, True, False])))
    # a graph replay and the eager calls, both in this process (this setting)
    sim, q0, u = push(8, 3, 2)
    eager = _episode(sim, q0, u, 2, torch, launches=2)
    sim, q0, u = push(8, 3, 2)
    g = torch.Generator().manual_seed(9)
    seeds = tuple(torch.randn(3, 8, n, generator=g, dtype=torch.float64).to(DEV, torch.float32) for n in (sim.ndof_r, sim.ndof_var, sim.ndof_tactile))
    ge = GraphedEpisode(sim, q0, u, 2, seeds=seeds)
    ro, du, _ = ge.replay()
    torch.cuda.synchronize()
    put("graph_b8", sim, eager)
    for k in ("q", "var", "tactile", "status"):
        res["graph_b8/replay_" + k] = ro[k].cpu().numpy()
    res["graph_b8/replay_du"] = du.cpu().numpy()
    res["graph_b8/replay_frame_records"] = np.array(sim.get_option(sim.OPT_FRAME_RECORDS))
    sim, q0, u = push(8, 3, 2, record=False)
    put("forward_only_b8", sim, _episode(sim, q0, u, 2, torch, record=False))
    ball = load_model(os.path.join(HERE, "models", "ball_push.xml"))
    rng = np.random.default_rng(3)
    q0 = np.tile(np.array([0, 0, 0, 0, 0, 0, 0.3, -0.2, 0.5]), (3, 1)) + 0.02 * rng.normal(size=(3, 9)) * np.array([0, 0, 0, 0.05, 0.05, 0, 1, 1, 1])
    u = np.stack([[[0.3 * np.sin(t + e), 0.25 * np.cos(t - e), -0.4] for t in range(4)] for e in range(3)])
    sim = BatchSim(ball, 3, dtype=torch.float32, tape_capacity=4 * 3)
    put("generic_ball_push", sim, _episode(sim, torch.tensor(q0, device=DEV, dtype=torch.float32),
                                           torch.tensor(u, device=DEV, dtype=torch.float32).transpose(0, 1).contiguous(), 3, torch))
    torch.cuda.synchronize()
    np.savez(path, **res)


# ---------------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: the child's .npz} for the default path and for TSIM_INKERNEL_FRAME_OUT=1: one fresh process each"""
    d = tmp_path_factory.mktemp("frame_records")
    procs = {}
    for setting in ("default", "inkernel"):      # side by side: most of a child's time is start-up
        env = {k: v for k, v in os.environ.items() if k != "TSIM_INKERNEL_FRAME_OUT"}
        if setting == "inkernel":
            env["TSIM_INKERNEL_FRAME_OUT"] = "1"
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
def test_frame_records_equal_the_in_kernel_frame_end(runs, case):
    variant, path = CASES[case]
    new, old = ({k[len(case) + 1:]: v for k, v in runs[s].items() if k.startswith(case + "/")} for s in ("default", "inkernel"))
    assert str(new["variant"]) == variant and str(old["variant"]) == variant
    assert int(new["frame_records"]) == path, "the default run did not take the path this case is about"
    assert int(old["frame_records"]) == 0
    skip = ("variant", "frame_records", "replay_frame_records")      # (which path ran: asserted above, different by design)
    keys = sorted(k for k in old if k not in skip)
    assert set(keys) >= {"q", "qd", "status", "evals"} and sorted(k for k in new if k not in skip) == keys
    if case not in ("forward_only_b8",):
        assert {"du", "lamq", "lamv"} <= set(keys)
    if case != "generic_ball_push":
        assert {"var", "tactile"} <= set(keys) and np.abs(old["tactile"]).max() > 0
    for k in keys:
        assert _same_bits(new[k], old[k]), (case, k, float(np.abs(new[k].astype(np.float64) - old[k].astype(np.float64)).max()))
    assert np.isfinite(old["q"]).all() and int(old["evals"].min()) > 0


def test_a_graph_replay_equals_the_eager_calls_on_the_new_path(runs):
    r = {k[len("graph_b8/"):]: v for k, v in runs["default"].items() if k.startswith("graph_b8/")}
    assert int(r["replay_frame_records"]) == 2 and int(r["frame_records"]) == 2
    for k in ("q", "var", "tactile", "status", "du"):
        assert _same_bits(r["replay_" + k], r[k]), k


def test_a_masked_frame_gets_its_state_and_no_tactile_frame(runs):
    r = {k[len("masked_b8/"):]: v for k, v in runs["default"].items() if k.startswith("masked_b8/")}
    assert r["q"].shape[0] == 4 and r["var"].shape[0] == 4 and r["tactile"].shape[0] == 2
    full = {k[len("static_f32_b5/"):]: v for k, v in runs["default"].items() if k.startswith("static_f32_b5/")}
    assert full["tactile"].shape[0] == 3


if __name__ == "__main__":
    _child(sys.argv[1])
