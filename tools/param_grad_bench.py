"""Cost of the parameter gradient (include/tsim.h tsim_set_param_grad): backward_episode of an open-loop episode with and without the table
gradient, device events, median of 5 windows.  Default: TactilePush at B = 4096 fp32 (param:pusher with per-environment tables), 20 frames x 5
sub-steps; --model stable_grasp / tactile_insertion for the other two; --groups contact,inertial,motor,limit (or all) for the body groups' pass as
well (BatchSim.set_param_grad_groups; default: contact).  One JSON line per configuration (profiles/r07_param_grad.md)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tactilesimulation_amd.host.batch import BatchSim      # noqa: E402
from tactilesimulation_amd.model.compiler import load_model      # noqa: E402
from tactilesimulation_amd.workloads import asset, push_workload, insertion_workload      # noqa: E402


def inputs(name, m, B, T):
    if name == "pusher":
        q0, u, _ = push_workload(B, T, seed=11)
        return q0, u, 5
    if name == "tactile_insertion":
        q0, u = insertion_workload(B, T, seed=7)
        return q0, u, 5
    q0 = np.zeros((B, m.ndof_r)); u = np.zeros((B, T, m.ndof_u)); u[:, :, -2:] = 1.0
    return q0, u, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="pusher")
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", default="contact", help="comma-separated groups of the table gradient, or 'all'")
    a = ap.parse_args()
    m = load_model(asset(a.model))
    q0, u, S = inputs(a.model, m, a.B, a.frames)
    T = a.frames
    sim = BatchSim(m, a.B, dtype=torch.float32, tape_capacity=T * S)
    tab = sim.base_tables()
    sim.set_env_tables(tab)
    groups = tuple(BatchSim.PARAM_GRAD_GROUPS) if a.groups == "all" else tuple(a.groups.split(","))
    sim.set_param_grad_groups(groups)
    dev = sim.device
    q0t = torch.tensor(q0, device=dev, dtype=torch.float32)
    ut = torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device=dev, dtype=torch.float32)
    g = torch.zeros_like(tab)
    wq = torch.randn(T, a.B, m.ndof_r, device=dev)
    wt = torch.randn(T, a.B, m.ndof_tactile, device=dev) if m.ndof_tactile else None
    res = {"model": a.model, "B": a.B, "frames": T, "substeps": S, "variant": sim.kernel_variant(), "groups": list(groups)}
    for on in (False, True, False, True):
        times = []
        for _ in range(a.windows):
            tot = 0.0
            for _ in range(a.reps):
                sim.reset(q0t, None, backward_flag=True)
                sim.rollout(ut, S, want_var=False)
                sim.set_param_grad(g if on else None)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sim.backward_episode(T, S, wq, None, wt)
                e1.record()
                torch.cuda.synchronize()
                tot += e0.elapsed_time(e1)
                sim.set_param_grad(None)
            times.append(tot / a.reps)
        res["with_grad_ms" if on else "without_ms"] = float(np.median(times))
    res["param_pass_ms"] = res["with_grad_ms"] - res["without_ms"]
    res["ratio_to_adjoint"] = res["param_pass_ms"] / res["without_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
