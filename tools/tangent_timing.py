"""What a tangent launch costs beside the adjoint of the same tape (profiles/r17_tangent.md): TactilePush, B = 4096, 20 frames x 5 sub-steps, fp32,
generic kernels.  Per repetition: reset + roll-out, tsim_tangent_episode at ndir = 1, 4 and 8 (every input given, tactile output on) and at
ndir = 1 and 8 without dtables, then the generic k_backward of the same tape.  Run it under the profiler, in a run of its own without counters and under a time limit of its own (it takes well under a minute), then summarise the kernel trace (the three
k_tangent launches of a repetition are one instantiation: they are told apart by their order):

    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/tangent_timing.py
    python tools/tangent_timing.py --summarise OUT
"""
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NDIRS, REPS = (1, 4, 8), 4
NOTAB = (1, 8)      # ... and ndir = 1, 8 once more without dtables (no parameter term: control and start-state sensitivities only)


def run(B=4096, T=20, S=5):
    import torch
    from tactilesimulation_amd.host.batch import BatchSim
    from tactilesimulation_amd.model.compiler import load_model
    from tactilesimulation_amd.workloads import asset, push_workload
    m = load_model(asset("pusher"))
    sim = BatchSim(m, B, device="cuda:0", dtype=torch.float32, tape_capacity=T * S)
    sim.set_static(False)
    q0, u, _ = push_workload(B, T, seed=1)
    q0 = torch.tensor(q0, device="cuda:0", dtype=torch.float32)
    ut = torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device="cuda:0", dtype=torch.float32)
    g = torch.Generator(device="cuda:0").manual_seed(0)
    rnd = lambda *s: torch.randn(s, device="cuda:0", dtype=torch.float32, generator=g)
    ntab = sim.base_tables().shape[1]
    cols = torch.tensor([c for (_, _, _, c) in m.param_columns()], device="cuda:0")
    w = (rnd(T, B, sim.ndof_r), rnd(T, B, sim.ndof_var), rnd(T, B, sim.ndof_tactile))
    for _ in range(REPS + 1):                      # the first repetition is the warm-up
        sim.reset(q0, None, backward_flag=True)
        sim.rollout(ut, S)
        for nd in NDIRS:
            dt = torch.zeros((nd, B, ntab), device="cuda:0", dtype=torch.float32)
            dt[:, :, cols] = rnd(nd, B, cols.numel())
            sim.tangent_episode(T, S, du=rnd(nd, T, B, sim.ndof_u), dq0=rnd(nd, B, sim.ndof_r), dqd0=rnd(nd, B, sim.ndof_r), dtables=dt)
        for nd in NOTAB:
            sim.tangent_episode(T, S, du=rnd(nd, T, B, sim.ndof_u), dq0=rnd(nd, B, sim.ndof_r), dqd0=rnd(nd, B, sim.ndof_r))
        sim.backward_episode(T, S, *w)
        torch.cuda.synchronize()
    print("tangent_timing: %d repetitions of ndir %s + k_backward, variant %s, lanes %d" % (REPS, NDIRS, sim.kernel_variant(), sim.launch_info()["lanes_per_env"]))


def summarise(out):
    files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + out
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
    tan = [r for r in rows if "k_tangent" in r["Kernel_Name"]]
    bwd = [r for r in rows if "k_backward" in r["Kernel_Name"]]
    per = len(NDIRS) + len(NOTAB)
    assert len(tan) == per * (REPS + 1) and len(bwd) == REPS + 1, (len(tan), len(bwd))
    tb = float(np.median([ms(r) for r in bwd[1:]]))
    print("kernel                      ms per launch (median of %d)   / k_backward" % REPS)
    print("%-60s %8.3f   1.00" % (bwd[0]["Kernel_Name"][:60], tb))
    t = {}
    for i, (nd, tab) in enumerate([(n, True) for n in NDIRS] + [(n, False) for n in NOTAB]):
        t[nd, tab] = float(np.median([ms(r) for r in tan[per + i::per]]))
        print("%-60s %8.3f   %.2f" % (tan[0]["Kernel_Name"][:36] + " ndir=%d%s" % (nd, "" if tab else " no dtables"), t[nd, tab], t[nd, tab] / tb))
    for tab in (True, False):
        d = (t[8, tab] - t[1, tab]) / 7
        print("per added direction%s: %.3f ms (ndir 1 -> 8), %.2f of k_backward" % ("" if tab else ", no dtables", d, d / tb))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        run()
