"""What a tangent launch costs beside the adjoint of the same tape (profiles/r17_tangent.md): TactilePush, B = 4096, 20 frames x 5 sub-steps, fp32,
generic kernels.  Per repetition: reset + roll-out, tsim_tangent_episode at ndir = 1, 4 and 8 (every input given, tactile output on) and at
ndir = 1 and 8 without dtables, then the generic k_backward of the same tape.  Run it under the profiler, in a run of its own without counters and under a time limit of its own (it takes well under a minute), then summarise the kernel trace (the three
k_tangent launches of a repetition are one instantiation: they are told apart by their order):

    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/tangent_timing.py
    python tools/tangent_timing.py --summarise OUT

--body (profiles/r18_tangent_body.md): every repetition then switches every body group on (tsim_set_param_grad_groups) and launches ndir = 1, 4 and 8
once more with directions on the body columns too — k_tangent_body_src, then k_tangent_src — and the adjoint with the table-gradient buffer set, whose
k_param_grad_body is the pre-pass's transpose.  The launches of the default mask come first and are the same with and without --body, so a library
built from another commit can be timed beside this one with the plain command; --summarise prints the minimum, maximum and spread of the
repetitions' k_tangent launches for that comparison.

    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/tangent_timing.py --body
    python tools/tangent_timing.py --summarise OUT --body
"""
import csv
import glob
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NDIRS, REPS = (1, 4, 8), 4
NOTAB = (1, 8)      # ... and ndir = 1, 8 once more without dtables (no parameter term: control and start-state sensitivities only)


def run(B=4096, T=20, S=5, body=False):
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
    bcols = torch.tensor([c for (_, _, _, c) in m.param_columns() + m.body_param_columns()], device="cuda:0")
    gtab = torch.zeros((B, ntab), device="cuda:0", dtype=torch.float32)
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
        if body:      # every body group on: the pre-pass and k_tangent_src, then the adjoint with both parameter passes (it pops the tape)
            sim.set_param_grad_groups(("contact", "inertial", "motor", "limit"))
            for nd in NDIRS:
                dt = torch.zeros((nd, B, ntab), device="cuda:0", dtype=torch.float32)
                dt[:, :, bcols] = rnd(nd, B, bcols.numel())
                sim.tangent_episode(T, S, du=rnd(nd, T, B, sim.ndof_u), dq0=rnd(nd, B, sim.ndof_r), dqd0=rnd(nd, B, sim.ndof_r), dtables=dt)
            sim.set_param_grad(gtab)
            sim.backward_episode(T, S, *w)
            sim.set_param_grad(None)
            sim.set_param_grad_groups(("contact",))
        else:
            sim.backward_episode(T, S, *w)
        torch.cuda.synchronize()
    print("tangent_timing: %d repetitions of ndir %s + k_backward, variant %s, lanes %d" % (REPS, NDIRS, sim.kernel_variant(), sim.launch_info()["lanes_per_env"]))


def summarise(out, body=False):
    files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + out
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
    named = lambda k: [r for r in rows if re.search(r"\b%s<" % k, r["Kernel_Name"])]
    tan, bwd = named("k_tangent"), named("k_backward") + named("k_backward_z")
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
    print("k_tangent, default mask, the %d timed launches each:" % REPS)
    for i, nd in enumerate(NDIRS):
        x = [ms(r) for r in tan[per + i::per]]
        print("  ndir=%d  %s  min %.3f max %.3f spread %.3f median %.3f ms" % (nd, " ".join("%.3f" % v for v in x), min(x), max(x), max(x) - min(x), float(np.median(x))))
    if not body:
        return
    src, tsrc, pgb = named("k_tangent_body_src"), named("k_tangent_src"), named("k_param_grad_body")
    assert len(src) == len(tsrc) == len(NDIRS) * (REPS + 1) and len(pgb) == REPS + 1, (len(src), len(tsrc), len(pgb))
    tp = float(np.median([ms(r) for r in pgb[1:]]))
    print("%-60s %8.3f   (its transpose: the ratios below are to it)" % (pgb[0]["Kernel_Name"][:60], tp))
    for i, nd in enumerate(NDIRS):
        a, b = float(np.median([ms(r) for r in src[len(NDIRS) + i::len(NDIRS)]])), float(np.median([ms(r) for r in tsrc[len(NDIRS) + i::len(NDIRS)]]))
        print("%-60s %8.3f   %.2f   (k_tangent_src behind it: %.3f ms, the default mask's k_tangent %.3f)" % (
            src[0]["Kernel_Name"][:40] + " ndir=%d" % nd, a, a / tp, b, t[nd, True]))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2], body="--body" in sys.argv[3:])
    else:
        run(body="--body" in sys.argv[1:])
