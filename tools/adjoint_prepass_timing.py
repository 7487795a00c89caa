"""The adjoint side of a TactilePush episode with the seed pre-pass on and off (csrc/tsim_adjoint_pre.h, profiles/r30_adjoint_prepass.md).

The library's events (tsim_kernel_timing) bracket the whole adjoint side as `k_backward`: k_adjoint_seeds + k_backward_pre with the pre-pass, k_backward
alone without.  Prints the median (min ... max) of both over `calls` episodes and their difference; the durations of the single kernels come from
a kernel trace of bench.py (one rocprofv3 --kernel-trace --stats run per setting).

    python tools/adjoint_prepass_timing.py [B [T [S]]]      (default 4096 20 5, the bench's batch)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from tactilesimulation_amd.host.batch import BatchSim
    from tactilesimulation_amd.model.compiler import load_model
    from tactilesimulation_amd.workloads import PUSHER_BLOB, push_workload
    B, T, S = (int(a) for a in (sys.argv[1:4] + ["4096", "20", "5"][len(sys.argv[1:4]):]))
    dt, calls = torch.float32, 15
    q0_np, u_np, _ = push_workload(B, T, seed=0)
    sim = BatchSim(load_model(PUSHER_BLOB), B, dtype=dt, tape_capacity=T * S)
    q0 = torch.tensor(q0_np, device="cuda", dtype=dt)
    u = torch.tensor(u_np, device="cuda", dtype=dt).transpose(0, 1).contiguous()
    w = [torch.ones(T, B, d, device="cuda", dtype=dt) for d in (sim.ndof_r, sim.ndof_var, sim.ndof_tactile)]
    sim.kernel_timing(True)
    res = {}
    for on in (1, 0, 1, 0):
        sim.set_option(sim.OPT_ADJOINT_PREPASS, on)
        ms = []
        for k in range(calls + 3):
            sim.reset(q0, None, backward_flag=True)
            sim.rollout(u, S)
            sim.kernel_times()
            sim.backward_episode(T, S, *w)
            torch.cuda.synchronize()
            assert sim.get_option(sim.OPT_ADJOINT_PREPASS) == on
            t = sim.kernel_times()["k_backward"]
            if k >= 3:
                ms.append(t[0] / max(t[1], 1))
        res.setdefault(on, []).extend(ms)
    for on in (1, 0):
        print("B %d, %d x %d: adjoint side, pre-pass %s   %.4f ms (%.4f ... %.4f)" % (B, T, S, "on " if on else "off", float(np.median(res[on])), min(res[on]), max(res[on])))
    print("difference of the medians: %.4f ms per launch" % (float(np.median(res[0])) - float(np.median(res[1]))))


if __name__ == "__main__":
    main()
