"""What the per-frame parameter Jacobians cost beside the only other route to the same matrices (profiles/r26_param_jacobians.md).

Workloads: TactilePush, B = 4096, and D'Claw, B = 2048; T = 20 frames x 5 sub-steps on the workload inputs (workloads.push_workload seed 0,
workloads.dclaw_random_workload seed 7), shared tables, generic kernels; fp32 and fp64; the dynamics columns of model.param_columns() (pair and
dof-damping columns: 15 and 22 — the sensor columns of E are exactly zero).  Timed, each with device events around the Python call (the outputs'
torch.empty included), three warm-up calls, the median (min ... max) of five windows of three calls:
    param_jacobians E alone, Ft alone, both; frame_jacobians A + B on the same tape (the same evaluation with 2 nr + nu columns);
and, one warm-up pass and the median of three passes, the same E from tangent_episode: T windows (frame f: the newest T - f frames) x
ceil(ncols / 8) launches with unit dtables columns, inputs prepared outside the clock, dq and dqd out only.
It also prints the largest difference between the two routes' E on the scale of the column half, so that the timing compares like with like.

    python tools/param_jacobian_timing.py [push|dclaw] [f32|f64] ...      (default: all four)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, S = 20, 5


def _timed(torch, fn, warm=3, windows=5, calls=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return float(np.median(out)), min(out), max(out)


def run(workload, real):
    import torch
    from tactilesimulation_amd.host.batch import BatchSim
    from tactilesimulation_amd.model.compiler import load_model
    from tactilesimulation_amd.workloads import asset, dclaw_random_workload, push_workload
    dev, dt = "cuda:0", torch.float32 if real == "f32" else torch.float64
    if workload == "push":
        m, B = load_model(asset("pusher")), 4096
        q0, u, _ = push_workload(B, T, seed=0)
    else:
        m, B = load_model(asset("dclaw_position_control")), 2048
        q0, u = dclaw_random_workload(B, T, seed=7)[:2]
    sim = BatchSim(m, B, device=dev, dtype=dt, tape_capacity=T * S)
    sim.set_static(False)
    sim.reset(torch.tensor(q0, device=dev, dtype=dt), None, backward_flag=True)
    sim.rollout(torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device=dev, dtype=dt), S)
    cols = [c for (k, _, _, c) in m.param_columns() if k != "sensor"]
    nr, nc = sim.ndof_r, len(cols)
    fl = sim.param_jacobians_launch_info()
    print("%s %s: B %d, %d frames x %d sub-steps, %d dynamics columns (%d launches), lanes %d, %d blocks / frame, %d B LDS" % (
        workload, real, B, T, S, nc, -(-nc // sim.PARAM_JACOBIAN_MAX_COLS), fl["lanes_per_env"], fl["blocks"], fl["lds_bytes"]))
    mx = sim.PARAM_JACOBIAN_MAX_COLS
    e_only = lambda: [sim.param_jacobians(T, S, cols[c0:c0 + mx]) for c0 in range(0, nc, mx)]      # noqa: E731
    rows = [("param_jacobians E", e_only),
            ("param_jacobians Ft", lambda: sim.param_jacobians(T, S, (), want_E=False, want_tactile=True)),
            ("param_jacobians E + Ft", lambda: [sim.param_jacobians(T, S, cols[c0:c0 + mx], want_tactile=c0 == 0) for c0 in range(0, nc, mx)]),
            ("frame_jacobians A + B", lambda: sim.frame_jacobians(T, S))]
    res = {}
    for name, fn in rows:
        res[name] = _timed(torch, fn)
        print("  %-28s %9.3f ms (%.3f ... %.3f)" % ((name,) + res[name]))
    # the same E from tangent_episode
    ntab = sim.base_tables().shape[1]
    dtabs = []
    for c0 in range(0, nc, 8):
        ch = cols[c0:c0 + 8]
        d = torch.zeros((len(ch), B, ntab), device=dev, dtype=dt)
        for k, c in enumerate(ch):
            d[k, :, c] = 1
        dtabs.append(d)
    ref = torch.zeros((T, B, 2 * nr, nc), device=dev, dtype=dt)

    def tangent_route():
        for f in range(T):
            for i, d in enumerate(dtabs):
                o = sim.tangent_episode(T - f, S, dtables=d, want_qd=True, want_var=False, want_tactile=False)
                ref[f, :, :nr, 8 * i:8 * i + d.shape[0]] = o["dq"][:, 0].permute(1, 2, 0)
                ref[f, :, nr:, 8 * i:8 * i + d.shape[0]] = o["dqd"][:, 0].permute(1, 2, 0)
    tt = _timed(torch, tangent_route, warm=1, windows=3, calls=1)
    print("  %-28s %9.3f ms (%.3f ... %.3f), %d launches" % (("the same E from tangent_episode",) + tt + (T * len(dtabs),)))
    print("  one launch / the tangent route: %.1f x" % (tt[0] / res["param_jacobians E"][0]))
    E = torch.cat([o["E"] for o in e_only()], 3).double()
    R = ref.double()
    worst = 0.0
    for half in (slice(0, nr), slice(nr, 2 * nr)):
        sc = R[:, :, half].abs().amax(2, keepdim=True).expand_as(R[:, :, half])
        diff = (E[:, :, half] - R[:, :, half]).abs()
        ok = sc > 0
        worst = max(worst, float((diff[ok] / sc[ok]).max()))
    print("  largest |E - tangent route| / column-half scale: %.3e" % worst)


if __name__ == "__main__":
    args = sys.argv[1:]
    for w in [a for a in args if a in ("push", "dclaw")] or ["push", "dclaw"]:
        for r in [a for a in args if a in ("f32", "f64")] or ["f32", "f64"]:
            run(w, r)
