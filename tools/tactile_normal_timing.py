"""What the tactile normal equations cost beside the only other route to the same matrices (profiles/r29_tactile_normal_equations.md).

Workloads: TactilePush, B = 4096 (all 20 frames and 1 in 5), and D'Claw, B = 2048 (the last frame and all 20); T = 20 frames x 5 sub-steps on
the workload inputs (workloads.push_workload seed 0, workloads.dclaw_random_workload seed 7), shared tables, generic kernels; fp32 and fp64.
Timed with device events around each call, three warm-up calls, the median (min ... max) of 15 calls, every output and intermediate allocated
outside the timed region (the C entries are called on buffers made once):
    (i)  tsim_tactile_normal_equations: state block alone and with the sensors' parameter columns, each with and without a residual;
    (ii) the route through the Jacobians: tsim_tactile_jacobians (Ct) + tsim_param_jacobians (Ft) + the scatter of Ft to the dense F + the
         products in torch, block by block (Ct W Ct^T, Ct W F, F^T W F, Ct W r, F^T W r), so that H = [C | F] is never copied together.
D'Claw at all 20 frames: route (ii) needs 8.9 GB for Ct in fp32 and as much again for its weighted copy; it is not attempted and (i) is
reported alone.  Also: the bytes each route writes, the peak of torch's allocator over one Python-level call of each, the largest difference
between the two on yardstick A's scale, and for TactilePush the new call at 16 / 32 / 64 forced lanes.

    python tools/tactile_normal_timing.py [push|dclaw] [f32|f64] ...      (default: all four)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, S = 20, 5


def _timed(torch, fn, warm=3, calls=15):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), min(out), max(out)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _sensors(m):
    from tactilesimulation_amd.model import blob as B
    off = int(m.I[B.TSIM_IH_OFF_SENSOR])
    return [(int(m.I[off + s * B.TSIM_SI_SIZE + B.TSIM_SI_TAX0]), int(m.I[off + s * B.TSIM_SI_SIZE + B.TSIM_SI_NTAX])) for s in range(int(m.I[B.TSIM_IH_NSENSOR]))]


def run(workload, real):
    import torch
    from tactilesimulation_amd.host import capi
    from tactilesimulation_amd.host.batch import BatchSim
    from tactilesimulation_amd.model.compiler import load_model
    from tactilesimulation_amd.workloads import asset, dclaw_random_workload, push_workload
    dev, dt = "cuda:0", torch.float32 if real == "f32" else torch.float64
    esz = 4 if real == "f32" else 8
    if workload == "push":
        m, B = load_model(asset("pusher")), 4096
        q0, u, _ = push_workload(B, T, seed=0)
        masks = [("all 20 frames", None), ("1 frame in 5", [f % 5 == 4 for f in range(T)])]
    else:
        m, B = load_model(asset("dclaw_position_control")), 2048
        q0, u = dclaw_random_workload(B, T, seed=7)[:2]
        masks = [("the last frame", [f == T - 1 for f in range(T)]), ("all 20 frames", None)]
    sim = BatchSim(m, B, device=dev, dtype=dt, tape_capacity=T * S)
    sim.set_static(False)
    sim.reset(torch.tensor(q0, device=dev, dtype=dt), None, backward_flag=True)
    sim.rollout(torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device=dev, dtype=dt), S)
    L, st = capi.lib(), sim._stream()
    nr, ntac, sens = sim.ndof_r, sim.ndof_tactile, _sensors(m)
    xs, Z = 2 * nr, 2 * nr + 4 * len(sens)
    rng = np.random.default_rng(3)
    w = torch.tensor(10.0 ** rng.uniform(0, 2, size=ntac), device=dev, dtype=dt)
    for label, mask in masks:
        slots, nm = sim._tactile_slots(T, None if mask is None else torch.tensor(mask))
        r = torch.tensor(rng.normal(size=(nm, B, ntac)), device=dev, dtype=dt)
        fl = sim.tactile_normal_equations_launch_info(True)
        print("%s %s, %s: B %d, %d of %d frames x %d sub-steps, Z %d, lanes %d, %d blocks / frame, %d B LDS" % (
            workload, real, label, B, nm, T, S, Z, fl["lanes_per_env"], fl["blocks"], fl["lds_bytes"]))
        N, n = torch.empty((nm, B, Z, Z), device=dev, dtype=dt), torch.empty((nm, B, Z), device=dev, dtype=dt)
        Nx, nx = torch.empty((nm, B, xs, xs), device=dev, dtype=dt), torch.empty((nm, B, xs), device=dev, dtype=dt)

        def new(wp, res):
            No, no = (N, n) if wp else (Nx, nx)
            capi.check(L.tsim_tactile_normal_equations(sim._h, T, S, _ptr(slots), int(wp), _ptr(w), _ptr(r) if res else None, _ptr(No), _ptr(no) if res else None, st))
        for wp in (False, True):
            for res in (False, True):
                t = _timed(torch, lambda: new(wp, res))
                zz = Z if wp else xs
                print("  (i)  normal equations, %s, %s   %9.3f ms (%.3f ... %.3f)   writes %.1f MB" % (
                    "state + parameters" if wp else "state block alone ", "with r   " if res else "without r", t[0], t[1], t[2], nm * B * (zz * zz + (zz if res else 0)) * esz / 1e6))
        if workload == "push":
            for lanes in (16, 32, 64):
                sim.set_lanes_per_env(lanes)
                t = _timed(torch, lambda: new(True, True))
                print("  (i)  at %d forced lanes (kernel at %d), state + parameters, with r   %9.3f ms (%.3f ... %.3f)" % (
                    (lanes, sim.tactile_normal_equations_launch_info(True)["lanes_per_env"]) + t))
            sim.set_lanes_per_env(0)
        new(True, True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        o = sim.tactile_normal_equations(T, S, weight=w, residual=r, with_params=True, tactile_mask=None if mask is None else torch.tensor(mask))
        torch.cuda.synchronize()
        print("  (i)  peak of the allocator over one BatchSim.tactile_normal_equations call: + %.1f MB" % ((torch.cuda.max_memory_allocated() - base) / 1e6))
        del o
        ct_bytes = nm * B * xs * ntac * esz
        if workload == "dclaw" and mask is None:
            print("  (ii) not attempted: Ct alone is %.2f GB, its weighted copy as much again" % (ct_bytes / 1e9))
            continue
        # ---- (ii) the route through the Jacobians, every buffer made once
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        Ct = torch.empty((nm, B, xs, ntac), device=dev, dtype=dt)
        Ctw = torch.empty_like(Ct)
        Ft = torch.empty((nm, B, 4, ntac), device=dev, dtype=dt)
        F = torch.zeros((nm, B, ntac, 4 * len(sens)), device=dev, dtype=dt)
        Fw = torch.empty_like(F)
        N2, n2 = torch.empty_like(N), torch.empty_like(n)
        rw = torch.empty_like(r)

        def jac():
            capi.check(L.tsim_tactile_jacobians(sim._h, T, S, _ptr(slots), _ptr(Ct), st))
            capi.check(L.tsim_param_jacobians(sim._h, T, S, 0, None, _ptr(slots), None, _ptr(Ft), st))

        def scatter():
            for s, (t0, nt) in enumerate(sens):
                F[:, :, 3 * t0:3 * (t0 + nt), 4 * s:4 * s + 4] = Ft[:, :, :, 3 * t0:3 * (t0 + nt)].transpose(-1, -2)

        def products():
            torch.mul(Ct, w, out=Ctw)
            torch.mul(F, w[:, None], out=Fw)
            torch.mul(r, w, out=rw)
            N2[..., :xs, :xs] = torch.matmul(Ctw, Ct.transpose(-1, -2))
            N2[..., :xs, xs:] = torch.matmul(Ctw, F)
            N2[..., xs:, :xs] = N2[..., :xs, xs:].transpose(-1, -2)
            N2[..., xs:, xs:] = torch.matmul(Fw.transpose(-1, -2), F)
            n2[..., :xs] = torch.matmul(Ct, rw.unsqueeze(-1)).squeeze(-1)
            n2[..., xs:] = torch.matmul(F.transpose(-1, -2), rw.unsqueeze(-1)).squeeze(-1)
        tot = 0.0
        for name, fn in (("tactile_jacobians + param_jacobians (Ft)", jac), ("scatter Ft to the dense F", scatter), ("the products in torch", products)):
            t = _timed(torch, fn)
            tot += t[0]
            print("  (ii) %-42s %9.3f ms (%.3f ... %.3f)" % ((name,) + t))
        wrote = ct_bytes + Ft.numel() * esz + F.numel() * esz + Ctw.numel() * esz + Fw.numel() * esz + rw.numel() * esz + (N2.numel() + n2.numel()) * esz
        print("  (ii) the route's sum %9.3f ms, writes %.1f MB (Ct %.1f MB); peak of the allocator with its buffers: + %.1f MB" % (
            tot, wrote / 1e6, ct_bytes / 1e6, (torch.cuda.max_memory_allocated() - base) / 1e6))
        new(True, True)
        torch.cuda.synchronize()
        ne = min(B, 64)      # (the first environments: the comparison needs H in float64)
        H = torch.cat([Ct[:, :ne].transpose(-1, -2), F[:, :ne]], -1).double()
        sc = torch.einsum("...id,i,...ie->...de", H.abs(), w.double(), H.abs())
        d = (N[:, :ne].double() - N2[:, :ne].double()).abs()
        print("  largest |(i) - (ii)| / sum w |h||h| over N, %d environments: %.3e" % (ne, float((d / sc.clamp_min(1e-300))[sc > 0].max())))
        del H, sc, d, Ct, Ctw, Ft, F, Fw, N2, n2, rw
        torch.cuda.empty_cache()


if __name__ == "__main__":
    args = sys.argv[1:]
    for w_ in [a for a in args if a in ("push", "dclaw")] or ["push", "dclaw"]:
        for r_ in [a for a in args if a in ("f32", "f64")] or ["f32", "f64"]:
            run(w_, r_)
