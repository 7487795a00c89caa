"""Numbers behind profiles/r19_closed_loop_tangent.md.

    python tools/measure_closed_loop_tangent.py            timing at B = 4096, T = 20, fp32, tactile observation, ndir 1 / 4 / 8:
        FusedPushEpisode.tangent's launch (tsim_push_closed_tangent: k_closed_tangent) beside tsim_tangent_episode (k_tangent) fed the closed
        call's du on the same tape — the difference is the policy's tangent — and beside the closed-loop adjoint launch
        (tsim_push_closed_backward).  Device events around the bare C call on the current stream, five warm-up calls, then the median of five
        windows of REPS calls each (the tangent calls change nothing, so they repeat on one tape; the adjoint pops the tape, so every timed adjoint
        call has a roll-out in front of it, outside the events).
    python tools/measure_closed_loop_tangent.py --floor    the regression floor of tests/test_gpu_closed_loop_tangent.py test 3: the OPEN-loop
        transpose identity (tangent_episode against backward_episode + get_adjoint + the table-gradient buffer, the measure of
        tests/test_gpu_tangent.py::_identity_errors) on the tapes of that file's closed roll-outs, every case, default groups and all groups.  Run it
        with the library of the commit the floor is wanted for (TSIM_HIP_LIB names an older build)."""
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def floor():
    import test_gpu_closed_loop_param_grad as PG
    from param_grad_util import ALL
    from test_gpu_tangent import _identity_errors
    from tactilesimulation_amd.envs.push_closed_loop import FusedPushEpisode
    configs = [("tactile_flatten", False, 0.0), ("tactile_flatten", True, 0.0), ("tactile_flatten", False, PG.PUSH), ("tactile_flatten", True, PG.PUSH),
               ("privilege", False, 0.0), ("privilege", True, PG.PUSH), ("no_tactile", False, PG.PUSH)]      # tests/test_gpu_closed_loop_tangent.py CONFIGS
    B, T = PG.B0, PG.T0
    m = PG._model()
    worst = {}
    for dtype in (torch.float64, torch.float32):
        errs = []
        for lanes in (16, 32, 64):
            for obs, tables, push in configs:
                for body in (False, True):
                    q0, goal, dist = (torch.tensor(a, device="cuda", dtype=dtype) for a in PG._episode(B, T, PG.SEED0))
                    env = PG._env(dtype, lanes, obs, tables, B, T)
                    sim, S = env.sim, env.frame_skip
                    sim.set_param_grad_groups(ALL if body else ("contact",))
                    ep = FusedPushEpisode(env, PG._actor(obs, dtype, push), T)
                    ep.rollout(q0, goal, dist)
                    assert int((ep.status != 0).sum()) == 0
                    rng = np.random.default_rng(31)
                    t = lambda x: torch.tensor(np.ascontiguousarray(x), device="cuda", dtype=dtype)
                    base = sim.base_tables().double().cpu().numpy()
                    cols = [c for (_, _, _, c) in m.param_columns() + (m.body_param_columns() if body else [])]
                    dtab = np.zeros((3,) + base.shape)
                    dtab[:, :, cols] = rng.normal(size=(3, B, len(cols))) * (np.abs(base[:, cols]) + 0.1)
                    v = {"du": t(rng.normal(size=(3, T, B, 6))), "dq0": t(1e-2 * rng.normal(size=(3, B, 7))), "dqd0": t(1e-1 * rng.normal(size=(3, B, 7))), "dtables": t(dtab)}
                    o = sim.tangent_episode(T, S, want_qd=True, **v)
                    w = (t(rng.normal(size=(T, B, 7))), t(rng.normal(size=(T, B, 6))), t(rng.normal(size=(T, B, 390))))
                    g = torch.zeros_like(sim.base_tables())
                    sim.set_param_grad(g)
                    du = sim.backward_episode(T, S, w[0], w[1], w[2])
                    sim.set_param_grad(None)
                    lq, lv = sim.get_adjoint()
                    e = _identity_errors(o, v, w, (du, lq, lv, g))
                    errs.append(e.ravel())
                    print("open-loop identity on the closed tape %s lanes %d %s tables %d push %.1f body %d: max %.3e median %.3e" % (
                        dtype, lanes, obs, tables, push, body, e.max(), np.median(e)), flush=True)
        errs = np.concatenate(errs)
        worst[dtype] = errs.max()
        print("FLOOR %s: max %.3e p99 %.3e median %.3e over %d (environment, direction) pairs" % (dtype, errs.max(), np.quantile(errs, 0.99), np.median(errs), errs.size), flush=True)
    return worst


def timing(B=4096, T=20, reps=3):
    import test_gpu_closed_loop_param_grad as PG
    from tactilesimulation_amd.envs.push_closed_loop import FusedPushEpisode, _p
    from tactilesimulation_amd.host import capi
    dtype, obs = torch.float32, "tactile_flatten"
    q0, goal, dist = (torch.tensor(a, device="cuda", dtype=dtype) for a in PG._episode(B, T, PG.SEED0))
    env = PG._env(dtype, 0, obs, False, B, T)
    sim, S, L = env.sim, env.frame_skip, capi.lib()
    ep = FusedPushEpisode(env, PG._actor(obs, dtype, PG.PUSH), T)
    ep.rollout(q0, goal, dist)
    assert int((ep.status != 0).sum()) == 0
    print("B %d T %d x %d sub-steps fp32 %s, batch variant %s, k_closed_tangent shape %s, k_tangent shape %s" % (
        B, T, S, obs, sim.kernel_variant(), ep.tangent_launch_info(8, True), sim.tangent_launch_info(8, True)))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    m = PG._model()
    cols = [c for (_, _, _, c) in m.param_columns()]
    ntab = sim.base_tables().shape[1]

    def window(fn, before=None):
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            tot = 0.0
            for _ in range(reps):
                if before:
                    before()
                a.record()
                fn()
                b.record()
                b.synchronize()
                tot += a.elapsed_time(b)
            ms.append(tot / reps)
        return statistics.median(ms), min(ms), max(ms)

    rows = []
    for nd in (1, 4, 8):
        gen = torch.Generator().manual_seed(nd)
        r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to("cuda", dtype)
        dtab = torch.zeros(nd, B, ntab, device="cuda", dtype=dtype)
        dtab[:, :, cols] = r(nd, B, len(cols)) * 0.1
        s1, s2, s3, dtac0 = r(nd, T, B, 64), r(nd, T, B, 64), r(nd, T, B, 3), 1e-2 * r(nd, B, 390)
        new = lambda d: torch.empty(nd, T, B, d, device="cuda", dtype=dtype)
        dq, dvar, dtac, dupol, du = new(7), new(6), new(390), new(3), new(6)
        dq2, dvar2, dtac2 = new(7), new(6), new(390)

        def closed():
            capi.check(L.tsim_push_closed_tangent(sim._h, C.byref(ep._pol), _p(ep.goal), T, S, nd, _p(ep.u), _p(ep.h1), _p(ep.h2), _p(s1), _p(s2), _p(s3),
                                                  None, _p(dtac0), None, None, _p(dtab), _p(dq), None, _p(dvar), _p(dtac), _p(dupol), _p(du), st))

        def opened():
            capi.check(L.tsim_tangent_episode(sim._h, T, S, nd, None, _p(du), None, None, _p(dtab), _p(dq2), None, _p(dvar2), _p(dtac2), st))
        for _ in range(5):
            closed(); opened()
        torch.cuda.synchronize()
        tc, to = window(closed), window(opened)
        torch.cuda.synchronize()
        assert torch.equal(dq, dq2) and torch.equal(dtac, dtac2)
        rows.append((nd, tc, to))
        print("ndir %d: closed tangent %.3f ms (min %.3f max %.3f)   open-loop tangent on the same tape %.3f ms (min %.3f max %.3f)   policy tangent %.3f ms = %.1f us per frame and direction" % (
            (nd,) + tc + to + (tc[0] - to[0], 1e3 * (tc[0] - to[0]) / (T * nd))), flush=True)
    print("ndir 8 / ndir 1: closed %.2f, open-loop %.2f" % (rows[2][1][0] / rows[0][1][0], rows[2][2][0] / rows[0][2][0]))

    def backward():
        capi.check(L.tsim_push_closed_backward(sim._h, C.byref(ep._pol), _p(ep.goal), T, S, _p(ep.df_dq), _p(ep.df_dvar), _p(ep.du_direct), _p(ep.u), _p(ep.h1), _p(ep.h2),
                                               _p(ep.g1), _p(ep.g2), _p(ep.g3), _p(ep.dobs_tac), None, st))
    for _ in range(3):
        backward(); ep.rollout(q0, goal, dist)
    torch.cuda.synchronize()
    held = []

    def again():
        held.append((ep.goal, ep.q0, ep.tac0, ep._w, ep.df_dq, ep.df_dvar, ep.du_direct))
        ep.rollout(q0, goal, dist)
    backward()
    tb = window(backward, before=again)
    print("closed-loop adjoint launch (k_backward, no table gradient): %.3f ms (min %.3f max %.3f)" % tb)


if __name__ == "__main__":
    if "--floor" in sys.argv:
        floor()
    else:
        timing()
