"""Time-varying LQR around a recorded TactilePush roll-out, from the per-frame transition Jacobians (include/tsim.h tsim_frame_jacobians,
BatchSim.frame_jacobians): record T frames of the push workload, take A_f = dx_{f+1} / dx_f and B_f = dx_{f+1} / du_f of every frame and
environment in ONE launch, run the batched Riccati recursion in torch, and replay the episode frame by frame from perturbed start states — once
open loop (u = u_ref) and once with u = u_ref - K_f (x - x_ref).  Only the robot's three action channels are fed back; the workload's external
disturbance channels are left as recorded.  Prints the final state deviation of both replays and the per-frame spectral norm of A_f.

    python examples/push_tvlqr.py [--envs 64] [--frames 20] [--sigma 2e-3]

It is a demonstration, not a test: there is no threshold.  What it printed on an MI355X is in profiles/r22_frame_jacobians.md."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tactilesimulation_amd.functions import episode_transition      # noqa: E402
from tactilesimulation_amd.host.batch import BatchSim      # noqa: E402
from tactilesimulation_amd.model.compiler import load_model      # noqa: E402
from tactilesimulation_amd.workloads import asset, push_workload      # noqa: E402

CTRL = (0, 1, 2)      # the robot's action channels of the workload's u (3, 4: the external disturbance; 5: unused)


def riccati(A, B, Q, R, Qf):
    """gains K [T, nenv, nc, nx] of the finite-horizon discrete LQR  min sum x'Qx + u'Ru + x_T'Qf x_T,  x_{f+1} = A_f x_f + B_f u_f, batched over
    the environments"""
    T = A.shape[0]
    P = Qf.expand(A.shape[1], -1, -1).clone()
    K = []
    for f in reversed(range(T)):
        BtP = B[f].transpose(1, 2) @ P
        Kf = torch.linalg.solve(R + BtP @ B[f], BtP @ A[f])
        P = Q + A[f].transpose(1, 2) @ P @ (A[f] - B[f] @ Kf)
        P = 0.5 * (P + P.transpose(1, 2))
        K.append(Kf)
    return torch.stack(K[::-1], 0)


def run(nenv=64, T=20, S=5, sigma=2e-3, seed=0, device="cuda:0", verbose=True):
    dt = torch.float64
    m = load_model(asset("pusher"))
    sim = BatchSim(m, nenv, device=device, dtype=dt, tape_capacity=T * S)
    q0, u, _ = push_workload(nenv, T, seed=seed + 1)
    u[:, :, 0] = 0.9                                                          # the pad is driven into the box
    q0 = torch.tensor(q0, device=device, dtype=dt)
    ut = torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device=device, dtype=dt)
    # 1. the recorded roll-out and its reference states x_f = (q, qd), f = 0 .. T
    sim.reset(q0, None, backward_flag=True)
    out = sim.rollout(ut, S, want_qd=True)
    xref = torch.cat([torch.cat([q0, torch.zeros_like(q0)], 1).unsqueeze(0), torch.cat([out["q"], out["qd"]], 2)], 0)
    # 2. the local linearisation of every frame, one launch
    A, Bm = episode_transition(sim, T, S)
    Bc = Bm[..., list(CTRL)]
    nx = A.shape[2]
    # 3. the Riccati recursion: positions weigh more than velocities, a cheap control
    nr = nx // 2
    qdiag = torch.cat([torch.full((nr,), 1.0), torch.full((nr,), 1e-4)]).to(device=device, dtype=dt)
    Q, R = torch.diag(qdiag), 1e-6 * torch.eye(len(CTRL), device=device, dtype=dt)
    K = riccati(A, Bc, Q, R, 10.0 * Q)
    # 4. replays from perturbed start states (a few mm / mrad)
    rng = np.random.default_rng(seed + 2)
    dq0 = torch.tensor(sigma * rng.normal(size=tuple(q0.shape)), device=device, dtype=dt)

    def replay(feedback):
        sim.reset(q0 + dq0, None, backward_flag=False)
        x = torch.cat([q0 + dq0, torch.zeros_like(q0)], 1)
        for f in range(T):
            uf = ut[f].clone()
            if feedback:
                uf[:, list(CTRL)] -= (K[f] @ (x - xref[f]).unsqueeze(2)).squeeze(2)
                uf[:, list(CTRL)] = uf[:, list(CTRL)].clamp(-1.0, 1.0)
            o = sim.step(uf, S, want_qd=True, want_var=False, want_tactile=False)
            x = torch.cat([o["q"], o["qd"]], 1)
        return (x - xref[T])

    dev_open, dev_closed = replay(False), replay(True)
    norms = torch.linalg.matrix_norm(A, ord=2)                                # [T, nenv]
    res = {"open_q": dev_open[:, :nr].norm(dim=1).cpu().numpy(), "closed_q": dev_closed[:, :nr].norm(dim=1).cpu().numpy(),
           "start_q": dq0.norm(dim=1).cpu().numpy(), "norm_A": norms.cpu().numpy(), "K_max": float(K.abs().max())}
    if verbose:
        pr = lambda k: "median %.3e  max %.3e" % (np.median(res[k]), res[k].max())
        print("TactilePush fp64, %d environments, %d frames of %d sub-steps; start perturbed by sigma = %g per dof" % (nenv, T, S, sigma))
        print("|dq| at the start            : " + pr("start_q"))
        print("|dq| at the end, open loop   : " + pr("open_q"))
        print("|dq| at the end, TVLQR       : " + pr("closed_q"))
        print("environments where TVLQR ends closer than open loop: %d of %d" % (int((res["closed_q"] < res["open_q"]).sum()), nenv))
        print("largest gain entry |K|       : %.3e" % res["K_max"])
        print("spectral norm of A_f per frame (median / max over the environments), and the product over the episode:")
        for f in range(T):
            print("  frame %2d: %.4f / %.4f" % (f, np.median(res["norm_A"][f]), res["norm_A"][f].max()))
        prod = res["norm_A"].prod(0)
        print("  product : median %.3e  max %.3e" % (np.median(prod), prod.max()))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--sigma", type=float, default=2e-3)
    a = ap.parse_args()
    run(nenv=a.envs, T=a.frames, sigma=a.sigma)
