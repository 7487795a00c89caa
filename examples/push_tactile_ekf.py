"""A linearised Kalman filter around a recorded TactilePush roll-out whose sensor is the tactile pad, from the per-frame transition Jacobians
(BatchSim.frame_jacobians / functions.episode_transition) and the per-frame tactile Jacobians (include/tsim.h tsim_tactile_jacobians,
functions.episode_observation): record T frames of the push workload with their tactile frames, take (A_f, B_f) and C_f = dtactile / dx at each
frame's end in ONE launch each, replay the episode open loop from start states whose BOX pose is perturbed (the robot does not know where the box
is), and estimate the deviation dx_f = x_f - x_ref_f of every replay from the difference between its tactile frames and the reference's alone:

    predict   x^- = A_f x^ ,  P^- = A_f P A_f^T + Q                       (the controls are the recorded ones: du = 0)
    update    P^-1 = (P^-)^-1 + C_f^T R^-1 C_f ,  P^-1 x^ = (P^-)^-1 x^- + C_f^T R^-1 y_f ,   y_f = tactile_f - tactile_ref_f

batched over the environments in torch, in information form: C_f^T R^-1 C_f is 2 nr x 2 nr whatever the pad's size.  Prints the error of the
estimated box pose (x, y, z, angle: dofs 3 .. 6) at the end with the tactile update and without it (prediction alone, which stays at the prior).

    python examples/push_tactile_ekf.py [--envs 64] [--frames 20] [--sigma 2e-3]

It is a demonstration, not a test: there is no threshold.  What it printed on an MI355X is in profiles/r25_tactile_jacobians.md."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tactilesimulation_amd.functions import episode_observation, episode_transition      # noqa: E402
from tactilesimulation_amd.host.batch import BatchSim      # noqa: E402
from tactilesimulation_amd.model.compiler import load_model      # noqa: E402
from tactilesimulation_amd.workloads import asset, push_workload      # noqa: E402

BOX = (3, 4, 5, 6)      # the box's dofs of the pusher model: translation x y z, rotation


def run(nenv=64, T=20, S=5, sigma=2e-3, seed=0, device="cuda:0", verbose=True):
    dt = torch.float64
    m = load_model(asset("pusher"))
    sim = BatchSim(m, nenv, device=device, dtype=dt, tape_capacity=T * S)
    q0, u, _ = push_workload(nenv, T, seed=seed + 1)
    u[:, :, 0] = 0.9                                                          # the pad is driven into the box
    q0 = torch.tensor(q0, device=device, dtype=dt)
    ut = torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device=device, dtype=dt)
    nr = sim.ndof_r
    nx = 2 * nr
    # 1. the recorded roll-out: reference states x_f = (q, qd) and tactile frames at the end of every frame
    sim.reset(q0, None, backward_flag=True)
    ref = sim.rollout(ut, S, want_qd=True)
    xref = torch.cat([ref["q"], ref["qd"]], 2)                                # [T, nenv, nx]: x_{f+1}
    # 2. the linearisation: dynamics and measurement, one launch each
    A, _ = episode_transition(sim, T, S)
    C = episode_observation(sim, T, S)                                        # [T, nenv, ntac, nx], the transposed view of Ct
    Ct = C.transpose(-1, -2)                                                  # [T, nenv, nx, ntac], contiguous
    # 3. replays from start states with the box displaced; their states are the truth, their tactile frames the measurements
    rng = np.random.default_rng(seed + 2)
    dq0 = torch.zeros_like(q0)
    dq0[:, [3, 4, 6]] = torch.tensor(sigma * rng.normal(size=(nenv, 3)), device=device, dtype=dt)
    sim.reset(q0 + dq0, None, backward_flag=False)
    rep = sim.rollout(ut, S, want_qd=True)
    dx_true = torch.cat([rep["q"], rep["qd"]], 2) - xref                      # [T, nenv, nx]
    y = rep["tactile"] - ref["tactile"]                                       # [T, nenv, ntac]
    loaded = ref["tactile"].abs() > 0
    r = 0.05 * float(ref["tactile"][loaded].pow(2).mean().sqrt()) if bool(loaded.any()) else 1.0      # 5 % of a loaded taxel's typical force
    # 4. the filter, with and without the tactile update
    p0 = torch.full((nx,), 1e-10, device=device, dtype=dt)
    p0[[3, 4, 6]] = sigma ** 2
    Q = 1e-12 * torch.eye(nx, device=device, dtype=dt)
    eye = torch.eye(nx, device=device, dtype=dt)

    def kalman(update):
        x = torch.zeros((nenv, nx, 1), device=device, dtype=dt)
        P = torch.diag(p0).expand(nenv, -1, -1).clone()
        err = []
        for f in range(T):
            x = A[f] @ x
            P = A[f] @ P @ A[f].transpose(1, 2) + Q
            if update:
                Pinv = torch.linalg.solve(P, eye.expand(nenv, -1, -1))
                info = Pinv + (Ct[f] @ C[f]) / r ** 2                         # C^T R^-1 C: 2 nr x 2 nr
                eta = Pinv @ x + (Ct[f] @ y[f].unsqueeze(2)) / r ** 2
                P = torch.linalg.solve(info, eye.expand(nenv, -1, -1))
                P = 0.5 * (P + P.transpose(1, 2))
                x = P @ eta
            err.append((x.squeeze(2) - dx_true[f])[:, list(BOX)].norm(dim=1))
        return torch.stack(err, 0)                                            # [T, nenv]

    e_tac, e_open = kalman(True), kalman(False)
    res = {"start": dq0[:, list(BOX)].norm(dim=1).cpu().numpy(), "tactile": e_tac.cpu().numpy(), "prediction": e_open.cpu().numpy(),
           "loaded_share": float(loaded.double().mean()), "r": r}
    if verbose:
        pr = lambda a: "median %.3e  max %.3e" % (np.median(a), a.max())      # noqa: E731
        print("TactilePush fp64, %d environments, %d frames of %d sub-steps; box start displaced by sigma = %g per dof (x, y, angle)" % (nenv, T, S, sigma))
        print("tactile Jacobians: Ct %s, %.1f MB; %.1f %% of the reference's tactile values loaded; measurement sigma %.3e" % (
            tuple(Ct.shape), Ct.numel() * Ct.element_size() / 1e6, 100 * res["loaded_share"], r))
        print("|box pose deviation| at the start              : " + pr(res["start"]))
        print("box pose error at the end, prediction alone    : " + pr(res["prediction"][-1]))
        print("box pose error at the end, with tactile update : " + pr(res["tactile"][-1]))
        print("environments where the tactile update ends closer: %d of %d" % (int((res["tactile"][-1] < res["prediction"][-1]).sum()), nenv))
        print("per frame (median over the environments): prediction alone / with tactile update")
        for f in range(T):
            print("  frame %2d: %.3e / %.3e" % (f, np.median(res["prediction"][f]), np.median(res["tactile"][f])))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--sigma", type=float, default=2e-3)
    a = ap.parse_args()
    run(nenv=a.envs, T=a.frames, sigma=a.sigma)
