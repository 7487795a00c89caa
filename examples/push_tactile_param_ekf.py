"""examples/push_tactile_ekf.py extended to the augmented state (x, p): a linearised Kalman filter around a recorded TactilePush roll-out that
estimates contact PARAMETERS of the pusher from the tactile frames alone, from the per-frame Jacobians of the recorded episode in one launch each:
(A_f, B_f) (functions.episode_transition), C_f = dtactile / dx (functions.episode_observation) and the parameter block E_f = dx_{f+1} / dp,
F_f = dtactile / dp (include/tsim.h tsim_param_jacobians, functions.episode_parameters).  p is the pad-box pair's kn and mu.  The replays run the
recorded controls from the recorded start with those two parameters perturbed per environment (BatchSim.set_env_tables), so the state deviation
dx_f = x_f - x_ref_f is caused by the parameters alone; the filter's state is z = (dx, dp / p_nominal):

    predict   z^- = [[A_f, E_f], [0, I]] z^ ,  P^- = (.) P (.)^T + Q
    update    P^-1 = (P^-)^-1 + H_f^T R^-1 H_f ,  P^-1 z^ = (P^-)^-1 z^- + H_f^T R^-1 y_f ,   H_f = [C_f | F_f] ,  y_f = tactile_f - tactile_ref_f

batched over the environments in torch, in information form.  A pair's parameters have no direct tactile term (F_f is zero in their columns: only a
SENSOR's own parameters have one), so what the pad feels of them is the box's and the pad's changed motion, C_f E_f.  Prints the relative
parameter error at the end with the tactile update and without it (prediction alone, which stays at the prior: the nominal values).

    python examples/push_tactile_param_ekf.py [--envs 64] [--frames 20] [--sigma 0.1] [--normal-equations]

With --normal-equations the update's H_f^T H_f and H_f^T y_f come from ONE launch (include/tsim.h tsim_tactile_normal_equations,
functions.episode_information) and neither C_f nor F_f is stored; the replays then run on a second batch, because the launch reads the recorded
tape with the measurements as its residual.  Without the flag nothing changes.

It is a demonstration, not a test: there is no threshold.  What it printed on an MI355X is in profiles/r26_param_jacobians.md, and with the flag
next to it in profiles/r29_tactile_normal_equations.md."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tactilesimulation_amd.functions import episode_information, episode_observation, episode_parameters, episode_transition      # noqa: E402
from tactilesimulation_amd.host.batch import BatchSim      # noqa: E402
from tactilesimulation_amd.model.compiler import load_model      # noqa: E402
from tactilesimulation_amd.workloads import asset, push_workload      # noqa: E402

PARAMS = (("tactile_pad_left", "box"), ("kn", "mu"))      # the pad-box pair's normal stiffness and friction coefficient


def run(nenv=64, T=20, S=5, sigma=0.1, seed=0, device="cuda:0", verbose=True, normal_equations=False):
    dt = torch.float64
    m = load_model(asset("pusher"))
    cols = [m.table_offset("pair", PARAMS[0], f) for f in PARAMS[1]]
    np_ = len(cols)
    sim = BatchSim(m, nenv, device=device, dtype=dt, tape_capacity=T * S)
    q0, u, _ = push_workload(nenv, T, seed=seed + 1)
    u[:, :, 0] = 0.9                                                          # the pad is driven into the box
    q0 = torch.tensor(q0, device=device, dtype=dt)
    ut = torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device=device, dtype=dt)
    nr = sim.ndof_r
    nx, nz = 2 * nr, 2 * nr + np_
    base = sim.base_tables()                                                  # [nenv, table_size]: the shared model's row, per environment
    pnom = base[0, cols].clone()
    # 1. the recorded roll-out on the nominal parameters
    sim.set_env_tables(base)
    sim.reset(q0, None, backward_flag=True)
    ref = sim.rollout(ut, S, want_qd=True)
    xref = torch.cat([ref["q"], ref["qd"]], 2)                                # [T, nenv, nx]: x_{f+1}
    # 2. the linearisation, one launch each; the parameter columns scaled to relative changes
    A, _ = episode_transition(sim, T, S)
    if normal_equations:                                                      # E alone: no Ct, no F
        E = sim.param_jacobians(T, S, cols, want_E=True)["E"] * pnom
        C = F = H = Ht = None
    else:
        C = episode_observation(sim, T, S)                                    # [T, nenv, ntac, nx]
        E, F = episode_parameters(sim, T, S, cols)                            # [T, nenv, nx, np], [T, nenv, ntac, np]
        E, F = E * pnom, F * pnom
        assert not bool(F.any())                                              # a pair column has no direct tactile term
        H = torch.cat([C, F], 3)                                              # [T, nenv, ntac, nz]
        Ht = H.transpose(-1, -2).contiguous()
    Az = torch.zeros((T, nenv, nz, nz), device=device, dtype=dt)
    Az[:, :, :nx, :nx], Az[:, :, :nx, nx:] = A, E
    Az[:, :, nx:, nx:] = torch.eye(np_, device=device, dtype=dt)
    # 3. replays with the parameters perturbed per environment; their tactile frames are the measurements
    rng = np.random.default_rng(seed + 2)
    dp_true = torch.tensor(sigma * rng.uniform(-1, 1, size=(nenv, np_)), device=device, dtype=dt)      # relative
    tab = base.clone()
    tab[:, cols] = pnom * (1 + dp_true)
    rsim = BatchSim(m, nenv, device=device, dtype=dt, tape_capacity=T * S) if normal_equations else sim      # (sim keeps the recorded tape)
    rsim.set_env_tables(tab)
    rsim.reset(q0, None, backward_flag=False)
    rep = rsim.rollout(ut, S, want_qd=True)
    dx_true = torch.cat([rep["q"], rep["qd"]], 2) - xref
    y = rep["tactile"] - ref["tactile"]                                       # [T, nenv, ntac]
    loaded = ref["tactile"].abs() > 0
    r = 0.05 * float(ref["tactile"][loaded].pow(2).mean().sqrt()) if bool(loaded.any()) else 1.0      # 5 % of a loaded taxel's typical force
    if normal_equations:                                                      # H^T H and H^T y of every frame in one launch (W = I; 1 / r^2 below)
        scale = torch.cat([torch.ones(nx, device=device, dtype=dt), pnom])
        HtH, Hty = episode_information(sim, T, S, residual=y.contiguous(), cols=cols)
        HtH, Hty = HtH * scale[:, None] * scale[None, :], Hty * scale
    # 4. the filter, with and without the tactile update
    p0 = torch.full((nz,), 1e-12, device=device, dtype=dt)                    # the start state is known
    p0[nx:] = sigma ** 2
    Q = 1e-12 * torch.eye(nz, device=device, dtype=dt)
    Q[nx:, nx:] = 0                                                           # the parameters are constants
    eye = torch.eye(nz, device=device, dtype=dt)

    def kalman(update):
        z = torch.zeros((nenv, nz, 1), device=device, dtype=dt)
        P = torch.diag(p0).expand(nenv, -1, -1).clone()
        ep, ex = [], []
        for f in range(T):
            z = Az[f] @ z
            P = Az[f] @ P @ Az[f].transpose(1, 2) + Q
            if update:
                Pinv = torch.linalg.solve(P, eye.expand(nenv, -1, -1))
                info = Pinv + (HtH[f] if normal_equations else Ht[f] @ H[f]) / r ** 2      # H^T R^-1 H: nz x nz
                eta = Pinv @ z + (Hty[f].unsqueeze(2) if normal_equations else Ht[f] @ y[f].unsqueeze(2)) / r ** 2
                P = torch.linalg.solve(info, eye.expand(nenv, -1, -1))
                P = 0.5 * (P + P.transpose(1, 2))
                z = P @ eta
            ep.append((z.squeeze(2)[:, nx:] - dp_true).abs())
            ex.append((z.squeeze(2)[:, :nx] - dx_true[f]).norm(dim=1))
        return torch.stack(ep, 0), torch.stack(ex, 0)                         # [T, nenv, np], [T, nenv]

    (p_tac, x_tac), (p_open, x_open) = kalman(True), kalman(False)
    res = {"dp_true": dp_true.abs().cpu().numpy(), "tactile": p_tac.cpu().numpy(), "prediction": p_open.cpu().numpy(),
           "x_tactile": x_tac.cpu().numpy(), "x_prediction": x_open.cpu().numpy(), "r": r}
    if verbose:
        pr = lambda a: "median %.3e  max %.3e" % (np.median(a), a.max())      # noqa: E731
        print("TactilePush fp64, %d environments, %d frames of %d sub-steps; pad-box %s perturbed by up to %g of their values (%s)" % (
            nenv, T, S, " and ".join(PARAMS[1]), sigma, ", ".join("%g" % v for v in pnom.tolist())))
        if normal_equations:
            print("E %s, H^T H %s, H^T y %s from one launch (no C, no F); measurement sigma %.3e" % (tuple(E.shape), tuple(HtH.shape), tuple(Hty.shape), r))
        else:
            print("E %s, F %s (zero: pair columns), C %s; measurement sigma %.3e" % (tuple(E.shape), tuple(F.shape), tuple(C.shape), r))
        for k, name in enumerate(PARAMS[1]):
            print("relative error of %-3s  at the prior (prediction alone) : %s" % (name, pr(res["prediction"][-1][:, k])))
            print("relative error of %-3s  with the tactile update         : %s" % (name, pr(res["tactile"][-1][:, k])))
            print("  environments where the tactile update ends closer: %d of %d" % (int((res["tactile"][-1][:, k] < res["prediction"][-1][:, k]).sum()), nenv))
        print("state error at the end, prediction alone / with tactile update: %s / %s" % (pr(res["x_prediction"][-1]), pr(res["x_tactile"][-1])))
        print("per frame (median over the environments), relative error of %s: with tactile update" % " / ".join(PARAMS[1]))
        for f in range(T):
            print("  frame %2d: %s" % (f, " / ".join("%.3e" % np.median(res["tactile"][f][:, k]) for k in range(np_))))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--normal-equations", action="store_true", help="H^T H and H^T y from tsim_tactile_normal_equations; no C or F is stored")
    a = ap.parse_args()
    run(nenv=a.envs, T=a.frames, sigma=a.sigma, normal_equations=a.normal_equations)
