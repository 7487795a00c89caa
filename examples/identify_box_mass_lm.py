"""examples/identify_box_mass.py with Gauss-Newton instead of Adam: the same recorded episodes (each environment's box has its own true mass, 0.8 ..
1.25 times the model's; its box poses and the pad's tactile frames of a pushing episode are recorded with it), the same starts at 0.5 and at 2 times
the truth, fp64, log-mass — but the residual (the scaled trajectory and tactile frames) is kept as a vector and each environment runs
Levenberg-Marquardt on its one unknown.  The Jacobian of the frames w.r.t. the box link's mass column comes from functions.episode_jacobian: a
forward-mode tangent pass over the recorded episode with the inertial group switched on (include/tsim.h tsim_tangent_episode,
BatchSim.set_param_grad_groups), where identify_box_mass.py needs one adjoint pass per Adam iteration.  A step is accepted only where the
environment's own residual falls (else its damping grows).  Only the mass entry of the box link moves; its inertia and centre of mass keep the
model's values.

    python examples/identify_box_mass_lm.py [--envs 16] [--iters 12]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from identify_box_mass import BOX_JOINT      # noqa: E402
from tactilesimulation_amd.functions import episode_jacobian      # noqa: E402
from tactilesimulation_amd.host.batch import BatchSim      # noqa: E402
from tactilesimulation_amd.model.compiler import load_model      # noqa: E402
from tactilesimulation_amd.workloads import asset, push_workload      # noqa: E402


def run(B=16, iters=12, T=12, S=5, seed=0, device="cuda:0", verbose=True, starts=(0.5, 2.0), lam0=1e-3):
    """per start: {"reached": iteration (1-based) at which each environment's mass was within 1 % of the truth (-1: never), "rel_err": the final
    relative errors, "loss": the summed cost per iteration}"""
    m = load_model(asset("pusher"))
    col = m.table_offset("link", (BOX_JOINT, None), "mass")
    sim = BatchSim(m, B, device=device, dtype=torch.float64, tape_capacity=T * S)
    sim.set_param_grad_groups(("contact", "inertial"))                     # the tangent pass reads the mass column only with its group on
    rng = np.random.default_rng(seed)
    q0, u, _ = push_workload(B, T, seed=seed + 1)
    u[:, :, 0] = 0.9                                                       # the pad pushes the box
    q0 = torch.tensor(q0, device=device, dtype=torch.float64)
    ut = torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device=device, dtype=torch.float64)
    base = sim.base_tables()
    true = base[:, col] * torch.tensor(rng.uniform(0.8, 1.25, size=B), device=device)

    def frames(mass, record):
        tb = base.clone()
        tb[:, col] = mass
        sim.set_env_tables(tb); sim.reset(q0, None, backward_flag=record)
        o = sim.rollout(ut, S)
        return o["q"], o["tactile"]                                        # [T, B, nr], [T, B, ntac]

    q_true, tac_true = frames(true, False)
    qs = (q_true - q0).abs().amax((0, 2), keepdim=True).clamp_min(1e-9)     # per environment
    ts = tac_true.abs().amax((0, 2), keepdim=True).clamp_min(1e-9)
    flat = lambda x: x.permute(1, 0, 2).reshape(B, -1)
    resid = lambda q, tac: torch.cat([flat((q - q_true) / qs), flat((tac - tac_true) / ts)], 1)      # [B, T (nr + ntac)]
    jscale = torch.cat([flat(qs.expand_as(q_true)), flat(ts.expand_as(tac_true))], 1)
    out = {}
    try:
        for f in starts:
            mass = (f * true).clone()
            lam = torch.full((B,), lam0, device=device, dtype=torch.float64)
            reached = np.full(B, -1)
            losses = []
            for it in range(iters):
                r = resid(*frames(mass, True))
                cost = (r * r).sum(1)
                # d residual / d log m = (d outputs / d m) m / scale
                J = episode_jacobian(sim, T, S, [col], outputs=("q", "tactile"))[:, :, 0] * mass.unsqueeze(1) / jscale
                a, g = (J * J).sum(1), (J * r).sum(1)
                step = (-g / (a * (1.0 + lam)).clamp_min(1e-300)).clamp(-1.0, 1.0)
                trial = mass * torch.exp(step)
                rt = resid(*frames(trial, False))
                better = (rt * rt).sum(1) < cost
                mass = torch.where(better, trial, mass)
                lam = torch.where(better, lam / 3.0, lam * 4.0).clamp(1e-9, 1e9)
                err = ((mass - true) / true).abs()
                losses.append(float(torch.where(better, (rt * rt).sum(1), cost).sum()))
                reached[(reached < 0) & (err <= 0.01).cpu().numpy()] = it + 1
                if verbose:
                    print("start %.1fx  iter %3d  loss %.3e  accepted %2d of %d  |m / m* - 1| median %.2e max %.2e" % (
                        f, it, losses[-1], int(better.sum()), B, float(err.median()), float(err.max())))
            out[str(f)] = {"reached": reached, "rel_err": err.cpu().numpy(), "loss": losses}
    finally:
        sim.set_param_grad_groups(("contact",))                            # (also when an iteration raises)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--iters", type=int, default=12)
    a = ap.parse_args()
    res = run(B=a.envs, iters=a.iters)
    for f, r in res.items():
        print("start %sx the true mass: |m / m* - 1| median %.2e, max %.2e; iteration at which each environment was within 1 %% (-1: never): %s"
              % (f, float(np.median(r["rel_err"])), float(r["rel_err"].max()), r["reached"].tolist()))


if __name__ == "__main__":
    main()
