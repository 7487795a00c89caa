"""Cost of an evaluation round of the forward episode kernel where NO slot is ever done before the others (GPU box): 4096 IDENTICAL TactilePush
environments, so every wavefront does the same work, its four slots finish in the same round and no helper slot ever exists — the rounds that
speculation cannot help and must not tax.  Episodes of 20 env-steps x 5 sub-steps through tsim_rollout (the k_forward_fr path of the bench's headline),
the forward kernel timed by the library's own HIP events; a round is one evaluation of every slot, so rounds = the evaluation count of an environment.
   python tools/identical_round_cost.py            (parent against child: TSIM_HIP_LIB=<the parent's library>, alternating, profiles/r28_predictor_helpers.md)"""
import os, sys, json
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from tactilesimulation_amd.model.compiler import load_model
from tactilesimulation_amd.host.batch import BatchSim
from tactilesimulation_amd.workloads import push_workload, PUSHER_BLOB
B, T, S, REPS = 4096, 20, 5, int(os.environ.get("REPS", "10"))
q0, u, _ = push_workload(1, T, seed=0)
sim = BatchSim(load_model(PUSHER_BLOB), B, dtype=torch.float32, tape_capacity=T * S)
q0t = torch.tensor(np.tile(q0, (B, 1)), device="cuda:0", dtype=torch.float32)
ut = torch.tensor(np.tile(u, (B, 1, 1)), device="cuda:0", dtype=torch.float32).transpose(0, 1).contiguous()
for _ in range(3):      # clocks, code objects
    sim.reset(q0t, None, backward_flag=True); sim.rollout(ut, S)
torch.cuda.synchronize()
sim.kernel_timing(True)
us = []
for _ in range(REPS):
    sim.reset(q0t, None, backward_flag=True); sim.rollout(ut, S)
    torch.cuda.synchronize()
    ms, n = sim.kernel_times()["k_forward"]
    us.append(1e3 * ms / max(1, n))
ev = sim.last_evals()
assert int(ev.min()) == int(ev.max()), "identical environments: identical evaluation counts"
rounds = int(ev[0])
print(json.dumps({"lib": os.environ.get("TSIM_HIP_LIB", "built"), "rounds": rounds, "helped_max": int(sim.last_helper_trials().max()),
                  "k_forward_us_median": float(np.median(us)), "k_forward_us_min_max": [float(min(us)), float(max(us))],
                  "us_per_round_median": float(np.median(us)) / rounds, "us_per_round_min_max": [float(min(us)) / rounds, float(max(us)) / rounds]}))
