"""Sizing of the forward launch split by LPT rank (profiles/r27_forward_split.md; A/B build with -DTS_ROUND_STATS; GPU box):
   python tools/build_ab.py rounds -DTS_ROUND_STATS
   TSIM_NO_FORWARD_SPLIT=1 TSIM_HIP_LIB=tactilesimulation_amd/csrc/ab/libtsim_rounds.so python tools/forward_split_sizing.py
Percentiles over the wavefronts of their rounds and shader clocks in a 20-step episode launch of the headline batch (repetitions 1 and 2 run in the
LPT order of the one before; every environment reports its wavefront's figures, so percentiles over environments are percentiles over wavefronts),
and the light group's last round: the largest figure among the wavefronts that do not hold one of the 128 environments of most evaluations.  Then
the bench's own sequence of episode lengths (100, 5, 20 env-steps): which order that leaves for the timed launch, and how well the totals of an
episode of another length would rank the timed one's heavy environments."""
import os, sys, json
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from tactilesimulation_amd.model.compiler import load_model
from tactilesimulation_amd.host.batch import BatchSim
from tactilesimulation_amd.workloads import push_workload, PUSHER_BLOB
B, S = int(os.environ.get("BATCH", "4096")), 5
q0, u, _ = push_workload(B, 100, seed=0)       # the bench's table
sim = BatchSim(load_model(PUSHER_BLOB), B, dtype=torch.float32, tape_capacity=100 * S)
ut = torch.tensor(u, device="cuda:0", dtype=torch.float32).transpose(0, 1).contiguous()
q0t = torch.tensor(q0, device="cuda:0", dtype=torch.float32)


def run(T):
    sim.reset(q0t, None, backward_flag=True)
    ro = sim.rollout(ut[:T], S)
    torch.cuda.synchronize()
    return ro["status"].cpu().numpy().astype(np.int64), sim.last_gnorm().astype(np.float64), sim.last_evals().astype(np.int64)


def pct(x, ps=(50, 75, 87.5, 90, 95, 97, 99, 100)):
    return {str(p): float(np.percentile(x, p)) for p in ps}


res = {}
for rep in range(3):
    r, c, e = run(20)
    heavy = np.argsort(-e, kind="stable")[:B // 32]                      # one environment per wavefront of the heavy eighth
    light = ~np.isin(r * (1 << 40) + c.astype(np.int64), r[heavy] * (1 << 40) + c[heavy].astype(np.int64))      # wavefronts told apart by (rounds, clocks)
    res["ep20_rep%d" % rep] = {"rounds": pct(r), "cycles": pct(c), "evals": pct(e), "rounds_mean": float(r.mean()), "cycles_mean": float(c.mean()),
                               "light_group": {"environments": int(light.sum()), "last_round": int(r[light].max()), "last_cycle": float(c[light].max())}}
e20_lpt = e
r100, c100, e100 = run(100)
r5, c5, e5 = run(5)
r20, c20, e20 = run(20)
res["bench_sequence_ep20"] = {"rounds": pct(r20), "cycles": pct(c20), "rounds_mean": float(r20.mean()), "evals_equal_those_under_the_order": bool((e20 == e20_lpt).all())}


def overlap(pred, true, k):
    return len(set(np.argsort(-pred, kind="stable")[:k]) & set(np.argsort(-true, kind="stable")[:k])) / k


for name, pred in (("ep5", e5), ("ep100", e100)):
    res["rank_by_" + name] = {"top128_shared": overlap(pred, e20, 128), "top512_shared": overlap(pred, e20, 512),
                              "rank_correlation": float(np.corrcoef(np.argsort(np.argsort(pred)), np.argsort(np.argsort(e20)))[0, 1]),
                              "most_evals_outside_its_top512": int(e20[np.argsort(-pred, kind="stable")[512:]].max()), "most_evals": int(e20.max())}
print(json.dumps(res, indent=1))
