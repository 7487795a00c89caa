"""Go / no-go sizing of predictor helpers (profiles/r28_predictor_helpers.md; A/B build with -DTS_ROUND_STATS; GPU box):
   python tools/build_ab.py rounds -DTS_ROUND_STATS
   TSIM_HIP_LIB=tactilesimulation_amd/csrc/ab/libtsim_rounds.so python tools/predictor_helper_sizing.py [out.json]
A finished slot of a wavefront could evaluate, in the round in which a live slot evaluates the point that ends its sub-step, the predictor of that
slot's next sub-step: the commit would then cost the live slot one round instead of two.  The build leaves, per slot (tsim_kernels.h, hr_ / hc_ /
hcs_): the rounds in which it was live while a slot of its wavefront was done, its commits in such rounds that another sub-step follows, and those of
them a helper could really have served (the evaluation was the sub-step's first or a full Newton step's first trial, and a done slot was left for
this one).  From that, per wavefront: its rounds R, the round F in which its first slot finished (R - max hr), every slot's last round F + hr, and the
last round it would have had if every such commit had saved one round, max over its slots of (F + hr - hc) — `if_all` — or only the served ones —
`if_served`.  The launch lasts as long as its slowest wavefront: the gate is the maximum of that figure over the wavefronts against the measured
maximum.  Two launch sequences of the headline batch: episodes of 100, 5 and 20 env-steps (bench.py --steps 20 --warmup 5: the last launch has no
order) and 100, 20, 20 (--warmup 20: LPT order and split in place)."""
import os, sys, json
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from tactilesimulation_amd.model.compiler import load_model
from tactilesimulation_amd.host.batch import BatchSim
from tactilesimulation_amd.workloads import push_workload, PUSHER_BLOB
B, S = int(os.environ.get("BATCH", "4096")), 5
NS = 4                                          # fp32 pusher: 16 lanes per environment
q0, u, _ = push_workload(B, 100, seed=0)        # the bench's table


def run(sim, ut, q0t, T):
    sim.reset(q0t, None, backward_flag=True)
    ro = sim.rollout(ut[:T], S)
    torch.cuda.synchronize()
    return ro["status"].cpu().numpy().astype(np.int64), sim.last_gnorm().astype(np.float64), sim.last_evals().astype(np.int64), sim.last_helper_trials().astype(np.int64)


def wavefronts(r, c, ordered):
    """Environment indices per wavefront.  No order: wavefront w holds environments 4 w .. 4 w + 3; under an order the deal is the library's, and the
    slots of a wavefront are told by their common (rounds, clocks) pair, as tools/forward_split_sizing.py does."""
    if not ordered:
        return [np.arange(w * NS, min(B, (w + 1) * NS)) for w in range((B + NS - 1) // NS)]
    key = r * (1 << 40) + c.astype(np.int64)
    idx = np.argsort(key, kind="stable")
    cuts = np.flatnonzero(np.diff(key[idx])) + 1
    return np.split(idx, cuts)


def sizing(r, c, e, pk, ordered):
    hr, hc, hcs = pk & 2047, (pk >> 11) & 1023, (pk >> 21) & 1023
    rows = []
    for w in wavefronts(r, c, ordered):
        R = int(r[w[0]]); F = R - int(hr[w].max())
        rows.append((R, float(c[w[0]]), int(hr[w].max()), int(hc[w].sum()), int(hcs[w].sum()), int((F + hr[w] - hc[w]).max()), int((F + hr[w] - hcs[w]).max()), len(w)))
    t = np.array(rows, dtype=np.float64)
    R, cyc, hrw, hcw, hcsw, if_all, if_served, nsl = t.T
    i = int(np.argmax(R))
    top = np.argsort(-R, kind="stable")[:8]
    return {"wavefronts": len(rows), "slots_per_wavefront_min_max": [int(nsl.min()), int(nsl.max())],
            "rounds_max": int(R.max()), "rounds_mean": float(R.mean()), "cycles_max": float(cyc.max()), "cycles_per_round_of_the_slowest": float(cyc[i] / R[i]),
            "evals_median": float(np.median(e)), "evals_max": int(e.max()),
            "helper_rounds_mean": float(hrw.mean()), "helper_rounds_of_the_slowest": int(hrw[i]),
            "commits_in_helper_rounds_mean": float(hcw.mean()), "commits_in_helper_rounds_of_the_slowest": int(hcw[i]), "served_of_the_slowest": int(hcsw[i]),
            "predicted_rounds_max_if_all": int(if_all.max()), "predicted_rounds_max_if_served": int(if_served.max()),
            "saving_if_all": float(1 - if_all.max() / R.max()), "saving_if_served": float(1 - if_served.max() / R.max()),
            "gate_5_per_cent_if_all": bool(if_all.max() <= 0.95 * R.max()), "gate_5_per_cent_if_served": bool(if_served.max() <= 0.95 * R.max()),
            "slowest_8": [{"rounds": int(R[k]), "helper_rounds": int(hrw[k]), "commits": int(hcw[k]), "served": int(hcsw[k]), "if_all": int(if_all[k]), "if_served": int(if_served[k])} for k in top]}


def main():
    res = {}
    ut = torch.tensor(u, device="cuda:0", dtype=torch.float32).transpose(0, 1).contiguous()
    q0t = torch.tensor(q0, device="cuda:0", dtype=torch.float32)
    for name, seq in (("headline_100_5_20", (100, 5, 20)), ("ordered_100_20_20", (100, 20, 20))):
        sim = BatchSim(load_model(PUSHER_BLOB), B, dtype=torch.float32, tape_capacity=100 * S)      # a batch of its own per sequence: no order carried over
        for T in seq:
            r, c, e, pk = run(sim, ut, q0t, T)
        ordered = seq[-1] == seq[-2]
        res[name] = sizing(r, c, e, pk, ordered)
        if not ordered:      # the (rounds, clocks) grouping, checked where the deal is known
            res[name]["grouping_by_rounds_and_clocks_agrees"] = sorted(tuple(sorted(w)) for w in wavefronts(r, c, True)) == sorted(tuple(w) for w in wavefronts(r, c, False))
        del sim
    txt = json.dumps(res, indent=1)
    print(txt)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
