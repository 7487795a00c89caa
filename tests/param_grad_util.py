"""What the tests of the per-environment table gradient share (tsim_set_param_grad, tsim_set_param_grad_groups): the cases, the loss, the fp64 CPU
oracle's episode and its cache, the per-environment rows, the mirror of the host's chunk layout, and the batch factory and episode runner of the GPU
files.  Used by tests/test_oracle_param_grad.py, test_oracle_body_param_grad.py, test_gpu_param_grad.py, test_gpu_param_grad_oracle.py,
test_gpu_body_param_grad.py, test_gpu_body_param_grad_oracle.py and body_param_util.py.  Importable without torch and without a GPU (body_param_util
runs in spawned CPU processes): torch is imported inside the GPU helpers only."""
import copy
import functools
import os
import pathlib
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
from tactilesimulation_amd.model.compiler import load_model, parse_xml, compile_spec      # noqa: E402
from tactilesimulation_amd.workloads import asset, push_workload      # noqa: E402

DEV = "cuda:0"
# ---------------------------------------------------------------------------------------------------- groups, kinds, cases
BODY = ("inertial", "motor", "limit")
ALL = ("contact",) + BODY
# the kinds of model.param_columns() and of model.body_param_columns()
CONTACT_KINDS = ("pair kn", "pair kt", "pair mu", "pair damping", "sensor kn", "sensor kt", "sensor mu", "sensor damping", "dof damping")
BODY_KINDS = ("mass", "com", "inertia", "motor lo", "motor hi", "motor P", "motor D", "limit lo", "limit hi", "limit k")
# (name, frames) of the body groups' finite-difference yardstick
MODELS = [("pusher", 4), ("tactile_insertion", 3), ("stable_grasp", 3), ("dclaw_position_control", 3), ("tactile_pad", 3), ("box_slide", 4),
          ("pad_press", 4), ("slider_push", 4), ("ball_push", 4), ("bdf2:ball_push", 3), ("bdf2:tactile_pad", 3), ("small:3", 4), ("small:11", 4),
          ("large:L3", 4), ("large:L7", 4), ("large:L16", 4), ("limit_push", 4)]
# a second model whose lower AND upper limit springs act in every environment, without contact (so that fp32 keeps the oracle's branches): the
# files that hold something to the oracle's exact adjoint run it beside MODELS
LIMIT_CHAIN = ("limit_chain", 4)


def kind_of(col):
    """'pair kn' ... 'dof damping' of a param_columns() entry; 'mass' / 'com' / 'inertia', 'motor lo' ... 'limit k' of a body_param_columns() entry"""
    kind, _, f, _ = col
    return {"link": "mass" if f == "mass" else "com" if f.startswith("com") else "inertia"}.get(kind) or "%s %s" % (kind, f)


def fixed_case(name, B):
    """model, q0 [B, nr], u [B, T, nu], sub-steps per frame: a few frames in contact"""
    from test_gpu_models import CASES, _inputs
    if name.startswith("random"):
        import pytest
        from test_native_model_loader import _random_model
        rng = np.random.default_rng(5000 + int(name[6:]))
        d = tempfile.mkdtemp(prefix="tsim_pg_")
        for _ in range(20):
            p = os.path.join(d, "m.xml")
            open(p, "w").write(_random_model(rng, max_dof=10))
            spec = parse_xml(p)
            m = compile_spec(spec)
            if 1 <= m.ndof_r <= 16 and m.ndof_u <= 16 and sum(J["type"] == "free3d-exp" for J in spec["joints"]) <= 1:
                break
        else:
            pytest.skip("no model within the kernels' sizes")
        q0 = np.tile(0.02 * rng.normal(size=(1, m.ndof_r)), (B, 1))
        u = np.tile(rng.uniform(-1, 1, size=(1, 4, max(m.ndof_u, 1)))[:, :, :m.ndof_u], (B, 1, 1))
        return m, q0, u, 2
    if name.startswith("large:"):      # the large corpus of tests/random_corpus.py (ndof_r 13 .. 16)
        import random_corpus as RC
        m, rng = RC.draw(name[6:], pathlib.Path(tempfile.mkdtemp(prefix="tsim_pg_")))
        q0 = np.tile(0.02 * rng.normal(size=(1, m.ndof_r)), (B, 1))
        u = np.tile(rng.uniform(-1, 1, size=(1, 4, max(m.ndof_u, 1)))[:, :, :m.ndof_u], (B, 1, 1))
        return m, q0, u, 2
    p = os.path.join(HERE, "models", name + ".xml")
    m = load_model(p if os.path.exists(p) else asset(name))
    if name == "pusher":
        q0, u, _ = push_workload(B, 12, seed=3)
        u[:, :, 0] = 0.9                                                 # drive the pad into the box
        return m, q0, u, 5
    if name == "stable_grasp":
        q0 = np.zeros((B, m.ndof_r)); u = np.zeros((B, 6, m.ndof_u)); u[:, :, -2:] = 1.0
        return m, q0, u, 1
    if name == "tactile_pad":
        q0 = np.zeros((B, m.ndof_r)); u = np.zeros((B, 70, 3)); u[:, :, 2] = 0.2; u[:, 60:, 0] = 0.1
        return m, q0, u, 2
    T, S = CASES[name][2], CASES[name][3]
    q0, u = _inputs(name, m, B, T)
    return m, q0, u, S


def bdf2_case(name):
    """model, q0, u, sub-steps per frame of a BDF2 case (tests/test_gpu_bdf2_adjoint.py _case)"""
    from test_gpu_bdf2_adjoint import _case
    return _case(name)


@functools.lru_cache(maxsize=None)
def _preroll(name, S):
    """(q, qd) of the tactile_pad case after its first 56 frames (pressed on the ball, just before the drag), on the oracle"""
    from oracle.oracle import OracleSim
    m, q0, u, S = bdf2_case(name[5:]) if name.startswith("bdf2:") else fixed_case(name, 1)
    o = OracleSim(m)
    o.reset(q0[0])
    for t in range(56):
        o.forward(u[0, t], S)
    return o.state()


def case(name, B, T=None):
    """model, q0 [B, nr], qd0 [B, nr], u [B, T, nu], sub-steps per frame.  The same inputs as the kernels' older tests
    (fixed_case, tests/test_gpu_bdf2_adjoint.py _case, tests/random_corpus.py)."""
    if name.startswith("bdf2:"):
        m, q0, u, S = bdf2_case(name[5:])
        q0, u = np.resize(q0, (B, q0.shape[1])), np.resize(u, (B,) + u.shape[1:])
    elif name.startswith(("small:", "large:")):
        import random_corpus as RC
        cid = int(name[6:]) if name.startswith("small:") else name[6:]
        got = RC.draw(cid, pathlib.Path(tempfile.mkdtemp(prefix="tsim_opg_")))
        if got is None:
            raise AssertionError("no model within the kernels' sizes for %s" % name)
        m, rng = got
        q0 = np.tile(0.02 * rng.normal(size=(1, m.ndof_r)), (B, 1))
        u = np.tile(rng.uniform(-1, 1, size=(1, 4, max(m.ndof_u, 1)))[:, :, :m.ndof_u], (B, 1, 1))
        S = 2
    else:
        m, q0, u, S = fixed_case(name, B)
    qd0 = np.zeros_like(q0)
    if name.endswith("tactile_pad"):                                     # start pressed on the ball, just before the drag (frame 56 of the case)
        q, qd = _preroll(name, S)
        q0, qd0, u = np.tile(q, (B, 1)), np.tile(qd, (B, 1)), u[:, 56:]
    if T is not None:
        u = u[:, :T]
    return m, q0, qd0, u, S


def body_case(name, B, T):
    """case(), and the body groups' own models: tests/models/limit_push.xml — a slider a force motor pushes below its lower limit and an arm a
    position motor holds above its upper limit, both in the limit from the first sub-step on — and tests/models/limit_chain.xml"""
    if name == "limit_chain":      # the shoulder below its lower limit, the elbow above its upper one
        m = load_model(os.path.join(HERE, "models", "limit_chain.xml"))
        q0 = np.tile([[-0.25, 0.3]], (B, 1))
        u = np.tile(np.array([[-0.6, 0.5], [-0.4, 0.45], [-0.7, 0.55], [-0.5, 0.4]])[None], (B, 1, 1))[:, :T]
        return m, q0, np.zeros_like(q0), u, 2
    if name != "limit_push":
        return case(name, B, T)
    m = load_model(os.path.join(HERE, "models", "limit_push.xml"))
    q0 = np.tile([[-0.03, 0.25]], (B, 1))
    u = np.tile(np.array([[-0.8, 0.6], [-0.6, 0.7], [-0.9, 0.5], [-0.7, 0.6]])[None], (B, 1, 1))[:, :T]
    return m, q0, np.zeros_like(q0), u, 2


def pusher_case(B, T, seed=3):
    """TactilePush with the pad dragged into and across the box, from the workload's third frame on"""
    m = load_model(asset("pusher"))
    q0, u, _ = push_workload(B, T + 2, seed=seed)
    u[:, :, 0] = 0.9
    return m, q0, np.zeros_like(q0), u[:, 2:], 5


# ---------------------------------------------------------------------------------------------------- loss, oracle, rows
def loss_weights(m, T, seed=0):
    """(wq [T, nr], wv [T, nvar], wt [T, ntactile]) of the loss sum_t wq[t].q_t + wv[t].var_t + wt[t].tac_t"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(T, m.ndof_r)), rng.normal(size=(T, m.ndof_var)), rng.normal(size=(T, m.ndof_tactile))


def oracle_episode(m, q0, u, S, w, grad=True, tac_mask=None, qd0=None, groups=None):
    """One environment on the fp64 oracle from (q0, qd0): the frames of u [T, nu], the loss sum_t wq[t].q_t + wv[t].var_t + wt[k].tac_t at each frame's end
    (tac only at the frames tac_mask keeps, seeded by their own rows of wt), and its adjoint frame by frame with the table gradient on.
    groups: OracleSim.set_param_grad_groups' names (None: the default, the contact columns).
    Returns (loss, table gradient [table_size] or None, signatures [T S, 2], non-converged sub-steps, frame states [(q, qd)])."""
    from oracle.oracle import OracleSim
    o = OracleSim(m)
    nr, T = m.ndof_r, u.shape[0]
    wq, wv, wt = w
    keep = np.ones(T, bool) if tac_mask is None else np.asarray(tac_mask, bool)
    o.reset(q0, qd0, record=grad)
    L, sigs, bad, states = 0.0, [], 0, []
    for t in range(T):
        b, sg = o.forward_sig(u[t], S)
        bad += b
        sigs.append(sg)
        q, qd = o.state()
        var, tac = o.outputs(tactile=bool(m.ndof_tactile) and keep[t])
        states.append((q, qd))
        L += float(wq[t] @ q) + (float(wv[t] @ var) if m.ndof_var else 0.0) + (float(wt[t] @ tac) if m.ndof_tactile and keep[t] else 0.0)
    g = None
    if grad:
        g = np.zeros(o._L.orc_table_size(o._h))
        o.set_param_grad(g)
        if groups is not None:
            o.set_param_grad_groups(groups)
        for t in reversed(range(T)):
            dq = np.zeros((S, nr)); dq[-1] = wq[t]
            dv = np.zeros((S, m.ndof_var)); dv[-1] = wv[t]
            dt = np.zeros((S, m.ndof_tactile))
            if keep[t]:
                dt[-1] = wt[t]
            o.backward_steps(S, dq, dv if m.ndof_var else None, dt if m.ndof_tactile else None)
        o.set_param_grad(None)
    return L, g, np.concatenate(sigs, 0), bad, states


_ORACLE = {}


def oracle_cached(m, q0, qd0, u, S, w, tac_mask=None, groups=None):
    """(key, (oracle gradient, signatures [n, 2], non-converged sub-steps, frame states)) of oracle_episode for one environment, kept across
    parametrisations under a key made of everything the run depends on: the model's arrays, the start, the controls, the loss, the mask, the groups"""
    key = (m.F.tobytes(), m.I.tobytes(), q0.tobytes(), qd0.tobytes(), u.tobytes(), S, tuple(x.tobytes() for x in w),
           None if tac_mask is None else tuple(bool(k) for k in tac_mask), None if groups is None else tuple(groups))
    if key not in _ORACLE:
        _ORACLE[key] = oracle_episode(m, q0, u, S, w, tac_mask=tac_mask, qd0=qd0, groups=groups)[1:]
    return key, _ORACLE[key]


def row_model(m, row):
    """the model with one environment's table row in place of its own"""
    me = copy.copy(m)
    me.F = m.F.copy()
    me.F[:row.size] = row
    return me


def table_rows(m, B, fp32, seed, lo=0.8, hi=1.25):
    """[B, table_size] per-environment tables: every column a gradient is computed for — contact and body columns alike — scaled by a seeded
    factor (numpy only, so that the cases can be examined without a GPU); rounded to the batch's type"""
    n = int(m.I[Bl.TSIM_IH_FOFF_CPT])
    cols = [c for (_, _, _, c) in m.param_columns() + m.body_param_columns()]
    tab = np.tile(np.asarray(m.F[:n], dtype=np.float64), (B, 1))
    tab[:, cols] *= np.random.default_rng(seed).uniform(lo, hi, size=(B, len(cols)))
    return tab.astype(np.float32 if fp32 else np.float64)


# ---------------------------------------------------------------------------------------------------- the host's chunk layout
def pg_layout(B, n, n_simd=None):
    """(nchunk, chunk_len) of a parameter pass over n sub-steps: the mirror of tsim_hip.hip pg_layout (n_simd: the device's, 4 per compute unit)"""
    if n_simd is None:
        import torch
        n_simd = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    want = max(1, (16 * n_simd + B - 1) // B)
    most = max(1, min(n, want))
    cl = (n + most - 1) // most
    return (n + cl - 1) // cl, cl


def layout_kind(B, n, n_simd=None):
    nchunk, cl = pg_layout(B, n, n_simd)
    return "single" if nchunk == 1 else "len1" if cl == 1 else "ragged" if n % cl else "even"


# ---------------------------------------------------------------------------------------------------- GPU: batch and episode
def make_sim(m, B, dtype, cap, lanes=0, static=False, tally=None):
    """a batch at `lanes` lanes per environment (0: the library's choice; the explicit setting wins over TSIM_LPE).  The shape the launch reports
    is checked (random_corpus.force_lanes: the forced one, 64 with a rotation-vector joint — the EXPJ instantiations exist at 64 lanes only —, wider
    only where the LDS does not fit) and recorded in tally.lanes"""
    import random_corpus as RC
    from tactilesimulation_amd.host.batch import BatchSim
    sim = BatchSim(m, B, device=DEV, dtype=dtype, tape_capacity=cap)
    sim.set_static(static)
    if lanes:
        got = RC.force_lanes(sim, m, lanes)
        if tally is not None:
            tally.lanes.add(got)
    return sim


def gpu_episode(sim, tab, q0, qd0, u, S, w, groups=("contact",), mode="episode", tac_mask=None, grad=True, want_qd=True):
    """forward of the episode (tab: per-environment tables or None; qd0 None: at rest) and its adjoint with the table gradient of `groups` into a
    zeroed buffer — in one launch ("episode"), frame by frame ("steps") or as two half-episodes into the one buffer ("halves"); tac_mask (episode
    only): the frames whose tactile output is computed and seeded; want_qd: the forward launch also writes the frames' velocities.  Returns (table gradient [B, table_size] or None, signatures [n_sub, B, 2],
    status [B], outputs, dL/du [T, B, nu], carried adjoint)."""
    import torch
    B, T, dt = sim.B, u.shape[1], sim.dtype
    if tab is not None:
        sim.set_env_tables(tab)
    sim.reset(torch.tensor(q0, device=DEV, dtype=dt), None if qd0 is None else torch.tensor(qd0, device=DEV, dtype=dt), backward_flag=True)
    ut = torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device=DEV, dtype=dt)
    mask = None if tac_mask is None else torch.tensor(tac_mask, dtype=torch.bool)
    out = sim.rollout(ut, S, want_qd=want_qd, tactile_mask=mask)
    sig = sim.branch_signature()
    wq, wv, wt = (torch.tensor(x, device=DEV, dtype=dt).unsqueeze(1).expand(-1, B, -1).contiguous() for x in w)
    if mask is not None:
        wt = wt[mask.to(DEV)].contiguous()
    g = None
    if grad:
        g = torch.zeros((B, sim.base_tables().shape[1]), device=DEV, dtype=dt)
        sim.set_param_grad_groups(groups)
        sim.set_param_grad(g)
    nv, nt = sim.ndof_var, sim.ndof_tactile
    if mode == "episode":
        du = sim.backward_episode(T, S, wq, wv if nv else None, wt if nt else None, tactile_mask=mask)
    elif mode == "halves":
        h = T // 2
        d1 = sim.backward_episode(T - h, S, wq[h:], wv[h:] if nv else None, wt[h:] if nt else None)
        d0 = sim.backward_episode(h, S, wq[:h], wv[:h] if nv else None, wt[:h] if nt else None)
        du = torch.cat([d0, d1], 0)
    else:
        du = []
        for t in reversed(range(T)):
            du.append(sim.backward_steps(S, wq[t], wv[t] if nv else None, wt[t] if nt else None))
        du = torch.stack(du[::-1], 0)
    sim.set_param_grad(None)
    sim.set_param_grad_groups(("contact",))
    lq, lv = sim.get_adjoint()
    torch.cuda.synchronize()
    return g, sig, out["status"], out, du, (lq, lv)
