"""The forward-mode tangent pass through the fused closed-loop episode (include/tsim_env.h tsim_push_closed_tangent, FusedPushEpisode.tangent,
csrc/tsim_tangent_closed.hip k_closed_tangent): k_tangent's walk over the tape with the policy's tangent evaluated in the slot at every frame start.

Episodes, policies and tables are those of tests/test_gpu_closed_loop_param_grad.py (B = 10: ragged at four and two environments per wavefront,
T = 12 frames, the seed-1 actor scaled by 3; push = 0 never brings the pad to the box, push = 1.5 loads it in all ten environments).

1. Sim half: BatchSim.tangent_episode (the pinned open-loop k_tangent / k_tangent_src) fed the closed call's du returns the closed call's dq, dqd,
   dvar, dtac bit for bit — the sub-step code is the same, only the origin of du differs.
2. Policy half: du and dupol rebuilt in torch fp64 from the closed call's own dq, dtac, the records and the sources (a manual forward-mode pass of
   the actor).  fp64: 1e-12 of the frame's scale (the bound the fused env kernels are held to against plain torch).  fp32: 4 x the largest
   difference, in the same measure, between that torch pass evaluated in fp32 and in fp64 on the same inputs — no code under test enters the bound
   (measured: profiles/r19_closed_loop_tangent.md).
3. Transpose identity against tsim_push_closed_backward, per environment and direction, none left out, in the measure of
   tests/test_gpu_tangent.py::_identity_errors.  Bounds: the project's caps (1e-10 fp64, 1e-4 fp32) and 10 x the largest error of the OPEN-loop
   identity (tangent_episode against backward_episode) of the parent commit's kernels on the same closed roll-out tapes, measured once
   (tools/measure_closed_loop_tangent.py --floor; profiles/r19_closed_loop_tangent.md): fp64 8.969e-16, fp32 1.903e-7 over 1260 (environment, direction) pairs each -> IDENT_BOUND.
4. Against the oracle-pinned per-step loop of tests/test_gpu_closed_loop_param_grad.py: dloss along eight unit table directions equals that
   file's table gradient, dloss along a random policy direction equals <grad, dtheta> of the per-step autograd loop; its measure, its bounds.
5. Conventions: directions independent of ndir, backward() unchanged by tangent calls, exact zeros, refusals, graph replay, run to run."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_gpu_closed_loop_param_grad as PG      # noqa: E402
from param_grad_util import ALL      # noqa: E402

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
B0, T0, SEED0, PUSH = PG.B0, PG.T0, PG.SEED0, PG.PUSH
CAP = {F64: 1e-10, F32: 1e-4}                     # the project's hard caps on a transpose identity
OPEN_FLOOR = {F64: 8.969e-16, F32: 1.903e-7}         # largest open-loop identity error of the parent's kernels on these tapes (module docstring, 3.)
IDENT_BOUND = {dt: min(CAP[dt], 10 * OPEN_FLOOR[dt]) for dt in (F64, F32)}
# (observation, per-environment tables, push)
CONFIGS = [("tactile_flatten", False, 0.0), ("tactile_flatten", True, 0.0), ("tactile_flatten", False, PUSH), ("tactile_flatten", True, PUSH),
           ("privilege", False, 0.0), ("privilege", True, PUSH), ("no_tactile", False, PUSH)]


def _rollout(dtype, lanes, obs, tables, push, groups=("contact",), T=T0, buf=True):
    """a recorded closed roll-out on a fresh batch -> (episode, table-gradient buffer or None)"""
    from tactilesimulation_amd.envs.push_closed_loop import FusedPushEpisode
    q0, goal, dist = (torch.tensor(a, device="cuda", dtype=dtype) for a in PG._episode(B0, T, SEED0))
    env = PG._env(dtype, lanes, obs, tables, B0, T)
    gbuf = PG._new_buf(env.sim) if buf else None
    env.sim.set_param_grad_groups(groups)
    env.sim.set_param_grad(gbuf)
    ep = FusedPushEpisode(env, PG._actor(obs, dtype, push), T)
    ep.rollout(q0, goal, dist)
    assert int((ep.status != 0).sum()) == 0
    assert env.sim.tape_len() == T * env.frame_skip
    return ep, gbuf


def _table_columns(body):
    m = PG._model()
    return [c for (_, _, _, c) in m.param_columns() + (m.body_param_columns() if body else [])]


def _directions(ep, nd, seed, body, T=T0):
    """random directions in every input of the call: sources on the three layers, dact, dtac0, dq0, dqd0, dtables (contact columns; body: the body
    groups' columns too), each entry of the size of what it perturbs"""
    rng = np.random.default_rng(seed)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), device="cuda", dtype=ep.dt)
    base = ep.sim.base_tables().double().cpu().numpy()
    cols = _table_columns(body)
    dtab = np.zeros((nd,) + base.shape)
    dtab[:, :, cols] = rng.normal(size=(nd, B0, len(cols))) * (np.abs(base[:, cols]) + 0.1)
    n = lambda *s: rng.normal(size=s)
    return dict(sources=(t(n(nd, T, B0, 64)), t(n(nd, T, B0, 64)), t(n(nd, T, B0, 3))), dact=t(n(nd, T, B0, 6)), dtac0=t(1e-2 * n(nd, B0, 390)),
                dq0=t(1e-2 * n(nd, B0, 7)), dqd0=t(1e-1 * n(nd, B0, 7)), dtables=t(dtab))


@functools.lru_cache(maxsize=None)
def _case(dtype, lanes, obs, tables, push, body):
    """One roll-out per case, shared by tests 1 - 3 and never written to afterwards: the closed call along three random directions, the open-loop
    call fed its du on the same tape, then the closed adjoint with random seeds."""
    groups = ALL if body else ("contact",)
    ep, gbuf = _rollout(dtype, lanes, obs, tables, push, groups)
    sim, S = ep.sim, ep.env.frame_skip
    v = _directions(ep, 3, 31, body)
    rng = np.random.default_rng(32)
    t = lambda x: torch.tensor(x, device="cuda", dtype=dtype)
    ep.df_dq, ep.df_dvar, ep.du_direct = t(rng.normal(size=(T0, B0, 7))), t(rng.normal(size=(T0, B0, 6))), t(rng.normal(size=(T0, B0, 3)))      # the seeds w
    o = ep.tangent(want=("q", "qd", "var", "tac"), **v)
    assert sim.tape_len() == T0 * S
    shape = ep.tangent_launch_info(3, True)
    assert shape == sim.tangent_launch_info(3, True) and shape["lanes_per_env"] == ep.tangent_launch_info(8, False)["lanes_per_env"]      # TS_K_TANGENT's rule
    opened = sim.tangent_episode(T0, S, du=o["du"], dq0=v["dq0"], dqd0=v["dqd0"], dtables=v["dtables"], want_qd=True)
    df_du = torch.zeros(T0, B0, 6, device="cuda", dtype=dtype)
    ep.backward(df_du=df_du)
    lq, lv = sim.get_adjoint()
    sim.set_param_grad(None)
    torch.cuda.synchronize()
    adj = dict(g=(ep.g1.clone(), ep.g2.clone(), ep.g3.clone()), df_du=df_du, dobs_tac0=ep.dobs_tac[0].clone() if ep.dobs_tac is not None else None,
               lq=lq, lv=lv, buf=gbuf)
    return dict(ep=ep, v=v, o=o, opened=opened, adj=adj, w=(ep.df_dq, ep.df_dvar, ep.du_direct), shape=shape)


CASES = [(dt, l) + c for dt in (F64, F32) for l in (16, 32, 64) for c in CONFIGS]
_ids = lambda p: "-".join(str(x).replace("torch.", "") for x in p)


# ---------------------------------------------------------------------------------------------------- 1. the sim half, bit for bit
@pytest.mark.parametrize("body", [False, True], ids=["contact", "all_groups"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_sim_half_equals_the_open_loop_kernel_fed_the_closed_du(case, body):
    dtype, lanes, obs, tables, push = case
    c = _case(dtype, lanes, obs, tables, push, body)
    o, p = c["o"], c["opened"]
    assert float(o["du"].abs().max()) > 0 and float(o["dq"].abs().max()) > 0
    for k, k2 in (("dq", "dq"), ("dqd", "dqd"), ("dvar", "dvar"), ("dtac", "dtactile")):
        assert torch.equal(o[k], p[k2]), (k, float((o[k] - p[k2]).abs().max()))
    if push:
        assert float(o["dtac"].abs().max()) > 0 and float(o["dtac"][:, -1].abs().max()) > 0      # the last frame's row is written (and observed by nobody)
    elif obs == "tactile_flatten":                                                                # that actor at push = 0 never brings the pad to the box
        assert int((c["ep"].tac != 0).sum()) == 0
        assert int((o["dtac"] != 0).sum()) == 0                                                   # no tactile contact: every sensor term exactly zero


# ---------------------------------------------------------------------------------------------------- 2. the policy half against plain torch
def _torch_policy_jvp(c, dt):
    """du [nd, T, B, 6] and dupol [nd, T, B, 3] by a manual forward-mode pass of the actor in precision dt, from the closed call's own dq, dtac,
    the records and the sources"""
    ep, v, o = c["ep"], c["v"], c["o"]
    d = lambda x: x.to(dt)
    W1, b1, W2, b2, W3, b3 = (d(m) for lin in ep.lin for m in (lin.weight.detach(), lin.bias.detach()))
    s1, s2, s3 = (d(s) for s in v["sources"])
    nd, T, B = s1.shape[0], ep.T, ep.B
    qb = d(torch.cat([ep.q0.unsqueeze(0), ep.q[:-1]], dim=0))                                  # the state before every frame
    dqb = torch.cat([torch.zeros(nd, 1, B, 7, device="cuda", dtype=dt), d(o["dq"])[:, :-1]], dim=1)      # its tangent; frame 0: zero (the convention)
    sn, cs = torch.sin(qb[:, :, 0]), torch.cos(qb[:, :, 0])
    g = d(ep.goal).unsqueeze(0)
    gx, gy, ox, oy = g[:, :, 0], g[:, :, 1], qb[:, :, 3], qb[:, :, 4]
    dgl = torch.stack([(-sn * gx + cs * gy) * dqb[..., 0] - dqb[..., 1], (-cs * gx - sn * gy) * dqb[..., 0] - dqb[..., 2], -dqb[..., 0]], dim=-1)
    if ep.mode == 0:
        dtp = torch.cat([d(v["dtac0"]).unsqueeze(1), d(o["dtac"])[:, :-1]], dim=1)
        dobs = torch.cat([dgl, dtp], dim=-1)
    elif ep.mode == 1:
        dobs = dgl
    else:
        dobj = torch.stack([(-sn * ox + cs * oy) * dqb[..., 0] + cs * dqb[..., 3] + sn * dqb[..., 4] - dqb[..., 1],
                            (-cs * ox - sn * oy) * dqb[..., 0] - sn * dqb[..., 3] + cs * dqb[..., 4] - dqb[..., 2], dqb[..., 6] - dqb[..., 0]], dim=-1)
        dobj[:, 0] = 0
        dobs = torch.cat([dobj, dgl], dim=-1)
    elu_grad = lambda h: torch.where(h > 0, torch.ones_like(h), h + 1)
    dh1 = elu_grad(d(ep.h1)) * (dobs @ W1.t() + s1)
    dh2 = elu_grad(d(ep.h2)) * (dh1 @ W2.t() + s2)
    dupol = dh2 @ W3.t() + s3
    du = d(v["dact"]).clone()
    du[..., 0:3] += (1 - torch.tanh(d(ep.u)) ** 2) * dupol
    return du, dupol


def _frame_err(got, ref):
    """largest |got - ref| of a (direction, frame) over that frame's scale max |ref|: [nd, T]"""
    scale = ref.abs().amax(dim=(2, 3))
    assert float(scale.min()) > 0
    return (got.double() - ref).abs().amax(dim=(2, 3)) / scale


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_policy_half_equals_a_torch_forward_mode_pass(case):
    dtype, lanes, obs, tables, push = case
    c = _case(dtype, lanes, obs, tables, push, False)
    du64, dupol64 = _torch_policy_jvp(c, F64)
    e_du, e_up = _frame_err(c["o"]["du"], du64), _frame_err(c["o"]["dupol"], dupol64)
    worst = max(float(e_du.max()), float(e_up.max()))
    if dtype == F64:
        bound = 1e-12
    else:
        du32, dupol32 = _torch_policy_jvp(c, F32)
        bound = 4 * max(float(_frame_err(du32, du64).max()), float(_frame_err(dupol32, dupol64).max()))
    print("closed tangent policy half %s: max %.3e (du %.3e dupol %.3e) bound %.3e" % (_ids(case), worst, float(e_du.max()), float(e_up.max()), bound))
    assert worst <= bound, (case, worst, bound)


# ---------------------------------------------------------------------------------------------------- 3. transpose identity against the closed adjoint
def _closed_identity_errors(c):
    """[nd, B]: |<w, J v> - <J^T w, v>| / (sum |w_i (J v)_i| + sum |(J^T w)_j v_j|), the measure of tests/test_gpu_tangent.py::_identity_errors"""
    d = lambda x: x.double()
    o, v, a, (wq, wv, wu) = c["o"], c["v"], c["adj"], c["w"]
    lhs = lhs_a = 0
    for out, w in ((o["dq"], wq), (o["dvar"], wv), (o["dupol"], wu)):
        x = d(out) * d(w).unsqueeze(0)
        lhs, lhs_a = lhs + x.sum((1, 3)), lhs_a + x.abs().sum((1, 3))
    rhs = rhs_a = 0
    for vin, grad in zip(v["sources"] + (v["dact"],), a["g"] + (a["df_du"],)):
        x = d(vin) * d(grad).unsqueeze(0)
        rhs, rhs_a = rhs + x.sum((1, 3)), rhs_a + x.abs().sum((1, 3))
    pairs = [(v["dq0"], a["lq"]), (v["dqd0"], a["lv"]), (v["dtables"], a["buf"])]
    if a["dobs_tac0"] is not None:
        pairs.append((v["dtac0"], a["dobs_tac0"]))
    for vin, grad in pairs:
        x = d(vin) * d(grad).unsqueeze(0)
        rhs, rhs_a = rhs + x.sum(2), rhs_a + x.abs().sum(2)
    err = ((lhs - rhs).abs() / (lhs_a + rhs_a)).cpu().numpy()
    assert np.all(np.isfinite(err)) and float((lhs_a + rhs_a).min()) > 0
    return err


@pytest.mark.parametrize("body", [False, True], ids=["contact", "all_groups"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_transpose_identity_against_the_closed_adjoint(case, body):
    dtype, lanes, obs, tables, push = case
    c = _case(dtype, lanes, obs, tables, push, body)
    err = _closed_identity_errors(c)
    print("closed tangent identity %s body %d (k_closed_tangent at %d lanes): max %.3e median %.3e" % (_ids(case), body, c["shape"]["lanes_per_env"], err.max(), np.median(err)))
    # dloss is the left-hand side
    lhs = sum((x.double() * w.double().unsqueeze(0)).sum((1, 3)) for x, w in zip((c["o"]["dq"], c["o"]["dvar"], c["o"]["dupol"]), c["w"]))
    assert float((c["o"]["dloss"].double() - lhs).abs().max()) <= (1e-12 if dtype == F64 else 1e-4) * float(lhs.abs().max())
    assert err.max() <= IDENT_BOUND[dtype], (case, body, err)


# ---------------------------------------------------------------------------------------------------- 4. against the oracle-pinned per-step loop
def _unit_columns():
    """pair kn kt mu, sensor kn kt, box dof damping, box mass, a motor's P: (kind, column), the entries tests/test_gpu_closed_loop_param_grad.py randomises"""
    import tactilesimulation_amd.model.blob as BL
    I = PG._model().I
    fp, fs, fd, fl, fm = (int(I[k]) for k in (BL.TSIM_IH_FOFF_PAIR, BL.TSIM_IH_FOFF_SENSOR, BL.TSIM_IH_FOFF_DOF, BL.TSIM_IH_FOFF_LINK, BL.TSIM_IH_FOFF_MOTOR))
    pair = fp + BL.TSIM_PF_SIZE
    return [("pair", pair + BL.TSIM_PF_KN), ("pair", pair + BL.TSIM_PF_KT), ("pair", pair + BL.TSIM_PF_MU), ("sensor", fs + BL.TSIM_SF_KN), ("sensor", fs + BL.TSIM_SF_KT),
            ("dof", fd + 6 * BL.TSIM_DF_SIZE + BL.TSIM_DF_DAMPING), ("link", fl + 3 * BL.TSIM_LF_SIZE + BL.TSIM_LF_MASS), ("motor", fm + BL.TSIM_MF_P)]


def _per_step_policy_loss(dtype, lanes, obs, tables, push):
    """the per-step autograd loop of tests/test_gpu_closed_loop_param_grad.py::_per_step, keeping the graph: per-environment loss [B], signatures, actor"""
    q0, goal, dist = (torch.tensor(a, device="cuda", dtype=dtype) for a in PG._episode(B0, T0, SEED0))
    actor = PG._actor(obs, dtype, push)
    env = PG._env(dtype, lanes, obs, tables, B0, T0)
    o = env.reset(q0, goal)
    total = o.new_zeros(B0)
    for t in range(T0):
        o, rew, _ = env.step(actor(o), dist[t])
        total = total - rew
    return total, env.sim.branch_signature(), actor, env


@pytest.mark.parametrize("obs,tables,push", PG.CONFIGS)
@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("dtype", [F64, F32])
def test_dloss_equals_the_per_step_loops_gradients(dtype, lanes, obs, tables, push):
    ref, sig_ref, _, _ = PG._per_step(dtype, lanes, obs, tables, B0, T0, SEED0, push=push)      # [B, table_size], pinned to the oracle's parameter adjoint
    ep, _ = _rollout(dtype, lanes, obs, tables, push, ALL, buf=False)
    sim = ep.sim
    same = PG._same_piece(sim.branch_signature(), sig_ref)
    assert bool(same.all()) if dtype == F64 else int((~same).sum()) <= B0 // 10, same
    units = _unit_columns()
    dtab = torch.zeros(len(units), B0, ref.shape[1], device="cuda", dtype=dtype)
    for d, (_, col) in enumerate(units):
        dtab[d, :, col] = 1
    dloss = ep.tangent(dtables=dtab)["dloss"].double()                                         # one launch, eight columns
    by_kind, _ = PG._columns()
    errs = []
    for d, (kind, col) in enumerate(units):
        assert col in by_kind[kind], (kind, col)
        r = ref.double()[:, torch.tensor(by_kind[kind], device="cuda")]
        batch_scale = float(r.abs().max())
        rc = ref.double()[:, col]
        if batch_scale == 0.0:                                                                 # that file: a kind that is zero in the whole yardstick is exactly zero here
            assert int((dloss[d] != 0).sum()) == 0, (kind, col, float(dloss[d].abs().max()))
            continue
        scale = r.abs().max(dim=1).values
        scale = torch.where(scale > 0, scale, torch.full_like(scale, batch_scale))
        errs.append(((dloss[d] - rc).abs() / scale)[same])
    # a random direction over all six policy tensors, three of them: dloss summed over the kept environments = <grad, dtheta> of the per-step loop
    total, sig_ps, actor, env_ps = _per_step_policy_loss(dtype, lanes, obs, tables, push)
    keep = same & PG._same_piece(sim.branch_signature(), sig_ps)
    params = [p for lin in [m for m in actor.mu_net if isinstance(m, torch.nn.Linear)] for p in (lin.weight, lin.bias)]
    grads = torch.autograd.grad((total * keep.to(dtype)).sum(), params)
    gen = torch.Generator().manual_seed(41)
    dth = tuple(torch.randn((3,) + tuple(p.shape), generator=gen, dtype=torch.float64).to("cuda", dtype) for p in params)
    dl = ep.tangent(dtheta=dth)["dloss"].double()
    got = (dl * keep.double().unsqueeze(0)).sum(1)
    per_tensor = torch.stack([(g.double().unsqueeze(0) * t.double()).flatten(1).sum(1) for g, t in zip(grads, dth)])      # [6, 3]
    errs.append((got - per_tensor.sum(0)).abs() / per_tensor.abs().sum(0))
    flat = torch.cat([e.reshape(-1) for e in errs])
    worst, p99 = float(flat.max()), float(torch.quantile(flat, 0.99))
    print("closed tangent dloss vs per-step %s lanes %d %s tables %d push %.1f: max %.3e p99 %.3e over %d pairs (policy directions: %s)" % (
        dtype, lanes, obs, tables, push, worst, p99, flat.numel(), " ".join("%.2e" % float(x) for x in errs[-1])))
    if dtype == F64:
        assert worst < PG.TOL64, worst
    else:
        assert worst < PG.TOL32_MAX and p99 < PG.TOL32_P99, (worst, p99)


# ---------------------------------------------------------------------------------------------------- 5. conventions
@pytest.mark.parametrize("dtype,lanes", [(F64, 64), (F32, 16)])
def test_directions_are_independent_of_ndir_and_of_each_other(dtype, lanes):
    ep, _ = _rollout(dtype, lanes, "tactile_flatten", True, PUSH, ALL, buf=False)
    v = _directions(ep, 8, 51, True)
    take = lambda sel: {k: (tuple(x[sel] for x in t) if isinstance(t, tuple) else t[sel]) for k, t in v.items()}
    o8 = ep.tangent(want=("q", "qd", "var", "tac"), **v)
    o3 = ep.tangent(want=("q", "qd", "var", "tac"), **take([5, 0, 2]))
    o1 = ep.tangent(want=("q", "qd", "var", "tac"), **take([5]))
    for k in ("dq", "dqd", "dvar", "dtac", "dupol", "du", "dloss"):
        assert float(o8[k].abs().max()) > 0
        assert torch.equal(o3[k], o8[k][[5, 0, 2]]) and torch.equal(o1[k], o8[k][[5]]), k


def _backward_bits(dtype, lanes, ncalls):
    ep, gbuf = _rollout(dtype, lanes, "tactile_flatten", True, PUSH, ALL)
    for i in range(ncalls):
        ep.tangent(want=("q", "qd", "var", "tac"), **_directions(ep, 2 + 3 * i, 61 + i, True))
    assert ep.sim.tape_len() == T0 * ep.env.frame_skip
    ep.backward()
    out = [p.grad.clone() for n, p in ep.actor.named_parameters() if n != "logstd"] + list(ep.sim.get_adjoint()) + [gbuf, ep.g1, ep.g2, ep.g3, ep.dobs_tac]
    assert ep.sim.tape_len() == 0
    ep.sim.set_param_grad(None)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype,lanes", [(F64, 32), (F32, 16)])
def test_backward_after_two_tangent_calls_returns_the_bits_of_a_run_without(dtype, lanes):
    a, b = _backward_bits(dtype, lanes, 0), _backward_bits(dtype, lanes, 2)
    assert float(a[-5].abs().max()) > 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_refusals_launch_nothing():
    from tactilesimulation_amd.host import capi
    ep, _ = _rollout(F32, 16, "tactile_flatten", False, PUSH, buf=False)
    sim, S, L = ep.sim, ep.env.frame_skip, capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    sent = lambda *s: torch.full(s, 7.0, device="cuda", dtype=F32)
    outs = dict(dq=sent(1, T0 + 1, B0, 7), dtac=sent(1, T0 + 1, B0, 390), du=sent(1, T0 + 1, B0, 6))

    def call(b=sim._h, pol=C.byref(ep._pol), T=T0, ndir=1, dtac=outs["dtac"]):
        return L.tsim_push_closed_tangent(b, pol, p(ep.goal), T, S, ndir, p(ep.u), p(ep.h1), p(ep.h2), None, None, None, None, None, None, None, None,
                                          p(outs["dq"]), None, None, p(dtac), None, p(outs["du"]), None)

    def refused(rc, word):
        torch.cuda.synchronize()
        assert rc != 0 and word in L.tsim_last_error().decode(), (rc, L.tsim_last_error())
        assert all(bool((t == 7.0).all()) for t in outs.values())
    refused(call(b=None), "null")
    refused(call(pol=None), "null")
    refused(call(ndir=0), "ndir")
    refused(call(ndir=9), "ndir")
    refused(call(T=T0 + 1), "tape")                     # a window longer than the tape
    refused(call(dtac=None), "dtac_out")
    mean = torch.zeros(393, device="cuda", dtype=F32)
    ep._pol.obs_mean, ep._pol.obs_istd = mean.data_ptr(), mean.data_ptr()
    refused(call(), "obs_mean")
    ep._pol.obs_mean, ep._pol.obs_istd = None, None
    assert call() == 0                                  # ... and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert not bool((outs["du"][:, :T0] == 7.0).any())
    for t in outs.values():
        t.fill_(7.0)
    ep.backward()
    refused(call(), "tape")                             # the tape is gone
    with pytest.raises(RuntimeError):
        ep.tangent()
    ep2, _ = _rollout(F32, 16, "no_tactile", False, PUSH, buf=False)      # without the tactile observation dtac_out is optional: the read-out tangent is skipped
    o = ep2.tangent(want=("q",))
    assert "dtac" not in o and float(o["dq"].abs().max()) == 0 and int((o["du"] != 0).sum()) == 0      # one zero direction


def test_captured_tangent_replays_to_eager():
    """modelled on tests/test_gpu_closed_loop_param_grad.py::test_captured_fused_backward_replays_to_eager: one stream, a warm-up call of that size first
    (the body columns' workspace grows only outside a capture)"""
    dtype, T = F32, 4
    ep, _ = _rollout(dtype, 16, "tactile_flatten", False, PUSH, ALL, T=T, buf=False)
    v = _directions(ep, 3, 71, True, T=T)
    eager = ep.tangent(want=("q", "qd", "var", "tac"), **v)
    q0, goal, dist = ep.q0, ep.goal, torch.tensor(PG._episode(B0, T, SEED0)[2], device="cuda", dtype=dtype)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ep.rollout(q0, goal, dist)
        ep.tangent(want=("q", "qd", "var", "tac"), **v)                  # warm-up on the capture's stream
        held = (ep.goal, ep.q0, ep.tac0, ep._w, ep.df_dq, ep.df_dvar, ep.du_direct)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cap = ep.tangent(want=("q", "qd", "var", "tac"), **v)
        for _ in range(2):
            ep.rollout(q0, goal, dist)
            for t in cap.values():
                t.zero_()
            graph.replay()
            side.synchronize()
            for k in ("dq", "dqd", "dvar", "dtac", "dupol", "du"):
                assert torch.equal(cap[k], eager[k]), k
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    del held


def test_two_runs_from_scratch_give_the_same_bits():
    outs = []
    for _ in range(2):
        ep, _ = _rollout(F32, 16, "tactile_flatten", True, PUSH, ALL, buf=False)
        outs.append(ep.tangent(want=("q", "qd", "var", "tac"), **_directions(ep, 8, 81, True)))
        torch.cuda.synchronize()
    for k in outs[0]:
        assert float(outs[0][k].abs().max()) > 0 and torch.equal(outs[0][k], outs[1][k]), k


def test_the_trajectory_sensitivity_example_runs():
    """examples/closed_loop_trajectory_sensitivity.py: one launch, eight columns, beside the secant of +-1 % re-simulations (printed by the example; a
    secant over a contact model's kinks has no bound to hold the tangent to, so only what is exact is asserted)"""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
    import closed_loop_trajectory_sensitivity as ex
    r = ex.run(B=4, T=6, verbose=False)
    assert r["columns"][-1] == "motor P" and len(r["columns"]) == 8
    assert tuple(r["tangent"].shape) == (8, 4, 3) and bool(torch.isfinite(r["tangent"]).all()) and bool(torch.isfinite(r["secant"]).all())
    assert float(r["tangent"][0].abs().max()) > 0 and float(r["tangent"][6].abs().max()) > 0      # pair kn, box mass
    assert int((r["tangent"][7] != 0).sum()) == 0 and int((r["secant"][7] != 0).sum()) == 0        # force control: a motor's P moves nothing, exactly
