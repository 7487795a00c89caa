"""The per-environment table gradient behind the fused closed loop (include/tsim_env.h tsim_push_closed_backward with a tsim_set_param_grad buffer
set; FusedPushEpisode.backward with sim.set_param_grad(buf)): k_closed_backward_z saves z of every sub-step, the contact pass and the body groups'
pass follow it on the stream.

The yardstick is the per-step autograd loop of tests/test_gpu_closed_loop.py (BatchedTactilePushEnv.step + Actor + torch.autograd.grad) run with
env.sim.set_param_grad(buf_ref) set, so that every per-step adjoint launch adds its share: that path is pinned to the fp64 oracle's own parameter
adjoint by tests/test_gpu_param_grad_oracle.py and tests/test_gpu_body_param_grad_oracle.py.  Same episode, same policy, same tables: the two
buffers must agree per (environment, column).

Error measure: |fused - per-step| divided by the largest |per-step value| among that environment's columns of the same kind (pair, sensor,
damping, link, motor, limit).  An environment whose columns of a kind are all zero in the yardstick (no tactile contact: sensor) has no scale of
its own: the kind's largest value in the batch stands in; a kind that is zero in the whole batch must be EXACTLY zero in the fused run too.
TactilePush has no joint limit (lim_k = 0 on every dof), so the limit columns are exactly zero in both runs — asserted as such.

Two policies.  The episode of tests/test_gpu_closed_loop.py (B = 10, T = 12, episode seed 3, the seed-1 actor scaled by 3) never brings the pad to
the box: in the per-step yardstick every sensor column is exactly zero, in fp64 and fp32, shared and per-environment tables alike — that episode
checks the pair, damping, link and motor columns and that the sensor columns stay exactly zero.  The tactile seeds (dobs_tac[f + 1], the -1 slot of
the last frame) are what this feature adds, so every case also runs with a PRESSING policy: the same actor with PUSH added to the output bias of
the gripper's forward motor.  PUSH was chosen on the per-step loop alone (0.5, 1.0, 1.5, 2.5 tried: from 1.0 on all ten environments get a
sensor gradient; at 1.5 fp32 keeps all ten on fp64's stick / slip pieces, with shared and with per-environment tables), never on a fused result."""
import functools
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.abspath(__file__)))
from _report import rep as _rep
import numpy as np
import pytest
import torch

from param_grad_util import ALL, layout_kind

pytestmark = pytest.mark.gpu

KINDS = ("pair", "sensor", "dof", "link", "motor", "limit")      # 'dof': the damping columns
TOL64 = 1e-7      # the bound tests/test_gpu_closed_loop.py holds the same two computations to for the policy gradient; measured maximum 7.7e-13
# fp32: fused against per-step compares two fp32 evaluations of the same sums in another order, on controls that carry the in-kernel policy's
# rounding.  The floor is per-step fp32 against per-step fp64 in the same measure over all parametrisations of test 1 (the parent's code only);
# the bounds are 4 x that floor's 99th percentile, which 99 % of a run's compared pairs must meet, and 4 x its maximum, which every pair must
# meet.  Floor and fused distributions side by side: profiles/r15_closed_loop_param_grad.md.
TOL32_P99 = 4 * 2.61e-6      # floor: 99th percentile 2.61e-6 over 12090 pairs (fused fp32: 8.8e-7)
TOL32_MAX = 4 * 8.22e-5      # floor: maximum 8.22e-5 (fused fp32: 4.6e-5)


def _episode(B, T, seed, advance=0.0):
    """tests/test_gpu_closed_loop.py _episode; advance: the gripper starts that much closer to the box (0: that file's episode)"""
    rng = np.random.default_rng(seed)
    q0 = np.zeros((B, 7)); q0[:, 1] = -0.001 + advance; q0[:, 4] = rng.uniform(-0.02, 0.02, size=B)
    goal = np.zeros((B, 3)); goal[:, 0:2] = rng.uniform([0.15, -0.2], [0.25, 0.2], size=(B, 2))
    goal[:, 2] = rng.uniform(goal[:, 1] * np.pi - np.pi / 16.0, goal[:, 1] * np.pi + np.pi / 16.0)
    dist = rng.uniform(-1.0, 1.0, size=(T, B, 2)) * (rng.uniform(size=(T, B, 1)) < 0.5)
    return q0, goal, dist


def _randomised_tables(sim, model, B, seed=4):
    """One parameter table per environment (tests/test_gpu_closed_loop.py _randomised_tables)"""
    import tactilesimulation_amd.model.blob as BL
    I = model.I
    fp, fs, fd, fl = (int(I[k]) for k in (BL.TSIM_IH_FOFF_PAIR, BL.TSIM_IH_FOFF_SENSOR, BL.TSIM_IH_FOFF_DOF, BL.TSIM_IH_FOFF_LINK))
    tab = sim.base_tables()
    r = torch.rand(B, 6, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(tab)
    tab[:, fp + BL.TSIM_PF_SIZE + BL.TSIM_PF_KN] *= 0.7 + 0.6 * r[:, 0]
    tab[:, fp + BL.TSIM_PF_SIZE + BL.TSIM_PF_MU] *= 0.5 + r[:, 1]
    tab[:, fs + BL.TSIM_SF_KN] *= 0.7 + 0.6 * r[:, 2]
    tab[:, fs + BL.TSIM_SF_KT] *= 0.7 + 0.6 * r[:, 3]
    tab[:, fd + 6 * BL.TSIM_DF_SIZE + BL.TSIM_DF_DAMPING] = 0.01 + 0.1 * r[:, 4]
    scale = 0.8 + 0.4 * r[:, 5]
    for e in (BL.TSIM_LF_MASS, BL.TSIM_LF_INERTIA, BL.TSIM_LF_INERTIA + 1, BL.TSIM_LF_INERTIA + 2):
        tab[:, fl + 3 * BL.TSIM_LF_SIZE + e] *= scale
    return tab


@functools.lru_cache(maxsize=None)
def _model():
    from tactilesimulation_amd.model.compiler import load_model
    from tactilesimulation_amd.workloads import asset
    return load_model(asset("pusher"))


@functools.lru_cache(maxsize=None)
def _columns():
    """{kind: [column]} of every column a gradient is computed for, and (kind, field) -> [column]"""
    m = _model()
    by_kind, by_field = {k: [] for k in KINDS}, {}
    for kind, _, f, c in m.param_columns() + m.body_param_columns():
        by_kind[kind].append(c)
        by_field.setdefault((kind, f), []).append(c)
    return by_kind, by_field


NIN = {"tactile_flatten": 393, "no_tactile": 3, "privilege": 6}


def _actor(obs, dtype, push=0.0):
    """the actor of tests/test_gpu_closed_loop.py (seed 1, scaled by 3); push: added to the output bias of the gripper's forward motor, so that the
    policy also drives the pad into the box (0: that file's actor)"""
    from tactilesimulation_amd.algorithms.batched_gd import Actor
    torch.manual_seed(1)
    actor = Actor(obs_dim=NIN[obs], dtype=dtype).cuda()
    with torch.no_grad():                                            # a policy that acts (the initial one outputs ~0)
        for p in actor.parameters():
            p.mul_(3.0)
        [m for m in actor.mu_net if isinstance(m, torch.nn.Linear)][-1].bias[0] += push
    return actor


def _env(dtype, lanes, obs, tables, B, T):
    from tactilesimulation_amd.envs.tactile_push import BatchedTactilePushEnv
    env = BatchedTactilePushEnv(_model(), B, dtype=dtype, gradient=True, seed=0, tape_steps=T, observation_type=obs)
    env.sim.set_lanes_per_env(lanes)
    if tables:
        env.sim.set_env_tables(_randomised_tables(env.sim, _model(), B))
    return env


def _new_buf(sim, fill=None):
    n = sim.base_tables().shape[1]
    if fill is None:
        return torch.zeros(sim.B, n, device="cuda", dtype=sim.dtype)
    return _sentinel(sim.B, n, sim.dtype, fill)


def _sentinel(B, n, dtype, fill):
    e, c = torch.meshgrid(torch.arange(B, dtype=torch.float64), torch.arange(n, dtype=torch.float64), indexing="ij")
    return (fill + c + 0.5 * e).to("cuda", dtype).contiguous()      # a pattern that names its place: exact in fp32


@functools.lru_cache(maxsize=None)
def _per_step(dtype, lanes, obs, tables, B, T, seed, groups=ALL, push=0.0, advance=0.0):
    """The yardstick, once per case (shared, never written to): the per-step loop with autograd, the table gradient of `groups` into a zeroed buffer.
    -> (buffer [B, table_size], branch signatures [T frame_skip, B, 2], loss, kernel variant)"""
    q0, goal, dist = (torch.tensor(a, device="cuda", dtype=dtype) for a in _episode(B, T, seed, advance))
    actor = _actor(obs, dtype, push)
    env = _env(dtype, lanes, obs, tables, B, T)
    buf = _new_buf(env.sim)
    env.sim.set_param_grad_groups(groups)
    env.sim.set_param_grad(buf)
    o = env.reset(q0, goal)
    total = o.new_zeros(())
    for t in range(T):
        o, rew, _ = env.step(actor(o), dist[t])
        total = total - rew.sum()
    sig = env.sim.branch_signature()
    torch.autograd.grad(total, [p for n, p in actor.named_parameters() if n != "logstd"])
    env.sim.set_param_grad(None)
    assert env.sim.tape_len() == 0
    torch.cuda.synchronize()
    return buf, sig, float(total.detach()), env.sim.kernel_variant()


def _fused(dtype, lanes, obs, tables, B, T, seed, groups=ALL, buf="zero", episodes=1, df_du=False, push=0.0, advance=0.0):
    """The fused episode(s) with the table gradient of `groups` adding into buf ("zero": a zeroed buffer; None: no buffer set; a tensor: that one).
    -> dict of everything the launch leaves"""
    from tactilesimulation_amd.envs.push_closed_loop import FusedPushEpisode
    q0, goal, dist = (torch.tensor(a, device="cuda", dtype=dtype) for a in _episode(B, T, seed, advance))
    actor = _actor(obs, dtype, push)
    env = _env(dtype, lanes, obs, tables, B, T)
    sim = env.sim
    if isinstance(buf, str):
        buf = _new_buf(sim)
    sim.set_param_grad_groups(groups)
    sim.set_param_grad(buf)
    ep = FusedPushEpisode(env, actor, T)
    du = torch.zeros(T, B, 6, device="cuda", dtype=dtype) if df_du else None
    after = []
    for _ in range(episodes):
        loss = ep.rollout(q0, goal, dist)
        assert int((ep.status != 0).sum()) == 0
        sig = sim.branch_signature()
        ep.backward(df_du=du)
        assert sim.tape_len() == 0
        if buf is not None:
            after.append(buf.clone())
    launch = sim.last_adjoint_launch()
    lq, lv = sim.get_adjoint()
    sim.set_param_grad(None)
    torch.cuda.synchronize()
    named = [(n, p.grad.clone()) for n, p in actor.named_parameters() if n != "logstd"]
    return dict(buf=buf, after=after, sig=sig, loss=float(loss), variant=sim.kernel_variant(), launch=launch, ep=ep, sim=sim, env=env, actor=actor,
                grads=named, adjoint=(lq, lv), df_du=du, g=(ep.g1, ep.g2, ep.g3), dobs_tac=ep.dobs_tac)


def _same_piece(sig_a, sig_b):
    """[B] bool: the environment is on the same contact / friction branches in both runs over the whole taped window"""
    return (sig_a == sig_b).all(dim=2).all(dim=0)


def _errors(got, ref, keep=None):
    """The module's error measure per compared (environment, column): {kind: tensor [kept environments, columns of the kind]}; a kind that is zero
    in the whole yardstick is asserted to be exactly zero in `got` and left out."""
    by_kind, _ = _columns()
    got, ref = got.double(), ref.double()
    if keep is not None:
        got, ref = got[keep], ref[keep]
    out = {}
    for kind in KINDS:
        c = torch.tensor(by_kind[kind], device=ref.device)
        r, g = ref[:, c], got[:, c]
        batch_scale = float(r.abs().max())
        if batch_scale == 0.0:
            assert int((g != 0).sum()) == 0, (kind, "zero in the yardstick, not in the fused run", float(g.abs().max()))
            continue
        scale = r.abs().max(dim=1, keepdim=True).values
        scale = torch.where(scale > 0, scale, torch.full_like(scale, batch_scale))
        out[kind] = (g - r).abs() / scale
    return out


def _check(got, ref, keep, dtype, tag, **where):
    """errors -> report, then the module's bounds"""
    errs = _errors(got, ref, keep)
    flat = torch.cat([e.reshape(-1) for e in errs.values()])
    worst, p99 = float(flat.max()), float(torch.quantile(flat, 0.99))
    for kind, e in errs.items():
        _rep("closed_loop_param_grad_" + tag, dtype=str(dtype), kind=kind, max=float(e.max()), median=float(e.median()), pairs=e.numel(), **where)
    _rep("closed_loop_param_grad_" + tag, dtype=str(dtype), kind="all", max=worst, p99=p99, pairs=flat.numel(), **where)
    print("closed-loop param grad %s %s %s: max %.3e p99 %.3e over %d pairs" % (tag, dtype, where, worst, p99, flat.numel()))
    if dtype == torch.float64:
        assert worst < TOL64, (tag, where, worst)      # measured maximum: see the module's profile note
    else:
        assert worst < TOL32_MAX and p99 < TOL32_P99, (tag, where, worst, p99)
    return errs


def _assert_nontrivial(ref, obs, push):
    by_kind, by_field = _columns()
    nz = lambda cols: float(ref[:, torch.tensor(cols, device=ref.device)].abs().max()) > 0.0
    for kind in ("pair", "dof", "link", "motor"):
        assert nz(by_kind[kind]), kind
    assert not nz(by_kind["limit"])      # TactilePush has no joint limit: lim_k = 0 on every dof, exactly zero (include/tsim.h TSIM_PG_LIMIT)
    for f in ("P", "D"):                 # force control: exactly zero (include/tsim.h TSIM_PG_MOTOR)
        assert not nz(by_field[("motor", f)]), f
    if obs == "tactile_flatten" and push:
        assert nz(by_field[("sensor", "kn")]) and nz(by_field[("sensor", "kt")])
    else:
        assert not nz(by_kind["sensor"])     # nothing observes the tactile output, or (push = 0) no taxel ever touches: exactly zero


PUSH = 1.5
# (observation, per-environment tables, push): the three configurations of tests/test_gpu_closed_loop.py on its episode, and the pressing policy
CONFIGS = [("tactile_flatten", False, 0.0), ("tactile_flatten", True, 0.0), ("privilege", False, 0.0),
           ("tactile_flatten", False, PUSH), ("tactile_flatten", True, PUSH)]
B0, T0, SEED0 = 10, 12, 3      # a batch that is no multiple of the slots per wavefront; the policy acts, contacts happen


# ---------------------------------------------------------------------------------------------------- 1. fused == per-step
@pytest.mark.parametrize("obs,tables,push", CONFIGS)
@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fused_table_gradient_equals_the_per_step_loop(dtype, lanes, obs, tables, push):
    ref, sig_ref, loss_ref, _ = _per_step(dtype, lanes, obs, tables, B0, T0, SEED0, push=push)
    f = _fused(dtype, lanes, obs, tables, B0, T0, SEED0, push=push)
    # the batch's view (tsim_kernel_variant): fp32 at four environments per wavefront runs the compiled-in closed-loop kernels; an fp64 batch at 16
    # lanes or with per-environment tables is generic throughout (at 32 / 64 lanes an fp64 batch reports its OPEN-loop view, the closed loop is generic)
    if dtype == torch.float32 and lanes == 16:
        assert f["variant"] == ("param:pusher" if tables else "static:pusher")
    elif dtype == torch.float64 and (lanes == 16 or tables):
        assert f["variant"] == "generic"
    assert f["launch"] == {"kernel": "k_closed_backward_z", "param_passes": ("k_param_grad", "k_param_grad_body")}
    _assert_nontrivial(ref, obs, push)
    same = _same_piece(f["sig"], sig_ref)
    if dtype == torch.float64:
        assert bool(same.all()), same
    else:
        assert int((~same).sum()) <= B0 // 10, same      # the two runs' controls differ in the last bits: at most 1 of 10 on another stick / slip piece
    _check(f["buf"], ref, same, dtype, "fused_vs_per_step", lanes=lanes, obs=obs, tables=int(tables), push=push)
    # the exact zeros of the yardstick are exact zeros here
    _, by_field = _columns()
    for fld in ("P", "D"):
        assert int((f["buf"][:, by_field[("motor", fld)]] != 0).sum()) == 0
    if obs != "tactile_flatten" or not push:
        assert int((f["buf"][:, _columns()[0]["sensor"]] != 0).sum()) == 0


# ---------------------------------------------------------------------------------------------------- 2. nothing else moves
@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_everything_else_keeps_its_bits_with_the_buffer_set(dtype, lanes):
    a = _fused(dtype, lanes, "tactile_flatten", False, B0, T0, SEED0, buf=None, df_du=True, push=PUSH)
    b = _fused(dtype, lanes, "tactile_flatten", False, B0, T0, SEED0, df_du=True, push=PUSH)
    assert a["launch"] == {"kernel": "k_backward", "param_passes": ()}      # no buffer: the kernel it always was, and no parameter pass
    assert b["launch"]["kernel"] == "k_closed_backward_z"
    assert float(b["buf"].abs().max()) > 0
    for x, y in zip(a["g"] + (a["dobs_tac"], a["df_du"]) + a["adjoint"], b["g"] + (b["dobs_tac"], b["df_du"]) + b["adjoint"]):
        assert torch.equal(x, y)
    assert float(a["df_du"].abs().max()) > 0
    for (n, x), (_, y) in zip(a["grads"], b["grads"]):
        assert torch.equal(x, y), n


def test_a_batch_that_never_saw_a_buffer_runs_k_backward():
    from tactilesimulation_amd.envs.push_closed_loop import FusedPushEpisode
    q0, goal, dist = (torch.tensor(a, device="cuda", dtype=torch.float32) for a in _episode(B0, 2, SEED0))
    env = _env(torch.float32, 16, "tactile_flatten", False, B0, 2)
    assert env.sim.last_adjoint_launch() == {"kernel": None, "param_passes": ()}
    ep = FusedPushEpisode(env, _actor("tactile_flatten", torch.float32), 2)
    ep.rollout(q0, goal, dist)
    ep.backward()
    assert env.sim.last_adjoint_launch() == {"kernel": "k_backward", "param_passes": ()}
    # ... and the open-loop launches say which twin they took
    buf = _new_buf(env.sim)
    env.sim.set_param_grad(buf)
    env.sim.reset(q0, None, backward_flag=True)
    env.sim.step(torch.zeros(B0, 6, device="cuda"), 2)
    env.sim.backward_steps(2, torch.ones(B0, 7, device="cuda"), torch.ones(B0, 6, device="cuda"), torch.ones(B0, 390, device="cuda"))
    assert env.sim.last_adjoint_launch() == {"kernel": "k_backward_z", "param_passes": ("k_param_grad",)}
    env.sim.set_param_grad(None)


# ---------------------------------------------------------------------------------------------------- 3. accumulate and leave alone
@pytest.mark.parametrize("dtype,lanes", [(torch.float64, 64), (torch.float32, 16)])
def test_the_gradient_adds_and_leaves_the_other_columns_alone(dtype, lanes):
    by_kind, _ = _columns()
    g0 = _fused(dtype, lanes, "tactile_flatten", False, B0, T0, SEED0, push=PUSH)["buf"]
    sent = _sentinel(B0, g0.shape[1], dtype, 1000.0)
    f = _fused(dtype, lanes, "tactile_flatten", False, B0, T0, SEED0, buf=sent.clone(), episodes=2, push=PUSH)
    on = torch.zeros(sent.shape[1], dtype=torch.bool, device="cuda")
    on[[c for k in KINDS for c in by_kind[k]]] = True
    first, second = f["after"]
    assert torch.equal(first[:, ~on], sent[:, ~on]) and torch.equal(second[:, ~on], sent[:, ~on])
    # each episode adds the same bits: one rounded addition of the episode's sum per column (k_param_reduce), twice
    assert torch.equal(first, sent + g0) and torch.equal(second, first + g0)
    eps = torch.finfo(dtype).eps
    assert float(((second - sent) - 2 * g0)[:, on].abs().max()) <= 4 * eps * float(second.abs().max())
    # one group only: every other group's columns keep the sentinel
    f = _fused(dtype, lanes, "tactile_flatten", False, B0, T0, SEED0, groups=("inertial",), buf=sent.clone(), push=PUSH)
    link = torch.zeros_like(on)
    link[by_kind["link"]] = True
    assert f["launch"]["param_passes"] == ("k_param_grad_body",)
    assert torch.equal(f["buf"][:, ~link], sent[:, ~link])
    assert torch.equal(f["buf"][:, link], (sent + g0)[:, link])
    assert float((f["buf"] - sent)[:, link].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 4. the last frame carries no tactile seed
@pytest.mark.parametrize("dtype,lanes", [(torch.float64, 64), (torch.float32, 16)])
def test_the_last_frame_carries_no_tactile_seed(dtype, lanes):
    by_kind, _ = _columns()
    f = _fused(dtype, lanes, "tactile_flatten", False, B0, 1, SEED0, push=PUSH)
    assert int((f["buf"][:, by_kind["sensor"]] != 0).sum()) == 0      # the episode's only tactile output is observed by nobody
    assert float(f["buf"][:, by_kind["pair"]].abs().max()) > 0 and float(f["buf"][:, by_kind["link"]].abs().max()) > 0
    ref1 = _per_step(dtype, lanes, "tactile_flatten", False, B0, 1, SEED0, push=PUSH)
    _check(f["buf"], ref1[0], _same_piece(f["sig"], ref1[1]), dtype, "one_frame", lanes=lanes)
    # two frames: frame 0 is seeded by frame 1's observation (row 1), frame 1 by nothing
    ref, sig_ref, _, _ = _per_step(dtype, lanes, "tactile_flatten", False, B0, 2, SEED0, push=PUSH)
    f = _fused(dtype, lanes, "tactile_flatten", False, B0, 2, SEED0, push=PUSH)
    same = _same_piece(f["sig"], sig_ref)
    assert int((~same).sum()) <= (0 if dtype == torch.float64 else B0 // 10)
    assert float(ref[:, by_kind["sensor"]].abs().max()) > 0
    _check(f["buf"], ref, same, dtype, "two_frames", lanes=lanes)


# ---------------------------------------------------------------------------------------------------- 5. chunk layouts
@pytest.mark.parametrize("B,kind", [(2000, "ragged"), (4096, "even")])
def test_chunk_layouts_of_the_parameter_passes(B, kind):
    """B = 10 gives one sub-step per chunk; here several per chunk, with a ragged last chunk and with even ones (on a 1024-SIMD device), fp32 at 16
    lanes on the static:pusher kernels: the first 64 environments per (environment, column), and the batch sum"""
    dtype, lanes = torch.float32, 16
    n = T0 * 5
    assert layout_kind(B0, n) == "len1"
    assert layout_kind(B, n) == kind, (B, layout_kind(B, n))
    ref, sig_ref, _, _ = _per_step(dtype, lanes, "tactile_flatten", False, B, T0, SEED0, push=PUSH)
    f = _fused(dtype, lanes, "tactile_flatten", False, B, T0, SEED0, push=PUSH)
    assert f["variant"] == "static:pusher"
    assert float(ref[:64, _columns()[0]["sensor"]].abs().max()) > 0
    same = _same_piece(f["sig"], sig_ref)
    assert int((~same).sum()) <= B // 10, int((~same).sum())
    head = same.clone(); head[64:] = False
    assert int((~same[:64]).sum()) <= 6
    _check(f["buf"], ref, head, dtype, "layout_" + kind, B=B)
    _check(f["buf"][same].double().sum(0, keepdim=True), ref[same].double().sum(0, keepdim=True), None, dtype, "layout_sum_" + kind, B=B)


# ---------------------------------------------------------------------------------------------------- 6. graph capture, 7. run to run
def test_captured_fused_backward_replays_to_eager():
    from tactilesimulation_amd.envs.push_closed_loop import FusedPushEpisode
    dtype, T = torch.float32, 4
    eager = _fused(dtype, 16, "tactile_flatten", False, B0, T, SEED0, push=PUSH)
    q0, goal, dist = (torch.tensor(a, device="cuda", dtype=dtype) for a in _episode(B0, T, SEED0))
    env = _env(dtype, 16, "tactile_flatten", False, B0, T)
    sim = env.sim
    buf = _new_buf(sim)
    sim.set_param_grad_groups(ALL)
    sim.set_param_grad(buf)
    ep = FusedPushEpisode(env, _actor("tactile_flatten", dtype, PUSH), T)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                     # eager warm-up on the side stream the capture runs on
        ep.rollout(q0, goal, dist)
        ep.backward()
        ep.rollout(q0, goal, dist)
        # what the captured launches read besides the episode's own records: the seeds, the goal and the weight snapshots of THIS roll-out — every
        # roll-out makes new ones, so these are held while the graph lives (the same episode: the same values)
        held = (ep.df_dq, ep.df_dvar, ep.du_direct, ep.goal, ep.q0, ep.tac0, ep._w)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):                    # the adjoint launch, both passes, the weight-gradient GEMMs: one linear chain
            ep.backward()
        for _ in range(2):
            ep.rollout(q0, goal, dist)                                # the tape again, and the carried adjoint back at zero
            buf.zero_()
            graph.replay()
            side.synchronize()
            assert torch.equal(buf, eager["buf"])
            for (n, x), (_, p) in zip(eager["grads"], [(n, p) for n, p in ep.actor.named_parameters() if n != "logstd"]):
                assert torch.equal(x, p.grad), n
    torch.cuda.current_stream().wait_stream(side)
    sim.set_param_grad(None)
    torch.cuda.synchronize()
    del held


def test_two_runs_from_scratch_give_the_same_bits():
    a = _fused(torch.float32, 16, "tactile_flatten", True, B0, T0, SEED0, push=PUSH)
    b = _fused(torch.float32, 16, "tactile_flatten", True, B0, T0, SEED0, push=PUSH)
    assert float(a["buf"].abs().max()) > 0 and torch.equal(a["buf"], b["buf"])
