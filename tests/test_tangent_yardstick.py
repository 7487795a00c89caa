"""The yardstick of the tangent pass's tests (tests/test_gpu_tangent.py), checked on the CPU.  No GPU.

tsim_tangent_episode is held to the inner-product identity <w, J v> = <J^T w, v> against the adjoint, and the adjoint to the fp64 oracle's.  That
measures a directional derivative only if the oracle's adjoint IS the derivative of its forward pass, so here the oracle's <J^T w, v> — dL/du,
dL/dq0 and the table gradient dotted with one random direction v in (u, q0, contact columns) — is held against Richardson-extrapolated central
differences of the oracle's own loss along v ((4 D(h/2) - D(h)) / 3 at Newton tol 1e-13), with the tolerance and the branch-signature filter of
tests/test_oracle_param_grad.py: the moved runs must keep the base's signature at every sub-step, and the two numbers agree to 1e-3.
It also confirms that every case of the GPU file converges on the oracle at the frames and sub-steps used there (bad == 0), so that the GPU tests
against the oracle need no exclusions."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
import param_grad_util as PU      # noqa: E402

# the cases of tests/test_gpu_tangent.py: the inputs of param_grad_util's cases, T = 3 frames of 2 sub-steps (pusher: 5)
TANGENT_CASES = ["pusher", "box_slide", "pad_press", "limit_push", "dclaw_position_control", "tactile_insertion", "bdf2:ball_push", "bdf2:tactile_pad",
                 "small:3", "large:L7"]
T_FRAMES = 3


def tangent_case(name, B):
    """model, q0, qd0, u [B, T, nu], sub-steps per frame of a tangent test case"""
    m, q0, qd0, u, _ = PU.body_case(name, B, T_FRAMES)
    return m, q0, qd0, u, 5 if name == "pusher" else 2


def _episode(m, q0, qd0, u, S, w, grad):
    """loss, (dL/du [T, nu], dL/dq0, dL/dqd0, table gradient), signatures, non-converged sub-steps on the oracle"""
    from oracle.oracle import OracleSim
    o = OracleSim(m)
    T, nr = u.shape[0], m.ndof_r
    wq, wv, wt = w
    o.reset(q0, qd0, record=grad)
    L, sigs, bad = 0.0, [], 0
    for t in range(T):
        b, sg = o.forward_sig(u[t], S)
        bad += b
        sigs.append(sg)
        q, _ = o.state()
        var, tac = o.outputs(tactile=bool(m.ndof_tactile))
        L += float(wq[t] @ q) + (float(wv[t] @ var) if m.ndof_var else 0.0) + (float(wt[t] @ tac) if m.ndof_tactile else 0.0)
    adj = None
    if grad:
        g = np.zeros(o._L.orc_table_size(o._h))
        o.set_param_grad(g)
        du = np.zeros((T, m.ndof_u))
        for t in reversed(range(T)):
            dq = np.zeros((S, nr)); dq[-1] = wq[t]
            dv = np.zeros((S, m.ndof_var)); dv[-1] = wv[t]
            dt = np.zeros((S, m.ndof_tactile)); dt[-1] = wt[t]
            du[t] = np.asarray(o.backward_steps(S, dq, dv if m.ndof_var else None, dt if m.ndof_tactile else None)).reshape(S, -1).sum(0)
        o.set_param_grad(None)
        lq, lv = o.adjoint()
        adj = (du, lq, lv, g)
    return L, adj, np.concatenate(sigs, 0), bad


# the (step, seed) of the draw below that each case is compared at: the first that keeps the base's branches
DRAW_USED = {"pusher": (1e-5, 0), "bdf2:ball_push": (1e-4, 2)}


@pytest.mark.parametrize("name", ["pusher", "bdf2:ball_push"])
def test_oracle_adjoint_satisfies_the_identity_against_its_finite_differences(name):
    m, q0, qd0, u, S = tangent_case(name, 1)
    m = copy.deepcopy(m)
    m.F[Bl.TSIM_FH_TOL] = 1e-13
    q0, qd0, u = q0[0], qd0[0], u[0]
    T = u.shape[0]
    w = PU.loss_weights(m, T, 1)
    cols = [c for (_, _, _, c) in m.param_columns()]
    L0, (du, lq, lv, g), sig0, bad0 = _episode(m, q0, qd0, u, S, w, True)
    assert bad0 == 0
    # the signature filter: a seeded draw of directions and steps (1e-4, the step of tests/test_oracle_param_grad.py, then 1e-5, 1e-6: a
    # direction moves every input at once, and the pad's stick / slip switches are close), the first whose four moved runs keep the base's
    # branches at every sub-step is compared
    for h, seed in [(h_, s_) for h_ in (1e-4, 1e-5, 1e-6) for s_ in range(4)]:
        rng = np.random.default_rng(7 + seed)
        vu, vq = 0.1 * rng.normal(size=u.shape), 0.01 * rng.normal(size=q0.shape)
        vp = np.zeros(m.F.size); vp[cols] = rng.normal(size=len(cols)) * np.maximum(np.abs(m.F[cols]), 1.0)
        Ls = []
        for e in (h, -h, h / 2, -h / 2):
            mm = copy.deepcopy(m)
            mm.F[cols] = m.F[cols] + e * vp[cols]
            Lx, _, sx, bx = _episode(mm, q0 + e * vq, qd0, u + e * vu, S, w, False)
            if bx or not np.array_equal(sx, sig0):
                break
            Ls.append(Lx)
        if len(Ls) == 4:
            break
    assert len(Ls) == 4, "no direction of the draw keeps the base's branches: no finite difference across a kink"
    print("yardstick %s: step %g, seed %d" % (name, h, seed))
    assert (h, seed) == DRAW_USED[name], (name, h, seed)      # a drift of the draw that is compared is to be seen, not absorbed
    ad = float((du * vu).sum() + lq @ vq + g[cols] @ vp[cols])
    fd = (4 * (Ls[2] - Ls[3]) / h - (Ls[0] - Ls[1]) / (2 * h)) / 3
    scale = abs((du * vu)).sum() + abs(lq * vq).sum() + abs(g[cols] * vp[cols]).sum()
    assert abs(ad - fd) <= 1e-3 * max(abs(fd), 1e-5 * scale), (name, ad, fd, scale)


@pytest.mark.parametrize("name", TANGENT_CASES)
def test_every_tangent_case_converges_on_the_oracle(name):
    """bad == 0 at T = 3 and the case's sub-steps, on the base model and on the per-environment rows the GPU file uses"""
    B = 5
    m, q0, qd0, u, S = tangent_case(name, B)
    assert u.shape[1] == T_FRAMES and S == (5 if name == "pusher" else 2)
    w = PU.loss_weights(m, T_FRAMES, 0)
    tab = PU.table_rows(m, B, False, 11)
    for e in range(B):
        for mm in (m, PU.row_model(m, tab[e])):
            _, _, _, bad = _episode(mm, q0[e], qd0[e], u[e], S, w, False)
            assert bad == 0, (name, e)
