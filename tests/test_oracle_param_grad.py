"""The fp64 CPU oracle's parameter adjoint (oracle/tsim_oracle.cpp orc_set_param_grad, OracleSim.set_param_grad) against central differences
of the oracle's own forward pass.  No GPU.

The oracle is the reference the kernels' table gradient (tsim_set_param_grad, tests/test_gpu_param_grad_oracle.py) is held to, so here it is
pinned to something that shares none of its derivative code: the episode loss of the oracle's forward pass at p +- h and p +- h / 2 per
parameter column, Richardson-extrapolated ((4 D(h/2) - D(h)) / 3), at Newton tol 1e-13.  A column is compared only where the branch signatures
(forward_sig) of all four moved runs equal the base's at every sub-step: the stick / slip switch and a cuboid's face switch are kinks.  Each
column is held relative to its own finite-difference value, with a floor of a small fraction of the largest entry of the gradient (the
finite-difference noise is far below it).  Entries outside model.param_columns() stay exactly 0."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
from param_grad_util import CONTACT_KINDS as KINDS, case, kind_of, loss_weights, oracle_episode      # noqa: E402

FD_FIXED = ["pusher", "tactile_insertion", "stable_grasp", "dclaw_position_control", "tactile_pad", "box_slide", "pad_press", "sphere_rest",
            "slider_push", "ball_push"]
BDF2 = ["bdf2:tactile_pad", "bdf2:ball_push"]
RANDOM = ["small:%d" % k for k in (1, 3, 5, 8, 11, 14, 17, 21, 26, 31, 37, 44)] + ["large:L26", "large:L7", "large:L16", "large:L3", "large:L10",
                                                                                   "large:L45", "large:L0", "large:L2"]
FLOOR = 1e-5        # of the row's largest entry: the finite differences' own noise is about 2e-8 of it (measured: profiles/r10_param_grad_oracle.md)


def fd_compare(m, q0, qd0, u, S, hrel=1e-4, floor=FLOOR, seed=1, max_cols=10):
    """Per compared column: |g_c - fd_c| / max(|fd_c|, floor max_c |g_c|), for the columns whose moved runs keep the base's branch signature at
    every sub-step.  Compared (a seeded draw): one column of every kind, whatever its own gradient, of a pair or sensor that is in contact (some
    other column of its four above the floor) or of any dof; then columns above the floor up to max_cols; then two below it.  Returns (errors,
    kinds, gradient, number of compared columns, row scale, finite differences)."""
    m = copy.deepcopy(m)
    m.F[Bl.TSIM_FH_TOL] = 1e-13
    T = u.shape[0]
    w = loss_weights(m, T, seed)
    pcols = m.param_columns()
    L0, g, sig0, bad0, _ = oracle_episode(m, q0, u, S, w, qd0=qd0)
    assert bad0 == 0
    other = np.setdiff1d(np.arange(g.size), [c for (_, _, _, c) in pcols])
    assert np.all(g[other] == 0)
    scale = np.abs(g[[c for (_, _, _, c) in pcols]]).max()
    rng = np.random.default_rng(seed)
    big = [pc for pc in pcols if abs(g[pc[3]]) >= floor * scale]
    small = [pc for pc in pcols if abs(g[pc[3]]) < floor * scale]
    active = {}                                                           # pair / sensor: the largest |g| over its four columns
    for pc in pcols:
        active[(pc[0], pc[1])] = max(active.get((pc[0], pc[1]), 0.0), abs(g[pc[3]]))
    pick = []
    for k in KINDS:                                                       # one of every kind first (not chosen by its own |g|), then a draw
        ks = [pc for pc in pcols if kind_of(pc) == k and (pc[0] == "dof" or active[(pc[0], pc[1])] >= floor * scale)]
        if ks:
            pick.append(ks[int(rng.integers(len(ks)))])
    rest = [pc for pc in big if pc not in pick]
    small = [pc for pc in small if pc not in pick]
    pick += [rest[i] for i in rng.permutation(len(rest))[:max(0, max_cols - len(pick))]]
    pick += [small[i] for i in rng.permutation(len(small))[:2]]
    errs, kinds, fds = [], [], []
    for pc in pick:
        c = pc[3]
        p = float(m.F[c])
        h = hrel * max(abs(p), 1.0)
        Ls = []
        for dp in (h, -h, h / 2, -h / 2):
            mm = copy.deepcopy(m)
            mm.F[c] = p + dp
            Lx, _, sx, bx, _ = oracle_episode(mm, q0, u, S, w, grad=False, qd0=qd0)
            if bx or not np.array_equal(sx, sig0):
                break
            Ls.append(Lx)
        if len(Ls) < 4:
            continue
        d1 = (Ls[0] - Ls[1]) / (2 * h)
        d2 = (Ls[2] - Ls[3]) / h
        fd = (4 * d2 - d1) / 3
        errs.append(abs(g[c] - fd) / max(abs(fd), floor * scale))
        kinds.append(kind_of(pc))
        fds.append(fd)
    return np.array(errs), kinds, g, len(pick), scale, np.array(fds)


# (name, frames): short episodes keep the column loop of every model within a few seconds
CASES = [(n, 3 if n in ("tactile_pad", "dclaw_position_control", "tactile_insertion") else 4) for n in FD_FIXED] + [(n, 3) for n in BDF2] + \
    [(n, 4) for n in RANDOM]


@pytest.mark.parametrize("name,T", CASES)
def test_oracle_parameter_adjoint_equals_its_finite_differences(name, T):
    m, q0, qd0, u, S = case(name, 1, T)
    errs, kinds, g, ncol, scale, fds = fd_compare(m, q0[0], qd0[0], u[0], S)
    assert ncol == 0 or errs.size >= 0.5 * ncol, (name, errs.size, ncol)
    if errs.size:
        assert errs.max() <= 1e-3, (name, sorted(zip(errs, kinds))[-5:])


def test_oracle_parameter_adjoint_sees_every_column_kind():
    """Across the fixed models, every kind of parameter column has a compared entry above the floor; the pusher's pad is dragged so that mu
    and the sensors' damping move the loss"""
    seen = {}
    for name in ("pusher", "tactile_pad"):
        m, q0, qd0, u, S = case(name, 1, 3)
        errs, kinds, g, ncol, scale, fds = fd_compare(m, q0[0], qd0[0], u[0], S)
        for e, k, fd in zip(errs, kinds, fds):
            if abs(fd) >= 1e-6 * scale:
                seen[k] = seen.get(k, 0) + 1
    assert all(seen.get(k, 0) >= 1 for k in KINDS), seen


def test_gradient_off_and_on_leave_the_adjoint_unchanged():
    """Setting the buffer changes nothing else the oracle returns: dL/du and the carried adjoint bit for bit"""
    from oracle.oracle import OracleSim
    m, q0, _, u, S = case("pusher", 1, 3)
    T = u.shape[1]
    w = loss_weights(m, T)
    res = []
    for on in (False, True):
        o = OracleSim(m)
        o.reset(q0[0], record=True)
        for t in range(T):
            o.forward(u[0, t], S)
        if on:
            buf = np.full(o._L.orc_table_size(o._h), np.nan)
            buf[[c for (_, _, _, c) in m.param_columns()]] = 0.0
            o.set_param_grad(buf)
        du = []
        for t in reversed(range(T)):
            dq = np.zeros((S, m.ndof_r)); dq[-1] = w[0][t]
            dt = np.zeros((S, m.ndof_tactile)); dt[-1] = w[2][t]
            du.append(o.backward_steps(S, dq, None, dt))
        res.append((np.array(du), o.adjoint()))
        if on:
            other = np.setdiff1d(np.arange(buf.size), [c for (_, _, _, c) in m.param_columns()])
            assert np.isnan(buf[other]).all() and np.isfinite(np.delete(buf, other)).all()
    assert np.array_equal(res[0][0], res[1][0]) and all(np.array_equal(a, b) for a, b in zip(res[0][1], res[1][1]))
