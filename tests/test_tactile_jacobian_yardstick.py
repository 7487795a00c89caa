"""The yardstick of the tactile Jacobians' oracle test (tests/test_gpu_tactile_jacobians.py), checked on the CPU.  No GPU.

tsim_tactile_jacobians' C_f, multiplied by tsim_frame_jacobians' [A_f | B_f], is held to rows built from the fp64 oracle's adjoint
(tactile_jacobian_cases.oracle_tactile_rows): the oracle is reset at (q_f, qd_f), runs the frame, and one adjoint pass per loaded tactile component
with a unit df_dtac seed on the last sub-step gives that row of d tac_{f+1} / d (q_f, qd_f, u_f) = [C A | C B].  That builder is the derivative of
the oracle's one-frame tactile map only if it agrees with finite differences of that map, so here rows @ v is held against Richardson-extrapolated
central differences ((4 D(h/2) - D(h)) / 3 at Newton tol 1e-13) along one random direction v in (q_f, qd_f, u_f), with the step ladder, the tolerance
(1e-3) and the branch-signature filter of tests/test_frame_jacobian_yardstick.py, extended by the end state's taxel_list items (taxel, pair, branch)
being equal: no difference is taken across a taxel that loads, unloads or switches between stick and slip.  The (step, seed) each case is compared
at is pinned.  On the pad models the taxels pad_models.borderline flags at the frame's end are left out, at most pad_models.BORDER_CAP = 1 % of them
(tactile_jacobian_cases.pad_keep asserts it): the states are pad_models.states' for which the oracle alone stays within that.
The second test pins the draw of the GPU file's direct check: C v against differences of the read-out map tac(q, qd) itself."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
import pad_models as P      # noqa: E402
import tactile_jacobian_cases as TC      # noqa: E402
from test_tangent_yardstick import T_FRAMES, tangent_case      # noqa: E402
from test_frame_jacobian_yardstick import oracle_frame_states      # noqa: E402

PAD_CASES = {"pad_4x2": "small_130_4x2", "pad_1x8": "small_130_1x8"}      # (4 sensors, 2 primitives each), (1 sensor, 8 primitives)
LADDER = [(h_, s_) for h_ in (1e-4, 1e-5, 1e-6) for s_ in range(4)]


@pytest.fixture(scope="module")
def pad_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("tj_pads")


def yardstick_case(name, pad_dir):
    """model (Newton tol 1e-13), the frame's start (q, qd), its control, the sub-steps of the case"""
    if name in PAD_CASES:
        m = copy.deepcopy(P.table_model(PAD_CASES[name], pad_dir))
        m.F[Bl.TSIM_FH_TOL] = 1e-13
        q, qd = P.table_states(PAD_CASES[name], m)[0]
        return m, q, qd, TC.PAD_U, 1
    m, q0, qd0, u, S_case = tangent_case(name, 1)
    m = copy.deepcopy(m)
    m.F[Bl.TSIM_FH_TOL] = 1e-13
    f = T_FRAMES - 1                                   # the last frame of the case: the pad is on the box
    q, qd = oracle_frame_states(m, q0[0], qd0[0], u[0, :f], S_case)[f]
    return m, q, qd, u[0, f], S_case


def draw(nr, nu, seed):
    rng = np.random.default_rng(7 + seed)
    return 0.01 * rng.normal(size=nr), 0.01 * rng.normal(size=nr), 0.1 * rng.normal(size=nu)


# the (step, seed) of the ladder that each (case, S) is compared at: the first that keeps the base's branches and taxel items
DRAW_USED = {("pusher", 1): (1e-4, 0), ("pusher", 2): (1e-4, 0), ("pad_4x2", 1): (1e-4, 0), ("pad_1x8", 1): (1e-4, 0)}


@pytest.mark.parametrize("name,S", list(DRAW_USED))
def test_oracle_tactile_rows_are_the_derivative_of_its_one_frame_tactile_map(name, S, pad_dir):
    m, q, qd, uf, _ = yardstick_case(name, pad_dir)
    nr, nu = m.ndof_r, m.ndof_u
    rows, ld = TC.oracle_tactile_rows(m, q, qd, uf, S)
    tac0, sig0, items0, bad0, (q1, qd1) = TC.frame_tactile(m, q, qd, uf, S)
    assert bad0 == 0 and ld.any() and not ld.all()
    keep = TC.pad_keep(m, q1, qd1)[1] if name in PAD_CASES else np.ones_like(ld)
    x0 = np.concatenate([q, qd, uf])

    def fmap(x):
        tac, sig, items, bad, _ = TC.frame_tactile(m, x[:nr], x[nr:2 * nr], x[2 * nr:], S)
        return tac, (bad, sig.tobytes(), tuple(items))
    for h, seed in LADDER:
        v = np.concatenate(draw(nr, nu, seed))
        fd = TC.richardson(fmap, x0, v, h)
        if fd is not None:
            break
    assert fd is not None, "no direction of the ladder keeps the base's branches: no finite difference across a kink"
    print("tactile yardstick %s S = %d: step %g, seed %d, %d of %d taxels loaded, %d left out" % (name, S, h, seed, ld.sum(), ld.size, (~keep).sum()))
    assert (h, seed) == DRAW_USED[name, S], (name, S, h, seed)      # a drift of the draw that is compared is to be seen, not absorbed
    ad = rows @ v
    scale = np.abs(rows) @ np.abs(v)
    k3 = np.repeat(keep, 3)
    assert np.all(ad[np.repeat(~ld, 3)] == 0) and np.all(fd[np.repeat(~ld, 3)] == 0)
    assert np.any(ad[k3] != 0)
    worst = float(np.max((np.abs(ad - fd) / np.maximum(np.abs(fd), np.maximum(1e-5 * scale, 1e-300)))[k3]))
    print("tactile yardstick %s S = %d: worst |rows v - fd| / max(|fd|, 1e-5 scale) = %.3e" % (name, S, worst))
    assert np.all((np.abs(ad - fd) <= 1e-3 * np.maximum(np.abs(fd), 1e-5 * scale))[k3]), (name, S)


# the draw of the GPU file's direct check (C v against differences of tac(q, qd) at the frame's END state, v in (q, qd)): pinned likewise
READOUT_DRAW_USED = {"pusher": (1e-4, 0), "pad_4x2": (1e-4, 0), "pad_1x8": (1e-4, 0)}


def readout_difference(m, q1, qd1, name):
    """(fd [ndof_tactile], v [2 nr], (step, seed)) of the read-out map at (q1, qd1): the first draw of the ladder that keeps the taxel items"""
    nr = m.ndof_r
    fmap = lambda x: (lambda r: (r[0], tuple(r[1])))(TC.readout(m, x[:nr], x[nr:]))      # noqa: E731
    for h, seed in LADDER:
        vq, vqd, _ = draw(nr, m.ndof_u, seed)
        v = np.concatenate([vq, vqd])
        fd = TC.richardson(fmap, np.concatenate([q1, qd1]), v, h)
        if fd is not None:
            return fd, v, (h, seed)
    raise AssertionError("no direction of the ladder keeps the taxel items of %s" % name)


@pytest.mark.parametrize("name", list(READOUT_DRAW_USED))
def test_the_direct_check_draw_is_pinned(name, pad_dir):
    m, q, qd, uf, S = yardstick_case(name, pad_dir)
    _, _, _, bad, (q1, qd1) = TC.frame_tactile(m, q, qd, uf, S)
    assert bad == 0
    fd, v, used = readout_difference(m, q1, qd1, name)
    assert used == READOUT_DRAW_USED[name], (name, used)
    assert np.any(fd != 0)
