"""The frame-Jacobian edge cases: models of the random corpus whose taped Newton matrix makes k_frame_jacobian's pivoted solve exchange rows, and
whose sizes end its column passes, its Jvar task loop and its launch plan at their edges.  Used by tests/test_frame_jacobian_cases.py (CPU) and
tests/test_gpu_frame_jacobian_edges.py.  Importable without torch and without a GPU.

A case is a corpus model through param_grad_util.case (tangent_case: T = 3 frames of S = 2 sub-steps; every environment starts alike, the GPU
files run B = 5 on the per-environment rows of param_grad_util.table_rows(m, 5, fp32, 11)), as a BDF1 model (as_bdf1: tsim_frame_jacobians
refuses BDF2).  CASES says what each is there for, and what the CPU file asserts of it rather than assumes: nr, nu, the variables, the frames
in which it pivots; ORDERS the pivot orders of environment 0 on the shared table; SHAPES the launch plan's answer.

The pivot rule (csrc/tsim_eval.h solve_lanes_many, solve_lanes): Gauss-Jordan in double, lanes = rows; at column c every row not yet used
as a pivot offers the bit pattern of (float)|a[c]| with its low four bits replaced by 15 - lane (and bit 4 set), the largest key wins — the
largest magnitude to 16 float ulp, the lowest lane on ties.  pivot_order replays it in numpy on a matrix H and also returns how close the
runner-up came: below 16 ulp a kernel that picks the other row is right too."""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
import param_grad_util as PU      # noqa: E402

B_ENVS, T_FRAMES, SUBSTEPS, ROWS_SEED = 5, 3, 2, 11

# name: (nr, nu, variables, drawn with BDF2 and run as BDF1, the frames in which EVERY environment (both roundings of its rows) takes an
#        off-diagonal pivot on some sub-step, what the case is there for).  ncol = 2 nr + nu; Jvar has variables x nr tasks.
_ALL = (0, 1, 2)
CASES = {
    "small:88":  (2, 0, 0, False, (0,), "NRM 8, one pass, no B, no Jvar"),
    "small:90":  (3, 3, 1, False, (1,), "NRM 8, pivoting switches within an episode"),
    "small:11":  (4, 1, 1, False, _ALL, "NRM 8 at 16 / 32 / 64 lanes, both types"),
    "small:35":  (5, 0, 2, True, (0,), "NRM 8, 3-cycle, nb = 2"),
    "small:51":  (6, 0, 0, False, (0,), "fp64 plan doubles 16 -> 32 beyond the batch"),
    "small:113": (6, 6, 0, False, (0,), "EXPJ with pivoting, nb = 2"),
    "small:52":  (9, 8, 2, False, _ALL, "NRM 16, fp32 plan doubles 16 -> 32; fp64 at 32 lanes fits by 384 B (65 152 B)"),
    "small:111": (9, 6, 3, False, _ALL, "full last pass at NRM 16; NRM 16 at 16 lanes fp32 (60 688 B)"),
    "small:30":  (9, 5, 4, True, _ALL, "nb = 7; 36 Jvar tasks at 16 lanes (three trips)"),
    "small:99":  (11, 5, 3, False, _ALL, "8-cycle; fp64 plan doubles 32 -> 64"),
    "small:100": (12, 8, 1, False, _ALL, "four full passes"),
    "small:12":  (12, 7, 3, True, _ALL, "nb = 7 at NRM 16"),
    "large:L26": (13, 9, 7, False, _ALL, "91 Jvar tasks: second trip at 64 lanes (fp64), three trips at 32 (fp32)"),
    "large:L2":  (16, 6, 4, False, _ALL, "n = NRM = 16 (fp32, 64 lanes); 64 Jvar tasks = LPE exactly; fp64: the refusal"),
    "large:L3":  (16, 12, 5, False, _ALL, "EXPJ, n = 16, 80 Jvar tasks; fp64: the refusal"),
    "large:L1":  (16, 1, 0, True, _ALL, "n = 16 in fp64 (63 072 B); fp32 forced to 16 lanes: n = 16 at two environments per wavefront (64 848 B)"),
    # three more for their sizes alone: none pivots (of the corpus models of the 8-row solve only small:11 pivots in every frame, see
    # tests/test_frame_jacobian_cases.py test_no_other_model_of_the_8_row_solve_pivots_in_every_frame)
    "small:102": (8, 3, 1, False, (), "n = NRM = 8: every row of the 8-row solve in use"),
    "small:6":   (3, 2, 0, False, (), "NRM 8 with ncol = 8: nb = 8 ends the loop after one pass"),
    "small:28":  (7, 1, 0, False, (), "NRM 8 with ncol = 15: nb = 7"),
}
NAMES = list(CASES)
PIVOT_EVERY_FRAME = [n for n in NAMES if CASES[n][4] == _ALL]
# the cases tests/test_gpu_frame_jacobian_edges.py holds to the oracle's rows in fp64, on rows of their own (seed 12, four environments)
ORACLE_CASES = ["small:11", "small:35", "small:52", "small:99", "large:L1"]
ORACLE_ENVS, ORACLE_ROWS_SEED = 4, 12
# left out of the list: the oracle does not converge on one of their sub-steps
NOT_CONVERGED = ["small:49", "small:78", "small:86", "small:103"]

# Environment 0 on the shared table: (the distinct pivot orders seen, which of them each of the T x S = 6 sub-steps takes)
ORDERS = {
    "small:88": ([[1, 0]], [0, 0, 0, 0, 0, 0]),
    "small:90": ([[0, 1, 2], [2, 1, 0]], [0, 1, 1, 1, 0, 0]),
    "small:11": ([[3, 1, 2, 0]], [0, 0, 0, 0, 0, 0]),
    "small:35": ([[3, 1, 0, 2, 4], [0, 1, 2, 3, 4]], [0, 0, 1, 1, 1, 1]),
    "small:51": ([[2, 0, 1, 3, 4, 5], [0, 1, 2, 3, 4, 5]], [0, 1, 1, 1, 1, 1]),
    "small:113": ([[2, 1, 0, 3, 4, 5], [0, 1, 2, 3, 4, 5]], [0, 0, 1, 1, 1, 1]),
    "small:52": ([[5, 3, 4, 1, 2, 0, 6, 7, 8], [4, 3, 5, 1, 2, 0, 6, 7, 8], [5, 4, 3, 1, 2, 0, 6, 7, 8]], [0, 1, 1, 0, 2, 2]),
    "small:111": ([[0, 1, 3, 2, 4, 5, 6, 7, 8]], [0, 0, 0, 0, 0, 0]),
    "small:30": ([[1, 2, 0, 3, 4, 5, 6, 7, 8]], [0, 0, 0, 0, 0, 0]),
    "small:99": ([[4, 5, 3, 7, 1, 2, 6, 0, 8, 9, 10]], [0, 0, 0, 0, 0, 0]),
    "small:100": ([[1, 2, 6, 3, 4, 5, 0, 7, 8, 9, 10, 11], [1, 2, 0, 3, 4, 5, 6, 7, 8, 9, 10, 11]], [0, 1, 1, 1, 1, 1]),
    "small:12": ([[0, 2, 1, 3, 4, 10, 6, 7, 8, 9, 5, 11]], [0, 0, 0, 0, 0, 0]),
    "large:L26": ([[0, 1, 2, 11, 9, 5, 6, 7, 8, 4, 10, 3, 12], [0, 1, 2, 11, 4, 5, 6, 7, 8, 9, 10, 3, 12]], [0, 1, 1, 1, 1, 1]),
    "large:L2": ([[0, 1, 2, 3, 8, 6, 4, 7, 5, 9, 10, 11, 12, 13, 14, 15]], [0, 0, 0, 0, 0, 0]),
    "large:L3": ([[0, 1, 2, 12, 4, 7, 6, 8, 13, 9, 10, 11, 3, 5, 14, 15], [0, 1, 2, 12, 3, 7, 6, 13, 8, 9, 10, 11, 4, 5, 14, 15],
                  [0, 1, 2, 12, 4, 7, 6, 13, 8, 9, 10, 11, 3, 5, 14, 15], [0, 1, 2, 12, 4, 5, 6, 7, 8, 9, 10, 11, 3, 13, 14, 15]], [0, 1, 2, 2, 3, 3]),
    "large:L1": ([[0, 1, 2, 7, 4, 5, 6, 3, 8, 9, 10, 11, 12, 13, 14, 15]], [0, 0, 0, 0, 0, 0]),
    "small:102": ([[0, 1, 2, 3, 4, 5, 6, 7]], [0, 0, 0, 0, 0, 0]),
    "small:6": ([[0, 1, 2]], [0, 0, 0, 0, 0, 0]),
    "small:28": ([[0, 1, 2, 3, 4, 5, 6]], [0, 0, 0, 0, 0, 0]),
}

# k_frame_jacobian's launch for B = 5 with per-environment rows, by (case, bytes of a real): lanes forced (0: the library's choice) ->
# (lanes per environment, LDS bytes, fits) — what wide_models.frame_jacobian_shape computes (the CPU file) and the library reports (the GPU file)
SHAPES = {
    ("small:88", 4): {0: (32, 7776, True), 16: (16, 14608, True), 32: (32, 7776, True), 64: (64, 4352, True)},
    ("small:88", 8): {0: (32, 13696, True), 16: (16, 26080, True), 32: (32, 13696, True), 64: (64, 7488, True)},
    ("small:90", 4): {0: (32, 9680, True), 16: (16, 18336, True), 32: (32, 9680, True), 64: (64, 5360, True)},
    ("small:90", 8): {0: (32, 17376, True), 16: (16, 33344, True), 32: (32, 17376, True), 64: (64, 9408, True)},
    ("small:11", 4): {0: (32, 14288, True), 16: (16, 27344, True), 32: (32, 14288, True), 64: (64, 7760, True)},
    ("small:11", 8): {0: (32, 25792, True), 16: (16, 50112, True), 32: (32, 25792, True), 64: (64, 13632, True)},
    ("small:35", 4): {0: (32, 16368, True), 16: (16, 31344, True), 32: (32, 16368, True), 64: (64, 8880, True)},
    ("small:35", 8): {0: (32, 29952, True), 16: (16, 58048, True), 32: (32, 29952, True), 64: (64, 15904, True)},
    ("small:51", 4): {0: (32, 19600, True), 16: (16, 38144, True), 32: (32, 19600, True), 64: (64, 10336, True)},
    ("small:51", 8): {0: (32, 36096, True), 16: (32, 36096, True), 32: (32, 36096, True), 64: (64, 18624, True)},
    ("small:113", 4): {0: (64, 8944, True), 16: (64, 8944, True), 32: (64, 8944, True), 64: (64, 8944, True)},
    ("small:113", 8): {0: (64, 16192, True), 16: (64, 16192, True), 32: (64, 16192, True), 64: (64, 16192, True)},
    ("small:52", 4): {0: (32, 34720, True), 16: (32, 34720, True), 32: (32, 34720, True), 64: (64, 18608, True)},
    ("small:52", 8): {0: (64, 34272, True), 16: (32, 65152, True), 32: (32, 65152, True), 64: (64, 34272, True)},
    ("small:111", 4): {0: (32, 31136, True), 16: (16, 60688, True), 32: (32, 31136, True), 64: (64, 16352, True)},
    ("small:111", 8): {0: (64, 30080, True), 16: (32, 58400, True), 32: (32, 58400, True), 64: (64, 30080, True)},
    ("small:30", 4): {0: (32, 30768, True), 16: (16, 60096, True), 32: (32, 30768, True), 64: (64, 16112, True)},
    ("small:30", 8): {0: (64, 29728, True), 16: (32, 57792, True), 32: (32, 57792, True), 64: (64, 29728, True)},
    ("small:99", 4): {0: (32, 38432, True), 16: (32, 38432, True), 32: (32, 38432, True), 64: (64, 20592, True)},
    ("small:99", 8): {0: (64, 38368, True), 16: (64, 38368, True), 32: (64, 38368, True), 64: (64, 38368, True)},
    ("small:100", 4): {0: (64, 26848, True), 16: (32, 50576, True), 32: (32, 50576, True), 64: (64, 26848, True)},
    ("small:100", 8): {0: (64, 50112, True), 16: (64, 50112, True), 32: (64, 50112, True), 64: (64, 50112, True)},
    ("small:12", 4): {0: (64, 27008, True), 16: (32, 50656, True), 32: (32, 50656, True), 64: (64, 27008, True)},
    ("small:12", 8): {0: (64, 50528, True), 16: (64, 50528, True), 32: (64, 50528, True), 64: (64, 50528, True)},
    ("large:L26", 4): {0: (64, 29888, True), 16: (32, 55856, True), 32: (32, 55856, True), 64: (64, 29888, True)},
    ("large:L26", 8): {0: (64, 55936, True), 16: (64, 55936, True), 32: (64, 55936, True), 64: (64, 55936, True)},
    ("large:L2", 4): {0: (64, 38208, True), 16: (64, 38208, True), 32: (64, 38208, True), 64: (64, 38208, True)},
    ("large:L2", 8): {0: (64, 72160, False), 16: (64, 72160, False), 32: (64, 72160, False), 64: (64, 72160, False)},
    ("large:L3", 4): {0: (64, 36448, True), 16: (64, 36448, True), 32: (64, 36448, True), 64: (64, 36448, True)},
    ("large:L3", 8): {0: (64, 68864, False), 16: (64, 68864, False), 32: (64, 68864, False), 64: (64, 68864, False)},
    ("large:L1", 4): {0: (64, 33200, True), 16: (32, 64848, True), 32: (32, 64848, True), 64: (64, 33200, True)},
    ("large:L1", 8): {0: (64, 63072, True), 16: (64, 63072, True), 32: (64, 63072, True), 64: (64, 63072, True)},
    ("small:102", 4): {0: (32, 28608, True), 16: (16, 55072, True), 32: (32, 28608, True), 64: (64, 15376, True)},
    ("small:102", 8): {0: (64, 28160, True), 16: (32, 53408, True), 32: (32, 53408, True), 64: (64, 28160, True)},
    ("small:6", 4): {0: (32, 11648, True), 16: (16, 22512, True), 32: (32, 11648, True), 64: (64, 6224, True)},
    ("small:6", 8): {0: (32, 20832, True), 16: (16, 40832, True), 32: (32, 20832, True), 64: (64, 10848, True)},
    # (fp64: the library's own shape leaves the contact points in global memory, staged they would cost the 40 KB block its 32 lanes; forced, they are staged)
    ("small:28", 4): {0: (32, 25008, True), 16: (16, 48256, True), 32: (32, 25008, True), 64: (64, 13392, True)},
    ("small:28", 8): {0: (32, 45472, True), 16: (32, 46368, True), 32: (32, 46368, True), 64: (64, 24320, True)},
}
REFUSED = [("large:L2", 8), ("large:L3", 8)]      # fp64: one environment's context and its column block exceed 64 KB
# the forced shapes the GPU file runs next to the library's own (0), by (case, bytes of a real): the shapes a case's entry above is there for
FORCED = {("small:11", 4): (16, 32, 64), ("small:11", 8): (16, 32, 64), ("small:51", 8): (16,), ("small:52", 4): (16,), ("small:52", 8): (32,), ("large:L1", 4): (16,), ("small:111", 4): (16,),
          ("small:30", 4): (16,), ("small:99", 8): (32,), ("large:L26", 4): (32,), ("large:L2", 4): (16,), ("small:102", 4): (16,), ("small:6", 4): (16,), ("small:28", 4): (16,), ("small:28", 8): (16,)}


def as_bdf1(m, q0, qd0, u, S):
    """the case with the integrator of the same model set to BDF1 — everything else of the model, the start state and the controls are the case's"""
    if int(m.I[Bl.TSIM_IH_INTEGRATOR]) != 1:
        m = copy.deepcopy(m)
        m.I = np.array(m.I, copy=True)
        m.I[Bl.TSIM_IH_INTEGRATOR] = 1
    return m, q0, qd0, u, S


_MODELS = {}


def fj_case(name, B=B_ENVS, T=T_FRAMES):
    """model (BDF1), q0 [B, nr], qd0 [B, nr], u [B, T, nu], sub-steps per frame; the corpus draw of a name is made once"""
    if name not in _MODELS:
        _MODELS[name] = PU.case(name, 1)
    m, q0, qd0, u, S = _MODELS[name]
    assert S == SUBSTEPS
    rep = lambda x: np.tile(x, (B,) + (1,) * (x.ndim - 1))      # noqa: E731
    return as_bdf1(m, rep(q0), rep(qd0), rep(u)[:, :T], S)


def nvariables(m):
    return m.ndof_var // 3


# ---------------------------------------------------------------------------------------------------- the pivot rule
def _bits(x):
    return int(np.abs(np.float32(x)).view(np.uint32))


def pivot_order(H):
    """(rows in the order the kernel's rule takes them as pivots — the identity permutation when the diagonal is always taken —, the smallest
    distance in float ulp between the winning magnitude and the runner-up's over the columns: the rule is unambiguous above 16)"""
    a = np.array(H, dtype=np.float64)
    n = a.shape[0]
    done, order, gap = np.zeros(n, bool), [], 1 << 31
    for col in range(n):
        cand = [r for r in range(n) if not done[r]]
        key = {r: (_bits(a[r, col]) & ~0xF) | (15 - r) | 0x10 for r in cand}
        p = max(cand, key=lambda r: key[r])
        assert p == 15 - (key[p] & 0xF)
        if len(cand) > 1:
            gap = min(gap, _bits(a[p, col]) - max(_bits(a[r, col]) for r in cand if r != p))
        f = a[:, col] / a[p, col]
        f[p] = 0.0
        a -= np.outer(f, a[p])
        done[p] = True
        order.append(p)
    return order, gap


def newton_matrices(m, q0, qd0, u, S):
    """One environment on the oracle, sub-step by sub-step (u [T, nu]): (non-converged sub-steps, [H of every sub-step's converged point]) —
    H = dg/dq1 of the oracle's residual at (q1; q0, qd0, u), the matrix the kernels tape"""
    from oracle.oracle import OracleSim
    o = OracleSim(m)
    o.reset(q0, qd0)
    bad, Hs = 0, []
    for t in range(u.shape[0]):
        for _ in range(S):
            qa, qda = o.state()
            bad += o.forward(u[t], 1)
            q1, _ = o.state()
            Hs.append(o.residual(q1, qa, qda, u[t], which=0)[1])
    return bad, Hs


def env_models(m, fp32, B=B_ENVS, seed=ROWS_SEED):
    """the models of the B environments on the rows the GPU files set"""
    tab = PU.table_rows(m, B, fp32, seed).astype(np.float64)
    return [PU.row_model(m, tab[e]) for e in range(B)]
