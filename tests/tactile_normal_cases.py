"""What the tactile normal equations' tests share (tests/test_tactile_normal_cases.py on the CPU, tests/test_gpu_tactile_normal_equations.py on the
GPU): the launch plan of k_tactile_normal restated, the scatter of the compact Ft to the dense F, and the reference products with their scales.

The reference uses only what the tactile and parameter Jacobians give (both pinned to the oracle by their own tests): H = [C | F] in float64 and
    N = sum_i w_i h_id h_ie ,   S_N = sum_i w_i |h_id| |h_ie| ,   n = sum_i w_i h_id r_i ,   S_n = sum_i w_i |h_id| |r_i|
An entry's error is |got - reference| / S; where S is 0 the entry must be exactly 0.

Importable without torch and without a GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
import wide_models as W      # noqa: E402

MIN_ROWS = 4      # csrc/tsim_tactile_normal.h TS_TN_MIN_ROWS


# ---------------------------------------------------------------------------------------------------- the launch plan, restated
def tn_zc(nr, with_params, with_resid):
    """csrc/tsim_tactile_normal.h ts_tn_zc: the columns the symmetric product runs over"""
    return 2 * nr + (4 if with_params else 0) + (1 if with_resid else 0)


def tn_stride(nr, with_params):
    """ts_tn_stride: a tile row — the product's columns with a residual, the weight — rounded up to an odd number of reals"""
    return (tn_zc(nr, with_params, True) + 1) | 1


def tn_entries(zc):
    return zc * (zc + 1) // 2


def tn_entry_index(zc, d, e):
    """entry (d <= e) of the symmetric zc x zc block in the running sums"""
    assert d <= e < zc
    return d * zc - d * (d - 1) // 2 + e - d


def tn_slot_reals(nr, with_params, rows):
    """ts_tn_slot_reals: the pair's records, the running sums and the tile of `rows` taxels of a slot, each rounded up to four reals"""
    r4 = lambda x: (x + 3) & ~3      # noqa: E731
    return r4(18 * nr) + r4(tn_entries(tn_zc(nr, with_params, True))) + r4(3 * rows * tn_stride(nr, with_params))


def tn_table_bytes(nr, with_params):
    return (tn_entries(tn_zc(nr, with_params, True)) * 4 + 15) // 16 * 16


def tactile_normal_shape(m, lanes, esz, with_params, env_tables=True, B=5, n_simd=1024, fused=False):
    """(lanes per environment, LDS bytes, fits, taxels per trip) of k_tactile_normal for a batch of B environments forced to `lanes` (0: the
    library's choice) — csrc/tsim_hip.hip tactile_normal_plan: the batch's shape, then the lanes double while the contexts, the slots' blocks
    (rounded up to 16 bytes together) and the entry table are over 64 KB; at 64 lanes the taxels per trip halve instead, down to MIN_ROWS.
    fits: the launch is not refused"""
    st = False
    if 3 * int(m.I[Bl.TSIM_IH_NCPT]) * esz <= W.CPT_LDS_BYTES:      # decide_stage_cpt
        st = W._launch_lanes(m, lanes, esz, env_tables, False, B, n_simd, fused) == W._launch_lanes(m, lanes, esz, env_tables, True, B, n_simd, fused) \
            and W.block_bytes(m, 1, esz, env_tables, True) <= W.LDS_CAP
    lanes = W._launch_lanes(m, lanes, esz, env_tables, st, B, n_simd, fused)
    nr = m.ndof_r

    def nbytes(lpe, rows):
        ns = 64 // lpe
        return W.block_bytes(m, ns, esz, env_tables, st) + (ns * tn_slot_reals(nr, with_params, rows) * esz + 15) // 16 * 16 + tn_table_bytes(nr, with_params)
    while lanes < 64 and nbytes(lanes, lanes) > W.LDS_CAP:
        lanes *= 2
    rows = lanes
    while rows > MIN_ROWS and nbytes(lanes, rows) > W.LDS_CAP:
        rows //= 2
    n = nbytes(lanes, rows)
    return lanes, n, n <= W.LDS_CAP, rows


# ---------------------------------------------------------------------------------------------------- the reference
def sensor_ranges(m):
    """[(first taxel, taxels, paired primitives)] per sensor"""
    I = m.I
    out = []
    for s in range(int(I[Bl.TSIM_IH_NSENSOR])):
        si = int(I[Bl.TSIM_IH_OFF_SENSOR]) + s * Bl.TSIM_SI_SIZE
        out.append((int(I[si + Bl.TSIM_SI_TAX0]), int(I[si + Bl.TSIM_SI_NTAX]), int(I[si + Bl.TSIM_SI_NSPRIM])))
    return out


def dense_F(Ft, sensors):
    """[..., 4, ntac] compact Ft -> [..., ntac, 4 nsensor] dense F: column 4 s + k is row k of Ft on sensor s's taxels, zero elsewhere.  numpy
    arrays or torch tensors"""
    ntac = Ft.shape[-1]
    shape = tuple(Ft.shape[:-2]) + (ntac, 4 * len(sensors))
    F = np.zeros(shape, Ft.dtype) if isinstance(Ft, np.ndarray) else Ft.new_zeros(shape)
    for s, (t0, nt, _) in enumerate(sensors):
        for k in range(4):
            F[..., 3 * t0:3 * (t0 + nt), 4 * s + k] = Ft[..., k, 3 * t0:3 * (t0 + nt)]
    return F


def reference(H, w, r=None):
    """H [..., ntac, Z], w [ntac], r [..., ntac] (float64; numpy arrays or torch tensors) -> (N, S_N, n, S_n); n and S_n are None without r"""
    xp = np if isinstance(H, np.ndarray) else __import__("torch")
    A = abs(H)
    N = xp.einsum("...id,i,...ie->...de", H, w, H)
    SN = xp.einsum("...id,i,...ie->...de", A, abs(w), A)
    if r is None:
        return N, SN, None, None
    return N, SN, xp.einsum("...id,i,...i->...d", H, w, r), xp.einsum("...id,i,...i->...d", A, abs(w), abs(r))
