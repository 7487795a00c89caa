"""The compact many-dof models (tests/models/wide9.xml, wide10.xml: more than 8 dofs on few links, so that two or four environments share a
wavefront at the 16-row register solve), their cases, and the arithmetic of a block's LDS that decides the launch shape.  Used by
tests/test_wide_models.py (CPU) and tests/test_gpu_wide_models.py.  Importable without torch and without a GPU.

A case, in the style of param_grad_util.body_case: q0, qd0 [B, nr], u [B, T, nu] with T = 3 frames of S = 2 sub-steps; the GPU file runs B = 5
(ragged at 4 and at 2 environments per wavefront) on the per-environment rows of param_grad_util.table_rows.  In every environment the sled
slides on the ground (a ground pair with general contact points, loaded and slipping), the pad is pressed on the sled's top face (general-primitive
pair, taxels loaded), the finger sits beyond a limit (wide9: the upper, wide10: the lower one), and force and position motors drive the chain.

The LDS arithmetic restates csrc/tsim_device.h (ts_lds_env_reals, ts_tab_reals, ts_lds_reals), csrc/tsim_tangent.h (ts_tan_slot_reals) and the size
of the host's sweep schedule (csrc/tsim_hip.hip build_sched); the GPU file holds block_bytes() to what the library reports.  frame_jacobian_shape
restates the launch plan of k_frame_jacobian (csrc/tsim_frame_jacobian.h ts_fj_slot_reals, csrc/tsim_hip.hip ts_plan / frame_jacobian_plan /
launch_shape) for any model; tests/test_gpu_frame_jacobians.py and tests/test_gpu_frame_jacobian_edges.py hold it to the library."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tactilesimulation_amd.model.blob as Bl      # noqa: E402
from tactilesimulation_amd.model.compiler import load_model      # noqa: E402

WIDE = ["wide9", "wide10"]
T_FRAMES, SUBSTEPS, B_ENVS = 3, 2, 5
LDS_CAP = 64 * 1024
# csrc/tsim_device.h: contact pairs staged at a time; reals of a link's value record, of a (link, direction) tangent record, of a staged pair's value
# part and of its per-direction part; the threshold below which the contact points are staged in LDS
PAIR_GROUP, LK_SIZE, DT_SIZE, PP_SIZE, PT_SIZE, CPT_LDS_BYTES = 4, 45, 18, 36, 18, 8192
SCHED_ENT, LR_SIZE = 37, 8          # csrc/tsim_device.h TS_SCHED_ENT, TS_LR_SIZE
TAN_MAX_DIR = 8                     # include/tsim.h TSIM_TANGENT_MAX_DIR
MAX_DOF_PER_LINK = 3                # the joint grammar (model/blob.py JOINT_NDOF): a link carries at most a translational joint's three dofs


# ---------------------------------------------------------------------------------------------------- LDS arithmetic
def lds_env_reals(nl, nr, nu, esz):
    """csrc/tsim_device.h ts_lds_env_reals: LDS reals of one environment's context"""
    n = (4 * nr + (nl + 1) * 12 + PAIR_GROUP * 12) * (8 // esz)      # the double block
    n += 15 * nr + nu
    n += 2 * nr * nr
    n += 4 * nr
    n += (nl + 1) * LK_SIZE
    n += nr * 6
    n += (nl + 1) * nr * DT_SIZE
    n += PAIR_GROUP * PP_SIZE
    n += PAIR_GROUP * nr * PT_SIZE
    n += 16 + 54
    return (n + 8 + 3) & ~3


def min_links(nr):
    """the fewest links that carry nr dofs"""
    return -(-nr // MAX_DOF_PER_LINK)


def env_bytes_lower_bound(nr, esz):
    """bytes of the smallest context a model of nr dofs can have: the fewest links, no motor (the context grows with nl and with nu)"""
    return lds_env_reals(min_links(nr), nr, 0, esz) * esz


def sched_ints(m):
    """number of ints of the host's sweep schedule (csrc/tsim_hip.hip build_sched)"""
    I = m.I
    nl, npair, nu, ns = (int(I[k]) for k in (Bl.TSIM_IH_NL, Bl.TSIM_IH_NPAIR, Bl.TSIM_IH_NU, Bl.TSIM_IH_NSENSOR))
    ol = int(I[Bl.TSIM_IH_OFF_LINK])
    parent = [0] + [int(I[ol + i * Bl.TSIM_LI_SIZE + Bl.TSIM_LI_PARENT]) for i in range(nl)]
    branch, sizes = [None] * (nl + 1), []
    for i in range(1, nl + 1):
        if parent[i] == 0:
            branch[i] = len(sizes)
            sizes.append(0)
        else:
            branch[i] = branch[parent[i]]
        sizes[branch[i]] += 1
    nsteps = max(sizes) if sizes else 0
    os_ = int(I[Bl.TSIM_IH_OFF_SENSOR])
    nsprim = sum(int(I[os_ + s * Bl.TSIM_SI_SIZE + Bl.TSIM_SI_NSPRIM]) for s in range(ns))
    return SCHED_ENT + nsteps * 16 + nl * LR_SIZE + npair * Bl.TSIM_PI_SIZE + 16 + nu * Bl.TSIM_MI_SIZE + 3 * ns + 2 * nsprim + 4 * npair


def pg_count(m):
    """csrc/tsim_param_grad.h ts_pg_count: entries of a direction's compact parameter vector"""
    I = m.I
    return 4 * int(I[Bl.TSIM_IH_NPAIR]) + 4 * int(I[Bl.TSIM_IH_NSENSOR]) + m.ndof_r


def block_bytes(m, nslot, esz, env_tables=True, stage_cpt=True):
    """csrc/tsim_hip.hip lds_bytes_for: dynamic LDS of a forward / adjoint block of nslot environments"""
    I = m.I
    nl, nr, nu, ncpt, nfrec = int(I[Bl.TSIM_IH_NL]), m.ndof_r, m.ndof_u, int(I[Bl.TSIM_IH_NCPT]), int(I[Bl.TSIM_IH_FOFF_CPT])
    tab = ((nslot if env_tables else 1) * (nfrec + 2) + (3 * ncpt if stage_cpt else 0) + 3) & ~3
    nsched = sched_ints(m) + len(I)
    reals = tab + ((nsched * 4 + esz - 1) // esz + 3) // 4 * 4 + nslot * lds_env_reals(nl, nr, nu, esz) + 8
    return (reals * esz + 15) // 16 * 16


def tangent_slot_bytes(m, esz, ndir=TAN_MAX_DIR, with_dtables=True, nhist=4):
    """csrc/tsim_tangent.h ts_tan_slot_reals: a slot's tangent block behind the contexts.  nhist: the states a direction keeps, 2, or 4 for a BDF2
    model; the launch plan sizes the SHAPE for 4 whatever the model's integrator (csrc/tsim_hip.hip ts_plan), a launch allocates its own"""
    per_dir = nhist * m.ndof_r + (pg_count(m) if with_dtables else 0) + max(m.ndof_r, 12) + m.ndof_u
    return ((ndir * per_dir + 3) & ~3) * esz


def tangent_block_bytes_of_counts(nr, nl, nu, nvar, npair, nsensor, nsprim, nsteps, esz, nslot, ncpt_staged=0):
    """LDS bytes of a k_tangent block of nslot environments with per-environment rows, as the plan sizes its shape (eight directions, dtables, four
    history states), from the model's counts alone: the table and the int blob follow from them (include/tsim_blob.h: a header, then a record per
    link, dof, motor, variable, pair and sensor), and so does the schedule (sched_ints).  nsprim: (sensor, primitive) pairs; nsteps: links of the
    longest root branch; ncpt_staged: contact points staged in LDS.  Non-decreasing in every count, so the smallest counts a set of models can
    have bound their blocks from below"""
    nfrec = Bl.TSIM_FH_SIZE + nl * Bl.TSIM_LF_SIZE + nr * Bl.TSIM_DF_SIZE + nu * Bl.TSIM_MF_SIZE + nvar * Bl.TSIM_VF_SIZE + npair * Bl.TSIM_PF_SIZE + nsensor * Bl.TSIM_SF_SIZE
    nints = Bl.TSIM_IH_SIZE + nl * Bl.TSIM_LI_SIZE + nr * Bl.TSIM_DI_SIZE + nu * Bl.TSIM_MI_SIZE + nvar * Bl.TSIM_VI_SIZE + npair * Bl.TSIM_PI_SIZE + nsensor * Bl.TSIM_SI_SIZE + nsprim
    sched = SCHED_ENT + nsteps * 16 + nl * LR_SIZE + npair * Bl.TSIM_PI_SIZE + 16 + nu * Bl.TSIM_MI_SIZE + 3 * nsensor + 2 * nsprim + 4 * npair
    tab = (nslot * (nfrec + 2) + 3 * ncpt_staged + 3) & ~3
    reals = tab + (((sched + nints) * 4 + esz - 1) // esz + 3) // 4 * 4 + nslot * lds_env_reals(nl, nr, nu, esz) + 8
    per_dir = 4 * nr + (4 * npair + 4 * nsensor + nr) + max(nr, 12) + nu
    return (reals * esz + 15) // 16 * 16 + nslot * ((TAN_MAX_DIR * per_dir + 3) & ~3) * esz


def stages_cpt(m, lanes, esz, env_tables=True):
    """csrc/tsim_hip.hip decide_stage_cpt for a batch forced to `lanes`: the contact points are staged when they are small and cost the launch
    neither its shape nor the 64 KB of a one-environment block"""
    if 3 * int(m.I[Bl.TSIM_IH_NCPT]) * esz > CPT_LDS_BYTES:
        return False
    shape = lambda st: next(l for l in (16, 32, 64) if l >= lanes and (l == 64 or block_bytes(m, 64 // l, esz, env_tables, st) <= LDS_CAP))      # noqa: E731
    return shape(True) == shape(False) and block_bytes(m, 1, esz, env_tables, True) <= LDS_CAP


def forced_shape(m, lanes, esz, env_tables=True):
    """(lanes per environment, LDS bytes) of the forward / adjoint launches of a batch forced to `lanes` (csrc/tsim_hip.hip launch_shape; no
    rotation-vector joint): the lanes double until the block fits 64 KB"""
    st = stages_cpt(m, lanes, esz, env_tables)
    while lanes < 64 and block_bytes(m, 64 // lanes, esz, env_tables, st) > LDS_CAP:
        lanes *= 2
    return lanes, block_bytes(m, 64 // lanes, esz, env_tables, st)


def tangent_shape(m, lanes, esz, env_tables=True):
    """lanes per environment of k_tangent for a batch forced to `lanes` (csrc/tsim_hip.hip ts_plan): chosen for eight directions with dtables"""
    st = stages_cpt(m, lanes, esz, env_tables)
    lanes = forced_shape(m, lanes, esz, env_tables)[0]
    while lanes < 64 and block_bytes(m, 64 // lanes, esz, env_tables, st) + (64 // lanes) * tangent_slot_bytes(m, esz) > LDS_CAP:
        lanes *= 2
    return lanes


FJ_RHS = 8                          # csrc/tsim_frame_jacobian.h TS_FJ_RHS
AUTO_LDS_CAP = 40 * 1024            # csrc/tsim_hip.hip launch_shape: the cap of a block where no shape is forced (room for four blocks per CU)


def fj_slot_reals(nr, nu):
    """csrc/tsim_frame_jacobian.h ts_fj_slot_reals: X [2 nr + nu][2 nr], MM [nr][nr], W [8][nr], DU [nu] of a slot, rounded up to four reals"""
    return ((2 * nr + nu) * 2 * nr + nr * nr + FJ_RHS * nr + nu + 3) & ~3


def _launch_lanes(m, lanes, esz, env_tables, st, B, n_simd, fused):
    """csrc/tsim_hip.hip launch_shape for a batch of B environments: `lanes` forced, or (0) the shape of the fewest rounds x latency whose block
    stays under 40 KB; 64 with a rotation-vector joint; then the lanes double until the block fits the cap"""
    import random_corpus as RC
    cap = LDS_CAP if lanes else AUTO_LDS_CAP
    if not lanes:
        lanes, best = 64, 1e30
        lat = (1.0, 1.13, 1.24) if fused else (1.0, 0.93, 1.02)
        for i, cand in enumerate((64, 32, 16)):
            ns = 64 // cand
            if i > 0 and block_bytes(m, ns, esz, env_tables, st) > cap:
                break
            t = -(-(-(-B // ns)) // n_simd) * lat[i]
            if t < best:
                best, lanes = t, cand
    if RC.has_exp_joint(m):
        lanes = 64
    while lanes < 64 and block_bytes(m, 64 // lanes, esz, env_tables, st) > cap:
        lanes *= 2
    return lanes


def frame_jacobian_shape(m, lanes, esz, env_tables=True, B=B_ENVS, n_simd=1024, fused=False):
    """(lanes per environment, LDS bytes, fits) of k_frame_jacobian for a batch of B environments forced to `lanes` (0: the library's choice, which
    depends on the device's SIMDs only for batches of more environments than it has SIMDs) — csrc/tsim_hip.hip ts_plan's TS_K_FRAME_JACOBIAN branch
    and frame_jacobian_plan: the batch's shape (launch_shape, decide_stage_cpt; 64 lanes with a rotation-vector joint), then the lanes double until
    the contexts and the slots' column blocks (fj_slot_reals) fit 64 KB; the blocks together are rounded up to 16 bytes.  fits: the launch is not
    refused ("do not fit the block's LDS").  fused: the batch runs a compiled-in model's fused kernels (their latencies decide the automatic
    shape)"""
    st = False
    if 3 * int(m.I[Bl.TSIM_IH_NCPT]) * esz <= CPT_LDS_BYTES:      # decide_stage_cpt
        st = _launch_lanes(m, lanes, esz, env_tables, False, B, n_simd, fused) == _launch_lanes(m, lanes, esz, env_tables, True, B, n_simd, fused) \
            and block_bytes(m, 1, esz, env_tables, True) <= LDS_CAP
    lanes = _launch_lanes(m, lanes, esz, env_tables, st, B, n_simd, fused)
    blk = fj_slot_reals(m.ndof_r, m.ndof_u) * esz
    while lanes < 64 and block_bytes(m, 64 // lanes, esz, env_tables, st) + (64 // lanes) * blk > LDS_CAP:
        lanes *= 2
    ns = 64 // lanes
    nbytes = block_bytes(m, ns, esz, env_tables, st) + (ns * blk + 15) // 16 * 16
    return lanes, nbytes, nbytes <= LDS_CAP


# ---------------------------------------------------------------------------------------------------- models and cases
def wide_model(name):
    return load_model(os.path.join(HERE, "models", name + ".xml"))


# start and velocity per model, by dof in the XML's order: sled x y z, carriage x y z, arm x y, finger [, tail y]
_Q0 = {"wide9": [0, 0, -0.0003, 0, 0, -0.0006, 0, 0, 0.3],
       "wide10": [0, 0, -0.0003, 0, 0, -0.0006, 0, 0, -0.3, -0.001]}
_QD0 = {"wide9": [0.6, 0.1, 0, 0, 0, 0, 0.005, -0.002, 0.05],
        "wide10": [0.6, 0.1, 0, 0, 0, 0, 1.2, -0.4, -0.05, -0.3]}
# u per frame.  wide9: sled force x y z, carriage position x y z (a position motor's control is its target, in metres), arm force x y, finger force;
# wide10: sled force, carriage position, finger force
_U = {"wide9": [[0.9, 0.2, -0.1, 0.002, 0.000, -0.0020, 0.10, -0.05, 0.7],
                [0.7, 0.3, 0.0, 0.003, 0.001, -0.0024, 0.15, -0.05, 0.8],
                [0.8, 0.1, -0.2, 0.001, -0.001, -0.0018, 0.90, -0.60, 0.6]]}
_U["wide10"] = [r[:6] + [-r[8]] for r in _U["wide9"]]      # (the finger pushed below its LOWER limit: wide9 has it above the upper one)


def wide_case(name, B=B_ENVS, T=T_FRAMES):
    """model, q0 [B, nr], qd0 [B, nr], u [B, T, nu], sub-steps per frame; the environments differ by a seeded offset of start and controls small
    enough that each keeps the case's conditions (tests/test_wide_models.py asserts them on every environment)"""
    m = wide_model(name)
    rng = np.random.default_rng(900 + m.ndof_r)
    q0 = np.tile(np.asarray(_Q0[name], dtype=np.float64), (B, 1)) + 5e-5 * rng.normal(size=(B, m.ndof_r))
    qd0 = np.tile(np.asarray(_QD0[name], dtype=np.float64), (B, 1)) * (1.0 + 0.1 * rng.normal(size=(B, m.ndof_r)))
    u = np.tile(np.asarray(_U[name], dtype=np.float64)[None, :T], (B, 1, 1))
    u = np.clip(u * (1.0 + 0.1 * rng.normal(size=u.shape)), -0.98, 0.98)
    assert q0.shape[1] == m.ndof_r and u.shape[2] == m.ndof_u
    return m, q0, qd0, u, SUBSTEPS


# The column kinds a gradient tally of the GPU file must hold above its floor (tests/test_gpu_param_grad_oracle.py, test_gpu_body_param_grad_oracle.py
# Tally.check): the kinds the ORACLE's gradient has there in at least three entries over the five environments — tests/test_wide_models.py
# asserts it on the CPU with those tallies.  Contact columns, by (model, fp64): wide9's pad creeps and then slides, so its taxels stick and slip;
# wide10's pad slides throughout (kt has no gradient there).  The fp32 floor is 1e-3 of the row's largest entry, which the damping columns do not
# reach (as on TactilePush, F32_PUSHER_KINDS).  Body columns: the finger is beyond its upper limit in wide9 and below its lower one in wide10.
_C = ("pair kn", "pair kt", "pair mu", "pair damping", "sensor kn", "sensor kt", "sensor mu", "sensor damping", "dof damping")
CONTACT_KINDS = {("wide9", True): _C, ("wide9", False): tuple(k for k in _C if not k.endswith(" damping") or k == "dof damping"),
                 ("wide10", True): tuple(k for k in _C if not k.endswith(" kt")), ("wide10", False): ("pair mu", "sensor kn", "sensor mu", "dof damping")}
_B = ("mass", "com", "inertia", "motor lo", "motor hi", "motor P", "motor D", "limit lo", "limit hi", "limit k")
BODY_KINDS = {"wide9": tuple(k for k in _B if k != "limit lo"), "wide10": tuple(k for k in _B if k != "limit hi")}


def limit_dofs(m):
    """[(dof, lo, hi)] of the dofs with a limit spring"""
    d0 = int(m.I[Bl.TSIM_IH_FOFF_DOF])
    out = []
    for k in range(m.ndof_r):
        lo, hi, kk = (float(m.F[d0 + k * Bl.TSIM_DF_SIZE + j]) for j in (Bl.TSIM_DF_LIM_LO, Bl.TSIM_DF_LIM_HI, Bl.TSIM_DF_LIM_K))
        if kk > 0:
            out.append((k, lo, hi))
    return out


def conditions(m, q0, qd0, u, S):
    """One environment on the oracle, sub-step by sub-step: (non-converged sub-steps, sub-steps, sub-steps with a loaded point of a ground pair
    with general contact points, sub-steps with such a point slipping, sub-steps with a loaded taxel, sub-steps with a dof outside its limit)"""
    from oracle.oracle import OracleSim
    import random_corpus as RC
    o = OracleSim(m)
    o.reset(q0, qd0)
    info = RC.pair_info(m)
    ground = {p for p in range(len(info)) if info[p][0] == Bl.TSIM_P_PLANE and not info[p][1]}      # a plane pair that is no sphere-on-plane pair
    lim = limit_dofs(m)
    bad = n = loaded = slip = tax = inlim = 0
    for t in range(u.shape[0]):
        for _ in range(S):
            bad += o.forward(u[t], 1)
            q, qd = o.state()
            c = [r for r in o.contact_list(q, qd) if r[0] in ground]
            n += 1
            loaded += bool(c)
            slip += any((r[2] & 1) == 0 for r in c)
            tax += bool(o.taxel_list(q, qd)) if m.ndof_tactile else 0
            inlim += any(q[k] < lo or q[k] > hi for k, lo, hi in lim)
    return bad, n, loaded, slip, tax, inlim
