"""The random-model corpora of the random-model tests (tests/test_gpu_random_models.py and the tests that borrow its models), and a sampler of
contact states on the CPU oracle.

  small corpus  "0" .. "119": `_random_model(max_dof=12)` at seed SEED0 + k, any size the kernels take (what the suite has run since round 5);
  large corpus  "L<k>": `_random_model(max_dof=16)` at seed LARGE_SEED0 + k, redrawn until 13 <= ndof_r <= 16 — the sizes where every lane of a
                16-lane slot and every row of the 16-row register solve is in use; 24 offsets k chosen so that every ndof_r of 13..16 is present
                (4 / 3 / 3 / 14 models: tests/test_oracle_random_models.py asserts the histogram);
  "chain16"     tests/models/chain16.xml: ndof_r = ndof_u = 16 (every joint driven), ground and general-primitive contact — no drawn model
                reaches ndof_u = 16.

A case id is an int (small corpus: the ids the tests have always had) or one of the strings above."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_native_model_loader import _random_model      # noqa: E402

SEED0 = int(os.environ.get("TSIM_RANDOM_SEED0", "1000"))
N_MODELS = int(os.environ.get("TSIM_RANDOM_MODELS", "120"))      # (a soak: TSIM_RANDOM_MODELS=2000 TSIM_RANDOM_SEED0=100000)
LARGE_SEED0 = 7000
LARGE = ["L%d" % k for k in (26, 36, 66, 94,  7, 22, 45,  10, 16, 77,  0, 1, 2, 3, 4, 5, 6, 8, 9, 11, 12, 13, 14, 15)]
CHAIN16 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "models", "chain16.xml")
PRIM_NAMES = {0: "plane", 1: "cuboid", 2: "sphere", 3: "cylinder"}


def _fits(m, spec, nr_lo):
    # (the kernels take ndof_r 1..16, ndof_u <= 16 and one rotation-vector joint per model: include/tsim.h)
    return nr_lo <= m.ndof_r <= 16 and m.ndof_u <= 16 and sum(J["type"] == "free3d-exp" for J in spec["joints"]) <= 1


def draw(case, tmp_path, files=False):
    """(model, rng after the draw) of a case id, or None when no draw within the kernels' sizes was found; the model XML is written to
    tmp_path / "m<seed>.xml" (chain16: its own file)."""
    from tactilesimulation_amd.model.compiler import parse_xml, compile_spec, load_model
    if case == "chain16":
        return load_model(CHAIN16), np.random.default_rng(16016)
    if isinstance(case, str):
        seed, max_dof, nr_lo, tries = LARGE_SEED0 + int(case[1:]), 16, 13, 200
    else:
        seed, max_dof, nr_lo, tries = SEED0 + int(case), 12, 1, 20
    rng = np.random.default_rng(seed)
    p = str(tmp_path / ("m%d.xml" % seed))
    for _ in range(tries):
        open(p, "w").write(_random_model(rng, max_dof=max_dof, files_dir=str(tmp_path) if files else None))
        spec = parse_xml(p)
        m = compile_spec(spec)
        if _fits(m, spec, nr_lo):
            return m, rng
    return None


def xml_path(case, tmp_path):
    if case == "chain16":
        return CHAIN16
    return str(tmp_path / ("m%d.xml" % ((LARGE_SEED0 + int(case[1:])) if isinstance(case, str) else (SEED0 + int(case)))))


def pair_info(m):
    """per contact pair: (primitive type, sphere-on-plane flag, offset of the pair's reals in the blob)"""
    import tactilesimulation_amd.model.blob as BL
    I = m.I
    out = []
    for p in range(int(I[BL.TSIM_IH_NPAIR])):
        pi = int(I[BL.TSIM_IH_OFF_PAIR]) + p * BL.TSIM_PI_SIZE
        out.append((int(I[pi + BL.TSIM_PI_PRIM]), bool(int(I[pi + BL.TSIM_PI_FLAGS]) & 2), int(I[BL.TSIM_IH_FOFF_PAIR]) + p * BL.TSIM_PF_SIZE))
    return out


def state_keys(m, contacts):
    """coverage keys of a state's penetrating points: ("prim", name), ("sphere_plane",), ("stick" | "slip", name)"""
    info = pair_info(m)
    keys = set()
    for pair, _, br, _, _ in contacts:
        prim, sp, _ = info[pair]
        name = PRIM_NAMES[prim]
        keys.add(("prim", name))
        if sp:
            keys.add(("sphere_plane",))
        keys.add(("stick" if br & 1 else "slip", name))
    return keys


def without_contact(m, pairs):
    """copy of the model with kn = kt = 0 on the given contact pairs (the contact part of H is H minus H of this model)"""
    import copy
    import tactilesimulation_amd.model.blob as BL
    m2 = copy.copy(m)
    m2.F = m.F.copy()
    info = pair_info(m)
    for p in pairs:
        m2.F[info[p][2] + BL.TSIM_PF_KN] = 0.0
        m2.F[info[p][2] + BL.TSIM_PF_KT] = 0.0
    return m2


def contact_states(m, seed, k=6, draws=400):
    """Up to k states in contact, by rejection sampling on the CPU oracle: q1 ~ N(0, sigma^2) for sigma in (0.05, 0.3, 1), qd ~ N(0, 0.3^2),
    q0 = q1 - h qd, random u.  A draw is kept when it has a penetrating point and brings a coverage key (state_keys) not yet seen, or while fewer
    than k/2 are kept.  Returns [(q1, q0, qd0, u, contacts)]."""
    from oracle.oracle import OracleSim
    rng = np.random.default_rng(seed)
    o = OracleSim(m)
    nr, nu = m.ndof_r, m.ndof_u
    out, seen = [], set()
    for j in range(draws):
        if len(out) >= k:
            break
        sigma = (0.05, 0.3, 1.0)[j % 3]
        q1 = sigma * rng.normal(size=nr)
        qd = 0.3 * rng.normal(size=nr)
        u = rng.uniform(-1, 1, size=max(nu, 1))[:nu]
        c = o.contact_list(q1, qd)
        if not c:
            continue
        keys = state_keys(m, c)
        if keys - seen or len(out) < k // 2:
            seen |= keys
            out.append((q1, q1 - m.h * qd, qd, u, c))
    return out


def state_seed(case):
    """seed of a case's contact-state sampler"""
    if case == "chain16":
        return 31999
    return 31000 + (500 + LARGE.index(case) if isinstance(case, str) else int(case))


def has_exp_joint(m):
    import tactilesimulation_amd.model.blob as BL
    I = m.I
    return any(int(I[int(I[BL.TSIM_IH_OFF_LINK]) + l * BL.TSIM_LI_SIZE + BL.TSIM_LI_JTYPE]) == BL.TSIM_J_SPHERICAL_EXP for l in range(int(I[BL.TSIM_IH_NL])))


def force_lanes(sim, m, lanes):
    """sim.set_lanes_per_env(lanes) and the shape the library reports: the forced one, or 64 with a rotation-vector joint, or the next wider one where
    the block's LDS would exceed 64 KB (tsim_hip.hip launch_shape: the lanes double until it fits)"""
    sim.set_lanes_per_env(lanes)
    got = sim.launch_info()["lanes_per_env"]
    if has_exp_joint(m):
        assert got == 64, (lanes, got)
    else:
        assert got == lanes or (got > lanes and sim.launch_info()["lds_bytes"] <= 64 * 1024), (lanes, got, m.ndof_r, str(sim.dtype))
    return got
