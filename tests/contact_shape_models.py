"""Small synthetic models for the contact-pair and branch loops of the evaluation (csrc/tsim_eval.h phase2, pair_points_matrix,
pair_contacts_per_direction, phase3; the copies of the point loop in csrc/tsim_param_grad.hip and csrc/tsim_tangent_kernel.h; csrc/tsim_hip.hip
decide_stage_cpt): own XML text, written to a directory the caller owns, in the style of tests/pad_models.py and tests/wide_models.py.  Used by
tests/test_contact_shape_models.py (CPU) and tests/test_gpu_contact_pair_shapes.py.  Importable without torch and without a GPU.

A model is `nb` root branches that only TRANSLATE.  Branch b starts at world (0.4 b, 0, 0) with a prismatic-z (1 dof: z), planar (2: x, z) or
translational (3: x, y, z) joint; dofs beyond three are child links on prismatic joints along x and y, and the branch's last link (its leaf)
carries everything.  A contact pair is an abstract body with a contact-point file (so that npt is exact) on a fixed joint under the leaf of branch
`on`, against the ground plane, or a cuboid / sphere / upright cylinder whose top touches z = 0 at q = 0, world-fixed (a fixed joint at the
root: merged into the world, lb = 0) or on a fixed joint under the leaf of branch `prim_on` (lb > 0); kind "sphere_plane" is a sphere body with
a ground_contact (flag 2, one point).  At q = 0 the lowest point of every pair is GAP above its primitive.

The points of a pair: one LOW point (index `low`) over the primitive's centre, the other near points STEP higher on a 1 mm lattice around it,
and `nfar` points 0.3 m up that never touch.  So which points touch is chosen by how deep the pair is pressed — "graze": GRAZE below the
surface, the low point alone; "deep": DEEP below, every near point — and WHICH index is the low one (point 0, the last point, a point of a
middle chunk) is a datum of the pair.  Because the branches only translate, the gap of every point is plain arithmetic (gaps()), which the CPU
file holds against OracleSim.contact_list.

compile_spec gives every pair its own copy of its body's points: ncpt is the sum of the pairs' npt (the P5 models).  The compiler sets bit 0
of the flags of every pair it emits (model/compiler.py), so the `!(flags & 1)` skips of the loops cannot be reached from XML; no blob is built
by hand to reach them."""
import os

import numpy as np

from tactilesimulation_amd.model.compiler import compile_spec, parse_xml

GAP, STEP, GRAZE, DEEP, FAR_UP, FAR_LIFT = 2e-3, 2e-3, 1e-3, 3.5e-3, 0.3, 0.25
PITCH, SPACING, SLOT = 1e-3, 0.4, 0.1      # lattice of a pair's near points; distance of the branches; distance of the pairs of one branch
MARGIN = 1e-5                              # no point of a named state is this close to its primitive's surface, either side
H = 5e-3
T_FRAMES, SUBSTEPS, B_ENVS = 3, 2, 5
# a root joint's damping: near critical for a branch of 0.1 kg on one contact point of kn = 2e3 (2 sqrt(k m) = 28), so that a pressed branch settles
# on its contact and does not bounce off it within an episode — a depth of 1e-5 m at a sub-step's end would leave the branch to the Newton tolerance
ROOT_DAMPING = 30.0
EPISODE_SEED = 4000      # tests/test_contact_shape_models.py holds every episode drawn from it to one branch signature per environment
PRIM_XML = {"cuboid": ('type="cuboid" size="0.06 0.06 0.04"', 0.02), "sphere": ('type="sphere" radius="0.05"', 0.05),
            "cylinder": ('type="cylinder" radius="0.03" length="0.04"', 0.02)}
SPHERE_R, BALL_R = 0.05, 0.01


def pair(kind, npt=1, on=None, prim_on=None, low=0, nfar=0):
    """a pair of the builder: kind "ground" | "sphere_plane" | "cuboid" | "sphere" | "cylinder"; npt points, `nfar` of them far; general body on
    branch `on` (None: pair index mod nb); primitive world-fixed (prim_on None) or on branch prim_on; low: index of the low point (negative: from
    the end)"""
    assert kind in ("ground", "sphere_plane") + tuple(PRIM_XML) and (kind != "sphere_plane" or npt == 1) and 0 <= nfar < npt
    assert prim_on is None or kind in PRIM_XML
    return {"kind": kind, "npt": npt, "on": on, "prim_on": prim_on, "low": low % npt, "nfar": nfar}


def branch_dofs(nr, nb):
    """dofs per branch: nr dealt over nb branches, the first ones one more"""
    assert nr >= nb >= 1
    return [nr // nb + (b < nr % nb) for b in range(nb)]


def _axes(d):
    """translation axes of a branch's d dofs, in dof order; the z dof is _axes(d).index(z)"""
    root = {1: [(0, 0, 1)], 2: [(1, 0, 0), (0, 0, 1)], 3: [(1, 0, 0), (0, 1, 0), (0, 0, 1)]}[min(d, 3)]
    return root + [((1, 0, 0), (0, 1, 0))[k % 2] for k in range(d - 3)]


def _lattice(n):
    """n lattice offsets (x, y) of pitch PITCH, nearest the centre first"""
    k = int(np.ceil(np.sqrt(n))) // 2 + 1
    pts = sorted(((i, j) for i in range(-k, k + 1) for j in range(-k, k + 1)), key=lambda p: (p[0] * p[0] + p[1] * p[1], p))
    return PITCH * np.asarray(pts[:n], dtype=np.float64)


def pair_points(p):
    """([npt, 3] points of the pair's file, bool [npt] near): the low point at the origin, the other near points STEP up, the far ones FAR_UP up"""
    npt, low, nnear = p["npt"], p["low"], p["npt"] - p["nfar"]
    near = np.zeros(npt, bool)
    near[[i for i in range(npt) if i != low][:nnear - 1] + [low]] = True
    P = np.zeros((npt, 3))
    xy = _lattice(nnear)
    P[low, :2] = xy[0]
    others = [i for i in range(npt) if near[i] and i != low]
    P[others, :2], P[others, 2] = xy[1:], STEP
    far = np.flatnonzero(~near)
    P[far, :2], P[far, 2] = _lattice(len(far)) if len(far) else np.zeros((0, 2)), FAR_UP + 1e-3 * np.arange(len(far))
    return P, near


class Spec:
    """what the builder was asked for, with the derived layout: pairs (on / prim_on filled in), dofs per branch, the first dof of each branch"""

    def __init__(self, nr, pairs, nb):
        self.nr, self.nb, self.dofs = nr, nb, branch_dofs(nr, nb)
        self.dof0 = [sum(self.dofs[:b]) for b in range(nb)]
        self.pairs = [dict(p, on=j % nb if p["on"] is None else p["on"]) for j, p in enumerate(pairs)]
        self.slot = []
        for j, p in enumerate(self.pairs):
            assert p["prim_on"] != p["on"]
            self.slot.append(sum(q["on"] == p["on"] for q in self.pairs[:j]))

    def zdof(self, b):
        return self.dof0[b] + _axes(self.dofs[b]).index((0, 0, 1))

    def shift(self, q):
        """[nb, 3] translation of every branch's leaf at q"""
        q = np.asarray(q, dtype=np.float64)
        return np.stack([np.asarray(_axes(d), dtype=np.float64).T @ q[d0:d0 + d] for d0, d in zip(self.dof0, self.dofs)])


def shape_xml(dirpath, nr, pairs, nb):
    """the XML text of a model of exactly nr dofs, len(pairs) contact pairs and nb root branches; the pairs' point files go to dirpath"""
    s = Spec(nr, pairs, nb)
    under = [""] * nb                      # what hangs under each branch's leaf
    world, contacts = "", ""
    for j, p in enumerate(s.pairs):
        a, cx = p["on"], SLOT * s.slot[j]
        par = 'kn="%.9g" kt="5." mu="0.5" damping="10."' % (2e3 * (1 + 0.1 * j))
        if p["kind"] == "sphere_plane":
            under[a] += ('<link name="g%d"><joint name="g%d" type="fixed" pos="%.9g 0 %.9g" quat="1 0 0 0"/><body name="g%d" type="sphere" radius="%.9g" pos="0 0 0" quat="1 0 0 0" density="1000"/></link>'
                         % (j, j, cx, GAP + BALL_R, j, BALL_R))
        else:
            P, _ = pair_points(p)
            with open(os.path.join(dirpath, "pts_%d.txt" % j), "w") as fh:
                fh.write("%d\n" % len(P) + "".join("%.9g %.9g %.9g\n" % tuple(x) for x in P))
            under[a] += ('<link name="g%d"><joint name="g%d" type="fixed" pos="%.9g 0 %.9g" quat="1 0 0 0"/><body name="g%d" type="abstract" mass="0.02" inertia="1e-5 1e-5 1e-5" pos="0 0 0" quat="1 0 0 0">'
                         '<collision contacts="pts_%d.txt" pos="0 0 0" quat="1 0 0 0"/></body></link>' % (j, j, cx, GAP, j, j))
        if p["kind"] in ("ground", "sphere_plane"):
            contacts += '<ground_contact body="g%d" %s/>' % (j, par)
            continue
        attr, hh = PRIM_XML[p["kind"]]
        b = p["prim_on"]
        x = SPACING * a + cx - (0.0 if b is None else SPACING * b)
        link = ('<link name="p%d"><joint name="p%d" type="fixed" pos="%.9g 0 %.9g" quat="1 0 0 0"/><body name="p%d" %s pos="0 0 0" quat="1 0 0 0" density="200"/></link>' % (j, j, x, -hh, j, attr))
        if b is None:
            world += "<robot>%s</robot>" % link
        else:
            under[b] += link
        contacts += '<general_primitive_contact general_body="g%d" primitive_body="p%d" %s/>' % (j, j, par)
    robots, motors = "", ""
    for b, d in enumerate(s.dofs):
        body = '<body name="%s" type="cuboid" size="0.05 0.05 0.02" pos="0 0 0.1" quat="1 0 0 0" density="1000"/>'
        root = {1: 'type="prismatic" axis="0 0 1"', 2: 'type="planar" axis0="1 0 0" axis1="0 0 1"', 3: 'type="translational"'}[min(d, 3)]
        names = ["b%d" % b] + ["b%d_%d" % (b, k) for k in range(d - 3)]
        inner = under[b]
        for k in reversed(range(1, len(names))):      # the chain below the root, leaf first
            inner = '<link name="%s"><joint name="%s" type="prismatic" axis="%s" pos="0 0 0" quat="1 0 0 0" damping="0.5"/>%s%s</link>' % (
                names[k], names[k], "1 0 0" if (k - 1) % 2 == 0 else "0 1 0", body % names[k], inner)
        robots += '<robot><link name="%s"><joint name="%s" %s pos="%.9g 0 0" quat="1 0 0 0" damping="%g"/>%s%s</link></robot>' % (
            names[0], names[0], root, SPACING * b, ROOT_DAMPING, body % names[0], inner)
        motors += '<motor joint="%s" ctrl="force" ctrl_range="-0.2 0.2"/>' % names[0]
    leaf0 = "b0" if s.dofs[0] <= 3 else "b0_%d" % (s.dofs[0] - 4)
    return ('<redmax model="contact_shape"><option integrator="BDF1" timestep="%g" unit="m-kg" gravity="0. 0. -9.8"/><solver_option tol="1e-5" max_iter="100" max_ls="20"/>'
            '<ground pos="0 0 0" normal="0 0 1"/>%s%s<contact>%s</contact><actuator>%s</actuator><variable><endeffector joint="%s" pos="0.01 0 0"/></variable></redmax>'
            % (H, robots, world, contacts, motors, leaf0))


def shape_model(dirpath, nr, pairs, nb):
    """(compiled model, Spec); dirpath receives model.xml and the point files"""
    dirpath = str(dirpath)
    os.makedirs(dirpath, exist_ok=True)
    p = os.path.join(dirpath, "model.xml")
    with open(p, "w") as fh:
        fh.write(shape_xml(dirpath, nr, pairs, nb))
    return compile_spec(parse_xml(p)), Spec(nr, pairs, nb)


def counts(m):
    """(nr, npair, [npt], ncpt, root branches, [(la, lb)]) of a compiled model, read from its blob"""
    import tactilesimulation_amd.model.blob as Bl
    I = m.I
    npair, nl = int(I[Bl.TSIM_IH_NPAIR]), int(I[Bl.TSIM_IH_NL])
    rec = lambda p, f: int(I[int(I[Bl.TSIM_IH_OFF_PAIR]) + p * Bl.TSIM_PI_SIZE + f])      # noqa: E731
    roots = sum(int(I[int(I[Bl.TSIM_IH_OFF_LINK]) + i * Bl.TSIM_LI_SIZE + Bl.TSIM_LI_PARENT]) == 0 for i in range(nl))
    return (m.ndof_r, npair, [rec(p, Bl.TSIM_PI_NPT) for p in range(npair)], int(I[Bl.TSIM_IH_NCPT]), roots,
            [(rec(p, Bl.TSIM_PI_LINKA), rec(p, Bl.TSIM_PI_LINKB)) for p in range(npair)])


# ---------------------------------------------------------------------------------------------------- geometry of a state
def gaps(s, q):
    """per pair the signed distance [npt] of every point from its primitive's surface at q (negative: inside), by the layout alone"""
    sh = s.shift(q)
    out = []
    for j, p in enumerate(s.pairs):
        if p["kind"] == "sphere_plane":
            out.append(np.array([GAP + sh[p["on"], 2]]))
            continue
        P, _ = pair_points(p)
        rel = P + [0.0, 0.0, GAP] + sh[p["on"]] - (0.0 if p["prim_on"] is None else sh[p["prim_on"]])      # relative to the centre of the primitive's top
        if p["kind"] == "ground":
            out.append(rel[:, 2])
        elif p["kind"] == "sphere":
            out.append(np.linalg.norm(rel + [0.0, 0.0, SPHERE_R], axis=1) - SPHERE_R)
        else:      # a flat top: the points stay over it (asserted), the distance is the height
            half = 0.03
            assert np.all(np.abs(rel[:, :2]).max(1) < half * 0.7), (j, np.abs(rel[:, :2]).max())
            out.append(rel[:, 2])
    return out


def expected_contacts(s, touching):
    """{(pair, point)} a state is designed to have: touching maps a pair to "graze" (its low point) or "deep" (every near point)"""
    out = set()
    for j, how in touching.items():
        p = s.pairs[j]
        near = pair_points(p)[1] if p["kind"] != "sphere_plane" else np.ones(1, bool)
        out |= {(j, p["low"])} if how == "graze" else {(j, int(i)) for i in np.flatnonzero(near)}
    return out


def pose(s, touching, others="far"):
    """q [nr]: the z dofs that press exactly the pairs of `touching` ({pair: "graze" | "deep"}); the branches it leaves free hover at q = 0
    (every pair GAP above its primitive: near, nothing penetrates) or are lifted `far` (FAR_LIFT (b + 1): out of every bounding sphere's reach,
    whose radius is half of FAR_UP; no further, because an fp32 residual loses digits with the size of q)"""
    z = {}
    depth = lambda j: GAP + (GRAZE if touching[j] == "graze" else DEEP)      # noqa: E731
    for j in touching:
        p = s.pairs[j]
        if p["prim_on"] is None:
            assert z.setdefault(p["on"], -depth(j)) == -depth(j), "two world pairs of one branch at different depths"
    for _ in range(len(touching) + 1):
        for j in touching:
            a, b = s.pairs[j]["on"], s.pairs[j]["prim_on"]
            if b is None:
                continue
            if a in z and b not in z:
                z[b] = z[a] + depth(j)
            elif b in z and a not in z:
                z[a] = z[b] - depth(j)
    for j in touching:      # a pair between two branches nothing else holds: the primitive comes up to the body
        a, b = s.pairs[j]["on"], s.pairs[j]["prim_on"]
        if b is not None and a not in z and b not in z:
            z[a], z[b] = 0.0, depth(j)
    q = np.zeros(s.nr)
    top = max(z.values(), default=0.0)
    for b in range(s.nb):
        q[s.zdof(b)] = z[b] if b in z else (top + FAR_LIFT * (b + 1) if others == "far" else 0.0)
    return q


def state(s, m, touching, others="far", seed=0):
    """(q1, q0, qd0, u) of one evaluation: q1 = pose, a small seeded velocity on every dof (far below what moves a point across MARGIN within
    GRAZE), q0 = q1 - h qd0, seeded controls"""
    rng = np.random.default_rng(1000 + seed)
    q1 = pose(s, touching, others)
    qd0 = 0.02 * rng.normal(size=s.nr)
    u = rng.uniform(-0.9, 0.9, size=m.ndof_u)
    return q1, q1 - m.h * qd0, qd0, u


def named_states(s, m):
    """{name: ((q1, q0, qd0, u), {(pair, point)} designed to penetrate)}: "none" (everything far), "hover" (every pair near, nothing penetrates),
    "all" (every pair deep), and per pair j "only<j>:deep" and "only<j>:graze" with the other branches far.  A pair another pair's pose drags
    along (two world pairs of one branch) is in the designed set with it."""
    out = {"none": (state(s, m, {}, "far", 1), set()), "hover": (state(s, m, {}, "hover", 2), set())}
    out["all"] = (state(s, m, {j: "deep" for j in range(len(s.pairs))}, "far", 3), expected_contacts(s, {j: "deep" for j in range(len(s.pairs))}))
    for j, p in enumerate(s.pairs):
        for how in ("deep", "graze"):
            t = {i: how for i, r in enumerate(s.pairs) if i == j or (p["prim_on"] is None and r["prim_on"] is None and r["on"] == p["on"])}
            out["only%d:%s" % (j, how)] = (state(s, m, t, "far", 10 + 2 * j + (how == "graze")), expected_contacts(s, t))
    return out


def eval_batch(s, m):
    """the batch of the debug_eval comparison, in order: per pair "only<j>:deep" (environment e: only pair e mod npair), "none", "all", "hover",
    then per pair "only<j>:graze"; one more "hover" when that makes a multiple of 4.  Returns ([names], [states])"""
    ns = named_states(s, m)
    names = ["only%d:deep" % j for j in range(len(s.pairs))] + ["none", "all", "hover"] + ["only%d:graze" % j for j in range(len(s.pairs))]
    if len(names) % 4 == 0:
        names.append("hover")
    return names, [ns[n][0] for n in names]


def touching_of_env(s, e, only):
    """the pairs environment e of an episode presses: all of them, or (only) pair e mod npair with what its pose drags along — the world pairs of
    its own branch, and for a pair whose primitive sits on another branch the world pairs of THAT branch, which carry the primitive (lifted
    to the body instead, the primitive's branch would fall away from it within a sub-step)"""
    if not only:
        return set(range(len(s.pairs)))
    j = e % len(s.pairs)
    p = s.pairs[j]
    held = {p["on"]} if p["prim_on"] is None else {p["prim_on"]}
    return {j} | {i for i, r in enumerate(s.pairs) if r["prim_on"] is None and r["on"] in held}


def episode_case(s, m, B=B_ENVS, T=T_FRAMES, only=False):
    """(q0 [B, nr], qd0, u [B, T, nu], S): a short episode from a pressed state — every pair grazing, at rest up to a seeded 1e-3 m/s, seeded
    controls (only=True: environment e presses touching_of_env(s, e, True), the other branches far above)"""
    q0 = np.stack([pose(s, {i: "graze" for i in touching_of_env(s, e, only)}, "far") for e in range(B)])
    rngs = [np.random.default_rng(EPISODE_SEED + s.nr + 17 * len(s.pairs) + 1000 * e) for e in range(B)]      # (an environment's draw does not depend on B)
    qd0 = np.stack([1e-3 * r.normal(size=s.nr) for r in rngs])
    u = np.stack([r.uniform(-0.9, 0.9, size=(T, m.ndof_u)) for r in rngs])
    return q0, qd0, u, SUBSTEPS


# ---------------------------------------------------------------------------------------------------- the models
# name -> (nr, nb, pairs, edges).  edges: [(table row, lanes the edge needs (0: any), what)] — the reason the model is here, as data;
# tests/test_contact_shape_models.py holds the compiled counts and the launch arithmetic against it.
def _table():
    T = {}
    T["p1_1"] = (1, 1, [pair("ground", 5, low=0)], [("P1", 0, "npair 1: one group of one"), ("P4", 0, "act / hit masks")])
    T["p1_4"] = (4, 4, [pair("ground", 3, low=0), pair("cuboid", 4, low=-1), pair("sphere", 5, low=2), pair("cylinder", 6, prim_on=0, low=0)],
                 [("P1", 0, "npair 4: one full group"), ("P2", 16, "np nr = 16 = LPE"), ("P4", 16, "four slots with different pairs"),
                  ("P6", 16, "nb nr = 16 = LPE"), ("P6", 0, "cylinder on branch 0 against branch 3, ground pair")])
    T["p1_5"] = (5, 4, [pair("ground", 3, on=0, low=0), pair("sphere", 5, on=0, low=-1), pair("cuboid", 4, on=1, low=1), pair("sphere_plane", 1, on=2),
                        pair("cylinder", 6, on=3, prim_on=1, low=0)],
                 [("P1", 0, "npair 5: a trailing group of one"), ("P2", 16, "np nr = 20 = LPE + 4: a second trip"), ("P4", 16, "act / hit masks"),
                  ("P6", 16, "nb nr = 20"), ("same link", 0, "pairs 0 and 1 on branch 0"), ("lb > 0", 0, "pair 4's cylinder on branch 1")])
    kinds8 = ["ground", "cuboid", "sphere", "cylinder", "sphere_plane", "cuboid", "ground", "sphere"]
    T["p1_8"] = (8, 8, [pair(k, 1 if k == "sphere_plane" else 3 + j, low=0, prim_on=(0 if j == 5 else None)) for j, k in enumerate(kinds8)],
                 [("P1", 0, "npair 8: two full groups"), ("P2", 32, "np nr = 32 = LPE"), ("P4", 32, "act / hit masks"), ("P6", 32, "nb nr = 64")])
    kinds9 = kinds8 + ["cylinder"]
    T["p1_9"] = (9, 9, [pair(k, 1 if k == "sphere_plane" else 3 + j, low=0, prim_on=(0 if j == 5 else 1 if j == 8 else None)) for j, k in enumerate(kinds9)],
                 [("P1", 0, "npair 9: two groups and a trailing group of one"), ("P2", 32, "np nr = 36 = LPE + 4: a second trip"), ("P4", 32, "act / hit masks"),
                  ("P6", 64, "nb = nr = 9: 81 tasks, a second trip at 64 lanes"), ("P6", 0, "pairs 5 and 8 between branches, ground pairs")])
    mid = lambda n: n // 2      # noqa: E731
    T["p2_3x5"] = (5, 3, [pair("ground", 6, low=mid(6)), pair("cuboid", 7, low=mid(7)), pair("sphere", 8, prim_on=0, low=mid(8))],
                   [("P2", 16, "np nr = 15 = LPE - 1"), ("P6", 16, "nb nr = 15")])
    T["p2_4x8"] = (8, 4, [pair("ground", 6, low=3), pair("cuboid", 7, low=3), pair("sphere", 8, low=4), pair("cylinder", 9, prim_on=0, low=4)],
                   [("P2", 32, "np nr = 32 = LPE"), ("P6", 32, "nb nr = 32 = LPE")])
    T["p2_4x9"] = (9, 4, [pair("ground", 6, low=3), pair("cuboid", 7, low=3), pair("sphere", 8, low=4), pair("cylinder", 9, prim_on=0, low=4)],
                   [("P2", 32, "np nr = 36 = LPE + 4: a second trip"), ("P6", 32, "nb nr = 36: a second trip")])
    T["p2_4x16"] = (16, 4, [pair("ground", 6, low=3), pair("cuboid", 7, low=3), pair("sphere", 8, low=4), pair("cylinder", 9, prim_on=0, low=4)],
                    [("P2", 64, "np nr = 64 = LPE"), ("P6", 64, "nb nr = 64 = LPE")])
    # P3: one pair per npt, the low point the LAST one: "graze" is the state in which only the tail chunk's last point touches
    T["p3_a"] = (4, 4, [pair("sphere_plane", 1), pair("ground", 15, low=-1), pair("cuboid", 16, low=-1), pair("sphere", 17, low=-1)],
                 [("P3", l, "npt 1, 15, 16, 17") for l in (16, 32, 64)])
    T["p3_b"] = (4, 4, [pair("cylinder", 31, low=-1), pair("ground", 32, low=-1), pair("sphere", 33, low=-1), pair("cuboid", 63, low=-1, prim_on=0)],
                 [("P3", l, "npt 31, 32, 33, 63") for l in (16, 32, 64)])
    T["p3_c"] = (4, 4, [pair("ground", 64, low=-1), pair("sphere", 65, low=-1), pair("cuboid", 129, low=-1), pair("cylinder", 129, low=70)],
                 [("P3", l, "npt 64, 65, 129 (the last point low), 129 (point 70 low: a middle chunk)") for l in (16, 32, 64)])
    # P5: ncpt on both sides of both staging thresholds (3 ncpt esz <= 8192: 341 | 342 doubles, 682 | 683 floats); all but ten points far
    for n in (341, 342, 682, 683):
        T["p5_%d" % n] = (2, 2, [pair("ground", n - 40, low=-1, nfar=n - 44), pair("cuboid", 40, low=0, nfar=34)],
                          [("P5", 0, "ncpt %d: %s" % (n, {341: "fp64 staged", 342: "fp64 not staged", 682: "fp32 staged", 683: "fp32 not staged"}[n]))])
    # The same edges on the smallest models that carry them: k_tangent holds eight directions' tangent state per slot beside the contexts, and on the
    # four-branch models above four fp64 environments with it exceed a block's 64 KB (p3_a: 53 792 + 4 x 3 328 bytes), so that k_tangent<double>
    # would run them at 32 lanes.  Three one-dof branches (P3), two branches (P2) fit four fp64 slots: the 16-lane edges at 16 lanes in both precisions
    T["t3_a"] = (3, 3, [pair("ground", 15, low=-1), pair("cuboid", 16, low=-1), pair("sphere", 17, low=-1)], [("P3'", 16, "npt 15, 16, 17 in k_tangent")])
    T["t3_b"] = (3, 3, [pair("cylinder", 31, low=-1), pair("ground", 32, low=-1), pair("sphere", 33, low=-1)], [("P3'", 16, "npt 31, 32, 33 in k_tangent")])
    T["t3_c"] = (3, 3, [pair("cuboid", 63, low=-1), pair("ground", 64, low=-1), pair("sphere", 65, low=-1)], [("P3'", 16, "npt 63, 64, 65 in k_tangent")])
    T["t3_d"] = (3, 3, [pair("sphere_plane", 1), pair("cuboid", 129, low=-1), pair("cylinder", 129, low=70, prim_on=0)], [("P3'", 16, "npt 1, 129, 129 in k_tangent")])
    T["t2_4x4"] = (4, 2, [pair("ground", 6, on=0, low=3), pair("cuboid", 7, on=0, low=3), pair("sphere", 8, on=0, low=4), pair("cylinder", 9, on=1, prim_on=0, low=4)],
                   [("P2", 16, "np nr = 16 = LPE in k_tangent's evaluation")])
    T["t2_3x5"] = (5, 2, [pair("ground", 6, on=0, low=3), pair("cuboid", 7, on=0, low=3), pair("sphere", 8, on=1, prim_on=0, low=4)],
                   [("P2", 16, "np nr = 15 = LPE - 1 in k_tangent's evaluation")])
    T["t2_4x5"] = (5, 2, [pair("ground", 3, on=0, low=0), pair("cuboid", 4, on=0, low=1), pair("sphere_plane", 1, on=1), pair("sphere", 5, on=1, low=-1),
                          pair("ground", 6, on=1, low=0)], [("P2", 16, "np nr = 20 = LPE + 4 in k_tangent's evaluation: a second trip")])
    return T


TABLE = _table()
P1 = ("p1_1", "p1_4", "p1_5", "p1_8", "p1_9")
P2 = ("p1_4", "p2_3x5", "p1_5", "p2_4x8", "p2_4x9", "p2_4x16")
P3 = ("p3_a", "p3_b", "p3_c")
P5 = ("p5_341", "p5_342", "p5_682", "p5_683")
P6 = ("p1_9", "p1_4", "p2_4x9")
EPISODE_MODELS = ("p1_5", "p2_4x9", "p3_c", "p1_9") + P5      # one per table row: P1 / P4, P2, P3, P6, P5
GRADIENT_MODELS = P1 + P3 + P5      # the table-gradient comparison: P1, P3, P5
SMALL = ("t3_a", "t3_b", "t3_c", "t3_d", "t2_4x4", "t2_3x5", "t2_4x5")      # the 16-lane edges at 16 lanes in k_tangent<double> too
TANGENT_MODELS = ("p1_4", "p2_3x5", "p1_5", "p2_4x8", "p2_4x9", "p2_4x16", "p3_a", "p3_b", "p3_c", "p1_9") + SMALL      # the tangent identity: P2, P3, P6


def gradient_batch(name):
    """environments of the table-gradient comparison: five, or one more than the pairs — every pair is the lone touching pair of some environment"""
    return max(B_ENVS, len(TABLE[name][2]) + 1)
# lanes per environment when 16 / 32 / 64 are forced, by (bytes of a real, per-environment tables): tests/wide_models.py forced_shape, asserted by
# tests/test_contact_shape_models.py and, against the library, by the GPU file.  Where a block of four (two) contexts exceeds 64 KB the lanes double
_ALL = (16, 32, 64)
_EVERY = {(4, False): _ALL, (4, True): _ALL, (8, False): _ALL, (8, True): _ALL}
_WIDE64 = {**_EVERY, (8, False): (32, 32, 64), (8, True): (32, 32, 64)}
SHAPES = {n: _EVERY for n in TABLE}
SHAPES.update({"p1_8": _WIDE64, "p2_4x8": _WIDE64, "p2_4x9": _WIDE64,
               "p1_9": {(4, False): _ALL, (4, True): (32, 32, 64), (8, False): (32, 32, 64), (8, True): (64, 64, 64)},
               "p2_4x16": {(4, False): (32, 32, 64), (4, True): (32, 32, 64), (8, False): (64, 64, 64), (8, True): (64, 64, 64)}})
# lanes per environment of k_tangent (eight directions, dtables, per-environment tables) when 16 / 32 / 64 are forced, by bytes of a real:
# tests/wide_models.py tangent_shape.  The SMALL models are the ones whose 16-lane edges k_tangent<double> runs at 16 lanes
_T64 = {4: _ALL, 8: (32, 32, 64)}
TAN_SHAPES = {n: _T64 for n in TANGENT_MODELS}
TAN_SHAPES.update({n: {4: _ALL, 8: _ALL} for n in SMALL})
TAN_SHAPES.update({"p2_4x16": {4: (32, 32, 64), 8: (64, 64, 64)}, "p1_9": {4: (32, 32, 64), 8: (64, 64, 64)}})
_MODELS = {}


def table_model(name, dirpath):
    """(compiled model, Spec) of a TABLE entry, compiled once per process; dirpath/name receives its files"""
    if name not in _MODELS:
        nr, nb, pairs, _ = TABLE[name]
        _MODELS[name] = shape_model(os.path.join(str(dirpath), name), nr, pairs, nb)
    return _MODELS[name]


def trips(s, lanes):
    """the trip counts of the loops at `lanes`: (phase2 (pair, direction) per group, point chunks per pair, phase3 (branch, direction))"""
    c = lambda a: -(-a // lanes)      # noqa: E731
    groups = [min(4, len(s.pairs) - g) for g in range(0, len(s.pairs), 4)]
    return [c(np_ * s.nr) for np_ in groups], [c(p["npt"]) for p in s.pairs], c(s.nb * s.nr)
