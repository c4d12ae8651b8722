"""Kinematic trees of chosen topology and size for the floating-base dynamics tests, and the case
matrix that tests/test_fb_models.py (CPU: the oracle on these trees, and the conditioning of every
case) and tests/test_gpu_fb_topologies.py (the blf_fbd_* / blf_fb_* kernels against the oracle)
share.  Plain helper module: the models are in the layout of blf/robot.py, the physics is
oracle/fb_dynamics.py's.

The kernels of csrc/fb_dynamics.hip choose their control flow by the tree: joints in DFS preorder
or not (Topo.dfs: the subtree sums of the mass-matrix path), n + 6 <= 32 or not (two systems per
wavefront or one), the depth (pointer-jumping rounds, tree levels), the children per link (child
masks) and the contacts per link.  The builders below put a model on each side of each of them."""
import functools

import numpy as np

import fb_dynamics as F
import oracle as O
from blf import robot
from blf.robot import _rotvec

CONTACT_CONTINUOUS, CONTACT_WRENCH = 0, F.CONTACT_WRENCH


# ---- topologies: parent[j] = parent LINK of joint j (link 0 the base, joint j moves link j + 1) ----
def chain(n):
    return list(range(n))


def star(n):
    return [0] * n


def bfs_binary(n):
    """Binary tree numbered level by level: topological, not DFS preorder (n >= 3)."""
    return [j // 2 for j in range(n)]


def random_tree(n, seed):
    rng = np.random.default_rng(seed)
    return [int(rng.integers(0, j + 1)) for j in range(n)]


def ancestor_joints(parent):
    """anc[l] = the joints on the path base -> link l."""
    anc = [[]]
    for j, P in enumerate(parent):
        anc.append(anc[int(P)] + [j])
    return anc


def depths(parent):
    """Ancestor joints of every joint (the kernels' Topo.depth): 0 for a child of the base."""
    return [len(a) - 1 for a in ancestor_joints(parent)[1:]]


def is_dfs_preorder(parent):
    """build_topo's rule (csrc/fb_dynamics.hip): joint k attaches to the base or to a link whose
    joint is joint k - 1 or one of joint k - 1's ancestors.  Then every subtree is a contiguous run
    of joints, and the mass-matrix path takes its subtree sums from one prefix sum."""
    anc = ancestor_joints(parent)
    for k in range(1, len(parent)):
        P = int(parent[k])
        if P != 0 and (P - 1) not in anc[k]:   # anc[k]: link k = joint k - 1's child
            return False
    return True


def default_frame_links(parent):
    """Base, the deepest leaf (the first of them), a link halfway down to it, the last link."""
    n = len(parent)
    anc = ancestor_joints(parent)
    deepest = max(range(1, n + 1), key=lambda l: (len(anc[l]), -l))
    path = anc[deepest]
    mid = path[len(path) // 2] + 1
    return [0, deepest, mid, n]


def tree_model(parent, seed, link_len=0.1, prismatic=(), frame_links=None):
    """A model on the tree `parent`: masses, COMs and inertias drawn as robot.humanoid24 draws them
    (base 8 kg, the principal moments' triangle inequality kept), random unit joint axes, joint
    origins N(0, 0.03) with -link_len on z, mounting rotations _rotvec(N(0, 0.05)); one frame per
    entry of frame_links (default_frame_links if None) with a non-identity rotation and a non-zero
    offset in its link; the joints listed in `prismatic` slide."""
    rng = np.random.default_rng(seed)
    n = len(parent)
    parent = np.array(parent, dtype=np.int32)
    assert all(0 <= parent[j] <= j for j in range(n)), "topological order"
    joint_rot = np.stack([_rotvec(rng.normal(size=3) * 0.05) for _ in range(n)])
    masses = rng.uniform(0.4, 3.0, n + 1)
    masses[0] = 8.0
    com = rng.normal(size=(n + 1, 3)) * 0.02
    inertia = np.zeros((n + 1, 3, 3))
    for l in range(n + 1):
        Q = _rotvec(rng.normal(size=3))
        # humanoid24's draw, sorted so that its clamp of d[2] bounds the largest moment
        d = np.sort(rng.uniform(0.3, 1.0, 3) * masses[l] * 0.004)
        d[2] = min(d[2], d[0] + d[1] - 1e-6)
        inertia[l] = Q @ np.diag(d) @ Q.T
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    origin = rng.normal(size=(n, 3)) * 0.03
    origin[:, 2] -= link_len
    fl = default_frame_links(parent) if frame_links is None else list(frame_links)
    frame_pose = np.zeros((len(fl), 12))
    for f in range(len(fl)):
        frame_pose[f, :3] = rng.normal(size=3) * 0.03 + np.array([0.02, 0.0, -0.04])
        frame_pose[f, 3:] = _rotvec(rng.normal(size=3) * 0.3).reshape(-1)
    model = dict(n=n, parent=parent, joint_origin=origin, joint_rot=joint_rot, joint_axis=axis,
                 link_mass=masses, link_com=com, link_inertia=inertia,
                 frame_link=np.array(fl, dtype=np.int32), frame_pose=frame_pose,
                 names=["base"] + [f"j{j}" for j in range(n)])
    if len(prismatic):
        model = robot.with_joint_types(model, prismatic=[int(j) for j in prismatic])
    return model


def dfs_relabel(model):
    """The same physical tree with joints and links renumbered into DFS preorder (children in
    their old order).  model["perm"][k] = the old index of new joint k; the frames move with their
    links.  permute_states carries a state batch over."""
    n = model["n"]
    parent = [int(p) for p in model["parent"]]
    kids = [[] for _ in range(n + 1)]
    for j, P in enumerate(parent):
        kids[P].append(j)
    order, stack = [], list(reversed(kids[0]))
    while stack:
        j = stack.pop()
        order.append(j)
        stack.extend(reversed(kids[j + 1]))
    assert sorted(order) == list(range(n))
    newlink = np.zeros(n + 1, dtype=np.int64)
    for k, j in enumerate(order):
        newlink[j + 1] = k + 1
    links = [0] + [j + 1 for j in order]
    out = dict(model)
    out["parent"] = np.array([newlink[parent[j]] for j in order], dtype=np.int32)
    for k in ("joint_origin", "joint_rot", "joint_axis"):
        out[k] = np.asarray(model[k])[order]
    for k in ("link_mass", "link_com", "link_inertia"):
        out[k] = np.asarray(model[k])[links]
    if model.get("joint_type") is not None:
        out["joint_type"] = np.asarray(model["joint_type"])[order]
    out["frame_link"] = newlink[np.asarray(model["frame_link"])].astype(np.int32)
    out["names"] = [model["names"][l] for l in links]
    out["perm"] = np.array(order)
    return out


def permute_states(states, perm):
    return {k: (v[:, perm] if k in ("joint_pos", "joint_vel", "joint_torque") else v)
            for k, v in states.items()}


def null_poses_near(model, states, frames, noise=(0.01, 0.02), seed=0):
    """Contact null poses [B][C][12] near where the frames are: the oracle's frame_state at each
    state, moved by N(0, noise[0]) m and rotated by _rotvec(N(0, noise[1])).  The contact springs
    then pull with a physical force on any tree (the idea of robot.sole_null_poses)."""
    rng = np.random.default_rng(seed)
    B = states["base_pos"].shape[0]
    null = np.zeros((B, len(frames), 12))
    for i in range(B):
        K = F.kinematics(model, states["base_pos"][i], states["base_rot"][i], states["joint_pos"][i],
                         states["base_vel"][i], states["joint_vel"][i])
        for c, f in enumerate(frames):
            pf, Rf, _, _ = F.frame_state(model, K, f)
            null[i, c, :3] = pf + rng.normal(size=3) * noise[0]
            null[i, c, 3:] = (_rotvec(rng.normal(size=3) * noise[1]) @ Rf).reshape(-1)
    return null


def contact_set(model, states, frames, seed, mixed=False):
    """Host-side contacts on the model's frames `frames`: parameters (L, W, k, b) that differ per
    contact, null poses from null_poses_near, and with `mixed` alternating laws (continuous,
    given wrench, ...) with random given wrenches."""
    rng = np.random.default_rng(seed)
    C, B = len(frames), states["base_pos"].shape[0]
    params = np.array([0.12, 0.09, 3.0e4, 300.0]) * rng.uniform(0.6, 1.4, (C, 4))
    ct = dict(frame=np.array(frames, dtype=np.int32), params=params,
              null_pose=null_poses_near(model, states, frames, seed=seed + 1), law=None, wrench=None)
    if mixed:
        ct["law"] = np.array([CONTACT_WRENCH if c % 2 else CONTACT_CONTINUOUS for c in range(C)], dtype=np.int32)
        ct["wrench"] = rng.normal(size=(B, C, 6)) * np.array([4.0, 4.0, 30.0, 0.5, 0.5, 0.2])
    return ct


def oracle_kw(ct, i):
    """oracle/fb_dynamics.py dynamics / euler_integrate keywords for system i."""
    if ct is None:
        return {}
    kw = dict(contacts=ct["frame"], contact_params=ct["params"], null_poses=ct["null_pose"][i])
    if ct["law"] is not None:
        kw.update(laws=ct["law"], wrenches=ct["wrench"][i])
    return kw


def system_matrices(model, states, i, ct=None, reg=None):
    """(A, rhs) of system i as F.dynamics assembles them: A = M [+ reg],
    rhs = -h + sum_c J_c^T w_c + [0; tau]."""
    s = {k: v[i] for k, v in states.items()}
    K = F.kinematics(model, s["base_pos"], s["base_rot"], s["joint_pos"], s["base_vel"], s["joint_vel"])
    M, h = F.mass_and_bias(model, K)
    rhs = -h
    if ct is not None:
        for c, f in enumerate(ct["frame"]):
            pf, Rf, vel, J = F.frame_state(model, K, f)
            if ct["law"] is not None and ct["law"][c] == CONTACT_WRENCH:
                w = ct["wrench"][i][c]
            else:
                w = O.contact_eval(ct["params"][c], vel, np.concatenate([pf, Rf.reshape(-1)]),
                                   ct["null_pose"][i][c])[0]
            rhs = rhs + J.T @ w
    rhs[6:] += s["joint_torque"]
    return (M + reg if reg is not None else M), rhs


def refined_solve(A, b, rounds=5):
    """A^-1 b by LAPACK, improved by `rounds` of iterative refinement with the residual
    accumulated in np.longdouble."""
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    x = np.linalg.solve(A, b).astype(np.longdouble)
    for _ in range(rounds):
        r = bl - Al @ x
        x = x + np.linalg.solve(A, r.astype(np.float64)).astype(np.longdouble)
    return x


def rel_err(a, b):
    """tests/gpu_util.py's metric as a Python float (this module imports no torch, so not gpu_util)."""
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def backward_error(A, x, b):
    """|A x - b|_inf / (|A|_inf |x|_inf + |b|_inf) in np.longdouble."""
    Al, xl, bl = A.astype(np.longdouble), np.asarray(x).astype(np.longdouble), b.astype(np.longdouble)
    r = np.abs(Al @ xl - bl).max()
    return float(r / (np.abs(Al).sum(axis=1).max() * np.abs(xl).max() + np.abs(bl).max()))


# ---- the case matrix ------------------------------------------------------------------------------
# id -> (topology, n, seed, options).  Options: contacts = the model's frame indices in contact
# (frames: default_frame_links unless frame_links is given), mixed (given-wrench laws), prismatic
# (joint indices), relabel (dfs_relabel of the same tree), link_len.
def _c8_links(parent):
    """C = 8: the base, the deepest leaf, one interior link twice, the last link, three others."""
    n = len(parent)
    base, deepest, mid, last = default_frame_links(parent)
    interior = next(l for l in range(1, n + 1) if l in set(parent) and l not in (deepest, mid))
    rest = [l for l in (n // 3, n // 2 + 1, n - 2) if l >= 1][:3]
    return [base, deepest, interior, interior, last] + rest


_TOPO = dict(chain=lambda n, seed: chain(n), star=lambda n, seed: star(n),
             bfs=lambda n, seed: bfs_binary(n), rand=random_tree)

CASES = {}


def _case(cid, topo, n, seed, **opt):
    CASES[cid] = (topo, n, seed, opt)


# articulated-body path, no contacts: sizes 1, 2, NV = 32 (n = 26), the first one-per-wavefront
# size (27) and the largest (48), as the deepest and the widest tree of each size
for _n in (1, 2, 26, 27, 48):
    _case(f"chain{_n}", "chain", _n, 100 + _n)
    _case(f"star{_n}", "star", _n, 200 + _n)
for _n in (26, 27, 48):
    _case(f"bfs{_n}", "bfs", _n, 300 + _n)
    _case(f"rand{_n}", "rand", _n, 400 + _n)
# maxdepth 7 | 8 and 31 | 32: the two sides of a pointer-jumping round boundary (15 | 16 lie inside
# the longer chains, whose joints run through every depth)
for _n in (8, 9, 32, 33):
    _case(f"chain{_n}", "chain", _n, 100 + _n)
# with contacts, for both solve paths: the non-DFS trees and their DFS relabelling
_case("rand26-c8", "rand", 26, 426, contacts="c8")
_case("rand26-c8-dfs", "rand", 26, 426, contacts="c8", relabel=True)
_case("bfs26-c1base", "bfs", 26, 326, contacts=[0])
_case("bfs26-c1base-dfs", "bfs", 26, 326, contacts=[0], relabel=True)
_case("rand48-c8mixed", "rand", 48, 448, contacts="c8", mixed=True)
_case("rand48-c8mixed-dfs", "rand", 48, 448, contacts="c8", mixed=True, relabel=True)
_case("bfs48-c8", "bfs", 48, 348, contacts="c8")
_case("bfs48-c8-dfs", "bfs", 48, 348, contacts="c8", relabel=True)
_case("rand48-c1base", "rand", 48, 448, contacts=[0])
_case("chain48-c2", "chain", 48, 148, contacts=[1, 2])
_case("star48-c2", "star", 48, 248, contacts=[0, 3])
_case("n1-c2", "chain", 1, 101, contacts=[0, 1])
# prismatic joints: joint 0, the last joint, an interior joint and a child of a prismatic joint
_case("pri-chain26-c2", "chain", 26, 126, contacts=[1, 2], prismatic=[0, 12, 13, 25])
_case("pri-rand48-c2", "rand", 48, 448, contacts=[1, 3], prismatic="tree")

# (case, solve path): "aba" the default articulated-body solve, "matrix" the mass-matrix /
# Cholesky path (mass_reg given: 0.05 I, and zeros, which has the ABA's solution)
RUNS = [(c, "aba") for c in CASES if "-" not in c]
RUNS += [(c, s) for c in ("rand26-c8", "bfs26-c1base", "rand48-c8mixed", "bfs48-c8", "rand48-c1base",
                          "pri-chain26-c2", "pri-rand48-c2") for s in ("aba", "matrix")]
RUNS += [(c, "matrix") for c in ("rand26-c8-dfs", "bfs26-c1base-dfs", "rand48-c8mixed-dfs", "bfs48-c8-dfs",
                                 "chain48-c2", "star48-c2", "n1-c2")]
REG = 0.05
T0, T1, DT = 0.0, 0.0025, 0.001   # three Euler steps, the last one stale-time


def _tree_prismatic(parent):
    """Joint 0, the last joint, an interior joint with a child, and that child."""
    n = len(parent)
    j = next(j for j in range(1, n - 1) if (j + 1) in set(parent[j + 1:]))
    k = next(k for k in range(j + 1, n) if parent[k] == j + 1)
    return sorted({0, j, k, n - 1})


@functools.lru_cache(maxsize=None)
def build_case(cid):
    """dict(model, B, states [B + 1 rows: the last one the sentinel row's], contacts (host dict over
    B + 1 systems, or None)) of case `cid`."""
    topo, n, seed, opt = CASES[cid]
    parent = _TOPO[topo](n, seed)
    pri = opt.get("prismatic", ())
    if isinstance(pri, str):
        pri = _tree_prismatic(parent)
    fl = None
    contacts = opt.get("contacts")
    if contacts == "c8":
        fl = _c8_links(parent)
        contacts = list(range(8))
    model = tree_model(parent, seed, link_len=opt.get("link_len", 0.1), prismatic=pri, frame_links=fl)
    B = 5 if n + 6 <= 32 else 3
    states = robot.random_states(model, B + 1, seed=seed + 7)
    if opt.get("relabel"):
        model = dfs_relabel(model)
        states = permute_states(states, model["perm"])
    ct = contact_set(model, states, contacts, seed + 11, mixed=opt.get("mixed", False)) if contacts else None
    return dict(model=model, B=B, states=states, contacts=ct)


def reg_of(model, kind):
    NV = model["n"] + 6
    return {"none": None, "reg": REG * np.eye(NV), "zero": np.zeros((NV, NV))}[kind]


@functools.lru_cache(maxsize=None)
def reference(cid, kind):
    """The oracle's dynamics and three-step Euler result of every system of the case, computed
    once per (case, regularisation kind) and shared: (list of F.dynamics tuples, list of final
    states).  kind "zero" is the unregularised solution."""
    cs = build_case(cid)
    reg = reg_of(cs["model"], "reg") if kind == "reg" else None
    dyn, eul = [], []
    for i in range(cs["B"]):
        kw = oracle_kw(cs["contacts"], i)
        dyn.append(F.dynamics(cs["model"], cs["states"], i, reg=reg, **kw))
        eul.append(F.euler_integrate(cs["model"], cs["states"], i, T0, T1, DT, reg=reg, **kw))
    return dyn, eul


# ---- translations of the world frame ------------------------------------------------------------------
# tests/test_fb_translation.py (CPU: the references are insensitive to where the origin is) and
# tests/test_gpu_fb_translation.py (the kernels on the shifted inputs against the references on the
# unshifted ones) share these.  Positions are first rounded to a grid of 2^-bits m, so adding a power-
# of-two shift is exact and the shifted problem is the same physical problem bit for bit.
SHIFTS = (3, 7, 10, 13)   # 8 m, 128 m, 1 km, 8 km from the origin


def on_grid(a, bits=20):
    """a rounded to multiples of 2^-bits."""
    s = float(2 ** bits)
    return np.round(np.asarray(a, dtype=np.float64) * s) / s


def shift_vec(k):
    return np.array([2.0 ** k, -(2.0 ** k), 2.0 ** (k - 1)])


def _shifted(a, d):
    """a + d on the leading len(d) components of the last axis, asserted exact."""
    m = len(d)
    out = np.array(a, dtype=np.float64, copy=True)
    out[..., :m] = out[..., :m] + d
    assert np.array_equal(out[..., :m] - d, np.asarray(a)[..., :m]), "the shift must be exact"
    return out


def shift_case(states, contacts, k):
    """((states, contacts) with base_pos and null_pose[..., :3] on the grid, the same shifted by
    shift_vec(k)); contacts may be None."""
    d = shift_vec(k)
    g_st = dict(states, base_pos=on_grid(states["base_pos"]))
    s_st = dict(g_st, base_pos=_shifted(g_st["base_pos"], d))
    g_ct = s_ct = None
    if contacts is not None:
        null = np.array(contacts["null_pose"], dtype=np.float64, copy=True)
        null[..., :3] = on_grid(null[..., :3])
        g_ct = dict(contacts, null_pose=null)
        s_ct = dict(contacts, null_pose=_shifted(null, d))
    return (g_st, g_ct), (s_st, s_ct)


def shift_ik(states, tasks, k):
    """The same for an IK case: base_pos, se3_pose[..., :3] and com_pos."""
    d = shift_vec(k)
    g_st = dict(states, base_pos=on_grid(states["base_pos"]))
    s_st = dict(g_st, base_pos=_shifted(g_st["base_pos"], d))
    g_tk, s_tk = dict(tasks), dict(tasks)
    pose = np.array(tasks["se3_pose"], dtype=np.float64, copy=True)
    pose[..., :3] = on_grid(pose[..., :3])
    g_tk["se3_pose"], s_tk["se3_pose"] = pose, _shifted(pose, d)
    if tasks.get("com_pos") is not None:
        g_tk["com_pos"] = on_grid(tasks["com_pos"])
        s_tk["com_pos"] = _shifted(g_tk["com_pos"], d)
    return (g_st, g_tk), (s_st, s_tk)


QP_SHIFTS = (10, 13)
QP_KEYS = ("xi_init", "xi_ref", "vrp_ref", "corners")


def shift_plan(prob, k):
    """(the DCM-MPC batch `prob` with xi_init, xi_ref, vrp_ref and corners rounded to 2^-24 m, the same
    shifted by (2^k, -2^(k-1)))."""
    d = np.array([2.0 ** k, -(2.0 ** (k - 1))])
    g = dict(prob)
    for key in QP_KEYS:
        g[key] = np.ascontiguousarray(on_grid(prob[key], 24))
    s = dict(g)
    for key in QP_KEYS:
        s[key] = np.ascontiguousarray(_shifted(g[key], d))
    return g, s


def base_pos_allowance(k, steps):
    """|(base_pos shifted back) - reference| after `steps` Euler steps: one rounding of a coordinate of
    size <= 2^(k+1) per step and per side, and the 1e-9 of the comparison itself."""
    return steps * 2.0 ** (k - 51) + 1e-9


def position_allowance(k, tol=1e-9):
    """A position written in shifted world coordinates and shifted back: 4 roundings at 2^(k-52)."""
    return 4 * 2.0 ** (k - 52) + tol


# (case, regularisation kind) of the translation tests: "none" the articulated-body solve, "reg" /
# "zero" the mass-matrix path with mass_reg = REG I / zeros.  "humanoid24": robot.humanoid24 with
# two sole contacts whose null poses lie N(0, 0.01) m from the origin, identity rotations.
TRANSLATION_RUNS = [("humanoid24", k) for k in ("none", "zero", "reg")]
for _c, _kinds in (("rand26-c8", "nrz"), ("rand26-c8-dfs", "rz"), ("rand48-c8mixed", "nrz"),
                   ("rand48-c8mixed-dfs", "rz"), ("chain48-c2", "nrz"), ("star48-c2", "rz"),
                   ("pri-rand48-c2", "nrz"), ("n1-c2", "rz")):
    TRANSLATION_RUNS += [(_c, dict(n="none", r="reg", z="zero")[_k]) for _k in _kinds]
TRANSLATION_KIN_CASES = ("chain48", "bfs27")
TRANSLATION_IK_CASES = ("rand24-k2com", "chain27-k2com", "rand48-k4com-dfs", "chain48-k2com-far",
                        "pri-rand48-k2", "star48-k0com")
IK_STEPS, IK_DT = 3, 0.01
EULER_STEPS = 3   # of (T0, T1, DT)


@functools.lru_cache(maxsize=None)
def translation_case(cid):
    """build_case(cid), or the humanoid with its two sole contacts (B = 5 and a sentinel row)."""
    if cid != "humanoid24":
        return build_case(cid)
    model, B = robot.humanoid24(), 5
    states = robot.random_states(model, B + 1, seed=21)
    null = np.zeros((B + 1, 2, 12))
    null[:, :, :3] = np.random.default_rng(0).normal(size=(B + 1, 2, 3)) * 0.01
    null[:, :, 3:] = np.eye(3).reshape(-1)
    ct = dict(frame=np.array([0, 1], dtype=np.int32), params=np.array([[0.12, 0.09, 3.0e4, 300.0]] * 2),
              null_pose=null, law=None, wrench=None)
    return dict(model=model, B=B, states=states, contacts=ct)


def oracle_run(model, B, states, contacts, kind):
    """F.dynamics and the three-step F.euler_integrate of systems 0 .. B - 1 (reference()'s pair)."""
    reg = reg_of(model, "reg") if kind == "reg" else None
    dyn, eul = [], []
    for i in range(B):
        kw = oracle_kw(contacts, i)
        dyn.append(F.dynamics(model, states, i, reg=reg, **kw))
        eul.append(F.euler_integrate(model, states, i, T0, T1, DT, reg=reg, **kw))
    return dyn, eul


@functools.lru_cache(maxsize=None)
def translation_reference(cid, kind):
    """oracle_run on the case's grid-rounded, UNSHIFTED inputs (kind "zero" is "none"'s), once per
    (case, kind) and shared; the rounding does not depend on the shift."""
    cs = translation_case(cid)
    (st, ct), _ = shift_case(cs["states"], cs["contacts"], 0)
    return oracle_run(cs["model"], cs["B"], st, ct, "reg" if kind == "reg" else "none")


@functools.lru_cache(maxsize=None)
def impedance_case(stiff=True):
    """The arguments of tests/test_gpu_closed_loop.py::test_fbd_euler_impedance_vs_oracle: six standing
    humanoids on their soles, 20 Euler steps of 1 ms under the posture law's joint impedance.
    stiff=False: the soles of tests/test_gpu_fb_dynamics.py (k = 3e4 N/m^3, b = 300) in place of the
    closed loop's (k = 2e6, b = 2e4), which turn the last place of a world coordinate 8 km out
    (2^-40 m) into 1.6e-9 of joint velocity in the references themselves."""
    from blf import closed_loop as DL
    model, B = robot.humanoid24(), 6
    st = robot.standing_states(model, B, seed=5)
    law = robot.posture_law_arrays(model)
    ct = dict(frame=np.arange(2, dtype=np.int32), params=np.tile(np.asarray(DL.CONTACT_PARAMS if stiff else (0.12, 0.09, 3.0e4, 300.0)), (2, 1)),
              null_pose=robot.sole_null_poses(model, st), law=None, wrench=None)
    return dict(model=model, B=B, states=st, contacts=ct, kp=law["kp"], kd=law["kd"],
                q_ref=np.random.default_rng(3).normal(size=(B, model["n"])) * 0.02,
                t0=0.0, t1=0.02, dT=0.001, steps=20)


def state_errors(got, ref, k, keys):
    """(worst rel_err over the state keys but base_pos, |(got base_pos - shift_vec(k)) - ref|_inf) of
    one system: `got` in the shifted world, `ref` in the unshifted one."""
    worst = max(rel_err(np.asarray(got[key]).reshape(-1), np.asarray(ref[key]).reshape(-1))
                for key in keys if key != "base_pos")
    back = float(np.abs((np.asarray(got["base_pos"]) - shift_vec(k)) - ref["base_pos"]).max())
    return worst, back
