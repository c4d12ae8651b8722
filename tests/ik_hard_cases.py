"""The case matrix of the hard-task IK tests (include/blf/blf_c.h section 12b):
tests/test_ik_hard_reference.py (CPU: the conditioning of every case) and tests/test_gpu_ik_hard.py
(blf_fb_ik_solve_hard / blf_fb_ik_integrate_hard against tests/ik_hard_reference.py) share it.
Plain helper module.

A case is a case of tests/ik_cases.py (model, states, tasks) or the four-limbed tree below, with a
mask of hard rows.  Well-posed masks ("ok") have relative pivots of S of at least 1e-5 on every robot,
dependent ones ("dep") of at most 1e-11 in magnitude at the pivot that fails
(test_ik_hard_reference.py::test_case_conditioning holds every case to its band)."""
import functools

import numpy as np

import fb_models as FM
import ik_cases as IC
import ik_hard_reference as HR
from blf import robot

ALL, NONE = [True] * 6, [False] * 6
LIN, ANG = [True] * 3 + [False] * 3, [False] * 3 + [True] * 3
COM, COMXY, NOCOM = [True] * 3, [True, True, False], [False] * 3

# id -> (base case, se3 [K][6], com [3], kind, overrides of the task set)
CASES = {}


def _case(cid, base, se3, com=NOCOM, kind="ok", **over):
    CASES[cid] = (base, se3, com, kind, over)


# n = 24, two robots per wavefront: every row hard (15), one task and the CoM's x, y (8)
_case("rand24-k2com-15", "rand24-k2com", [ALL, ALL], COM)
_case("rand24-k2com-8", "rand24-k2com", [ALL, NONE], COMXY)
# the optional inputs NULL
_case("rand24-k2com-null-15", "rand24-k2com-null", [ALL, ALL], COM)
# an SO3-only and an R3-only task with the CoM (9 rows; their zero-weight rows cannot be hard)
_case("rand24-so3-r3-9", "rand24-so3-r3", [ANG, LIN, NONE], COM)
# the humanoid's standing set at B = 130 (65 wavefronts), the base held by the hard feet alone
_case("humanoid-15-nodamp-b130", "humanoid-standing-b130", [ALL, ALL], COM, base_damping=0.0)
# n = 26 | 27: the boundary between two robots per wavefront and one; prismatic joints at both layouts
_case("pri-chain26-k2com-15", "pri-chain26-k2com", [ALL, ALL], COM)
_case("chain27-k2com-15", "chain27-k2com", [ALL, ALL], COM)
_case("chain27-k2com-9", "chain27-k2com", [ALL, NONE], COM)
_case("pri-rand48-k2-12", "pri-rand48-k2", [ALL, ALL])
_case("chain48-k2com-far-15", "chain48-k2com-far", [ALL, ALL], COM)
# small sizes: 7 rows against 9 unknowns, 1 row against 7
_case("chain3-k4-7", "chain3-k4", [ALL, [True] + [False] * 5, NONE, NONE])
_case("chain1-k2com-1", "chain1-k2com", [NONE, NONE], [False, False, True])
# the CoM alone; one task 3 rad from its target; B = 1
_case("star27-k0com-3", "star27-k0com", [], COM)
_case("rand24-far-6", "rand24-far", [ALL])
_case("rand24-b1-9", "rand24-b1", [ALL, NONE], COM)   # (its two frames sit on one link)
# every one of the 27 rows, n = 48: four 12-joint limbs with a frame on each tip
_case("limbs48-k4com-27", "limbs48", [ALL, ALL, ALL, ALL], COM)
# dependent: two hard tasks on one frame; 12 rows against 7 unknowns; three tasks down one chain of a
# tree; four frames of which one sits on the base link
_case("rand26-k4-same-dep", "rand26-k4-same", [ALL, ALL, NONE, NONE], kind="dep")
_case("chain1-k2com-12-dep", "chain1-k2com", [ALL, ALL], kind="dep")
_case("rand24-so3-r3-dep", "rand24-so3-r3", [ANG, LIN, ALL], kind="dep")
_case("rand48-k4com-dfs-dep", "rand48-k4com-dfs", [ALL, ALL, ALL, ALL], kind="dep")

OK_CASES = sorted(c for c in CASES if CASES[c][3] == "ok")
DEP_CASES = sorted(c for c in CASES if CASES[c][3] == "dep")


@functools.lru_cache(maxsize=None)
def _limbs48():
    """Four chains of 12 joints from the base (DFS preorder), a frame on the tip of each."""
    n, seed, B = 48, 33, 3
    parent = [0 if j % 12 == 0 else j for j in range(n)]
    model = FM.tree_model(parent, seed, frame_links=[12, 24, 36, 48])
    states = robot.random_states(model, B, seed=seed + 7)
    return dict(model=model, B=B, states=states, tasks=IC.make_tasks(model, states, [0, 1, 2, 3], seed + 3))


@functools.lru_cache(maxsize=None)
def build_case(cid):
    """dict(model, B, states, tasks, rows (section 12b's mask), se3, com, kind) of case `cid`."""
    base, se3, com, kind, over = CASES[cid]
    cs = _limbs48() if base == "limbs48" else IC.build_case(base)
    return dict(model=cs["model"], B=cs["B"], states=cs["states"], tasks=dict(cs["tasks"], **over),
                rows=HR.mask(se3, com), se3=se3, com=com, kind=kind)


# The cases that are also integrated, over 1, 2 and 20 steps of DT.  A trajectory of 20 steps can be
# far more sensitive than one solve (the set points are 0.05 m and 0.3 rad away and the hard rows
# force the motion through whatever configuration lies between), so every (case, steps) here is held
# on the CPU to the reference's own accuracy: the float64 projection's loop agrees with the KKT loop to
# 1e-10 (test_ik_hard_reference.py::test_integrate_case_conditioning).  rand24-k2com-15 (1.8e-10),
# chain27-k2com-15 (5.1e-10) and the four-limbed tree drawn with seeds 31 and 32 (6.4e-7, 2.3e-9) were
# outside that band at 20 steps and were replaced by rand24-k2com-null-15, chain27-k2com-9 and seed 33.
INTEGRATE_CASES = ["chain1-k2com-1", "chain3-k4-7", "rand24-k2com-null-15", "rand24-so3-r3-9",
                   "pri-chain26-k2com-15", "chain27-k2com-9", "pri-rand48-k2-12", "chain48-k2com-far-15",
                   "limbs48-k4com-27", "humanoid-15-nodamp-b130"]
DT = 0.01


@functools.lru_cache(maxsize=None)
def integrate_reference(cid, steps):
    """HR.integrate of the case's first three robots over `steps` steps of DT, computed once."""
    cs = build_case(cid)
    return [HR.integrate(cs["model"], cs["states"], cs["tasks"], cs["rows"], i, steps, DT)
            for i in range(min(cs["B"], 3))]


@functools.lru_cache(maxsize=None)
def planted_feet():
    """The humanoid standing with each sole about 0.3 mm and 0.3 mrad (N(0, 1e-4) per coordinate) off
    its set point and the CoM target 3 cm ahead of the CoM: dict(model, B, states, tasks, rows) with
    robot.standing_ik_tasks and robot.standing_ik_hard.  On the reference, 20 steps of DT with the
    hard rows shrink every sole's pose error to about 0.35 of its value (kp dT = 0.05 per step; the
    Euler step's own drift is about 1e-5), and with the weights alone both soles end 0.36 to 0.63 mm
    away, further than they began."""
    import fb_dynamics as F
    import ik_reference as IK
    from blf.robot import _rotvec
    model, B = robot.humanoid24(), 5
    st = robot.standing_states(model, B, seed=5, spread=0.2)
    tasks = robot.standing_ik_tasks(model, st)
    rng = np.random.default_rng(8)
    for i in range(B):
        K = IK.kin(model, {k: st[k][i] for k in IK.STATE_KEYS})
        for k, f in enumerate(tasks["frame"]):
            pf, Rf, _, _ = F.frame_state(model, K, int(f))
            tasks["se3_pose"][i, k, :3] = pf + rng.normal(size=3) * 1.0e-4
            tasks["se3_pose"][i, k, 3:] = (_rotvec(rng.normal(size=3) * 1.0e-4) @ Rf).reshape(-1)
        tasks["com_pos"][i] = IK.com(model, K)[0] + np.array([0.03, 0.0, 0.0])
    return dict(model=model, B=B, states=st, tasks=tasks, rows=HR.mask(**robot.standing_ik_hard(model)))


def sole_errors(model, tasks, state, i):
    """|(p_des - p, Log(R_des R^T))| of every SE3 task of robot i at the one-robot state `state`."""
    import fb_dynamics as F
    import ik_reference as IK
    K = IK.kin(model, state)
    out = []
    for k, f in enumerate(tasks["frame"]):
        pf, Rf, _, _ = F.frame_state(model, K, int(f))
        des = tasks["se3_pose"][i, k]
        out.append(np.linalg.norm(np.concatenate([des[:3] - pf, IK.log3(des[3:].reshape(3, 3), Rf)])))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """HR.solve of every robot of the case, computed once and shared: list of (nu, status, parts)."""
    cs = build_case(cid)
    return [HR.solve(cs["model"], cs["states"], cs["tasks"], cs["rows"], i) for i in range(cs["B"])]
