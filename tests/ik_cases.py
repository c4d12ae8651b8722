"""The case matrix of the whole-body IK tests: tests/test_ik_reference.py (CPU: the conditioning of
every case) and tests/test_gpu_ik.py (blf_fb_ik_solve / blf_fb_ik_integrate against
tests/ik_reference.py) share it.  Plain helper module.

A case is (model, states, tasks): a tree of tests/fb_models.py or the humanoid, a batch of
robot.random_states, and a task set drawn around the robots' own frame poses: each SE3 set point is
the frame's pose moved by N(0, 0.05) m and turned by _rotvec(N(0, 0.3)) (or by 3 rad where the case
says so), the CoM set point the robot's CoM moved by N(0, 0.03) m, the joint set points the joint
positions moved by N(0, 0.1).  SE3 and CoM row weights are drawn from 1..100, joint weights from
1e-2..1; base_damping is 1e-3 where the tasks leave base directions unconstrained (no SE3 task with
all six weights) and 0 otherwise."""
import functools

import numpy as np

import fb_dynamics as F
import fb_models as FM
import ik_reference as IK
from blf import robot
from blf.robot import _rotvec


def make_tasks(model, states, frames, seed, com=True, twist=True, com_vel=True, joint_vel=True,
               zero_linear=(), zero_angular=(), far=(), base_damping=None):
    """A task set for the B robots of `states` on the model's frames `frames` (see the module
    docstring).  zero_linear / zero_angular: task indices whose linear / angular weights are zero
    (SO3-only / R3-only); far: task indices whose desired rotation is 3 rad from the current one."""
    rng = np.random.default_rng(seed)
    B, n = states["joint_pos"].shape
    K = len(frames)
    pose = np.zeros((B, K, 12))
    cpos = np.zeros((B, 3))
    for i in range(B):
        s = {k: states[k][i] for k in IK.STATE_KEYS}
        Kn = IK.kin(model, s)
        for k, f in enumerate(frames):
            pf, Rf, _, _ = F.frame_state(model, Kn, f)
            if k in far:
                ax = rng.normal(size=3)
                dR = _rotvec(3.0 * ax / np.linalg.norm(ax))
            else:
                dR = _rotvec(rng.normal(size=3) * 0.3)
            pose[i, k, :3] = pf + rng.normal(size=3) * 0.05
            pose[i, k, 3:] = (dR @ Rf).reshape(-1)
        cpos[i] = IK.com(model, Kn)[0] + rng.normal(size=3) * 0.03
    w = rng.uniform(1.0, 100.0, (K, 6))
    for k in zero_linear:
        w[k, :3] = 0.0
    for k in zero_angular:
        w[k, 3:] = 0.0
    full = any((w[k] > 0).all() for k in range(K))
    if base_damping is None:
        base_damping = 0.0 if full else 1.0e-3
    return dict(frame=np.array(frames, dtype=np.int32), se3_weight=w,
                se3_kp=rng.uniform(0.5, 5.0, (K, 2)), se3_pose=pose,
                se3_twist=rng.normal(size=(B, K, 6)) * 0.2 if twist and K else None,
                com_weight=rng.uniform(1.0, 100.0, 3) if com else None, com_kp=2.0,
                com_pos=cpos if com else None,
                com_vel=rng.normal(size=(B, 3)) * 0.1 if com and com_vel else None,
                joint_weight=rng.uniform(1.0e-2, 1.0, n), joint_kp=rng.uniform(0.5, 2.0, n),
                joint_pos=states["joint_pos"] + rng.normal(size=(B, n)) * 0.1,
                joint_vel=rng.normal(size=(B, n)) * 0.1 if joint_vel else None,
                base_damping=float(base_damping))


# id -> (topology, n, seed, B, options).  The trees' frames (fb_models.default_frame_links): 0 on the
# base link (no joint columns), 1 the deepest leaf, 2 halfway down to it, 3 the last link.
# Options: frames, com, twist, com_vel, joint_vel, zero_linear, zero_angular, far (make_tasks),
# prismatic (joint indices or "tree"), relabel (fb_models.dfs_relabel).
CASES = {}


def _case(cid, topo, n, seed, B=3, **opt):
    CASES[cid] = (topo, n, seed, B, opt)


# sizes 1, 2, 3 (K = 2 with CoM, K = 0 with the CoM alone, K = 4 without it)
_case("chain1-k2com", "chain", 1, 11, frames=[0, 1])
_case("star2-k0com", "star", 2, 12, frames=[])
_case("chain3-k4", "chain", 3, 13, frames=[0, 1, 2, 3], com=False)
# n = 24 on a random tree; the optional inputs given, then every one of them NULL
_case("rand24-k2com", "rand", 24, 14, frames=[1, 3])
_case("rand24-k2com-null", "rand", 24, 14, frames=[1, 3], twist=False, com_vel=False, joint_vel=False)
# SO3-only and R3-only tasks beside a full one
_case("rand24-so3-r3", "rand", 24, 15, frames=[1, 2, 3], zero_linear=[0], zero_angular=[1])
# n = 26 | 27: the last size served two robots per wavefront and the first served one;
# two tasks on one frame
_case("rand26-k4-same", "rand", 26, 16, frames=[1, 1, 2, 0], com=False, twist=False, joint_vel=False)
_case("chain27-k2com", "chain", 27, 17, frames=[1, 2])
_case("star27-k0com", "star", 27, 18, frames=[])
# n = 48: a DFS-relabelled random tree with every task, the widest tree, a 3 rad rotation error
_case("rand48-k4com-dfs", "rand", 48, 19, frames=[0, 1, 2, 3], relabel=True)
_case("star48-k0com", "star", 48, 20, frames=[])
_case("chain48-k2com-far", "chain", 48, 21, frames=[1, 2], far=[0])
_case("rand24-far", "rand", 24, 22, frames=[3], far=[0], com=False)
# prismatic joints at both layouts; the task frames on the deepest leaf have prismatic ancestors
_case("pri-chain26-k2com", "chain", 26, 23, frames=[1, 2], prismatic=[0, 12, 13, 25])
_case("pri-rand48-k2", "rand", 48, 448, frames=[1, 3], prismatic="tree", com=False)
# batch sizes: 1, and 130 (65 wavefronts of two robots; one more than 128)
_case("rand24-b1", "rand", 24, 24, B=1, frames=[1, 3])
_case("humanoid-standing-b130", "humanoid", 24, 25, B=130)
_case("chain27-b130", "chain", 27, 26, B=130, frames=[1])


@functools.lru_cache(maxsize=None)
def build_case(cid):
    """dict(model, B, states, tasks) of case `cid`."""
    topo, n, seed, B, opt = CASES[cid]
    if topo == "humanoid":
        model = robot.humanoid24()
        states = robot.standing_states(model, B, seed=seed, spread=0.2)
        states["joint_pos"] = states["joint_pos"] + np.random.default_rng(seed).normal(size=(B, n)) * 0.05
        return dict(model=model, B=B, states=states, tasks=robot.standing_ik_tasks(model, states))
    parent = FM._TOPO[topo](n, seed)
    pri = opt.get("prismatic", ())
    if isinstance(pri, str):
        pri = FM._tree_prismatic(parent)
    model = FM.tree_model(parent, seed, prismatic=pri)
    states = robot.random_states(model, B, seed=seed + 7)
    if opt.get("relabel"):
        model = FM.dfs_relabel(model)
        states = FM.permute_states(states, model["perm"])
    kw = {k: opt[k] for k in ("com", "twist", "com_vel", "joint_vel", "zero_linear", "zero_angular", "far")
          if k in opt}
    return dict(model=model, B=B, states=states, tasks=make_tasks(model, states, opt["frames"], seed + 3, **kw))


@functools.lru_cache(maxsize=None)
def reference(cid):
    """IK.solve of every robot of the case, computed once and shared: list of (nu, status, H, g)."""
    cs = build_case(cid)
    return [IK.solve(cs["model"], cs["states"], cs["tasks"], i) for i in range(cs["B"])]


@functools.lru_cache(maxsize=None)
def translation_reference(cid):
    """The reference on the case's grid-rounded, unshifted inputs (fb_models.shift_ik), once per case
    and shared by the translation tests: (list of IK.solve tuples, list of IK.integrate tuples over
    fb_models.IK_STEPS steps)."""
    cs = build_case(cid)
    (st, tk), _ = FM.shift_ik(cs["states"], cs["tasks"], 0)
    B = min(cs["B"], 3)
    return ([IK.solve(cs["model"], st, tk, i) for i in range(B)],
            [IK.integrate(cs["model"], st, tk, i, FM.IK_STEPS, FM.IK_DT) for i in range(B)])
