"""The case matrix of the reference-tracking IK tests (include/blf/blf_c.h section 12d):
tests/test_ik_track_reference.py (CPU: intended statuses, the conditioning band) and
tests/test_gpu_ik_track.py (blf_fb_ik_track against tests/ik_track_reference.py) share it.  Plain helper module.

A case: dict(model, B, states, tasks (section 12's host arrays; its se3_pose / com_pos are not used),
rows (hard->rows), limits (dict or None), schedule (tests/ik_track_reference.py's dict), dT, expect [B]:
the status each robot ends with).

  walk        humanoid24 (two robots per wavefront), B = 3, T = 20: robot.walking_ik_schedule with the
              gaits at 0, 1/2 and 1/4 of a cycle, so robots 0 and 1 (one wavefront) hold opposite stance
              soles and each robot's mask changes at its own lift-offs and touch-downs; CoM x and y hard,
              robot.humanoid24_joint_limits.  T = 1 and 2 are prefixes of the same trajectory.
  limbs48     the four-limbed tree of tests/ik_hard_cases.py (n = 48, one robot per wavefront, K = 4
              and the CoM), B = 3, T = 4, a different contact pattern per robot and per step
  limbs12     a four-limbed tree of n = 12 (K = 4): robot 0 holds tasks {0, 1}, robot 1 tasks {2, 3}, so
              the wavefront's union counts 24 rows > 6 + n = 18 while each robot's own 12 do not
  limbs12-over  the same pair with robot 0 holding all four tasks (24 rows > 6 + n: dependent by count)
  limbs12-dup   tasks 2 and 3 on one frame with different targets: robot 0 holds both (a pivot of S
              fails), robot 1 holds {0, 1}
Draws outside the band (tests/test_ik_track_reference.py) were replaced by changing the seed."""
import functools

import numpy as np

import fb_models as FM
import ik_cases as IC
import ik_hard_cases as HC
import ik_hard_reference as HR
import ik_limits_cases as LC
import ik_limits_reference as LR
import ik_reference as IK
import ik_track_reference as TR
import swing_foot_reference as SF
from blf import robot

DT = HC.DT
WALK_T = 20
WALK_SHIFT = (0.0, 0.5, 0.25)

# How far the reference's own stance soles are from (1 - kp_lin dT)^m times their error at the start of
# a contact of m steps: the hard rows give the sole exactly the velocity kp_lin (p_des - p) at the state
# of the solve, but the explicit Euler step of the joints moves it by that velocity times dT only to
# first order.  The rest is the step's second-order term, about |s_dot|^2 dT^2 times the leg's length per
# step: with the other sole swinging 4 cm in 6 steps the joints turn at about 1 rad/s, so about 4e-5 m
# per step and a few 1e-4 m over a contact.  Measured on the reference over the walking case (printed by
# tests/test_ik_track_reference.py): 4.42e-4 m at most over a contact, against 3.46e-3 m with the weights alone.  The GPU test
# allows STANCE_LAW_TOL for the hard rows and asks the weights-only run to be CONTRAST_MIN away.
STANCE_LAW_TOL, CONTRAST_MIN = 6.0e-4, 3.0e-3


def swing_schedule(w, B, K):
    """robot.walking_ik_schedule's dict through the numpy swing_foot_eval: the schedule dict."""
    r = SF.swing_foot_eval(w["contact_pose"], w["contact_time"], w["ncontacts"], w["tq"],
                           step_height=w["step_height"])
    T = w["steps"]
    return dict(steps=T, stance_rows=w["stance_rows"], contact=r["in_contact"].reshape(B, K, T),
                se3_pose=r["pose"].reshape(B, K, T, 12), se3_twist=r["twist"].reshape(B, K, T, 6),
                com_pos=w["com_pos"], com_vel=None)


def walk_inputs(B, shift, seed=5, steps=WALK_T):
    """The walking humanoids: (model, states, tasks, rows, limits, walking_ik_schedule's dict).  Every
    base starts about 0.3 mm and 0.3 mrad off the pose the schedule was built for, so the soles start
    with an error for the hard rows to shrink."""
    model = robot.humanoid24()
    st = robot.standing_states(model, B, seed=seed, spread=0.2)
    w = robot.walking_ik_schedule(model, st, steps, DT, shift=shift)
    rng = np.random.default_rng(seed + 1)
    st = dict(st, base_pos=st["base_pos"] + rng.normal(size=(B, 3)) * 3.0e-4,
              base_rot=np.stack([robot._rotvec(rng.normal(size=3) * 3.0e-4) for _ in range(B)]))
    tasks = robot.standing_ik_tasks(model, st)
    rows = HR.mask([[False] * 6] * 2, [True, True, False])
    limits = dict(robot.humanoid24_joint_limits(model, sampling_time=DT), max_iter=0)
    return model, st, tasks, rows, limits, w


@functools.lru_cache(maxsize=None)
def _limbs12(seed=33):
    n, B = 12, 2
    parent = [0 if j % 3 == 0 else j for j in range(n)]
    model = FM.tree_model(parent, seed, frame_links=[3, 6, 9, 12])
    states = robot.random_states(model, B, seed=seed + 7)
    return dict(model=model, B=B, states=states)


def _held(cs, frames, contact, T, seed, rows=0, limits=None, expect=None):
    """A case whose set points are held over the T steps (make_tasks' targets) with the contact flags
    contact [B][K] (held) or [B][K][T]."""
    model, B, states = cs["model"], cs["B"], cs["states"]
    tasks = cs["tasks"] if "tasks" in cs else IC.make_tasks(model, states, frames, seed)
    K = len(tasks["frame"])
    c = np.asarray(contact, dtype=np.int32)
    c = np.repeat(c[:, :, None], T, axis=2) if c.ndim == 2 else c
    com = tasks.get("com_weight") is not None
    sch = dict(steps=T, stance_rows=(1 << (6 * K)) - 1, contact=np.ascontiguousarray(c),
               se3_pose=np.repeat(np.asarray(tasks["se3_pose"])[:, :, None, :], T, axis=2),
               se3_twist=None if tasks.get("se3_twist") is None
               else np.repeat(np.asarray(tasks["se3_twist"])[:, :, None, :], T, axis=2),
               com_pos=np.repeat(np.asarray(tasks["com_pos"])[:, None, :], T, axis=1) if com else None,
               com_vel=None)
    return dict(model=model, B=B, states=states, tasks=tasks, rows=rows, limits=limits, schedule=sch, dT=DT,
                expect=[LR.OK] * B if expect is None else expect)


@functools.lru_cache(maxsize=None)
def build_case(cid):
    if cid == "walk":
        model, st, tasks, rows, limits, w = walk_inputs(3, WALK_SHIFT)
        return dict(model=model, B=3, states=st, tasks=tasks, rows=rows, limits=limits,
                    schedule=swing_schedule(w, 3, 2), dT=DT, expect=[LR.OK] * 3)
    if cid == "limbs48":
        cs = LC.build_case("limbs48-hard-27")
        contact = np.zeros((3, 4, 4), dtype=np.int32)
        contact[0, [0, 1]] = 1            # robot 0: tasks 0 and 1 throughout
        contact[1, 2, :2] = 1             # robot 1: task 2 lifts off after step 1, task 3 lands at step 2
        contact[1, 3, 2:] = 1
        contact[2, [0, 2, 3], 1:] = 1     # robot 2: nothing at step 0, then three tasks
        return _held(cs, None, contact, 4, 0, rows=HR.mask([[False] * 6] * 4, HC.COM), limits=cs["limits"])
    if cid == "limbs12":
        return _held(_limbs12(), [0, 1, 2, 3], [[1, 1, 0, 0], [0, 0, 1, 1]], 3, 36)
    if cid == "limbs12-over":
        return _held(_limbs12(), [0, 1, 2, 3], [[1, 1, 1, 1], [0, 0, 1, 1]], 3, 36,
                     expect=[LR.HARD_DEPENDENT, LR.OK])
    if cid == "limbs12-dup":
        return _held(_limbs12(), [0, 1, 2, 2], [[0, 0, 1, 1], [1, 1, 0, 0]], 3, 36,
                     expect=[LR.HARD_DEPENDENT, LR.OK])
    raise KeyError(cid)


CASES = ["walk", "limbs48", "limbs12", "limbs12-over", "limbs12-dup"]


@functools.lru_cache(maxsize=None)
def reference(cid):
    """TR.track of every robot of the case, computed once and shared (and never changed)."""
    cs = build_case(cid)
    return [TR.track(cs["model"], cs["states"], cs["tasks"], cs["rows"], cs["limits"], cs["schedule"], i, cs["dT"])
            for i in range(cs["B"])]


def prefix(ref, T):
    """The result of a T-step call from the reference of a longer one with the same first T slices
    (every step of `ref` up to T resolved)."""
    assert ref["fail_step"] < 0 or ref["fail_step"] >= T
    bt, nt = ref["base_traj"][T - 1], ref["nu_traj"][T - 1]
    state = dict(base_pos=bt[:3], base_rot=bt[3:].reshape(3, 3), joint_pos=ref["joint_traj"][T - 1],
                 base_vel=nt[:6], joint_vel=nt[6:])
    return dict(state=state, joint_traj=ref["joint_traj"][:T], base_traj=ref["base_traj"][:T],
                nu_traj=ref["nu_traj"][:T], status=LR.OK, fail_step=-1,
                iters=sum(s["iters"] for s in ref["steps"][:T]), active=ref["steps"][T - 1]["active"])


def sole_positions(model, tasks, base_traj, joint_traj):
    """The sole frames' positions [T, K, 3] along one robot's trajectory."""
    import fb_dynamics as F
    out = np.empty((base_traj.shape[0], len(tasks["frame"]), 3))
    for t in range(base_traj.shape[0]):
        s = dict(base_pos=base_traj[t, :3], base_rot=base_traj[t, 3:].reshape(3, 3), joint_pos=joint_traj[t])
        K = IK.kin(model, s)
        for k, f in enumerate(tasks["frame"]):
            out[t, k] = F.frame_state(model, K, int(f))[0]
    return out


def stance_law_error(model, tasks, states, sch, i, base_traj, joint_traj, dT):
    """How far robot i's stance soles are from the hard rows' law: over every run of steps t0 .. t1 - 1
    in which sole k is in contact, the linear error after step t1 - 1 should be (1 - kp_lin dT)^(t1 - t0)
    times the error before step t0 (the set point is constant over a contact).  Returns the largest
    |e_end - f e_start| over the runs [m], and the largest |e_start| met."""
    T = base_traj.shape[0]
    bt = np.vstack([np.concatenate([states["base_pos"][i], np.asarray(states["base_rot"][i]).reshape(-1)]), base_traj])
    jt = np.vstack([states["joint_pos"][i], joint_traj])
    p = sole_positions(model, tasks, bt, jt)          # p[t]: before step t; p[T]: after the last
    worst, start = 0.0, 0.0
    c = np.asarray(sch["contact"])[i]
    for k in range(c.shape[0]):
        t = 0
        while t < T:
            if not c[k, t]:
                t += 1
                continue
            t1 = t
            while t1 < T and c[k, t1]:
                t1 += 1
            des = np.asarray(sch["se3_pose"])[i, k, t, :3]
            f = (1.0 - float(tasks["se3_kp"][k][0]) * dT) ** (t1 - t)
            worst = max(worst, np.abs((des - p[t1, k]) - f * (des - p[t, k])).max())
            start = max(start, np.abs(des - p[t, k]).max())
            t = t1
    return worst, start
