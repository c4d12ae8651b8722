"""TEST INFRASTRUCTURE ONLY -- numpy restatement of include/blf/blf_c.h section 12d (reference tracking
with a per-robot, per-step contact schedule) for one robot, the checker of blf_fb_ik_track: the
per-step loop of tests/ik_limits_reference.py's solve() and the oracle's fbk_euler_integrate, with the
hard rows rows(b, t) and the set points of step t taken from the schedule.

A schedule dict: steps T, stance_rows (section 12b's bit layout, SE3 bits only), contact [B, K, T] int
or None, se3_pose [B, K, T, 12], se3_twist [B, K, T, 6] or None, com_pos [B, T, 3] (iff the task set has
a CoM task), com_vel [B, T, 3] or None: blf_swing_foot_eval's outputs for B*K lists reshaped."""
import numpy as np

import ik_limits_reference as LR
import ik_reference as IK
import oracle as O

OK = LR.OK


def rows_at(rows, sch, i, t):
    """rows(b, t) of section 12d for robot i."""
    r = int(rows)
    if sch.get("contact") is not None:
        c = np.asarray(sch["contact"])
        for k in range(c.shape[1]):
            if c[i, k, t] != 0:
                r |= int(sch["stance_rows"]) & (0x3F << (6 * k))
    return r


def step_tasks(tasks, sch, i, t):
    """The one-robot task set of robot i with step t's set points."""
    out = dict(tasks)
    K = len(tasks["frame"]) if tasks.get("frame") is not None else 0
    out["se3_pose"] = np.asarray(sch["se3_pose"], dtype=np.float64)[i, :, t][None] if K else None
    tw = sch.get("se3_twist")
    out["se3_twist"] = np.asarray(tw, dtype=np.float64)[i, :, t][None] if K and tw is not None else None
    com = tasks.get("com_weight") is not None
    out["com_pos"] = np.asarray(sch["com_pos"], dtype=np.float64)[i, t][None] if com else None
    cv = sch.get("com_vel")
    out["com_vel"] = np.asarray(cv, dtype=np.float64)[i, t][None] if com and cv is not None else None
    for k in ("joint_pos", "joint_vel"):
        out[k] = np.asarray(tasks[k], dtype=np.float64)[i:i + 1] if tasks.get(k) is not None else None
    return out


def slice_schedule(sch, t):
    """The one-step schedule of step t (P1's slices)."""
    out = dict(sch, steps=1)
    for k in ("contact", "se3_pose", "se3_twist"):
        if sch.get(k) is not None:
            out[k] = np.ascontiguousarray(np.asarray(sch[k])[:, :, t:t + 1])
    for k in ("com_pos", "com_vel"):
        if sch.get(k) is not None:
            out[k] = np.ascontiguousarray(np.asarray(sch[k])[:, t:t + 1])
    return out


def track(model, states, tasks, rows, lim, sch, i, dT, rho=0.01):
    """blf_fb_ik_track of robot i: dict(state (five keys), joint_traj [T, n], base_traj [T, 12], nu_traj
    [T, 6+n], status, fail_step, iters, active, and per step: rows (the masks), steps (LR.solve's dicts:
    margin, pivots, iters, status))."""
    n, T = model["n"], int(sch["steps"])
    lim = LR.no_limits(n) if lim is None else lim
    s = {k: np.array(states[k][i], dtype=np.float64) for k in IK.STATE_KEYS}
    jt, bt, nt = np.full((T, n), np.nan), np.full((T, 12), np.nan), np.full((T, 6 + n), np.nan)
    nu, status, fail, iters, act = np.full(6 + n, np.nan), OK, -1, 0, (0, 0)
    masks, steps = [], []
    for t in range(T):
        rt = rows_at(rows, sch, i, t)
        r = LR.solve(model, {k: v[None] for k, v in s.items()}, step_tasks(tasks, sch, i, t), rt, lim, 0)
        masks.append(rt)
        steps.append(r)
        nu, status, act = r["nu"], r["status"], r["active"]
        iters += r["iters"]
        if status != OK:
            nu, fail = np.full(6 + n, np.nan), t
            break
        st, p, R, q = O.fbk_euler_integrate(rho, s["base_pos"], s["base_rot"], s["joint_pos"], nu[:6], nu[6:],
                                            0.0, dT, dT)
        assert st == 0
        s = dict(base_pos=p, base_rot=R, joint_pos=q)
        jt[t], bt[t], nt[t] = q, np.concatenate([p, np.asarray(R).reshape(-1)]), nu
    state = dict(s, base_vel=nu[:6].copy(), joint_vel=nu[6:].copy())
    return dict(state=state, joint_traj=jt, base_traj=bt, nu_traj=nt, status=status, fail_step=fail, iters=iters,
                active=act if status == OK else (0, 0), rows=masks, steps=steps)
