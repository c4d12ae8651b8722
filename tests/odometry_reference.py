"""TEST INFRASTRUCTURE ONLY -- numpy restatement of include/blf/blf_c.h section 13 (Schmitt-trigger
contact detection and legged odometry) for one robot, the checker of blf_schmitt_trigger_advance and
blf_legged_odometry_advance.  Built on oracle/fb_dynamics.py (kinematics, frame_state); the trigger
step is written in the header's order, one subtraction and one comparison per test.

A trigger is (state, edge_time, switch_time) with state's bit 0 the contact state and bit 1 "an edge
is pending"; its parameters are (on_threshold, off_threshold, switch_on_after, switch_off_after)."""
import numpy as np

import fb_dynamics as F

OK, BAD_INPUT = 0, 2


def trigger_step(prm, t, v, state, edge, sw):
    """One sample (t, v): the new (state, edge_time, switch_time)."""
    t, v = np.float64(t), np.float64(v)
    if not (np.isfinite(v) and np.isfinite(t)):
        return state, edge, sw
    on, pend = bool(state & 1), bool(state & 2)
    cross = (v <= prm[1]) if on else (v >= prm[0])
    after = prm[3] if on else prm[2]
    if cross:
        if not pend:
            pend, edge = True, t
    else:
        pend = False
    if pend and (t - edge) >= after:
        on, sw, pend = not on, t, False
    return int(on) | (int(pend) << 1), edge, sw


def trigger_advance(params, time, value, state, timers):
    """blf_schmitt_trigger_advance on host arrays: value [T, B, K], state [B, K], timers [B, K, 2],
    params [4] or [K, 4].  Returns (state, timers, state_out [T, B, K]); the inputs are not modified."""
    value = np.asarray(value, dtype=np.float64)
    T, B, K = value.shape
    prm = np.broadcast_to(np.asarray(params, dtype=np.float64), (K, 4))
    state, timers = np.array(state, dtype=np.int32), np.array(timers, dtype=np.float64)
    out = np.zeros((T, B, K), dtype=np.int32)
    for t in range(T):
        for b in range(B):
            for c in range(K):
                s, e, w = trigger_step(prm[c], time[t], value[t, b, c], int(state[b, c]), timers[b, c, 0],
                                       timers[b, c, 1])
                state[b, c], timers[b, c, 0], timers[b, c, 1] = s, e, w
                out[t, b, c] = s & 1
    return state, timers, out


def relative_frames(model, frames, joint_pos, joint_vel):
    """Step 2: (p, R, v, w) of every slot's frame with the base at the identity and at rest."""
    K = F.kinematics(model, np.zeros(3), np.eye(3), joint_pos, np.zeros(6), joint_vel)
    out = []
    for f in frames:
        pf, Rf, vel, _ = F.frame_state(model, K, int(f))
        out.append((pf, Rf, vel[:3], vel[3:]))
    return out


def choose_fixed(f, on, sw):
    """Step 4's rule: f while it is on, else the slot on with the greatest switch_time (lowest among equals)."""
    if on[f]:
        return f
    best = -1
    for c in range(len(on)):
        if on[c] and (best < 0 or sw[c] > sw[best]):
            best = c
    return best if best >= 0 else f


def advance_one(model, frames, params, time, joint_pos, joint_vel, force, state, timers, fixed, fixed_pose):
    """T steps of one robot: joint_pos, joint_vel [T, n] (joint_vel may be None), force [T, K], state [K],
    timers [K, 2], fixed (a slot), fixed_pose [12].  Returns a dict of the outputs (base_pos [T, 3], base_rot
    [T, 3, 3], base_vel [T, 6], contact [T, K], fixed_out [T], status) and of the final state arrays
    (trig_state, trig_timers, fixed_frame, fixed_pose)."""
    T, K = np.asarray(force).shape
    n = model["n"]
    prm = np.broadcast_to(np.asarray(params, dtype=np.float64), (K, 4))
    state, timers = np.array(state, dtype=np.int32), np.array(timers, dtype=np.float64)
    fp = np.array(fixed_pose, dtype=np.float64)
    f = int(fixed)
    o = dict(base_pos=np.full((T, 3), np.nan), base_rot=np.full((T, 3, 3), np.nan), base_vel=np.full((T, 6), np.nan),
             contact=np.zeros((T, K), dtype=np.int32), fixed_out=np.full(T, -1, dtype=np.int32))
    frames_ok = all(0 <= int(x) < len(model["frame_link"]) for x in frames)
    bad = not frames_ok
    for t in range(T):
        for c in range(K):
            state[c], timers[c, 0], timers[c, 1] = trigger_step(prm[c], time[t], force[t, c], int(state[c]),
                                                                timers[c, 0], timers[c, 1])
        o["contact"][t] = state & 1
        q = np.asarray(joint_pos[t], dtype=np.float64)
        qd = np.zeros(n) if joint_vel is None else np.asarray(joint_vel[t], dtype=np.float64)
        bad = bad or not (np.isfinite(q).all() and np.isfinite(qd).all() and np.isfinite(fp).all()
                          and 0 <= f < K)
        if not bad:
            with np.errstate(invalid="ignore"):
                rel = relative_frames(model, frames, q, qd)
                pf, Rf, _, _ = rel[f]
                RB = fp[3:].reshape(3, 3) @ Rf.T
                pB = fp[:3] - RB @ pf
                f2 = choose_fixed(f, state & 1, timers[:, 1])
                pg, Rg, vg, wg = rel[f2]
                wB = -(RB @ wg)
                vB = -(RB @ vg) - np.cross(wB, RB @ pg)
            bad = not (np.isfinite(pB).all() and np.isfinite(RB).all() and np.isfinite(vB).all()
                       and np.isfinite(wB).all())
        if bad:
            fp[:] = np.nan
            continue
        if f2 != f:
            fp = np.concatenate([pB + RB @ pg, (RB @ Rg).reshape(-1)])
            f = f2
        o["base_pos"][t], o["base_rot"][t], o["base_vel"][t] = pB, RB, np.concatenate([vB, wB])
        o["fixed_out"][t] = f
    o.update(status=BAD_INPUT if bad else OK, trig_state=state, trig_timers=timers, fixed_frame=f, fixed_pose=fp)
    return o


def advance(model, frames, params, time, joint_pos, joint_vel, force, state, timers, fixed, fixed_pose):
    """The batch: joint_pos [T, B, n], force [T, B, K], state [B, K], timers [B, K, 2], fixed [B], fixed_pose
    [B, 12].  Returns advance_one's dict with the robots stacked on axis 1 (outputs) or 0 (state, status)."""
    B = np.asarray(joint_pos).shape[1]
    runs = [advance_one(model, frames, params, time, np.asarray(joint_pos)[:, b],
                        None if joint_vel is None else np.asarray(joint_vel)[:, b], np.asarray(force)[:, b], state[b],
                        timers[b], fixed[b], fixed_pose[b]) for b in range(B)]
    out = {}
    for k in ("base_pos", "base_rot", "base_vel", "contact", "fixed_out"):
        out[k] = np.stack([r[k] for r in runs], axis=1)
    for k in ("status", "trig_state", "trig_timers", "fixed_frame", "fixed_pose"):
        out[k] = np.stack([np.asarray(r[k]) for r in runs], axis=0)
    out["status"], out["fixed_frame"] = out["status"].astype(np.int32), out["fixed_frame"].astype(np.int32)
    return out


def initial_fixed_pose(model, state, frame):
    """fixed_pose of a robot whose true one-robot `state` is known: that frame's world transform."""
    K = F.kinematics(model, state["base_pos"], state["base_rot"], state["joint_pos"], np.zeros(6),
                     np.zeros(model["n"]))
    pf, Rf, _, _ = F.frame_state(model, K, int(frame))
    return np.concatenate([pf, Rf.reshape(-1)])
