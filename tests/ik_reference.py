"""TEST INFRASTRUCTURE ONLY -- numpy restatement of include/blf/blf_c.h section 12 (whole-body
inverse kinematics: SE3, CoM and joint-tracking tasks at priority 1, H nu = g) for one robot, the
checker of blf_fb_ik_solve / blf_fb_ik_integrate.  Built on oracle/fb_dynamics.py (kinematics,
frame_state, point_jacobian, ancestors); Log is tests/swing_foot_reference.py's; the solve is
fb_models.refined_solve; the Euler step is the oracle's fbk_euler_integrate.

A task set is a dict of host arrays with the fields of blf_ik_tasks:
  frame [K] int32, se3_weight [K,6], se3_kp [K,2], se3_pose [B,K,12], se3_twist [B,K,6] or None,
  com_weight [3] or None, com_kp, com_pos [B,3], com_vel [B,3] or None,
  joint_weight [n], joint_kp [n], joint_pos [B,n], joint_vel [B,n] or None, base_damping."""
import numpy as np

import fb_dynamics as F
import fb_models as FM
import oracle as O
import swing_foot_reference as SR

OK, NOT_POSITIVE, BAD_INPUT = 0, 1, 2
STATE_KEYS = ("base_pos", "base_rot", "joint_pos")


def kin(model, s):
    """Kinematics at (base_pos, base_rot, joint_pos) of the one-robot state s, zero velocities."""
    n = model["n"]
    return F.kinematics(model, s["base_pos"], s["base_rot"], s["joint_pos"], np.zeros(6), np.zeros(n))


def com(model, K):
    """Centre of mass c and total mass m."""
    cl = K["p"] + np.einsum("lab,lb->la", K["R"], np.asarray(model["link_com"]))
    m = np.asarray(model["link_mass"], dtype=np.float64)
    return (m[:, None] * cl).sum(axis=0) / m.sum(), m.sum()


def com_jacobian(model, K):
    """J_c = (1/m) sum_l m_l J_lin,l(c_l), 3 x (6+n)."""
    anc = F.ancestors(model)
    n = model["n"]
    J = np.zeros((3, 6 + n))
    mt = 0.0
    for l in range(n + 1):
        c = K["p"][l] + K["R"][l] @ model["link_com"][l]
        J += model["link_mass"][l] * F.point_jacobian(model, K, anc, l, c)[:3]
        mt += model["link_mass"][l]
    return J / mt


def log3(Rdes, R):
    """Log(R_des R^T) = theta u."""
    u, th = SR.log_rel(Rdes, R)
    return th * u


def one(tasks, i):
    """The task set with robot i's set points (the batch axis removed)."""
    out = dict(tasks)
    for k in ("se3_pose", "se3_twist", "com_pos", "com_vel", "joint_pos", "joint_vel"):
        if tasks.get(k) is not None:
            out[k] = np.asarray(tasks[k], dtype=np.float64)[i]
    return out


def rows(model, s, t):
    """The stacked task rows A [M, 6+n], their weights w [M] and targets v [M] of one robot (t: one())
    in the order of section 12: SE3 task 0 (linear xyz, angular xyz), ..., then the CoM rows."""
    K = kin(model, s)
    A, w, v = [], [], []
    for k, f in enumerate(np.asarray(t["frame"], dtype=np.int64)):
        pf, Rf, _, J = F.frame_state(model, K, int(f))
        des = t["se3_pose"][k]
        ff = t["se3_twist"][k] if t.get("se3_twist") is not None else np.zeros(6)
        kpl, kpa = t["se3_kp"][k]
        A.append(J)
        w.append(np.asarray(t["se3_weight"][k], dtype=np.float64))
        v.append(np.concatenate([ff[:3] + kpl * (des[:3] - pf),
                                 ff[3:] + kpa * log3(des[3:].reshape(3, 3), Rf)]))
    if t.get("com_weight") is not None:
        c, _ = com(model, K)
        cv = t["com_vel"] if t.get("com_vel") is not None else np.zeros(3)
        A.append(com_jacobian(model, K))
        w.append(np.asarray(t["com_weight"], dtype=np.float64))
        v.append(cv + t["com_kp"] * (t["com_pos"] - c))
    n = model["n"]
    if not A:
        return np.zeros((0, 6 + n)), np.zeros(0), np.zeros(0)
    return np.vstack(A), np.concatenate(w), np.concatenate(v)


def system(model, s, t):
    """(H, g) of one robot."""
    n = model["n"]
    A, w, v = rows(model, s, t)
    jv = t["joint_vel"] if t.get("joint_vel") is not None else np.zeros(n)
    sd = jv + np.asarray(t["joint_kp"]) * (t["joint_pos"] - s["joint_pos"])
    jw = np.asarray(t["joint_weight"], dtype=np.float64)
    H = A.T @ (w[:, None] * A) + np.diag(np.concatenate([np.full(6, float(t["base_damping"])), jw]))
    g = A.T @ (w * v) + np.concatenate([np.zeros(6), jw * sd])
    return H, g


def bad_input(model, s, t):
    fr = np.asarray(t["frame"], dtype=np.int64)
    if ((fr < 0) | (fr >= len(model["frame_link"]))).any():
        return True
    vals = [s[k] for k in STATE_KEYS] + [t["joint_pos"]]
    vals += [t[k] for k in ("se3_twist", "com_vel", "joint_vel") if t.get(k) is not None]
    if len(fr):
        vals.append(t["se3_pose"])
    if t.get("com_weight") is not None:
        vals.append(t["com_pos"])
    return not all(np.isfinite(np.asarray(x, dtype=np.float64)).all() for x in vals)


def solve(model, states, tasks, i):
    """blf_fb_ik_solve of robot i: (nu [6+n], status, H, g); H, g None for BAD_INPUT."""
    n = model["n"]
    s = {k: np.asarray(states[k][i], dtype=np.float64) for k in STATE_KEYS}
    t = one(tasks, i)
    nan = np.full(6 + n, np.nan)
    if bad_input(model, s, t):
        return nan, BAD_INPUT, None, None
    with np.errstate(all="ignore"):
        H, g = system(model, s, t)
        try:
            L = np.linalg.cholesky(H)
            if not np.isfinite(L).all():
                raise np.linalg.LinAlgError
        except np.linalg.LinAlgError:
            return nan, NOT_POSITIVE, H, g
    return np.asarray(FM.refined_solve(H, g), dtype=np.float64), OK, H, g


def cholesky_solve(H, g):
    """The plain float64 Cholesky solve (the conditioning guard's other side)."""
    L = np.linalg.cholesky(H)
    return np.linalg.solve(L.T, np.linalg.solve(L, g))


def integrate(model, states, tasks, i, steps, dT, rho=0.01):
    """blf_fb_ik_integrate of robot i: (state dict with all five keys, nu of the last step, status)."""
    n = model["n"]
    s = {k: np.array(states[k][i], dtype=np.float64) for k in STATE_KEYS}
    nu, status = np.full(6 + n, np.nan), OK
    for _ in range(steps):
        one_state = {k: v[None] for k, v in s.items()}
        nu, status, _, _ = solve(model, one_state, tasks_at(tasks, i), 0)
        if status != OK:
            break
        st, p, R, q = O.fbk_euler_integrate(rho, s["base_pos"], s["base_rot"], s["joint_pos"], nu[:6], nu[6:],
                                            0.0, dT, dT)
        assert st == 0
        s = dict(base_pos=p, base_rot=R, joint_pos=q)
    return dict(s, base_vel=nu[:6].copy(), joint_vel=nu[6:].copy()), nu, status


def tasks_rows(tasks, rows):
    """The task set of the robots `rows` (a slice) of the batch."""
    out = dict(tasks)
    for k in ("se3_pose", "se3_twist", "com_pos", "com_vel", "joint_pos", "joint_vel"):
        if tasks.get(k) is not None:
            out[k] = np.asarray(tasks[k], dtype=np.float64)[rows]
    return out


def tasks_at(tasks, i):
    """The task set of the one-robot batch [i:i+1]."""
    return tasks_rows(tasks, slice(i, i + 1))
