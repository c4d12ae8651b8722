"""Numpy restatement of include/blf/blf_c.h section 11 (blf_swing_foot_eval / blf_so3_eval), in its
arithmetic order, vectorised over the batch only.  The translation goes through the oracle's
quintic_fit / quintic_eval on section 11's knots, so it is bit-exact by construction against the
unchanged oracle; Log and Exp are restated here (numpy's sin / atan2 may differ from the device's
in the last bits: the tests compare rotations at 1e-9)."""
import numpy as np

import oracle as O


def rz(yaw):
    yaw = np.asarray(yaw, dtype=np.float64)
    c, s = np.cos(yaw), np.sin(yaw)
    z, o = np.zeros_like(c), np.ones_like(c)
    return np.stack([c, -s, z, s, c, z, z, z, o], axis=-1).reshape(yaw.shape + (3, 3))


def axis_angle(axis, angle):
    """Rodrigues' formula in the textbook form (test inputs; not the formula under test)."""
    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def log_rel(Rb, Ra):
    """Unit axis u [..., 3] and angle theta [...] of Rb Ra^T ([..., 3, 3] each); u = 0, theta = 0
    where nv == 0."""
    Ra, Rb = np.asarray(Ra, dtype=np.float64), np.asarray(Rb, dtype=np.float64)
    E = np.empty(np.broadcast(Ra, Rb).shape)
    for i in range(3):
        for j in range(3):
            E[..., i, j] = (Rb[..., i, 0] * Ra[..., j, 0] + Rb[..., i, 1] * Ra[..., j, 1]) + \
                Rb[..., i, 2] * Ra[..., j, 2]
    e = lambda i, j: E[..., i, j]   # noqa: E731
    tr = (e(0, 0) + e(1, 1)) + e(2, 2)
    b0 = (tr >= e(0, 0)) & (tr >= e(1, 1)) & (tr >= e(2, 2))
    b1 = ~b0 & (e(0, 0) >= e(1, 1)) & (e(0, 0) >= e(2, 2))
    b2 = ~b0 & ~b1 & (e(1, 1) >= e(2, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        g0 = 2.0 * np.sqrt(1.0 + tr)
        g1 = 2.0 * np.sqrt(((1.0 + e(0, 0)) - e(1, 1)) - e(2, 2))
        g2 = 2.0 * np.sqrt(((1.0 + e(1, 1)) - e(0, 0)) - e(2, 2))
        g3 = 2.0 * np.sqrt(((1.0 + e(2, 2)) - e(0, 0)) - e(1, 1))
        q0 = (0.25 * g0, (e(2, 1) - e(1, 2)) / g0, (e(0, 2) - e(2, 0)) / g0, (e(1, 0) - e(0, 1)) / g0)
        q1 = ((e(2, 1) - e(1, 2)) / g1, 0.25 * g1, (e(0, 1) + e(1, 0)) / g1, (e(0, 2) + e(2, 0)) / g1)
        q2 = ((e(0, 2) - e(2, 0)) / g2, (e(0, 1) + e(1, 0)) / g2, 0.25 * g2, (e(1, 2) + e(2, 1)) / g2)
        q3 = ((e(1, 0) - e(0, 1)) / g3, (e(0, 2) + e(2, 0)) / g3, (e(1, 2) + e(2, 1)) / g3, 0.25 * g3)
    q = [np.where(b0, q0[k], np.where(b1, q1[k], np.where(b2, q2[k], q3[k]))) for k in range(4)]
    neg = q[0] < 0.0
    w, x, y, z = [np.where(neg, -c, c) for c in q]
    nv = np.sqrt((x * x + y * y) + z * z)
    zero = nv == 0.0
    safe = np.where(zero, 1.0, nv)
    theta = np.where(zero, 0.0, 2.0 * np.arctan2(nv, w))
    u = np.stack([np.where(zero, 0.0, c / safe) for c in (x, y, z)], axis=-1)
    return u, theta


def min_jerk(tau, T):
    s = ((tau * tau) * tau) * (10.0 + tau * (-15.0 + 6.0 * tau))
    sd = ((tau * tau) * (30.0 + tau * (-60.0 + 30.0 * tau))) / T
    sdd = (tau * (60.0 + tau * (-180.0 + 120.0 * tau))) / (T * T)
    return s, sd, sdd


def exp_apply(a, u, Ra):
    """Exp(a u) Ra; a [...], u [..., 3], Ra [..., 3, 3]."""
    sa = np.sin(a)
    sh = np.sin(0.5 * a)
    cv = 2.0 * (sh * sh)
    u0, u1, u2 = u[..., 0], u[..., 1], u[..., 2]
    M = np.empty(np.shape(a) + (3, 3))
    M[..., 0, 0] = 1.0 + cv * (u0 * u0 - 1.0)
    M[..., 1, 1] = 1.0 + cv * (u1 * u1 - 1.0)
    M[..., 2, 2] = 1.0 + cv * (u2 * u2 - 1.0)
    M[..., 0, 1] = sa * (-u2) + cv * (u0 * u1)
    M[..., 0, 2] = sa * u1 + cv * (u0 * u2)
    M[..., 1, 0] = sa * u2 + cv * (u1 * u0)
    M[..., 1, 2] = sa * (-u0) + cv * (u1 * u2)
    M[..., 2, 0] = sa * (-u1) + cv * (u2 * u0)
    M[..., 2, 1] = sa * u0 + cv * (u2 * u1)
    R = np.empty_like(M)
    for i in range(3):
        for j in range(3):
            R[..., i, j] = (M[..., i, 0] * Ra[..., 0, j] + M[..., i, 1] * Ra[..., 1, j]) + \
                M[..., i, 2] * Ra[..., 2, j]
    return R


def rotation(Ra, Rb, tau, T):
    """R(t) [..., 3, 3], omega [..., 3], alpha [..., 3] of the minimum-jerk geodesic Ra -> Rb."""
    u, theta = log_rel(Rb, Ra)
    s, sd, sdd = min_jerk(tau, T)
    R = exp_apply(s * theta, u, Ra)
    hold = np.broadcast_to((theta == 0.0)[..., None, None], R.shape)
    R = np.where(hold, np.broadcast_to(Ra, R.shape), R)   # nv == 0: R_a bit for bit
    phi = theta[..., None] * u
    return R, sd[..., None] * phi, sdd[..., None] * phi


def swing_knots(pa, pb, t0, t1, step_height, apex_ratio, v_land, a_land):
    """knots_t [3], knots_pva [3, 3, 3] of one swing (section 11)."""
    rho, T = apex_ratio, t1 - t0
    kt = np.array([t0, (1.0 - rho) * t0 + rho * t1, t1])
    pva = np.zeros((3, 3, 3))
    pva[0, 0] = pa
    pva[1, 0, :2] = (1.0 - rho) * pa[:2] + rho * pb[:2]
    pva[1, 0, 2] = max(pa[2], pb[2]) + step_height
    pva[1, 1, :2] = (pb[:2] - pa[:2]) / T
    pva[2, 0] = pb
    pva[2, 1, 2] = v_land
    pva[2, 2, 2] = a_land
    return kt, pva


def swing_foot_eval(contact_pose, contact_time, ncontacts, tq, step_height=0.05, apex_ratio=0.5,
                    landing_velocity=0.0, landing_acceleration=0.0):
    """contact_pose [L, C, 12], contact_time [L, C, 2], ncontacts [L], tq [L, Q] -> dict of pose
    [L, Q, 12], twist, accel [L, Q, 6], contact_idx, in_contact [L, Q] int32 and (not a device
    output) swing [L, Q] bool: the queries in a swing."""
    cp = np.asarray(contact_pose, dtype=np.float64)
    ct = np.asarray(contact_time, dtype=np.float64)
    tq = np.asarray(tq, dtype=np.float64)
    L, C = cp.shape[:2]
    Q = tq.shape[1]
    pose = np.zeros((L, Q, 12))
    twist = np.zeros((L, Q, 6))
    accel = np.zeros((L, Q, 6))
    idx = np.full((L, Q), -1, dtype=np.int32)
    inc = np.zeros((L, Q), dtype=np.int32)
    swing = np.zeros((L, Q), dtype=bool)
    for l in range(L):
        n = int(ncontacts[l])
        ok = 1 <= n <= C
        if ok:
            ok = bool(np.isfinite(cp[l, :n]).all() and np.isfinite(ct[l, :n]).all())
        fits = {}
        for q in range(Q):
            t = tq[l, q]
            if not ok or not np.isfinite(t):
                pose[l, q], twist[l, q], accel[l, q] = np.nan, np.nan, np.nan
                continue
            raw = -1
            for c in range(n):
                if ct[l, c, 0] <= t:
                    raw = c
            idx[l, q] = raw
            if raw < 0:
                pose[l, q] = cp[l, 0]
            elif t < ct[l, raw, 1]:
                pose[l, q] = cp[l, raw]
                inc[l, q] = 1
            elif raw == n - 1:
                pose[l, q] = cp[l, raw]
            else:
                swing[l, q] = True
                t0, t1 = ct[l, raw, 1], ct[l, raw + 1, 0]
                pa, pb = cp[l, raw], cp[l, raw + 1]
                if raw not in fits:
                    kt, pva = swing_knots(pa[:3], pb[:3], t0, t1, step_height, apex_ratio,
                                          landing_velocity, landing_acceleration)
                    fits[raw] = (kt, O.quintic_fit(kt, pva))
                kt, coeffs = fits[raw]
                out, _ = O.quintic_eval(kt, coeffs, np.array([t]))
                pose[l, q, :3], twist[l, q, :3], accel[l, q, :3] = out[0, 0], out[0, 1], out[0, 2]
                T = t1 - t0
                tau = (t - t0) / T
                R, w, al = rotation(pa[3:].reshape(3, 3), pb[3:].reshape(3, 3), np.float64(tau),
                                    np.float64(T))
                pose[l, q, 3:], twist[l, q, 3:], accel[l, q, 3:] = R.reshape(9), w, al
    return dict(pose=pose, twist=twist, accel=accel, contact_idx=idx, in_contact=inc, swing=swing)


def so3_eval(R0, R1, duration, tq):
    """R0, R1 [S, 3, 3], duration [S], tq [S, Q] -> rot [S, Q, 9], omega, alpha [S, Q, 3]."""
    R0 = np.asarray(R0, dtype=np.float64).reshape(-1, 1, 3, 3)
    R1 = np.asarray(R1, dtype=np.float64).reshape(-1, 1, 3, 3)
    T = np.asarray(duration, dtype=np.float64)[:, None]
    tq = np.asarray(tq, dtype=np.float64)
    bad = ~(np.isfinite(T) & (T > 0.0)) | ~np.isfinite(tq) | \
        ~np.isfinite(R0).all(axis=(2, 3)) | ~np.isfinite(R1).all(axis=(2, 3))
    Ts = np.where(bad, 1.0, T) * np.ones_like(tq)
    tc = np.where(tq < 0.0, 0.0, np.where(tq > Ts, Ts, tq))
    with np.errstate(invalid="ignore"):
        R, w, al = rotation(np.where(np.isfinite(R0), R0, 0.0), np.where(np.isfinite(R1), R1, 0.0),
                            np.where(bad, 0.0, tc / Ts), Ts)
    R = R.reshape(tq.shape + (9,)).copy()
    w, al = w.copy(), al.copy()
    R[bad], w[bad], al[bad] = np.nan, np.nan, np.nan
    return dict(rot=R, omega=w, alpha=al)
