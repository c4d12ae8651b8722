"""TEST INFRASTRUCTURE ONLY -- numpy restatement of include/blf/blf_c.h section 12c (whole-body IK with
a box on the joint velocities) for one robot, the checker of blf_fb_ik_solve_limits /
blf_fb_ik_integrate_limits.  Built on tests/ik_hard_reference.py (parts(): H, g, H_soft, g_soft, A_h, b_h).

  active_set()  the rule of section 12c in plain float64: the working set, the modes and the counters
                exactly as the header states them, each equality problem by eliminating the held joints
                and running section 12b's projection on what is left.  It also records, per iteration,
                how far every comparison the rule makes is from a tie (the conditioning band).
  certify()     an independent certificate of a final working set: the dense KKT system
                [[H_soft, A_h^T, E^T], [A_h, 0, 0], [E, 0, 0]] through fb_models.refined_solve (LU with
                long-double refinement), accepted only if the solution is inside the box and every
                multiplier of a held joint has the sign of its bound.  H_soft is positive definite on
                the feasible set, so a certified point is THE solution, whatever route found the set.
  feasible()    whether { A_h nu = b_h, lo <= s_dot <= up } is non-empty, by scipy.optimize.linprog.

A limits dict: pos_lower, pos_upper, klim [n], vel_max [n] or None, sampling_time, max_iter (0: default)."""
import numpy as np

import fb_models as FM
import ik_hard_reference as HR
import ik_reference as IK
import oracle as O

OK, NOT_POSITIVE, BAD_INPUT, HARD_DEPENDENT, LIMITS_UNRESOLVED = 0, 1, 2, 3, 4
DEFAULT_MAX_ITER = 32   # BLF_IK_LIMITS_DEFAULT_MAX_ITER
STALL = 8               # iterations without a new minimum that end block mode
BAND = 1.0e-7           # every comparison of an OK case is at least this far (relative) from a tie


def box(lim, s):
    """(lo, up) of section 12c at the joint positions s, in the header's order of operations."""
    kl, T = np.asarray(lim["klim"], dtype=np.float64), float(lim["sampling_time"])
    with np.errstate(all="ignore"):
        lo = kl * (np.asarray(lim["pos_lower"], dtype=np.float64) - s) / T
        up = kl * (np.asarray(lim["pos_upper"], dtype=np.float64) - s) / T
    if lim.get("vel_max") is not None:
        vm = np.asarray(lim["vel_max"], dtype=np.float64)
        lo, up = np.minimum(np.maximum(lo, -vm), vm), np.minimum(np.maximum(up, -vm), vm)
    return lo, up


def no_limits(n, sampling_time=0.01):
    """The limits dict that bounds nothing."""
    return dict(pos_lower=np.full(n, -np.inf), pos_upper=np.full(n, np.inf), klim=np.ones(n), vel_max=None,
                sampling_time=sampling_time, max_iter=0)


def equality_solve(P, side, lo, up, tau=HR.TAU):
    """One iteration's equality problem: joints with side -1 / +1 held at lo / up.  The held joints
    are eliminated from H, g and the hard rows (a held row of H becomes e_i), then section 12b's
    projection runs: (nu, lambda, pivot_ok, relative pivots of S)."""
    H, g, _, _, Ah, bh = P
    NV = H.shape[0]
    held = np.flatnonzero(side != 0)
    val = np.where(side < 0, lo, up)[held]
    Hm, gm, Am, bm = H.copy(), g.copy(), Ah.copy(), bh.copy()
    c = 6 + held
    gm -= H[:, c] @ val
    Hm[:, c] = 0.0
    Hm[c, :] = 0.0
    Hm[c, c] = 1.0
    gm[c] = val
    bm = bm - Ah[:, c] @ val
    Am[:, c] = 0.0
    L = np.linalg.cholesky(Hm)
    z = np.linalg.solve(L, gm)
    m = Am.shape[0]
    if m == 0:
        return np.linalg.solve(L.T, z), np.zeros(0), True, np.zeros(0)
    if m > NV:
        return np.full(NV, np.nan), np.zeros(m), False, np.zeros(0)
    Y = np.linalg.solve(L, Am.T)
    C, rel = HR.pivots(Y.T @ Y, tau)
    if C is None:
        return np.full(NV, np.nan), np.zeros(m), False, rel
    lam = np.linalg.solve(C.T, np.linalg.solve(C, Y.T @ z - bm))
    return np.linalg.solve(L.T, z - Y @ lam), lam, True, rel


def masks(side):
    """(word 0, word 1) of `active`: the joints held at their lower / upper bound."""
    wl = sum(1 << int(j) for j in np.flatnonzero(side < 0))
    wu = sum(1 << int(j) for j in np.flatnonzero(side > 0))
    return wl, wu


def active_set(P, lo, up, max_iter=0, tau=HR.TAU):
    """Section 12c's rule on parts() P with the box (lo, up): dict(nu, status, iters, side (-1 / 0 /
    +1 per joint), active (two masks), left_block, margin (the smallest relative distance from a tie
    over every comparison made), pivots (every relative pivot of S met, with whether its solve passed))."""
    H, g, Hs, gs, Ah, bh = P
    NV = H.shape[0]
    n = NV - 6
    max_iter = max_iter if max_iter > 0 else DEFAULT_MAX_ITER
    side = np.zeros(n, dtype=np.int64)
    prev = side.copy()
    block, best, stall = True, np.iinfo(np.int64).max, 0
    out = dict(nu=np.full(NV, np.nan), status=LIMITS_UNRESOLVED, iters=0, left_block=False, margin=np.inf,
               pivots=[])
    try:
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return dict(out, status=NOT_POSITIVE, iters=1, side=side, active=(0, 0))
    for it in range(1, max_iter + 1):
        out["iters"] = it
        nu, lam, pok, rel = equality_solve(P, side, lo, up, tau)
        out["pivots"].append((rel, pok))
        if not pok:
            if not side.any():
                out["status"] = HARD_DEPENDENT
                break
            if not block:
                break
            side, block, out["left_block"] = prev.copy(), False, True
            continue
        sd = nu[6:]
        free, scale = side == 0, np.abs(nu).max()
        vl, vu = free & (sd < lo), free & (sd > up)
        for b in (lo, up):   # how far every free joint is from each finite bound
            fin = free & np.isfinite(b)
            if fin.any():
                out["margin"] = min(out["margin"], (np.abs(sd[fin] - b[fin]) / scale).min())
        rl = ru = np.zeros(n, dtype=bool)
        if side.any():
            rho = gs - Hs @ nu - Ah.T @ lam
            size = np.abs(gs) + np.abs(Hs) @ np.abs(nu) + np.abs(Ah.T) @ np.abs(lam)
            held = side != 0
            out["margin"] = min(out["margin"], (np.abs(rho[6:][held]) / size[6:][held]).min())
            rl, ru = (side < 0) & (rho[6:] > 0.0), (side > 0) & (rho[6:] < 0.0)
        ninf = int((vl | vu | rl | ru).sum())
        if ninf == 0:
            out.update(nu=nu, status=OK)
            break
        if it == max_iter:
            break
        if block:
            stall = 0 if ninf < best else stall + 1
            best = min(best, ninf)
            block = stall < STALL
            out["left_block"] = out["left_block"] or not block
        if block:
            prev = side.copy()
            side = np.where(rl | ru, 0, side)
            side = np.where(vl, -1, np.where(vu, 1, side))
        elif (vl | vu).any():
            mag = np.where(vl, lo - sd, np.where(vu, sd - up, -np.inf))
            j = int(np.argmax(mag))
            rest = np.delete(mag, j)
            if rest.size and np.isfinite(rest.max()):
                out["margin"] = min(out["margin"], (mag[j] - rest.max()) / mag[j])
            side[j] = -1 if vl[j] else 1
        else:
            side[int(np.flatnonzero(rl | ru)[0])] = 0
    ok = out["status"] == OK
    return dict(out, side=side, active=masks(side) if ok else (0, 0))


def certify(P, lo, up, side, tol=1.0e-12):
    """The dense KKT solve of the working set `side`: (nu, accepted).  Accepted: inside the box to
    `tol` and every held joint's multiplier of the right sign (E^T gamma = rho: gamma <= 0 at a lower
    bound, >= 0 at an upper one)."""
    _, _, Hs, gs, Ah, bh = P
    NV, m = Hs.shape[0], Ah.shape[0]
    held = np.flatnonzero(side != 0)
    E = np.zeros((held.size, NV))
    E[np.arange(held.size), 6 + held] = 1.0
    val = np.where(side < 0, lo, up)[held]
    A = np.vstack([Ah, E])
    k = A.shape[0]
    KKT = np.block([[Hs, A.T], [A, np.zeros((k, k))]])
    x = np.asarray(FM.refined_solve(KKT, np.concatenate([gs, bh, val])), dtype=np.float64)
    nu, gam = x[:NV], x[NV + m:]
    sd = nu[6:]
    inside = bool(((sd >= lo - tol) & (sd <= up + tol)).all())
    signs = bool((gam * side[held] >= 0.0).all())
    return nu, inside and signs and bool(np.isfinite(x).all())


def feasible(P, lo, up):
    """Whether A_h nu = b_h has a solution with lo <= s_dot <= up (scipy's HiGHS LP, zero objective)."""
    from scipy.optimize import linprog
    Ah, bh = P[4], P[5]
    if Ah.shape[0] == 0:
        return True
    NV = Ah.shape[1]
    bounds = [(None, None)] * 6 + [(None if not np.isfinite(a) else float(a), None if not np.isfinite(b) else float(b))
                                   for a, b in zip(lo, up)]
    res = linprog(np.zeros(NV), A_eq=Ah, b_eq=bh, bounds=bounds, method="highs")
    return res.status == 0


def solve(model, states, tasks, rows, lim, i):
    """blf_fb_ik_solve_limits of robot i: active_set()'s dict, with `parts`, `lo`, `up` (None for a
    BLF_IK_BAD_INPUT robot, whose iters is 0)."""
    n = model["n"]
    s = {k: np.asarray(states[k][i], dtype=np.float64) for k in IK.STATE_KEYS}
    t = IK.one(tasks, i)
    if IK.bad_input(model, s, t):
        return dict(nu=np.full(6 + n, np.nan), status=BAD_INPUT, iters=0, active=(0, 0), parts=None,
                    side=np.zeros(n, dtype=np.int64), margin=np.inf, pivots=[], left_block=False)
    with np.errstate(all="ignore"):
        P = HR.parts(model, s, t, rows)
        lo, up = box(lim, s["joint_pos"])
        return dict(active_set(P, lo, up, int(lim.get("max_iter", 0))), parts=P, lo=lo, up=up)


def integrate(model, states, tasks, rows, lim, i, steps, dT, rho=0.01, certified=False):
    """blf_fb_ik_integrate_limits of robot i: (state dict, last nu, status, summed iters, last masks).
    certified: every step takes certify()'s nu of the rule's final set instead of the rule's own (the
    second route of the trajectory screening)."""
    n = model["n"]
    s = {k: np.array(states[k][i], dtype=np.float64) for k in IK.STATE_KEYS}
    nu, status, iters, act = np.full(6 + n, np.nan), OK, 0, (0, 0)
    for _ in range(steps):
        r = solve(model, {k: v[None] for k, v in s.items()}, IK.tasks_at(tasks, i), rows, lim, 0)
        nu, status, act = r["nu"], r["status"], r["active"]
        iters += r["iters"]
        if status != OK:
            nu = np.full(6 + n, np.nan)
            break
        if certified:
            nu, good = certify(r["parts"], r["lo"], r["up"], r["side"])
            assert good
        st, p, R, q = O.fbk_euler_integrate(rho, s["base_pos"], s["base_rot"], s["joint_pos"], nu[:6], nu[6:],
                                            0.0, dT, dT)
        assert st == 0
        s = dict(base_pos=p, base_rot=R, joint_pos=q)
    return dict(s, base_vel=nu[:6].copy(), joint_vel=nu[6:].copy()), nu, status, iters, act
