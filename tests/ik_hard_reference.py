"""TEST INFRASTRUCTURE ONLY -- numpy restatement of include/blf/blf_c.h section 12b (whole-body IK
with hard, priority-0, task rows) for one robot, the checker of blf_fb_ik_solve_hard /
blf_fb_ik_integrate_hard.  Built on tests/ik_reference.py (the task rows, H and g of section 12).

Two solves of the same problem, by different algorithms:
  solve()    the reference: the dense KKT system [[H_soft, A_h^T], [A_h, 0]] (nu, mu) = (g_soft, b_h)
             through fb_models.refined_solve (LU with long-double refinement), H_soft and g_soft
             WITHOUT the hard rows; the status from the singular values of A_h.
  project()  the device's method in plain float64: H and g with the hard rows, H = L L^T,
             Y = L^-1 A_h^T, S = Y^T Y factorized with the relative pivot rule, lambda, nu.

A mask is section 12b's `rows` word: bit 6k + a row a of SE3 task k, bits 24..26 the CoM rows."""
import numpy as np

import fb_models as FM
import ik_reference as IK
import oracle as O

OK, NOT_POSITIVE, BAD_INPUT, HARD_DEPENDENT = 0, 1, 2, 3
TAU = 1.0e-8
# A_h counts as rank deficient when sigma_min <= SV_REL * sigma_max: the dependent cases of
# tests/ik_hard_cases.py repeat rows exactly (1e-16), the well-posed ones are above 1e-3
SV_REL = 1.0e-9


def mask(se3=(), com=(False, False, False)):
    """The `rows` word of se3 [K][6] bools and com [3] bools (native.Handle.ik_hard's arguments)."""
    rows = 0
    for k, r in enumerate(se3):
        for a, on in enumerate(r):
            rows |= int(bool(on)) << (6 * k + a)
    for a, on in enumerate(com):
        rows |= int(bool(on)) << (24 + a)
    return rows


def slots(tasks, rows):
    """Indices of the hard rows in ik_reference.rows()'s stacking (SE3 rows, then the CoM's)."""
    K = len(tasks["frame"])
    out = [r for r in range(6 * K) if (rows >> r) & 1]
    out += [6 * K + a for a in range(3) if (rows >> (24 + a)) & 1]
    return out


def scale_hard_weights(tasks, rows, factor):
    """The task set with the weights of the hard rows multiplied by `factor`."""
    w = np.array(tasks["se3_weight"], dtype=np.float64, copy=True)
    for r in range(w.size):
        if (rows >> r) & 1:
            w[r // 6, r % 6] *= factor
    out = dict(tasks, se3_weight=w)
    if tasks.get("com_weight") is not None:
        cw = np.array(tasks["com_weight"], dtype=np.float64, copy=True)
        for a in range(3):
            if (rows >> (24 + a)) & 1:
                cw[a] *= factor
        out["com_weight"] = cw
    return out


def parts(model, s, t, rows):
    """One robot (t: ik_reference.one()): H, g of section 12 (hard rows included), H_soft, g_soft
    (without them), A_h and b_h."""
    n = model["n"]
    A, w, v = IK.rows(model, s, t)
    hs = slots(t, rows)
    H, g = IK.system(model, s, t)
    ws = w.copy()
    ws[hs] = 0.0
    jv = t["joint_vel"] if t.get("joint_vel") is not None else np.zeros(n)
    sd = jv + np.asarray(t["joint_kp"]) * (t["joint_pos"] - s["joint_pos"])
    jw = np.asarray(t["joint_weight"], dtype=np.float64)
    Hs = A.T @ (ws[:, None] * A) + np.diag(np.concatenate([np.full(6, float(t["base_damping"])), jw]))
    gs = A.T @ (ws * v) + np.concatenate([np.zeros(6), jw * sd])
    return H, g, Hs, gs, A[hs], v[hs]


def pivots(S, tau=TAU):
    """Cholesky of S with section 12b's rule: (C or None, the relative pivots d_i / S_ii up to and
    including the first that fails)."""
    m = S.shape[0]
    C = np.zeros((m, m))
    W = S.copy()
    rel = []
    for i in range(m):
        d, d0 = W[i, i], S[i, i]
        rel.append(d / d0 if d0 != 0.0 else -np.inf)
        if not (d > tau * d0 and np.isfinite(d)):
            return None, np.array(rel)
        C[i:, i] = W[i:, i] / np.sqrt(d)
        W[i + 1:, i + 1:] -= np.outer(C[i + 1:, i], C[i + 1:, i])
    return C, np.array(rel)


def project(H, g, Ah, bh, tau=TAU):
    """The device's method (section 12b steps 2-4) in plain float64: (nu, status, relative pivots)."""
    NV = H.shape[0]
    nan = np.full(NV, np.nan)
    try:
        L = np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return nan, NOT_POSITIVE, np.zeros(0)
    z = np.linalg.solve(L, g)
    if Ah.shape[0] == 0:
        return np.linalg.solve(L.T, z), OK, np.zeros(0)
    if Ah.shape[0] > NV:
        return nan, HARD_DEPENDENT, np.zeros(0)
    Y = np.linalg.solve(L, Ah.T)
    S = Y.T @ Y
    C, rel = pivots(S, tau)
    if C is None:
        return nan, HARD_DEPENDENT, rel
    lam = np.linalg.solve(C.T, np.linalg.solve(C, Y.T @ z - bh))
    return np.linalg.solve(L.T, z - Y @ lam), OK, rel


def solve(model, states, tasks, rows, i):
    """blf_fb_ik_solve_hard of robot i: (nu [6+n], status, parts() tuple or None for BAD_INPUT)."""
    n = model["n"]
    s = {k: np.asarray(states[k][i], dtype=np.float64) for k in IK.STATE_KEYS}
    t = IK.one(tasks, i)
    nan = np.full(6 + n, np.nan)
    if IK.bad_input(model, s, t):
        return nan, BAD_INPUT, None
    with np.errstate(all="ignore"):
        P = parts(model, s, t, rows)
        H, g, Hs, gs, Ah, bh = P
        try:
            L = np.linalg.cholesky(H)
            if not np.isfinite(L).all():
                raise np.linalg.LinAlgError
        except np.linalg.LinAlgError:
            return nan, NOT_POSITIVE, P
        m = Ah.shape[0]
        if m == 0:
            return np.asarray(FM.refined_solve(H, g), dtype=np.float64), OK, P
        if m > 6 + n:
            return nan, HARD_DEPENDENT, P
        sv = np.linalg.svd(Ah, compute_uv=False)
        if sv[-1] <= SV_REL * sv[0]:
            return nan, HARD_DEPENDENT, P
        KKT = np.block([[Hs, Ah.T], [Ah, np.zeros((m, m))]])
        x = FM.refined_solve(KKT, np.concatenate([gs, bh]))
    return np.asarray(x[:6 + n], dtype=np.float64), OK, P


def integrate(model, states, tasks, rows, i, steps, dT, rho=0.01):
    """blf_fb_ik_integrate_hard of robot i, as ik_reference.integrate: (state dict, last nu, status)."""
    n = model["n"]
    s = {k: np.array(states[k][i], dtype=np.float64) for k in IK.STATE_KEYS}
    nu, status = np.full(6 + n, np.nan), OK
    for _ in range(steps):
        one_state = {k: v[None] for k, v in s.items()}
        nu, status, _ = solve(model, one_state, IK.tasks_at(tasks, i), rows, 0)
        if status != OK:
            break
        st, p, R, q = O.fbk_euler_integrate(rho, s["base_pos"], s["base_rot"], s["joint_pos"], nu[:6], nu[6:],
                                            0.0, dT, dT)
        assert st == 0
        s = dict(base_pos=p, base_rot=R, joint_pos=q)
    return dict(s, base_vel=nu[:6].copy(), joint_vel=nu[6:].copy()), nu, status


def integrate_projection(model, states, tasks, rows, i, steps, dT, rho=0.01):
    """integrate() with project() in place of the KKT solve (plain float64 throughout): the state
    dict.  How far it lands from integrate() is the accuracy of the reference trajectory itself."""
    s = {k: np.array(states[k][i], dtype=np.float64) for k in IK.STATE_KEYS}
    t = IK.one(tasks, i)
    nu = np.full(6 + model["n"], np.nan)
    for _ in range(steps):
        H, g, _, _, Ah, bh = parts(model, s, t, rows)
        nu, status, _ = project(H, g, Ah, bh)
        assert status == OK
        st, p, R, q = O.fbk_euler_integrate(rho, s["base_pos"], s["base_rot"], s["joint_pos"], nu[:6], nu[6:],
                                            0.0, dT, dT)
        assert st == 0
        s = dict(base_pos=p, base_rot=R, joint_pos=q)
    return dict(s, base_vel=nu[:6].copy(), joint_vel=nu[6:].copy())
