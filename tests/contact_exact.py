"""An independent, 50-digit restatement of ContinuousContactModel from its point law.

The model (ContactModels/src/ContinuousContactModel.cpp) is a rectangular sole, L x W, covered by
springs and dampers.  The only thing taken from the reference here is the law of one point of the
sole, getForceAtPoint / getTorqueGeneratedAtPoint (:173-221).  Everything the reference then states
in closed form (:79-171, :223-254: wrench, regressor, control matrix, autonomous dynamics) is derived
from that point law by a quadrature that is exact for it, in mpmath at 50 digits, without
looking at any closed form.  A closed form with a lost factor, a swapped axis or a wrong sign
therefore disagrees with this module in the first digit.

Layout (the one of the C ABI): prm = (L, W, k, b); twist = (v, w), mixed representation;
pose / null = (p, R row-major).  All inputs are doubles and enter the arithmetic exactly.

mpmath is needed only by the functions that compute; `block_err`, `GAUSS_X`, `GAUSS_W` and
`fixture_points` work without it, so the GPU tests can use the metric on the committed fixture."""
import numpy as np

try:
    import mpmath as mp
except ImportError:  # the metric and the point set do not need it
    mp = None

DPS = 50
DIFF_H = "1e-15"
SNAP = "1e-30"

# 3-point Gauss-Legendre rule on [-1, 1] as doubles (the fixture's point set, the GPU tests' sum)
GAUSS_X = np.array([-np.sqrt(0.6), 0.0, np.sqrt(0.6)])
GAUSS_W = np.array([5.0, 8.0, 5.0]) / 9.0


def _mpf(a):
    return [mp.mpf(float(x)) for x in np.asarray(a, dtype=np.float64).reshape(-1)]


def _split(prm, twist, pose, null):
    L, W, k, b = _mpf(prm)
    tw, ps, nl = _mpf(twist), _mpf(pose), _mpf(null)
    R = [ps[3 + 3 * i:6 + 3 * i] for i in range(3)]
    R0 = [nl[3 + 3 * i:6 + 3 * i] for i in range(3)]
    return (L, W, k, b), (tw[:3], tw[3:]), (ps[:3], R), (nl[:3], R0)


def _matvec(M, v):
    return [M[i][0] * v[0] + M[i][1] * v[1] + M[i][2] * v[2] for i in range(3)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _point_force(P, T, X, N, x, y):
    """k ((p0 - p) + (R0 - R) q) - b (v + w x (R q)),  q = (x, y, 0)   (:196-199)."""
    (L, W, k, b), (v, w), (p, R), (p0, R0) = P, T, X, N
    if abs(x) > L / 2 or abs(y) > W / 2:            # :185, the edge itself is inside
        return [mp.mpf(0)] * 3
    q = [x, y, mp.mpf(0)]
    Rq, R0q = _matvec(R, q), _matvec(R0, q)
    wRq = _cross(w, Rq)
    return [k * ((p0[i] - p[i]) + (R0q[i] - Rq[i])) - b * (v[i] + wRq[i]) for i in range(3)]


def _point_torque(P, T, X, N, x, y):
    """(R q) x f(x, y)   (:219)."""
    (L, W, _, _), _, (_, R), _ = P, T, X, N
    if abs(x) > L / 2 or abs(y) > W / 2:            # :207
        return [mp.mpf(0)] * 3
    return _cross(_matvec(R, [x, y, mp.mpf(0)]), _point_force(P, T, X, N, x, y))


def point_force(prm, twist, pose, null, x, y):
    """getForceAtPoint(x, y) as three mpf."""
    with mp.workdps(DPS):
        return _point_force(*_split(prm, twist, pose, null), mp.mpf(float(x)), mp.mpf(float(y)))


def point_torque(prm, twist, pose, null, x, y):
    """getTorqueGeneratedAtPoint(x, y) as three mpf."""
    with mp.workdps(DPS):
        return _point_torque(*_split(prm, twist, pose, null), mp.mpf(float(x)), mp.mpf(float(y)))


def _wrench(P, T, X, N, signed):
    L, W = P[0], P[1]
    a = mp.sqrt(mp.mpf(3) / 5)
    nodes = [(-a, mp.mpf(5) / 9), (mp.mpf(0), mp.mpf(8) / 9), (a, mp.mpf(5) / 9)]
    out = [mp.mpf(0)] * 6
    for xi, wi in nodes:
        for yj, wj in nodes:
            x, y = L / 2 * xi, W / 2 * yj
            ft = _point_force(P, T, X, N, x, y) + _point_torque(P, T, X, N, x, y)
            c = wi * wj * (L * W / 4)
            out = [o + c * g for o, g in zip(out, ft)]
    R22 = X[1][2][2]
    s = R22 if signed else abs(R22)
    return [s * o for o in out]


def wrench(prm, twist, pose, null, signed=False):
    """The contact wrench: s times the integral over the sole of (f, (R q) x f), as six mpf.

    s = |R22| (the wrench of :96, :102), or R22 itself when `signed` (the quantity whose rates
    the reference calls control matrix and autonomous dynamics, :127-170).

    The integral is taken with the 3 x 3 Gauss-Legendre rule scaled to the patch,
    s * sum_ij w_i w_j (L W / 4) (f, (R q_ij) x f).  It is exact, not approximate: f is affine in
    (x, y) and R q is linear in (x, y), so the integrand has degree <= 2 in x and <= 2 in y, and
    an n-point Gauss rule integrates degree <= 2n - 1 = 5 per variable exactly.  What is left is
    the 50-digit rounding of the nine terms."""
    with mp.workdps(DPS):
        return _wrench(*_split(prm, twist, pose, null), signed)


def regressor(prm, twist, pose, null):
    """6 x 2 (rows of mpf): the wrench at (k, b) = (1, 0) and at (0, 1).  The point law is linear
    in (k, b), so regressor @ (k, b) is the wrench."""
    with mp.workdps(DPS):
        P, T, X, N = _split(prm, twist, pose, null)
        ck = _wrench((P[0], P[1], mp.mpf(1), mp.mpf(0)), T, X, N, False)
        cb = _wrench((P[0], P[1], mp.mpf(0), mp.mpf(1)), T, X, N, False)
        return [[ck[i], cb[i]] for i in range(6)]


def control(prm, twist, pose, null):
    """6 x 6 (rows of mpf): the derivative of the signed wrench with respect to the twist.  The
    signed wrench is affine in the twist, so column j is exactly
    wrench_signed(twist = e_j) - wrench_signed(twist = 0); the twist passed in does not matter."""
    with mp.workdps(DPS):
        P, _, X, N = _split(prm, twist, pose, null)
        zero = [mp.mpf(0)] * 3
        base = _wrench(P, (zero, zero), X, N, True)
        cols = []
        for j in range(6):
            e = [mp.mpf(1 if i == j else 0) for i in range(6)]
            wj = _wrench(P, (e[:3], e[3:]), X, N, True)
            cols.append([wj[i] - base[i] for i in range(6)])
        return [[cols[j][i] for j in range(6)] for i in range(6)]


def _exp_so3(w, t):
    """Exp(t skew(w)) by Rodrigues' formula."""
    n = mp.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    I = [[mp.mpf(1 if i == j else 0) for j in range(3)] for i in range(3)]
    if n == 0:
        return I
    K = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    K2 = [[sum(K[i][l] * K[l][j] for l in range(3)) for j in range(3)] for i in range(3)]
    a, c = mp.sin(n * t) / n, (1 - mp.cos(n * t)) / (n * n)
    return [[I[i][j] + a * K[i][j] + c * K2[i][j] for j in range(3)] for i in range(3)]


def autonomous(prm, twist, pose, null):
    """Six mpf: the time derivative of the signed wrench along the motion p + t v,
    Exp(t skew(w)) R with the twist held (the part of the wrench rate that is not control @
    acceleration).

    This is the reference's definition: :125 takes R' = skew(w) R and :127-144 differentiate
    R22 * (...), with R22 unsigned, while the wrench itself carries |R22| (:96, :102).  For
    R22 < 0 the autonomous dynamics (and the control matrix, :165-170) are therefore *minus* the
    derivative of the wrench that the model reports.  That is upstream behaviour and is pinned
    here as it is.

    Computed by a central difference, (F(h) - F(-h)) / 2h with h = 1e-15 at 50 digits, not by
    mp.diff.  F is a product of R22(t) and a polynomial of degree <= 2 in the entries of R(t) and
    degree 1 in p(t); each entry of R(t) is a trigonometric polynomial in |w| t, so
    |F'''| <= 27 |w|^3 max(1, |v| / |p0 - p|) |F|-scale, and the truncation h^2 |F'''| / 6 is
    below 1e-26 of the result's scale for every |w| <= 10.  The rounding of F at 50 digits,
    divided by 2h, adds 1e-35.  Both are far below half an ulp of a double (1.1e-16)."""
    with mp.workdps(DPS):
        P, T, X, N = _split(prm, twist, pose, null)
        h = mp.mpf(DIFF_H)

        def at(t):
            E = _exp_so3(T[1], t)
            Rt = [[sum(E[i][l] * X[1][l][j] for l in range(3)) for j in range(3)]
                  for i in range(3)]
            return _wrench(P, T, ([X[0][i] + t * T[0][i] for i in range(3)], Rt), N, True)

        fp, fm = at(h), at(-h)
        return [(fp[i] - fm[i]) / (2 * h) for i in range(6)]


def to_double(a, extended=False):
    """Round nested mpf to the nearest doubles (or, `extended`, to long doubles, for measuring
    an error against more than a double's worth of the truth).  An entry below 1e-30 of the
    largest entry of its array is set to exactly zero first: at 50 digits a sum whose terms
    cancel analytically (the odd moments of the patch, the off-diagonal blocks of the control
    matrix, a finite difference of two equal values) leaves 1e-48 to 1e-35 of the terms' size,
    never a true zero, and no quantity of this model on any family of the fixture is that small
    without being zero."""
    with mp.workdps(DPS):
        flat = np.array(a, dtype=object)
        top = max([abs(x) for x in flat.reshape(-1)] + [mp.mpf(0)])
        cut = top * mp.mpf(SNAP)
        vals = [mp.mpf(0) if abs(x) <= cut else x for x in flat.reshape(-1)]
        out = np.array([float(x) for x in vals])
        if extended:
            out = out.astype(np.longdouble) + np.array([float(x - float(x)) for x in vals])
        return out.reshape(flat.shape)


def _blocks(shape):
    if shape == (3,):
        return [(slice(0, 3),)]
    if shape == (6,):                                   # force / torque
        return [(slice(0, 3),), (slice(3, 6),)]
    if shape == (6, 2):                                 # per column and block
        return [(slice(r, r + 3), c) for r in (0, 3) for c in (0, 1)]
    if shape == (6, 6):                                 # the four 3 x 3 blocks
        return [(slice(r, r + 3), slice(c, c + 3)) for r in (0, 3) for c in (0, 3)]
    raise ValueError(f"no block structure for shape {shape}")


def block_err(got, exact):
    """Worst block-relative error of one output of one contact: max |got - exact| / max |exact|
    over each block, evaluated in long double.  A block whose exact value is all zero must be
    reproduced as exact zeros; anything else gives inf, and so does a NaN or an infinity.
    Blocks: force / torque of a 6-vector, per column and force / torque rows of the 6 x 2
    regressor, the four 3 x 3 blocks of the control matrix, the whole of a 3-vector (a point
    force or torque).  The off-diagonal entries of the control matrix's top-left block are
    exactly zero in the model and are held to exact zero as well."""
    got = np.asarray(got, dtype=np.longdouble)
    exact = np.asarray(exact, dtype=np.longdouble)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    worst = 0.0
    for n, blk in enumerate(_blocks(exact.shape)):
        g, e = got[blk], exact[blk]
        if not np.all(np.isfinite(g)):
            return float("inf")
        if exact.shape == (6, 6) and n == 0 and np.any(g[~np.eye(3, dtype=bool)] != 0):
            return float("inf")
        top = np.max(np.abs(e))
        if top == 0:
            if np.any(g != 0):
                return float("inf")
            continue
        worst = max(worst, float(np.max(np.abs(g - e)) / top))
    return worst


def batch_block_err(got, exact):
    """The worst `block_err` over a batch of contacts (or points) along axis 0."""
    assert len(got) == len(exact)
    return max((block_err(g, e) for g, e in zip(got, exact)), default=0.0)


def fixture_points(L, W):
    """The 18 points of the fixture for a sole of L x W: the centre, the four corners (inside, by
    the > rule), one nextafter outside the middle of each of the four edges, the nine Gauss
    nodes.  Returns an (18, 2) array of doubles."""
    hl, hw = L / 2, W / 2
    pts = [(0.0, 0.0), (hl, hw), (hl, -hw), (-hl, hw), (-hl, -hw),
           (np.nextafter(hl, np.inf), 0.0), (np.nextafter(-hl, -np.inf), 0.0),
           (0.0, np.nextafter(hw, np.inf)), (0.0, np.nextafter(-hw, -np.inf))]
    pts += [(hl * gx, hw * gy) for gx in GAUSS_X for gy in GAUSS_X]
    return np.array(pts, dtype=np.float64)


CENTRE, CORNERS, OUTSIDE, NODES = slice(0, 1), slice(1, 5), slice(5, 9), slice(9, 18)
