"""numpy restatement of blf_rls_advance's arithmetic order (include/blf/blf_c.h section 10), the
reference the device is compared with bit for bit, and, independently, the literal three-line
update of the reference (RecursiveLeastSquare.cpp:119-130) with numpy.linalg.inv.

`advance` is vectorised over the batch axis only: every sum is written out term by term, left to
right, and elementwise float64 numpy does not fuse a multiply into an add, so every bit is defined.
"""
import numpy as np


def advance(regressor, measurements, state, covariance, meas_cov, lam=1.0):
    """regressor [T,B,m,n], measurements [T,B,m], state [B,n], covariance [B,n,n] (read through its
    upper triangle), meas_cov [m] or [B,m].  Returns the new (state [B,n], covariance [B,n,n])."""
    H = np.asarray(regressor, dtype=np.float64)
    Y = np.asarray(measurements, dtype=np.float64)
    T, B, m, n = H.shape
    r = np.broadcast_to(np.asarray(meas_cov, dtype=np.float64), (B, m))
    lam = np.float64(lam)
    x = [np.array(state[:, a], dtype=np.float64) for a in range(n)]
    # P[a][b] for a <= b; P[a][c] with a > c is P[c][a]
    P = {(a, b): np.array(covariance[:, a, b], dtype=np.float64) for a in range(n) for b in range(a, n)}
    nan = np.float64("nan")
    with np.errstate(all="ignore"):
        for t in range(T):
            for j in range(m):
                h = [H[t, :, j, c] for c in range(n)]
                g = []
                for a in range(n):
                    acc = P[(0, a)] * h[0]
                    for c in range(1, n):
                        acc = acc + P[(c, a) if c < a else (a, c)] * h[c]
                    g.append(acc)
                hg = h[0] * g[0]
                hx = h[0] * x[0]
                for a in range(1, n):
                    hg = hg + h[a] * g[a]
                    hx = hx + h[a] * x[a]
                s = (lam * r[:, j]) + hg
                e = Y[t, :, j] - hx
                good = (s > 0.0) & (s < np.inf)
                k = [g[a] / s for a in range(n)]
                for a in range(n):
                    x[a] = np.where(good, x[a] + k[a] * e, nan)
                    for b in range(a, n):
                        P[(a, b)] = np.where(good, P[(a, b)] - k[a] * g[b], nan)
            for key in P:
                P[key] = P[key] / lam
    xo = np.stack(x, axis=1)
    Po = np.empty((B, n, n))
    for a in range(n):
        for b in range(n):
            Po[:, a, b] = P[(a, b) if a <= b else (b, a)]
    return xo, Po


def advance_literal(regressor, measurements, state, covariance, meas_cov, lam=1.0):
    """The reference's advance(), one filter at a time:
    K = P H^T (lam R + H P H^T)^-1;  x = x + K (y - H x);  P = (P - K H P) / lam."""
    H = np.asarray(regressor, dtype=np.float64)
    Y = np.asarray(measurements, dtype=np.float64)
    T, B, m, n = H.shape
    r = np.broadcast_to(np.asarray(meas_cov, dtype=np.float64), (B, m))
    xo = np.array(state, dtype=np.float64)
    Po = np.array(covariance, dtype=np.float64)
    for q in range(B):
        x, P, R = xo[q].copy(), Po[q].copy(), np.diag(r[q])
        for t in range(T):
            Ht = H[t, q]
            K = P @ Ht.T @ np.linalg.inv(lam * R + Ht @ P @ Ht.T)
            x = x + K @ (Y[t, q] - Ht @ x)
            P = (P - K @ Ht @ P) / lam
        xo[q], Po[q] = x, P
    return xo, Po


def model_samples(seeds, steps=10000, params=(43.2, 12.2)):
    """The reference test's model (RecursiveLeastSquareTest.cpp:36-142), one filter per noise seed:
    H_i = [[x, x^2], [sin x, cos x]] with x = cos(i / 10), y_i = H_i params + noise, noise from
    numpy.random.RandomState(seed).normal(0, 0.5, 2) per step.  Returns regressor [T,B,2,2] and
    measurements [T,B,2]."""
    xs = np.cos(np.arange(steps) / 10.0)
    H1 = np.stack([np.stack([xs, xs * xs], 1), np.stack([np.sin(xs), np.cos(xs)], 1)], 1)   # [T,2,2]
    p = np.asarray(params, dtype=np.float64)
    clean = H1 @ p
    B = len(seeds)
    H = np.ascontiguousarray(np.broadcast_to(H1[:, None], (steps, B, 2, 2)))
    Y = np.empty((steps, B, 2))
    for q, seed in enumerate(seeds):
        # one draw of (steps, 2) is the same stream as `steps` draws of 2
        Y[:, q] = clean + np.random.RandomState(seed).normal(0, 0.5, (steps, 2))
    return H, Y


def read_ini(path):
    """The four settings of the reference's Estimators test configuration: scalars and
    parenthesised lists by key."""
    out = {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            key, val = line.split(None, 1)
            val = val.strip()
            if val.startswith("("):
                out[key] = [float(v) for v in val.strip("()").split(",")]
            else:
                out[key] = float(val)
    return out
