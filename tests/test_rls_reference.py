"""CPU tests of the recursive-least-squares feature: the ordered numpy reference (the arithmetic
order of include/blf/blf_c.h section 10) against the reference's literal formula, the reference
test's model (RecursiveLeastSquareTest.cpp:36-142) at its own 0.1 % bar, and the C ABI's argument
validation, which happens before any device work."""
import ctypes
import os

import numpy as np
import pytest

import rls_reference as R
from blf import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "tests", "golden", "estimators_config.ini")

# Largest relative difference, over the ten cases below, between the sequential form and the
# literal K = P H^T (lam R + H P H^T)^-1 update: measured 2.52e-13 (the (8, 8), lambda = 1
# case).  Both sides are this project's code and the test only has to catch a wrong formula, so
# the bound is 100 times the measured value.
LITERAL_MEASURED = 2.52e-13
LITERAL_BOUND = 100 * LITERAL_MEASURED


def random_problem(n, m, lam, seed, B=3, T=50):
    rs = np.random.RandomState(seed)
    H = rs.standard_normal((T, B, m, n))
    truth = rs.standard_normal((B, n))
    Y = np.einsum("tbmn,bn->tbm", H, truth) + 0.1 * rs.standard_normal((T, B, m))
    r = rs.uniform(0.1, 1.0, (B, m))
    x0 = np.zeros((B, n))
    P0 = np.broadcast_to(10.0 * np.eye(n), (B, n, n)).copy()
    return H, Y, x0, P0, r


def literal_difference(n, m, lam):
    H, Y, x0, P0, r = random_problem(n, m, lam, seed=100 * n + m)
    xs, Ps = R.advance(H, Y, x0, P0, r, lam)
    xl, Pl = R.advance_literal(H, Y, x0, P0, r, lam)
    dx = np.abs(xs - xl).max() / np.abs(xl).max()
    dP = np.abs(Ps - Pl).max() / np.abs(Pl).max()
    return max(dx, dP), Ps


@pytest.mark.parametrize("lam", [1.0, 0.98])
@pytest.mark.parametrize("n,m", [(1, 1), (2, 2), (2, 6), (5, 7), (8, 8)])
def test_ordered_reference_matches_literal_formula(n, m, lam):
    diff, Ps = literal_difference(n, m, lam)
    print(f"n={n} m={m} lambda={lam}: relative difference {diff:.3e}")
    assert diff < LITERAL_BOUND
    np.testing.assert_array_equal(Ps, np.swapaxes(Ps, 1, 2))   # mirrored: exactly symmetric


def test_reference_model_meets_the_reference_bar():
    cfg = R.read_ini(CONFIG)
    assert set(cfg) == {"lambda", "measurement_covariance", "state", "state_covariance"}
    H, Y = R.model_samples([42])
    x0 = np.array([cfg["state"]])
    P0 = np.diag(cfg["state_covariance"])[None]
    x, P = R.advance(H, Y, x0, P0, np.array(cfg["measurement_covariance"]), cfg["lambda"])
    err = np.abs((x[0] - [43.2, 12.2]) / [43.2, 12.2])
    print("relative errors", err)   # 1.05e-4 and 4.46e-4 with seed 42
    assert (err < 0.1 / 100.0).all()
    assert (np.linalg.eigvalsh(P[0]) > 0).all()


def test_poisoned_filter_goes_nan_alone():
    H, Y, x0, P0, r = random_problem(2, 3, 1.0, seed=5, B=4, T=6)
    r = r.copy()
    r[2, 1] = 0.0
    H[3, 2, 1] = 0.0   # s = 0 at step 3, row 1 of filter 2
    x, P = R.advance(H, Y, x0, P0, r, 1.0)
    assert np.isnan(x[2]).all() and np.isnan(P[2]).all()
    keep = [0, 1, 3]
    xk, Pk = R.advance(H[:, keep], Y[:, keep], x0[keep], P0[keep], r[keep], 1.0)
    np.testing.assert_array_equal(x[keep], xk)
    np.testing.assert_array_equal(P[keep], Pk)


# ---- argument validation through ctypes: no device is touched ---------------------------------
_FAKE = ctypes.c_void_p(1)     # the handle is only compared with null before any device work
_PTR = ctypes.c_void_p(8)      # likewise every buffer


def _rls(handle=_FAKE, n=2, m=2, lam=1.0, cov=_PTR, reg=_PTR, meas=_PTR, steps=1, state=_PTR,
         covariance=_PTR, batch=4):
    return native.lib().blf_rls_advance(handle, n, m, lam, cov, 0, reg, meas, steps, state,
                                        covariance, batch, None)


def _contact_rls(handle=_FAKE, lam=1.0, cov=_PTR, geometry=_PTR, twist=_PTR, pose=_PTR,
                 null_pose=_PTR, wrench=_PTR, steps=1, state=_PTR, covariance=_PTR, batch=4):
    return native.lib().blf_contact_rls_advance(handle, lam, cov, 0, geometry, 0, twist, pose,
                                                null_pose, wrench, steps, state, covariance, batch,
                                                None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(handle=None), 1, "handle"),
    (dict(cov=None), 1, "meas_cov"),
    (dict(reg=None), 1, "regressor"),
    (dict(meas=None), 1, "measurements"),
    (dict(state=None), 1, "state"),
    (dict(covariance=None), 1, "covariance"),
    (dict(steps=0), 1, "steps"),
    (dict(batch=-1), 1, "batch"),
    (dict(lam=0.0), 1, "lambda"),
    (dict(lam=-0.5), 1, "lambda"),
    (dict(lam=float("nan")), 1, "lambda"),
    (dict(lam=float("inf")), 1, "lambda"),
    (dict(n=0), 3, "n="),
    (dict(n=9), 3, "n="),
    (dict(m=0), 3, "m="),
    (dict(m=9), 3, "m="),
])
def test_rls_advance_rejects_bad_arguments(kw, code, word):
    assert _rls(**kw) == code
    assert "blf_rls_advance" in native.last_error() and word in native.last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(handle=None), "handle"), (dict(cov=None), "meas_cov"), (dict(geometry=None), "geometry"),
    (dict(twist=None), "twist"), (dict(pose=None), "pose"), (dict(null_pose=None), "null_pose"),
    (dict(wrench=None), "wrench"), (dict(state=None), "state"),
    (dict(covariance=None), "covariance"), (dict(steps=0), "steps"), (dict(batch=-1), "batch"),
    (dict(lam=0.0), "lambda"), (dict(lam=float("nan")), "lambda"),
])
def test_contact_rls_advance_rejects_bad_arguments(kw, word):
    assert _contact_rls(**kw) == 1
    assert "blf_contact_rls_advance" in native.last_error() and word in native.last_error()


def test_empty_batch_is_ok_without_a_device():
    assert _rls(batch=0) == 0
    assert _contact_rls(batch=0) == 0


def test_abi_version_is_three():
    assert "(abi 3," in native.version()
    assert {"blf_rls_advance", "blf_contact_rls_advance"} <= set(native.EXPORTED)
