"""CPU tests of the swing-foot / SO(3) planner feature: the numpy restatement of include/blf/blf_c.h
section 11 (tests/swing_foot_reference.py) against independent closed forms (yaw-only feet, central
differences, orthonormality, continuity into the landing contact), problems.foot_contact_tables, and
the C ABI's argument validation, which happens before any device work."""
import ctypes

import numpy as np
import pytest

import swing_foot_reference as S
from blf import native
from blf import problems as P

FD_STEP = 1e-6    # as the contact model's finite-difference test (tests/test_oracle_contact.py)
FD_TOL = 1e-4


def two_contact_list(Ra, Rb, pa=(0.1, 0.05, 0.0), pb=(0.45, 0.12, 0.03)):
    """One list, stance [0, 0.4), swing [0.4, 1.0), stance [1.0, 1.8)."""
    cp = np.zeros((1, 2, 12))
    cp[0, 0, :3], cp[0, 0, 3:] = pa, np.asarray(Ra).reshape(9)
    cp[0, 1, :3], cp[0, 1, 3:] = pb, np.asarray(Rb).reshape(9)
    ct = np.array([[[0.0, 0.4], [1.0, 1.8]]])
    return cp, ct, np.array([2], dtype=np.int32)


PRM = dict(step_height=0.04, apex_ratio=0.4, landing_velocity=-0.05, landing_acceleration=0.3)


def test_yaw_only_feet_follow_the_closed_form():
    psi0, psi1 = 0.07, -0.09
    cp, ct, n = two_contact_list(S.rz(psi0), S.rz(psi1))
    t = np.linspace(0.4, 1.0, 41)[None, :-1]
    r = S.swing_foot_eval(cp, ct, n, t, **PRM)
    assert r["swing"].all() and (r["contact_idx"] == 0).all() and (r["in_contact"] == 0).all()
    tau = (t[0] - 0.4) / 0.6
    s, sd, sdd = S.min_jerk(tau, 0.6)
    dpsi = psi1 - psi0
    np.testing.assert_allclose(r["pose"][0, :, 3:], S.rz(psi0 + s * dpsi).reshape(-1, 9),
                               rtol=0, atol=1e-14)
    w = np.zeros((t.shape[1], 3))
    w[:, 2] = sd * dpsi
    np.testing.assert_allclose(r["twist"][0, :, 3:], w, rtol=0, atol=1e-14)
    a = np.zeros_like(w)
    a[:, 2] = sdd * dpsi
    np.testing.assert_allclose(r["accel"][0, :, 3:], a, rtol=0, atol=2e-14)   # |alpha| up to 2.6


def vee(M):
    return np.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0],
                     M[..., 1, 0] - M[..., 0, 1]], axis=-1) * 0.5


@pytest.mark.parametrize("angle", [0.15, 2.0, np.pi - 1e-6])
def test_twist_and_acceleration_match_central_differences(angle):
    Ra = S.axis_angle([0.3, -0.5, 0.8], 0.4)
    Rb = S.axis_angle([1.0, 2.0, -0.5], angle) @ Ra
    cp, ct, n = two_contact_list(Ra, Rb)
    t = np.linspace(0.43, 0.97, 19)[None]
    h = FD_STEP
    r0, rp, rm = (S.swing_foot_eval(cp, ct, n, t + k * h, **PRM) for k in (0, 1, -1))
    assert r0["swing"].all() and rp["swing"].all() and rm["swing"].all()
    np.testing.assert_allclose((rp["pose"][..., :3] - rm["pose"][..., :3]) / (2 * h),
                               r0["twist"][..., :3], rtol=0, atol=FD_TOL)
    Rp, Rm = rp["pose"][..., 3:].reshape(-1, 3, 3), rm["pose"][..., 3:].reshape(-1, 3, 3)
    w_num = vee(Rp @ np.swapaxes(Rm, 1, 2)) / (2 * h)
    np.testing.assert_allclose(w_num, r0["twist"][0, :, 3:], rtol=0, atol=FD_TOL)
    np.testing.assert_allclose((rp["twist"] - rm["twist"]) / (2 * h), r0["accel"], rtol=0,
                               atol=FD_TOL)


def rotation_cases():
    """(name, R_a, R_b): the relative rotations the device tests use."""
    rs = np.random.RandomState(7)
    base = S.axis_angle(rs.standard_normal(3), 0.7)
    cases = [("identical", base, base.copy()),
             ("tiny", base, S.axis_angle([0.2, -1.0, 0.4], 1e-10) @ base),
             ("yaw", S.rz(0.08), S.rz(-0.06)),
             ("general", base, S.axis_angle([0.5, 0.3, -0.8], 2.0) @ base),
             ("near_pi", base, S.axis_angle([-0.4, 0.9, 0.2], np.pi - 1e-6) @ base),
             ("pi_z", np.eye(3), np.diag([-1.0, -1.0, 1.0]))]
    return cases


@pytest.mark.parametrize("name,Ra,Rb", rotation_cases(), ids=[c[0] for c in rotation_cases()])
def test_rotation_is_orthonormal_and_continuous_into_the_landing_contact(name, Ra, Rb):
    cp, ct, n = two_contact_list(Ra, Rb)
    t = np.concatenate([np.linspace(0.4, 1.0, 33)[:-1], [1.0 - 1e-9, 1.0 - 1e-12]])[None]
    r = S.swing_foot_eval(cp, ct, n, t, **PRM)
    R = r["pose"][0, :, 3:].reshape(-1, 3, 3)
    np.testing.assert_allclose(R @ np.swapaxes(R, 1, 2), np.broadcast_to(np.eye(3), R.shape),
                               rtol=0, atol=1e-14)
    np.testing.assert_array_equal(R[0], Ra)   # s = 0 at lift: Exp(0) R_a is R_a
    # tau -> 1: the pose tends to the landing contact's (s - 1 = O((1 - tau)^3), the position
    # within |v_land| (t1 - t)).  Log then Exp is a chain of some 60 rounded operations on O(1)
    # terms, so the round trip is bounded at 1e-13 (450 ulp), not at the 1e-14 of a single product.
    np.testing.assert_allclose(r["pose"][0, -1, 3:], Rb.reshape(9), rtol=0, atol=1e-13)
    np.testing.assert_allclose(r["pose"][0, -1, :3], cp[0, 1, :3], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["pose"][0, -2, :3], cp[0, 1, :3], rtol=0, atol=1e-9)
    land = S.swing_foot_eval(cp, ct, n, np.array([[1.0]]), **PRM)
    np.testing.assert_array_equal(land["pose"][0, 0], cp[0, 1])
    assert land["in_contact"][0, 0] == 1 and land["contact_idx"][0, 0] == 1
    if name == "identical":
        np.testing.assert_array_equal(r["pose"][0, :, 3:], np.broadcast_to(Ra.reshape(9), (t.shape[1], 9)))
        assert not r["twist"][0, :, 3:].any()


def test_lookup_rule_ties_and_poisoning():
    cp, ct, n = two_contact_list(S.rz(0.1), S.rz(0.2))
    t = np.array([[-0.5, 0.0, 0.2, 0.4, 0.7, 1.0, 1.5, 1.8, 2.5]])
    r = S.swing_foot_eval(cp, ct, n, t, **PRM)
    np.testing.assert_array_equal(r["contact_idx"][0], [-1, 0, 0, 0, 0, 1, 1, 1, 1])
    np.testing.assert_array_equal(r["in_contact"][0], [0, 1, 1, 0, 0, 1, 1, 0, 0])
    np.testing.assert_array_equal(r["swing"][0], [0, 0, 0, 1, 1, 0, 0, 0, 0])
    np.testing.assert_array_equal(r["pose"][0, 0], cp[0, 0])    # before the first activation
    np.testing.assert_array_equal(r["pose"][0, 3], cp[0, 0])    # lift-off: still the old pose
    np.testing.assert_array_equal(r["pose"][0, 8], cp[0, 1])    # after the last deactivation
    assert not r["twist"][0, [0, 1, 2, 3, 5, 6, 7, 8]].any()
    for bad_n in (0, 3):
        rb = S.swing_foot_eval(cp, ct, np.array([bad_n], dtype=np.int32), t, **PRM)
        assert np.isnan(rb["pose"]).all() and np.isnan(rb["twist"]).all() and np.isnan(rb["accel"]).all()
        assert (rb["contact_idx"] == -1).all() and (rb["in_contact"] == 0).all()


def test_so3_reference_clamps_and_matches_the_swing_rotation():
    Ra = S.axis_angle([0.1, 0.2, 0.9], 0.3)
    Rb = S.axis_angle([0.5, 0.3, -0.8], 2.0) @ Ra
    cp, ct, n = two_contact_list(Ra, Rb)
    tq = np.array([[-0.3, 0.0, 0.15, 0.3, 0.45, 0.6, 0.9]])
    r = S.so3_eval(Ra[None], Rb[None], np.array([0.6]), tq)
    sw = S.swing_foot_eval(cp, ct, n, 0.4 + tq[:, 2:5], **PRM)
    np.testing.assert_allclose(r["rot"][0, 2:5], sw["pose"][0, :, 3:], rtol=0, atol=1e-14)
    np.testing.assert_allclose(r["omega"][0, 2:5], sw["twist"][0, :, 3:], rtol=0, atol=1e-13)
    np.testing.assert_array_equal(r["rot"][0, 0], r["rot"][0, 1])
    np.testing.assert_array_equal(r["rot"][0, 5], r["rot"][0, 6])
    np.testing.assert_allclose(r["rot"][0, 6], Rb.reshape(9), rtol=0, atol=1e-14)
    assert not r["omega"][0, [0, 1, 5, 6]].any() and not r["alpha"][0, [0, 1, 5, 6]].any()
    assert np.isnan(S.so3_eval(Ra[None], Rb[None], np.array([0.0]), tq)["rot"]).all()


def test_foot_contact_tables_follow_the_schedule():
    prob = P.make_batch(4, horizon=100, n_footsteps=6)
    tabs = P.foot_contact_tables(prob)
    assert set(tabs) == {"left", "right"}
    C = max(len(v) for v in prob["schedule"].values())
    for foot, tab in tabs.items():
        lst = prob["schedule"][foot]
        assert tab["contact_pose"].shape == (4, C, 12) and tab["contact_time"].shape == (4, C, 2)
        assert tab["ncontacts"].dtype == np.int32 and (tab["ncontacts"] == len(lst)).all()
        for c, (act, deact, slot) in enumerate(lst):
            np.testing.assert_array_equal(tab["contact_time"][:, c], [[act * prob["dt"],
                                                                       deact * prob["dt"]]] * 4)
            np.testing.assert_array_equal(tab["contact_pose"][:, c, :2], prob["poses"][:, slot, :2])
            assert not tab["contact_pose"][:, c, 2].any()
            np.testing.assert_array_equal(tab["contact_pose"][:, c, 3:].reshape(4, 3, 3),
                                          S.rz(prob["poses"][:, slot, 2]))
    # with rho = 0.5, z = 0 and no landing terms, section 11's knots are problems.swing_splines'
    kt, kp, _ = P.swing_splines(prob, apex_height=0.05)
    tab, lst = tabs["left"], prob["schedule"]["left"]
    k, pva = S.swing_knots(tab["contact_pose"][0, 0, :3], tab["contact_pose"][0, 1, :3],
                           tab["contact_time"][0, 0, 1], tab["contact_time"][0, 1, 0], 0.05, 0.5,
                           0.0, 0.0)
    np.testing.assert_array_equal(k, kt[0])
    np.testing.assert_array_equal(pva, kp[0])


# ---- argument validation through ctypes: no device is touched ---------------------------------
_FAKE = ctypes.c_void_p(1)     # the handle is only compared with null before any device work
_PTR = ctypes.c_void_p(8)      # likewise every buffer


def _swing(handle=_FAKE, prm=True, pose=_PTR, time=_PTR, nc=_PTR, batch=4, tq=_PTR, nq=3, out=_PTR,
           **fields):
    p = native.SwingFootParams(4, 0, 0.05, 0.5, 0.0, 0.0)
    for k, v in fields.items():
        setattr(p, k, v)
    outs = [out, None, None, None, None]
    return native.lib().blf_swing_foot_eval(handle, ctypes.byref(p) if prm else None, pose, time, nc,
                                            batch, tq, nq, *outs, None)


def _so3(handle=_FAKE, R0=_PTR, R1=_PTR, duration=_PTR, batch=4, tq=_PTR, nq=3, out=_PTR):
    return native.lib().blf_so3_eval(handle, R0, R1, duration, batch, tq, nq, out, None, None, None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(handle=None), 1, "handle"),
    (dict(prm=False), 1, "params"),
    (dict(pose=None), 1, "contact_pose"),
    (dict(time=None), 1, "contact_time"),
    (dict(nc=None), 1, "ncontacts"),
    (dict(tq=None), 1, "tq"),
    (dict(out=None), 1, "output"),
    (dict(batch=-1), 1, "batch"),
    (dict(nq=-1), 1, "nq"),
    (dict(reserved=1), 1, "reserved"),
    (dict(step_height=-0.01), 1, "step_height"),
    (dict(step_height=float("nan")), 1, "step_height"),
    (dict(apex_ratio=0.0), 1, "apex_ratio"),
    (dict(apex_ratio=1.0), 1, "apex_ratio"),
    (dict(apex_ratio=float("nan")), 1, "apex_ratio"),
    (dict(landing_velocity=float("inf")), 1, "landing_velocity"),
    (dict(landing_acceleration=float("nan")), 1, "landing_acceleration"),
    (dict(max_contacts=0), 3, "max_contacts"),
    (dict(max_contacts=17), 3, "max_contacts"),
])
def test_swing_foot_eval_rejects_bad_arguments(kw, code, word):
    assert _swing(**kw) == code
    assert "blf_swing_foot_eval" in native.last_error() and word in native.last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(handle=None), "handle"), (dict(R0=None), "R0"), (dict(R1=None), "R1"),
    (dict(duration=None), "duration"), (dict(tq=None), "tq"), (dict(out=None), "output"),
    (dict(batch=-1), "batch"), (dict(nq=-1), "nq"),
])
def test_so3_eval_rejects_bad_arguments(kw, word):
    assert _so3(**kw) == 1
    assert "blf_so3_eval" in native.last_error() and word in native.last_error()


def test_empty_batch_is_ok_without_a_device():
    assert _swing(batch=0) == 0 and _swing(nq=0) == 0
    assert _so3(batch=0) == 0 and _so3(nq=0) == 0


def test_entry_points_were_added_within_abi_three():
    assert "(abi 3," in native.version()
    assert {"blf_swing_foot_eval", "blf_so3_eval"} <= set(native.EXPORTED)
