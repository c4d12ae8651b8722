"""CPU checks of tests/closed_loop_ik_reference.py, the numpy restatements the GPU tests of
blf_dcm_com_reference and blf_fbd_euler_integrate_impedance_traj compare against."""
import numpy as np

import closed_loop as CL
import closed_loop_ik_reference as IR
from blf import closed_loop as DL
from blf import robot as R


def _inputs(B, seed=0):
    rng = np.random.default_rng(seed)
    return dict(xi0=rng.normal(size=(B, 2)) * 0.05, r0=rng.normal(size=(B, 2)) * 0.05,
                omega0=np.sqrt(9.81 / rng.uniform(0.5, 0.6, B)), z_ref=rng.uniform(0.5, 0.6, B),
                c_ref=rng.normal(size=(B, 2)) * 0.05)


def test_com_reference_two_calls_equal_one():
    """c_ref and xi_end carried: two calls of T steps are one call of 2 T, bit for bit."""
    a, T, h = _inputs(5), 4, 0.005
    p2, v2, c2, x2 = IR.com_reference(a["xi0"], a["r0"], a["omega0"], a["z_ref"], a["c_ref"], 2 * T, h)
    pa, va, ca, xa = IR.com_reference(a["xi0"], a["r0"], a["omega0"], a["z_ref"], a["c_ref"], T, h)
    pb, vb, cb, xb = IR.com_reference(xa, a["r0"], a["omega0"], a["z_ref"], ca, T, h)
    np.testing.assert_array_equal(np.concatenate([pa, pb], axis=1), p2)
    np.testing.assert_array_equal(np.concatenate([va, vb], axis=1), v2)
    np.testing.assert_array_equal(cb, c2)
    np.testing.assert_array_equal(xb, x2)


def test_com_reference_fixed_point():
    """r0 = xi_0 = c_0: nothing moves."""
    a = _inputs(3, seed=1)
    p, v, c, x = IR.com_reference(a["r0"], a["r0"], a["omega0"], a["z_ref"], a["r0"], 6, 0.005)
    np.testing.assert_array_equal(p[:, :, :2], np.repeat(a["r0"][:, None], 6, axis=1))
    np.testing.assert_array_equal(p[:, :, 2], np.repeat(a["z_ref"][:, None], 6, axis=1))
    assert (v == 0.0).all()
    np.testing.assert_array_equal(c, a["r0"])
    np.testing.assert_array_equal(x, a["r0"])


def test_com_reference_first_order():
    """Halving h halves the distance to the closed form at t = T h, within 10 % (explicit Euler)."""
    a, t = _inputs(4, seed=2), 0.02
    err = []
    for T in (4, 8):
        _, _, c, _ = IR.com_reference(a["xi0"], a["r0"], a["omega0"], a["z_ref"], a["c_ref"], T, t / T)
        exact = np.array([[IR.com_closed_form(a["xi0"][b, k], a["r0"][b, k], a["omega0"][b], a["c_ref"][b, k], t)
                           for k in range(2)] for b in range(4)])
        err.append(np.abs(c - exact))
    ratio = err[1] / err[0]
    print("error ratio at h / 2:", ratio.min(), ratio.max())
    assert (np.abs(ratio - 0.5) <= 0.05).all(), ratio


def test_com_reference_nan_is_per_robot():
    a = _inputs(3, seed=3)
    clean = IR.com_reference(a["xi0"], a["r0"], a["omega0"], a["z_ref"], a["c_ref"], 4, 0.005)
    xi = a["xi0"].copy()
    xi[1, 0] = np.nan
    bad = IR.com_reference(xi, a["r0"], a["omega0"], a["z_ref"], a["c_ref"], 4, 0.005)
    for c, b in zip(clean, bad):
        assert np.isnan(b[1]).all()
        np.testing.assert_array_equal(b[[0, 2]], c[[0, 2]])


def test_traj_impedance_identical_slices_is_held_reference():
    """T identical slices, no qd_ref, no bias: oracle/closed_loop.py's euler_integrate_impedance, bit for
    bit (humanoid24, one robot on its soles, 0 -> 0.019 s at dT = 1 ms)."""
    model = R.humanoid24()
    st = R.standing_states(model, 1, seed=5)
    law = R.posture_law_arrays(model)
    q_ref = np.random.default_rng(3).normal(size=model["n"]) * 0.02
    kw = dict(contacts=[0, 1], contact_params=np.tile(np.asarray(DL.CONTACT_PARAMS), (2, 1)),
              null_poses=R.sole_null_poses(model, st)[0])
    held = CL.euler_integrate_impedance(model, st, 0, q_ref, law["kp"], law["kd"], 0.0, 0.019, 0.001, **kw)
    traj = IR.euler_integrate_impedance_traj(model, st, 0, np.tile(q_ref, (3, 1)), law["kp"], law["kd"], 4, 0.0,
                                             0.019, 0.001, **kw)
    assert len(DL.fixed_step_schedule(0.0, 0.019, 0.001)) == 19
    for k in held:
        np.testing.assert_array_equal(traj[k], held[k], err_msg=k)


def test_slice_indexing():
    assert [IR.slice_of(i, 5, 4) for i in range(19)] == [0] * 5 + [1] * 5 + [2] * 5 + [3] * 4
    assert [IR.slice_of(i, 3, 2) for i in range(8)] == [0, 0, 0, 1, 1, 1, 1, 1]
