"""GPU tests of blf.closed_loop.ClosedLoop(reference="ik", control="computed_torque"): the IK period with
its dynamics call replaced by blf_fbd_euler_integrate_computed_torque_traj, against
tests/inverse_dynamics_reference.py's ComputedTorqueOracleLoop and the per-joint recurrence; the impedance
modes untouched; and the tracking error against the existing IK mode's."""
import numpy as np
import pytest
import torch

import fb_models as FM
import ik_limits_reference as LR
import inverse_dynamics_reference as ID
from blf import closed_loop as DL
from blf import native, problems as P, robot as R

pytestmark = pytest.mark.gpu
MODEL = R.humanoid24()
TOL = 1e-9


def _setup(B, periods, seed=3):
    """tests/test_gpu_closed_loop_ik.py's fixture."""
    N = 100
    plan = P.make_batch(B, horizon=N + periods, n_footsteps=8, seed=P.SEED, first_ds=periods + 10)
    return plan, R.standing_states(MODEL, B, seed=seed)


def test_computed_torque_loop(handle):
    """B = 3, three coupled periods.  Device against the CPU composition: plan and IK statuses equal and OK,
    the robot state within 1e-9 relative per key; joint_pos / joint_vel at each period end against
    joint_recurrence driven by the device's own joint_traj / nu_traj from the period's start values; the
    impedance IK mode, default and named, bit for bit the same; and the RMS of q - joint_traj[-1] at the
    period ends below the impedance IK mode's (printed: the pair and the ratio)."""
    B, S = 3, 3
    plan, st = _setup(B, S)
    loop = DL.ClosedLoop(handle, MODEL, plan, st, reference="ik", control="computed_torque")
    imp = DL.ClosedLoop(handle, MODEL, plan, st, reference="ik")
    named = DL.ClosedLoop(handle, MODEL, plan, st, reference="ik", control="impedance")
    ref = ID.ComputedTorqueOracleLoop(MODEL, plan, st, R.sole_null_poses(MODEL, st), R.posture_law_arrays(MODEL),
                                      DL.CONTACT_PARAMS)
    assert loop.control == "computed_torque" and imp.control == "impedance" and not loop.lean and imp.lean
    assert loop.steps_per_slice == 5 and len(loop.steps) == 19 and not hasattr(imp, "ctq")
    err_ct, err_imp, worst = [], [], 0.0
    for s in range(S):
        q0, qd0 = loop.state["joint_pos"].cpu().numpy().copy(), loop.state["joint_vel"].cpu().numpy().copy()
        out = loop.period()
        imp.period()
        named.period()
        torch.cuda.synchronize()
        o = ref.period()
        np.testing.assert_array_equal(out["status"].cpu().numpy(), o["status"])
        assert (o["status"] == 0).all()
        assert all(r["status"] == LR.OK for r in o["track"]), s
        assert (loop.ik_status.cpu().numpy() == LR.OK).all() and (loop.ik_fail_step.cpu().numpy() == -1).all()
        np.testing.assert_array_equal(loop.ik_iters.cpu().numpy(), [r["iters"] for r in o["track"]])
        for k in native.FB_STATE_KEYS:
            e = FM.rel_err(loop.state[k].cpu().numpy(), ref.state[k])
            worst = max(worst, e)
            print("period", s, k, "rel err %.3g" % e)
            assert e <= TOL, (s, k, e)
        assert FM.rel_err(loop.tau_last.cpu().numpy(), ref.tau_last) <= TOL, s
        jt, nu = loop.joint_traj.cpu().numpy(), loop.nu_traj.cpu().numpy()
        q, qd = ID.joint_recurrence(q0, qd0, dict(q_ref=jt, qd_ref=nu[..., 6:]), 400.0, 40.0, loop.steps,
                                    loop.steps_per_slice)
        e_q = FM.rel_err(loop.state["joint_pos"].cpu().numpy(), q)
        e_v = FM.rel_err(loop.state["joint_vel"].cpu().numpy(), qd)
        print("period", s, "joint recurrence: pos %.3g vel %.3g" % (e_q, e_v))
        assert e_q <= TOL and e_v <= TOL, (s, e_q, e_v)
        err_ct.append(loop.state["joint_pos"].cpu().numpy() - jt[-1])
        err_imp.append(imp.state["joint_pos"].cpu().numpy() - imp.joint_traj.cpu().numpy()[-1])
    for k in native.FB_STATE_KEYS:
        np.testing.assert_array_equal(imp.state[k].cpu().numpy(), named.state[k].cpu().numpy(), err_msg=k)
    np.testing.assert_array_equal(imp.joint_traj.cpu().numpy(), named.joint_traj.cpu().numpy())
    rms = lambda e: float(np.sqrt(np.mean(np.square(np.stack(e)))))
    r_ct, r_imp = rms(err_ct), rms(err_imp)
    print("worst state rel err %.3g" % worst)
    print("RMS of q - joint_traj[-1] at the period ends [rad]: computed torque %.3g, impedance %.3g, ratio %.3g"
          % (r_ct, r_imp, r_imp / r_ct))
    assert r_ct < r_imp


def test_split_groups_passes_the_mode_through(handle):
    B, S = 4, 2
    plan, st = _setup(B, S)
    loops = DL.split_groups(handle, MODEL, plan, st, 2, reference="ik", control="computed_torque",
                            computed_torque=dict(freq=20.0, tau_max=80.0))
    whole = DL.ClosedLoop(handle, MODEL, plan, st, reference="ik", control="computed_torque",
                          computed_torque=dict(freq=20.0, tau_max=80.0))
    assert [lp.control for lp in loops] == ["computed_torque"] * 2
    for s in range(S):
        for lp in loops + [whole]:
            lp.period()
    torch.cuda.synchronize()
    for k in native.FB_STATE_KEYS:
        got = torch.cat([lp.state[k] for lp in loops]).cpu().numpy()
        assert np.isfinite(got).all(), k
        np.testing.assert_array_equal(got, whole.state[k].cpu().numpy(), err_msg=k)
    assert (torch.cat([lp.tau_last for lp in loops]).abs() <= 80.0).all()
    with pytest.raises(ValueError):
        DL.ClosedLoop(handle, MODEL, plan, st, control="computed_torque")
