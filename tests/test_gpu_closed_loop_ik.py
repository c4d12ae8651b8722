"""GPU tests of blf.closed_loop.ClosedLoop(reference="ik"): the plan's CoM schedule -> blf_fb_ik_track ->
the trajectory impedance, against tests/closed_loop_ik_reference.py's IkOracleLoop; the default mode
untouched; and the IK mode standing for ten periods."""
import numpy as np
import pytest
import torch

import closed_loop_ik_reference as IR
import ik_limits_reference as LR
from blf import closed_loop as DL
from blf import native, problems as P, robot as R
from gpu_util import rel_err

pytestmark = pytest.mark.gpu
MODEL = R.humanoid24()


def _setup(B, periods, seed=3):
    """test_closed_loop_vs_oracle's fixture."""
    N = 100
    plan = P.make_batch(B, horizon=N + periods, n_footsteps=8, seed=P.SEED, first_ds=periods + 10)
    return plan, R.standing_states(MODEL, B, seed=seed)


def com_error(loop):
    """|c_xy - c_ref| of every robot: the measured CoM of the state now against the loop's reference."""
    com, _ = loop.h.fb_dcm(loop.dm, loop.state, stream=loop.stream)
    torch.cuda.synchronize()
    return np.linalg.norm(com[:, :2].cpu().numpy() - loop.c_ref.cpu().numpy(), axis=1)


def test_ik_loop_vs_oracle(handle):
    """B = 3, three coupled periods, device against the CPU composition.  The default limits and seed keep
    every IK step of the reference at least LR.BAND = 1e-7 from a tie of the active-set rule (asserted
    below on the reference alone), so `iters` and `active` are comparable.
    Also printed (nothing asserted): |c_xy - c_ref| after the periods, IK mode and posture mode; on an
    MI355X 1.6 mm for each robot in IK mode and 1.2 - 1.4 mm in posture mode (against the IK loop's c_ref);
    the smallest margin met was 1.6e-3."""
    B, S = 3, 3
    plan, st = _setup(B, S)
    loop = DL.ClosedLoop(handle, MODEL, plan, st, reference="ik")
    ref = IR.IkOracleLoop(MODEL, plan, st, R.sole_null_poses(MODEL, st), R.posture_law_arrays(MODEL),
                          DL.CONTACT_PARAMS)
    assert loop.steps_per_slice == 5 and len(loop.steps) == 19 and loop.ik_steps == 4
    for s in range(S):
        out = loop.period()
        torch.cuda.synchronize()
        xi_init = loop.xi.cpu().numpy().copy()
        o = ref.period()
        np.testing.assert_array_equal(out["status"].cpu().numpy(), o["status"])
        assert (o["status"] == 0).all()
        for i, r in enumerate(o["track"]):
            assert r["status"] == LR.OK, (s, i)
            margin = min(x["margin"] for x in r["steps"])
            print("period", s, "robot", i, "IK iters", r["iters"], "margin %.3g" % margin)
            assert margin >= LR.BAND, (s, i, margin)
        assert (loop.ik_status.cpu().numpy() == LR.OK).all() and (loop.ik_fail_step.cpu().numpy() == -1).all()
        np.testing.assert_array_equal(loop.ik_iters.cpu().numpy(), [r["iters"] for r in o["track"]])
        np.testing.assert_array_equal(loop.ik_active.cpu().numpy(), [list(r["active"]) for r in o["track"]])
        assert np.abs(xi_init - o["xi_init"]).max() <= 1e-9, s
        assert np.abs(out["vrp"].cpu().numpy() - o["vrp"]).max() <= 1e-8, s
        assert np.abs(out["xi"].cpu().numpy() - o["xi"]).max() <= 1e-8, s
        for k in native.FB_STATE_KEYS:
            e = rel_err(loop.state[k].cpu().numpy(), ref.state[k])
            print("period", s, k, "rel err %.3g" % e)
            assert e <= 1e-8, (s, k, e)
        for k in ref.kin:
            assert rel_err(loop.ik_state[k].cpu().numpy(), ref.kin[k]) <= 1e-9, (s, k)
        assert rel_err(loop.c_ref.cpu().numpy(), o["c_ref"]) <= 1e-12, s
        jt = np.stack([r["joint_traj"] for r in o["track"]], axis=1)
        assert rel_err(loop.joint_traj.cpu().numpy(), jt) <= 1e-9, s
    posture = DL.ClosedLoop(handle, MODEL, plan, st)
    for s in range(S):
        posture.period()
    posture.c_ref = loop.c_ref
    print("CoM tracking error |c_xy - c_ref| after", S, "periods [m]: ik", com_error(loop), "posture", com_error(posture))


def test_default_mode_is_untouched(handle):
    """ClosedLoop(...) and ClosedLoop(..., reference="posture"): the same states and plans, bit for bit."""
    B, S = 6, 3
    plan, st = _setup(B, S)
    a = DL.ClosedLoop(handle, MODEL, plan, st)
    b = DL.ClosedLoop(handle, MODEL, plan, st, reference="posture")
    assert a.reference == "posture" and not hasattr(a, "traj")
    for s in range(S):
        oa, ob = a.period(), b.period()
        torch.cuda.synchronize()
        for k in ("xi", "vrp", "status", "iters"):
            np.testing.assert_array_equal(oa[k].cpu().numpy(), ob[k].cpu().numpy(), err_msg=k)
        np.testing.assert_array_equal(a.q_ref.cpu().numpy(), b.q_ref.cpu().numpy())
    for k in native.FB_STATE_KEYS:
        np.testing.assert_array_equal(a.state[k].cpu().numpy(), b.state[k].cpu().numpy(), err_msg=k)
    with pytest.raises(ValueError):
        DL.ClosedLoop(handle, MODEL, plan, st, reference="other")
    with pytest.raises(ValueError):
        DL.ClosedLoop(handle, MODEL, plan, st, ik=dict(steps=2))


def test_ik_mode_stands(handle):
    """B = 6 standing for ten periods with the defaults (lean=True, steps=4): every plan solved, every IK
    status OK, every state finite at each period; and the joint references move, between the slices of a
    period and between periods.  No tracking number is asserted."""
    B, S = 6, 10
    plan, st = _setup(B, S)
    loops = DL.split_groups(handle, MODEL, plan, st, 2, reference="ik", ik=dict(steps=4, lean=True))
    assert [lp.B for lp in loops] == [3, 3] and all(lp.reference == "ik" for lp in loops)
    prev = None
    for s in range(S):
        outs = [lp.period() for lp in loops]
        torch.cuda.synchronize()
        for lp, out in zip(loops, outs):
            assert (out["status"].cpu().numpy() == 0).all(), (s, out["status"])
            assert (lp.ik_status.cpu().numpy() == LR.OK).all(), (s, lp.ik_status, lp.ik_fail_step)
            for k in native.FB_STATE_KEYS:
                assert torch.isfinite(lp.state[k]).all(), (s, k)
        jt = torch.cat([lp.joint_traj for lp in loops], dim=1).cpu().numpy()
        assert np.abs(jt[1:] - jt[:-1]).max() > 0.0, s
        if prev is not None:
            assert np.abs(jt - prev).max() > 0.0, s
        prev = jt
    z = torch.cat([lp.state["base_pos"][:, 2] for lp in loops])
    print("base height after", S, "periods:", z.cpu().numpy())
    print("CoM tracking error |c_xy - c_ref| [m]:", np.concatenate([com_error(lp) for lp in loops]))
