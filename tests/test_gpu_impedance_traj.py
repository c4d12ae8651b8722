"""GPU tests of blf_fbd_euler_integrate_impedance_traj (include/blf/blf_c.h section 9): the joint impedance
whose reference changes inside the launch, against blf_fbd_euler_integrate_impedance (bit for bit where
the two are the same arithmetic) and against tests/closed_loop_ik_reference.py (1e-9 relative per state
key, the bar of test_fbd_euler_impedance_vs_oracle).  Cases: tests/impedance_traj_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import impedance_traj_cases as TC
from blf import native
from gpu_util import assert_bitwise, rel_err, to_device as _d

pytestmark = pytest.mark.gpu
TOL = 1e-9
T0, T1, DT = TC.T0, TC.T1, TC.DT


def dev_case(handle, cid, B):
    cs = TC.build_case(cid)
    ct = cs["contacts"]
    contacts = dict(frame=_d(ct["frame"], torch.int32), params=_d(ct["params"]), null_pose=_d(ct["null_pose"][:B]))
    return dict(dm=handle.fb_model(cs["model"]), state={k: _d(cs["states"][k][:B]) for k in native.FB_STATE_KEYS},
                contacts=contacts, imp=handle.joint_impedance(cs["kp"], cs["kd"]))


def run_traj(handle, cid, B, q_ref, sps, nu=None, q_bias=None, mass_reg=None):
    """The trajectory call on robots 0 .. B - 1 of the case; the final state as host arrays."""
    d = dev_case(handle, cid, B)
    tr = handle.joint_impedance_traj(d["imp"], _d(q_ref), sps, qd_ref=None if nu is None else _d(nu), qd_offset=6,
                                     q_bias=None if q_bias is None else _d(q_bias))
    handle.fbd_euler_integrate_impedance_traj(d["dm"], d["state"], tr, T0, T1, DT, contacts=d["contacts"],
                                              mass_reg=None if mass_reg is None else _d(mass_reg))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d["state"].items()}


def run_held(handle, cid, B, q_ref, mass_reg=None):
    d = dev_case(handle, cid, B)
    handle.fbd_euler_integrate_impedance(d["dm"], d["state"], d["imp"], _d(q_ref), T0, T1, DT, contacts=d["contacts"],
                                         mass_reg=None if mass_reg is None else _d(mass_reg))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d["state"].items()}


def assert_close(got, ref, what):
    for i, r in enumerate(ref):
        for k in native.FB_STATE_KEYS:
            e = rel_err(got[k][i], r[k])
            print(what, "robot", i, k, "rel err %.3g" % e)
            assert e <= TOL, (what, i, k, e)


@pytest.mark.parametrize("cid,B,reg", [("h24", 1, False), ("h24", 2, False), ("h24", 3, False), ("n48", 2, False),
                                       ("h24", 2, True)])
def test_e1_identical_slices_equal_held_reference_bitwise(handle, cid, B, reg):
    """E1: T = 3 identical slices, steps_per_slice = 4, no qd_ref, no bias: the held-reference call with
    that q_ref, bit for bit (the odd batch, the pair, one system per wavefront, and with mass_reg = zeros
    the mass-matrix instantiation)."""
    q = TC.references(cid, B, 1)["q_ref"][0]
    n = q.shape[1]
    mass_reg = np.zeros((n + 6, n + 6)) if reg else None
    held = run_held(handle, cid, B, q, mass_reg=mass_reg)
    traj = run_traj(handle, cid, B, np.repeat(q[None], 3, axis=0), 4, mass_reg=mass_reg)
    assert all(np.isfinite(v).all() for v in held.values())
    assert np.abs(held["joint_pos"] - TC.build_case(cid)["states"]["joint_pos"][:B]).max() > 0.0
    assert_bitwise(traj, held)


@pytest.mark.parametrize("cid,B", [("h24", 3), ("n48", 2), ("h24p", 3)])
def test_parity_with_reference(handle, cid, B):
    """T = 4 distinct slices of 5 steps over the 19 steps, qd_ref through a nu_traj-shaped buffer
    (qd_stride = 6 + n) and q_bias given."""
    r = TC.references(cid, B, 4)
    got = run_traj(handle, cid, B, r["q_ref"], 5, nu=r["nu"], q_bias=r["q_bias"])
    assert_close(got, TC.reference(cid, B, 4, 5), cid)
    # the feed-forward and the bias are not no-ops
    plain = run_traj(handle, cid, B, r["q_ref"], 5)
    assert np.abs(plain["joint_vel"] - got["joint_vel"]).max() > 1e-6


@pytest.mark.parametrize("cid,B", [("h24", 3), ("n48", 2)])
def test_last_slice_is_held(handle, cid, B):
    """7a: T = 2, steps_per_slice = 3 over 19 steps: slice 1 from step 3 on.  Equal (1e-9) to the reference
    and to T = 7 with slices 1 .. 6 copies of slice 1."""
    q = TC.references(cid, B, 2)["q_ref"]
    got = run_traj(handle, cid, B, q, 3)
    assert_close(got, TC.reference(cid, B, 2, 3, full=False), cid + " held")
    q7 = np.concatenate([q[:1]] + [q[1:2]] * 6, axis=0)
    got7 = run_traj(handle, cid, B, q7, 3)
    for k in native.FB_STATE_KEYS:
        assert rel_err(got7[k], got[k]) <= TOL, k


@pytest.mark.parametrize("cid,B", [("h24", 3), ("n48", 2)])
def test_slices_past_the_last_used_are_not_read(handle, cid, B):
    """7b: T = 8, steps_per_slice = 5 over 19 steps uses slices 0 .. 3; slices 4 .. 7 full of NaN (q_ref and
    qd_ref) change nothing: the T = 4 run, bit for bit."""
    r = TC.references(cid, B, 4)
    got4 = run_traj(handle, cid, B, r["q_ref"], 5, nu=r["nu"], q_bias=r["q_bias"])
    nan = lambda a: np.concatenate([a, np.full_like(a, np.nan)], axis=0)
    got8 = run_traj(handle, cid, B, nan(r["q_ref"]), 5, nu=nan(r["nu"]), q_bias=r["q_bias"])
    assert all(np.isfinite(v).all() for v in got4.values())
    assert_bitwise(got8, got4)


@pytest.mark.parametrize("field", ["q_ref", "nu", "q_bias"])
def test_nan_reference_is_per_robot(handle, field):
    """8: a NaN in robot 1's slice 2 gives robot 1 a NaN state; robots 0 and 2 (its wavefront partner and
    the next wavefront) keep the clean run's bits."""
    r = TC.references("h24", 3, 4)
    clean = run_traj(handle, "h24", 3, r["q_ref"], 5, nu=r["nu"], q_bias=r["q_bias"])
    bad = {k: v.copy() for k, v in r.items()}
    if field == "q_bias":
        bad["q_bias"][1, 7] = np.nan
    else:
        bad[field][2, 1, 6 + 7 if field == "nu" else 7] = np.nan
    got = run_traj(handle, "h24", 3, bad["q_ref"], 5, nu=bad["nu"], q_bias=bad["q_bias"])
    for k in native.FB_STATE_KEYS:
        assert np.isnan(got[k][1]).all(), k
    assert_bitwise(got, clean, robots=[0, 2])


def test_call_level_errors(handle):
    """9: the refused calls return their codes and leave the state untouched."""
    B, cid = 2, "h24"
    cs, r = TC.build_case(cid), TC.references(cid, 2, 4)
    n = cs["model"]["n"]
    d = dev_case(handle, cid, B)
    q, nu = _d(r["q_ref"]), _d(r["nu"])
    before = {k: v.clone() for k, v in d["state"].items()}

    def call(t0=T0, t1=T1, dT=DT, state=True, contacts=True, **over):
        tr = handle.joint_impedance_traj(d["imp"], q, 5, qd_ref=nu, qd_offset=6)
        for k, v in over.items():
            setattr(tr.c, k, v)
        fs = handle._fb_state(d["state"], B, n)
        return native.lib().blf_fbd_euler_integrate_impedance_traj(
            handle._h, ctypes.byref(d["dm"].c), ctypes.byref(fs) if state else None, ctypes.byref(tr.c),
            ctypes.byref(handle._fb_contacts(d["contacts"] if contacts else None, B)), None, B, t0, t1, dT,
            native._stream(None))

    INVALID = 1
    for over in (dict(slices=0), dict(slices=-1), dict(steps_per_slice=0), dict(reserved=1), dict(qd_stride=n - 1),
                 dict(ndof=n + 1), dict(kp=None), dict(kd=None), dict(q_ref=None), dict(state=False)):
        assert call(**over) == INVALID, over
        assert "blf_fbd_euler_integrate_impedance_traj" in native.last_error(), over
    # the schedule's errors are the held-reference call's
    assert call(t0=1.0, t1=0.0) == 4 and call(dT=0.0) == 4 and call(t0=0.5, t1=0.5) == 5
    torch.cuda.synchronize()
    for k in native.FB_STATE_KEYS:
        assert torch.equal(d["state"][k], before[k]), k
    # qd_stride is not read without qd_ref, and the call itself goes through
    assert call(qd_ref=None, qd_stride=0) == 0
    torch.cuda.synchronize()
    assert not torch.equal(d["state"]["joint_pos"], before["joint_pos"])
    # an empty batch is no error
    assert native.lib().blf_fbd_euler_integrate_impedance_traj(
        handle._h, ctypes.byref(d["dm"].c), ctypes.byref(handle._fb_state(d["state"], B, n)),
        ctypes.byref(handle.joint_impedance_traj(d["imp"], q, 5).c), ctypes.byref(handle._fb_contacts(None, 0)),
        None, 0, T0, T1, DT, native._stream(None)) == 0
