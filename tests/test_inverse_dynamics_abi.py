"""CPU tests of the inverse-dynamics boundary (include/blf/blf_c.h sections 8b and 9): the header declares
blf_fb_inverse_dynamics and blf_fbd_euler_integrate_computed_torque_traj, the library exports them, the
refusals that need no device hold, and the closed loop accepts the computed-torque mode only over the IK
reference."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from blf import closed_loop as DL
from blf import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "blf", "blf_c.h")
NEW = ("blf_fb_inverse_dynamics", "blf_fbd_euler_integrate_computed_torque_traj")
INVALID, UNSUPPORTED = 1, 3


def test_header_declares_and_library_exports_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(blf_[a-z0-9_]+)\s*\(", txt))
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (blf_[a-z0-9_]+)$", out, flags=re.M))
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in native.EXPORTED, name
    assert "typedef struct blf_computed_torque_traj" in txt


def _model(ndof=3):
    m = native.FbModel()
    m.ndof = ndof
    one = ctypes.c_void_p(8)   # never dereferenced: the refusals come first
    for k in ("parent", "joint_origin", "joint_rot", "joint_axis", "link_mass", "link_com", "link_inertia"):
        setattr(m, k, one)
    return m


def test_inverse_dynamics_refusals_without_a_device():
    L = native.lib()
    fake = ctypes.c_void_p(1)
    m, st, ct = _model(), native.FbState(), native.FbContacts()
    call = lambda h, mp, sp, batch, reserved: L.blf_fb_inverse_dynamics(
        h, mp, sp, None, None, ctypes.byref(ct), batch, None, None, None, None, reserved, None)
    assert call(None, ctypes.byref(m), ctypes.byref(st), 0, 0) == INVALID and "null handle" in native.last_error()
    assert call(fake, None, ctypes.byref(st), 0, 0) == INVALID
    assert call(fake, ctypes.byref(m), None, 0, 0) == INVALID
    assert call(fake, ctypes.byref(m), ctypes.byref(st), 0, 1) == INVALID and "reserved" in native.last_error()
    assert call(fake, ctypes.byref(m), ctypes.byref(st), -1, 0) == INVALID and "batch" in native.last_error()
    # null state buffers and a null required output with batch > 0
    assert call(fake, ctypes.byref(m), ctypes.byref(st), 2, 0) == INVALID
    for ndof in (0, 49):
        big = _model(ndof)
        assert call(fake, ctypes.byref(big), ctypes.byref(st), 0, 0) == UNSUPPORTED, ndof
        assert "ndof" in native.last_error()
    ct.ncontacts = 9
    assert call(fake, ctypes.byref(m), ctypes.byref(st), 0, 0) == UNSUPPORTED and "contacts" in native.last_error()
    ct.ncontacts = 0
    assert call(fake, ctypes.byref(m), ctypes.byref(st), 0, 0) == 0   # an empty batch is no error


def test_computed_torque_refusals_without_a_device():
    L = native.lib()
    fake = ctypes.c_void_p(1)
    m, st, ct = _model(), native.FbState(), native.FbContacts()
    one = ctypes.c_void_p(8)

    def law(**over):
        c = native.ComputedTorqueTraj()
        c.ndof, c.slices, c.steps_per_slice, c.reserved = 3, 2, 5, 0
        c.kp = c.kd = one
        for k, v in over.items():
            setattr(c, k, v)
        return c

    def call(c, h=fake, reg=None, batch=0):
        return L.blf_fbd_euler_integrate_computed_torque_traj(
            h, ctypes.byref(m), ctypes.byref(st), ctypes.byref(c) if c is not None else None, ctypes.byref(ct), reg,
            batch, 0.0, 0.019, 0.001, None)

    assert call(None) == INVALID and "null law" in native.last_error()
    assert call(law(reserved=1)) == INVALID and "reserved" in native.last_error()
    for over in (dict(slices=0), dict(steps_per_slice=0), dict(ndof=4), dict(kp=None), dict(kd=None),
                 dict(qd_ref=one, qd_stride=2), dict(qdd_ref=one, qdd_stride=2)):
        assert call(law(**over)) == INVALID, over
        assert "blf_fbd_euler_integrate_computed_torque_traj" in native.last_error()
    assert call(law(), h=None) == INVALID
    assert call(law(), batch=-1) == INVALID
    assert call(law(), reg=one) == UNSUPPORTED and "mass_reg" in native.last_error()
    assert call(law()) == 0   # an empty batch is no error


def test_closed_loop_accepts_computed_torque_over_the_ik_reference_only():
    plan = dict(dt=0.02, omega=np.zeros((1, 4)))
    for ref in ("posture",):
        with pytest.raises(ValueError, match="computed_torque"):
            DL.ClosedLoop(None, None, plan, None, reference=ref, control="computed_torque")
    with pytest.raises(ValueError, match="control"):
        DL.ClosedLoop(None, None, plan, None, control="pd")
    with pytest.raises(ValueError, match="computed_torque"):
        DL.ClosedLoop(None, None, plan, None, computed_torque=dict(freq=10.0))
