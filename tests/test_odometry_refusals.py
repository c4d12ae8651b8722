"""CPU test of section 13's C boundary: every refusal blf_schmitt_trigger_advance and
blf_legged_odometry_advance make before any HIP call, and their accepted empty-batch calls, as a call list
in the manner of tests/fb_refusal_calls.py: a fake non-null handle and fake array pointers that are never
dereferenced (no row passes the checks with a batch above zero).  The trigger parameters are host memory
the call reads, so they are real arrays."""
import ctypes

import numpy as np
import pytest

from blf import native

FAKE_HANDLE, FAKE = 1, 8
INVALID, UNSUPPORTED = 1, 3
MODEL_ARRAYS = ("parent", "joint_origin", "joint_rot", "joint_axis", "link_mass", "link_com", "link_inertia",
                "frame_link", "frame_pose")
GOOD = [10.0, 4.0, 0.0, 0.0]


def _model(**over):
    m = native.FbModel()
    m.ndof, m.nframes = 3, 2
    for k in MODEL_ARRAYS:
        setattr(m, k, FAKE)
    for k, v in over.items():
        setattr(m, k, v)
    return m


def _call(entry, **over):
    """The accepted empty-batch call of `entry` with the arguments in `over` replaced; params: a list of rows."""
    args = {"handle": FAKE_HANDLE, "ncontacts": 2, "params": [GOOD, GOOD], "steps": 1, "fb_model": _model()}
    args.update(over)
    prm = args["params"]
    keep = None if prm is None else np.ascontiguousarray(prm, dtype=np.float64)
    actual = []
    for name, kind in native.SIGNATURES[entry][1]:
        if name == "params":
            actual.append(None if keep is None else ctypes.c_void_p(keep.ctypes.data))
        elif name == "fb_model":
            actual.append(None if args[name] is None else ctypes.byref(args[name]))
        elif kind is ctypes.c_void_p:
            v = args.get(name, None if name in ("stream", "joint_vel") else FAKE)
            actual.append(None if v is None else ctypes.c_void_p(v))
        else:
            actual.append(int(args.get(name, 0)))
    status = getattr(native.lib(), entry)(*actual)
    return status, (native.last_error() if status else None)


BOTH = ("blf_schmitt_trigger_advance", "blf_legged_odometry_advance")
nan, inf = float("nan"), float("inf")
COMMON = [
    (dict(handle=None), INVALID, "null handle"),
    (dict(steps=0), INVALID, "steps=0"),
    (dict(batch=-1), INVALID, "negative batch"),
    (dict(params=None), INVALID, "null params"),
    (dict(ncontacts=0), UNSUPPORTED, "ncontacts=0"),
    (dict(ncontacts=9, params=[GOOD] * 9), UNSUPPORTED, "ncontacts=9"),
    (dict(ncontacts=9, params=[[nan, 0, 0, 0]] * 9), UNSUPPORTED, "ncontacts=9"),   # the count is checked first
    (dict(params=[GOOD, [nan, 4.0, 0.0, 0.0]]), INVALID, "params[1] holds a threshold or delay that is not finite"),
    (dict(params=[[10.0, -inf, 0.0, 0.0], GOOD]), INVALID, "params[0] holds a threshold"),
    (dict(params=[GOOD, [10.0, 4.0, inf, 0.0]]), INVALID, "not finite"),
    (dict(params=[GOOD, [10.0, 4.0, 0.0, nan]]), INVALID, "not finite"),
    (dict(params=[GOOD, [10.0, 4.0, -0.5, 0.0]]), INVALID, "negative delay"),
    (dict(params=[GOOD, [10.0, 4.0, 0.0, -1e-9]]), INVALID, "negative delay"),
    (dict(params=[[4.0, 10.0, 0.0, 0.0], GOOD]), INVALID, "on_threshold=4 below off_threshold=10"),
    (dict(time=None), INVALID, "null time"),
    # shared parameters: row 0 alone is read
    (dict(shared_params=1, params=[[10.0, 4.0, 0.0, -1.0]]), INVALID, "params[0] holds a negative delay"),
]
TRIGGER = [
    (dict(batch=1, value=None), INVALID, "null value"),
    (dict(batch=1, state=None), INVALID, "null state"),
    (dict(batch=1, timers=None), INVALID, "null timers"),
]
ODOMETRY = [
    (dict(reserved=1), INVALID, "reserved must be 0"),
    (dict(fb_model=None), INVALID, "null model"),
    (dict(fb_model=_model(ndof=0)), UNSUPPORTED, "ndof=0"),
    (dict(fb_model=_model(ndof=49)), UNSUPPORTED, "ndof=49"),
    (dict(fb_model=_model(joint_axis=None)), INVALID, "null model array"),
    (dict(frames=None), INVALID, "null frame buffer"),
    (dict(fb_model=_model(frame_pose=None)), INVALID, "null frame buffer"),
    (dict(fb_model=_model(nframes=0)), INVALID, "null frame buffer"),
    (dict(batch=1, joint_pos=None), INVALID, "null joint_pos"),
    (dict(batch=1, normal_force=None), INVALID, "null normal_force"),
    (dict(batch=1, trig_state=None), INVALID, "null estimator state"),
    (dict(batch=1, trig_timers=None), INVALID, "null estimator state"),
    (dict(batch=1, fixed_frame=None), INVALID, "null estimator state"),
    (dict(batch=1, fixed_pose=None), INVALID, "null estimator state"),
    (dict(batch=1, base_pos=None, base_rot=None, base_vel=None, contact_out=None, fixed_out=None, status=None),
     INVALID, "no output requested"),
]
CALLS = [(e, *row) for e in BOTH for row in COMMON] + [(BOTH[0], *row) for row in TRIGGER] + \
        [(BOTH[1], *row) for row in ODOMETRY]


@pytest.mark.parametrize("entry,over,status,fragment", CALLS,
                         ids=[f"{e.split('_')[1]}-{i}" for i, (e, *_) in enumerate(CALLS)])
def test_refusal(entry, over, status, fragment):
    got, message = _call(entry, **over)
    assert got == status, (got, message)
    assert message.startswith(entry + ": ") and fragment in message, message


@pytest.mark.parametrize("entry", BOTH)
def test_empty_batch_is_accepted(entry):
    assert _call(entry) == (0, None)
    assert _call(entry, shared_params=1, params=[GOOD]) == (0, None)
    # nothing but the handle, the parameters, the clock (and the model with its frames) is needed for it
    nulls = {k: None for k in ("value", "state", "timers", "state_out", "joint_pos", "normal_force", "trig_state",
                                "trig_timers", "fixed_frame", "fixed_pose", "base_pos", "base_rot", "base_vel",
                                "contact_out", "fixed_out", "status")}
    assert _call(entry, **nulls) == (0, None)
