"""Helpers the tests/test_gpu_*.py files share: host arrays onto the device, the error metric, and
the refusal / bit-equality assertions.  It imports torch, so only test_gpu_*.py files import it.
Variants that do something else (a misaligned or always-copied device array, a state cut to the first
B robots, fb_models.rel_err's float) stay in the file that needs them."""
import numpy as np
import pytest
import torch

from blf import native


def to_device(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def rel_err(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def dev_state(states, rows=None):
    """The floating-base state arrays (of the robots `rows`) on the device."""
    rows = slice(None) if rows is None else rows
    return {k: to_device(states[k][rows]) for k in native.FB_STATE_KEYS}


def dev_tasks(handle, model, tasks, B):
    return handle.ik_tasks(B, model["n"], **tasks)


def dev_contacts(ct, B):
    """The first B systems of a case's contacts on the device; None for a case without contacts."""
    if ct is None:
        return None
    dev = dict(frame=to_device(ct["frame"], torch.int32), params=to_device(ct["params"]),
               null_pose=to_device(ct["null_pose"][:B]))
    if ct.get("law") is not None:
        dev.update(law=to_device(ct["law"], torch.int32), wrench=to_device(ct["wrench"][:B]))
    return dev


def raises(code, fn, *a, **kw):
    """fn(*a, **kw) raises native.BlfError with this status code."""
    with pytest.raises(native.BlfError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def assert_bitwise(a, b, robots=None):
    """Two states equal bit for bit in every key (of the robots `robots`)."""
    for k in native.FB_STATE_KEYS:
        x, y = (a[k], b[k]) if robots is None else (a[k][robots], b[k][robots])
        np.testing.assert_array_equal(x, y, err_msg=k)
