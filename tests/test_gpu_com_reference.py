"""GPU tests of blf_dcm_com_reference (include/blf/blf_c.h section 9b), the plan -> CoM set point map,
against tests/closed_loop_ik_reference.py at 1e-12 relative (the bar of test_fb_dcm_vs_oracle)."""
import ctypes

import numpy as np
import pytest
import torch

import closed_loop_ik_reference as IR
from blf import native
from gpu_util import rel_err, to_device as _d

pytestmark = pytest.mark.gpu
N, K, COL = 5, 7, 3   # vrp [B][N][2] and omega [B][K] read at column COL: both strided


def inputs(B, seed=0):
    rng = np.random.default_rng(seed)
    return dict(xi0=rng.normal(size=(B, 2)) * 0.05, vrp=rng.normal(size=(B, N, 2)) * 0.05,
                omega=np.sqrt(9.81 / rng.uniform(0.5, 0.6, (B, K))), z_ref=rng.uniform(0.5, 0.6, B),
                c_ref=rng.normal(size=(B, 2)) * 0.05)


def device_call(handle, a, T, dT, c_ref):
    pos, vel, xe = handle.dcm_com_reference(_d(a["xi0"]), _d(a["vrp"]), _d(a["omega"]), _d(a["z_ref"]), c_ref, T, dT,
                                            column=COL)
    torch.cuda.synchronize()
    return pos.cpu().numpy(), vel.cpu().numpy(), xe.cpu().numpy()


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("B", [1, 3, 130])
def test_com_reference_vs_reference(handle, B, T):
    """Two calls with c_ref carried on the device, against the numpy restatement carried the same way."""
    a, dT = inputs(B, seed=B + T), 0.02 / T
    c_dev, c_ref = _d(a["c_ref"]), a["c_ref"]
    for call in range(2):
        pos, vel, xe = device_call(handle, a, T, dT, c_dev)
        rp, rv, c_ref, rx = IR.com_reference(a["xi0"], a["vrp"][:, 0], a["omega"][:, COL], a["z_ref"], c_ref, T, dT)
        for name, got, ref in (("com_pos", pos, rp), ("com_vel", vel, rv), ("c_ref", c_dev.cpu().numpy(), c_ref),
                               ("xi_end", xe, rx)):
            assert rel_err(got, ref) <= 1e-12, (call, name)
        np.testing.assert_array_equal(pos[:, :, 2], np.repeat(a["z_ref"][:, None], T, axis=1))
        assert (vel[:, :, 2] == 0.0).all()
    assert np.abs(c_ref - a["c_ref"]).max() > 1e-6   # the reference moved


@pytest.mark.parametrize("field", ["xi0", "vrp", "omega", "z_ref", "c_ref"])
def test_non_finite_input_is_per_robot(handle, field):
    B, T, dT = 3, 4, 0.005
    a = inputs(B, seed=7)
    c_clean = _d(a["c_ref"])
    clean = device_call(handle, a, T, dT, c_clean) + (c_clean.cpu().numpy(),)
    bad = {k: v.copy() for k, v in a.items()}
    at = dict(xi0=(1, 0), vrp=(1, 0, 1), omega=(1, COL), z_ref=(1,), c_ref=(1, 1))[field]
    bad[field][at] = np.inf if field == "omega" else np.nan
    c_bad = _d(bad["c_ref"])
    got = device_call(handle, bad, T, dT, c_bad) + (c_bad.cpu().numpy(),)
    for g, c in zip(got, clean):
        assert np.isnan(g[1]).all()
        np.testing.assert_array_equal(g[[0, 2]], c[[0, 2]])
    # a NaN the call does not read (another knot's VRP, another omega column) changes nothing
    other = {k: v.copy() for k, v in a.items()}
    other["vrp"][1, 1:] = np.nan
    other["omega"][1, COL + 1] = np.nan
    c_o = _d(other["c_ref"])
    for g, c in zip(device_call(handle, other, T, dT, c_o) + (c_o.cpu().numpy(),), clean):
        np.testing.assert_array_equal(g, c)


def test_call_level_errors(handle):
    """Each refused call returns BLF_ERR_INVALID_ARGUMENT and writes nothing; batch == 0 is BLF_OK."""
    B, T = 3, 4
    a = inputs(B, seed=9)
    t = {k: _d(a[k]) for k in a}
    out = dict(com_pos=torch.full((B, T, 3), 7.0, dtype=torch.float64).cuda(),
               com_vel=torch.full((B, T, 3), 7.0, dtype=torch.float64).cuda(),
               xi_end=torch.full((B, 2), 7.0, dtype=torch.float64).cuda())
    c0 = t["c_ref"].clone()
    p = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(handle_=True, steps=T, dT=0.005, batch=B, vstride=2 * N, ostride=K, **null):
        g = lambda k, x: None if null.get(k) else p(x)
        return native.lib().blf_dcm_com_reference(
            handle._h if handle_ else None, g("xi0", t["xi0"]), g("vrp", t["vrp"]), vstride,
            g("omega0", t["omega"]), ostride, g("z_ref", t["z_ref"]), g("c_ref", t["c_ref"]), steps, dT, batch,
            g("com_pos", out["com_pos"]), g("com_vel", out["com_vel"]), g("xi_end", out["xi_end"]),
            native._stream(None))

    refused = [dict(handle_=False), dict(steps=0), dict(steps=-2), dict(dT=0.0), dict(dT=-0.005),
               dict(dT=float("nan")), dict(dT=float("inf")), dict(batch=-1), dict(vstride=1), dict(ostride=-1)]
    refused += [{k: True} for k in ("xi0", "vrp", "omega0", "z_ref", "c_ref", "com_pos", "com_vel")]
    for kw in refused:
        assert call(**kw) == 1, kw
        assert "blf_dcm_com_reference" in native.last_error(), kw
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in out.values())
    assert torch.equal(t["c_ref"], c0)
    assert call(batch=0) == 0
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in out.values()) and torch.equal(t["c_ref"], c0)
    # xi_end is optional
    assert call(xi_end=True) == 0
    torch.cuda.synchronize()
    assert bool((out["xi_end"] == 7.0).all()) and not bool((out["com_pos"] == 7.0).any())
    assert not torch.equal(t["c_ref"], c0)
