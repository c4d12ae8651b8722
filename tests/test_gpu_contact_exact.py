"""The device's ContinuousContactModel against an exact quadrature of the model's point law.

tests/test_gpu_contact.py proves that the kernels equal the oracle; this module ties them to the
truth.  tests/golden/contact_exact.npz holds 80 contacts in eight pose families (generic,
non-orthonormal rotations, a sole on edge with R22 == 0 and +-1e-9, stiff soles 8 km from the
origin, a nearly flat sole, the rest pose, shared parameters) with every output of the model
computed by tests/contact_exact.py: the point law of ContinuousContactModel.cpp:173-221 integrated
over the sole with a 3 x 3 Gauss-Legendre rule, exact for it, in mpmath at 50 digits.  Only the
fixture is read here; mpmath is not needed.

The bar is contact_exact.block_err <= 1e-14: per force / torque block relative to the block's
largest entry, and exact zeros where the truth is zero.

Measured on an MI355X, worst block_err per family and output: the device against the fixture's
doubles | the oracle as the fixture records it (`oracle_err`, measured by the generating script
against the unrounded 50-digit values, hence the small differences: the two sides are built
without FMA contraction in one expression order, and against the fixture's doubles the oracle
gives the device's figures to the digit, tests/test_contact_exact.py):

               wrench              autonomous          control             regressor
    generic    4.10e-16 | 3.76e-16  1.38e-15 | 1.38e-15  3.22e-16 | 2.92e-16  3.33e-16 | 2.69e-16
    nonortho   3.45e-16 | 3.97e-16  3.25e-16 | 2.64e-16  3.00e-16 | 2.59e-16  4.26e-16 | 4.95e-16
    zero22     0        | 0         4.07e-16 | 4.41e-16  0        | 0         0        | 0
    tiny22     3.51e-16 | 3.02e-16  4.60e-16 | 3.87e-16  2.50e-16 | 2.42e-16  2.29e-16 | 1.74e-16
    stiff_far  1.89e-16 | 2.37e-16  3.81e-16 | 3.74e-16  3.57e-16 | 2.92e-16  2.84e-16 | 2.58e-16
    flat       4.14e-16 | 4.02e-16  2.85e-16 | 2.52e-16  3.53e-16 | 2.77e-16  4.78e-16 | 4.11e-16
    rest       0        | 0         0        | 0         3.73e-16 | 3.47e-16  0        | 0
    shared     2.20e-16 | 3.09e-16  2.80e-16 | 2.79e-16  4.02e-16 | 3.71e-16  4.60e-16 | 5.12e-16

               point force         point torque
    generic    4.03e-16 | 3.86e-16  1.04e-15 | 1.11e-15
    nonortho   2.13e-16 | 1.88e-16  7.30e-16 | 7.33e-16
    zero22     3.15e-16 | 2.59e-16  5.75e-16 | 5.98e-16
    tiny22     3.49e-16 | 3.87e-16  8.38e-16 | 8.10e-16
    stiff_far  2.37e-16 | 2.57e-16  4.77e-16 | 4.57e-16
    flat       1.48e-16 | 1.28e-16  3.39e-16 | 2.99e-16
    rest       0        | 0         0        | 0
    shared     5.30e-16 | 4.95e-16  6.45e-16 | 6.49e-16

The Gauss sum of the device's point law against the device's wrench: 5.3e-16 at worst (flat).
"""
import os

import numpy as np
import pytest
import torch

import contact_exact as CE
import rls_reference as R
from blf import native, robot
from gpu_util import to_device as _d

pytestmark = pytest.mark.gpu

BAR = 1e-14
OUTPUTS = ("wrench", "autonomous", "control", "regressor")
PER_FAMILY = 10
FX = {k: v for k, v in np.load(os.path.join(os.path.dirname(__file__), "golden",
                                            "contact_exact.npz")).items()}
FAMILIES = [str(f) for f in FX["families"]]
INPUTS = ("prm", "twist", "pose", "null")


def _d_unaligned(a):
    """The same values at a device address 8 bytes past a 16-byte boundary."""
    a = np.array(a, dtype=np.float64, order="C")
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


def _rows(name):
    i = FAMILIES.index(name)
    return slice(i * PER_FAMILY, (i + 1) * PER_FAMILY)


@pytest.fixture(scope="module")
def clean(handle):
    """One launch on all 80 contacts with per-contact parameters; shared, never written to."""
    out = handle.contact_model_eval(*[_d(FX[k]) for k in INPUTS])
    return {k: v.cpu().numpy() for k, v in out.items()}


def _table(worst, cols):
    print(f"\n{'':10s}" + "".join(f"{k:>12s}" for k in cols))
    for i, name in enumerate(FAMILIES):
        print(f"{name:10s}" + "".join(f"{e:12.2e}" for e in worst[i]))


def test_contact_model_eval_against_the_exact_quadrature(clean):
    worst = np.zeros((len(FAMILIES), 4))
    for n, k in enumerate(OUTPUTS):
        for q in range(80):
            worst[q // PER_FAMILY, n] = max(worst[q // PER_FAMILY, n],
                                            CE.block_err(clean[k][q], FX[k][q]))
    _table(worst, OUTPUTS)
    print("oracle (fixture):")
    _table(FX["oracle_err"][:, :4], OUTPUTS)
    assert worst.max() <= BAR, worst


def test_shared_parameters_against_the_exact_quadrature(handle, clean):
    rows = _rows("shared")
    assert (FX["prm"][rows] == FX["prm"][rows][0]).all()
    out = handle.contact_model_eval(_d(FX["prm"][rows][0]), *[_d(FX[k][rows]) for k in INPUTS[1:]])
    for k in OUTPUTS:
        got = out[k].cpu().numpy()
        assert CE.batch_block_err(got, FX[k][rows]) <= BAR, k
        np.testing.assert_array_equal(got, clean[k][rows], err_msg=k)   # one law on both paths


def test_unaligned_buffers_give_the_same_bits(handle, clean):
    """Inputs 8 B past a 16-B boundary take the tile load's element-wise path."""
    out = handle.contact_model_eval(_d(FX["prm"]), *[_d_unaligned(FX[k]) for k in INPUTS[1:]])
    for k in OUTPUTS:
        np.testing.assert_array_equal(out[k].cpu().numpy(), clean[k], err_msg=k)


def test_a_poisoned_contact_stays_in_its_row(handle, clean):
    """NaN in the pose of contact 63 (its R22, which every output reads) and in the twist of
    contact 64, the two sides of the tile edge.  Every entry that reads the poisoned input is NaN:
    all of the wrench and of the autonomous dynamics of both, the regressor of 63 and the damper
    column of 64, the model entries of 63's control matrix.  The control matrix and the regressor's
    spring column do not read the twist (ContinuousContactModel.cpp:165-170, :240-248), so for
    contact 64 they are the clean bits.  The other 78 contacts are bit-identical to the clean
    call."""
    twist, pose = FX["twist"].copy(), FX["pose"].copy()
    pose[63, 11] = np.nan
    twist[64, :] = np.nan
    out = handle.contact_model_eval(_d(FX["prm"]), _d(twist), _d(pose), _d(FX["null"]))
    out = {k: v.cpu().numpy() for k, v in out.items()}
    keep = np.ones(80, dtype=bool)
    keep[[63, 64]] = False
    for k in OUTPUTS:
        np.testing.assert_array_equal(out[k][keep], clean[k][keep], err_msg=k)
    for q in (63, 64):
        assert np.isnan(out["wrench"][q]).all() and np.isnan(out["autonomous"][q]).all(), q
    assert np.isnan(out["regressor"][63]).all()
    model = np.zeros((6, 6), dtype=bool)
    model[:3, :3] = np.eye(3, dtype=bool)
    model[3:, 3:] = True
    assert np.isnan(out["control"][63][model]).all()
    assert (out["control"][63][~model] == 0.0).all()
    assert np.isnan(out["regressor"][64][:, 1]).all()
    np.testing.assert_array_equal(out["regressor"][64][:, 0], clean["regressor"][64][:, 0])
    np.testing.assert_array_equal(out["control"][64], clean["control"][64])


@pytest.fixture(scope="module")
def points(handle):
    """blf_contact_point_wrench on the 16 x 18 fixture points, one launch."""
    pc = FX["point_contact"]
    f, t = handle.contact_point_wrench(*[_d(FX[k][pc]) for k in INPUTS], _d(FX["points"]))
    return f.cpu().numpy(), t.cpu().numpy()


def test_point_law_against_the_exact_values(points):
    f, t = points
    worst = np.zeros((len(FAMILIES), 2))
    for i, q in enumerate(FX["point_contact"]):
        fam = q // PER_FAMILY
        worst[fam, 0] = max(worst[fam, 0], CE.batch_block_err(f[i], FX["point_force"][i]))
        worst[fam, 1] = max(worst[fam, 1], CE.batch_block_err(t[i], FX["point_torque"][i]))
    _table(worst, ("point f", "point t"))
    print("oracle (fixture):")
    _table(FX["oracle_err"][:, 4:], ("point f", "point t"))
    assert worst.max() <= BAR, worst
    # the edge rule is > : the corners are inside, one ulp past an edge is outside
    assert not f[:, CE.OUTSIDE].any() and not t[:, CE.OUTSIDE].any()
    assert not np.signbit(f[:, CE.OUTSIDE]).any() and not np.signbit(t[:, CE.OUTSIDE]).any()
    rest = FAMILIES.index("rest")
    for i, q in enumerate(FX["point_contact"]):
        if q // PER_FAMILY != rest:
            assert f[i, CE.CORNERS].any(axis=1).all() and t[i, CE.CORNERS].any(axis=1).all(), q


def gauss_wrench(prm, pose, f, t):
    """|R22| sum_ij w_i w_j (L W / 4) (f_ij, t_ij) over the nine Gauss nodes (the order of
    contact_exact.fixture_points), in long double: [..., 9, 3] twice -> [..., 6]."""
    w = np.outer(CE.GAUSS_W, CE.GAUSS_W).reshape(-1).astype(np.longdouble)
    ft = np.concatenate([f, t], axis=-1).astype(np.longdouble)
    L, W = prm[..., 0].astype(np.longdouble), prm[..., 1].astype(np.longdouble)
    s = np.abs(pose[..., 11].astype(np.longdouble)) * (L * W / 4)
    return (w[:, None] * ft).sum(axis=-2) * s[..., None]


def test_wrench_is_the_gauss_sum_of_the_device_point_law(points, clean):
    """The reference test's Monte Carlo property (1e-2, tests/test_gpu_contact.py) made exact: the
    rule integrates the point law without error, so the sum of the device's own point forces and
    torques is the device's wrench up to the rounding of the nine doubles that enter it."""
    f, t = points
    pc = FX["point_contact"]
    got = gauss_wrench(FX["prm"][pc], FX["pose"][pc], f[:, CE.NODES], t[:, CE.NODES])
    errs = [CE.block_err(clean["wrench"][q], got[i]) for i, q in enumerate(pc)]
    print("\ngauss sum vs wrench:", " ".join(f"{e:.1e}" for e in errs))
    assert max(errs) <= BAR, errs


def test_contact_rls_on_the_degenerate_families(handle, oracle):
    """blf_contact_rls_advance, T = 3, on the soles on edge, the rest pose and the stiff far
    soles: bit for bit against rls_reference.advance fed the oracle's regressors.  On zero22 the
    regressor is exactly zero, so the filter keeps its state and only forgets: P = P0 / lam^3."""
    names = ("zero22", "tiny22", "rest", "stiff_far")
    idx = np.concatenate([np.arange(80)[_rows(n)] for n in names])
    B, T, lam = len(idx), 3, 0.98
    geometry, null = FX["prm"][idx, :2], FX["null"][idx]
    twist = np.stack([FX["twist"][idx] * s for s in (1.0, -0.5, 0.25)])
    pose = np.stack([FX["pose"][idx]] * T)
    prm = np.concatenate([geometry, np.ones((B, 2))], axis=1)
    H = np.stack([oracle.contact_eval_batch(prm, twist[t], pose[t], null)[3] for t in range(T)])
    rs = np.random.RandomState(5)
    wrench = np.einsum("tbmn,bn->tbm", H, FX["prm"][idx, 2:]) + rs.standard_normal((T, B, 6))
    r = rs.uniform(0.1, 1.0, (B, 6))
    x0 = np.stack([np.full(B, 1000.0), np.full(B, 100.0)], axis=1)
    P0 = np.broadcast_to(np.diag([1e6, 1e4]), (B, 2, 2)).copy()
    xr, Pr = R.advance(H, wrench, x0, P0, r, lam)
    x, P = _d(x0), _d(P0)
    handle.contact_rls_advance(_d(geometry), _d(twist), _d(pose), _d(null), _d(wrench), x, P,
                               _d(r), lam=lam)
    x, P = x.cpu().numpy(), P.cpu().numpy()
    np.testing.assert_array_equal(x, xr)
    np.testing.assert_array_equal(P, Pr)
    z = slice(0, PER_FAMILY)                            # zero22 comes first in `names`
    assert not H[:, z].any()
    np.testing.assert_array_equal(x[z], x0[z])
    np.testing.assert_array_equal(P[z], ((P0[z] / lam) / lam) / lam)
    assert np.isfinite(x).all() and np.isfinite(P).all()


def test_fbd_in_kernel_law_equals_the_gauss_sum_of_the_point_law(handle):
    """The in-kernel contact law of blf_fbd_dynamics against the quadrature of the point law,
    after test_fbd_given_wrench_of_the_continuous_model_equals_the_continuous_law: the soles'
    state from blf_fb_frame_state, the point law on the device at the nine Gauss nodes, their
    Gauss sum as a given wrench.  The base is rolled by 1.45 rad, which puts the soles of the
    three robots on both sides of R22 = 0 (asserted), where the law carries |R22|."""
    from scipy.spatial.transform import Rotation as Rot
    model = robot.humanoid24()
    B, C = 3, 2
    st = robot.random_states(model, B, seed=31)
    st["base_rot"] = Rot.from_euler("x", 1.45).as_matrix() @ st["base_rot"]
    rng = np.random.default_rng(6)
    params = np.array([[0.12, 0.09, 3.0e4, 300.0]] * C)
    null = np.zeros((B, C, 12))
    null[:, :, :3] = rng.normal(size=(B, C, 3)) * 0.01
    null[:, :, 3:] = np.eye(3).reshape(-1)
    dev = dict(frame=_d(np.array([0, 1], dtype=np.int32), torch.int32), params=_d(params),
               null_pose=_d(null))
    dm = handle.fb_model(model)
    dst = {k: _d(st[k]) for k in native.FB_STATE_KEYS}
    tau = _d(st["joint_torque"])
    pose, twist = handle.fb_frame_state(dm, dst, dev["frame"])
    r22 = pose.cpu().numpy().reshape(B * C, 12)[:, 11]
    assert (r22 < 0).any() and (r22 > 0).any(), r22
    assert (np.sign(r22.reshape(B, C)[:, 0]) != np.sign(r22.reshape(B, C)[:, 1])).any(), r22
    prm = np.tile(params, (B, 1))
    pts = np.stack([CE.fixture_points(L, W)[CE.NODES] for L, W in prm[:, :2]])
    f, t = handle.contact_point_wrench(_d(prm), twist.reshape(B * C, 6).contiguous(),
                                       pose.reshape(B * C, 12).contiguous(),
                                       dev["null_pose"].reshape(B * C, 12).contiguous(), _d(pts))
    w = gauss_wrench(prm, pose.cpu().numpy().reshape(B * C, 12), f.cpu().numpy(), t.cpu().numpy())
    law = _d(np.array([native.CONTACT_WRENCH] * C, dtype=np.int32), torch.int32)
    given = dict(dev, law=law, wrench=_d(w.astype(np.float64).reshape(B, C, 6)))
    a = handle.fbd_dynamics(dm, dst, tau, contacts=dev)
    b = handle.fbd_dynamics(dm, dst, tau, contacts=given)
    none = handle.fbd_dynamics(dm, dst, tau)
    for k in ("base_vel", "joint_vel"):
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert np.abs(x - y).max() <= 1e-12 * max(1.0, np.abs(x).max()), k
        # the contacts matter at this state: without them the accelerations are others
        assert np.abs(x - none[k].cpu().numpy()).max() > 1e-3 * max(1.0, np.abs(x).max()), k
