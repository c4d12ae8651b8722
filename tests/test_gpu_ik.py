"""GPU parity of blf_fb_ik_solve / blf_fb_ik_integrate (csrc/fb_ik.hip, include/blf/blf_c.h section
12) against tests/ik_reference.py over the cases of tests/ik_cases.py:

  sizes                       n = 1, 2, 3, 24, 48, and 26 | 27: the last size served two robots per
                              wavefront and the first served one
  topologies                  chain, star, random tree, a DFS-relabelled tree, prismatic joints at both
                              layouts with prismatic ancestors of the task frames
  task sets                   K = 0 with the CoM alone, K = 4 without it, K = 2 with it (and the
                              humanoid's standing set), a frame on the base link, two tasks on one
                              frame, SO3-only and R3-only weights, the optional inputs given and NULL,
                              a desired rotation 3 rad from the current one
  batch                       1, 3, 130; nu and status written at odd offsets into larger tensors

Metric: fb_models.rel_err < 1e-9 on nu (and on every state key after an integration) against the
reference, whose own plain-Cholesky solve is within 1e-10 of its refined one on every case
(tests/test_ik_reference.py).  The backward error |H nu - g| / (|H||nu| + |g|) of the device's nu in
the reference's (H, g) is printed next to the reference Cholesky's own; no bound is set on it.

Measured on an MI355X (worst over the robots of a case): nu rel_err 8.1e-12 on chain48-k2com-far,
6.9e-12 on pri-chain26-k2com, 3.6e-12 on the 27-joint chains, at most 7e-13 on every other case (1e-15
at n = 1 and n = 3); state rel_err after 1, 2 and 20 integration steps at most 3.2e-11
(chain48-k2com-far, one step), 1.5e-11 on pri-chain26-k2com, below 6e-12 elsewhere.  Backward error of
the device's nu 2.6e-17 to 6.4e-16 (worst: star48-k0com), the reference Cholesky's own 5.6e-18 to
2.0e-16; the device's is at most 7.8 times the reference's on the same case (chain27-b130)."""
import numpy as np
import pytest
import torch

import fb_models as FM
import ik_cases as IC
import ik_reference as IK
from blf import native
from gpu_util import dev_state, dev_tasks, raises as _raises

pytestmark = pytest.mark.gpu
TOL = 1e-9
rel_err = FM.rel_err
DT = 0.01


def odd_outputs(B, NV):
    """nu [B, NV] and status [B] as views one element into larger, sentinel-filled buffers."""
    nb = torch.full((B * NV + 3,), -7.0, dtype=torch.float64, device="cuda")
    sb = torch.full((B + 3,), -7, dtype=torch.int32, device="cuda")
    return nb, nb[1:1 + B * NV].view(B, NV), sb, sb[1:1 + B]


def check_sentinels(nb, sb):
    assert nb[0].item() == -7.0 and (nb[-2:] == -7.0).all().item()
    assert sb[0].item() == -7 and (sb[-2:] == -7).all().item()


@pytest.mark.parametrize("cid", sorted(IC.CASES))
def test_ik_solve_vs_reference(handle, cid):
    """blf_fb_ik_solve of every robot of one case of the matrix against the reference."""
    cs = IC.build_case(cid)
    model, B = cs["model"], cs["B"]
    NV = model["n"] + 6
    dm = handle.fb_model(model)
    st = dev_state(cs["states"])
    before = {k: v.clone() for k, v in st.items()}
    nb, nu, sb, status = odd_outputs(B, NV)
    handle.fb_ik_solve(dm, st, dev_tasks(handle, model, cs["tasks"], B), nu=nu, status=status)
    torch.cuda.synchronize()
    check_sentinels(nb, sb)
    for k in st:   # the solve reads the state only
        assert torch.equal(st[k], before[k]), k
    got, ref = nu.cpu().numpy(), IC.reference(cid)
    assert (status.cpu().numpy() == IK.OK).all()
    worst = max(rel_err(got[i], ref[i][0]) for i in range(B))
    be_dev = max(FM.backward_error(ref[i][2], got[i], ref[i][3]) for i in range(B))
    be_ref = max(FM.backward_error(ref[i][2], IK.cholesky_solve(ref[i][2], ref[i][3]), ref[i][3]) for i in range(B))
    print(f"{cid}: nu rel_err {worst:.2e}, backward error device {be_dev:.2e} reference Cholesky {be_ref:.2e}")
    for i in range(B):
        assert rel_err(got[i], ref[i][0]) < TOL, (cid, i)


INTEGRATE_CASES = ["chain1-k2com", "star2-k0com", "rand24-k2com", "rand26-k4-same", "chain27-k2com",
                   "rand48-k4com-dfs", "pri-chain26-k2com", "pri-rand48-k2", "chain48-k2com-far"]


def run_integrate(handle, cs, steps, rows=None, states=None, tasks=None):
    model = cs["model"]
    states = cs["states"] if states is None else states
    tasks = cs["tasks"] if tasks is None else tasks
    st = dev_state(states, rows)
    B = st["joint_pos"].shape[0]
    _, nu, status = handle.fb_ik_integrate(handle.fb_model(model), st, dev_tasks(handle, model, tasks, B), steps, DT)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in st.items()}, nu.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("steps", [1, 2, 20])
@pytest.mark.parametrize("cid", INTEGRATE_CASES)
def test_ik_integrate_vs_reference(handle, cid, steps):
    """blf_fb_ik_integrate against the reference's loop (solve, one Euler step) on every state key."""
    cs = IC.build_case(cid)
    B = min(cs["B"], 3)
    got, nu, status = run_integrate(handle, cs, steps, slice(0, B), tasks=IK.tasks_rows(cs["tasks"], slice(0, B)))
    worst = 0.0
    for i in range(B):
        ref, rnu, rst = IK.integrate(cs["model"], cs["states"], cs["tasks"], i, steps, DT)
        assert status[i] == rst == IK.OK
        for k in native.FB_STATE_KEYS:
            e = rel_err(got[k][i], ref[k])
            worst = max(worst, e)
            assert e < TOL, (cid, steps, i, k, e)
        np.testing.assert_array_equal(nu[i, :6], got["base_vel"][i])
        np.testing.assert_array_equal(nu[i, 6:], got["joint_vel"][i])
    print(f"{cid} steps {steps}: state rel_err {worst:.2e}")


@pytest.mark.parametrize("cid", ["rand24-k2com", "rand26-k4-same", "chain27-k2com", "pri-rand48-k2",
                                 "humanoid-standing-b130"])
def test_ik_integrate_is_the_unfused_sequence(handle, cid):
    """20 fused steps equal, bit for bit, 20 x { blf_fb_ik_solve; blf_fbk_euler_integrate(0, dT, dT)
    with that nu } on every state key, nu and status."""
    cs = IC.build_case(cid)
    model, B, steps = cs["model"], cs["B"], 20
    n = model["n"]
    dm = handle.fb_model(model)
    tk = dev_tasks(handle, model, cs["tasks"], B)
    fused = dev_state(cs["states"])
    _, fnu, fstatus = handle.fb_ik_integrate(dm, fused, tk, steps, DT)
    un = dev_state(cs["states"])
    for _ in range(steps):
        nu, status = handle.fb_ik_solve(dm, un, tk)
        twist, jv = nu[:, :6].contiguous(), nu[:, 6:].contiguous()
        handle.fbk_euler_integrate(dm.c.rho, un["base_pos"], un["base_rot"], un["joint_pos"], twist, jv, 0.0, DT, DT)
    un["base_vel"], un["joint_vel"] = twist, jv
    torch.cuda.synchronize()
    assert (fstatus == 0).all().item() and (status == 0).all().item()
    for k in native.FB_STATE_KEYS:
        assert torch.equal(fused[k], un[k]), (cid, k)
    assert torch.equal(fnu, nu) and n + 6 == nu.shape[1]


def _nan_pose(tasks, i):
    pose = tasks["se3_pose"].copy()
    pose[i, -1, 7] = np.nan
    return dict(tasks, se3_pose=pose)


def _nan_joint_setpoint(tasks, i):
    q = tasks["joint_pos"].copy()
    q[i, 0] = np.inf
    return dict(tasks, joint_pos=q)


@pytest.mark.parametrize("cid", ["rand24-k2com", "chain27-k2com"])
@pytest.mark.parametrize("kind", ["nan-pose", "inf-joint-setpoint", "nan-state", "overflow"])
def test_ik_bad_robot_is_contained(handle, cid, kind):
    """One bad robot in the middle of the batch (robot 1 of 3; with two robots per wavefront it
    shares its wavefront with robot 0): the documented status and a NaN nu for it, and the robots on
    either side bit-identical to the run without it, in the solve and in a 3-step integration, which
    also leaves the bad robot's state as it was.  "overflow" is the robot that is not positive with
    finite inputs (base_rot scaled by 1e160: H overflows; tests/test_ik_reference.py shows the
    reference failing the same way)."""
    cs = IC.build_case(cid)
    model, B, bad = cs["model"], cs["B"], 1
    states, tasks = {k: v.copy() for k, v in cs["states"].items()}, cs["tasks"]
    want = IK.BAD_INPUT
    if kind == "nan-pose":
        tasks = _nan_pose(tasks, bad)
    elif kind == "inf-joint-setpoint":
        tasks = _nan_joint_setpoint(tasks, bad)
    elif kind == "nan-state":
        states["joint_pos"][bad, -1] = np.nan
    else:
        states["base_rot"][bad] = states["base_rot"][bad] * 1e160
        want = IK.NOT_POSITIVE
    assert IK.solve(model, states, tasks, bad)[1] == want   # the reference agrees on the status
    dm = handle.fb_model(model)
    good_nu, _ = handle.fb_ik_solve(dm, dev_state(cs["states"]), dev_tasks(handle, model, cs["tasks"], B))
    nu, status = handle.fb_ik_solve(dm, dev_state(states), dev_tasks(handle, model, tasks, B))
    status = status.cpu().numpy()
    assert status[bad] == want and torch.isnan(nu[bad]).all().item()
    for i in (0, 2):
        assert status[i] == IK.OK and torch.equal(nu[i], good_nu[i]), (kind, i)
    good_st, good_nu, _ = run_integrate(handle, cs, 3)
    st, nu, status = run_integrate(handle, cs, 3, states=states, tasks=tasks)
    assert status[bad] == want and np.isnan(nu[bad]).all()
    assert np.isnan(st["base_vel"][bad]).all() and np.isnan(st["joint_vel"][bad]).all()
    for k in IK.STATE_KEYS:   # frozen at the state before the failing (first) step
        np.testing.assert_array_equal(st[k][bad], states[k][bad], err_msg=k)
    for i in (0, 2):
        assert status[i] == IK.OK
        np.testing.assert_array_equal(nu[i], good_nu[i])
        for k in native.FB_STATE_KEYS:
            np.testing.assert_array_equal(st[k][i], good_st[k][i], err_msg=k)


@pytest.mark.parametrize("cid", ["rand24-k2com", "chain27-k2com"])
def test_ik_frame_index_out_of_range(handle, cid):
    """The frame indices are shared by the batch: one past the model's frames (or -1) makes every
    robot BLF_IK_BAD_INPUT with a NaN nu, reads nothing out of bounds and leaves the states alone."""
    cs = IC.build_case(cid)
    model, B = cs["model"], cs["B"]
    dm = handle.fb_model(model)
    for f in (len(model["frame_link"]), -1, 2 ** 30):
        tasks = dict(cs["tasks"], frame=np.array([1, f], dtype=np.int32))
        nu, status = handle.fb_ik_solve(dm, dev_state(cs["states"]), dev_tasks(handle, model, tasks, B))
        assert (status == IK.BAD_INPUT).all().item() and torch.isnan(nu).all().item()
        st, nu, status = run_integrate(handle, cs, 2, tasks=tasks)
        assert (status == IK.BAD_INPUT).all() and np.isnan(nu).all()
        for k in IK.STATE_KEYS:
            np.testing.assert_array_equal(st[k], cs["states"][k], err_msg=k)


def test_ik_unknown_joint_type(handle):
    """A joint_type that is neither revolute nor prismatic: every robot's nu is NaN."""
    cs = IC.build_case("pri-chain26-k2com")
    model, B = cs["model"], cs["B"]
    dm = handle.fb_model(model)
    dm.t["joint_type"][3] = 7   # (native.fb_model refuses it up front: set behind its back)
    nu, status = handle.fb_ik_solve(dm, dev_state(cs["states"]), dev_tasks(handle, model, cs["tasks"], B))
    assert torch.isnan(nu).all().item() and (status != IK.OK).all().item()


def test_ik_optional_outputs_and_empty_batch(handle):
    """status = NULL in both calls, nu = NULL in the integration, batch == 0."""
    cs = IC.build_case("rand24-k2com")
    model, B = cs["model"], cs["B"]
    dm = handle.fb_model(model)
    tk = dev_tasks(handle, model, cs["tasks"], B)
    nu, status = handle.fb_ik_solve(dm, dev_state(cs["states"]), tk, status=False)
    assert status is None and rel_err(nu.cpu().numpy()[0], IC.reference("rand24-k2com")[0][0]) < TOL
    full, fnu, _ = handle.fb_ik_integrate(dm, dev_state(cs["states"]), tk, 2, DT)
    st, nu, status = handle.fb_ik_integrate(dm, dev_state(cs["states"]), tk, 2, DT, nu=False, status=False)
    assert nu is None and status is None
    for k in native.FB_STATE_KEYS:
        assert torch.equal(st[k], full[k]), k
    empty = {k: v[:0] for k, v in dev_state(cs["states"]).items()}
    handle.fb_ik_solve(dm, empty, dev_tasks(handle, model, IK.tasks_rows(cs["tasks"], slice(0, 0)), 0))
    handle.fb_ik_integrate(dm, empty, dev_tasks(handle, model, IK.tasks_rows(cs["tasks"], slice(0, 0)), 0), 1, DT)


def test_ik_call_errors(handle):
    """Every call-level error of section 12, through the raw entry points where the wrapper would
    refuse first."""
    import ctypes
    INVALID, UNSUPPORTED = 1, 3
    cs = IC.build_case("rand24-k2com")
    model, B = cs["model"], cs["B"]
    n = model["n"]
    dm = handle.fb_model(model)
    st = dev_state(cs["states"])
    base = cs["tasks"]

    def solve(tasks=None, **over):
        tk = dev_tasks(handle, model, base if tasks is None else tasks, B)
        for k, v in over.items():
            setattr(tk.c, k, v)
        return handle.fb_ik_solve(dm, st, tk)

    def integrate(steps, dT, **over):
        tk = dev_tasks(handle, model, base, B)
        for k, v in over.items():
            setattr(tk.c, k, v)
        return handle.fb_ik_integrate(dm, {k: v.clone() for k, v in st.items()}, tk, steps, dT)

    solve()   # the unmodified call is fine
    _raises(INVALID, solve, reserved=1)
    _raises(UNSUPPORTED, solve, nse3=5)
    _raises(UNSUPPORTED, solve, nse3=-1)
    for field in ("frame", "se3_weight", "se3_kp", "se3_pose", "joint_weight", "joint_kp", "joint_pos", "com_pos"):
        _raises(INVALID, solve, **{field: None})
    _raises(INVALID, solve, base_damping=-1.0)
    _raises(INVALID, solve, base_damping=float("nan"))
    _raises(INVALID, solve, com_kp=float("inf"))
    for key, idx, val in (("se3_weight", (1, 4), -1.0), ("se3_weight", (0, 0), np.nan), ("se3_kp", (1, 1), np.inf),
                          ("se3_kp", (0, 0), -2.0), ("com_weight", (2,), -1e-3), ("com_weight", (0,), np.nan),
                          ("joint_weight", (n - 1,), 0.0), ("joint_weight", (0,), -1.0), ("joint_weight", (3,), np.inf),
                          ("joint_kp", (5,), -1.0), ("joint_kp", (n - 1,), np.nan)):
        a = np.array(base[key], dtype=np.float64, copy=True)
        a[idx] = val
        _raises(INVALID, solve, dict(base, **{key: a}))
    _raises(INVALID, integrate, 0, DT)
    _raises(INVALID, integrate, -3, DT)
    for dT in (0.0, -DT, float("nan"), float("inf")):
        _raises(INVALID, integrate, 1, dT)
    _raises(INVALID, integrate, 1, DT, reserved=2)
    # null handle / model / state / tasks / nu, negative batch, ndof out of range: the raw calls
    L = native.lib()
    tk = dev_tasks(handle, model, base, B)
    fs = handle._fb_state(st, B, n)
    nu = torch.empty((B, n + 6), dtype=torch.float64, device="cuda")
    args = [handle._h, ctypes.byref(dm.c), ctypes.byref(fs), ctypes.byref(tk.c), B, nu.data_ptr(), None, None]
    assert L.blf_fb_ik_solve(*args) == 0
    for pos in (0, 1, 2, 3, 5):
        bad = list(args)
        bad[pos] = None
        assert L.blf_fb_ik_solve(*bad) == INVALID, pos
    bad = list(args)
    bad[4] = -1
    assert L.blf_fb_ik_solve(*bad) == INVALID
    iargs = args[:5] + [1, DT] + args[5:]
    for pos in (0, 1, 2, 3):
        bad = list(iargs)
        bad[pos] = None
        assert L.blf_fb_ik_integrate(*bad) == INVALID, pos
    big = native.FbModel.from_buffer_copy(dm.c)
    for ndof in (0, 49):
        big.ndof = ndof
        assert L.blf_fb_ik_solve(handle._h, ctypes.byref(big), *args[2:]) == UNSUPPORTED
    none_state = native.FbState()
    assert L.blf_fb_ik_solve(args[0], args[1], ctypes.byref(none_state), *args[3:]) == INVALID
    torch.cuda.synchronize()
