"""GPU parity of blf_fb_ik_solve_hard / blf_fb_ik_integrate_hard (csrc/fb_ik.hip, include/blf/blf_c.h
section 12b) against tests/ik_hard_reference.py (a dense KKT solve with long-double refinement: another
algorithm than the device's projection) over the cases of tests/ik_hard_cases.py:

  masks        1, 3, 6, 7, 8, 9, 12, 15 and all 27 rows; SE3 rows alone, the CoM alone, both; an SO3-only
               and an R3-only task; base_damping = 0 with the base held by the hard feet alone
  sizes        n = 1, 3, 24, 48, and 26 | 27 (two robots per wavefront | one); prismatic joints at both
  batch        1, 3, 130
  dependent    two hard tasks on one frame, more rows than unknowns, tasks down one chain, a frame on
               the base link beside three others: BLF_IK_HARD_DEPENDENT and a NaN nu

Metric: fb_models.rel_err < 1e-9 on nu (and on every state key after an integration), and the
constraint residual |A_h nu - b_h| <= 1e-9 max(1, |b_h|) in the reference's rows.
tests/test_ik_hard_reference.py holds every case to its conditioning band on the CPU.

Measured on an MI355X (worst over the robots of a case): nu rel_err 6.6e-12 on pri-chain26-k2com-15,
6.5e-12 on chain48-k2com-far-15, 4.9e-12 on the 27-joint chains, at most 4.4e-13 on every other case
(2.3e-13 with all 27 rows hard, 9e-16 at n = 1); constraint residual at most 8.3e-15; state rel_err
after 1, 2 and 20 integration steps at most 3.3e-11 (chain48-k2com-far-15), 1.2e-11 on
pri-chain26-k2com-15, below 8e-12 elsewhere; nu moves by at most 2.0e-11 (chain48-k2com-far-15) when
the hard rows' weights are scaled by 0.25 or by 4.  Planted feet (ik_hard_cases.planted_feet): sole
errors of 0.19-0.36 mm fall to 0.07-0.13 mm with the hard rows and rise to 0.36-0.64 mm with the
weights alone."""
import ctypes

import numpy as np
import pytest
import torch

import fb_models as FM
import ik_hard_cases as HC
import ik_hard_reference as HR
import ik_reference as IK
from blf import native, robot
from gpu_util import dev_state, dev_tasks, raises as _raises

pytestmark = pytest.mark.gpu
TOL = 1e-9
rel_err = FM.rel_err
DT = HC.DT


# local: the mask of a case, with a pivot threshold
def hard_of(cs, tau=0.0):
    h = native.IkHard()
    h.rows, h.reserved, h.rel_pivot_min = cs["rows"], 0, tau
    return h


def solve_hard(handle, cs, states=None, tasks=None, hard=None):
    model, B = cs["model"], cs["B"]
    tk = dev_tasks(handle, model, cs["tasks"] if tasks is None else tasks, B)
    nu, status = handle.fb_ik_solve(handle.fb_model(model), dev_state(cs["states"] if states is None else states),
                                    tk, hard=hard_of(cs) if hard is None else hard)
    torch.cuda.synchronize()
    return nu.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("cid", HC.OK_CASES)
def test_solve_hard_vs_reference(handle, cid):
    """blf_fb_ik_solve_hard of every robot of a well-posed case against the KKT reference, nu and
    status written at odd offsets into larger buffers."""
    cs = HC.build_case(cid)
    model, B = cs["model"], cs["B"]
    NV = model["n"] + 6
    nb = torch.full((B * NV + 3,), -7.0, dtype=torch.float64, device="cuda")
    sb = torch.full((B + 3,), -7, dtype=torch.int32, device="cuda")
    nu, status = nb[1:1 + B * NV].view(B, NV), sb[1:1 + B]
    st = dev_state(cs["states"])
    before = {k: v.clone() for k, v in st.items()}
    handle.fb_ik_solve(handle.fb_model(model), st, dev_tasks(handle, model, cs["tasks"], B), nu=nu, status=status,
                       hard=hard_of(cs))
    torch.cuda.synchronize()
    assert nb[0].item() == -7.0 and (nb[-2:] == -7.0).all().item()
    assert sb[0].item() == -7 and (sb[-2:] == -7).all().item()
    for k in st:
        assert torch.equal(st[k], before[k]), k
    got, ref = nu.cpu().numpy(), HC.reference(cid)
    assert (status.cpu().numpy() == HR.OK).all()
    errs = [rel_err(got[i], ref[i][0]) for i in range(B)]
    res = [np.abs(ref[i][2][4] @ got[i] - ref[i][2][5]).max() / max(1.0, np.abs(ref[i][2][5]).max()) for i in range(B)]
    print(f"{cid}: nu rel_err {max(errs):.2e}, constraint residual {max(res):.2e}")
    for i in range(B):
        assert errs[i] < TOL, (cid, i, errs[i])
        assert res[i] <= TOL, (cid, i, res[i])


def run_integrate(handle, cs, steps, rows=None, states=None, tasks=None, hard=None):
    model = cs["model"]
    states = cs["states"] if states is None else states
    tasks = cs["tasks"] if tasks is None else tasks
    st = dev_state(states, rows)
    B = st["joint_pos"].shape[0]
    _, nu, status = handle.fb_ik_integrate(handle.fb_model(model), st, dev_tasks(handle, model, tasks, B), steps, DT,
                                           hard=hard_of(cs) if hard is None else hard)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in st.items()}, nu.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("steps", [1, 2, 20])
@pytest.mark.parametrize("cid", HC.INTEGRATE_CASES)
def test_integrate_hard_vs_reference(handle, cid, steps):
    """blf_fb_ik_integrate_hard against the reference's loop (KKT solve, one Euler step) on every
    state key."""
    cs = HC.build_case(cid)
    B = min(cs["B"], 3)
    got, nu, status = run_integrate(handle, cs, steps, slice(0, B), tasks=IK.tasks_rows(cs["tasks"], slice(0, B)))
    worst = 0.0
    for i, (ref, rnu, rst) in enumerate(HC.integrate_reference(cid, steps)):
        assert status[i] == rst == HR.OK
        for k in native.FB_STATE_KEYS:
            e = rel_err(got[k][i], ref[k])
            worst = max(worst, e)
            assert e < TOL, (cid, steps, i, k, e)
        np.testing.assert_array_equal(nu[i, :6], got["base_vel"][i])
        np.testing.assert_array_equal(nu[i, 6:], got["joint_vel"][i])
    print(f"{cid} steps {steps}: state rel_err {worst:.2e}")


@pytest.mark.parametrize("cid", ["rand24-k2com-null-15", "pri-chain26-k2com-15", "chain27-k2com-9",
                                 "pri-rand48-k2-12", "limbs48-k4com-27", "humanoid-15-nodamp-b130"])
def test_integrate_hard_is_the_unfused_sequence(handle, cid):
    """20 fused steps equal, bit for bit, 20 x { blf_fb_ik_solve_hard; blf_fbk_euler_integrate(0, dT,
    dT) with that nu } on every state key, nu and status."""
    cs = HC.build_case(cid)
    model, B, steps = cs["model"], cs["B"], 20
    dm = handle.fb_model(model)
    tk = dev_tasks(handle, model, cs["tasks"], B)
    hard = hard_of(cs)
    fused = dev_state(cs["states"])
    _, fnu, fstatus = handle.fb_ik_integrate(dm, fused, tk, steps, DT, hard=hard)
    un = dev_state(cs["states"])
    for _ in range(steps):
        nu, status = handle.fb_ik_solve(dm, un, tk, hard=hard)
        twist, jv = nu[:, :6].contiguous(), nu[:, 6:].contiguous()
        handle.fbk_euler_integrate(dm.c.rho, un["base_pos"], un["base_rot"], un["joint_pos"], twist, jv, 0.0, DT, DT)
    un["base_vel"], un["joint_vel"] = twist, jv
    torch.cuda.synchronize()
    assert (fstatus == 0).all().item() and (status == 0).all().item()
    for k in native.FB_STATE_KEYS:
        assert torch.equal(fused[k], un[k]), (cid, k)
    assert torch.equal(fnu, nu)


@pytest.mark.parametrize("cid", ["rand24-k2com-15", "pri-chain26-k2com-15", "chain27-k2com-15", "pri-rand48-k2-12"])
def test_no_hard_rows_is_the_soft_call(handle, cid):
    """hard = NULL and rows = 0 (with any tau) are bit for bit blf_fb_ik_solve / blf_fb_ik_integrate."""
    cs = HC.build_case(cid)
    model, B = cs["model"], cs["B"]
    dm = handle.fb_model(model)
    tk = dev_tasks(handle, model, cs["tasks"], B)
    none = native.IkHard()
    none.rel_pivot_min = 0.5
    L = native.lib()
    n = model["n"]
    snu, sstatus = handle.fb_ik_solve(dm, dev_state(cs["states"]), tk)
    soft = dev_state(cs["states"])
    _, inu, istatus = handle.fb_ik_integrate(dm, soft, tk, 3, DT)
    for hp in (None, ctypes.byref(none)):
        st = dev_state(cs["states"])
        nu = torch.full((B, n + 6), -7.0, dtype=torch.float64, device="cuda")
        status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        assert L.blf_fb_ik_solve_hard(handle._h, ctypes.byref(dm.c), ctypes.byref(handle._fb_state(st, B, n)),
                                      ctypes.byref(tk.c), hp, B, nu.data_ptr(), status.data_ptr(), None) == 0
        assert torch.equal(nu, snu) and torch.equal(status, sstatus)
        assert L.blf_fb_ik_integrate_hard(handle._h, ctypes.byref(dm.c), ctypes.byref(handle._fb_state(st, B, n)),
                                          ctypes.byref(tk.c), hp, B, 3, DT, nu.data_ptr(), status.data_ptr(),
                                          None) == 0
        torch.cuda.synchronize()
        assert torch.equal(nu, inu) and torch.equal(status, istatus)
        for k in native.FB_STATE_KEYS:
            assert torch.equal(st[k], soft[k]), (cid, k)


@pytest.mark.parametrize("factor", [0.25, 4.0])
@pytest.mark.parametrize("cid", HC.OK_CASES)
def test_hard_weights_only_condition(handle, cid, factor):
    """Scaling the hard rows' weights by 0.25 and by 4 moves nu by less than 1e-9."""
    cs = HC.build_case(cid)
    a, sa = solve_hard(handle, cs)
    b, sb = solve_hard(handle, cs, tasks=HR.scale_hard_weights(cs["tasks"], cs["rows"], factor))
    assert (sa == HR.OK).all() and (sb == HR.OK).all()
    worst = max(rel_err(b[i], a[i]) for i in range(cs["B"]))
    print(f"{cid} x{factor}: nu moves by {worst:.2e}")
    assert worst < TOL, (cid, factor, worst)


def test_hard_feet_stay_planted(handle):
    """The point of the feature.  The humanoid with each sole a fraction of a millimetre off its set
    point and the CoM target 3 cm ahead (ik_hard_cases.planted_feet): after 20 fused steps with
    robot.standing_ik_hard no sole's pose error is above its value before the first step; with the
    same task set weighted, every robot ends with a sole further from its set point than it began."""
    cs = HC.planted_feet()
    model, B, tasks = cs["model"], cs["B"], cs["tasks"]
    hard = handle.ik_hard(**robot.standing_ik_hard(model))
    assert hard.rows == cs["rows"]
    hs, _, hstat = run_integrate(handle, cs, 20, hard=hard)
    st = dev_state(cs["states"])
    _, _, sstat = handle.fb_ik_integrate(handle.fb_model(model), st, dev_tasks(handle, model, tasks, B), 20, DT)
    ss = {k: v.cpu().numpy() for k, v in st.items()}
    assert (hstat == HR.OK).all() and (sstat.cpu().numpy() == IK.OK).all()
    for i in range(B):
        e0 = HC.sole_errors(model, tasks, {k: cs["states"][k][i] for k in IK.STATE_KEYS}, i)
        eh = HC.sole_errors(model, tasks, {k: hs[k][i] for k in IK.STATE_KEYS}, i)
        es = HC.sole_errors(model, tasks, {k: ss[k][i] for k in IK.STATE_KEYS}, i)
        print(f"robot {i}: sole errors before {e0}, hard {eh}, weighted {es}")
        assert (eh <= e0).all(), (i, e0, eh)
        assert (es > e0).any(), (i, e0, es)


@pytest.mark.parametrize("cid", HC.DEP_CASES)
def test_dependent_masks(handle, cid):
    """Dependent hard rows: BLF_IK_HARD_DEPENDENT and a NaN nu for every robot, in the solve and in a
    2-step integration, which leaves the states where they were."""
    cs = HC.build_case(cid)
    nu, status = solve_hard(handle, cs)
    assert (status == HR.HARD_DEPENDENT).all() and np.isnan(nu).all()
    assert all(r[1] == HR.HARD_DEPENDENT for r in HC.reference(cid))
    st, nu, status = run_integrate(handle, cs, 2)
    assert (status == HR.HARD_DEPENDENT).all() and np.isnan(nu).all()
    assert np.isnan(st["base_vel"]).all() and np.isnan(st["joint_vel"]).all()
    for k in IK.STATE_KEYS:
        np.testing.assert_array_equal(st[k], cs["states"][k], err_msg=k)


@pytest.mark.parametrize("cid", ["rand24-k2com-15", "chain27-k2com-15"])
def test_bad_robot_is_contained(handle, cid):
    """A NaN pose set point of robot 1 of 3 (it shares its wavefront with robot 0 when two robots
    take one): BLF_IK_BAD_INPUT and a NaN nu for it, its neighbours bit-identical to the run without
    it and within 1e-9 of the reference; a 3-step integration leaves the bad robot where it was."""
    cs = HC.build_case(cid)
    model, bad = cs["model"], 1
    pose = cs["tasks"]["se3_pose"].copy()
    pose[bad, -1, 7] = np.nan
    tasks = dict(cs["tasks"], se3_pose=pose)
    assert HR.solve(model, cs["states"], tasks, cs["rows"], bad)[1] == HR.BAD_INPUT
    good_nu, _ = solve_hard(handle, cs)
    nu, status = solve_hard(handle, cs, tasks=tasks)
    assert status[bad] == HR.BAD_INPUT and np.isnan(nu[bad]).all()
    ref = HC.reference(cid)
    for i in (0, 2):
        assert status[i] == HR.OK
        np.testing.assert_array_equal(nu[i], good_nu[i])
        assert rel_err(nu[i], ref[i][0]) < TOL
    good_st, good_nu, _ = run_integrate(handle, cs, 3)
    st, nu, status = run_integrate(handle, cs, 3, tasks=tasks)
    assert status[bad] == HR.BAD_INPUT and np.isnan(nu[bad]).all()
    for k in IK.STATE_KEYS:
        np.testing.assert_array_equal(st[k][bad], cs["states"][k][bad], err_msg=k)
    for i in (0, 2):
        assert status[i] == HR.OK
        for k in native.FB_STATE_KEYS:
            np.testing.assert_array_equal(st[k][i], good_st[k][i], err_msg=k)


def test_status_precedence(handle):
    """A dependent mask on a robot with a NaN set point is BLF_IK_BAD_INPUT, on one whose H overflows
    BLF_IK_NOT_POSITIVE, on its sound neighbour BLF_IK_HARD_DEPENDENT."""
    cs = HC.build_case("rand24-so3-r3-dep")
    states = {k: v.copy() for k, v in cs["states"].items()}
    pose = cs["tasks"]["se3_pose"].copy()
    pose[0, 0, 3] = np.nan
    states["base_rot"][2] = states["base_rot"][2] * 1e160
    nu, status = solve_hard(handle, cs, states=states, tasks=dict(cs["tasks"], se3_pose=pose))
    assert list(status) == [HR.BAD_INPUT, HR.HARD_DEPENDENT, HR.NOT_POSITIVE] and np.isnan(nu).all()


@pytest.mark.parametrize("cid", ["rand24-k2com-15", "chain27-k2com-15"])
def test_frame_index_out_of_range(handle, cid):
    """As in test_gpu_ik.py: a frame index outside the model's frames makes every robot
    BLF_IK_BAD_INPUT with a NaN nu, reads nothing out of bounds and leaves the states alone."""
    cs = HC.build_case(cid)
    model = cs["model"]
    for f in (len(model["frame_link"]), -1, 2 ** 30):
        tasks = dict(cs["tasks"], frame=np.array([1, f], dtype=np.int32))
        nu, status = solve_hard(handle, cs, tasks=tasks)
        assert (status == HR.BAD_INPUT).all() and np.isnan(nu).all()
        st, nu, status = run_integrate(handle, cs, 2, tasks=tasks)
        assert (status == HR.BAD_INPUT).all() and np.isnan(nu).all()
        for k in IK.STATE_KEYS:
            np.testing.assert_array_equal(st[k], cs["states"][k], err_msg=k)


def test_unknown_joint_type(handle):
    """A joint_type that is neither revolute nor prismatic: every robot's nu is NaN."""
    cs = HC.build_case("pri-chain26-k2com-15")
    model, B = cs["model"], cs["B"]
    dm = handle.fb_model(model)
    dm.t["joint_type"][3] = 7   # (native.fb_model refuses it up front: set behind its back)
    nu, status = handle.fb_ik_solve(dm, dev_state(cs["states"]), dev_tasks(handle, model, cs["tasks"], B),
                                    hard=hard_of(cs))
    assert torch.isnan(nu).all().item() and (status != HR.OK).all().item()


def test_rel_pivot_min_is_honoured(handle):
    """tau just below 1 refuses a well-posed mask whose smallest relative pivot is 1.3e-2
    (rand24-k2com-15), and tau = 1e-3 accepts it with the default's result."""
    cs = HC.build_case("rand24-k2com-15")
    nu0, _ = solve_hard(handle, cs)
    nu, status = solve_hard(handle, cs, hard=hard_of(cs, 0.5))
    assert (status == HR.HARD_DEPENDENT).all() and np.isnan(nu).all()
    nu, status = solve_hard(handle, cs, hard=hard_of(cs, 1e-3))
    assert (status == HR.OK).all()
    np.testing.assert_array_equal(nu, nu0)


def test_hard_call_errors(handle):
    """Every call-level error of section 12b with a batch on the device (the ones that need none
    are in tests/test_ik_hard_reference.py too), and section 12's through the new entry points."""
    INVALID, UNSUPPORTED = 1, 3
    cs = HC.build_case("rand24-so3-r3-9")   # task 0 has zero linear weights, task 1 zero angular ones
    model, B = cs["model"], cs["B"]
    dm = handle.fb_model(model)
    st = dev_state(cs["states"])
    base = cs["tasks"]

    def hard(rows, reserved=0, tau=0.0):
        h = native.IkHard()
        h.rows, h.reserved, h.rel_pivot_min = rows, reserved, tau
        return h

    def solve(h, tasks=None, **over):
        tk = dev_tasks(handle, model, base if tasks is None else tasks, B)
        for k, v in over.items():
            setattr(tk.c, k, v)
        return handle.fb_ik_solve(dm, st, tk, hard=h)

    def integrate(h, steps=1, dT=DT, **over):
        tk = dev_tasks(handle, model, base, B)
        for k, v in over.items():
            setattr(tk.c, k, v)
        return handle.fb_ik_integrate(dm, {k: v.clone() for k, v in st.items()}, tk, steps, dT, hard=h)

    solve(hard(cs["rows"]))
    integrate(hard(cs["rows"]))
    for call in (solve, integrate):
        _raises(INVALID, call, hard(1 << 0))               # a hard row of weight 0 (task 0, linear x)
        _raises(INVALID, call, hard(1 << 9))               # (task 1, angular x)
        _raises(INVALID, call, hard(1 << 18))              # SE3 task 3 of K = 3
        _raises(INVALID, call, hard(1 << 27))              # bits above 26
        _raises(INVALID, call, hard(cs["rows"], reserved=1))
        for tau in (1.0, -1e-3, float("nan"), float("inf")):
            _raises(INVALID, call, hard(cs["rows"], tau=tau))
        _raises(INVALID, call, hard(cs["rows"]), reserved=1)          # section 12's: tasks->reserved
        _raises(INVALID, call, hard(cs["rows"]), base_damping=-1.0)
        _raises(UNSUPPORTED, call, hard(cs["rows"]), nse3=5)
    # a CoM bit without a CoM task; a hard CoM row of weight 0
    nocom = dict(base, com_weight=None, com_pos=None, com_vel=None)
    _raises(INVALID, solve, hard(1 << 24), nocom)
    _raises(INVALID, solve, hard(1 << 25), dict(base, com_weight=np.array([1.0, 0.0, 1.0])))
    solve(hard(1 << 24), dict(base, com_weight=np.array([1.0, 0.0, 1.0])))
    _raises(INVALID, integrate, hard(cs["rows"]), 0)
    for dT in (0.0, -DT, float("nan"), float("inf")):
        _raises(INVALID, integrate, hard(cs["rows"]), 1, dT)
    # null handle / model / state / tasks / nu, negative batch: the raw calls
    L = native.lib()
    n = model["n"]
    tk = dev_tasks(handle, model, base, B)
    fs = handle._fb_state(st, B, n)
    nu = torch.empty((B, n + 6), dtype=torch.float64, device="cuda")
    h = hard(cs["rows"])
    args = [handle._h, ctypes.byref(dm.c), ctypes.byref(fs), ctypes.byref(tk.c), ctypes.byref(h), B, nu.data_ptr(),
            None, None]
    assert L.blf_fb_ik_solve_hard(*args) == 0
    for pos in (0, 1, 2, 3, 6):
        bad = list(args)
        bad[pos] = None
        assert L.blf_fb_ik_solve_hard(*bad) == INVALID, pos
    bad = list(args)
    bad[5] = -1
    assert L.blf_fb_ik_solve_hard(*bad) == INVALID
    iargs = args[:6] + [1, DT] + args[6:]
    for pos in (0, 1, 2, 3):
        bad = list(iargs)
        bad[pos] = None
        assert L.blf_fb_ik_integrate_hard(*bad) == INVALID, pos
    torch.cuda.synchronize()
