"""GPU parity of blf_fb_ik_solve_limits / blf_fb_ik_integrate_limits (csrc/fb_ik.hip, include/blf/blf_c.h
section 12c) against tests/ik_limits_reference.py over the cases of tests/ik_limits_cases.py:

  sizes        n = 1, 3, 24, 48, and 26 | 27 (two robots per wavefront | one); prismatic joints at both
  batch        3 (a wavefront with an idle half), 130
  rows         1 to 27 hard rows, and none (hard = NULL)
  boxes        velocity limits, position ranges, both; one-sided; zero width; a joint outside its range;
               vel_max = NULL; bounds on joint 0 and on joint n - 1; a case that leaves block mode
  infeasible   boxes that contradict the hard rows: BLF_IK_LIMITS_UNRESOLVED and a NaN nu

Metric: fb_models.rel_err < 1e-9 on nu against the certified reference; iters and active equal to the
reference's (tests/test_ik_limits_reference.py holds every case at least 1e-7 from a tie on the CPU);
lo - 1e-12 <= s_dot <= up + 1e-12; hard-row residual <= 1e-12 max(1, |b_h|).

Measured on an MI355X (worst over the robots of a case): nu rel_err 6.6e-12 on pri-chain26-hard-15-wide,
4.6e-12 on pri-chain26-hard-15, 1.5e-12 on chain48-far-hard-15, below 1e-12 elsewhere; hard-row residual
at most 3.7e-14; iters 2 to 13, equal to the reference's everywhere; 20-step states within 1.6e-10 of
the reference trajectory (pri-chain26-hard-15-wide), below 1e-11 elsewhere.  The raised-CoM scenario:
both knees end at 0 exactly with limits (40 iterations over 20 steps on every robot) and 0.011-0.012
rad past straight without."""
import ctypes

import numpy as np
import pytest
import torch

import fb_models as FM
import ik_hard_cases as HC
import ik_limits_cases as LC
import ik_limits_reference as LR
import ik_reference as IK
from blf import native, robot
from gpu_util import dev_state, raises as _raises

pytestmark = pytest.mark.gpu
TOL = 1e-9
rel_err = FM.rel_err
DT = LC.DT


# local: the mask of a case, None for a case without hard rows
def hard_of(cs):
    if cs["rows"] == 0:
        return None
    h = native.IkHard()
    h.rows, h.reserved, h.rel_pivot_min = cs["rows"], 0, 0.0
    return h


# local: one (word 0, word 1) pair per robot of a solve's active set
def masks_of(active):
    a = active.cpu().numpy().astype(np.uint64)
    return [(int(a[i, 0]), int(a[i, 1])) for i in range(a.shape[0])]


def solve_limits(handle, cs, limits=None, tasks=None, states=None):
    model, B = cs["model"], cs["B"]
    tk = handle.ik_tasks(B, model["n"], **(cs["tasks"] if tasks is None else tasks))
    lm = handle.ik_limits(**(cs["limits"] if limits is None else limits))
    nu, status, iters, active = handle.fb_ik_solve(handle.fb_model(model),
                                                   dev_state(cs["states"] if states is None else states), tk,
                                                   hard=hard_of(cs), limits=lm)
    torch.cuda.synchronize()
    return nu.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy(), masks_of(active)


def check_against_reference(cid, i, nu, it, act, ref, cert):
    """One resolved robot: nu against the certificate, the counts, the box and the hard rows."""
    r = ref[i]
    e = rel_err(nu, cert[i][0])
    assert e < TOL, (cid, i, e)
    assert it == r["iters"], (cid, i, it, r["iters"])
    assert act == r["active"], (cid, i, act, r["active"])
    sd = nu[6:]
    assert (sd >= r["lo"] - 1e-12).all() and (sd <= r["up"] + 1e-12).all(), (cid, i)
    Ah, bh = r["parts"][4], r["parts"][5]
    res = np.abs(Ah @ nu - bh).max() / max(1.0, np.abs(bh).max()) if bh.size else 0.0
    assert res <= 1e-12, (cid, i, res)
    return e, res


@pytest.mark.parametrize("cid", LC.OK_CASES)
def test_solve_limits_vs_reference(handle, cid):
    """blf_fb_ik_solve_limits of every robot of a feasible case."""
    cs = LC.build_case(cid)
    nu, status, iters, act = solve_limits(handle, cs)
    ref, cert = LC.reference(cid), LC.certificate(cid)
    assert (status == LR.OK).all(), status
    worst = [check_against_reference(cid, i, nu[i], iters[i], act[i], ref, cert) for i in range(cs["B"])]
    print(f"{cid}: nu rel_err {max(w[0] for w in worst):.2e}, hard residual {max(w[1] for w in worst):.2e}, "
          f"iters {iters.min()}-{iters.max()}")


@pytest.mark.parametrize("cid", LC.INFEASIBLE_CASES)
def test_infeasible_boxes(handle, cid):
    """Boxes that contradict the hard rows: BLF_IK_LIMITS_UNRESOLVED and a NaN nu for every robot, no
    active mask, and a 2-step integration that leaves the states where they were."""
    cs = LC.build_case(cid)
    nu, status, iters, act = solve_limits(handle, cs)
    assert (status == LR.LIMITS_UNRESOLVED).all() and np.isnan(nu).all()
    assert all(a == (0, 0) for a in act) and (iters >= 1).all() and (iters <= LR.DEFAULT_MAX_ITER).all()
    st = dev_state(cs["states"])
    model, B = cs["model"], cs["B"]
    _, nu, status, _, _ = handle.fb_ik_integrate(handle.fb_model(model), st,
                                                 handle.ik_tasks(B, model["n"], **cs["tasks"]), 2, DT,
                                                 hard=hard_of(cs), limits=handle.ik_limits(**cs["limits"]))
    assert (status.cpu().numpy() == LR.LIMITS_UNRESOLVED).all() and torch.isnan(nu).all().item()
    for k in IK.STATE_KEYS:
        np.testing.assert_array_equal(st[k].cpu().numpy(), cs["states"][k], err_msg=k)


def test_unresolved_robot_is_contained(handle):
    """Robot 1 of 3 (it shares its wavefront with robot 0) has an infeasible box: status 4 and a NaN nu
    for it, its neighbours resolve exactly as the reference does."""
    cid, bad = LC.MIXED_CASE, LC.MIXED_BAD
    cs = LC.build_case(cid)
    nu, status, iters, act = solve_limits(handle, cs)
    ref = LC.reference(cid)
    assert status[bad] == LR.LIMITS_UNRESOLVED and np.isnan(nu[bad]).all() and act[bad] == (0, 0)
    for i in (0, 2):
        assert status[i] == LR.OK
        cert = {i: LR.certify(ref[i]["parts"], ref[i]["lo"], ref[i]["up"], ref[i]["side"])}
        assert cert[i][1]
        check_against_reference(cid, i, nu[i], iters[i], act[i], ref, cert)


@pytest.mark.parametrize("cid", ["rand24-hard-15", "pri-chain26-hard-15", "pri-chain27-hard-15", "pri-rand48-hard-12",
                                 "rand24-soft-onesided", "chain27-soft-pos"])
def test_no_limits_is_the_hard_call(handle, cid):
    """limits = NULL is bit for bit blf_fb_ik_solve_hard / blf_fb_ik_integrate_hard (the soft calls
    when hard is NULL too), iters and active left alone; all-infinite limits give the same nu to 1e-9
    in one iteration."""
    cs = LC.build_case(cid)
    model, B = cs["model"], cs["B"]
    n = model["n"]
    dm = handle.fb_model(model)
    tk = handle.ik_tasks(B, n, **cs["tasks"])
    hard = hard_of(cs)
    hp = ctypes.byref(hard) if hard is not None else None
    L = native.lib()
    hnu, hstatus = handle.fb_ik_solve(dm, dev_state(cs["states"]), tk, hard=hard)
    ref_st = dev_state(cs["states"])
    _, inu, istatus = handle.fb_ik_integrate(dm, ref_st, tk, 3, DT, hard=hard)
    st = dev_state(cs["states"])
    nu = torch.full((B, n + 6), -7.0, dtype=torch.float64, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    iters = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    active = torch.full((B, 2), -7, dtype=torch.int64, device="cuda")
    assert L.blf_fb_ik_solve_limits(handle._h, ctypes.byref(dm.c), ctypes.byref(handle._fb_state(st, B, n)),
                                    ctypes.byref(tk.c), hp, None, B, nu.data_ptr(), status.data_ptr(),
                                    iters.data_ptr(), active.data_ptr(), None) == 0
    assert torch.equal(nu, hnu) and torch.equal(status, hstatus)
    assert L.blf_fb_ik_integrate_limits(handle._h, ctypes.byref(dm.c), ctypes.byref(handle._fb_state(st, B, n)),
                                        ctypes.byref(tk.c), hp, None, B, 3, DT, nu.data_ptr(), status.data_ptr(),
                                        iters.data_ptr(), active.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(nu, inu) and torch.equal(status, istatus)
    assert (iters == -7).all().item() and (active == -7).all().item()
    for k in native.FB_STATE_KEYS:
        assert torch.equal(st[k], ref_st[k]), (cid, k)
    fnu, fstatus, fiters, fact = solve_limits(handle, cs, limits=LR.no_limits(n))
    assert (fstatus == LR.OK).all() and (fiters == 1).all() and all(a == (0, 0) for a in fact)
    assert max(rel_err(fnu[i], hnu[i].cpu().numpy()) for i in range(B)) < TOL


@pytest.mark.parametrize("steps", [1, 2, 20])
@pytest.mark.parametrize("cid", LC.INTEGRATE_CASES)
def test_integrate_limits_is_the_unfused_sequence(handle, cid, steps):
    """`steps` fused steps equal, bit for bit, steps x { blf_fb_ik_solve_limits;
    blf_fbk_euler_integrate(0, dT, dT) with that nu } on every state key, nu, status and the masks, with
    iters the sum over the steps; the counts also equal the reference's trajectory."""
    cs = LC.build_case(cid)
    model = cs["model"]
    B = min(cs["B"], 3)
    dm = handle.fb_model(model)
    tk = handle.ik_tasks(B, model["n"], **IK.tasks_rows(cs["tasks"], slice(0, B)))
    lm = handle.ik_limits(**cs["limits"])
    hard = hard_of(cs)
    fused = dev_state(cs["states"], slice(0, B))
    _, fnu, fstatus, fiters, factive = handle.fb_ik_integrate(dm, fused, tk, steps, DT, hard=hard, limits=lm)
    un = dev_state(cs["states"], slice(0, B))
    total = torch.zeros((B,), dtype=torch.int32, device="cuda")
    for _ in range(steps):
        nu, status, iters, active = handle.fb_ik_solve(dm, un, tk, hard=hard, limits=lm)
        total += iters
        twist, jv = nu[:, :6].contiguous(), nu[:, 6:].contiguous()
        handle.fbk_euler_integrate(dm.c.rho, un["base_pos"], un["base_rot"], un["joint_pos"], twist, jv, 0.0, DT, DT)
    un["base_vel"], un["joint_vel"] = twist, jv
    torch.cuda.synchronize()
    assert (fstatus == 0).all().item() and (status == 0).all().item()
    for k in native.FB_STATE_KEYS:
        assert torch.equal(fused[k], un[k]), (cid, k)
    assert torch.equal(fnu, nu) and torch.equal(fiters, total) and torch.equal(factive, active)
    ref = LC.integrate_reference(cid, steps)
    worst = max(rel_err(fused[k][i].cpu().numpy(), ref[i][0][k]) for i in range(B) for k in native.FB_STATE_KEYS)
    print(f"{cid} steps {steps}: state rel_err against the reference {worst:.2e}, iters {fiters.tolist()} "
          f"(reference {[r[3] for r in ref]})")


def test_limits_keep_the_joints_in_range(handle):
    """What the feature is for (ik_limits_cases.raised_com): the humanoid on straight legs with hard
    feet and a CoM target 2 cm above what straight legs reach.  With robot.humanoid24_joint_limits and
    sampling_time = dT every joint of every robot stays in [pos_lower - 1e-12, pos_upper + 1e-12] over 20
    fused steps and no sole ends further from its set point than it began (the bound of
    test_hard_feet_stay_planted); the same call without limits pushes a knee past straight."""
    cs = LC.raised_com()
    model, B, tasks, lim = cs["model"], cs["B"], cs["tasks"], cs["limits"]
    dm = handle.fb_model(model)
    tk = handle.ik_tasks(B, model["n"], **tasks)
    hard = handle.ik_hard(**robot.standing_ik_hard(model))
    lm = handle.ik_limits(**robot.humanoid24_joint_limits(model, sampling_time=DT))
    st = dev_state(cs["states"])
    _, _, status, iters, active = handle.fb_ik_integrate(dm, st, tk, 20, DT, hard=hard, limits=lm)
    free = dev_state(cs["states"])
    _, _, fstatus = handle.fb_ik_integrate(dm, free, tk, 20, DT, hard=hard)
    torch.cuda.synchronize()
    assert (status == 0).all().item() and (fstatus == 0).all().item()
    q, qf = st["joint_pos"].cpu().numpy(), free["joint_pos"].cpu().numpy()
    held = {k: v.cpu().numpy() for k, v in st.items()}
    print("iters", iters.tolist(), "active", masks_of(active), "least q - lower: limits", (q - lim["pos_lower"]).min(),
          "none", (qf - lim["pos_lower"]).min())
    for i in range(B):
        assert (q[i] >= lim["pos_lower"] - 1e-12).all() and (q[i] <= lim["pos_upper"] + 1e-12).all(), i
        assert (qf[i] < lim["pos_lower"]).any(), i
        e0 = HC.sole_errors(model, tasks, {k: cs["states"][k][i] for k in IK.STATE_KEYS}, i)
        e1 = HC.sole_errors(model, tasks, {k: held[k][i] for k in IK.STATE_KEYS}, i)
        assert (e1 <= e0).all(), (i, e0, e1)


def test_max_iter_is_honoured(handle):
    """max_iter = 1 ends every robot that needs a second iteration unresolved, and leaves a robot that
    needs one alone; max_iter equal to the count a robot needs resolves it."""
    cid = "rand24-hard-15"
    cs = LC.build_case(cid)
    ref = LC.reference(cid)
    need = [r["iters"] for r in ref]
    for cap in (1, max(need)):
        nu, status, iters, _ = solve_limits(handle, cs, limits=dict(cs["limits"], max_iter=cap))
        for i in range(cs["B"]):
            assert status[i] == (LR.OK if need[i] <= cap else LR.LIMITS_UNRESOLVED), (cap, i)
            assert iters[i] == min(need[i], cap)


def test_status_precedence_and_containment(handle):
    """A NaN set point is BLF_IK_BAD_INPUT with iters 0 whatever the box; its wavefront neighbour
    resolves bit for bit as without it."""
    cid = "rand24-hard-15"
    cs = LC.build_case(cid)
    pose = cs["tasks"]["se3_pose"].copy()
    pose[1, -1, 7] = np.nan
    good = solve_limits(handle, cs)
    nu, status, iters, act = solve_limits(handle, cs, tasks=dict(cs["tasks"], se3_pose=pose))
    assert status[1] == LR.BAD_INPUT and np.isnan(nu[1]).all() and iters[1] == 0 and act[1] == (0, 0)
    for i in (0, 2):
        assert status[i] == LR.OK and iters[i] == good[2][i] and act[i] == good[3][i]
        np.testing.assert_array_equal(nu[i], good[0][i])


def test_limits_call_errors(handle):
    """Every call-level error of section 12c, and section 12b's through the new entry points."""
    INVALID = 1
    cs = LC.build_case("rand24-hard-15")
    model, B = cs["model"], cs["B"]
    n = model["n"]
    dm = handle.fb_model(model)
    st = dev_state(cs["states"])
    tk = handle.ik_tasks(B, n, **cs["tasks"])
    base = cs["limits"]

    def solve(lim, hard=hard_of(cs), **over):
        lm = handle.ik_limits(**lim)
        for k, v in over.items():
            setattr(lm.c, k, v)
        return handle.fb_ik_solve(dm, st, tk, hard=hard, limits=lm)

    def integrate(lim, steps=1, dT=DT, **over):
        lm = handle.ik_limits(**lim)
        for k, v in over.items():
            setattr(lm.c, k, v)
        return handle.fb_ik_integrate(dm, {k: v.clone() for k, v in st.items()}, tk, steps, dT, hard=hard_of(cs),
                                      limits=lm)

    def with_(key, j, v):
        a = np.array(base[key], dtype=np.float64, copy=True)
        a[j] = v
        return dict(base, **{key: a})

    solve(base)
    integrate(base)
    for call in (solve, integrate):
        _raises(INVALID, call, base, reserved=1)
        _raises(INVALID, call, base, max_iter=-1)
        for T in (0.0, -0.01, float("nan"), float("inf")):
            _raises(INVALID, call, dict(base, sampling_time=T))
        for kl in (0.0, -0.5, 1.5, float("nan")):
            _raises(INVALID, call, with_("klim", 3, kl))
        for vm in (0.0, -1.0, float("nan")):
            _raises(INVALID, call, with_("vel_max", 5, vm))
        _raises(INVALID, call, with_("pos_lower", 2, base["pos_upper"][2] + 1.0))
        _raises(INVALID, call, with_("pos_lower", 2, float("nan")))
        _raises(INVALID, call, with_("pos_upper", n - 1, float("nan")))
        _raises(INVALID, call, with_("pos_lower", 0, float("inf")))
        _raises(INVALID, call, base, pos_lower=None)
        _raises(INVALID, call, base, klim=None)
    bad = native.IkHard()
    bad.rows, bad.reserved = 1 << 27, 0
    _raises(INVALID, solve, base, hard=bad)                     # section 12b's, through the new call
    _raises(INVALID, integrate, base, 0)
    _raises(INVALID, integrate, base, 1, float("nan"))
    # batch == 0 is BLF_OK; null handle / model / state / tasks / nu and a negative batch are refused
    L = native.lib()
    lm = handle.ik_limits(**base)
    fs = handle._fb_state(st, B, n)
    nu = torch.empty((B, n + 6), dtype=torch.float64, device="cuda")
    h = hard_of(cs)
    args = [handle._h, ctypes.byref(dm.c), ctypes.byref(fs), ctypes.byref(tk.c), ctypes.byref(h), ctypes.byref(lm.c),
            B, nu.data_ptr(), None, None, None, None]
    assert L.blf_fb_ik_solve_limits(*args) == 0
    zero = list(args)
    zero[6] = 0
    assert L.blf_fb_ik_solve_limits(*zero) == 0
    for pos in (0, 1, 2, 3, 7):
        bad = list(args)
        bad[pos] = None
        assert L.blf_fb_ik_solve_limits(*bad) == INVALID, pos
    neg = list(args)
    neg[6] = -1
    assert L.blf_fb_ik_solve_limits(*neg) == INVALID
    torch.cuda.synchronize()
