"""tests/ik_hard_reference.py (the numpy restatement of include/blf/blf_c.h section 12b that checks
blf_fb_ik_solve_hard / blf_fb_ik_integrate_hard) and the cases of tests/ik_hard_cases.py pinned on
the CPU: every case inside its conditioning band, the float64 projection against the KKT reference,
its independence of the hard rows' weights, the constraint residual of the reference, and the
call-level errors that need no device."""
import ctypes

import numpy as np
import pytest

import fb_models as FM
import ik_hard_cases as HC
import ik_hard_reference as HR
import ik_reference as IK
from blf import native, robot

WELL, DEPENDENT = 1.0e-5, 1.0e-11   # 1e3 tau and 1e-3 tau


def _projection(cid, factor=1.0):
    """HR.project of every robot of the case with the hard rows' weights scaled by `factor`."""
    cs = HC.build_case(cid)
    tasks = HR.scale_hard_weights(cs["tasks"], cs["rows"], factor) if factor != 1.0 else cs["tasks"]
    out = []
    for i in range(min(cs["B"], 3)):
        s = {k: np.asarray(cs["states"][k][i], dtype=np.float64) for k in IK.STATE_KEYS}
        H, g, _, _, Ah, bh = HR.parts(cs["model"], s, IK.one(tasks, i), cs["rows"])
        out.append(HR.project(H, g, Ah, bh))
    return out


@pytest.mark.parametrize("cid", sorted(HC.CASES))
def test_case_conditioning(cid):
    """Every robot of every case sits in its band: the relative pivots of S are at least 1e-5 for a
    well-posed mask (1e3 tau) and the failing one at most 1e-11 in magnitude for a dependent mask
    (1e-3 tau), or the mask has more rows than unknowns; the reference's status (from the singular
    values of A_h) agrees with the pivot rule's."""
    cs = HC.build_case(cid)
    lo, fail = np.inf, 0.0
    for i, (nu, status, P) in enumerate(HC.reference(cid)):
        H, g, _, _, Ah, bh = P
        _, pstatus, rel = HR.project(H, g, Ah, bh)
        if cs["kind"] == "ok":
            assert status == pstatus == HR.OK, (cid, i)
            lo = min(lo, rel.min())
            assert rel.min() >= WELL, (cid, i, rel.min())
        else:
            assert status == pstatus == HR.HARD_DEPENDENT and np.isnan(nu).all(), (cid, i)
            if Ah.shape[0] <= H.shape[0]:
                assert (rel[:-1] >= WELL).all(), (cid, i, rel)   # the pivots before it are sound
                fail = max(fail, abs(rel[-1]))
                assert abs(rel[-1]) <= DEPENDENT, (cid, i, rel[-1])
    print(f"{cid}: smallest relative pivot {lo:.2e}, failing pivot {fail:.2e}")


@pytest.mark.parametrize("cid", HC.OK_CASES)
def test_projection_matches_kkt(cid):
    """The device's method in float64 is within 1e-10 of the refined dense KKT solve, and the
    reference meets the constraints: |A_h nu - b_h| <= 1e-12 max(1, |b_h|)."""
    worst = res = 0.0
    for i, ((nu, status, P), (pn, ps, _)) in enumerate(zip(HC.reference(cid), _projection(cid))):
        assert status == ps == HR.OK
        worst = max(worst, FM.rel_err(pn, nu))
        Ah, bh = P[4], P[5]
        r = np.abs(Ah @ nu - bh).max() / max(1.0, np.abs(bh).max())
        res = max(res, r)
        assert r <= 1e-12, (cid, i, r)
    print(f"{cid}: projection against KKT rel_err {worst:.2e}, reference residual {res:.2e}")
    assert worst < 1e-10, (cid, worst)


@pytest.mark.parametrize("factor", [0.25, 4.0])
@pytest.mark.parametrize("cid", HC.OK_CASES)
def test_projection_does_not_depend_on_hard_weights(cid, factor):
    """A hard row's weight only conditions H: scaled by 0.25 and by 4 the projection's nu moves by
    less than 1e-10."""
    for (a, sa, _), (b, sb, _) in zip(_projection(cid), _projection(cid, factor)):
        assert sa == sb == HR.OK
        assert FM.rel_err(b, a) < 1e-10, (cid, factor, FM.rel_err(b, a))


@pytest.mark.parametrize("steps", [1, 2, 20])
@pytest.mark.parametrize("cid", HC.INTEGRATE_CASES)
def test_integrate_case_conditioning(cid, steps):
    """The trajectories the GPU test compares at 1e-9 are themselves good to 1e-10: on every state
    key the float64 projection's loop lands within 1e-10 of the KKT reference's loop."""
    cs = HC.build_case(cid)
    worst = 0.0
    for i, (ref, _, status) in enumerate(HC.integrate_reference(cid, steps)):
        assert status == HR.OK
        got = HR.integrate_projection(cs["model"], cs["states"], cs["tasks"], cs["rows"], i, steps, HC.DT)
        worst = max(worst, max(FM.rel_err(got[k], ref[k]) for k in ref))
    print(f"{cid} steps {steps}: projection loop against KKT loop {worst:.2e}")
    assert worst < 1e-10, (cid, steps, worst)


def test_soft_mask_is_the_soft_reference():
    """rows == 0: ik_hard_reference.solve is ik_reference.solve."""
    cs = HC.build_case("rand24-k2com-15")
    for i in range(cs["B"]):
        a = HR.solve(cs["model"], cs["states"], cs["tasks"], 0, i)
        b = IK.solve(cs["model"], cs["states"], cs["tasks"], i)
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1] == b[1] == IK.OK


def test_standing_ik_hard_is_both_soles_and_com_xy():
    model = robot.humanoid24()
    h = native.Handle.ik_hard(**robot.standing_ik_hard(model))
    assert h.rows == HR.mask([HC.ALL, HC.ALL], HC.COMXY) == 0xfff | (3 << 24)
    assert h.reserved == 0 and h.rel_pivot_min == 0.0
    assert native.Handle.ik_hard([HC.LIN], [False, False, True], 1e-6).rows == 0x7 | (4 << 24)
    assert native.IK_HARD_DEPENDENT == HR.HARD_DEPENDENT == 3


def test_symbols_are_exported():
    assert {"blf_fb_ik_solve_hard", "blf_fb_ik_integrate_hard"} <= set(native.EXPORTED)
    L = native.lib()
    assert L.blf_fb_ik_solve_hard and L.blf_fb_ik_integrate_hard


# ---- argument validation through ctypes with batch = 0: no device is touched ---------------------
_FAKE = ctypes.c_void_p(1)   # the handle is only compared with null before any device work
_PTR = 8                     # likewise every buffer
INVALID, UNSUPPORTED = 1, 3


def _call(fn="solve", rows=0x3f, reserved=0, tau=0.0, nse3=2, com=True, hard=True, batch=0, steps=1, dT=0.01,
          handle=_FAKE, ndof=24):
    m = native.FbModel()
    m.ndof, m.nframes = ndof, 4
    for k in ("parent", "joint_origin", "joint_rot", "joint_axis", "link_mass", "link_com", "link_inertia",
              "frame_link", "frame_pose"):
        setattr(m, k, _PTR)
    t = native.IkTasks()
    t.nse3 = nse3
    for k in ("frame", "se3_weight", "se3_kp", "se3_pose", "joint_weight", "joint_kp", "joint_pos"):
        setattr(t, k, _PTR)
    if com:
        t.com_weight = t.com_pos = _PTR
    s = native.FbState()
    h = native.IkHard()
    h.rows, h.reserved, h.rel_pivot_min = rows, reserved, tau
    hp = ctypes.byref(h) if hard else None
    L = native.lib()
    if fn == "solve":
        return L.blf_fb_ik_solve_hard(handle, ctypes.byref(m), ctypes.byref(s), ctypes.byref(t), hp, batch, None,
                                      None, None)
    return L.blf_fb_ik_integrate_hard(handle, ctypes.byref(m), ctypes.byref(s), ctypes.byref(t), hp, batch, steps,
                                      dT, None, None, None)


@pytest.mark.parametrize("fn", ["solve", "integrate"])
@pytest.mark.parametrize("kw,code,word", [
    (dict(rows=1 << 27), INVALID, "above 26"),
    (dict(rows=1 << 31), INVALID, "above 26"),
    (dict(rows=1 << 12), INVALID, "nse3"),            # SE3 task 2 of K = 2
    (dict(rows=1 << 23, nse3=3), INVALID, "nse3"),    # SE3 task 3 of K = 3
    (dict(rows=1, nse3=0), INVALID, "nse3"),
    (dict(rows=1 << 24, com=False), INVALID, "CoM"),
    (dict(rows=7 << 24, com=False, nse3=0), INVALID, "CoM"),
    (dict(reserved=1), INVALID, "reserved"),
    (dict(rows=0, reserved=-1), INVALID, "reserved"),
    (dict(tau=1.0), INVALID, "rel_pivot_min"),
    (dict(tau=-1e-9), INVALID, "rel_pivot_min"),
    (dict(tau=float("nan")), INVALID, "rel_pivot_min"),
    (dict(tau=float("inf")), INVALID, "rel_pivot_min"),
    (dict(handle=None), INVALID, "handle"),
    (dict(batch=-1), INVALID, "batch"),
    (dict(nse3=5), UNSUPPORTED, "nse3"),
    (dict(ndof=49), UNSUPPORTED, "ndof"),
])
def test_hard_calls_reject_bad_arguments(fn, kw, code, word):
    assert _call(fn, **kw) == code
    assert f"blf_fb_ik_{fn}_hard" in native.last_error() and word in native.last_error()


def test_integrate_hard_rejects_bad_steps_and_dt():
    assert _call("integrate", steps=0) == INVALID and "steps" in native.last_error()
    for dT in (0.0, -0.01, float("nan"), float("inf")):
        assert _call("integrate", dT=dT) == INVALID and "dT" in native.last_error()


@pytest.mark.parametrize("fn", ["solve", "integrate"])
def test_empty_batch_is_ok_without_a_device(fn):
    assert _call(fn) == 0
    assert _call(fn, rows=0xffffff | (7 << 24), nse3=4, tau=0.5) == 0
    assert _call(fn, hard=False) == 0
    assert _call(fn, rows=0) == 0


def test_planted_feet_on_the_reference():
    """ik_hard_cases.planted_feet as tests/test_gpu_ik_hard.py uses it, on the reference: with the
    hard rows every sole's pose error shrinks over 20 steps; with the weights alone every robot ends
    with a sole further from its set point than it began."""
    cs = HC.planted_feet()
    model, tasks = cs["model"], cs["tasks"]
    for i in range(cs["B"]):
        e0 = HC.sole_errors(model, tasks, {k: cs["states"][k][i] for k in IK.STATE_KEYS}, i)
        hs, _, hst = HR.integrate(model, cs["states"], tasks, cs["rows"], i, 20, HC.DT)
        ss, _, sst = IK.integrate(model, cs["states"], tasks, i, 20, HC.DT)
        assert hst == sst == HR.OK
        assert (HC.sole_errors(model, tasks, hs, i) <= 0.5 * e0).all()
        assert (HC.sole_errors(model, tasks, ss, i) > e0).any()
