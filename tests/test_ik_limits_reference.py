"""CPU checks of the joint-limit IK's reference and case matrix (include/blf/blf_c.h section 12c):
tests/ik_limits_reference.py's rule against its independent certificate, the conditioning band of every
case of tests/ik_limits_cases.py, the default iteration bound, and the scenario the feature is for."""
import numpy as np
import pytest

import fb_models as FM
import ik_hard_cases as HC
import ik_hard_reference as HR
import ik_limits_cases as LC
import ik_limits_reference as LR
import ik_reference as IK
from blf import robot

PIVOT_OK, PIVOT_FAIL = 1.0e-5, 1.0e-11   # tests/ik_hard_cases.py's bands for the pivots of S


@pytest.mark.parametrize("cid", LC.OK_CASES)
def test_rule_is_certified(cid):
    """Every robot of every OK case resolves, its final set passes the dense-KKT certificate, and the
    rule's nu equals the certified nu to 1e-10."""
    ref, cert = LC.reference(cid), LC.certificate(cid)
    for i, (r, (nu, good)) in enumerate(zip(ref, cert)):
        assert r["status"] == LR.OK and good, (cid, i, r["status"], good)
        assert FM.rel_err(r["nu"], nu) < 1.0e-10, (cid, i)
        sd = r["nu"][6:]
        assert (sd >= r["lo"] - 1e-12).all() and (sd <= r["up"] + 1e-12).all()
        if r["parts"][4].shape[0]:
            assert np.abs(r["parts"][4] @ r["nu"] - r["parts"][5]).max() <= 1e-12 * max(1.0, np.abs(r["parts"][5]).max())


def _in_band(r):
    ok = r["margin"] >= LR.BAND
    for rel, passed in r["pivots"]:
        if rel.size:
            ok = ok and ((rel.min() >= PIVOT_OK) if passed else (abs(rel[-1]) <= PIVOT_FAIL))
    return ok


@pytest.mark.parametrize("cid", LC.OK_CASES + [LC.MIXED_CASE])
def test_case_conditioning(cid):
    """Every comparison the rule makes on a robot that resolves is at least 1e-7 (relative) from a
    tie, and every pivot of S is inside the bands of tests/ik_hard_cases.py: rounding cannot flip a
    decision on the device."""
    for i, r in enumerate(LC.reference(cid)):
        if cid == LC.MIXED_CASE and i == LC.MIXED_BAD:
            continue
        assert r["status"] == LR.OK and _in_band(r), (cid, i, r["margin"], r["pivots"])


def test_case_matrix_covers_the_paths():
    """The matrix has what tests/test_gpu_ik_limits.py relies on: two robots of one wavefront with
    different iteration counts, a case that leaves block mode, bounds on joint 0 and on joint n - 1,
    both sides, and more than one iteration everywhere a bound is active."""
    r = LC.reference("rand24-hard-15")
    assert r[0]["iters"] != r[1]["iters"]
    assert any(x["left_block"] for x in LC.reference("rand24-hard-9-block"))
    first = last = lower = upper = False
    for cid in LC.OK_CASES:
        n = LC.build_case(cid)["model"]["n"]
        for x in LC.reference(cid):
            wl, wu = x["active"]
            first, last = first or bool((wl | wu) & 1), last or bool(((wl | wu) >> (n - 1)) & 1)
            lower, upper = lower or wl != 0, upper or wu != 0
    assert first and last and lower and upper


def test_default_max_iter():
    """BLF_IK_LIMITS_DEFAULT_MAX_ITER is at least twice the largest count the reference needs."""
    worst = max(r["iters"] for cid in LC.OK_CASES for r in LC.reference(cid))
    print("largest iteration count of the case matrix:", worst)
    assert LR.DEFAULT_MAX_ITER >= 2 * worst
    src = open(FM.__file__.replace("tests/fb_models.py", "include/blf/blf_c.h")).read()
    assert f"#define BLF_IK_LIMITS_DEFAULT_MAX_ITER {LR.DEFAULT_MAX_ITER}\n" in src


@pytest.mark.parametrize("cid", LC.INFEASIBLE_CASES + [LC.MIXED_CASE])
def test_infeasible_cases(cid):
    """The LP finds no point in the box that satisfies the hard rows, and the rule ends unresolved."""
    for i, r in enumerate(LC.reference(cid)):
        if cid == LC.MIXED_CASE and i != LC.MIXED_BAD:
            continue
        assert r["status"] == LR.LIMITS_UNRESOLVED and np.isnan(r["nu"]).all()
        assert not LR.feasible(r["parts"], r["lo"], r["up"]), (cid, i)


@pytest.mark.parametrize("cid", ["chain3-k4-7", "rand24-k2com-15", "chain27-k2com-9", "pri-rand48-k2-12"])
def test_infinite_limits_are_the_hard_solve(cid):
    """All-infinite limits: one iteration, no active bound, and ik_hard_reference.solve's nu."""
    cs = HC.build_case(cid)
    lim = LR.no_limits(cs["model"]["n"])
    for i in range(cs["B"]):
        r = LR.solve(cs["model"], cs["states"], cs["tasks"], cs["rows"], lim, i)
        assert r["status"] == LR.OK and r["iters"] == 1 and r["active"] == (0, 0)
        assert FM.rel_err(r["nu"], HC.reference(cid)[i][0]) < 1.0e-10


@pytest.mark.parametrize("cid", LC.INTEGRATE_CASES)
def test_integrate_case_conditioning(cid):
    """The screening of INTEGRATE_CASES: over 20 steps the rule's trajectory and the certified one
    agree to 1e-10 on every state key, every step resolving."""
    a, b = LC.integrate_reference(cid, 20), LC.integrate_reference(cid, 20, certified=True)
    for (sa, _, st, _, _), (sb, _, stb, _, _) in zip(a, b):
        assert st == stb == LR.OK
        for k in sa:
            assert FM.rel_err(sa[k], sb[k]) < 1.0e-10, (cid, k)


def test_humanoid_joint_limits():
    """robot.humanoid24_joint_limits: ordered ranges around the nominal posture, the knees' lower
    limit at straight."""
    model = robot.humanoid24()
    lim = robot.humanoid24_joint_limits(model)
    names = model["names"][1:]
    assert (lim["pos_lower"] <= 0.0).all() and (lim["pos_upper"] > 0.0).all() and (lim["vel_max"] > 0).all()
    for k in ("l_knee", "r_knee"):
        assert lim["pos_lower"][names.index(k)] == 0.0


def test_what_the_limits_are_for():
    """ik_limits_cases.raised_com on the reference: without limits a knee leaves its range within 20
    steps on every robot; with them every joint stays in range and no sole ends further from its set
    point than it began."""
    cs = LC.raised_com()
    model, lim = cs["model"], cs["limits"]
    for i in range(cs["B"]):
        free, _, st = HR.integrate(model, cs["states"], cs["tasks"], cs["rows"], i, 20, LC.DT)
        assert st == HR.OK and (free["joint_pos"] < lim["pos_lower"] - 1e-3).any()
        held, _, st, iters, act = LR.integrate(model, cs["states"], cs["tasks"], cs["rows"], lim, i, 20, LC.DT)
        assert st == LR.OK and act[0] != 0
        assert (held["joint_pos"] >= lim["pos_lower"] - 1e-12).all()
        assert (held["joint_pos"] <= lim["pos_upper"] + 1e-12).all()
        e0 = HC.sole_errors(model, cs["tasks"], {k: cs["states"][k][i] for k in IK.STATE_KEYS}, i)
        e1 = HC.sole_errors(model, cs["tasks"], {k: held[k] for k in IK.STATE_KEYS}, i)
        assert (e1 <= e0).all()
