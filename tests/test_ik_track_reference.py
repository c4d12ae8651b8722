"""CPU checks of the reference-tracking IK's reference and case matrix (include/blf/blf_c.h section
12d): every (case, robot, step) of tests/ik_track_cases.py ends as intended and inside the conditioning
band that keeps tests/test_gpu_ik_track.py's exact iters / active comparison honest, the matrix covers
the paths the device test relies on, and the scenario the call is for behaves as section 12d says."""
import numpy as np
import pytest

import ik_limits_reference as LR
import ik_track_cases as TC
import ik_track_reference as TR
from blf import native, robot

PIVOT_OK, PIVOT_FAIL = 1.0e-5, 1.0e-11   # tests/ik_hard_cases.py's bands for the pivots of S


def _in_band(r):
    ok = r["margin"] >= LR.BAND
    for rel, passed in r["pivots"]:
        if rel.size:
            ok = ok and ((rel.min() >= PIVOT_OK) if passed else (abs(rel[-1]) <= PIVOT_FAIL))
    return ok


@pytest.mark.parametrize("cid", TC.CASES)
def test_case_conditioning(cid):
    """Every robot ends with the intended status; every step of a robot that resolves is at least 1e-7
    (relative) from a tie in every comparison of the rule, with the pivots of S above 1e-5; a robot
    meant to be dependent fails at step 0, by count (no pivot is met) or with a pivot below 1e-11."""
    cs, ref = TC.build_case(cid), TC.reference(cid)
    NV = cs["model"]["n"] + 6
    for i, r in enumerate(ref):
        assert r["status"] == cs["expect"][i], (cid, i, r["status"], r["fail_step"])
        if r["status"] == LR.OK:
            assert r["fail_step"] == -1 and len(r["steps"]) == cs["schedule"]["steps"]
            for t, s in enumerate(r["steps"]):
                assert s["status"] == LR.OK and _in_band(s), (cid, i, t, s["margin"], s["pivots"])
        else:
            assert r["fail_step"] == 0 and np.isnan(r["joint_traj"]).all()
            over = bin(r["rows"][0]).count("1") > NV
            rel, passed = r["steps"][0]["pivots"][0]
            assert not passed and ((over and rel.size == 0) or abs(rel[-1]) <= PIVOT_FAIL), (cid, i, rel)
        print(cid, i, "status", r["status"], "iters", r["iters"], "active", r["active"],
              "margin %.3g" % min([s["margin"] for s in r["steps"]] + [np.inf]))


def test_case_matrix_covers_the_paths():
    """What tests/test_gpu_ik_track.py relies on: in the walking pair the two robots of wavefront 0 hold
    different masks at some step and each robot's mask changes within the call (a lift-off and a
    touch-down); a bound is active somewhere; the limbs12 pair's union counts more rows than 6 + n while
    each robot's own mask does not; limbs48 has a different mask per robot at every step."""
    w = TC.reference("walk")
    assert any(a != b for a, b in zip(w[0]["rows"], w[1]["rows"]))
    for r in w:
        pop = [bin(m).count("1") for m in r["rows"]]
        assert any(b < a for a, b in zip(pop, pop[1:])) and any(b > a for a, b in zip(pop, pop[1:])), pop
    assert any(s["active"] != (0, 0) for r in w for s in r["steps"])
    assert any(s["iters"] > 1 for r in w for s in r["steps"])
    cs, l = TC.build_case("limbs12"), TC.reference("limbs12")
    NV = cs["model"]["n"] + 6
    own = [bin(r["rows"][0]).count("1") for r in l]
    assert max(own) <= NV < bin(l[0]["rows"][0] | l[1]["rows"][0]).count("1"), own
    b = TC.reference("limbs48")
    assert all(len({r["rows"][t] for r in b}) == 3 for t in range(4))


def test_prefix_is_the_shorter_call():
    """A T-step call is the first T steps of a longer one with the same slices (what the GPU test's
    T = 1 and 2 use): TR.track on the truncated schedule equals TC.prefix bit for bit."""
    cs, ref = TC.build_case("walk"), TC.reference("walk")
    sch = cs["schedule"]
    short = dict(sch, steps=2, contact=sch["contact"][:, :, :2], se3_pose=sch["se3_pose"][:, :, :2],
                 se3_twist=sch["se3_twist"][:, :, :2], com_pos=sch["com_pos"][:, :2])
    r = TR.track(cs["model"], cs["states"], cs["tasks"], cs["rows"], cs["limits"], short, 1, cs["dT"])
    p = TC.prefix(ref[1], 2)
    for k in ("joint_traj", "base_traj", "nu_traj"):
        np.testing.assert_array_equal(r[k], p[k])
    assert (r["iters"], r["active"], r["status"]) == (p["iters"], p["active"], p["status"])
    for k in native.FB_STATE_KEYS:
        np.testing.assert_array_equal(np.asarray(r["state"][k]), np.asarray(p["state"][k]), err_msg=k)


STANCE_LAW_TOL, CONTRAST_MIN = TC.STANCE_LAW_TOL, TC.CONTRAST_MIN


def test_stance_soles_follow_the_hard_rows_law():
    """What the call is for, on the reference: every stance sole's linear error shrinks by (1 - kp_lin
    dT) per step of its contact, to the Euler step's second-order drift; with stance_rows = 0 (weights
    only) the stance soles are far further from that law."""
    cs, ref = TC.build_case("walk"), TC.reference("walk")
    soft = dict(cs["schedule"], stance_rows=0)
    worst = away = 0.0
    for i in range(cs["B"]):
        r = ref[i]
        e, _ = TC.stance_law_error(cs["model"], cs["tasks"], cs["states"], cs["schedule"], i, r["base_traj"],
                                   r["joint_traj"], cs["dT"])
        s = TR.track(cs["model"], cs["states"], cs["tasks"], cs["rows"], cs["limits"], soft, i, cs["dT"])
        assert s["status"] == LR.OK
        a, _ = TC.stance_law_error(cs["model"], cs["tasks"], cs["states"], cs["schedule"], i, s["base_traj"],
                                   s["joint_traj"], cs["dT"])
        worst, away = max(worst, e), max(away, a)
    print(f"stance soles against the law: hard rows {worst:.3g} m, weights only {away:.3g} m")
    assert worst <= 0.75 * STANCE_LAW_TOL
    assert away >= 1.15 * CONTRAST_MIN


def test_walking_ik_schedule_shapes_and_phases():
    """robot.walking_ik_schedule: neighbours half a cycle apart by default, every sole's first contact is
    its nominal pose, its second one step ahead, and the CoM reference leans towards the stance sole."""
    model = robot.humanoid24()
    st = robot.standing_states(model, 4, seed=1)
    w = robot.walking_ik_schedule(model, st, 20, 0.01)
    assert w["contact_pose"].shape == (8, 2, 12) and w["tq"].shape == (8, 20) and w["com_pos"].shape == (4, 20, 3)
    assert w["stance_rows"] == 0xFFF
    null = robot.sole_null_poses(model, st).reshape(8, 12)
    np.testing.assert_array_equal(w["contact_pose"][:, 0], null)
    np.testing.assert_allclose(w["contact_pose"][:, 1, 0] - null[:, 0], 0.04)
    lift = w["contact_time"][:, 0, 1].reshape(4, 2)
    np.testing.assert_allclose(lift[0], [0.02, 0.12])
    np.testing.assert_allclose(lift[1], [0.12, 0.02])
    np.testing.assert_array_equal(lift[2], lift[0])
    sch = TC.swing_schedule(w, 4, 2)
    mid = null.reshape(4, 2, 12)[:, :, 1].mean(axis=1)
    for b in range(4):
        for k in range(2):
            sw = sch["contact"][b, k] == 0
            assert sw.any() and not sw.all()
            other = null.reshape(4, 2, 12)[b, 1 - k, 1]
            lean = (w["com_pos"][b, sw, 1] - mid[b]) * np.sign(other - mid[b])
            assert (lean >= 0.0).all() and lean.max() > 0.01
