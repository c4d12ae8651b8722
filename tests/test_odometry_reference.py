"""CPU tests of tests/odometry_reference.py (the checker of section 13) against facts that do not
depend on it: it recovers a known base, its twist holds the fixed frame at rest (through the oracle's
Jacobian), a switch leaves the pose continuous and stores the new frame's world pose, and the trigger
follows its truth table."""
import numpy as np

import fb_dynamics as F
import fb_models as FM
import odometry_reference as OR
from blf import robot

PRM = np.array([10.0, 4.0, 0.0, 0.0])


def _model():
    # a branching tree with a prismatic joint; frames on four links
    return FM.tree_model(FM.random_tree(9, 5), seed=11, prismatic=(3,))


def _true_state(model, seed):
    s = robot.random_states(model, 1, seed=seed)
    s["base_pos"] = s["base_pos"] + np.array([[0.7, -1.3, 0.2]])
    return {k: v[0] for k, v in s.items()}


def _frame_world(model, base_pos, base_rot, q, base_vel, qd, f):
    K = F.kinematics(model, base_pos, base_rot, q, base_vel, qd)
    return F.frame_state(model, K, f)


def test_recovers_a_known_base_and_keeps_the_fixed_frame_at_rest():
    model = _model()
    frames = [1, 3]
    for seed in range(4):
        s = _true_state(model, seed)
        fp = OR.initial_fixed_pose(model, s, frames[1])
        o = OR.advance_one(model, frames, PRM, [0.0], s["joint_pos"][None], s["joint_vel"][None],
                           np.array([[0.0, 20.0]]), [0, 1], np.zeros((2, 2)), 1, fp)
        assert o["status"] == OR.OK and o["fixed_out"][0] == 1
        assert np.abs(o["base_pos"][0] - s["base_pos"]).max() < 1e-14
        assert np.abs(o["base_rot"][0] - s["base_rot"]).max() < 1e-14
        # the fixed frame's mixed velocity J (base_vel, joint_vel) vanishes; so does frame_state's own
        _, _, vel, J = _frame_world(model, o["base_pos"][0], o["base_rot"][0], s["joint_pos"], o["base_vel"][0],
                                    s["joint_vel"], frames[1])
        nu = np.concatenate([o["base_vel"][0], s["joint_vel"]])
        scale = np.abs(J).max() * np.abs(nu).max()
        assert np.abs(J @ nu).max() < 1e-14 * max(1.0, scale)
        assert np.abs(vel).max() < 1e-14 * max(1.0, scale)


def test_pose_is_continuous_at_a_switch_and_the_new_frame_is_stored():
    model = _model()
    frames = [1, 3, 2]
    s = _true_state(model, 7)
    fp = OR.initial_fixed_pose(model, s, frames[0])
    rng = np.random.default_rng(3)
    q = s["joint_pos"][None] + rng.normal(size=(3, model["n"])) * 0.05
    qd = rng.normal(size=(3, model["n"])) * 0.3
    # slot 0 on until step 1, where it breaks and slot 2 makes on the same sample
    force = np.array([[20.0, 0.0, 0.0], [0.0, 0.0, 20.0], [0.0, 0.0, 20.0]])
    args = (model, frames, PRM, [0.0, 0.1, 0.2], q, qd)
    sw = OR.advance_one(*args, force, [1, 0, 0], np.zeros((3, 2)), 0, fp)
    held = OR.advance_one(*args, np.array([[20.0, 0.0, 0.0]] * 3), [1, 0, 0], np.zeros((3, 2)), 0, fp)
    assert list(sw["fixed_out"]) == [0, 2, 2] and list(held["fixed_out"]) == [0, 0, 0]
    # the switching step's pose is the pose without the switch, bit for bit
    assert np.array_equal(sw["base_pos"][1], held["base_pos"][1]) and np.array_equal(sw["base_rot"][1], held["base_rot"][1])
    # and the stored fixed_pose is the new frame's world pose at the estimated state, then and later
    for t in (1, 2):
        pf, Rf, vel, _ = _frame_world(model, sw["base_pos"][t], sw["base_rot"][t], q[t], sw["base_vel"][t], qd[t], frames[2])
        assert np.abs(pf - sw["fixed_pose"][:3]).max() < 1e-14
        assert np.abs(Rf.reshape(-1) - sw["fixed_pose"][3:]).max() < 1e-14
        assert np.abs(vel).max() < 1e-14


def test_no_contact_dead_reckons_on_the_last_foot_and_ties_take_the_lowest_slot():
    assert OR.choose_fixed(1, np.array([0, 0, 0]), np.array([0.0, 0.0, 0.0])) == 1
    assert OR.choose_fixed(1, np.array([1, 1, 0]), np.array([5.0, 0.0, 0.0])) == 1      # still on: kept
    assert OR.choose_fixed(1, np.array([1, 0, 1]), np.array([0.3, 9.0, 0.3])) == 0      # tie: lowest slot
    assert OR.choose_fixed(1, np.array([1, 0, 1]), np.array([0.2, 9.0, 0.3])) == 2      # latest switch


def _run(prm, samples, state=0, timers=(0.0, 0.0)):
    e, w = timers
    out = []
    for t, v in samples:
        state, e, w = OR.trigger_step(np.asarray(prm, dtype=np.float64), t, v, state, e, w)
        out.append((state, e, w))
    return out


def test_trigger_truth_table():
    # equality at both thresholds with zero delays: >= switches on, <= switches off, on the sample itself
    r = _run([10.0, 4.0, 0.0, 0.0], [(0.0, 9.999), (1.0, 10.0), (2.0, 4.001), (3.0, 4.0)])
    assert [s for s, _, _ in r] == [0, 1, 1, 0]
    assert r[1][2] == 1.0 and r[3][2] == 3.0 and r[2][2] == 1.0
    # a delay of several samples: pending from the first crossing, on when t - edge_time >= delay
    r = _run([10.0, 4.0, 0.25, 0.5], [(0.0, 11.0), (0.125, 11.0), (0.25, 11.0), (0.375, 3.0), (0.75, 3.0), (0.875, 3.0)])
    assert [s for s, _, _ in r] == [2, 2, 1, 3, 3, 0]
    assert r[2][1] == 0.0 and r[2][2] == 0.25 and r[5][1] == 0.375 and r[5][2] == 0.875
    # chatter: a sample back inside the band clears the pending edge, and the next crossing restamps it
    r = _run([10.0, 4.0, 0.25, 0.25], [(0.0, 11.0), (0.125, 9.0), (0.25, 11.0), (0.375, 11.0), (0.5, 11.0)])
    assert [s for s, _, _ in r] == [2, 0, 2, 2, 1]
    assert r[4][1] == 0.25 and r[4][2] == 0.5
    # a non-finite sample or time changes nothing, a pending edge included
    r = _run([10.0, 4.0, 0.25, 0.25], [(0.0, 11.0), (0.125, np.nan), (np.inf, 11.0), (0.25, -np.inf), (0.375, 11.0)])
    assert [s for s, _, _ in r] == [2, 2, 2, 2, 1] and r[4][1] == 0.0


def test_trigger_advance_is_the_step_over_the_batch():
    rng = np.random.default_rng(0)
    T, B, K = 7, 3, 2
    value = rng.uniform(0.0, 14.0, (T, B, K))
    time = np.arange(T) * 0.125
    prm = np.array([[10.0, 4.0, 0.125, 0.0], [8.0, 8.0, 0.0, 0.25]])
    st, tm, out = OR.trigger_advance(prm, time, value, np.zeros((B, K), dtype=np.int32), np.zeros((B, K, 2)))
    for b in range(B):
        for c in range(K):
            r = _run(prm[c], zip(time, value[:, b, c]))
            assert [s & 1 for s, _, _ in r] == list(out[:, b, c])
            assert r[-1] == (st[b, c], tm[b, c, 0], tm[b, c, 1])


def test_bad_robot_is_nan_from_that_step_on():
    model = _model()
    frames = [1, 3]
    s = _true_state(model, 2)
    fp = OR.initial_fixed_pose(model, s, frames[0])
    q = np.repeat(s["joint_pos"][None], 4, axis=0)
    q[2, 4] = np.nan
    force = np.array([[20.0, 0.0]] * 4)
    o = OR.advance_one(model, frames, PRM, np.arange(4) * 0.1, q, None, force, [1, 0], np.zeros((2, 2)), 0, fp)
    assert o["status"] == OR.BAD_INPUT and list(o["fixed_out"]) == [0, 0, -1, -1]
    assert np.isfinite(o["base_pos"][:2]).all() and np.isnan(o["base_pos"][2:]).all() and np.isnan(o["fixed_pose"]).all()
    assert o["contact"].tolist() == [[1, 0]] * 4
    for bad_fixed in (-1, 2):
        o = OR.advance_one(model, frames, PRM, [0.0], q[:1], None, force[:1], [1, 0], np.zeros((2, 2)), bad_fixed, fp)
        assert o["status"] == OR.BAD_INPUT and o["fixed_frame"] == bad_fixed and o["fixed_out"][0] == -1
    o = OR.advance_one(model, [1, 99], PRM, [0.0], q[:1], None, force[:1], [1, 0], np.zeros((2, 2)), 0, fp)
    assert o["status"] == OR.BAD_INPUT and np.isnan(o["base_rot"]).all()
