"""tests/ik_reference.py (the numpy restatement of include/blf/blf_c.h section 12 that checks
blf_fb_ik_solve / blf_fb_ik_integrate) pinned on the CPU: its Jacobians against finite differences
and against the mass matrix, the closed loop it is for, and the conditioning of every case of
tests/ik_cases.py."""
import numpy as np
import pytest

import fb_dynamics as F
import fb_models as FM
import ik_cases as IC
import ik_reference as IK
import swing_foot_reference as SR
from blf import robot
from blf.robot import _rotvec


def _models():
    rand = FM.random_tree(9, 5)
    return {"rand9": FM.tree_model(rand, 5),
            "pri-rand9": FM.tree_model(rand, 5, prismatic=FM._tree_prismatic(rand)),
            "pri-chain4": FM.tree_model(FM.chain(4), 6, prismatic=[0, 2])}


MODELS = _models()


def _state(model, seed):
    st = robot.random_states(model, 1, seed=seed)
    return {k: st[k][0] for k in IK.STATE_KEYS}


def _moved(model, s, nu, eps):
    """The state moved along nu by eps: p + eps v, Exp(eps w) R, s + eps s_dot (mixed velocities)."""
    return dict(base_pos=s["base_pos"] + eps * nu[:3], base_rot=_rotvec(eps * nu[3:6]) @ s["base_rot"],
                joint_pos=s["joint_pos"] + eps * nu[6:])


@pytest.mark.parametrize("name", sorted(MODELS))
def test_com_jacobian(name):
    """J_c equals the first three rows of the mass matrix over the total mass, and a central finite
    difference of the centre of mass along every generalized direction (prismatic joints included)."""
    model = MODELS[name]
    s = _state(model, 3)
    K = IK.kin(model, s)
    J = IK.com_jacobian(model, K)
    M, _ = F.mass_and_bias(model, K)
    np.testing.assert_allclose(J, M[:3] / IK.com(model, K)[1], rtol=0, atol=1e-14)
    eps = 1e-6
    for c in range(6 + model["n"]):
        e = np.zeros(6 + model["n"])
        e[c] = 1.0
        cp = IK.com(model, IK.kin(model, _moved(model, s, e, eps)))[0]
        cm = IK.com(model, IK.kin(model, _moved(model, s, e, -eps)))[0]
        np.testing.assert_allclose((cp - cm) / (2 * eps), J[:, c], rtol=0, atol=1e-8)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_frame_jacobians(name):
    """Every frame's mixed Jacobian equals a central finite difference of the frame pose: the
    origin's velocity, and Log(R(+) R(-)^T) / (2 eps) for the angular rows."""
    model = MODELS[name]
    s = _state(model, 4)
    K = IK.kin(model, s)
    eps = 1e-6
    for f in range(len(model["frame_link"])):
        J = F.frame_state(model, K, f)[3]
        for c in range(6 + model["n"]):
            e = np.zeros(6 + model["n"])
            e[c] = 1.0
            pp, Rp, _, _ = F.frame_state(model, IK.kin(model, _moved(model, s, e, eps)), f)
            pm, Rm, _, _ = F.frame_state(model, IK.kin(model, _moved(model, s, e, -eps)), f)
            np.testing.assert_allclose((pp - pm) / (2 * eps), J[:3, c], rtol=0, atol=1e-8)
            np.testing.assert_allclose(IK.log3(Rp, Rm) / (2 * eps), J[3:, c], rtol=0, atol=1e-8)


def test_integrated_pose_error_decreases():
    """One SE3 task of large weight with a reachable target (the frame's pose at other joint
    positions): the pose error falls at every one of 20 integration steps."""
    model = FM.tree_model(FM.chain(7), 8)
    st = robot.random_states(model, 1, seed=2)
    goal = {k: st[k][0] for k in IK.STATE_KEYS}
    goal["joint_pos"] = goal["joint_pos"] + np.random.default_rng(1).normal(size=7) * 0.3
    f = 1   # the deepest leaf
    pg, Rg, _, _ = F.frame_state(model, IK.kin(model, goal), f)
    tasks = dict(frame=np.array([f], dtype=np.int32), se3_weight=np.full((1, 6), 100.0),
                 se3_kp=np.array([[10.0, 10.0]]), se3_pose=np.concatenate([pg, Rg.reshape(-1)])[None, None],
                 se3_twist=None, com_weight=None, com_kp=0.0, com_pos=None, com_vel=None,
                 joint_weight=np.full(7, 1e-2), joint_kp=np.zeros(7), joint_pos=st["joint_pos"], joint_vel=None,
                 base_damping=1e-2)

    def err(s):
        pf, Rf, _, _ = F.frame_state(model, IK.kin(model, s), f)
        return np.linalg.norm(np.concatenate([pg - pf, IK.log3(Rg, Rf)]))
    cur = {k: st[k].copy() for k in IK.STATE_KEYS}
    errs = [err({k: v[0] for k, v in cur.items()})]
    for _ in range(20):
        out, _, status = IK.integrate(model, cur, tasks, 0, 1, 0.01)
        assert status == IK.OK
        cur = {k: out[k][None] for k in IK.STATE_KEYS}
        errs.append(err({k: v[0] for k, v in cur.items()}))
    assert all(b < a for a, b in zip(errs, errs[1:])), errs
    assert errs[-1] < 0.2 * errs[0]


def test_integrate_steps_compose():
    """integrate(steps = 3) is three integrate(steps = 1) calls, bit for bit."""
    cs = IC.build_case("rand24-k2com")
    model, tasks = cs["model"], cs["tasks"]
    out3, nu3, st3 = IK.integrate(model, cs["states"], tasks, 1, 3, 0.01)
    cur = {k: cs["states"][k][1:2] for k in IK.STATE_KEYS}
    for _ in range(3):
        out, nu, st = IK.integrate(model, cur, IK.tasks_at(tasks, 1), 0, 1, 0.01)
        cur = {k: out[k][None] for k in IK.STATE_KEYS}
    for k in out3:
        np.testing.assert_array_equal(out3[k], out[k])
    np.testing.assert_array_equal(nu3, nu)
    assert st3 == st == IK.OK


def test_log_is_the_swing_foot_reference():
    R0, R1 = _rotvec(np.array([0.2, -0.1, 0.3])), _rotvec(np.array([-0.4, 0.5, 0.1]))
    u, th = SR.log_rel(R1, R0)
    np.testing.assert_array_equal(IK.log3(R1, R0), th * u)
    np.testing.assert_allclose(_rotvec(IK.log3(R1, R0)) @ R0, R1, rtol=0, atol=1e-14)


@pytest.mark.parametrize("cid", sorted(IC.CASES))
def test_case_conditioning(cid):
    """The conditioning guard of tests/test_fb_models.py for the IK cases: on every robot of every
    case of the GPU matrix a plain float64 Cholesky solve agrees with the refined solve to 1e-10
    (rel_err), so the reference itself is ten times better than the device's 1e-9 bar."""
    cs = IC.build_case(cid)
    worst = 0.0
    for i, (nu, status, H, g) in enumerate(IC.reference(cid)):
        assert status == IK.OK, (cid, i)
        worst = max(worst, FM.rel_err(IK.cholesky_solve(H, g), nu))
    print(f"{cid}: Cholesky against refined solve rel_err {worst:.2e}")
    assert worst < 1e-10, (cid, worst)


def test_failures_of_the_reference():
    """Which inputs fail, on the reference: a frame index out of range and a NaN set point are
    BAD_INPUT; a finite base_rot scaled by 1e160 overflows H (1e320) and is NOT_POSITIVE."""
    cs = IC.build_case("rand24-k2com")
    model, st, tasks = cs["model"], cs["states"], cs["tasks"]
    t = dict(tasks, frame=np.array([1, len(model["frame_link"])], dtype=np.int32))
    assert IK.solve(model, st, t, 0)[1] == IK.BAD_INPUT
    pose = tasks["se3_pose"].copy()
    pose[1, 0, 4] = np.nan
    t = dict(tasks, se3_pose=pose)
    assert IK.solve(model, st, t, 1)[1] == IK.BAD_INPUT
    assert IK.solve(model, st, t, 0)[1] == IK.OK
    big = {k: v.copy() for k, v in st.items()}
    big["base_rot"][2] = big["base_rot"][2] * 1e160
    assert np.isfinite(big["base_rot"]).all()
    nu, status, _, _ = IK.solve(model, big, tasks, 2)
    assert status == IK.NOT_POSITIVE and np.isnan(nu).all()
