"""CPU checks of tests/inverse_dynamics_reference.py, the checker of blf_fb_inverse_dynamics and
blf_fbd_euler_integrate_computed_torque_traj, by self-consistency against oracle/fb_dynamics.py on
humanoid24, its prismatic variant and an fb_models random tree (non-DFS, eight contacts of mixed laws).
They pin the checker; they need neither the library nor a GPU."""
import functools

import numpy as np
import pytest

import fb_dynamics as F
import fb_models as FM
import impedance_traj_cases as TC
import inverse_dynamics_reference as ID
from blf.closed_loop import fixed_step_schedule

CASES = ("h24", "h24p", "rand26-c8")


@functools.lru_cache(maxsize=None)
def case(cid):
    """(model, states, contacts) with two robots."""
    if cid in ("h24", "h24p"):
        cs = TC.build_case(cid)
    else:
        cs = FM.build_case(cid)
    st = {k: np.ascontiguousarray(cs["states"][k][:2]) for k in ID.STATE_KEYS}
    ct = cs["contacts"]
    ct = dict(ct, null_pose=ct["null_pose"][:2], wrench=None if ct["wrench"] is None else ct["wrench"][:2])
    return cs["model"], st, ct


def weight(model):
    return float(np.sum(model["link_mass"])) * 9.81


@pytest.mark.parametrize("cid", CASES)
def test_round_trip_through_forward_dynamics(cid):
    """F.dynamics at the inverse-dynamics torque returns the requested joint accelerations and the same base
    acceleration, within 1e-10 relative."""
    model, st, ct = case(cid)
    rng = np.random.default_rng(4)
    for i in range(2):
        sdd = rng.normal(size=model["n"]) * 3.0
        ab, tau = ID.inverse_dynamics(model, st, i, joint_acc=sdd, **FM.oracle_kw(ct, i))
        one = dict(st, joint_torque=np.repeat(tau[None], 2, axis=0))
        ba, ja, _, _, _ = F.dynamics(model, one, i, **FM.oracle_kw(ct, i))
        assert FM.rel_err(ja, sdd) <= 1e-10
        assert FM.rel_err(ba, ab) <= 1e-10


@pytest.mark.parametrize("cid", CASES)
def test_given_base_mode_at_the_free_base_solution(cid):
    """The given-base mode at the free-base mode's base acceleration: the same torques and a base wrench
    below 1e-10 m g."""
    model, st, ct = case(cid)
    sdd = np.random.default_rng(5).normal(size=model["n"])
    for i in range(2):
        ab, tau = ID.inverse_dynamics(model, st, i, joint_acc=sdd, **FM.oracle_kw(ct, i))
        wr, tau2 = ID.inverse_dynamics(model, st, i, joint_acc=sdd, base_acc=ab, **FM.oracle_kw(ct, i))
        assert np.abs(wr).max() <= 1e-10 * weight(model)
        assert FM.rel_err(tau2, tau) <= 1e-10


def potential(model, st, i):
    """U = -sum_l m_l g . c_l, the gravitational potential energy."""
    K = F.kinematics(model, st["base_pos"][i], st["base_rot"][i], st["joint_pos"][i], np.zeros(6),
                     np.zeros(model["n"]))
    return -sum(model["link_mass"][l] * F.G @ (K["p"][l] + K["R"][l] @ model["link_com"][l])
                for l in range(model["n"] + 1))


@pytest.mark.parametrize("cid", CASES)
def test_gravity_torques_are_the_potential_gradient(cid):
    """Given-base mode at nu = 0, nu_dot = 0, no contacts: the joint torques hold the robot against gravity,
    tau = dU/dq = -(the generalized force of gravity, -dU/dq), by central differences; the base force is the
    weight."""
    model, st, _ = case(cid)
    rest = dict(st, base_vel=np.zeros_like(st["base_vel"]), joint_vel=np.zeros_like(st["joint_vel"]))
    for i in range(2):
        wr, tau = ID.inverse_dynamics(model, rest, i, base_acc=np.zeros(6))
        np.testing.assert_allclose(wr[:3], [0.0, 0.0, weight(model)], rtol=0, atol=1e-10 * weight(model))
        eps, grad = 1e-6, np.zeros(model["n"])
        for j in range(model["n"]):
            up, dn = {k: v.copy() for k, v in rest.items()}, {k: v.copy() for k, v in rest.items()}
            up["joint_pos"][i, j] += eps
            dn["joint_pos"][i, j] -= eps
            grad[j] = (potential(model, up, i) - potential(model, dn, i)) / (2 * eps)
        assert np.abs(tau - grad).max() <= 1e-7 * max(1.0, np.abs(grad).max())
        assert np.abs(grad).max() > 1e-2


@pytest.mark.parametrize("cid", ("h24", "h24p"))
def test_unclamped_trajectory_call_follows_the_joint_recurrence(cid):
    """euler_integrate_computed_torque_traj without tau_max: joint_pos / joint_vel equal joint_recurrence,
    which knows nothing of the dynamics, within 1e-12 (T = 4 slices over the closed loop's 19 steps)."""
    model, st, ct = case(cid)
    r = TC.references(cid, 2, 4)
    n = model["n"]
    qdd = np.random.default_rng(6).uniform(-1.0, 1.0, (4, 2, n))
    sched = fixed_step_schedule(TC.T0, TC.T1, TC.DT)
    assert len(sched) == TC.NSTEPS
    for i in range(2):
        s, tau, clamped = ID.euler_integrate_computed_torque_traj(
            model, st, i, r["q_ref"][:, i], 400.0, 40.0, 5, TC.T0, TC.T1, TC.DT, qd_ref=r["nu"][:, i, 6:],
            qdd_ref=qdd[:, i], q_bias=r["q_bias"][i], **FM.oracle_kw(ct, i))
        q, qd = ID.joint_recurrence(st["joint_pos"][i], st["joint_vel"][i],
                                    dict(q_ref=r["q_ref"][:, i], qd_ref=r["nu"][:, i, 6:], qdd_ref=qdd[:, i],
                                         q_bias=r["q_bias"][i]), 400.0, 40.0, sched, 5)
        assert not clamped and np.isfinite(tau).all()
        assert FM.rel_err(s["joint_pos"], q) <= 1e-12
        assert FM.rel_err(s["joint_vel"], qd) <= 1e-12
        assert np.abs(s["joint_pos"] - st["joint_pos"][i]).max() > 1e-5
