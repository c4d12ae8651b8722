"""The cases of tests/test_gpu_impedance_traj.py (blf_fbd_euler_integrate_impedance_traj against
tests/closed_loop_ik_reference.py).  Plain helper module.

A case: dict(model, states (host, B rows), contacts (fb_models.contact_set's host dict), kp, kd).
  h24    humanoid24 on its soles (two robots per wavefront), the posture law's gains: the arguments of
         test_fbd_euler_impedance_vs_oracle, up to three robots (the odd batch and the pair)
  h24p   the same with four prismatic joints (robot.with_joint_types)
  n48    fb_models' bfs48-c8 (n = 48, one robot per wavefront, eight contacts), kp = 400 I_j,
         kd = 40 I_j with I_j the joint's composite inertia floored at 1e-3 (20 rad/s, critically
         damped: 19 explicit Euler steps of 1 ms stay bounded on the reference)
Every run integrates 0 -> 0.019 s at dT = 1 ms: 19 steps, the last one of the stale schedule."""
import functools

import numpy as np

import closed_loop_ik_reference as IR
import fb_models as FM
from blf import closed_loop as DL
from blf import robot

T0, T1, DT, NSTEPS = 0.0, 0.019, 0.001, 19
PRISMATIC = ("neck_pitch", "torso_roll", "l_knee", "r_hip_pitch")
STATE_KEYS = ("base_vel", "joint_vel", "base_pos", "base_rot", "joint_pos")


@functools.lru_cache(maxsize=None)
def build_case(cid):
    if cid in ("h24", "h24p"):
        model = robot.humanoid24()
        law = robot.posture_law_arrays(model)
        if cid == "h24p":
            model = robot.with_joint_types(model, prismatic=PRISMATIC)
        st = robot.standing_states(model, 3, seed=5)
        ct = dict(frame=np.arange(2, dtype=np.int32), params=np.tile(np.asarray(DL.CONTACT_PARAMS), (2, 1)),
                  null_pose=robot.sole_null_poses(model, st), law=None, wrench=None)
        return dict(model=model, states=st, contacts=ct, kp=law["kp"], kd=law["kd"])
    if cid == "n48":
        cs = FM.build_case("bfs48-c8")
        model, B = cs["model"], 2
        I = np.maximum(robot.joint_inertias(model), 1.0e-3)
        st = {k: np.ascontiguousarray(cs["states"][k][:B]) for k in STATE_KEYS}
        ct = dict(cs["contacts"], null_pose=np.ascontiguousarray(cs["contacts"]["null_pose"][:B]))
        return dict(model=model, states=st, contacts=ct, kp=400.0 * I, kd=40.0 * I)
    raise KeyError(cid)


@functools.lru_cache(maxsize=None)
def references(cid, B, T, seed=1):
    """Distinct random slices around the start posture for robots 0 .. B - 1: q_ref [T,B,n] within 0.02 rad,
    nu [T,B,6+n] (a nu_traj-shaped buffer: the joint velocities at columns 6 ..) within 0.1, q_bias [B,n]
    within 0.01."""
    cs = build_case(cid)
    n = cs["model"]["n"]
    rng = np.random.default_rng(seed)
    return dict(q_ref=cs["states"]["joint_pos"][None, :B] + rng.uniform(-0.02, 0.02, (T, B, n)),
                nu=rng.uniform(-0.1, 0.1, (T, B, 6 + n)), q_bias=rng.uniform(-0.01, 0.01, (B, n)))


@functools.lru_cache(maxsize=None)
def reference(cid, B, T, sps, full=True):
    """IR.euler_integrate_impedance_traj of robots 0 .. B - 1 of the case over references(cid, B, T), with
    qd_ref and q_bias (full) or without; computed once and shared."""
    cs, r = build_case(cid), references(cid, B, T)
    out = []
    for i in range(B):
        out.append(IR.euler_integrate_impedance_traj(
            cs["model"], cs["states"], i, r["q_ref"][:, i], cs["kp"], cs["kd"], sps, T0, T1, DT,
            qd_ref=r["nu"][:, i, 6:] if full else None, q_bias=r["q_bias"][i] if full else None,
            **FM.oracle_kw(cs["contacts"], i)))
    for s in out:
        assert all(np.isfinite(v).all() for v in s.values()), (cid, "the reference diverged")
    return out
