"""TEST INFRASTRUCTURE ONLY -- numpy restatements of include/blf/blf_c.h section 9b (blf_dcm_com_reference),
of section 9's trajectory impedance (blf_fbd_euler_integrate_impedance_traj) and of the closed loop's IK
period (blf.closed_loop.ClosedLoop(reference="ik")), the checkers of the three.

The trajectory impedance steps over blf.closed_loop.fixed_step_schedule with the CPU dynamics
oracle/closed_loop.py uses (fb_dynamics.dynamics); IkOracleLoop is built from oracle/closed_loop.py's
pieces (the state -> plan map, the phase table, the warm solve, the posture map) and
tests/ik_track_reference.py's track().  Plain helper module."""
import math

import numpy as np

import closed_loop as CL
import fb_dynamics as F
import ik_limits_reference as LR
import ik_track_reference as TR
import oracle as O
from blf import robot as R
from blf.closed_loop import fixed_step_schedule


def com_reference(xi0, r0, omega0, z_ref, c_ref, T, dT):
    """Section 9b in its order, for B robots: xi0, r0, c_ref [B,2], omega0, z_ref [B].  Returns com_pos,
    com_vel [B,T,3], c_T [B,2], xi_T [B,2]; a robot with a non-finite input has NaN everywhere."""
    xi0, r0, c_ref = (np.asarray(a, dtype=np.float64) for a in (xi0, r0, c_ref))
    w, z = np.asarray(omega0, dtype=np.float64), np.asarray(z_ref, dtype=np.float64)
    B = xi0.shape[0]
    ok = (np.isfinite(xi0).all(1) & np.isfinite(r0).all(1) & np.isfinite(c_ref).all(1) & np.isfinite(w)
          & np.isfinite(z))
    pos, vel = np.empty((B, T, 3)), np.empty((B, T, 3))
    with np.errstate(all="ignore"):
        nwr = -w[:, None] * r0
        xi, c = xi0.copy(), c_ref.copy()
        for t in range(T):
            v = w[:, None] * (xi - c)
            pos[:, t, :2], pos[:, t, 2] = c, z
            vel[:, t, :2], vel[:, t, 2] = v, 0.0
            c = c + v * dT
            xi = xi + ((w[:, None] * xi) + nwr) * dT
    for a in (pos, vel, c, xi):
        a[~ok] = np.nan
    return pos, vel, c, xi


def com_closed_form(xi0, r0, omega, c0, t):
    """c(t) of cdot = omega (xi - c), xidot = omega (xi - r0):
    r0 + (xi0 - r0) e^{wt} / 2 + (c0 - r0 - (xi0 - r0) / 2) e^{-wt}."""
    a = 0.5 * (xi0 - r0)
    return r0 + a * math.exp(omega * t) + (c0 - r0 - a) * math.exp(-omega * t)


def slice_of(i, steps_per_slice, T):
    return min(i // steps_per_slice, T - 1)


def euler_integrate_impedance_traj(model, st, i, q_ref, kp, kd, steps_per_slice, t0, t1, dT, qd_ref=None,
                                   q_bias=None, **kw):
    """blf_fbd_euler_integrate_impedance_traj of system i: q_ref [T,n] (robot i's slices), qd_ref [T,n] or
    None, q_bias [n] or None.  Step k of fixed_step_schedule(t0, t1, dT) tracks slice
    min(k // steps_per_slice, T - 1): r = q_ref (+ q_bias), tau = kp (r - q) - kd (qdot - qd_ref)
    (qd_ref None: - kd qdot, oracle/closed_loop.py's expression)."""
    s = {k: np.array(v[i], dtype=np.float64) for k, v in st.items() if k != "joint_torque"}
    T = q_ref.shape[0]
    for k, h in enumerate(fixed_step_schedule(t0, t1, dT)):
        sl = slice_of(k, steps_per_slice, T)
        r = q_ref[sl] if q_bias is None else q_ref[sl] + q_bias
        if qd_ref is None:
            tau = kp * (r - s["joint_pos"]) - kd * s["joint_vel"]
        else:
            tau = kp * (r - s["joint_pos"]) - kd * (s["joint_vel"] - qd_ref[sl])
        one = {k2: v[None] for k2, v in s.items()}
        one["joint_torque"] = tau[None]
        ba, ja, dp, dR, dq = F.dynamics(model, one, 0, **kw)
        s["base_pos"] = s["base_pos"] + dp * h
        s["base_rot"] = s["base_rot"] + dR * h
        s["joint_pos"] = s["joint_pos"] + dq * h
        s["base_vel"] = s["base_vel"] + ba * h
        s["joint_vel"] = s["joint_vel"] + ja * h
    return s


def hard_rows(hard):
    """robot.standing_ik_hard's dict as section 12b's row mask (native.Handle.ik_hard's layout)."""
    rows = 0
    for k, r in enumerate(hard["se3"]):
        for a, on in enumerate(r):
            rows |= int(bool(on)) << (6 * k + a)
    for a, on in enumerate(hard["com"]):
        rows |= int(bool(on)) << (24 + a)
    return rows


class IkOracleLoop:
    """blf.closed_loop.ClosedLoop(reference="ik") restated on the CPU (same inputs, same sequence)."""

    def __init__(self, model, plan, states, null_pose, law, contact_params, horizon=100, dT=0.001,
                 tol_polish=1e-4, threads=8, tasks=None, hard=None, limits=None, steps=4, lean=True):
        self.model, self.N, self.dT = model, horizon, dT
        self.dt = float(plan["dt"])
        self.T = self.dt - dT
        self.law = law
        self.state = {k: np.array(states[k], dtype=np.float64) for k in TR.IK.STATE_KEYS + ("base_vel", "joint_vel")}
        self.null = null_pose
        C = len(model["frame_link"])
        self.cparams = np.tile(np.asarray(contact_params, np.float64), (C, 1))
        self.table = CL.phase_table(plan)
        self.omega = plan["omega"]
        self.params = O.default_params(horizon, tol_polish=tol_polish, max_iter=100)
        self.threads = threads
        self.prev, self.s = None, 0
        self.tasks = tasks if tasks is not None else R.standing_ik_tasks(model, states)
        self.rows = hard_rows(hard if hard is not None else R.standing_ik_hard(model))
        self.ik_steps = int(steps)
        self.ik_dT = self.dt / self.ik_steps
        lim = limits if limits is not None else R.humanoid24_joint_limits(model, sampling_time=self.ik_dT)
        self.limits = dict(lim, max_iter=lim.get("max_iter", 0))
        self.lean = lean
        self.kin = {k: np.array(states[k], dtype=np.float64) for k in TR.IK.STATE_KEYS}
        B = self.omega.shape[0]
        self.sole = np.repeat(np.asarray(self.tasks["se3_pose"], dtype=np.float64)[:, :, None, :], self.ik_steps, axis=2)
        self.contact = np.ones((B, self.sole.shape[1], self.ik_steps), dtype=np.int32)
        self.z_ref = np.asarray(self.tasks["com_pos"], dtype=np.float64)[:, 2].copy()
        self.c_ref = None
        self.nsteps = len(fixed_step_schedule(0.0, self.T, dT))
        self.sps = -(-self.nsteps // self.ik_steps)
        self.lean_law = dict(q_nominal=np.zeros(model["n"]), lean=law["lean"])

    def period(self):
        s, N, B = self.s, self.N, self.omega.shape[0]
        omega = np.ascontiguousarray(self.omega[:, s:s + N])
        com, xi = CL.dcm_from_state(self.model, self.state, omega[:, 0])
        w = O.dcm_phase_expand(self.table, s, self.dt, N)
        w.update(xi_init=xi, omega=omega)
        pv, pl, ps = ((None, None, None) if self.prev is None else
                      (self.prev["vrp"], self.prev["lam"], self.prev["status"]))
        if ps is not None:   # blf/closed_loop.py: cold after a handover
            ps = (ps | (self.prev["iters"] > 0)).astype(np.int32)
        pol = np.zeros(B, np.int32)
        st, xo, vrp, it, lam = O.dcm_mpc_solve_batch_warm(w, vrp_ws=pv, lam_ws=pl, shift=1, floor=1e-3,
                                                          params=self.params, threads=self.threads,
                                                          polished=pol, prev_status=ps)
        if self.c_ref is None:
            self.c_ref = com[:, :2].copy()
        pos, vel, self.c_ref, _ = com_reference(xi, vrp[:, 0], omega[:, 0], self.z_ref, self.c_ref,
                                                self.ik_steps, self.ik_dT)
        sch = dict(steps=self.ik_steps, stance_rows=0, contact=self.contact, se3_pose=self.sole, se3_twist=None,
                   com_pos=pos, com_vel=vel)
        tr = [TR.track(self.model, self.kin, self.tasks, self.rows, self.limits, sch, i, self.ik_dT)
              for i in range(B)]
        for i, r in enumerate(tr):
            for k in self.kin:
                self.kin[k][i] = r["state"][k]
        q_bias = CL.posture_reference(self.lean_law, com, vrp) if self.lean else None
        C = len(self.model["frame_link"])
        for i in range(B):
            si = euler_integrate_impedance_traj(
                self.model, self.state, i, tr[i]["joint_traj"], self.law["kp"], self.law["kd"], self.sps, 0.0,
                self.T, self.dT, qd_ref=tr[i]["nu_traj"][:, 6:], q_bias=None if q_bias is None else q_bias[i],
                contacts=list(range(C)), contact_params=self.cparams, null_poses=self.null[i])
            for k in self.state:
                self.state[k][i] = si[k]
        self.prev = dict(vrp=vrp, lam=lam, status=st, iters=it)
        self.s = s + 1
        return dict(status=st, xi=xo, vrp=vrp, iters=it, com=com, xi_init=xi, com_pos=pos, com_vel=vel,
                    track=tr, q_bias=q_bias, c_ref=self.c_ref.copy())
