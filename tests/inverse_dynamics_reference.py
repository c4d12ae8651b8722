"""TEST INFRASTRUCTURE ONLY -- numpy restatements of include/blf/blf_c.h section 8b
(blf_fb_inverse_dynamics), of section 9's computed-torque trajectory call
(blf_fbd_euler_integrate_computed_torque_traj) and of the closed loop's computed-torque period
(blf.closed_loop.ClosedLoop(reference="ik", control="computed_torque")), the checkers of the three.

The inverse dynamics goes through the dense M and h of oracle/fb_dynamics.py (mass_and_bias) and the
contact terms as fb_dynamics.dynamics forms them: no sweep over the tree, so it shares nothing with the
kernel's algorithm.  Plain helper module."""
import numpy as np

import closed_loop_ik_reference as IR
import fb_dynamics as F
import oracle as O
from blf.closed_loop import fixed_step_schedule

STATE_KEYS = ("base_vel", "joint_vel", "base_pos", "base_rot", "joint_pos")


def system_terms(model, state, i, contacts=(), contact_params=None, null_poses=None, laws=None, wrenches=None,
                 gravity=F.G):
    """(M, h, sum_c J_c^T w_c) of system i of a state batch, the contacts as F.dynamics takes them."""
    s = {k: v[i] for k, v in state.items()}
    K = F.kinematics(model, s["base_pos"], s["base_rot"], s["joint_pos"], s["base_vel"], s["joint_vel"])
    M, h = F.mass_and_bias(model, K, gravity)
    jw = np.zeros_like(h)
    for c, f in enumerate(contacts):
        pf, Rf, vel, J = F.frame_state(model, K, f)
        if laws is not None and laws[c] == F.CONTACT_WRENCH:
            w = np.asarray(wrenches[c], dtype=np.float64)
        else:
            w = O.contact_eval(contact_params[c], vel, np.concatenate([pf, Rf.reshape(-1)]), null_poses[c])[0]
        jw = jw + J.T @ w
    return M, h, jw


def inverse_dynamics(model, state, i, joint_acc=None, base_acc=None, **kw):
    """blf_fb_inverse_dynamics of system i.  base_acc None (free base): returns (base_acc [6], tau [n]), the
    unique pair with M [base_acc; sdd] + h = sum_c J_c^T w_c + [0; tau].  base_acc given: returns
    (base_wrench [6], tau [n]) = M [base_acc; sdd] + h - sum_c J_c^T w_c."""
    M, h, jw = system_terms(model, state, i, **kw)
    n = model["n"]
    sdd = np.zeros(n) if joint_acc is None else np.asarray(joint_acc, dtype=np.float64)
    if base_acc is None:
        ab = np.linalg.solve(M[:6, :6], jw[:6] - h[:6] - M[:6, 6:] @ sdd)
        tau = M[6:, :6] @ ab + M[6:, 6:] @ sdd + h[6:] - jw[6:]
        return ab, tau
    r = M @ np.concatenate([np.asarray(base_acc, dtype=np.float64), sdd]) + h - jw
    return r[:6], r[6:]


def commanded_acc(q, qd, q_ref, kp, kd, qd_ref=None, qdd_ref=None, q_bias=None):
    """sdd = qdd_ref + kp (q_ref + q_bias - q) + kd (qd_ref - qdot); absent terms are zero."""
    r = q_ref if q_bias is None else q_ref + q_bias
    a = kp * (r - q) + kd * ((0.0 if qd_ref is None else qd_ref) - qd)
    return a if qdd_ref is None else qdd_ref + a


def euler_integrate_computed_torque_traj(model, st, i, q_ref, kp, kd, steps_per_slice, t0, t1, dT, qd_ref=None,
                                         qdd_ref=None, q_bias=None, tau_max=None, **kw):
    """blf_fbd_euler_integrate_computed_torque_traj of system i: q_ref [T,n] (robot i's slices), qd_ref,
    qdd_ref [T,n] or None, q_bias [n] or None, tau_max [n] or None.  Returns (final state, the last step's
    applied torque, whether any step's torque was clamped)."""
    s = {k: np.array(v[i], dtype=np.float64) for k, v in st.items() if k != "joint_torque"}
    T = q_ref.shape[0]
    tau, clamped = None, False
    for k, h in enumerate(fixed_step_schedule(t0, t1, dT)):
        sl = IR.slice_of(k, steps_per_slice, T)
        sdd = commanded_acc(s["joint_pos"], s["joint_vel"], q_ref[sl], kp, kd,
                            None if qd_ref is None else qd_ref[sl], None if qdd_ref is None else qdd_ref[sl], q_bias)
        one = {k2: v[None] for k2, v in s.items()}
        _, tau = inverse_dynamics(model, one, 0, joint_acc=sdd, **kw)
        if tau_max is not None:
            clamped = clamped or bool((np.abs(tau) > tau_max).any())
            tau = np.minimum(np.maximum(tau, -tau_max), tau_max)
        one["joint_torque"] = tau[None]
        ba, ja, dp, dR, dq = F.dynamics(model, one, 0, **kw)
        s["base_pos"] = s["base_pos"] + dp * h
        s["base_rot"] = s["base_rot"] + dR * h
        s["joint_pos"] = s["joint_pos"] + dq * h
        s["base_vel"] = s["base_vel"] + ba * h
        s["joint_vel"] = s["joint_vel"] + ja * h
    return s, tau, clamped


def joint_recurrence(q, qd, refs, kp, kd, schedule, sps):
    """The per-joint scalar recurrence of the unclamped computed-torque call, no dynamics involved:
    q, qd [..., n] the start values; refs = dict(q_ref [T, ..., n], qd_ref, qdd_ref [T, ..., n] or None,
    q_bias [..., n] or None); schedule the step lengths.  Per step h with slice s = min(k // sps, T - 1):
    sdd = commanded_acc(...), q += h qd, qd += h sdd (both from the step's start values)."""
    q, qd = np.array(q, dtype=np.float64), np.array(qd, dtype=np.float64)
    T = refs["q_ref"].shape[0]
    pick = lambda key, sl: None if refs.get(key) is None else refs[key][sl]
    for k, h in enumerate(schedule):
        sl = IR.slice_of(k, sps, T)
        sdd = commanded_acc(q, qd, refs["q_ref"][sl], kp, kd, pick("qd_ref", sl), pick("qdd_ref", sl),
                            refs.get("q_bias"))
        q, qd = q + qd * h, qd + sdd * h
    return q, qd


class ComputedTorqueOracleLoop(IR.IkOracleLoop):
    """blf.closed_loop.ClosedLoop(reference="ik", control="computed_torque") restated on the CPU: the IK
    period of IkOracleLoop with its dynamics step replaced by euler_integrate_computed_torque_traj (scalar
    gains kp = freq^2, kd = 2 zeta freq; lean off by default)."""

    def __init__(self, *a, freq=20.0, zeta=1.0, tau_max=None, lean=False, **kw):
        super().__init__(*a, lean=lean, **kw)
        self.ct_kp, self.ct_kd, self.tau_max = freq * freq, 2.0 * zeta * freq, tau_max
        self.tau_last = None

    def _integrate(self, model, st, i, q_ref, kp, kd, sps, t0, t1, dT, qd_ref=None, q_bias=None, **kw):
        # IkOracleLoop.period's dynamics call, its impedance gains ignored
        s, tau, _ = euler_integrate_computed_torque_traj(model, st, i, q_ref, self.ct_kp, self.ct_kd, sps, t0, t1,
                                                         dT, qd_ref=qd_ref, q_bias=q_bias, tau_max=self.tau_max, **kw)
        self.tau_last[i] = tau
        return s

    def period(self):
        # the parent's period with the integration of each robot routed through _integrate: it looks the
        # trajectory impedance up in its module at call time
        self.tau_last = np.zeros((self.omega.shape[0], self.model["n"]))
        keep = IR.euler_integrate_impedance_traj
        IR.euler_integrate_impedance_traj = self._integrate
        try:
            return super().period()
        finally:
            IR.euler_integrate_impedance_traj = keep
