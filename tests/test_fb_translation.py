"""The references of the floating-base, inverse-kinematics and DCM-MPC tests are insensitive to a
translation of the world frame: the condition tests/test_gpu_fb_translation.py rests on, where the
kernels run on inputs shifted by fb_models.shift_vec(k) = (2^k, -2^k, 2^(k-1)) m and are compared
with the references on the unshifted inputs.  CPU only.

The positions (base_pos, the contacts' null poses, the IK set points) are first rounded to
multiples of 2^-20 m, so the shift is exact (asserted) and the shifted problem is the same physical
problem bit for bit; what differs is the rounding of the arithmetic alone.  The references take
point Jacobians z x (x - o), which lose accuracy linearly with the distance (2^k ulp), not with its
square as spatial quantities about the world origin do.

Bar: fb_models.rel_err < 2e-10 of the shifted reference against the unshifted one, five times under
the kernels' 1e-9; base_pos, which carries the shift, as |(got - d) - ref| < steps 2^(k-51) + 1e-9
(one rounding of a coordinate of size <= 2^(k+1) per step and per side).  Worst measured at k = 3, 7,
10, 13: accelerations 2.8e-11, 4.3e-11, 4.4e-11, 5.0e-11 (chain48-c2 at every shift: its own floor;
the Euler states below 1.5e-11), the humanoid 1.9e-14, 1.9e-13, 1.2e-12, 1.1e-11 (linear in the
distance); IK nu 4.6e-12, 4.6e-12, 8.4e-12, 3.5e-11 and states 8.9e-12 to 4.0e-11; the C restatement with
the joint impedance (20 steps, the dynamics tests' soles) 2.7e-14, 7.7e-13, 6.2e-12, 2.8e-11; the QP
oracle against the dense certificate 3.2e-12 at 2^10, 2.9e-11 at 2^13."""
import numpy as np
import pytest

import dense_qp
import fb_models as FM
import ik_cases as IC
import ik_reference as IK
import oracle as O
from blf import problems as P

BAR = 2e-10
STATE_KEYS = ("base_pos", "base_rot", "joint_pos", "base_vel", "joint_vel")
rel_err = FM.rel_err

# the oracle runs the same arithmetic for mass_reg = zeros and for none
ORACLE_RUNS = sorted({(c, "reg" if kind == "reg" else "none") for c, kind in FM.TRANSLATION_RUNS})


@pytest.mark.parametrize("k", FM.SHIFTS)
def test_shift_helpers_are_exact(k):
    cs = FM.translation_case("rand26-c8")
    (g_st, g_ct), (s_st, s_ct) = FM.shift_case(cs["states"], cs["contacts"], k)
    d = FM.shift_vec(k)
    np.testing.assert_array_equal(d, [2.0 ** k, -2.0 ** k, 2.0 ** (k - 1)])
    np.testing.assert_array_equal(s_st["base_pos"] - d, g_st["base_pos"])
    np.testing.assert_array_equal(s_ct["null_pose"][..., :3] - d, g_ct["null_pose"][..., :3])
    np.testing.assert_array_equal(s_ct["null_pose"][..., 3:], cs["contacts"]["null_pose"][..., 3:])
    np.testing.assert_array_equal(g_st["base_pos"] * 2.0 ** 20, np.round(g_st["base_pos"] * 2.0 ** 20))
    assert np.abs(g_st["base_pos"] - cs["states"]["base_pos"]).max() <= 2.0 ** -21
    for key in cs["states"]:
        if key != "base_pos":
            assert s_st[key] is cs["states"][key]
    ik = IC.build_case("rand24-k2com")
    (_, g_tk), (_, s_tk) = FM.shift_ik(ik["states"], ik["tasks"], k)
    np.testing.assert_array_equal(s_tk["se3_pose"][..., :3] - d, g_tk["se3_pose"][..., :3])
    np.testing.assert_array_equal(s_tk["com_pos"] - d, g_tk["com_pos"])
    with pytest.raises(AssertionError):   # an inexact shift is refused
        FM._shifted(np.array([[0.1, 0.2, 0.3]]), FM.shift_vec(13))


@pytest.mark.parametrize("k", FM.SHIFTS)
@pytest.mark.parametrize("cid,kind", ORACLE_RUNS, ids=[f"{c}-{s}" for c, s in ORACLE_RUNS])
def test_oracle_dynamics_and_euler_do_not_see_the_shift(cid, kind, k):
    cs = FM.translation_case(cid)
    _, (st, ct) = FM.shift_case(cs["states"], cs["contacts"], k)
    dyn, eul = FM.oracle_run(cs["model"], cs["B"], st, ct, kind)
    dyn0, eul0 = FM.translation_reference(cid, kind)
    worst_a = worst_e = worst_p = 0.0
    for i in range(cs["B"]):
        worst_a = max(worst_a, rel_err(dyn[i][0], dyn0[i][0]), rel_err(dyn[i][1], dyn0[i][1]))
        e, p = FM.state_errors(eul[i], eul0[i], k, STATE_KEYS)
        worst_e, worst_p = max(worst_e, e), max(worst_p, p)
    print(f"{cid} [{kind}] 2^{k}: acceleration {worst_a:.2e}, Euler state {worst_e:.2e}, base_pos {worst_p:.2e}")
    assert worst_a < BAR and worst_e < BAR
    assert worst_p < FM.base_pos_allowance(k, FM.EULER_STEPS)


@pytest.mark.parametrize("k", FM.SHIFTS)
@pytest.mark.parametrize("cid", FM.TRANSLATION_IK_CASES)
def test_ik_reference_does_not_see_the_shift(cid, k):
    cs = IC.build_case(cid)
    _, (st, tk) = FM.shift_ik(cs["states"], cs["tasks"], k)
    sol0, int0 = IC.translation_reference(cid)
    worst_n = worst_e = worst_p = 0.0
    for i in range(min(cs["B"], 3)):
        nu, status, _, _ = IK.solve(cs["model"], st, tk, i)
        assert status == sol0[i][1] == IK.OK
        worst_n = max(worst_n, rel_err(nu, sol0[i][0]))
        got, _, status = IK.integrate(cs["model"], st, tk, i, FM.IK_STEPS, FM.IK_DT)
        assert status == IK.OK
        e, p = FM.state_errors(got, int0[i][0], k, STATE_KEYS)
        worst_e, worst_p = max(worst_e, e), max(worst_p, p)
    print(f"{cid} 2^{k}: nu {worst_n:.2e}, state {worst_e:.2e}, base_pos {worst_p:.2e}")
    assert worst_n < BAR and worst_e < BAR
    assert worst_p < FM.base_pos_allowance(k, FM.IK_STEPS)


# With the closed loop's own soles (fb_models.impedance_case(stiff=True), k = 2e6 N/m^3: the arguments of
# the GPU test) the references themselves move with the shift: 1.4e-12, 3.5e-11, 1.0e-10 and 1.6e-9 at
# 2^3, 2^7, 2^10 and 2^13 m (the C restatement; the numpy one 8e-10 at 2^13), all of it joint velocity of
# the light foot links, on which the stiff springs act.  The bar is held on the softer soles of the
# dynamics tests.
@pytest.fixture(scope="module")
def impedance_unshifted():
    cs = FM.impedance_case(stiff=False)
    (st, ct), _ = FM.shift_case(cs["states"], cs["contacts"], 0)
    return O.fbd_euler_impedance_batch(cs["model"], st, cs["q_ref"], cs["kp"], cs["kd"], ct["params"],
                                       ct["null_pose"], cs["t0"], cs["t1"], cs["dT"])


@pytest.mark.parametrize("k", FM.SHIFTS)
def test_c_restatement_with_impedance_does_not_see_the_shift(impedance_unshifted, k):
    cs = FM.impedance_case(stiff=False)
    _, (st, ct) = FM.shift_case(cs["states"], cs["contacts"], k)
    got = O.fbd_euler_impedance_batch(cs["model"], st, cs["q_ref"], cs["kp"], cs["kd"], ct["params"],
                                      ct["null_pose"], cs["t0"], cs["t1"], cs["dT"])
    worst_e = worst_p = 0.0
    for i in range(cs["B"]):
        e, p = FM.state_errors({key: got[key][i] for key in STATE_KEYS},
                               {key: impedance_unshifted[key][i] for key in STATE_KEYS}, k, STATE_KEYS)
        worst_e, worst_p = max(worst_e, e), max(worst_p, p)
    print(f"impedance 2^{k}: state {worst_e:.2e}, base_pos {worst_p:.2e}")
    assert worst_e < BAR
    assert worst_p < FM.base_pos_allowance(k, cs["steps"])


@pytest.mark.parametrize("k", FM.QP_SHIFTS)
def test_qp_oracle_on_a_shifted_plan_is_the_dense_optimum(k):
    """The oracle's cold solve of a whole plan shifted by (2^k, -2^(k-1)): every status 0, every
    solve polished, and the solution within 1e-9 of the dense KKT certificate."""
    B = 64
    g, s = FM.shift_plan(P.make_batch(B, horizon=100, n_footsteps=6, seed=77), k)
    d = np.array([2.0 ** k, -(2.0 ** (k - 1))])
    for key in FM.QP_KEYS:
        np.testing.assert_array_equal(s[key] - d, g[key])
    host = O.assemble_constraints(s)
    pol = np.zeros(B, np.int32)
    st, xi, vrp, it, _ = O.dcm_mpc_solve_batch_warm(host, threads=8, polished=pol)
    assert (st == 0).all() and pol.all()
    worst = 0.0
    for i in range(0, B, 4):
        # a . r - b with |a| <= 1 and |r|, |b| <= 2^(k+1) rounds four times at 2^(k-52)
        xd, rd = dense_qp.certify(host, i, xi[i], vrp[i], feas=1e-12 + 8 * 2.0 ** (k - 52))
        worst = max(worst, np.abs(xd - xi[i]).max(), np.abs(rd - vrp[i]).max())
    print(f"QP oracle at 2^{k}: {worst:.2e} from the dense certificate, iterations {it.min()} - {it.max()}")
    assert worst < 1e-9
