"""The floating-base, inverse-kinematics and DCM-MPC kernels far from the world origin.  Every other
GPU test places its robots within a centimetre of the origin (robot.random_states /
standing_states); here the device runs on inputs shifted by fb_models.shift_vec(k) = (2^k, -2^k,
2^(k-1)) m, k in fb_models.SHIFTS (8 m, 128 m, 1 km, 8 km), and is compared with the references on the
UNSHIFTED inputs.  The shift is exact (positions on a 2^-20 m grid first), so the two are the same
physical problem bit for bit, and tests/test_fb_translation.py shows the references themselves move
by less than 2e-10 under it.

What is compared, at the existing bars (TOL = 1e-9 of tests/test_gpu_fb_dynamics.py and
tests/test_gpu_fb_topologies.py on fb_models.rel_err):
  * blf_fbd_dynamics and the three-step blf_fbd_euler_integrate on fb_models.TRANSLATION_RUNS (both
    solve paths, both wavefront layouts, DFS and level-by-level subtree sums, given wrenches,
    prismatic joints, n = 1): accelerations, the kinematic derivatives as check_against_oracle has
    them, every state key after the integration; base_pos shifted back, within
    steps 2^(k-51) + 1e-9 m; the sentinel row untouched;
  * blf_fbd_euler_integrate_impedance with the arguments of test_fbd_euler_impedance_vs_oracle (with
    these stiff soles the references, run on the shifted inputs, move by up to 1.6e-9 themselves at
    2^13 m, tests/test_fb_translation.py; the device is compared with the unshifted one);
  * blf_fb_frame_state and blf_fb_dcm on chain48 and bfs27: rotations, twists and the CoM velocity at
    the existing tests' 1e-12, positions and the DCM shifted back within 4 2^(k-52) + 1e-9 m;
  * blf_fb_ik_solve and three steps of blf_fb_ik_integrate on fb_models.TRANSLATION_IK_CASES: status
    OK, nu and the state keys at TOL against the unshifted tests/ik_reference.py;
  * blf_dcm_mpc_solve, cold, on a 64-plan batch shifted by (2^k, -2^(k-1)), k = 10 and 13, against the
    oracle on the same shifted problem bit for bit (status, xi, vrp, iters, passes), every status 0.

Measured on an MI355X (worst over the systems of the runs).  "before": the kernels of
csrc/fb_dynamics.hip with their spatial quantities about the world origin, as they stood when this
file was written; "now": about each system's own base position at kernel entry (that file's header).

  fbd_dynamics / fbd_euler_integrate, accelerations | Euler states, worst of the 23 runs (bar 1e-9)
    shift        before                 now
    2^3   m      6.6e-10 | 4.8e-10      4.9e-11 | 1.7e-11
    2^7   m      1.8e-07 | 9.8e-08      4.9e-11 | 1.7e-11
    2^10  m      1.8e-05 | 1.1e-05      4.9e-11 | 1.7e-11
    2^13  m      9.8e-04 | 4.8e-04      4.9e-11 | 1.7e-11
  Before, all 23 runs failed at 2^7, 2^10 and 2^13 (69 of 92 tests), worst on the DFS arm's prefix
  differences (rand48-c8mixed-dfs with mass_reg = zeros; the same physical tree with level sums
  2.4e-05 at 2^13); the humanoid 9.9e-12 / 3.3e-09 / 1.5e-07 / 2.5e-05 (articulated-body) and 4.5e-10 /
  4.2e-08 / 3.4e-06 / 3.0e-04 (mass_reg = zeros).  Now every run gives the same figure at every shift:
  chain48-c2 4.9e-11 (zeros) and 2.9e-11 (articulated-body), its floor near the origin too; every
  other tree at most 8.8e-13; the humanoid 1.8e-14 and 1.4e-13.  base_pos shifted back: 8e-16, 1e-14,
  1e-13, 9e-13 m (allowance 3 2^(k-51) + 1e-9).
  fbd_euler_integrate_impedance (20 steps): before 1.9e-12, 3.8e-10, 9.5e-09, 1.0e-06 (failed at 2^10
    and 2^13); now 4.1e-14 at every shift, base_pos within 8.4e-13 m at 2^13.
  fb_frame_state: rotation and twist before 6.0e-15, 4.3e-14, 6.6e-13, 6.8e-12 (failed its 1e-12 at
    2^13), now 1.4e-15 at every shift; positions shifted back 1.3e-15, 1.4e-14, 1.1e-13, 9.0e-13 m.
  fb_dcm: CoM velocity before 1.3e-15, 1.4e-14, 2.2e-13, 7.7e-13, now 4.8e-16 at every shift; CoM and DCM
    shifted back within 1.3e-12 m at 2^13 (before 3.3e-12).
  fb_ik_solve / fb_ik_integrate (unchanged kernels): nu 6.6e-12, 6.6e-12, 9.8e-12, 8.4e-11; states
    3.7e-11, 2.2e-11, 2.3e-11, 1.7e-10 (chain27 / chain48: linear in the distance, inside the bar).
  blf_dcm_mpc_solve (unchanged kernels): the oracle's bits at 2^10 and 2^13, every status 0, no interior
    point iteration, every solve polished, mean passes 4.98 and 5.64."""
import numpy as np
import pytest
import torch

import closed_loop as CL
import fb_dynamics as F
import fb_models as FM
import ik_cases as IC
import ik_reference as IK
from blf import native
from blf import problems as P
from gpu_util import dev_contacts, to_device as _d

pytestmark = pytest.mark.gpu
TOL = 1e-9
rel_err = FM.rel_err
RUN_IDS = [f"{c}-{s}" for c, s in FM.TRANSLATION_RUNS]


@pytest.mark.parametrize("k", FM.SHIFTS)
@pytest.mark.parametrize("cid,kind", FM.TRANSLATION_RUNS, ids=RUN_IDS)
def test_fbd_dynamics_and_euler_far_from_the_origin(handle, cid, kind, k):
    cs = FM.translation_case(cid)
    B, model = cs["B"], cs["model"]
    _, (st, ct) = FM.shift_case(cs["states"], cs["contacts"], k)
    dm = handle.fb_model(model)
    reg = FM.reg_of(model, kind)
    kw = dict(contacts=dev_contacts(ct, B), mass_reg=None if reg is None else _d(reg))
    full = {key: _d(st[key]) for key in native.FB_STATE_KEYS}
    view = {key: v[:B] for key, v in full.items()}
    tau = _d(st["joint_torque"][:B])
    acc = {key: v.cpu().numpy() for key, v in handle.fbd_dynamics(dm, view, tau, **kw).items()}
    for key in native.FB_STATE_KEYS:   # the dynamics reads the state only
        np.testing.assert_array_equal(full[key].cpu().numpy(), st[key], err_msg=key)
    handle.fbd_euler_integrate(dm, view, tau, FM.T0, FM.T1, FM.DT, **kw)
    torch.cuda.synchronize()
    for key in native.FB_STATE_KEYS:
        np.testing.assert_array_equal(full[key][B].cpu().numpy(), st[key][B], err_msg=f"sentinel row of {key}")
    got = {key: v.cpu().numpy() for key, v in view.items()}
    dyn, eul = FM.translation_reference(cid, kind)
    errs = [FM.state_errors({key: got[key][i] for key in got}, eul[i], k, native.FB_STATE_KEYS) for i in range(B)]
    worst_a = max(max(rel_err(acc["base_vel"][i], dyn[i][0]), rel_err(acc["joint_vel"][i], dyn[i][1]))
                  for i in range(B))
    print(f"{cid} [{kind}] 2^{k}: acceleration rel_err {worst_a:.2e}, Euler state rel_err "
          f"{max(e for e, _ in errs):.2e}, base_pos {max(p for _, p in errs):.2e} m")
    for i in range(B):
        ba, ja, dp, dR, dq = dyn[i]
        assert rel_err(acc["base_vel"][i], ba) < TOL, (cid, kind, k, i)
        assert rel_err(acc["joint_vel"][i], ja) < TOL, (cid, kind, k, i)
        np.testing.assert_array_equal(acc["base_pos"][i], dp)
        np.testing.assert_allclose(acc["base_rot"][i], dR, rtol=0, atol=1e-15)
        np.testing.assert_array_equal(acc["joint_pos"][i], dq)
        assert errs[i][0] < TOL, (cid, kind, k, i)
        assert errs[i][1] < FM.base_pos_allowance(k, FM.EULER_STEPS), (cid, kind, k, i)


@pytest.fixture(scope="module")
def impedance_reference():
    cs = FM.impedance_case()
    (st, ct), _ = FM.shift_case(cs["states"], cs["contacts"], 0)
    return [CL.euler_integrate_impedance(cs["model"], st, i, cs["q_ref"][i], cs["kp"], cs["kd"], cs["t0"],
                                         cs["t1"], cs["dT"], contacts=[0, 1], contact_params=ct["params"],
                                         null_poses=ct["null_pose"][i]) for i in range(cs["B"])]


@pytest.mark.parametrize("k", FM.SHIFTS)
def test_fbd_euler_impedance_far_from_the_origin(handle, impedance_reference, k):
    cs = FM.impedance_case()
    _, (st, ct) = FM.shift_case(cs["states"], cs["contacts"], k)
    dev = {key: _d(v) for key, v in st.items()}
    dm = handle.fb_model(cs["model"])
    imp = handle.joint_impedance(cs["kp"], cs["kd"])
    handle.fbd_euler_integrate_impedance(dm, dev, imp, _d(cs["q_ref"]), cs["t0"], cs["t1"], cs["dT"],
                                         contacts=dev_contacts(ct, cs["B"]))
    torch.cuda.synchronize()
    got = {key: dev[key].cpu().numpy() for key in native.FB_STATE_KEYS}
    errs = [FM.state_errors({key: got[key][i] for key in got}, impedance_reference[i], k, native.FB_STATE_KEYS)
            for i in range(cs["B"])]
    print(f"impedance 2^{k}: state rel_err {max(e for e, _ in errs):.2e}, base_pos {max(p for _, p in errs):.2e} m")
    for i in range(cs["B"]):
        assert errs[i][0] < TOL, (k, i)
        assert errs[i][1] < FM.base_pos_allowance(k, cs["steps"]), (k, i)


@pytest.mark.parametrize("k", FM.SHIFTS)
@pytest.mark.parametrize("cid", FM.TRANSLATION_KIN_CASES)
def test_fb_frame_state_far_from_the_origin(handle, cid, k):
    cs = FM.build_case(cid)
    B, model = cs["B"], cs["model"]
    (st0, _), (st, _) = FM.shift_case(cs["states"], None, k)
    d = FM.shift_vec(k)
    nf = len(model["frame_link"])
    frames = np.array([0, 1, 2, nf, 3], dtype=np.int32)
    pose, twist = handle.fb_frame_state(handle.fb_model(model), {key: _d(st[key][:B]) for key in native.FB_STATE_KEYS},
                                        _d(frames, torch.int32))
    pose, twist = pose.cpu().numpy(), twist.cpu().numpy()
    worst_p = worst_r = 0.0
    for i in range(B):
        K = F.kinematics(model, st0["base_pos"][i], st0["base_rot"][i], st0["joint_pos"][i],
                         st0["base_vel"][i], st0["joint_vel"][i])
        for c, f in enumerate(frames):
            if f >= nf:
                assert np.isnan(pose[i, c]).all() and np.isnan(twist[i, c]).all()
                continue
            pf, Rf, vel, _ = F.frame_state(model, K, f)
            ep = np.abs((pose[i, c, :3] - d) - pf).max()
            worst_p, worst_r = max(worst_p, ep), max(worst_r, np.abs(pose[i, c, 3:] - Rf.reshape(-1)).max(),
                                                     np.abs(twist[i, c] - vel).max() / max(1.0, np.abs(vel).max()))
            assert ep < FM.position_allowance(k, TOL), (cid, k, i, c)
            np.testing.assert_allclose(pose[i, c, 3:], Rf.reshape(-1), rtol=0, atol=1e-12)
            np.testing.assert_allclose(twist[i, c], vel, rtol=0, atol=1e-12 * max(1.0, np.abs(vel).max()))
    print(f"frame_state {cid} 2^{k}: position {worst_p:.2e} m, rotation / twist {worst_r:.2e}")


@pytest.mark.parametrize("k", FM.SHIFTS)
@pytest.mark.parametrize("cid", FM.TRANSLATION_KIN_CASES)
def test_fb_dcm_far_from_the_origin(handle, cid, k):
    cs = FM.build_case(cid)
    B, model = cs["B"], cs["model"]
    (st0, _), (st, _) = FM.shift_case(cs["states"], None, k)
    d = FM.shift_vec(k)
    omega = np.sqrt(9.81 / np.random.default_rng(1).uniform(0.5, 0.6, (B, 7)))
    com, xi = handle.fb_dcm(handle.fb_model(model), {key: _d(st[key][:B]) for key in native.FB_STATE_KEYS},
                            omega=_d(omega), column=3)
    torch.cuda.synchronize()
    com, xi = com.cpu().numpy(), xi.cpu().numpy()
    com_o, xi_o = CL.dcm_from_state(model, {key: st0[key][:B] for key in native.FB_STATE_KEYS}, omega[:, 3])
    ec = np.abs((com[:, :3] - d) - com_o[:, :3]).max()
    ex = np.abs((xi - d[:2]) - xi_o).max()
    ev = rel_err(com[:, 3:], com_o[:, 3:])
    print(f"fb_dcm {cid} 2^{k}: com {ec:.2e} m, dcm {ex:.2e} m, com velocity rel_err {ev:.2e}")
    assert ec < FM.position_allowance(k, TOL) and ex < FM.position_allowance(k, TOL)
    assert ev <= 1e-12


@pytest.mark.parametrize("k", FM.SHIFTS)
@pytest.mark.parametrize("cid", FM.TRANSLATION_IK_CASES)
def test_ik_far_from_the_origin(handle, cid, k):
    cs = IC.build_case(cid)
    model, B = cs["model"], min(cs["B"], 3)
    _, (st, tk) = FM.shift_ik(cs["states"], cs["tasks"], k)
    tk = IK.tasks_rows(tk, slice(0, B))
    sol0, int0 = IC.translation_reference(cid)
    dm = handle.fb_model(model)
    dev = lambda: {key: _d(st[key][:B]) for key in native.FB_STATE_KEYS}
    nu, status = handle.fb_ik_solve(dm, dev(), handle.ik_tasks(B, model["n"], **tk))
    nu = nu.cpu().numpy()
    assert (status.cpu().numpy() == IK.OK).all()
    worst_n = max(rel_err(nu[i], sol0[i][0]) for i in range(B))
    state = dev()
    _, _, status = handle.fb_ik_integrate(dm, state, handle.ik_tasks(B, model["n"], **tk), FM.IK_STEPS, FM.IK_DT)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == IK.OK).all()
    got = {key: v.cpu().numpy() for key, v in state.items()}
    errs = [FM.state_errors({key: got[key][i] for key in got}, int0[i][0], k, native.FB_STATE_KEYS) for i in range(B)]
    print(f"ik {cid} 2^{k}: nu rel_err {worst_n:.2e}, state rel_err {max(e for e, _ in errs):.2e}, "
          f"base_pos {max(p for _, p in errs):.2e} m")
    for i in range(B):
        assert sol0[i][1] == IK.OK and int0[i][2] == IK.OK
        assert rel_err(nu[i], sol0[i][0]) < TOL, (cid, k, i)
        assert errs[i][0] < TOL, (cid, k, i)
        assert errs[i][1] < FM.base_pos_allowance(k, FM.IK_STEPS), (cid, k, i)


@pytest.mark.parametrize("k", FM.QP_SHIFTS)
def test_dcm_mpc_cold_on_a_shifted_plan_matches_the_oracle_bitwise(handle, oracle, k):
    """The fp32 active-set search and the fp64 passes run on world coordinates: a whole plan at
    (2^k, -2^(k-1)) m, constraints assembled on the device as tests/test_gpu_dcm_mpc.py assembles
    them, against the oracle on the same shifted problem."""
    B = 64
    _, prob = FM.shift_plan(P.make_batch(B, horizon=100, n_footsteps=6, seed=77), k)
    dev = {key: torch.from_numpy(np.ascontiguousarray(prob[key])).cuda() for key in ("xi_init", "omega", "xi_ref", "vrp_ref")}
    A, b, nf = handle.assemble_constraints(torch.from_numpy(prob["corners"]).cuda(),
                                           torch.from_numpy(prob["ncorners"]).cuda())
    dev.update(A=A, b=b, nfacets=nf)
    out = handle.dcm_mpc_solve(dev)
    torch.cuda.synchronize()
    host = dict(prob, A=A.cpu().numpy(), b=b.cpu().numpy(), nfacets=nf.cpu().numpy())
    pol, pas = np.zeros(B, np.int32), np.zeros(B, np.int32)
    st_o, xi_o, vrp_o, it_o, _ = oracle.dcm_mpc_solve_batch_warm(host, threads=8, polished=pol, passes=pas)
    print(f"QP 2^{k}: iterations {it_o.min()} - {it_o.max()}, mean passes {pas.mean():.2f}, polished {pol.sum()} of {B}")
    assert (st_o == 0).all()
    np.testing.assert_array_equal(out["status"].cpu().numpy(), st_o)
    np.testing.assert_array_equal(out["iters"].cpu().numpy(), it_o)
    np.testing.assert_array_equal(out["passes"].cpu().numpy(), pas)
    np.testing.assert_array_equal(out["polished"].cpu().numpy(), pol)
    np.testing.assert_array_equal(out["xi"].cpu().numpy(), xi_o)
    np.testing.assert_array_equal(out["vrp"].cpu().numpy(), vrp_o)
