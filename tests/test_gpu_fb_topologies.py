"""GPU parity of the floating-base kernels of csrc/fb_dynamics.hip (fbd_dynamics_kernel,
fbd_euler_kernel, fb_dcm_kernel, fb_frame_state_kernel) against oracle/fb_dynamics.py across tree
topologies and sizes.  tests/test_gpu_fb_dynamics.py runs one tree, the humanoid (DFS preorder,
24 joints, depth 6, at most 4 children per link, two contacts on two leaves); the kernels' control
flow is chosen by the tree, so the cases of tests/fb_models.py put a model on each side of each
choice.  Which case drives which arm (tests/test_fb_models.py asserts the topology of each):

  mass-matrix path, Topo.dfs false      rand26-c8, bfs26-c1base, rand48-c8mixed, bfs48-c8 [matrix]
  mass-matrix path, Topo.dfs true       their -dfs relabellings (the same physical trees), chain48-c2,
                                        star48-c2, n1-c2 [matrix]
  mass-matrix path at HW = 64           every n = 48 [matrix] run (54-wide register row, DPP level 5,
                                        NV > 32 pivot columns, the factorization in the Euler kernel)
  NV = 32 exactly (n = 26)              chain26, star26, bfs26, rand26, and the n = 26 [matrix] runs
  n = 27, first one-per-wavefront size  chain27, star27, bfs27, rand27
  n = 48 = BLF_FBD_MAX_DOFS             chain48, star48, bfs48, rand48
  n = 1, n = 2                          chain1, star1, chain2, star2, n1-c2
  depth 7 | 8, 31 | 32 as maxdepth      chain8 | chain9, chain32 | chain33 (15 | 16 and every other
                                        depth up to 47 inside chain48: each joint of a chain has its
                                        own depth)
  star (48 children of the base)        star48, star48-c2
  C = 1 on the base link                bfs26-c1base, rand48-c1base [aba and matrix]
  C = 8: base, deepest leaf, two on one interior link, last link, three others
                                        rand26-c8, bfs48-c8; mixed laws: rand48-c8mixed [aba and matrix]
  prismatic at both wavefront layouts   pri-chain26-c2 (HW = 32), pri-rand48-c2 (HW = 64) [aba and matrix]

Metrics of tests/test_gpu_fb_dynamics.py: rel_err < 1e-9 on the accelerations and on every state key
after the Euler integration, exact base_pos / joint_pos derivatives, base_rot at 1e-15; every system
of every batch is checked, and a sentinel row past the batch must stay untouched.  The oracle's own
solve error on these systems is below 1e-10 (tests/test_fb_models.py).

Measured on an MI355X (worst acceleration rel_err of a run; the Euler states are below it): the
n = 48 chains 4.9e-11 (articulated-body) and 6.2e-11 (mass_reg = zeros), the 26- to 33-joint chains
1.5e-12 to 1.7e-11, every other tree at most 2e-12 -- the DFS arm's prefix differences cost a digit
against the level-by-level sums (up to 1e-12 against 3e-13 on the same physical tree) -- so no case
needs more than the forward bar.  The device solutions' backward errors |A x - b| / (|A||x| + |b|)
are 2e-18 to 1e-16, within 80 times the oracle's own on every run."""
import numpy as np
import pytest
import torch

import closed_loop as CL
import fb_dynamics as F
import fb_models as FM
from blf import native
from gpu_util import dev_contacts, to_device as _d

pytestmark = pytest.mark.gpu
TOL = 1e-9
rel_err = FM.rel_err


def run_device(handle, cid, kind):
    """blf_fbd_dynamics, then blf_fbd_euler_integrate over (T0, T1, DT), of the case's B systems
    with mass_reg of `kind` ("none": the articulated-body solve).  The state tensors hold one row
    more than the batch; that row must come back untouched."""
    cs = FM.build_case(cid)
    B, model, st = cs["B"], cs["model"], cs["states"]
    dm = handle.fb_model(model)
    reg = FM.reg_of(model, kind)
    kw = dict(contacts=dev_contacts(cs["contacts"], B), mass_reg=None if reg is None else _d(reg))
    full = {k: _d(st[k]) for k in native.FB_STATE_KEYS}
    view = {k: v[:B] for k, v in full.items()}
    tau = _d(st["joint_torque"][:B])
    acc = handle.fbd_dynamics(dm, view, tau, **kw)
    acc = {k: v.cpu().numpy() for k, v in acc.items()}
    for k in native.FB_STATE_KEYS:   # the dynamics reads the state only
        np.testing.assert_array_equal(full[k].cpu().numpy(), st[k], err_msg=k)
    handle.fbd_euler_integrate(dm, view, tau, FM.T0, FM.T1, FM.DT, **kw)
    torch.cuda.synchronize()
    for k in native.FB_STATE_KEYS:
        np.testing.assert_array_equal(full[k][B].cpu().numpy(), st[k][B], err_msg=f"sentinel row of {k}")
    return acc, {k: v.cpu().numpy() for k, v in view.items()}


def check_against_oracle(cid, kind, acc, got):
    """Every system of the batch against the oracle's reference of (case, kind)."""
    cs = FM.build_case(cid)
    dyn, eul = FM.reference(cid, "reg" if kind == "reg" else "none")
    worst_a = max(max(rel_err(acc["base_vel"][i], dyn[i][0]), rel_err(acc["joint_vel"][i], dyn[i][1]))
                  for i in range(cs["B"]))
    worst_e = max(rel_err(got[k][i], eul[i][k]) for i in range(cs["B"]) for k in native.FB_STATE_KEYS)
    print(f"{cid} [{kind}]: acceleration rel_err {worst_a:.2e}, Euler state rel_err {worst_e:.2e}")
    for i in range(cs["B"]):
        ba, ja, dp, dR, dq = dyn[i]
        assert rel_err(acc["base_vel"][i], ba) < TOL, (cid, kind, i)
        assert rel_err(acc["joint_vel"][i], ja) < TOL, (cid, kind, i)
        np.testing.assert_array_equal(acc["base_pos"][i], dp)
        np.testing.assert_allclose(acc["base_rot"][i], dR, rtol=0, atol=1e-15)
        np.testing.assert_array_equal(acc["joint_pos"][i], dq)
        for k in native.FB_STATE_KEYS:
            assert rel_err(got[k][i], eul[i][k]) < TOL, (cid, kind, i, k)


@pytest.mark.parametrize("cid,solve", FM.RUNS, ids=[f"{c}-{s}" for c, s in FM.RUNS])
def test_fbd_topologies_vs_oracle(handle, cid, solve):
    """Dynamics and a three-step Euler integration (the last step stale-time) of one case of the
    matrix in the module docstring.  "aba": the articulated-body solve.  "matrix": the mass-matrix /
    Cholesky path with mass_reg = 0.05 I against the oracle's reg=, and with mass_reg = zeros, the
    unregularised solution, against the oracle and against the device's own articulated-body
    result at 1e-9."""
    if solve == "aba":
        check_against_oracle(cid, "none", *run_device(handle, cid, "none"))
        return
    check_against_oracle(cid, "reg", *run_device(handle, cid, "reg"))
    acc0, got0 = run_device(handle, cid, "zero")
    check_against_oracle(cid, "zero", acc0, got0)
    acc_a, got_a = run_device(handle, cid, "none")
    for k in ("base_vel", "joint_vel"):
        assert rel_err(acc0[k], acc_a[k]) < TOL, (cid, k)
    for k in native.FB_STATE_KEYS:
        assert rel_err(got0[k], got_a[k]) < TOL, (cid, k)
    # the regularisation is seen: it changes the accelerations far beyond the tolerance
    dyn_r, dyn_0 = FM.reference(cid, "reg")[0], FM.reference(cid, "none")[0]
    assert rel_err(dyn_r[0][1], dyn_0[0][1]) > 1e-6


# depth 47 (6 jumping rounds), a non-DFS tree, and maxdepth 32 = 2^5, where a round short shows
KIN_CASES = ["chain48", "bfs27", "chain33"]


@pytest.mark.parametrize("cid", KIN_CASES)
def test_fb_frame_state_on_trees(handle, cid):
    """blf_fb_frame_state on the deepest chain and on a level-numbered tree: frames on the base,
    the deepest link, a link halfway down and the last link, and the index one past the model's
    frames, which must give NaN (tolerances of test_fb_frame_state_vs_oracle)."""
    cs = FM.build_case(cid)
    B, model, st = cs["B"], cs["model"], cs["states"]
    nf = len(model["frame_link"])
    frames = np.array([0, 1, 2, nf, 3], dtype=np.int32)
    dm = handle.fb_model(model)
    pose, twist = handle.fb_frame_state(dm, {k: _d(st[k][:B]) for k in native.FB_STATE_KEYS},
                                        _d(frames, torch.int32))
    pose, twist = pose.cpu().numpy(), twist.cpu().numpy()
    for i in range(B):
        K = F.kinematics(model, st["base_pos"][i], st["base_rot"][i], st["joint_pos"][i],
                         st["base_vel"][i], st["joint_vel"][i])
        for c, f in enumerate(frames):
            if f >= nf:
                assert np.isnan(pose[i, c]).all() and np.isnan(twist[i, c]).all()
                continue
            pf, Rf, vel, _ = F.frame_state(model, K, f)
            np.testing.assert_allclose(pose[i, c], np.concatenate([pf, Rf.reshape(-1)]), rtol=0, atol=1e-12)
            np.testing.assert_allclose(twist[i, c], vel, rtol=0, atol=1e-12 * max(1.0, np.abs(vel).max()))


@pytest.mark.parametrize("cid", KIN_CASES)
def test_fb_dcm_on_trees(handle, cid):
    """blf_fb_dcm on the same trees: centre of mass, its velocity and the DCM (tolerances of
    test_fb_dcm_vs_oracle)."""
    cs = FM.build_case(cid)
    B, model = cs["B"], cs["model"]
    st = {k: cs["states"][k][:B] for k in native.FB_STATE_KEYS}
    omega = np.sqrt(9.81 / np.random.default_rng(1).uniform(0.5, 0.6, (B, 7)))
    dm = handle.fb_model(model)
    com, xi = handle.fb_dcm(dm, {k: _d(v) for k, v in st.items()}, omega=_d(omega), column=3)
    torch.cuda.synchronize()
    com_o, xi_o = CL.dcm_from_state(model, st, omega[:, 3])
    assert rel_err(com.cpu().numpy(), com_o) <= 1e-12
    assert rel_err(xi.cpu().numpy(), xi_o) <= 1e-12
