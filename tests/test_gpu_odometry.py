"""GPU tests of blf_schmitt_trigger_advance and blf_legged_odometry_advance (include/blf/blf_c.h
section 13) through blf.native, against tests/odometry_reference.py and against the device itself.

Models: fb_models.tree_model chains with n = 1, 26, 27 and 48 (26 | 27: two robots per wavefront | one),
a branching tree with prismatic joints, robot.humanoid24 with its sole frames; B in {1, 2, 3, 65}, T in
{1, 2, 7}, K in {1, 2, 8}.  The forces of the first robots are written out so that within 7 steps the
fixed foot changes over a double support, nothing is in contact, two slots make on the same sample (the
tie), values sit exactly on a threshold, with zero delays (shared parameters) and delays of some samples
(per-slot parameters); the other robots draw from the same five force levels, and every robot starts
on its own slot.

Discrete outputs (contact_out, fixed_out, trig_state, trig_timers, fixed_frame, status) must equal the
reference exactly; the continuous ones (base_pos, base_rot, base_vel, fixed_pose) within TOL = 1e-9 on
fb_models.rel_err, the bar of tests/test_gpu_ik.py.

Worst values seen on an MI355X (bar 1e-9 except where said):
  continuous outputs against the reference: chain1 4.0e-16, chain26 6.9e-15, chain27 9.8e-15, chain48 1.6e-14,
    the prismatic tree 1.1e-15, humanoid24 1.1e-15 (B = 65 each; fewer robots: at most 7.6e-15)
  self-consistency through blf_fb_frame_state: fixed frame pose 1.9e-15, twist 9.8e-15 (chain27)
  1024 m from the origin: positions shifted back within 3.3e-13 m (allowance 1e-9 + 9.1e-13)
  against the simulator (20 steps of 1 ms): 1.1e-15.  With Rf^T in place of the inverse of the true sole
    rotation the same comparison read 2.1e-09 at the first step: ForwardEuler does not re-orthonormalise
    base_rot, and the identity needs the inverse."""
import functools

import numpy as np
import pytest
import torch

import fb_models as FM
import odometry_reference as OR
from blf import closed_loop as DL
from blf import native, robot
from gpu_util import raises, to_device as _d

pytestmark = pytest.mark.gpu
TOL = 1e-9
rel_err = FM.rel_err
BATCHES = (1, 2, 3, 65)
STEPS = (1, 2, 7)
BMAX, TMAX = max(BATCHES), max(STEPS)
LEVELS = np.array([0.0, 4.0, 7.0, 10.0, 20.0])   # off_threshold and on_threshold among them
SHARED = np.array([10.0, 4.0, 0.0, 0.0])
DISCRETE = ("contact_out", "fixed_out", "status")
CONTINUOUS = ("base_pos", "base_rot", "base_vel")
STATE = ("trig_state", "trig_timers", "fixed_frame", "fixed_pose")

# id -> (model builder, the K frame indices of the slots, shared parameters?)
MODELS = {
    "chain1-k1": (lambda: FM.tree_model(FM.chain(1), seed=1), [1], True),
    "chain26-k2": (lambda: FM.tree_model(FM.chain(26), seed=2), [1, 2], False),
    "chain27-k8": (lambda: FM.tree_model(FM.chain(27), seed=3), [1, 3, 2, 0, 1, 2, 3, 1], True),
    "chain48-k2": (lambda: FM.tree_model(FM.chain(48), seed=4), [3, 2], True),
    "tree12pri-k8": (lambda: FM.tree_model(FM.random_tree(12, 3), seed=5, prismatic=(2, 5)),
                     [1, 2, 3, 0, 3, 2, 1, 0], False),
    "humanoid24-k2": (lambda: robot.humanoid24(), [0, 1], False),
}
# the written-out forces of robot 0, slot by slot (K = 1, 2, 8; the slots not listed stay at 0)
DESIGNED = {
    1: [[20, 20, 4, 4, 20, 10, 0]],
    2: [[20, 20, 20, 0, 0, 0, 20], [0, 0, 20, 20, 0, 0, 20]],
    8: [[20, 20, 0, 0, 0, 0, 20], [0, 20, 20, 0, 0, 0, 0], [0, 0, 0, 0, 10, 20, 20], [0, 0, 0, 0, 10, 20, 20]],
}


def _params(K, shared):
    if shared:
        return SHARED.copy()
    c = np.arange(K)
    return np.stack([np.full(K, 10.0), np.where(c % 2 == 0, 4.0, 10.0), 0.01 * (c % 3), 0.01 * ((c + 1) % 2)], axis=1)


@functools.lru_cache(maxsize=None)
def case(mid):
    """The inputs of BMAX robots over TMAX steps and the reference after each step count of STEPS (it
    composes exactly, so one pass serves them all).  Computed once, shared, never written to."""
    build, frames, shared = MODELS[mid]
    model = build()
    n, K = model["n"], len(frames)
    rng = np.random.default_rng(len(mid) + 100 * n)
    st = robot.random_states(model, BMAX, seed=n)
    q = st["joint_pos"][None] + np.cumsum(rng.normal(size=(TMAX, BMAX, n)) * 0.02, axis=0)
    qd = rng.normal(size=(TMAX, BMAX, n)) * 0.5
    force = LEVELS[rng.integers(0, len(LEVELS), (TMAX, BMAX, K))]
    force[:, 0, :] = 0.0
    for c, row in enumerate(DESIGNED[K]):
        force[:, 0, c] = row
    time = 0.5 + 0.01 * np.arange(TMAX)
    fixed = (np.arange(BMAX) % K).astype(np.int32)
    state0 = np.zeros((BMAX, K), dtype=np.int32)
    state0[np.arange(BMAX), fixed] = 1   # every robot stands on its own slot
    timers0 = np.zeros((BMAX, K, 2))
    pose0 = np.stack([OR.initial_fixed_pose(model, {k: v[b] for k, v in st.items()}, frames[fixed[b]])
                      for b in range(BMAX)])
    prm = _params(K, shared)
    ref, est, done, parts = {}, (state0, timers0, fixed, pose0), 0, []
    for T in STEPS:
        r = OR.advance(model, frames, prm, time[done:T], q[done:T], qd[done:T], force[done:T], *est)
        parts.append(r)
        est = tuple(r[k] for k in STATE)
        done = T
        ref[T] = {k: np.concatenate([p[k] for p in parts], axis=0) for k in CONTINUOUS + ("contact", "fixed_out")}
        ref[T].update({k: r[k] for k in STATE + ("status",)})
        ref[T]["contact_out"] = ref[T].pop("contact")
    full = ref[TMAX]
    # the branches the forces are built for, in robot 0 and across the batch
    assert (full["status"] == OR.OK).all()
    assert (full["contact_out"].sum(axis=2) == 0).any()                       # nothing in contact
    assert K == 1 or (np.diff(full["fixed_out"], axis=0) != 0).any()          # the fixed foot changes
    if K == 8 and shared:
        assert list(full["fixed_out"][:, 0]) == [0, 0, 1, 1, 2, 2, 2]   # the tie at step 4 takes slot 2, not 3
    if K == 2 and shared:
        assert list(full["fixed_out"][:, 0]) == [0, 0, 0, 1, 1, 1, 1]
    for a in (q, qd, force, time, fixed, state0, timers0, pose0, prm):
        a.setflags(write=False)
    return dict(model=model, frames=np.array(frames, dtype=np.int32), params=prm, time=time, q=q, qd=qd, force=force,
                est=dict(trig_state=state0, trig_timers=timers0, fixed_frame=fixed, fixed_pose=pose0), ref=ref)


def _est(cs, B, **over):
    e = {k: np.array(v[:B]) for k, v in cs["est"].items()}
    e.update(over)
    return {k: _d(v, torch.int32 if v.dtype == np.int32 else torch.float64) for k, v in e.items()}


def _run(handle, cs, B, t0, t1, est, q=None, qd=None, frames=None, dm=None, **kw):
    q = cs["q"] if q is None else q
    qd = cs["qd"] if qd is None else qd
    dm = dm or handle.fb_model(cs["model"])
    out = handle.legged_odometry(dm, _d(cs["frames"] if frames is None else frames, torch.int32), cs["params"],
                                 _d(cs["time"][t0:t1]), _d(q[t0:t1, :B]), None if qd is False else _d(qd[t0:t1, :B]),
                                 _d(cs["force"][t0:t1, :B]), est, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _host(est):
    return {k: v.cpu().numpy() for k, v in est.items()}


def _check_against(got, est, ref, B, where):
    worst = 0.0
    for k in DISCRETE:
        want = ref[k][:B] if k == "status" else ref[k][:, :B]
        np.testing.assert_array_equal(got[k], want, err_msg=f"{where}: {k}")
    for k in ("trig_state", "trig_timers", "fixed_frame"):
        np.testing.assert_array_equal(est[k], ref[k][:B], err_msg=f"{where}: {k}")
    for b in range(B):
        errs = [rel_err(got[k][:, b], ref[k][:, b]) for k in CONTINUOUS] + [rel_err(est["fixed_pose"][b], ref["fixed_pose"][b])]
        worst = max(worst, *errs)
        assert max(errs) < TOL, (where, b, errs)
    return worst


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mid", list(MODELS))
def test_odometry_against_reference_composition_and_triggers(handle, mid, B):
    cs = case(mid)
    dm = handle.fb_model(cs["model"])
    K = len(cs["frames"])
    worst = 0.0
    runs = {}
    for T in STEPS:
        est = _est(cs, B)
        got = _run(handle, cs, B, 0, T, est, dm=dm)
        runs[T] = (got, _host(est))
        worst = max(worst, _check_against(got, runs[T][1], cs["ref"][T], B, f"{mid} B={B} T={T}"))
    print(f"{mid} B={B}: continuous outputs rel_err {worst:.2e}")
    # composition: 2 steps then 5 equal 7, bit for bit, in every output and every state array
    est = _est(cs, B)
    a = _run(handle, cs, B, 0, 2, est, dm=dm)
    b = _run(handle, cs, B, 2, TMAX, est, dm=dm)
    whole, whole_est = runs[TMAX]
    for k in CONTINUOUS + ("contact_out", "fixed_out"):
        np.testing.assert_array_equal(np.concatenate([a[k], b[k]]), whole[k], err_msg=k)
    np.testing.assert_array_equal(b["status"], whole["status"])
    for k, v in _host(est).items():
        np.testing.assert_array_equal(v, whole_est[k], err_msg=k)
    # fused against unfused: the stand-alone triggers on the same samples
    state, timers = _d(cs["est"]["trig_state"][:B], torch.int32), _d(cs["est"]["trig_timers"][:B])
    _, _, so = handle.schmitt_trigger_advance(cs["params"], _d(cs["time"]), _d(cs["force"][:, :B]), state, timers)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(so.cpu().numpy(), whole["contact_out"])
    np.testing.assert_array_equal(state.cpu().numpy(), whole_est["trig_state"])
    np.testing.assert_array_equal(timers.cpu().numpy(), whole_est["trig_timers"])
    assert so.shape == (TMAX, B, K)


@pytest.mark.parametrize("mid", ["chain26-k2", "chain27-k8", "tree12pri-k8", "humanoid24-k2"])
def test_estimate_is_consistent_with_frame_state(handle, mid):
    """No reference involved: blf_fb_frame_state at the estimated base and the measured joints puts the fixed
    frame at fixed_pose, at rest."""
    cs = case(mid)
    B = 65
    dm = handle.fb_model(cs["model"])
    frames = _d(cs["frames"], torch.int32)
    wp = wt = 0.0
    for T in STEPS:
        est = _est(cs, B)
        got = _run(handle, cs, B, 0, T, est, dm=dm)
        state = dict(base_pos=_d(got["base_pos"][-1]), base_rot=_d(got["base_rot"][-1]), base_vel=_d(got["base_vel"][-1]),
                     joint_pos=_d(cs["q"][T - 1, :B]), joint_vel=_d(cs["qd"][T - 1, :B]))
        pose, twist = handle.fb_frame_state(dm, state, frames)
        torch.cuda.synchronize()
        pose, twist, e = pose.cpu().numpy(), twist.cpu().numpy(), _host(est)
        for b in range(B):
            f = got["fixed_out"][-1, b]
            assert f == e["fixed_frame"][b]
            scale = max(1.0, np.abs(got["base_vel"][-1, b]).max(), np.abs(cs["qd"][T - 1, b]).max())
            ep, et = rel_err(pose[b, f], e["fixed_pose"][b]), np.abs(twist[b, f]).max() / scale
            wp, wt = max(wp, ep), max(wt, et)
            assert ep < TOL and et < TOL, (mid, T, b, ep, et)
    print(f"{mid}: fixed frame pose {wp:.2e}, twist {wt:.2e}")


def test_far_from_the_origin(handle):
    """The estimator 1024 m out: the same robots with fixed_pose shifted exactly, compared with the
    reference on the unshifted inputs (the allowance of tests/test_gpu_fb_translation.py)."""
    cs, k, B = case("chain27-k8"), 10, 65
    d = FM.shift_vec(k)
    pose = np.array(cs["est"]["fixed_pose"])
    pose[:, :3] = FM.on_grid(pose[:, :3])
    ref = OR.advance(cs["model"], cs["frames"], cs["params"], cs["time"], cs["q"], cs["qd"], cs["force"],
                     cs["est"]["trig_state"], cs["est"]["trig_timers"], cs["est"]["fixed_frame"], pose)
    far = pose.copy()
    far[:, :3] += d
    est = _est(cs, B, fixed_pose=far)
    got = _run(handle, cs, B, 0, TMAX, est)
    e = _host(est)
    for key in ("contact_out", "fixed_out"):
        np.testing.assert_array_equal(got[key], ref["contact"] if key == "contact_out" else ref[key])
    worst = max(np.abs(got["base_pos"] - d - ref["base_pos"]).max(), np.abs(e["fixed_pose"][:, :3] - d - ref["fixed_pose"][:, :3]).max())
    print(f"2^{k} m: positions shifted back within {worst:.2e} m")
    assert worst < FM.position_allowance(k)
    for b in range(B):
        assert rel_err(got["base_rot"][:, b], ref["base_rot"][:, b]) < TOL
        assert rel_err(got["base_vel"][:, b], ref["base_vel"][:, b]) < TOL
        assert rel_err(e["fixed_pose"][b, 3:], ref["fixed_pose"][b, 3:]) < TOL


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_slot"])
@pytest.mark.parametrize("B,K", [(1, 1), (63, 1), (8, 8), (65, 1), (65, 2)])   # B K = 1, 63, 64, 65, 130
def test_trigger_batch_edges(handle, B, K, shared):
    rng = np.random.default_rng(B * 10 + K)
    T = 7
    prm = _params(K, shared)
    value = LEVELS[rng.integers(0, len(LEVELS), (T, B, K))]
    value[3, 0, 0] = np.nan   # a non-finite sample changes nothing
    time = 0.25 + 0.01 * np.arange(T)
    s0 = rng.integers(0, 4, (B, K)).astype(np.int32)
    t0 = np.stack([np.full((B, K), 0.24), rng.uniform(0.0, 0.2, (B, K))], axis=2)
    rs, rt, ro = OR.trigger_advance(prm, time, value, s0, t0)
    state, timers = _d(s0, torch.int32), _d(t0)
    _, _, out = handle.schmitt_trigger_advance(prm, _d(time), _d(value), state, timers)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), ro)
    np.testing.assert_array_equal(state.cpu().numpy(), rs)
    np.testing.assert_array_equal(timers.cpu().numpy(), rt)
    # one sample at a time, without state_out: the same final state
    state, timers = _d(s0, torch.int32), _d(t0)
    for t in range(T):
        r = handle.schmitt_trigger_advance(prm, _d(time[t:t + 1]), _d(value[t]), state, timers, state_out=False)
        assert r[2] is None
    torch.cuda.synchronize()
    np.testing.assert_array_equal(state.cpu().numpy(), rs)
    np.testing.assert_array_equal(timers.cpu().numpy(), rt)


def test_poisoned_robot_does_not_touch_its_neighbours(handle):
    cs, B, T = case("chain26-k2"), 3, TMAX   # robots 0 and 1 share a wavefront, robot 2 has one of its own half
    clean_est = _est(cs, B)
    clean = _run(handle, cs, B, 0, T, clean_est)
    for victim in (0, 1, 2):
        q = np.array(cs["q"])
        q[3, victim, 5] = np.nan
        est = _est(cs, B)
        got = _run(handle, cs, B, 0, T, est, q=q)
        e, ce = _host(est), _host(clean_est)
        for b in range(B):
            if b != victim:
                for k in CONTINUOUS + ("contact_out", "fixed_out"):
                    np.testing.assert_array_equal(got[k][:, b], clean[k][:, b], err_msg=k)
                for k in STATE:
                    np.testing.assert_array_equal(e[k][b], ce[k][b], err_msg=k)
        assert list(got["status"]) == [OR.BAD_INPUT if b == victim else OR.OK for b in range(B)]
        for k in CONTINUOUS:
            np.testing.assert_array_equal(got[k][:3, victim], clean[k][:3, victim])
            assert np.isnan(got[k][3:, victim]).all(), k
        assert (got["fixed_out"][3:, victim] == -1).all() and np.isnan(e["fixed_pose"][victim]).all()
        np.testing.assert_array_equal(got["contact_out"], clean["contact_out"])   # the triggers run on
        np.testing.assert_array_equal(e["trig_state"], ce["trig_state"])


def test_bad_fixed_frame_bad_frame_index_unknown_joint_type_and_null_velocity(handle):
    cs, B, T = case("tree12pri-k8"), 3, 2
    K = len(cs["frames"])
    clean = _run(handle, cs, B, 0, T, _est(cs, B))
    # fixed_frame out of range: that robot alone, and its fixed_frame is left as given
    for bad in (-1, K):
        fixed = np.array(cs["est"]["fixed_frame"][:B])
        fixed[1] = bad
        est = _est(cs, B, fixed_frame=fixed)
        got = _run(handle, cs, B, 0, T, est)
        assert list(got["status"]) == [OR.OK, OR.BAD_INPUT, OR.OK] and (got["fixed_out"][:, 1] == -1).all()
        assert np.isnan(got["base_pos"][:, 1]).all() and _host(est)["fixed_frame"][1] == bad
        np.testing.assert_array_equal(got["base_vel"][:, [0, 2]], clean["base_vel"][:, [0, 2]])
    # a frame index outside the model: every robot, no read past the model
    for bad in (-1, len(cs["model"]["frame_link"])):
        frames = np.array(cs["frames"])
        frames[K - 1] = bad
        got = _run(handle, cs, B, 0, T, _est(cs, B), frames=frames)
        assert (got["status"] == OR.BAD_INPUT).all() and (got["fixed_out"] == -1).all()
        assert all(np.isnan(got[k]).all() for k in CONTINUOUS)
        np.testing.assert_array_equal(got["contact_out"], clean["contact_out"])
    # an unknown joint type: NaN everywhere (the binding refuses such a model, so it is patched on the device)
    dm = handle.fb_model(cs["model"])
    dm.t["joint_type"][:] = 7
    got = _run(handle, cs, B, 0, T, _est(cs, B), dm=dm)
    assert all(np.isnan(got[k]).all() for k in CONTINUOUS) and (got["status"] == OR.BAD_INPUT).all()
    # joint_vel = NULL is zero velocities, bit for bit; a subset of the outputs is the same numbers
    zero = _run(handle, cs, B, 0, T, _est(cs, B), qd=np.zeros_like(cs["qd"]))
    null = _run(handle, cs, B, 0, T, _est(cs, B), qd=False, outputs=("base_pos", "base_vel"))
    assert sorted(null) == ["base_pos", "base_vel"]
    np.testing.assert_array_equal(null["base_pos"], zero["base_pos"])
    np.testing.assert_array_equal(null["base_vel"], zero["base_vel"])


def test_python_wrapper_names_the_argument_it_refuses(handle):
    cs, B = case("chain1-k1"), 2
    dm = handle.fb_model(cs["model"])
    args = lambda: (dm, _d(cs["frames"], torch.int32), cs["params"], _d(cs["time"][:2]), _d(cs["q"][:2, :B]),  # noqa: E731
                    _d(cs["qd"][:2, :B]), _d(cs["force"][:2, :B]))
    with pytest.raises(ValueError, match="normal_force has shape"):
        a = list(args())
        a[6] = _d(cs["force"][:1, :B])
        handle.legged_odometry(*a, _est(cs, B))
    with pytest.raises(ValueError, match="est.fixed_pose has shape"):
        handle.legged_odometry(*args(), _est(cs, B, fixed_pose=np.zeros((B, 11))))
    with pytest.raises(ValueError, match="params has shape"):
        a = list(args())
        a[2] = np.zeros((3, 4))
        handle.legged_odometry(*a, _est(cs, B))
    with pytest.raises(ValueError, match="unknown outputs"):
        handle.legged_odometry(*args(), _est(cs, B), outputs=("pose",))
    raises(1, handle.legged_odometry, *args()[:2], np.array([4.0, 10.0, 0.0, 0.0]), *args()[3:], _est(cs, B))
    raises(1, handle.schmitt_trigger_advance, np.array([10.0, 4.0, -1.0, 0.0]), _d(cs["time"][:1]),
           _d(cs["force"][:1, :B]), _d(np.zeros((B, 1)), torch.int32), _d(np.zeros((B, 1, 2))))
    # an empty batch is accepted
    out = handle.legged_odometry(dm, _d(cs["frames"], torch.int32), cs["params"], _d(cs["time"][:2]),
                                 _d(np.zeros((2, 0, 1))), None, _d(np.zeros((2, 0, 1))), _est(cs, 0))
    assert out["base_pos"].shape == (2, 0, 3)


def test_odometry_init_and_the_simulator(handle):
    """humanoid24 standing on compliant soles, 20 Euler steps of 1 ms: the odometry started from the true
    state, fed the measured joints and the soles' normal forces, reproduces the simulator's base.  Rigid-body
    kinematics fixes what it must give: est W_B(t) = fixed_pose_0 (true W_f(t))^-1 true W_B(t), with the
    device's own frame poses."""
    model = robot.humanoid24()
    B, T, n = 5, 20, model["n"]
    st = robot.standing_states(model, B, seed=9)
    dev = {k: _d(v) for k, v in st.items()}
    dm = handle.fb_model(model)
    frames = _d(np.arange(2), torch.int32)
    cp = _d(np.tile(np.asarray(DL.CONTACT_PARAMS), (2, 1)))
    null = _d(robot.sole_null_poses(model, st))
    contacts = dict(frame=frames, params=cp, null_pose=null)
    est = robot.odometry_init(dm, dev, frames, torch.tensor([0, 1, 0, 1, 0], dtype=torch.int32), handle=handle)
    est["trig_state"][:] = 1   # both soles on the ground
    pose0 = est["fixed_pose"].cpu().numpy().copy()
    fixed0 = est["fixed_frame"].cpu().numpy().copy()
    tau = _d(np.zeros((B, n)))
    q, qd, fz, truth = [], [], [], []
    for t in range(T):
        handle.fbd_euler_integrate(dm, dev, tau, 0.0, 0.001, 0.001, contacts=contacts)
        pose, twist = handle.fb_frame_state(dm, dev, frames)
        w = handle.contact_model_eval(cp.repeat(B, 1), twist.reshape(2 * B, 6), pose.reshape(2 * B, 12),
                                      null.reshape(2 * B, 12), outputs=("wrench",))["wrench"]
        q.append(dev["joint_pos"].clone()), qd.append(dev["joint_vel"].clone()), fz.append(w.reshape(B, 2, 6)[:, :, 2].clone())
        truth.append((dev["base_pos"].cpu().numpy(), dev["base_rot"].cpu().numpy(), pose.cpu().numpy()))
    force = torch.stack(fz)
    assert bool(torch.isfinite(force).all()) and float(force.abs().max()) > 0.0
    # an off_threshold no force reaches: both soles stay in contact, so the fixed foot never changes
    out = handle.legged_odometry(dm, frames, np.array([1.0, -1.0e9, 0.0, 0.0]), _d(0.001 * np.arange(1, T + 1)),
                                 torch.stack(q), torch.stack(qd), force, est)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert (got["status"] == 0).all() and (got["contact_out"] == 1).all() and (got["fixed_out"] == fixed0[None]).all()
    worst = 0.0
    for t in range(T):
        pB, RB, pose = truth[t]
        for b in range(B):
            pf, Rf = pose[b, fixed0[b], :3], pose[b, fixed0[b], 3:].reshape(3, 3)
            P, Q = pose0[b, :3], pose0[b, 3:].reshape(3, 3)
            Rf_inv = np.linalg.inv(Rf)        # not Rf.T: ForwardEuler leaves the simulator's base_rot off SO(3)
            R_fB = Rf_inv @ RB[b]             # (W_f)^-1 W_B
            p_fB = Rf_inv @ (pB[b] - pf)
            want_R, want_p = Q @ R_fB, P + Q @ p_fB
            e = max(rel_err(got["base_rot"][t, b], want_R), rel_err(got["base_pos"][t, b], want_p))
            worst = max(worst, e)
            assert e < TOL, (t, b, e)
    print(f"simulator: estimated base against the rigid-body identity {worst:.2e}")
