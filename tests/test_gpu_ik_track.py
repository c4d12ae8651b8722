"""GPU parity of blf_fb_ik_track (csrc/fb_ik.hip, include/blf/blf_c.h section 12d) against
tests/ik_track_reference.py over the cases of tests/ik_track_cases.py, and the section's three equalities:

  reference    humanoid24 walking (two robots per wavefront) at B = 1, 2, 3 and T = 1, 2, 20: the pair of
               B = 2 holds opposite stance soles, T = 20 has every robot's lift-offs and touch-downs,
               B = 3 leaves a lone robot in the second wavefront; n = 48 (one robot per wavefront) with a
               mask per robot and per step; n = 12 where the wavefront's union of masks exceeds 6 + n
  independence a robot whose mask is dependent (by count, and by a failed pivot) next to one that resolves
  P1, P2       bit for bit at T = 20, B = 3 and 130; limits = NULL against the hard path to 1e-9
  P3           bit for bit: a robot's results do not depend on its wavefront's other robot
  failure      a NaN set point at step 2 of one robot of three
  purpose      swing_foot_eval -> fb_ik_track on device tensors: stance soles follow the hard rows' law;
               with the weights alone they do not
  refusals     call-level errors leave the outputs untouched

Metric: fb_models.rel_err < 1e-9 on every trajectory slice, the final state and nu against the reference;
status, fail_step, iters and active equal (tests/test_ik_track_reference.py holds every step of every case
at least 1e-7 from a tie on the CPU).

Measured on an MI355X (worst over the robots): walking humanoids 2.7e-14 at T = 20 (iters 23, 24, 28),
limbs48 1.4e-13 (iters 19, 15, 27), limbs12 2.1e-10; stance soles 4.42e-4 m from the hard rows' law and
3.46e-3 m with the weights alone, the reference's own figures."""
import ctypes

import numpy as np
import pytest
import torch

import fb_models as FM
import ik_limits_reference as LR
import ik_track_cases as TC
import ik_track_reference as TR
from blf import native
from gpu_util import dev_state, to_device as _d

pytestmark = pytest.mark.gpu
TOL = 1e-9
STANCE_LAW_TOL, CONTRAST_MIN = TC.STANCE_LAW_TOL, TC.CONTRAST_MIN
rel_err = FM.rel_err
DT = TC.DT
OUT = ("joint_traj", "base_traj", "nu_traj", "status", "fail_step", "iters", "active")


# local: the mask as a number, None for 0
def hard_of(rows):
    if rows == 0:
        return None
    h = native.IkHard()
    h.rows, h.reserved, h.rel_pivot_min = rows, 0, 0.0
    return h


def sub_schedule(sch, robots, steps=None):
    """The schedule of the robots `robots` (a slice) and the first `steps` steps."""
    T = sch["steps"] if steps is None else steps
    out = dict(sch, steps=T)
    for k in ("contact", "se3_pose", "se3_twist"):
        if sch.get(k) is not None:
            out[k] = np.ascontiguousarray(np.asarray(sch[k])[robots, :, :T])
    for k in ("com_pos", "com_vel"):
        if sch.get(k) is not None:
            out[k] = np.ascontiguousarray(np.asarray(sch[k])[robots, :T])
    return out


def dev_schedule(handle, sch, B, K):
    return handle.ik_schedule(B, K, sch["steps"], stance_rows=sch["stance_rows"],
                              contact=None if sch.get("contact") is None else np.asarray(sch["contact"], dtype=np.int32),
                              se3_pose=sch.get("se3_pose"), se3_twist=sch.get("se3_twist"),
                              com_pos=sch.get("com_pos"), com_vel=sch.get("com_vel"))


def run_track(handle, cs, robots=None, steps=None, schedule=None, limits="case", states=None, rows=None):
    """blf_fb_ik_track on the robots `robots` (a slice) of a case: (host dict of every output, final state)."""
    import ik_reference as IK
    robots = slice(None) if robots is None else robots
    model = cs["model"]
    st = dev_state(cs["states"] if states is None else states, robots)
    B = st["joint_pos"].shape[0]
    tasks = IK.tasks_rows(cs["tasks"], robots)
    K = len(tasks["frame"])
    tk = handle.ik_tasks(B, model["n"], **dict(tasks, se3_pose=None, com_pos=None, se3_twist=None, com_vel=None))
    sch = sub_schedule(cs["schedule"] if schedule is None else schedule, robots, steps)
    lim = cs["limits"] if limits == "case" else limits
    r = handle.fb_ik_track(handle.fb_model(model), st, tk, dev_schedule(handle, sch, B, K), cs["dT"],
                           hard=hard_of(cs["rows"] if rows is None else rows),
                           limits=None if lim is None else handle.ik_limits(**lim))
    torch.cuda.synchronize()
    out = {k: r[k].cpu().numpy() for k in OUT}
    return out, {k: v.cpu().numpy() for k, v in st.items()}


# local: robot i's (word 0, word 1) of a host array
def masks_of(active, i):
    a = active.astype(np.uint64)
    return (int(a[i, 0]), int(a[i, 1]))


def check_robot(tag, out, state, i, ref):
    """Robot i of a device run against a reference dict (TR.track's or TC.prefix's)."""
    assert out["status"][i] == ref["status"], (tag, i, out["status"][i], ref["status"])
    assert out["fail_step"][i] == ref["fail_step"], (tag, i, out["fail_step"][i])
    assert out["iters"][i] == ref["iters"], (tag, i, out["iters"][i], ref["iters"])
    assert masks_of(out["active"], i) == tuple(ref["active"]), (tag, i)
    worst = 0.0
    for k in ("joint_traj", "base_traj", "nu_traj"):
        got, want = out[k][:, i], ref[k]
        assert (np.isnan(got) == np.isnan(want)).all(), (tag, i, k)
        for t in range(want.shape[0]):
            if not np.isnan(want[t]).any():
                e = rel_err(got[t], want[t])
                assert e < TOL, (tag, i, k, t, e)
                worst = max(worst, e)
    for k in native.FB_STATE_KEYS:
        want = np.asarray(ref["state"][k], dtype=np.float64)
        got = state[k][i]
        if np.isnan(want).any():
            assert np.isnan(got).all(), (tag, i, k)
        else:
            e = rel_err(got, want)
            assert e < TOL, (tag, i, k, e)
            worst = max(worst, e)
    return worst


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("T", [1, 2, 20])
def test_walk_vs_reference(handle, B, T):
    """The walking humanoids against the reference: every slice, the final state, nu and the counters."""
    cs, ref = TC.build_case("walk"), TC.reference("walk")
    out, state = run_track(handle, cs, slice(0, B), T)
    worst = max(check_robot(("walk", B, T), out, state, i, TC.prefix(ref[i], T)) for i in range(B))
    print(f"walk B={B} T={T}: worst rel_err {worst:.2e}, iters {out['iters'].tolist()}")


@pytest.mark.parametrize("cid", ["limbs48", "limbs12"])
def test_per_robot_masks_vs_reference(handle, cid):
    """One robot per wavefront with a mask per robot and step (limbs48); a wavefront whose union of masks
    counts more rows than 6 + n while each robot's own does not (limbs12): every robot BLF_IK_OK."""
    cs, ref = TC.build_case(cid), TC.reference(cid)
    out, state = run_track(handle, cs)
    assert (out["status"] == LR.OK).all(), out["status"]
    worst = max(check_robot(cid, out, state, i, ref[i]) for i in range(cs["B"]))
    print(f"{cid}: worst rel_err {worst:.2e}, iters {out['iters'].tolist()}")


@pytest.mark.parametrize("cid", ["limbs12-over", "limbs12-dup"])
def test_dependent_neighbour_is_contained(handle, cid):
    """Robot 0's mask is dependent (more rows than 6 + n | two tasks on one frame): it alone gets
    BLF_IK_HARD_DEPENDENT at step 0, keeps its state and gets NaN slices; robot 1 of the same wavefront
    equals the reference, and its run alone (B = 1) bit for bit (P3)."""
    cs, ref = TC.build_case(cid), TC.reference(cid)
    out, state = run_track(handle, cs)
    assert out["status"].tolist() == [LR.HARD_DEPENDENT, LR.OK] and out["fail_step"].tolist() == [0, -1]
    check_robot(cid, out, state, 0, ref[0])
    check_robot(cid, out, state, 1, ref[1])
    for k in ("base_pos", "base_rot", "joint_pos"):
        np.testing.assert_array_equal(state[k][0], cs["states"][k][0], err_msg=k)
    alone, sa = run_track(handle, cs, slice(1, 2))
    for k in OUT:
        np.testing.assert_array_equal(alone[k][:, 0] if k.endswith("traj") else alone[k][0],
                                      out[k][:, 1] if k.endswith("traj") else out[k][1], err_msg=k)
    for k in native.FB_STATE_KEYS:
        np.testing.assert_array_equal(sa[k][0], state[k][1], err_msg=k)


def test_results_do_not_depend_on_the_neighbour(handle):
    """P3, bit for bit: each walking robot run alone, in the pair and in the three gives the same bits,
    although its neighbour's mask differs from its own at most steps and adds null rows to its solve."""
    cs = TC.build_case("walk")
    full, sf = run_track(handle, cs)
    for i in range(3):
        alone, sa = run_track(handle, cs, slice(i, i + 1))
        for k in OUT:
            np.testing.assert_array_equal(alone[k][:, 0] if k.endswith("traj") else alone[k][0],
                                          full[k][:, i] if k.endswith("traj") else full[k][i], err_msg=(i, k))
        for k in native.FB_STATE_KEYS:
            np.testing.assert_array_equal(sa[k][0], sf[k][i], err_msg=(i, k))
    # robots 1 and 2 swapped: robot 0 gets another neighbour
    perm = [0, 2, 1]
    st = {k: np.asarray(v)[perm] for k, v in cs["states"].items() if k in native.FB_STATE_KEYS}
    sch = sub_schedule(cs["schedule"], perm)
    import ik_reference as IK
    cs2 = dict(cs, states=st, tasks=IK.tasks_rows(cs["tasks"], perm), schedule=sch)
    other, so = run_track(handle, cs2)
    for k in OUT:
        np.testing.assert_array_equal(other[k][:, 0] if k.endswith("traj") else other[k][0],
                                      full[k][:, 0] if k.endswith("traj") else full[k][0], err_msg=k)


def _walk_case(B, shift):
    model, st, tasks, rows, limits, w = TC.walk_inputs(B, shift, seed=11)
    return dict(model=model, B=B, states=st, tasks=tasks, rows=rows, limits=limits,
                schedule=TC.swing_schedule(w, B, 2), dT=DT)


@pytest.mark.parametrize("B", [3, 130])
def test_fused_equals_stepped(handle, B):
    """P1: a 20-step call equals 20 one-step calls with the schedule's slices, bit for bit."""
    rng = np.random.default_rng(B)
    cs = _walk_case(B, rng.choice([0.0, 0.25, 0.5, 0.75], size=B))
    full, sf = run_track(handle, cs)
    assert (full["status"] == LR.OK).all(), full["status"]
    states = {k: np.asarray(cs["states"][k]).copy() for k in native.FB_STATE_KEYS}
    iters = np.zeros(B, dtype=np.int64)
    for t in range(20):
        one, states = run_track(handle, cs, schedule=TR.slice_schedule(cs["schedule"], t), states=states)
        assert (one["status"] == LR.OK).all()
        iters += one["iters"]
        for k in ("joint_traj", "base_traj", "nu_traj"):
            np.testing.assert_array_equal(one[k][0], full[k][t], err_msg=(t, k))
    for k in native.FB_STATE_KEYS:
        np.testing.assert_array_equal(states[k], sf[k], err_msg=k)
    np.testing.assert_array_equal(iters, full["iters"])
    np.testing.assert_array_equal(one["active"], full["active"])


@pytest.mark.parametrize("B", [3, 130])
def test_uniform_mask_equals_integrate_limits(handle, B):
    """P2: every robot in the same phase, so rows(., t) is one mask per step (it changes at the lift-offs
    and touch-downs): the call equals 20 x blf_fb_ik_integrate_limits(steps = 1) with that mask and step
    t's set points, bit for bit.  With limits = NULL it agrees with 20 x blf_fb_ik_integrate_hard to 1e-9."""
    cs = _walk_case(B, np.zeros(B))
    model, sch = cs["model"], cs["schedule"]
    dm = handle.fb_model(model)
    for lim in (cs["limits"], None):
        full, sf = run_track(handle, cs, limits=lim)
        assert (full["status"] == LR.OK).all(), full["status"]
        st = dev_state(cs["states"])
        iters = torch.zeros(B, dtype=torch.int64, device="cuda")
        seen = set()
        for t in range(20):
            rows = TR.rows_at(cs["rows"], sch, 0, t)
            assert all(TR.rows_at(cs["rows"], sch, i, t) == rows for i in range(B))
            seen.add(rows)
            tk = handle.ik_tasks(B, model["n"], **dict(cs["tasks"], se3_pose=sch["se3_pose"][:, :, t],
                                                       se3_twist=sch["se3_twist"][:, :, t],
                                                       com_pos=sch["com_pos"][:, t]))
            if lim is not None:
                _, nu, status, it, act = handle.fb_ik_integrate(dm, st, tk, 1, DT, hard=hard_of(rows),
                                                                limits=handle.ik_limits(**lim))
                iters += it
            else:
                _, nu, status = handle.fb_ik_integrate(dm, st, tk, 1, DT, hard=hard_of(rows))
            assert (status.cpu().numpy() == LR.OK).all()
            got = dict(nu_traj=nu.cpu().numpy(), joint_traj=st["joint_pos"].cpu().numpy(),
                       base_traj=np.concatenate([st["base_pos"].cpu().numpy(),
                                                 st["base_rot"].cpu().numpy().reshape(B, 9)], axis=1))
            for k, v in got.items():
                if lim is not None:
                    np.testing.assert_array_equal(full[k][t], v, err_msg=(t, k))
                else:
                    assert rel_err(full[k][t], v) < TOL, (t, k)
        assert len(seen) >= 3, seen
        if lim is not None:
            np.testing.assert_array_equal(iters.cpu().numpy(), full["iters"])
            np.testing.assert_array_equal(act.cpu().numpy(), full["active"])
            for k in native.FB_STATE_KEYS:
                np.testing.assert_array_equal(st[k].cpu().numpy(), sf[k], err_msg=k)


def test_nan_set_point_fails_at_its_step(handle):
    """Robot 1 of three has a NaN set point at step 2: BLF_IK_BAD_INPUT with fail_step 2, slices 0 and 1
    intact, NaN from slice 2 on, its state the one after step 1; robots 0 and 2 are bit for bit the
    clean run's."""
    cs = TC.build_case("walk")
    clean, sc = run_track(handle, cs, steps=6)
    sch = sub_schedule(cs["schedule"], slice(None), 6)
    sch["se3_pose"] = sch["se3_pose"].copy()
    sch["se3_pose"][1, 1, 2, 4] = np.nan
    out, state = run_track(handle, cs, schedule=sch)
    assert out["status"].tolist() == [LR.OK, LR.BAD_INPUT, LR.OK] and out["fail_step"].tolist() == [-1, 2, -1]
    for k in ("joint_traj", "base_traj", "nu_traj"):
        np.testing.assert_array_equal(out[k][:2, 1], clean[k][:2, 1], err_msg=k)
        assert np.isnan(out[k][2:, 1]).all(), k
        np.testing.assert_array_equal(out[k][:, [0, 2]], clean[k][:, [0, 2]], err_msg=k)
    np.testing.assert_array_equal(state["joint_pos"][1], clean["joint_traj"][1, 1])
    np.testing.assert_array_equal(state["base_pos"][1], clean["base_traj"][1, 1, :3])
    np.testing.assert_array_equal(state["base_rot"][1].reshape(-1), clean["base_traj"][1, 1, 3:])
    assert np.isnan(state["base_vel"][1]).all() and np.isnan(state["joint_vel"][1]).all()
    assert masks_of(out["active"], 1) == (0, 0)
    for k in native.FB_STATE_KEYS:
        np.testing.assert_array_equal(state[k][[0, 2]], sc[k][[0, 2]], err_msg=k)


def test_contact_lists_to_joint_trajectories_on_device(handle):
    """What the call is for: robot.walking_ik_schedule -> swing_foot_eval -> fb_ik_track, the device
    tensors passed on as they stand.  Every stance sole's linear error after a contact of m steps is
    (1 - kp_lin dT)^m times its error at the contact's start, to STANCE_LAW_TOL (the Euler step's drift,
    tests/ik_track_cases.py says where it comes from); with stance_rows = 0, the weights
    alone, the stance soles end at least CONTRAST_MIN from that law."""
    B, K, T = 3, 2, TC.WALK_T   # the walking case's own inputs: the two bounds were measured on them
    model, st, tasks, rows, limits, w = TC.walk_inputs(B, TC.WALK_SHIFT)
    dm = handle.fb_model(model)
    sw = handle.swing_foot_eval(_d(w["contact_pose"]), _d(w["contact_time"]), _d(w["ncontacts"], torch.int32),
                                _d(w["tq"]), step_height=w["step_height"],
                                outputs=("pose", "twist", "in_contact"))
    tk = handle.ik_tasks(B, model["n"], **dict(tasks, se3_pose=None, com_pos=None))
    lm = handle.ik_limits(**limits)
    worst = {}
    for name, stance in (("hard", w["stance_rows"]), ("weights", 0)):
        sc = handle.ik_schedule(B, K, T, stance_rows=stance, contact=sw["in_contact"], se3_pose=sw["pose"],
                                se3_twist=sw["twist"], com_pos=w["com_pos"])
        assert sc.t["se3_pose"].data_ptr() == sw["pose"].data_ptr()
        r = handle.fb_ik_track(dm, dev_state(st), tk, sc, DT, hard=hard_of(rows), limits=lm)
        torch.cuda.synchronize()
        assert (r["status"].cpu().numpy() == LR.OK).all(), r["status"]
        sch = dict(contact=sw["in_contact"].cpu().numpy().reshape(B, K, T),
                   se3_pose=sw["pose"].cpu().numpy().reshape(B, K, T, 12))
        bt, jt = r["base_traj"].cpu().numpy(), r["joint_traj"].cpu().numpy()
        worst[name] = max(TC.stance_law_error(model, tasks, st, sch, i, bt[:, i], jt[:, i], DT)[0] for i in range(B))
    print(f"stance soles against the law: hard rows {worst['hard']:.3g} m, weights only {worst['weights']:.3g} m")
    assert worst["hard"] <= STANCE_LAW_TOL
    assert worst["weights"] >= CONTRAST_MIN


def _raw_call(handle, cs, **over):
    """blf_fb_ik_track through ctypes with sentinel-filled outputs: (return code, outputs untouched)."""
    model, B = cs["model"], cs["B"]
    n, T = model["n"], cs["schedule"]["steps"]
    dm = handle.fb_model(model)
    st = dev_state(cs["states"])
    before = {k: v.clone() for k, v in st.items()}
    tk = handle.ik_tasks(B, n, **dict(cs["tasks"], se3_pose=None, com_pos=None, se3_twist=None, com_vel=None,
                                      **over.pop("tasks", {})))
    sc = dev_schedule(handle, cs["schedule"], B, len(cs["tasks"]["frame"]))
    for k, v in over.pop("schedule", {}).items():
        setattr(sc.c, k, v)
    hard = hard_of(over.pop("rows", cs["rows"]))
    outs = [torch.full((T, B, n), 7.0, dtype=torch.float64, device="cuda"),
            torch.full((T, B, 12), 7.0, dtype=torch.float64, device="cuda"),
            torch.full((T, B, 6 + n), 7.0, dtype=torch.float64, device="cuda"),
            torch.full((B,), 7, dtype=torch.int32, device="cuda"), torch.full((B,), 7, dtype=torch.int32, device="cuda"),
            torch.full((B,), 7, dtype=torch.int32, device="cuda"), torch.full((B, 2), 7, dtype=torch.int64, device="cuda")]
    fs = handle._fb_state(st, B, n)
    for k in over.pop("null_state", ()):
        setattr(fs, k, None)
    rc = native.lib().blf_fb_ik_track(handle._h, ctypes.byref(dm.c), ctypes.byref(fs), ctypes.byref(tk.c),
                                      ctypes.byref(hard) if hard is not None else None, None, ctypes.byref(sc.c),
                                      over.pop("batch", B), over.pop("dT", cs["dT"]),
                                      *[ctypes.c_void_p(o.data_ptr()) for o in outs], None)
    torch.cuda.synchronize()
    untouched = all(bool((o == 7).all().item()) for o in outs) and \
        all(torch.equal(st[k], before[k]) for k in st)
    return rc, untouched


@pytest.mark.parametrize("over,word", [
    (dict(schedule=dict(steps=0)), "steps"),
    (dict(schedule=dict(reserved=1)), "reserved"),
    (dict(schedule=dict(reserved2=1)), "reserved"),
    (dict(schedule=dict(stance_rows=1 << 12)), "stance_rows"),
    (dict(schedule=dict(se3_pose=None)), "se3_pose"),
    (dict(schedule=dict(com_pos=None)), "com_pos"),
    (dict(tasks=dict(se3_weight=np.array([[1.0] * 6, [1.0, 1.0, 0.0, 1.0, 1.0, 1.0]]))), "weight 0"),
    (dict(null_state=("base_vel",)), "state"),
    (dict(dT=0.0), "dT"),
    (dict(rows=1 << 13), "rows"),
])
def test_call_level_refusals(handle, over, word):
    """BLF_ERR_INVALID_ARGUMENT with a message that names the argument, and no output is written."""
    cs = TC.build_case("walk")
    rc, untouched = _raw_call(handle, cs, **over)
    assert rc == 1 and word in native.last_error() and "blf_fb_ik_track" in native.last_error(), native.last_error()
    assert untouched


def test_empty_batch_is_ok(handle):
    cs = TC.build_case("walk")
    rc, untouched = _raw_call(handle, cs, batch=0)
    assert rc == 0 and untouched
