"""GPU tests of blf_fb_inverse_dynamics (include/blf/blf_c.h section 8b) and of
blf_fbd_euler_integrate_computed_torque_traj (section 9) against tests/inverse_dynamics_reference.py, which
goes through the dense mass matrix of oracle/fb_dynamics.py.  The bar is the floating-base kernels' own:
1e-9 relative (fb_models.rel_err), fb_models.position_allowance for positions written 8 km out."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fb_models as FM
import impedance_traj_cases as TC
import inverse_dynamics_reference as ID
from blf import native
from blf import robot
from blf.closed_loop import fixed_step_schedule
from gpu_util import assert_bitwise, dev_contacts, to_device as _d

pytestmark = pytest.mark.gpu
TOL = 1e-9
INVALID, UNSUPPORTED = 1, 3
KP, KD = 400.0, 40.0   # 20 rad/s, critically damped: sqrt(kp) h = 0.04 at the stale 2 ms step
SCHEDULE = fixed_step_schedule(TC.T0, TC.T1, TC.DT)


def _np(d):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


# local: the first B robots of the state (gpu_util.dev_state takes an index set)
def dev_state(st, B):
    return {k: _d(st[k][:B]) for k in native.FB_STATE_KEYS}


# ---- the parity cases: id -> (model, states, contacts or None, B) -----------------------------------------
# h24-soles / h24p: two robots per wavefront and the odd batch's padding system, both soles continuous;
# h24-free: random states, no contacts; rand26-c8 | rand27: the last two-per-wavefront size and the first
# one-per-wavefront size; rand48-c8mixed: eight contacts of mixed laws; n1-c2: one joint; chain33, star26,
# rand48 (not DFS-ordered) at B = 2; h24-b130: more than one workgroup in either layout.
@functools.lru_cache(maxsize=None)
def id_case(cid):
    if cid in ("h24-soles", "h24p"):
        cs = TC.build_case("h24" if cid == "h24-soles" else "h24p")
        return cs["model"], cs["states"], cs["contacts"], 3
    if cid in ("h24-free", "h24-b130"):
        model = robot.humanoid24()
        B = 3 if cid == "h24-free" else 130
        return model, robot.random_states(model, B, seed=31), None, B
    cs = FM.build_case(cid)
    B = 2 if cid in ("chain33", "star26", "rand48") else 3
    return cs["model"], cs["states"], cs["contacts"], B


ID_CASES = ("h24-soles", "h24-free", "h24p", "rand26-c8", "rand27", "rand48-c8mixed", "n1-c2", "chain33", "star26",
            "rand48", "h24-b130")


@functools.lru_cache(maxsize=None)
def id_inputs(cid):
    model, _, _, B = id_case(cid)
    rng = np.random.default_rng(17)
    return rng.normal(size=(B, model["n"])) * 3.0, rng.normal(size=(B, 6)) * np.array([2.0] * 3 + [4.0] * 3)


@functools.lru_cache(maxsize=None)
def id_reference(cid):
    """The helper's free-base and given-base results of every robot of the case, computed once."""
    model, st, ct, B = id_case(cid)
    sdd, ba = id_inputs(cid)
    free = [ID.inverse_dynamics(model, st, i, joint_acc=sdd[i], **FM.oracle_kw(ct, i)) for i in range(B)]
    given = [ID.inverse_dynamics(model, st, i, joint_acc=sdd[i], base_acc=ba[i], **FM.oracle_kw(ct, i))
             for i in range(B)]
    return free, given


def run_id(handle, model, st, ct, B, joint_acc=None, base_acc=None):
    out = handle.fb_inverse_dynamics(handle.fb_model(model), dev_state(st, B),
                                     joint_acc=None if joint_acc is None else _d(joint_acc),
                                     base_acc=None if base_acc is None else _d(base_acc), contacts=dev_contacts(ct, B))
    torch.cuda.synchronize()
    return _np(out)


def test_the_tree_cases_are_what_they_claim():
    assert not FM.is_dfs_preorder(id_case("rand48")[0]["parent"])
    assert id_case("rand26-c8")[0]["n"] + 6 == 32 and id_case("rand27")[0]["n"] + 6 == 33
    assert id_case("rand48-c8mixed")[2]["law"] is not None and len(id_case("rand48-c8mixed")[2]["frame"]) == 8


@pytest.mark.parametrize("cid", ID_CASES)
def test_parity_both_modes(handle, cid):
    """1: joint torques and base acceleration (free base) / base wrench (given base) against the helper."""
    model, st, ct, B = id_case(cid)
    sdd, ba = id_inputs(cid)
    free, given = id_reference(cid)
    got = run_id(handle, model, st, ct, B, joint_acc=sdd)
    assert (got["status"] == 0).all()
    worst = 0.0
    for i in range(B):
        worst = max(worst, FM.rel_err(got["joint_torque"][i], free[i][1]), FM.rel_err(got["base_acc"][i], free[i][0]))
    got = run_id(handle, model, st, ct, B, joint_acc=sdd, base_acc=ba)
    assert (got["status"] == 0).all()
    for i in range(B):
        worst = max(worst, FM.rel_err(got["joint_torque"][i], given[i][1]),
                    FM.rel_err(got["base_wrench"][i], given[i][0]))
    print(cid, "worst rel err %.3g" % worst)
    assert worst <= TOL, (cid, worst)


def test_null_joint_acc_is_zero_and_bias_forces(handle):
    """joint_acc NULL is zero; given-base mode with nu_dot = 0 and no contacts is generalizedBiasForces."""
    model, st, _, B = id_case("h24-free")
    got = run_id(handle, model, st, None, B, base_acc=np.zeros((B, 6)))
    zero = run_id(handle, model, st, None, B, joint_acc=np.zeros((B, model["n"])), base_acc=np.zeros((B, 6)))
    np.testing.assert_array_equal(got["joint_torque"], zero["joint_torque"])
    for i in range(B):
        wr, tau = ID.inverse_dynamics(model, st, i, base_acc=np.zeros(6))
        assert FM.rel_err(got["joint_torque"][i], tau) <= TOL and FM.rel_err(got["base_wrench"][i], wr) <= TOL


@pytest.mark.parametrize("cid", ["h24-soles", "rand48-c8mixed"])
@pytest.mark.parametrize("reg", [False, True])
def test_device_round_trip(handle, cid, reg):
    """2: the torque of the new call fed into blf_fbd_dynamics returns the requested joint accelerations and
    the same base acceleration, on the articulated-body path and with mass_reg = zeros."""
    model, st, ct, B = id_case(cid)
    sdd, _ = id_inputs(cid)
    dm, ds, dc = handle.fb_model(model), dev_state(st, B), dev_contacts(ct, B)
    inv = handle.fb_inverse_dynamics(dm, ds, joint_acc=_d(sdd), contacts=dc)
    n = model["n"]
    fwd = handle.fbd_dynamics(dm, ds, inv["joint_torque"], contacts=dc,
                              mass_reg=_d(np.zeros((n + 6, n + 6))) if reg else None)
    torch.cuda.synchronize()
    e_j = FM.rel_err(fwd["joint_vel"].cpu().numpy(), sdd)
    e_b = FM.rel_err(fwd["base_vel"].cpu().numpy(), inv["base_acc"].cpu().numpy())
    print(cid, "mass_reg" if reg else "aba", "joint acc %.3g base acc %.3g" % (e_j, e_b))
    assert e_j <= TOL and e_b <= TOL


def test_far_from_the_origin(handle):
    """3: fb_models.shift_case(k = 13): 8 km from the origin the torques, the base acceleration and the base
    wrench are those of the unshifted problem within the bar."""
    cs = FM.translation_case("humanoid24")
    model, B = cs["model"], 3
    (g_st, g_ct), (s_st, s_ct) = FM.shift_case(cs["states"], cs["contacts"], 13)
    rng = np.random.default_rng(19)
    sdd, ba = rng.normal(size=(B, model["n"])) * 3.0, rng.normal(size=(B, 6))
    free = run_id(handle, model, s_st, s_ct, B, joint_acc=sdd)
    given = run_id(handle, model, s_st, s_ct, B, joint_acc=sdd, base_acc=ba)
    worst = 0.0
    for i in range(B):
        ab, tau = ID.inverse_dynamics(model, g_st, i, joint_acc=sdd[i], **FM.oracle_kw(g_ct, i))
        wr, tau2 = ID.inverse_dynamics(model, g_st, i, joint_acc=sdd[i], base_acc=ba[i], **FM.oracle_kw(g_ct, i))
        worst = max(worst, FM.rel_err(free["joint_torque"][i], tau), FM.rel_err(free["base_acc"][i], ab),
                    FM.rel_err(given["joint_torque"][i], tau2), FM.rel_err(given["base_wrench"][i], wr))
    print("8 km out: worst rel err %.3g" % worst)
    assert worst <= TOL, worst


@pytest.mark.parametrize("field", ["joint_acc", "base_acc", "joint_pos", "wrench"])
def test_bad_input_is_per_robot(handle, field):
    """4: a NaN in robot 1's input gives robot 1 NaN outputs and BLF_IK_BAD_INPUT; robots 0 (its wavefront
    partner) and 2 keep the clean run's bits and status 0."""
    cid = "rand26-c8" if field != "wrench" else "rand48-c8mixed"
    model, st, ct, B = id_case(cid)
    sdd, ba = id_inputs(cid)
    given = field == "base_acc"
    clean = run_id(handle, model, st, ct, B, joint_acc=sdd, base_acc=ba if given else None)
    sdd2, ba2, st2, ct2 = sdd.copy(), ba.copy(), {k: v.copy() for k, v in st.items()}, ct
    if field == "joint_acc":
        sdd2[1, 5] = np.nan
    elif field == "base_acc":
        ba2[1, 4] = np.inf
    elif field == "joint_pos":
        st2["joint_pos"][1, 3] = np.nan
    else:
        ct2 = dict(ct, wrench=ct["wrench"].copy())
        ct2["wrench"][1, 1, 2] = np.nan   # contact 1 follows the given-wrench law
        assert ct["law"][1] == FM.CONTACT_WRENCH
    got = run_id(handle, model, st2, ct2, B, joint_acc=sdd2, base_acc=ba2 if given else None)
    six = "base_wrench" if given else "base_acc"
    assert np.isnan(got["joint_torque"][1]).all() and np.isnan(got[six][1]).all()
    assert got["status"].tolist() == [0, native.IK_BAD_INPUT, 0]
    for k in ("joint_torque", six):
        np.testing.assert_array_equal(got[k][[0, 2]], clean[k][[0, 2]], err_msg=k)


def test_unknown_joint_type_gives_nan(handle):
    model, st, ct, B = id_case("h24p")
    dm = handle.fb_model(model)
    dm.t["joint_type"][4] = 7   # (blf.native refuses it on upload; written behind its back)
    out = handle.fb_inverse_dynamics(dm, dev_state(st, B), joint_acc=_d(id_inputs("h24p")[0]),
                                     contacts=dev_contacts(ct, B))
    torch.cuda.synchronize()
    assert torch.isnan(out["joint_torque"]).all() and torch.isnan(out["base_acc"]).all()
    assert (out["status"] != 0).all()


def test_call_level_refusals(handle):
    """4: every refusal of the header's statement, with live buffers; nothing is written."""
    model, st, ct, B = id_case("h24-soles")
    n = model["n"]
    dm, ds, dc = handle.fb_model(model), dev_state(st, B), dev_contacts(ct, B)
    tau = torch.full((B, n), 7.0, dtype=torch.float64, device="cuda")
    six = torch.full((B, 6), 7.0, dtype=torch.float64, device="cuda")
    ba = _d(np.zeros((B, 6)))
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(h=True, m=None, state=True, base_acc=None, jt=True, bao=True, bw=True, batch=B, reserved=0, contacts=None):
        fs = handle._fb_state(ds, B, n)
        return native.lib().blf_fb_inverse_dynamics(
            handle._h if h else None, ctypes.byref(m if m is not None else dm.c), ctypes.byref(fs) if state else None,
            None, base_acc, ctypes.byref(contacts if contacts is not None else handle._fb_contacts(dc, B)), batch,
            p(tau) if jt else None, p(six) if bao else None, p(six) if bw else None, None, reserved,
            native._stream(None))

    assert call(h=False) == INVALID and call(state=False) == INVALID
    assert native.lib().blf_fb_inverse_dynamics(handle._h, None, None, None, None, None, B, None, None, None, None, 0,
                                                None) == INVALID
    assert call(jt=False) == INVALID
    assert call(bao=False) == INVALID and "base_acc_out" in native.last_error()   # free-base mode needs it ...
    assert call(bw=False) == 0                                                    # ... and not the wrench
    assert call(base_acc=p(ba), bw=False) == INVALID and "base_wrench" in native.last_error()
    assert call(base_acc=p(ba), bao=False) == 0
    torch.cuda.synchronize()
    tau.fill_(7.0)
    six.fill_(7.0)
    assert call(reserved=1) == INVALID and call(batch=-1) == INVALID
    for ndof in (0, 49):
        m = native.FbModel.from_buffer_copy(dm.c)
        m.ndof = ndof
        assert call(m=m) == UNSUPPORTED, ndof
    many = handle._fb_contacts(dc, B)
    many.ncontacts = 9
    assert call(contacts=many) == UNSUPPORTED
    assert call(batch=0) == 0
    torch.cuda.synchronize()
    assert (tau == 7.0).all() and (six == 7.0).all()


# ---- the fused call ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ct_refs(cid, B, T=4):
    """TC.references' slices plus qdd_ref [T,B,n] within 1 rad/s^2."""
    r = dict(TC.references(cid, B, T))
    r["qdd"] = np.random.default_rng(23).uniform(-1.0, 1.0, (T, B, TC.build_case(cid)["model"]["n"]))
    return r


@functools.lru_cache(maxsize=None)
def ct_reference(cid, B, sps=5, tau_max=None, jump=0.0):
    """The helper over ct_refs(cid, B) (robot 1's q_ref moved by `jump` on every joint), once and shared:
    a list of (state, tau_last, clamped)."""
    cs, r = TC.build_case(cid), ct_refs(cid, B)
    out = []
    for i in range(B):
        q = r["q_ref"][:, i] + (jump if i == 1 else 0.0)
        out.append(ID.euler_integrate_computed_torque_traj(
            cs["model"], cs["states"], i, q, KP, KD, sps, TC.T0, TC.T1, TC.DT, qd_ref=r["nu"][:, i, 6:],
            qdd_ref=r["qdd"][:, i], q_bias=r["q_bias"][i], tau_max=tau_max, **FM.oracle_kw(cs["contacts"], i)))
    for s, _, _ in out:
        assert all(np.isfinite(v).all() for v in s.values()), (cid, "the reference diverged")
    return out


def run_ct(handle, cid, B, q_ref, sps=5, nu=None, qdd=None, q_bias=None, tau_max=None, mass_reg=None, check=True):
    """The fused call on robots 0 .. B - 1 of the case: (final state as host arrays, tau_last)."""
    cs = TC.build_case(cid)
    dm, ds, dc = handle.fb_model(cs["model"]), dev_state(cs["states"], B), dev_contacts(cs["contacts"], B)
    law = handle.computed_torque_traj(KP, KD, _d(q_ref), sps, qd_ref=None if nu is None else _d(nu), qd_offset=6,
                                      qdd_ref=None if qdd is None else _d(qdd),
                                      q_bias=None if q_bias is None else _d(q_bias), tau_max=tau_max, tau_last=True)
    handle.fbd_euler_integrate_computed_torque_traj(dm, ds, law, TC.T0, TC.T1, TC.DT, contacts=dc,
                                                    mass_reg=None if mass_reg is None else _d(mass_reg))
    torch.cuda.synchronize()
    return _np(ds), law.tau_last.cpu().numpy()


def full(handle, cid, B, r, **kw):
    return run_ct(handle, cid, B, r["q_ref"], nu=r["nu"], qdd=r["qdd"], q_bias=r["q_bias"], **kw)


@pytest.mark.parametrize("cid,B", [("h24", 3), ("h24p", 3), ("n48", 2)])
def test_fused_call_against_the_helper(handle, cid, B):
    """5: T = 4 distinct slices of 5 steps over the closed loop's 19-step schedule with qd_ref, qdd_ref and
    q_bias: every state key against the helper; joint_pos / joint_vel against joint_recurrence, which knows
    no dynamics; and the unfused device sequence (per step blf_fb_inverse_dynamics, then a one-step
    blf_fbd_euler_integrate) within the same bar."""
    cs, r = TC.build_case(cid), ct_refs(cid, B)
    got, tau_last = full(handle, cid, B, r)
    ref = ct_reference(cid, B)
    for i in range(B):
        for k in native.FB_STATE_KEYS:
            e = FM.rel_err(got[k][i], ref[i][0][k])
            print(cid, "robot", i, k, "rel err %.3g" % e)
            assert e <= TOL, (cid, i, k, e)
        assert FM.rel_err(tau_last[i], ref[i][1]) <= TOL
    q, qd = ID.joint_recurrence(cs["states"]["joint_pos"][:B], cs["states"]["joint_vel"][:B],
                                dict(q_ref=r["q_ref"], qd_ref=r["nu"][..., 6:], qdd_ref=r["qdd"], q_bias=r["q_bias"]),
                                KP, KD, SCHEDULE, 5)
    e_q, e_v = FM.rel_err(got["joint_pos"], q), FM.rel_err(got["joint_vel"], qd)
    print(cid, "joint recurrence: pos %.3g vel %.3g" % (e_q, e_v))
    assert e_q <= TOL and e_v <= TOL
    assert np.abs(got["joint_pos"] - cs["states"]["joint_pos"][:B]).max() > 1e-5
    # the unfused device sequence
    dm, ds, dc = handle.fb_model(cs["model"]), dev_state(cs["states"], B), dev_contacts(cs["contacts"], B)
    qr, nu, qdd, qb = _d(r["q_ref"]), _d(r["nu"]), _d(r["qdd"]), _d(r["q_bias"])
    for k, h in enumerate(SCHEDULE):
        sl = min(k // 5, 3)
        sdd = qdd[sl] + KP * (qr[sl] + qb - ds["joint_pos"]) + KD * (nu[sl][:, 6:] - ds["joint_vel"])
        tau = handle.fb_inverse_dynamics(dm, ds, joint_acc=sdd.contiguous(), contacts=dc)["joint_torque"]
        handle.fbd_euler_integrate(dm, ds, tau, 0.0, h, h, contacts=dc)
    torch.cuda.synchronize()
    seq = _np(ds)
    dev = max(FM.rel_err(got[k], seq[k]) for k in native.FB_STATE_KEYS)
    print(cid, "fused against the unfused device sequence: %.3g" % dev)
    assert dev <= TOL


def test_clamp(handle):
    """6: robot 1 of 3 gets a reference jump of 0.5 rad on every joint that saturates under tau_max = 40 N m;
    robots 0 and 2 stay inside it (both asserted against the helper).  Robot 1 matches the helper, tau_last
    respects the bound exactly, robots 0 and 2 equal the run without the jump bit for bit."""
    cid, B, tmax, jump = "h24", 3, 40.0, 0.5
    r = ct_refs(cid, B)
    ref = ct_reference(cid, B, tau_max=tmax, jump=jump)
    assert [c for _, _, c in ref] == [False, True, False]
    jumped = dict(r, q_ref=r["q_ref"].copy())
    jumped["q_ref"][:, 1] += jump
    got, tau_last = full(handle, cid, B, jumped, tau_max=tmax)
    plain, tau_plain = full(handle, cid, B, r, tau_max=tmax)
    for k in native.FB_STATE_KEYS:
        e = FM.rel_err(got[k][1], ref[1][0][k])
        print("clamped robot", k, "rel err %.3g" % e)
        assert e <= TOL, (k, e)
    assert FM.rel_err(tau_last[1], ref[1][1]) <= TOL
    assert (np.abs(tau_last) <= tmax).all() and (np.abs(tau_last[1]) == tmax).any()
    assert_bitwise(got, plain, robots=[0, 2])
    np.testing.assert_array_equal(tau_last[[0, 2]], tau_plain[[0, 2]])
    # unclamped robots: tau_max changes nothing
    free, _ = full(handle, cid, B, r)
    assert_bitwise(plain, free)


@pytest.mark.parametrize("cid,B", [("h24", 3), ("n48", 2)])
def test_slices(handle, cid, B):
    """7: NaN in the slices past the last one used changes no bit; T identical slices equal T = 1."""
    r = ct_refs(cid, B)
    got4, tl4 = full(handle, cid, B, r)
    nan = lambda a: np.concatenate([a, np.full_like(a, np.nan)], axis=0)
    got8, tl8 = run_ct(handle, cid, B, nan(r["q_ref"]), nu=nan(r["nu"]), qdd=nan(r["qdd"]), q_bias=r["q_bias"])
    assert all(np.isfinite(v).all() for v in got4.values())
    assert_bitwise(got8, got4)
    np.testing.assert_array_equal(tl8, tl4)
    one = {k: r[k][:1] for k in ("q_ref", "nu", "qdd")}
    rep = {k: np.repeat(v, 3, axis=0) for k, v in one.items()}
    a, _ = run_ct(handle, cid, B, one["q_ref"], nu=one["nu"], qdd=one["qdd"], q_bias=r["q_bias"])
    b, _ = run_ct(handle, cid, B, rep["q_ref"], sps=4, nu=rep["nu"], qdd=rep["qdd"], q_bias=r["q_bias"])
    assert_bitwise(a, b)


def test_mass_reg_is_refused(handle):
    cid, B = "h24", 2
    cs, r = TC.build_case(cid), ct_refs(cid, 2)
    n = cs["model"]["n"]
    with pytest.raises(native.BlfError) as e:
        full(handle, cid, B, r, mass_reg=np.zeros((n + 6, n + 6)))
    assert e.value.code == UNSUPPORTED


@pytest.mark.parametrize("field", ["q_ref", "nu", "qdd", "q_bias"])
def test_nan_reference_is_per_robot(handle, field):
    """7: a NaN in robot 1's slice 2 gives robot 1 a NaN state; robots 0 and 2 keep the clean run's bits."""
    r = ct_refs("h24", 3)
    clean, tl = full(handle, "h24", 3, r)
    bad = {k: v.copy() for k, v in r.items()}
    if field == "q_bias":
        bad["q_bias"][1, 7] = np.nan
    else:
        bad[field][2, 1, 6 + 7 if field == "nu" else 7] = np.nan
    got, tl2 = full(handle, "h24", 3, bad)
    for k in native.FB_STATE_KEYS:
        assert np.isnan(got[k][1]).all(), k
    assert np.isnan(tl2[1]).all()
    assert_bitwise(got, clean, robots=[0, 2])
    np.testing.assert_array_equal(tl2[[0, 2]], tl[[0, 2]])
