"""Device tests of blf_swing_foot_eval / blf_so3_eval against the numpy restatement of
include/blf/blf_c.h section 11 (tests/swing_foot_reference.py).

Bit for bit: contact_idx, in_contact, every stance or held sample, every translational channel.
Rotation, omega and alpha: within 1e-9 * max(1, |x|) (device and numpy sin / atan2 differ in the
last bits).  The swing through exactly pi about z is excluded from the rotational comparison only
(the axis sign is arbitrary there) and checked by properties instead."""
import numpy as np
import pytest
import torch

import swing_foot_reference as S
from blf import problems as P

pytestmark = pytest.mark.gpu

PRM = dict(step_height=0.04, apex_ratio=0.4, landing_velocity=-0.05, landing_acceleration=0.3)
ROT_TOL = 1e-9
N_CASES = 6
PI_CASE = 5


def relative_rotation(k, rs, yaw):
    """Case k of the relative rotations: identical, 1e-10 rad, a workload yaw, a general axis at
    2 rad, pi - 1e-6, exactly pi about z (applied on the left of the previous contact's R)."""
    if k == 0:
        return np.eye(3)
    if k == 1:
        return S.axis_angle(rs.standard_normal(3), 1e-10)
    if k == 2:
        return S.rz(yaw)
    if k == 3:
        return S.axis_angle(rs.standard_normal(3), 2.0)
    if k == 4:
        return S.axis_angle(rs.standard_normal(3), np.pi - 1e-6)
    return np.diag([-1.0, -1.0, 1.0])   # rows 0 and 1 negated exactly: w == 0 in the quaternion


def make_lists(L, C, Q, seed, poison=False):
    """L lists of 1..C contacts; swing s of the batch uses rotation case s % 6.  Returns the
    tables, the queries and case [L, C - 1] (the rotation case of swing c -> c + 1)."""
    rs = np.random.RandomState(seed)
    cp = np.zeros((L, C, 12))
    ct = np.zeros((L, C, 2))
    nc = np.zeros(L, dtype=np.int32)
    case = np.full((L, max(C - 1, 1)), -1)
    tq = np.zeros((L, Q))
    k = 0
    for l in range(L):
        n = C - (l % C)
        nc[l] = n
        t = rs.uniform(-0.1, 0.1)
        p = np.array([0.0, 0.1 * (-1) ** l, 0.0])
        R = S.rz(rs.uniform(-0.1, 0.1)) if l % 2 else S.axis_angle(rs.standard_normal(3), 0.5)
        for c in range(C):            # padding contacts are filled too: they must not be read
            if c:
                R = relative_rotation(k % N_CASES, rs, rs.uniform(-0.2, 0.2)) @ R
                case[l, c - 1] = k % N_CASES
                k += 1 if c < n else 0     # the cases cycle over the real swings
                p = p + np.array([rs.uniform(0.2, 0.4), rs.uniform(-0.05, 0.05), rs.uniform(-0.03, 0.03)])
            cp[l, c, :3], cp[l, c, 3:] = p, R.reshape(9)
            ct[l, c, 0] = t
            t += rs.uniform(0.2, 0.5)
            ct[l, c, 1] = t
            t += rs.uniform(0.4, 0.7)
        a, d = ct[l, :n, 0], ct[l, :n, 1]
        rho = PRM["apex_ratio"]
        times = [a[0] - 0.1, d[-1] + 0.1]                       # before the first, after the last
        times += list(a) + list(d)                              # ties on every (de)activation
        times += list(0.5 * (a + d))                            # mid-stance
        times += list(0.5 * (d[:-1] + a[1:]))                   # mid-swing
        times += list((1.0 - rho) * d[:-1] + rho * a[1:])       # the apex knot
        times += list(a[1:] - 1e-9)                             # just before landing
        assert len(times) <= Q
        times += list(rs.uniform(a[0] - 0.2, d[-1] + 0.2, Q - len(times)))
        tq[l] = times
    if poison:
        assert L >= 9
        nc[2] = 0
        nc[5] = C + 1
        cp[7, 0, 4] = np.nan
        nc[7] = max(nc[7], 1)
    return cp, ct, nc, tq, case


def device_eval(handle, cp, ct, nc, tq, offset=False):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    L, Q = tq.shape
    out = None
    if offset:
        # every output 8 B past a 16-B boundary: the slab stores' 8-B path
        shapes = dict(pose=(L, Q, 12), twist=(L, Q, 6), accel=(L, Q, 6), contact_idx=(L, Q),
                      in_contact=(L, Q))
        out = {}
        for k, sh in shapes.items():
            if k in ("contact_idx", "in_contact"):
                buf = torch.full((L * Q + 4,), -7, dtype=torch.int32, device="cuda")
                out[k] = buf[2:2 + L * Q].view(sh)
            else:
                n = int(np.prod(sh))
                buf = torch.full((n + 2,), -7.0, dtype=torch.float64, device="cuda")
                out[k] = buf[1:1 + n].view(sh)
            assert out[k].data_ptr() % 16 == 8
    r = handle.swing_foot_eval(dev(cp), dev(ct), dev(nc), dev(tq), out=out, **PRM)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def rot_dev(dev, ref):
    """Largest |dev - ref| / max(1, |ref|)."""
    if dev.size == 0:
        return 0.0
    return float((np.abs(dev - ref) / np.maximum(1.0, np.abs(ref))).max())


def check_against_reference(dev, cp, ct, nc, tq, case):
    ref = S.swing_foot_eval(cp, ct, nc, tq, **PRM)
    np.testing.assert_array_equal(dev["contact_idx"], ref["contact_idx"])
    np.testing.assert_array_equal(dev["in_contact"], ref["in_contact"])
    sw = ref["swing"]
    for k in ("pose", "twist", "accel"):
        np.testing.assert_array_equal(dev[k][~sw], ref[k][~sw])           # stance, held, poisoned
        np.testing.assert_array_equal(dev[k][sw][:, :3], ref[k][sw][:, :3])   # translation
    # the rotation case of each swing query
    qcase = np.full(sw.shape, -1)
    ls, qs = np.nonzero(sw)
    qcase[ls, qs] = case[ls, ref["contact_idx"][ls, qs]]
    assert (qcase[sw] >= 0).all()
    cmp_ = sw & (qcase != PI_CASE)
    hold = sw & (qcase == 0)
    assert cmp_.sum() + (sw & (qcase == PI_CASE)).sum() == sw.sum()
    worst = {k: rot_dev(dev[k][cmp_][:, 3:], ref[k][cmp_][:, 3:]) for k in ("pose", "twist", "accel")}
    print("worst rotational deviation (relative to max(1, |x|)):", worst,
          "swing queries compared:", int(cmp_.sum()), "cases present:", sorted(set(qcase[sw])))
    for k, w in worst.items():
        assert w <= ROT_TOL, (k, w)
    # identical rotations: R_raw bit for bit, no angular motion
    np.testing.assert_array_equal(dev["pose"][hold][:, 3:], ref["pose"][hold][:, 3:])
    assert not dev["twist"][hold][:, 3:].any() and not dev["accel"][hold][:, 3:].any()
    return ref, qcase


def check_pi_case(dev, cp, ct, ref, qcase, tq):
    """The swing through exactly pi: orthonormal everywhere, finite rates, and the landing pose is
    reached (Log then Exp: a chain of some 60 rounded operations, bounded at 1e-13)."""
    m = ref["swing"] & (qcase == PI_CASE)
    if not m.any():
        return 0
    R = dev["pose"][m][:, 3:].reshape(-1, 3, 3)
    np.testing.assert_allclose(R @ np.swapaxes(R, 1, 2), np.broadcast_to(np.eye(3), R.shape),
                               rtol=0, atol=1e-14)
    assert np.isfinite(dev["twist"][m]).all() and np.isfinite(dev["accel"][m]).all()
    reached = 0
    for l, q in zip(*np.nonzero(m)):
        c = ref["contact_idx"][l, q]
        if tq[l, q] == ct[l, c + 1, 0] - 1e-9:      # the query just before landing
            np.testing.assert_allclose(dev["pose"][l, q, 3:], cp[l, c + 1, 3:], rtol=0, atol=1e-13)
            reached += 1
    return reached


@pytest.mark.parametrize("L,C,Q,offset", [(3, 4, 37, False), (9, 5, 61, False), (3, 4, 37, True),
                                          (40, 3, 2, False), (2, 1, 5, False)],
                         ids=["one_partial_tile", "three_tiles", "outputs_offset_8B",
                              "every_lane_fits", "one_contact"])
def test_swing_foot_eval_matches_the_reference(handle, L, C, Q, offset):
    if Q >= 30:
        cp, ct, nc, tq, case = make_lists(L, C, Q, seed=100 + L, poison=L >= 9)
    else:
        # too few queries per list for the full set: take each list's first Q of a longer draw
        # (C = 3: before, after, two activations...; the tiles span > 36 lists, so every lane fits
        # its own segment instead of reading a staged record)
        cp, ct, nc, tq, case = make_lists(L, C, 30, seed=100 + L, poison=L >= 9)
        rs = np.random.RandomState(L)
        tq = np.stack([rs.permutation(row)[:Q] for row in tq])
    dev = device_eval(handle, cp, ct, nc, tq, offset)
    ref, qcase = check_against_reference(dev, cp, ct, nc, tq, case)
    reached = check_pi_case(dev, cp, ct, ref, qcase, tq)
    if Q >= 30 and C >= 4:
        assert set(qcase[ref["swing"]]) == set(range(N_CASES))     # every rotation case was queried
        assert reached >= 1
        assert len(set(nc)) >= min(L, C)                           # the contact counts vary
    if L >= 9:
        for l in (2, 5, 7):
            assert np.isnan(dev["pose"][l]).all() and np.isnan(dev["twist"][l]).all()
            assert np.isnan(dev["accel"][l]).all()
            assert (dev["contact_idx"][l] == -1).all() and (dev["in_contact"][l] == 0).all()
        for l in (1, 3, 4, 6, 8):
            assert np.isfinite(dev["pose"][l]).all()


def test_optional_outputs_are_skipped(handle):
    cp, ct, nc, tq, _ = make_lists(3, 4, 37, seed=103)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    full = handle.swing_foot_eval(dev(cp), dev(ct), dev(nc), dev(tq), **PRM)
    for keep in (("pose",), ("twist",), ("accel", "in_contact"), ("contact_idx",)):
        part = handle.swing_foot_eval(dev(cp), dev(ct), dev(nc), dev(tq), outputs=keep, **PRM)
        assert set(part) == set(keep)
        for k in keep:
            assert torch.equal(part[k], full[k])


def test_swing_translation_is_the_quintic_spline_path(handle):
    """The workload's feet: positions, velocities and accelerations equal blf_quintic_fit ->
    blf_quintic_eval on problems.swing_splines bit for bit; the rotation is Rz(psi0 + s dpsi)."""
    B, QS = 8, 32
    prob = P.make_batch(B, horizon=100, n_footsteps=6)
    tabs = P.foot_contact_tables(prob)
    kt, kp, tqs = P.swing_splines(prob, apex_height=0.05, queries=QS)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    coeffs = handle.quintic_fit(dev(kt), dev(kp))
    pva, _ = handle.quintic_eval(dev(kt), coeffs, dev(tqs))
    pva = pva.cpu().numpy()                       # [S, Q, 3 (p, v, a), 3]
    row, worst, compared = 0, 0.0, 0
    for foot in ("left", "right"):
        tab, lst = tabs[foot], prob["schedule"][foot]
        nsw = len(lst) - 1
        tq = np.concatenate([tqs[row + i * B: row + (i + 1) * B] for i in range(nsw)], axis=1)
        r = handle.swing_foot_eval(dev(tab["contact_pose"]), dev(tab["contact_time"]),
                                   dev(tab["ncontacts"]), dev(tq), step_height=0.05, apex_ratio=0.5)
        r = {k: v.cpu().numpy() for k, v in r.items()}
        for i in range(nsw):
            sl = slice(i * QS, (i + 1) * QS)
            t0, t1 = tab["contact_time"][:, i, 1], tab["contact_time"][:, i + 1, 0]
            swing = tq[:, sl] < t1[:, None]      # the last query is the landing instant: stance
            assert swing[:, :-1].all() and not swing[:, -1].any()
            assert (r["in_contact"][:, sl][swing] == 0).all() and (r["contact_idx"][:, sl][swing] == i).all()
            assert (r["in_contact"][:, sl][~swing] == 1).all()
            ref = pva[row + i * B: row + (i + 1) * B]
            np.testing.assert_array_equal(r["pose"][:, sl, :3][swing], ref[:, :, 0][swing])
            np.testing.assert_array_equal(r["twist"][:, sl, :3][swing], ref[:, :, 1][swing])
            np.testing.assert_array_equal(r["accel"][:, sl, :3][swing], ref[:, :, 2][swing])
            psi0, psi1 = prob["poses"][:, lst[i][2], 2], prob["poses"][:, lst[i + 1][2], 2]
            T = (t1 - t0)[:, None]
            s, sd, _ = S.min_jerk((tq[:, sl] - t0[:, None]) / T, T)
            Rz = S.rz(psi0[:, None] + s * (psi1 - psi0)[:, None]).reshape(B, QS, 9)
            worst = max(worst, rot_dev(r["pose"][:, sl, 3:][swing], Rz[swing]),
                        rot_dev(r["twist"][:, sl, 5][swing], (sd * (psi1 - psi0)[:, None])[swing]))
            compared += int(swing.sum())
        row += nsw * B
    assert row == kt.shape[0] and compared > 0
    print("worst deviation from the Rz closed form:", worst, "over", compared, "swing queries")
    assert worst <= ROT_TOL


def so3_set(seed=11):
    rs = np.random.RandomState(seed)
    R0 = np.stack([S.axis_angle(rs.standard_normal(3), 0.6) if k != 2 else S.rz(0.07)
                   for k in range(5)])
    R1 = np.stack([relative_rotation(k, rs, -0.15) @ R0[k] for k in range(5)])
    return R0, R1, np.array([0.6, 1.0, 0.6, 2.5, 0.3])


def test_so3_eval_matches_the_reference_and_clamps(handle):
    Sn, Q = 5, 33
    R0, R1, dur = so3_set()
    tq = np.stack([np.concatenate([[-0.5, -1e-9, 0.0, T, T + 1e-9, T + 3.0],
                                   np.linspace(0.0, T, Q - 6)]) for T in dur])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    r = handle.so3_eval(dev(R0), dev(R1), dev(dur), dev(tq))
    r = {k: v.cpu().numpy() for k, v in r.items()}
    ref = S.so3_eval(R0, R1, dur, tq)
    worst = {k: rot_dev(r[k], ref[k]) for k in ("rot", "omega", "alpha")}
    print("worst deviation (relative to max(1, |x|)):", worst)
    for k, w in worst.items():
        assert w <= ROT_TOL, (k, w)
    # clamped: before 0 the start rotation bit for bit, after the duration the value at it
    for k in ("rot", "omega", "alpha"):
        np.testing.assert_array_equal(r[k][:, 0], r[k][:, 2])
        np.testing.assert_array_equal(r[k][:, 1], r[k][:, 2])
        np.testing.assert_array_equal(r[k][:, 4], r[k][:, 3])
        np.testing.assert_array_equal(r[k][:, 5], r[k][:, 3])
    np.testing.assert_array_equal(r["rot"][:, 2], R0.reshape(5, 9))
    np.testing.assert_array_equal(r["rot"][0], np.broadcast_to(R0[0].reshape(9), (Q, 9)))   # identical
    assert not r["omega"][:, [0, 1, 2, 3, 4, 5]].any()
    # only some outputs
    part = handle.so3_eval(dev(R0), dev(R1), dev(dur), dev(tq), outputs=("omega",))
    assert set(part) == {"omega"} and np.array_equal(part["omega"].cpu().numpy(), r["omega"])


def test_so3_eval_through_exactly_pi_and_poisoned_trajectories(handle):
    R0 = np.stack([np.eye(3), np.eye(3), np.eye(3)])
    R1 = np.stack([np.diag([-1.0, -1.0, 1.0]), S.rz(0.3), S.rz(0.3)])
    dur = np.array([1.0, 0.0, 1.0])                   # trajectory 1: no duration -> NaN
    tq = np.tile(np.linspace(0.0, 1.0, 9), (3, 1))
    tq[2, 4] = np.nan                                 # one poisoned query
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    r = {k: v.cpu().numpy() for k, v in handle.so3_eval(dev(R0), dev(R1), dev(dur), dev(tq)).items()}
    R = r["rot"][0].reshape(-1, 3, 3)
    np.testing.assert_allclose(R @ np.swapaxes(R, 1, 2), np.broadcast_to(np.eye(3), R.shape),
                               rtol=0, atol=1e-14)
    np.testing.assert_allclose(R[-1], R1[0], rtol=0, atol=1e-13)
    np.testing.assert_allclose(np.abs(r["omega"][0, 4]), [0.0, 0.0, 1.875 * np.pi], rtol=0, atol=1e-12)
    assert all(np.isnan(r[k][1]).all() for k in r)
    assert all(np.isnan(r[k][2, 4]).all() for k in r)
    ref = S.so3_eval(R0, R1, dur, tq)
    keep = [0, 1, 2, 3, 5, 6, 7, 8]
    for k in r:
        assert rot_dev(r[k][2, keep], ref[k][2, keep]) <= ROT_TOL
