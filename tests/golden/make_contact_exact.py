"""Generates tests/golden/contact_exact.npz: inputs of ContinuousContactModel and its outputs
computed exactly, by tests/contact_exact.py (the 3 x 3 Gauss-Legendre quadrature of the point law
in mpmath at 50 digits, which integrates that law without error), rounded to the nearest double.
tests/test_contact_exact.py holds the oracle to it, tests/test_gpu_contact_exact.py the device;
neither of the GPU tests needs mpmath.

Eight families of 10 contacts, 80 in all, in this order (one launch crosses the 64-lane tile edge
inside `rest`):

  generic    random SO(3) pose and null pose, every third pose flipped by diag(1, -1, -1) so that
             R22 < 0; positions N(0, 0.02), twist U(-1, 1), L in [0.08, 0.2], W in [0.05, 0.12],
             k in [500, 5000], b in [10, 300] (the ranges of test_gpu_contact.contact_batch)
  nonortho   the same with 1e-3 N(0, 1) added to every entry of both rotations (what the Euler
             integration of the base really hands to the model)
  zero22     R = Rz(theta) Rx(+-pi/2) built from exact 0 / +-1 entries: R[2, 2] == 0.0, a sole on edge
  tiny22     the same with R[2, 2] = +-1e-9
  stiff_far  k = 2e6, b = 2e3, both positions offset by (8192, -4096, 0): the closed loop's soles
  flat       a tilt of 1e-3 rad about a horizontal axis over an identity null rotation, the twist
             and the offset from the null position scaled by 1e-2: a sole about to come to rest.
             (The torque is O(1e-3) of the generic one here.  The offset is scaled with the twist
             because the lever-times-force terms of the point torques, which cancel in the
             integral, grow with both; with a generic 2 cm offset they are 1e3 times the
             integral, and no sum of double-precision point torques can then reproduce the
             wrench to 1e-14, whatever the kernel does.)
  rest       pose equal to the null pose, zero twist: every output is exactly zero
  shared     the reference test's parameters (0.12, 0.09, 2000, 100) on generic poses

For the first two contacts of each family (16 contacts) the point law itself is stored at the 18
points of contact_exact.fixture_points: the centre, the four corners, one nextafter outside each
edge (exact zeros) and the nine Gauss nodes.

The script evaluates the oracle on every contact and point, prints its worst block-relative error
per family and output, refuses to write the file if any exceeds 2e-15, and stores those figures
(`oracle_err`, families x (wrench, autonomous, control, regressor, point force, point torque)).
The archive is written with fixed time stamps, so a second run reproduces it byte for byte.

    python tests/golden/make_contact_exact.py
"""
import io
import os
import sys
import zipfile

import numpy as np
from scipy.spatial.transform import Rotation as Rot

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import contact_exact as CE  # noqa: E402

FAMILIES = ("generic", "nonortho", "zero22", "tiny22", "stiff_far", "flat", "rest", "shared")
PER_FAMILY = 10
OUTPUTS = ("wrench", "autonomous", "control", "regressor")
SEED = 20201
GATE = 2e-15


def _generic(seed, B=PER_FAMILY):
    rng = np.random.default_rng(seed)
    R = Rot.random(B, random_state=seed).as_matrix()
    R[::3] = R[::3] @ np.diag([1.0, -1.0, -1.0])
    R0 = Rot.random(B, random_state=seed + 1).as_matrix()
    p, p0 = rng.normal(size=(B, 3)) * 0.02, rng.normal(size=(B, 3)) * 0.02
    twist = rng.uniform(-1, 1, (B, 6))
    prm = np.stack([rng.uniform(0.08, 0.2, B), rng.uniform(0.05, 0.12, B),
                    rng.uniform(500, 5000, B), rng.uniform(10, 300, B)], axis=1)
    return prm, twist, p, R, p0, R0


def _on_edge(seed, r22):
    prm, twist, p, R, p0, R0 = _generic(seed)
    rng = np.random.default_rng(seed + 2)
    for q in range(PER_FAMILY):
        th = rng.uniform(-np.pi, np.pi)
        c, s = np.cos(th), np.sin(th)
        sg = 1.0 if q % 2 == 0 else -1.0
        Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        Rx = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -sg], [0.0, sg, 0.0]])
        R[q] = Rz @ Rx
        assert R[q, 2, 2] == 0.0 and abs(R[q, 2, 1]) == 1.0
        R[q, 2, 2] = sg * r22 if q % 4 < 2 else -sg * r22
    return prm, twist, p, R, p0, R0


def family(name, seed):
    """(prm, twist, pose, null) of one family, [10, 4 | 6 | 12 | 12]."""
    prm, twist, p, R, p0, R0 = _generic(seed)
    rng = np.random.default_rng(seed + 3)
    if name == "nonortho":
        R = R + 1e-3 * rng.normal(size=R.shape)
        R0 = R0 + 1e-3 * rng.normal(size=R0.shape)
    elif name == "zero22":
        prm, twist, p, R, p0, R0 = _on_edge(seed, 0.0)
        assert np.all(R[:, 2, 2] == 0.0)
    elif name == "tiny22":
        prm, twist, p, R, p0, R0 = _on_edge(seed, 1e-9)
        assert np.all(np.abs(R[:, 2, 2]) == 1e-9) and len(set(np.sign(R[:, 2, 2]))) == 2
    elif name == "stiff_far":
        prm[:, 2], prm[:, 3] = 2e6, 2e3
        off = np.array([8192.0, -4096.0, 0.0])
        p, p0 = p + off, p0 + off
    elif name == "flat":
        ang = rng.uniform(-np.pi, np.pi, PER_FAMILY)
        axis = np.stack([np.cos(ang), np.sin(ang), np.zeros(PER_FAMILY)], axis=1)
        R = Rot.from_rotvec(1e-3 * axis).as_matrix()
        R0 = np.broadcast_to(np.eye(3), R.shape).copy()
        twist = twist * 1e-2
        p = p0 + (p - p0) * 1e-2
    elif name == "rest":
        p, R = p0.copy(), R0.copy()
        twist = np.zeros_like(twist)
    elif name == "shared":
        prm = np.broadcast_to(np.array([0.12, 0.09, 2000.0, 100.0]), prm.shape).copy()
    else:
        assert name == "generic"
    pose = np.concatenate([p, R.reshape(-1, 9)], axis=1)
    null = np.concatenate([p0, R0.reshape(-1, 9)], axis=1)
    return prm, twist, pose, null


def inputs():
    parts = [family(name, SEED + 10 * i) for i, name in enumerate(FAMILIES)]
    return [np.ascontiguousarray(np.concatenate([f[j] for f in parts])) for j in range(4)]


def exact_contact(prm, twist, pose, null, extended=False):
    a = (prm, twist, pose, null)
    return [CE.to_double(f(*a), extended) for f in
            (CE.wrench, CE.autonomous, CE.control, CE.regressor)]


def exact_points(prm, twist, pose, null, pts, extended=False):
    a = (prm, twist, pose, null)
    f = np.stack([CE.to_double(CE.point_force(*a, x, y), extended) for x, y in pts])
    t = np.stack([CE.to_double(CE.point_torque(*a, x, y), extended) for x, y in pts])
    return f, t


def write_npz(path, arrays):
    """np.load-compatible archive with fixed member time stamps (reproducible bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    import oracle as O
    prm, twist, pose, null = inputs()
    B = len(FAMILIES) * PER_FAMILY
    exact = [np.zeros((B, 6)), np.zeros((B, 6)), np.zeros((B, 6, 6)), np.zeros((B, 6, 2))]
    point_contact = np.array([PER_FAMILY * i + j for i in range(len(FAMILIES)) for j in (0, 1)])
    points = np.stack([CE.fixture_points(prm[q, 0], prm[q, 1]) for q in point_contact])
    pf, pt = np.zeros(points.shape[:2] + (3,)), np.zeros(points.shape[:2] + (3,))
    err = np.zeros((len(FAMILIES), 6))
    for q in range(B):
        a = (prm[q], twist[q], pose[q], null[q])
        ext = exact_contact(*a, extended=True)
        got = O.contact_eval(*a)
        for n in range(4):
            exact[n][q] = ext[n].astype(np.float64)
            err[q // PER_FAMILY, n] = max(err[q // PER_FAMILY, n], CE.block_err(got[n], ext[n]))
    for i, q in enumerate(point_contact):
        a = (prm[q], twist[q], pose[q], null[q])
        ef, et = exact_points(*a, points[i], extended=True)
        pf[i], pt[i] = ef.astype(np.float64), et.astype(np.float64)
        assert not pf[i, CE.OUTSIDE].any() and not pt[i, CE.OUTSIDE].any()
        for j, (x, y) in enumerate(points[i]):
            f, t = O.contact_point(*a, x, y)
            fam = q // PER_FAMILY
            err[fam, 4] = max(err[fam, 4], CE.block_err(f, ef[j]))
            err[fam, 5] = max(err[fam, 5], CE.block_err(t, et[j]))
    print("oracle, worst block-relative error against the exact quadrature")
    print(f"{'':10s}" + "".join(f"{n:>12s}" for n in OUTPUTS + ("point f", "point t")))
    for i, name in enumerate(FAMILIES):
        print(f"{name:10s}" + "".join(f"{e:12.2e}" for e in err[i]))
    assert np.all(err <= GATE), f"the oracle misses the exact value by more than {GATE}: not written"
    out = os.path.join(HERE, "contact_exact.npz")
    write_npz(out, dict(families=np.array(FAMILIES), prm=prm, twist=twist, pose=pose, null=null,
                        wrench=exact[0], autonomous=exact[1], control=exact[2],
                        regressor=exact[3], point_contact=point_contact, points=points,
                        point_force=pf, point_torque=pt, oracle_err=err))
    print(f"wrote {out}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
