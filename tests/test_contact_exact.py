"""The oracle's ContinuousContactModel against an exact quadrature of the model's point law.

tests/golden/contact_exact.npz (tests/golden/make_contact_exact.py) holds 80 contacts in eight
pose families with the wrench, autonomous dynamics, control matrix and regressor computed by
tests/contact_exact.py: the point law of ContinuousContactModel.cpp:173-221 integrated over the
sole by a 3 x 3 Gauss-Legendre rule (exact for it) in mpmath at 50 digits, rounded to double.
Unlike the reference's own three properties (tests/test_oracle_contact.py) this is a check from
outside the closed forms: a lost factor, a swapped axis or a wrong sign in any of them shows in the
first digit.

The bar is block_err <= 1e-14 (contact_exact.block_err: per force / torque block, relative to the
block's largest entry, exact zeros required where the truth is zero).  The oracle's worst figure on
these families, recorded in the fixture by the script that wrote it, is 1.4e-15."""
import os

import numpy as np
import pytest

import contact_exact as CE
import oracle as O

BAR = 1e-14
OUTPUTS = ("wrench", "autonomous", "control", "regressor")
PER_FAMILY = 10


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "contact_exact.npz"))
    return {k: z[k] for k in z.files}


def _args(fx, q):
    return fx["prm"][q], fx["twist"][q], fx["pose"][q], fx["null"][q]


def test_fixture_has_the_families_it_promises(fx):
    fam = list(fx["families"])
    assert fam == ["generic", "nonortho", "zero22", "tiny22", "stiff_far", "flat", "rest", "shared"]
    assert fx["prm"].shape == (80, 4) and fx["points"].shape == (16, 18, 2)
    r22 = fx["pose"][:, 11].reshape(8, PER_FAMILY)
    assert np.all(r22[fam.index("zero22")] == 0.0)
    assert np.all(np.abs(r22[fam.index("tiny22")]) == 1e-9)
    for name in ("generic", "nonortho", "tiny22", "stiff_far", "shared"):
        assert (r22[fam.index(name)] < 0).any() and (r22[fam.index(name)] > 0).any(), name
    q = fam.index("rest") * PER_FAMILY
    np.testing.assert_array_equal(fx["pose"][q:q + PER_FAMILY], fx["null"][q:q + PER_FAMILY])
    assert not fx["twist"][q:q + PER_FAMILY].any()
    for k in ("wrench", "autonomous", "regressor"):     # the control matrix does not vanish
        assert not fx[k][q:q + PER_FAMILY].any(), k
    # the script's gate: it does not write a fixture on which the oracle is worse than 2e-15
    assert fx["oracle_err"].shape == (8, 6) and fx["oracle_err"].max() <= 2e-15


def test_oracle_contact_eval_against_the_exact_quadrature(fx):
    worst = np.zeros((8, 4))
    for q in range(80):
        got = O.contact_eval(*_args(fx, q))
        for n, k in enumerate(OUTPUTS):
            worst[q // PER_FAMILY, n] = max(worst[q // PER_FAMILY, n],
                                            CE.block_err(got[n], fx[k][q]))
    print(f"\n{'':10s}" + "".join(f"{k:>12s}" for k in OUTPUTS))
    for i, name in enumerate(fx["families"]):
        print(f"{name:10s}" + "".join(f"{e:12.2e}" for e in worst[i]))
    assert worst.max() <= BAR, worst


def test_oracle_contact_point_against_the_exact_point_law(fx):
    worst = np.zeros((8, 2))
    for i, q in enumerate(fx["point_contact"]):
        for j, (x, y) in enumerate(fx["points"][i]):
            f, t = O.contact_point(*_args(fx, q), x, y)
            ef, et = fx["point_force"][i, j], fx["point_torque"][i, j]
            if CE.OUTSIDE.start <= j < CE.OUTSIDE.stop:
                assert not ef.any() and not et.any()
                assert not f.any() and not t.any(), (q, j)
            worst[q // PER_FAMILY, 0] = max(worst[q // PER_FAMILY, 0], CE.block_err(f, ef))
            worst[q // PER_FAMILY, 1] = max(worst[q // PER_FAMILY, 1], CE.block_err(t, et))
    print(f"\n{'':10s}{'point f':>12s}{'point t':>12s}")
    for i, name in enumerate(fx["families"]):
        print(f"{name:10s}" + "".join(f"{e:12.2e}" for e in worst[i]))
    assert worst.max() <= BAR, worst
    # the corners are inside (the rule is >): the law is not zero there except at rest
    rest = list(fx["families"]).index("rest")
    for i, q in enumerate(fx["point_contact"]):
        if q // PER_FAMILY != rest:
            assert fx["point_force"][i, CE.CORNERS].any(axis=1).all(), q


def test_fixture_is_current(fx):
    """Three contacts of each family (the two with points among them) recomputed at 50 digits:
    the file holds exactly what tests/contact_exact.py gives today."""
    pytest.importorskip("mpmath")
    for fam in range(8):
        for q in (fam * PER_FAMILY, fam * PER_FAMILY + 1, fam * PER_FAMILY + 9):
            a = _args(fx, q)
            for k, f in zip(OUTPUTS, (CE.wrench, CE.autonomous, CE.control, CE.regressor)):
                np.testing.assert_array_equal(CE.to_double(f(*a)), fx[k][q], err_msg=f"{k} {q}")
    for i, q in enumerate(fx["point_contact"]):
        a = _args(fx, q)
        np.testing.assert_array_equal(CE.fixture_points(a[0][0], a[0][1]), fx["points"][i])
        for j in (0, 1, 4, 5, 8, 9, 13, 17):
            x, y = fx["points"][i, j]
            np.testing.assert_array_equal(CE.to_double(CE.point_force(*a, x, y)),
                                          fx["point_force"][i, j])
            np.testing.assert_array_equal(CE.to_double(CE.point_torque(*a, x, y)),
                                          fx["point_torque"][i, j])


def test_contact_exact_agrees_with_itself(fx):
    """regressor @ (k, b) is the wrench and wrench == sign(R22) wrench_signed, to 1e-40 of the
    block at 50 digits."""
    mp = pytest.importorskip("mpmath")
    with mp.workdps(CE.DPS):
        for fam in range(8):
            for q in (fam * PER_FAMILY, fam * PER_FAMILY + 3):
                a = _args(fx, q)
                k, b = mp.mpf(float(a[0][2])), mp.mpf(float(a[0][3]))
                w, ws, reg = CE.wrench(*a), CE.wrench(*a, signed=True), CE.regressor(*a)
                sgn = mp.sign(mp.mpf(float(a[2][11])))
                for blk in (range(0, 3), range(3, 6)):
                    top = max(abs(w[i]) for i in blk)
                    for i in blk:
                        assert abs(reg[i][0] * k + reg[i][1] * b - w[i]) <= top * mp.mpf("1e-40")
                        assert abs(sgn * ws[i] - w[i]) <= top * mp.mpf("1e-40")


def test_block_err_demands_exact_zeros_and_finite_values():
    e = np.array([1.0, 2.0, -4.0, 0.0, 0.0, 0.0])
    assert CE.block_err(e, e) == 0.0
    assert CE.block_err(e + np.array([0, 0, 0, 0, 1e-300, 0]), e) == np.inf
    assert CE.block_err(e + np.array([0, 4e-15, 0, 0, 0, 0]), e) == pytest.approx(1e-15, rel=1e-2)
    g = e.copy()
    g[1] = np.nan
    assert CE.block_err(g, e) == np.inf
    c = np.zeros((6, 6))
    c[:3, :3] = np.diag([3.0, 3.0, 3.0])
    g = c.copy()
    g[0, 1] = 1e-30                                     # an off-diagonal of the top-left block
    assert CE.block_err(c, c) == 0.0 and CE.block_err(g, c) == np.inf
