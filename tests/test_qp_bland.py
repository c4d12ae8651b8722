"""The anti-cycling passes of the active-set QP kernels on the oracle (oracle
dcm_polish, the `bland && !ok` block; kernel as_passes in csrc/dcm_mpc_as.hip): from fp64 pass index
8 on, a failed pass changes ONE facet, at the lowest knot whose sets the certificate changed, the
lowest-index facet it dropped, else the lowest-index facet it added.

tests/golden/qp_bland_windows.npz (made by tests/golden/make_qp_bland_windows.py; read through
tests/qp_bland.py) holds, per instance of the kernels, QPs that reach the rule: "Bland rows", oracle
status 0 and at least 10 fp64 passes (passes64 of orc_dcm_mpc_solve_warm64; a QP that certifies at
its 9th pass never applies a Bland move).  This module checks the fixture's preconditions on the
oracle and the certified rows against an independent dense KKT solve;
tests/test_gpu_qp_bland.py compares the device with the oracle on the same rows bit for bit.

The generator's table (Bland rows of the source; rows kept; their fp64 passes 10/11/12; rows the
active-set passes certify / rows handed to the interior point method; genuinely warm rows):

  instance   Bland rows  kept   fp64 passes 10/11/12  certified/IPM  warm
  m8_n50             99    64                11/7/46     26 / 38       16
  m8_n64            114    64                 1/2/61      3 / 61       16
  m8_n65            115    64                 2/2/60      5 / 59       16
  m8_n100           122    64                 0/0/64      1 / 63        9
  m8_n64w           413    64               20/15/29     48 / 16        0
  m8_n65w           413    64               18/16/30     48 / 16        0
  m8_n100w          450    64               18/14/32     48 / 16        0
  m8_n127           441    64               18/14/32     48 / 16        0
  m8_n128           448    64               17/16/31     48 / 16        0
  m16_n50            19    19                 3/0/16     14 / 5         0
  m16_n64            19    19                 3/1/15     18 / 1         0
  m16_n100           51    51                17/5/29     32 / 19        0
  m16_n128           32    32                17/4/11     32 / 0         0
  m16_n100w         267    64                28/8/28     48 / 16        0
  m16_n128w          88    64               40/11/13     64 / 0         0

Sources: m8_n50 .. m8_n100 are c5_hard_windows.npz truncated to N knots; m8_n64w .. m8_n128 two-foot
walking plans with the initial DCM moved off the plan; m16_* three-contact plans (m16_n100w and
m16_n128w: a wider initial DCM offset).  No instance is empty.  Genuinely warm rows (certified by the warm kernel's own passes, at least 10 of them) exist
for the c5 instances only: the plan sources were searched as receding horizons (windows 1 .. 7,
each warm-started from the one before, whole sources) and every window certifies in fewer than 9
warm passes.  m16_n128 and m16_n128w have no handed-over Bland row: the rows of their sources that go
to the interior point method after more than 8 passes (7 in m16_n128's) all end with status 1 or 2
(VERDICT's open robustness item) and are left out.

Mutation record (not committed code).  In a scratch build of the oracle the Bland block was mutated:
(1) the HIGHEST changed knot, (2) the HIGHEST facet bit, (3) within the knot pair (2l, 2l + 1) of the
lowest changed lane the ODD knot first, and, for the knot-pair kernels, (4) the HIGHEST changed lane
(its lowest knot): what a wrong lane vote over the ballot would give.  Fixture rows that change an
asserted output (status, iters, xi, vrp, lam, polished or passes), as the GPU tests launch them (the
two scan trees of the horizons <= 64 give the same counts):

  rows                  (1)  (2)  (3)  (4)
  m8_n50     cold 64      9    3    4
  m8_n50     warm 16      1    0    0
  m8_n64     cold 64      0    0    0
  m8_n64     warm 16      1    0    0
  m8_n64w    cold 64     11    1    4
  m8_n65     cold 64      0    0    0    0
  m8_n65     warm 16      3    1    2    3
  m8_n65w    cold 64     12    1    4   15
  m8_n100    cold 64      0    0    0    0
  m8_n100    warm  9      1    0    1    1
  m8_n100w   cold 64      6    2    3    8
  m8_n127    cold 64      8    2    4   10
  m8_n128    cold 64     10    3    7   11
  m16_n50    cold 19     15   15   15
  m16_n64    cold 19     14   14   14
  m16_n100   cold 51      2   10    2    0
  m16_n100w  cold 64      2    8    0    2
  m16_n128   cold 32      2    6    2    0
  m16_n128w  cold 64      3    7    1    3

The cold rows of the c5 truncations at N = 64, 65 and 100 are blind to every mutant: all but 3, 5
and 1 of them fail their 12th pass and go to the interior point method, which restores the start
point and discards the Bland moves.  The walking-plan instances m8_n64w, m8_n65w and m8_n100w are
there for that reason, and m16_n100w / m16_n128w because the rows of m16_n100 / m16_n128 that see
mutant (1) have both changed knots in one lane, so they are blind to (4).  With them every kernel
instance (M, N) has rows that see each of the mutants (1), (2) and (3), and every knot-pair
instance rows that see (4).  The same was tried on the device: a build of the
kernels that votes for the highest set bit of the ballot (mutant (4); mutant (1) with one knot per
lane) fails tests/test_gpu_qp_bland.py at every (M, N), and one that keeps the lane's highest
changed slot fails it at every knot-pair (M, N) (N > 64; one knot per lane has no second slot).
"""
import numpy as np
import pytest

import dense_qp
import oracle as O
import qp_bland as QB

BAR = 1e-9   # the project's fp64 trajectory tolerance (test_c5_windows.BAR), absolute
# the instances the kernels' dispatch has (launch_kpl): every one must have rows
REQUIRED = ("m8_n50", "m8_n64", "m8_n65", "m8_n100", "m8_n127", "m8_n128",
            "m16_n50", "m16_n64", "m16_n100", "m16_n128")


instances, cold, warm = QB.instances, QB.cold, QB.warm


def names():
    return list(instances())


def test_every_instance_has_rows():
    inst = instances()
    for name in REQUIRED:
        assert name in inst and inst[name].n >= 3, name
    assert inst["m8_n100"].kind == "c5" and len(inst["m8_n100"].warm_rows) >= 3
    for M in (8, 16):   # both outcomes at each M: certified by the active-set passes / handed over
        both = [I.name for I in inst.values() if I.M == M and I.certified.any() and not I.certified.all()]
        assert both, M
    for I in inst.values():
        assert I.n <= 64 and len(I.warm_rows) <= 64


@pytest.mark.parametrize("name", names())
def test_cold_rows_reach_the_rule(name):
    """Every stored cold row: oracle status 0 and at least 10 fp64 passes, under the scan tree of
    each launch the GPU test makes; the outcome and pass count the fixture records."""
    I = instances()[name]
    assert I.n <= O.DPP_TREE_MAX_BATCH
    for db in QB.launch_batches(I):
        _, _, r = cold(name, db)
        assert (r["status"] == 0).all(), (db, np.nonzero(r["status"])[0])
        assert (r["passes64"] >= QB.BLAND_PASSES64).all(), (db, r["passes64"])
        assert (r["passes"] > r["passes64"]).all()   # the fp32 search ran too: passes > 8 + 1 on the device
        np.testing.assert_array_equal(r["iters"] == 0, I.certified)
        assert r["polished"].all()
    np.testing.assert_array_equal(cold(name, I.n)[2]["passes64"], I.passes64)


@pytest.mark.parametrize("name", [n for n in names() if len(instances()[n].warm_rows)])
def test_warm_rows_reach_the_rule(name):
    """The genuinely warm rows: certified by the warm passes themselves (no cold re-solve: the
    reported passes are the fp64 passes), at least 10 of them."""
    I, prob, v, l, ps, r = warm(name)
    assert (ps == 0).all()
    assert (r["status"] == 0).all() and (r["iters"] == 0).all() and r["polished"].all()
    np.testing.assert_array_equal(r["passes"], r["passes64"])
    assert (r["passes64"] >= QB.BLAND_PASSES64).all(), r["passes64"]
    check_optima(I, prob, r, np.arange(len(ps)))


def check_optima(I, prob, r, rows):
    """Rows `rows` of the oracle's result r against the dense KKT solve of the oracle's active set
    (tests/dense_qp.py: LU with extended-precision refinement), the row's own dt."""
    worst = 0.0
    for i in rows:
        x, v, ll, _ = dense_qp.kkt_solve(prob, i, r["lam"][i] > 0, dt=I.dt)
        ex, ev = np.abs(r["xi"][i] - x).max(), np.abs(r["vrp"][i] - v).max()
        worst = max(worst, ex, ev)
        assert ex <= BAR and ev <= BAR, (I.name, i, ex, ev)
        if len(ll):
            assert ll.min() >= -1e-9 * max(1.0, np.abs(ll).max()), (I.name, i, ll.min())
    print(f"{I.name}: {len(rows)} rows, worst |xi|, |vrp| error {worst:.2e}")


@pytest.mark.parametrize("name", names())
def test_certified_rows_vs_dense_kkt(name):
    """Independent optimum: every row the active-set passes certify (after Bland moves) is the
    optimum of the dense KKT system on its active set to 1e-9, with nonnegative multipliers."""
    I, prob, r = cold(name, instances()[name].n)
    check_optima(I, prob, r, np.nonzero(r["iters"] == 0)[0])
    if I.N <= 64:   # the other tree's optimum is a different rounding of the same point
        _, _, r2 = cold(name, 1025)
        check_optima(I, prob, r2, np.nonzero(r2["iters"] == 0)[0][:4])


@pytest.mark.parametrize("name", names())
def test_previous_status_starts_cold(name):
    """A warm start whose previous status is nonzero is solved as a cold start (what the GPU test of
    the warm kernels' cold path compares against)."""
    I, prob, r = cold(name, instances()[name].n)
    rw = QB.solve(prob, I.params(O), I.n, warm=(np.zeros((I.n, I.N, 2)), np.zeros((I.n, I.N, I.M))),
                  prev_status=np.ones(I.n, np.int32))
    for k in QB.OUT_KEYS + ("lam", "passes64"):
        np.testing.assert_array_equal(rw[k], r[k], err_msg=k)


def test_passes64_is_optional_and_changes_nothing():
    """passes64 is an extra output: the other outputs are the same bits with and without it, and
    a cold solve's passes are its fp32 search's plus passes64."""
    I, prob, r = cold("m16_n50", instances()["m16_n50"].n)
    pas = np.zeros(I.n, np.int32)
    st, xi, vrp, it, lam = O.dcm_mpc_solve_batch_warm(prob, params=I.params(O), threads=2, passes=pas,
                                                      device_batch=I.n)
    for k, v in (("status", st), ("xi", xi), ("vrp", vrp), ("iters", it), ("lam", lam), ("passes", pas)):
        np.testing.assert_array_equal(r[k], v, err_msg=k)
    assert ((r["passes"] - r["passes64"] >= 1) & (r["passes"] - r["passes64"] <= 8)).all()
