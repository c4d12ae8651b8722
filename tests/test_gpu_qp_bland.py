"""The anti-cycling passes of the active-set QP kernels on the device (csrc/dcm_mpc_as.hip,
as_passes: from fp64 pass index 8 on Bland's rule, one facet change per pass at the lowest knot the
certificate changed -- a ballot and count-trailing-zeros over the lanes, and the first changed slot
of the lane in the knot-pair kernels) against the oracle's plain loop over knots (dcm_polish), bit
for bit, on the rows of tests/golden/qp_bland_windows.npz: QPs that run at least 10 fp64 passes
(tests/test_qp_bland.py has the fixture's table, the oracle-side preconditions, the dense KKT check
of the certified rows and the mutation record of the rule).

Per instance m<M>_n<N> of launch_kpl (8 | 16 facet slots; N <= 64 one knot per lane, DPP tree up to
1024 QPs else Kogge-Stone; N <= 126 knot pairs with the pad tree, N = 127, 128 Kogge-Stone):
  * the cold per-knot solve with and without lambda_out (M = 8, N <= 64: the fused kernel);
  * N <= 64: the rows tiled to 1025 QPs (the Kogge-Stone tree), the precondition asserted again;
  * M = 8, N <= 64: the fused kernel and the two launches (fuse_stage2 = 1 | 0);
  * plan instances: blf_dcm_mpc_solve_phased on the rows' phase tables;
  * the warm kernel on the same rows with prev_status = 1 (they start cold inside the warm kernel);
  * the c5 instances: the genuinely warm rows (certified by at least 10 warm passes).
Every launch is compared on status, iters, xi, vrp, polished, passes (and lam where requested), and
every compared cold row ran more than 8 + 1 passes."""
import numpy as np
import pytest
import torch

import oracle as O
import qp_bland as QB
from blf import native

pytestmark = pytest.mark.gpu

NAMES = list(QB.instances())
SHORT = [n for n in NAMES if QB.instances()[n].N <= 64]
PLANS = [n for n in NAMES if QB.instances()[n].kind == "plan"]
WARM = [n for n in NAMES if len(QB.instances()[n].warm_rows)]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.cuda() if dtype is None else t.to("cuda", dtype)


def dev_problem(prob):
    return {k: dev(prob[k]) for k in QB.KEYS}


def compare(got, ref, what, lam=True, rows=None):
    """Device outputs `got` against the oracle's `ref` (rows: the oracle rows each device row is)."""
    torch.cuda.synchronize()
    for k in QB.OUT_KEYS + (("lam",) if lam else ()):
        r = ref[k] if rows is None else ref[k][rows]
        np.testing.assert_array_equal(got[k].cpu().numpy(), r, err_msg=f"{k} ({what})")


def assert_reaches_rule(ref):
    """The precondition on the compared rows: status 0 and at least 10 fp64 passes (the oracle's
    split), so the device's total exceeds 8 + 1."""
    assert (ref["status"] == 0).all()
    assert (ref["passes64"] >= QB.BLAND_PASSES64).all(), ref["passes64"]
    assert (ref["passes"] > 8 + 1).all(), ref["passes"]


@pytest.mark.parametrize("name", NAMES)
def test_cold_per_knot_vs_oracle(handle, name):
    I, prob, ref = QB.cold(name, QB.instances()[name].n)
    assert_reaches_rule(ref)
    d = dev_problem(prob)
    for lam in (True, False):
        got = handle.dcm_mpc_solve(d, I.params(native), lambda_out=lam)
        compare(got, ref, f"{name} lambda_out={lam}", lam=lam)
        assert (got["passes"].cpu().numpy() > 8 + 1).all()


@pytest.mark.parametrize("name", SHORT)
def test_cold_kogge_stone_tree_vs_oracle(handle, name):
    """One knot per lane past the DPP-tree limit: the rows tiled to 1025 QPs."""
    B = O.DPP_TREE_MAX_BATCH + 1
    I, prob, ref = QB.cold(name, B)
    assert_reaches_rule(ref)
    rows = np.arange(B) % I.n
    d = {k: dev(prob[k][rows]) for k in QB.KEYS}
    got = handle.dcm_mpc_solve(d, I.params(native), lambda_out=True)
    compare(got, ref, f"{name} tiled to {B}", rows=rows)
    assert (got["passes"].cpu().numpy() > 8 + 1).all()


@pytest.mark.parametrize("name", [n for n in SHORT if QB.instances()[n].M == 8])
def test_fused_and_two_launches_vs_oracle(handle, name):
    """M = 8, N <= 64, a small cold batch: stage 2 inside the active-set kernel's workgroup
    (dcm_mpc_cold_fused_kernel) and as its own launch; both the oracle's bits, hand-overs included."""
    I, prob, ref = QB.cold(name, QB.instances()[name].n)
    assert_reaches_rule(ref)
    d = dev_problem(prob)
    try:
        for fuse in (1, 0):
            native.set_qp_launch_mode(fuse_stage2=fuse)
            got = handle.dcm_mpc_solve(d, I.params(native), lambda_out=True)
            compare(got, ref, f"{name} fuse_stage2={fuse}")
    finally:
        native.set_qp_launch_mode(fuse_stage2=1)


@pytest.mark.parametrize("name", PLANS)
def test_phased_vs_per_knot_and_oracle(handle, name):
    """blf_dcm_mpc_solve_phased, cold, on the rows' phase tables (built on the device): the
    per-knot result and the oracle's."""
    I, prob, ref = QB.cold(name, QB.instances()[name].n)
    assert_reaches_rule(ref)
    p = I.plan
    tab = handle.phase_table(dev(p["nphases"], torch.int32), dev(p["phase_begin"]), dev(p["phase_end"]),
                             dev(p["phase_corners"]), dev(p["phase_ncorners"], torch.int32), max_facets=I.M,
                             ref=dev(p["phase_ref"]))
    omega = dev(p["omega"])
    got = handle.dcm_mpc_solve_phased(tab, 0, dev(p["xi_init"]), omega[:, :I.N], params=I.params(native),
                                      lambda_out=True)
    compare(got, ref, f"{name} phased")
    knot = handle.dcm_mpc_solve(dev_problem(prob), I.params(native), lambda_out=True)
    torch.cuda.synchronize()
    for k in QB.OUT_KEYS + ("lam",):
        assert torch.equal(got[k], knot[k]), k
    # and the phased warm kernel's cold path (previous status 1)
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    warm = dict(vrp=z(I.n, I.N, 2), lam=z(I.n, I.N, I.M), shift=QB.WARM_SHIFT, floor=QB.WARM_FLOOR,
                status=torch.ones(I.n, dtype=torch.int32, device="cuda"))
    got = handle.dcm_mpc_solve_phased(tab, 0, dev(p["xi_init"]), omega[:, :I.N], params=I.params(native),
                                      warm=warm, lambda_out=True)
    compare(got, ref, f"{name} phased, warm kernel, prev_status 1")


@pytest.mark.parametrize("name", NAMES)
def test_warm_kernel_cold_rows_vs_oracle(handle, name):
    """The warm kernels' own fp32 search and Bland passes: the same rows with a warm start whose
    previous status is 1, so each starts cold inside the warm kernel."""
    I, prob, ref = QB.cold(name, QB.instances()[name].n)
    assert_reaches_rule(ref)
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    warm = dict(vrp=z(I.n, I.N, 2), lam=z(I.n, I.N, I.M), shift=QB.WARM_SHIFT, floor=QB.WARM_FLOOR,
                status=torch.ones(I.n, dtype=torch.int32, device="cuda"))
    got = handle.dcm_mpc_solve(dev_problem(prob), I.params(native), warm=warm, lambda_out=True)
    compare(got, ref, f"{name} warm kernel, prev_status 1")


@pytest.mark.parametrize("name", WARM)
def test_genuinely_warm_rows_vs_oracle(handle, name):
    """Rows the warm passes themselves certify after at least 10 of them (no fp32 search, no cold
    re-solve: the device's passes are the fp64 passes)."""
    I, prob, v, l, ps, ref = QB.warm(name)
    assert (ref["status"] == 0).all() and (ref["passes"] == ref["passes64"]).all()
    assert (ref["passes64"] >= QB.BLAND_PASSES64).all()
    warm = dict(vrp=dev(v), lam=dev(l), shift=QB.WARM_SHIFT, floor=QB.WARM_FLOOR, status=dev(ps, torch.int32))
    got = handle.dcm_mpc_solve(dev_problem(prob), I.params(native, QB.WARM_TOL_POLISH), warm=warm, lambda_out=True)
    compare(got, ref, f"{name} warm rows")
    assert (got["passes"].cpu().numpy() >= QB.BLAND_PASSES64).all()
