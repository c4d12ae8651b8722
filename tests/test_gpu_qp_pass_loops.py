"""The drop/add pass loops of the active-set QP kernels (csrc/dcm_mpc_as.hip as_passes) at the
shapes where their register-level forms can go wrong: the fp32 search's facet rows held in
registers (RegRows: read and rounded once, rows i >= m masked by the knot's count), the
distance-1 DPP shuffles of the scans (dcm_qp_common.h dpp1), and the kernels built without SLP
packing.  Every case compares status, xi, vrp, iterations, polish flag, passes and multipliers bit
for bit against the oracle.

  * horizons 1, 2, 63, 64, 65, 100, 126, 127, 128: one and two knots per lane, the DPP tree (N <= 64
    at up to 1024 QPs, fused and as two launches), the pad tree (N <= 126) and the Kogge-Stone tree
    with lane 63 owning a knot (127, 128); one knot per lane past the DPP-tree limit (1025 QPs);
  * facet counts 4, 6 and 8 in 8 slots, counts one below the polygon's and m = 0 mixed in, and a
    16-slot launch;
  * the unused slots i >= m of A and b filled with NaN, and with huge finite values (1e300: +-inf
    as a float): the outputs are those of the clean input;
  * the cold, fused, warm and phase-indexed entry points;
  * a facet count outside [0, M] (BLF_QP_BAD_FACETS).

The batches are blf.problems.make_batch plans with fixed seeds whose initial DCM is moved off the
plan by up to PUSH m (fixed Philox draws), which is what makes the search take several passes.  The
main batch contains, asserted below from what the oracle returns: QPs the float search certifies,
QPs it hands over uncertified (orc_as32_search's return value), QPs with six or more passes, knots
with two active facets (two positive multipliers) and knots that enter the fp64 passes with more
than two candidate facets (the hand-over's candidate sets: the vertex-pair path of as_pass_setup).
Whether a *float* pass met more than two candidates cannot be told from what the oracle returns
(the search's intermediate sets are not exported); the windows of tests/golden/c5_hard_windows.npz
(test_gpu_c5_windows.py) and the rows of tests/golden/qp_bland (test_gpu_qp_bland.py), whose
searches run all eight float passes with two facets added at once, cover that path."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from blf import native
from blf import problems as P

pytestmark = pytest.mark.gpu

SEED = 11
PUSH = 0.05          # the initial DCM's offset from the plan, per axis (m)
B = 48
IN_KEYS = ("xi_init", "omega", "xi_ref", "vrp_ref", "A", "b", "nfacets")
OUT_KEYS = ("status", "xi", "vrp", "iters", "polished", "passes", "lam")
HORIZONS = (1, 2, 63, 64, 65, 100, 126, 127, 128)


def _octagons(prob, every=3):
    """Every `every`-th knot's polygon replaced by a regular octagon (radius 4 cm) about its
    reference: 8 facets.  (The VRP alone is constrained, so the QP stays feasible.)"""
    c, n = prob["corners"].copy(), prob["ncorners"].copy()
    ang = 2.0 * np.pi * np.arange(8) / 8.0 + 0.1
    ring = 0.04 * np.stack([np.cos(ang), np.sin(ang)], -1)
    N = n.shape[1]
    c[:, ::every] = prob["vrp_ref"][:, ::every, None, :] + ring[None, None]
    n[:, ::every] = 8
    return dict(prob, corners=c, ncorners=n), N


@functools.lru_cache(maxsize=None)
def _problem(N, M=8, batch=B, kind="plain", seed=SEED, push=PUSH):
    """The per-knot QPs (host arrays, constraints assembled by the oracle).
    kind: plain | octagons (8 facets on every third knot) | fewer (counts below the polygons', m = 0
    among them)."""
    import oracle as O
    prob = P.make_batch(batch, horizon=N, n_footsteps=6, seed=seed)
    rng = np.random.Generator(np.random.Philox(key=[seed, 99]))
    prob["xi_init"] = prob["xi_init"] + push * (rng.random((batch, 2)) * 2.0 - 1.0)
    if kind == "octagons":
        prob, _ = _octagons(prob)
    w = O.assemble_constraints(prob, max_facets=M)
    if kind == "fewer":   # relaxations: one facet fewer on every fifth knot, none on every seventh
        w["nfacets"][:, 2::5] -= 1
        w["nfacets"][:, 3::7] = 0
    return {k: np.ascontiguousarray(w[k]) for k in IN_KEYS}


def _solve_oracle(w, M=8, device_batch=None, warm=None, tol_polish=3e-4):
    import oracle as O
    n, N = w["omega"].shape
    pol = np.zeros(n, np.int32)
    pas = np.zeros(n, np.int32)
    p64 = np.zeros(n, np.int32)
    kw = dict(params=O.default_params(N, max_facets=M, tol_polish=tol_polish), threads=8, polished=pol, passes=pas,
              passes64=p64, device_batch=device_batch)
    if warm is None:
        st, xi, vrp, it, lam = O.dcm_mpc_solve_batch_warm(w, **kw)
    else:
        st, xi, vrp, it, lam = O.dcm_mpc_solve_batch_warm(w, warm[0], warm[1], 1, 1e-2, **kw)
    return dict(status=st, xi=xi, vrp=vrp, iters=it, polished=pol, passes=pas, lam=lam, passes64=p64)


@functools.lru_cache(maxsize=None)
def _cold_ref(N, M=8, batch=B, kind="plain", device_batch=None):
    return _solve_oracle(_problem(N, M, batch, kind), M, device_batch)


def _search(w, M=8):
    """The oracle's fp32 search alone, per QP: (certified [n], float passes [n], the candidate sets
    it hands to the fp64 passes [n][N])."""
    import oracle as O
    n, N = w["omega"].shape
    L = O.lib()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    L.orc_as32_search.restype = ctypes.c_int
    L.orc_as32_search.argtypes = [ctypes.POINTER(O.OrcParams), ctypes.c_int] + [dp] * 6 + [ip, dp, dp, ip, ip]
    prm = O._tree_params(O.default_params(N, max_facets=M), N, n)
    cert = np.zeros(n, np.int32)
    npass = np.zeros(n, np.int32)
    guess = np.zeros((n, N), np.int32)
    for i in range(n):
        r, x, np1 = np.zeros((N, 2)), np.zeros((N, 2)), np.zeros(1, np.int32)
        a = {k: np.ascontiguousarray(w[k][i]) for k in IN_KEYS}
        cert[i] = L.orc_as32_search(ctypes.byref(prm), 0, O._d(a["xi_init"]), O._d(a["omega"]), O._d(a["xi_ref"]),
                                    O._d(a["vrp_ref"]), O._d(a["A"]), O._d(a["b"]), O._i(a["nfacets"]), O._d(r),
                                    O._d(x), O._i(guess[i]), O._i(np1))
        npass[i] = np1[0]
    return cert, npass, guess


def _dev(w):
    return {k: torch.from_numpy(np.ascontiguousarray(w[k])).cuda() for k in IN_KEYS}


def _check(got, ref, what, rows=None, keys=OUT_KEYS):
    torch.cuda.synchronize()
    for k in keys:
        r = ref[k] if rows is None else ref[k][rows]
        np.testing.assert_array_equal(got[k].cpu().numpy(), r, err_msg=f"{k} ({what})")


def test_main_batch_reaches_every_path(oracle):
    """The classes of the N = 100 batch the other cases rely on, from the oracle's outputs."""
    w, ref = _problem(100), _cold_ref(100)
    cert, np32, guess = _search(w)
    assert (ref["status"] == 0).all() and (ref["polished"] == 1).all()
    assert (cert == 1).any(), "no QP the float search certifies"
    assert (cert == 0).any(), "no QP the float search hands over uncertified"
    np.testing.assert_array_equal(ref["passes"], np32 + ref["passes64"])
    assert (ref["passes"] >= 6).any(), ref["passes"]
    assert ((ref["lam"] > 0.0).sum(-1) == 2).any(), "no knot with two active facets"
    pc = np.array([[bin(int(v)).count("1") for v in row] for row in guess])
    assert ((pc > 2).any(-1) & (cert == 0)).any(), "no knot handed over with more than two candidates"
    nf = w["nfacets"]
    assert {4, 6} <= set(np.unique(nf)) and (nf < 8).all()   # every knot leaves slots unused


@pytest.mark.parametrize("N", HORIZONS)
def test_cold_horizons_bitwise(handle, oracle, N):
    """Cold, 8 slots: N <= 64 runs the fused kernel (DPP tree) and, with fusing off, the cold kernel
    and its stage-2 launch; N > 64 the knot-pair kernels (pad tree to 126, Kogge-Stone beyond)."""
    w, ref = _problem(N), _cold_ref(N)
    d = _dev(w)
    try:
        for fuse in ((1, 0) if N <= 64 else (1,)):
            native.set_qp_launch_mode(fuse_stage2=fuse)
            for lam in (True, False):
                got = handle.dcm_mpc_solve(d, native.default_params(N), lambda_out=lam)
                _check(got, ref, f"cold N={N} fuse={fuse} lambda_out={lam}", keys=OUT_KEYS if lam else OUT_KEYS[:-1])
    finally:
        native.set_qp_launch_mode(fuse_stage2=1)
    assert (ref["passes"] > 0).all()


def test_cold_one_knot_per_lane_kogge_stone_bitwise(handle, oracle):
    """N = 64 past the DPP-tree limit: 32 QPs tiled to 1025, so lane l owns knot l in the
    Kogge-Stone tree (Wrap shuffles at distance 1, lane 63 a real knot)."""
    n, Bt = 32, 1025
    w = _problem(64, batch=n)
    ref = _cold_ref(64, batch=n, device_batch=Bt)
    rows = np.arange(Bt) % n
    got = handle.dcm_mpc_solve(_dev({k: w[k][rows] for k in IN_KEYS}), native.default_params(64), lambda_out=True)
    _check(got, ref, "cold N=64 tiled to 1025", rows=rows)


@pytest.mark.parametrize("N,M,kind", [(100, 8, "octagons"), (64, 8, "octagons"), (100, 8, "fewer"), (64, 8, "fewer"),
                                      (100, 6, "plain"), (100, 4, "fewer"), (100, 16, "octagons")])
def test_cold_facet_counts_bitwise(handle, oracle, N, M, kind):
    """4, 6 and 8 facets in 8 slots, counts below the polygons' with m = 0 among them, 6 and 4 slots
    (M = 4: the double-support hexagons do not fit, so those knots' counts are relaxed to 0 by the
    assembly's clamp or the `fewer` rule), and the 16-slot kernels (rows read from LDS)."""
    if M == 4:
        w = {k: v.copy() for k, v in _problem(N, 8, B, kind).items()}
        w["A"], w["b"] = np.ascontiguousarray(w["A"][:, :, :4]), np.ascontiguousarray(w["b"][:, :, :4])
        w["nfacets"] = np.where(w["nfacets"] > 4, 0, w["nfacets"]).astype(np.int32)
        ref = _solve_oracle(w, M)
    else:
        w, ref = _problem(N, M, B, kind), _cold_ref(N, M, B, kind)
    nf = w["nfacets"]
    if kind == "octagons":
        assert {4, 6, 8} <= set(np.unique(nf))
    if kind == "fewer":
        assert (nf == 0).any() and ((nf > 0) & (nf < M)).any()
    assert (ref["status"] == 0).all()
    got = handle.dcm_mpc_solve(_dev(w), native.default_params(N, max_facets=M), lambda_out=True)
    _check(got, ref, f"cold N={N} M={M} {kind}")


@pytest.mark.parametrize("fill", [np.nan, 1e300, -1e300])
@pytest.mark.parametrize("N", [64, 100])
def test_unused_slots_never_read_into_a_result(handle, oracle, N, fill):
    """Slots i >= m of A and b hold NaN or huge values (+-inf once rounded to float): every output
    is the clean input's.  N = 64: the fused kernel; N = 100: the cold kernel; then the warm
    kernel's cold path (previous status 1)."""
    w, ref = _problem(N, 8, B, "fewer"), _cold_ref(N, 8, B, "fewer")
    unused = np.arange(8)[None, None, :] >= w["nfacets"][..., None]
    assert unused.any(-1).all() and (w["nfacets"] == 0).any()
    dirty = dict(w, A=np.where(unused[..., None], fill, w["A"]), b=np.where(unused, fill, w["b"]))
    d = _dev(dirty)
    got = handle.dcm_mpc_solve(d, native.default_params(N), lambda_out=True)
    _check(got, ref, f"cold N={N} unused slots = {fill}")
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    warm = dict(vrp=z(B, N, 2), lam=z(B, N, 8), shift=1, floor=1e-2,
                status=torch.ones(B, dtype=torch.int32, device="cuda"))
    got = handle.dcm_mpc_solve(d, native.default_params(N), warm=warm, lambda_out=True)
    _check(got, ref, f"warm kernel, prev_status 1, N={N} unused slots = {fill}")


@pytest.mark.parametrize("N", [64, 100, 127])
def test_warm_shifted_window_bitwise(handle, oracle, N):
    """The next window (shift 1) of a longer plan, warm-started from the oracle's cold solution."""
    import oracle as O
    plan = P.make_batch(B, horizon=N + 4, n_footsteps=6, seed=SEED + 1)
    rng = np.random.Generator(np.random.Philox(key=[SEED + 1, 99]))
    plan["xi_init"] = plan["xi_init"] + PUSH * (rng.random((B, 2)) * 2.0 - 1.0)
    full = O.assemble_constraints(plan, max_facets=8)
    w0 = P.window(full, 0, N)
    prev = _solve_oracle(w0)
    assert (prev["status"] == 0).all()
    w1 = P.window(full, 1, N, np.ascontiguousarray(prev["xi"][:, 1]))
    ref = _solve_oracle(w1, warm=(prev["vrp"], prev["lam"]))
    warm = dict(vrp=torch.from_numpy(prev["vrp"]).cuda(), lam=torch.from_numpy(prev["lam"]).cuda(), shift=1, floor=1e-2)
    got = handle.dcm_mpc_solve(_dev(w1), native.default_params(N), warm=warm, lambda_out=True)
    _check(got, ref, f"warm N={N}")
    assert (ref["passes"] > 0).all()


@pytest.mark.parametrize("N", [64, 100])
def test_phased_cold_bitwise(handle, oracle, N):
    """The phase-indexed entry point (rows gathered from the plan's phase table into LDS), cold."""
    O = oracle
    plan = P.make_batch(B, horizon=N + 2, n_footsteps=6, seed=SEED)
    rng = np.random.Generator(np.random.Philox(key=[SEED, 99]))
    plan["xi_init"] = plan["xi_init"] + PUSH * (rng.random((B, 2)) * 2.0 - 1.0)
    d = lambda k: torch.from_numpy(np.ascontiguousarray(plan[k])).cuda()
    tab = handle.phase_table(d("nphases"), d("phase_begin"), d("phase_end"), d("phase_corners"),
                             d("phase_ncorners"), ref=d("phase_ref"))
    n, Pn, C, _ = plan["phase_corners"].shape
    A, b, nf = O.hull2d_hrep_batch(plan["phase_corners"].reshape(n * Pn, C, 2), plan["phase_ncorners"].reshape(n * Pn),
                                   8, threads=8)
    otab = dict(nphases=plan["nphases"], phase_begin=plan["phase_begin"], phase_end=plan["phase_end"],
                phase_A=A.reshape(n, Pn, 8, 2), phase_b=b.reshape(n, Pn, 8), phase_nf=nf.reshape(n, Pn),
                phase_ref=plan["phase_ref"])
    omega = d("omega")
    for s in (0, 2):
        w = O.dcm_phase_expand_batch(otab, s, plan["dt"], N, threads=8)
        w["xi_init"] = np.ascontiguousarray(plan["xi_init"])
        w["omega"] = np.ascontiguousarray(plan["omega"][:, s:s + N])
        ref = _solve_oracle(w)
        got = handle.dcm_mpc_solve_phased(tab, s, d("xi_init"), omega[:, s:s + N], lambda_out=True)
        _check(got, ref, f"phased N={N} window {s}")
        assert (ref["passes"] > 0).all()


def test_bad_facet_count_bitwise(handle, oracle):
    """One QP with a count above M and one with a negative count, among solvable ones."""
    N = 100
    w = {k: v.copy() for k, v in _problem(N, batch=8).items()}
    w["nfacets"][2, 5] = 9
    w["nfacets"][5, 98] = -1
    ref = _solve_oracle(w)
    assert ref["status"][2] == native.QP_BAD_FACETS and ref["status"][5] == native.QP_BAD_FACETS
    assert (np.delete(ref["status"], [2, 5]) == 0).all()
    got = handle.dcm_mpc_solve(_dev(w), native.default_params(N), lambda_out=True)
    _check(got, ref, "bad facet counts")
