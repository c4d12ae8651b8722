"""The pass loops of the active-set QP kernels (csrc/dcm_mpc_as.hip as_passes) where the glue around
their arithmetic has forms of its own in the float passes of the knot-pair kernels (kPairFloat): the
scans' zero elements and Riccati identities selected by knot ownership instead of filled and
overwritten, pass invariants carried across the float loop; and the other instances of as_passes,
which keep the general forms.  Every case compares status, xi, vrp, iterations, polish flag, passes
and multipliers bit for bit against the oracle, and every QP of every batch is solved (status 0).

  * cold solves at N = 65, 100, 126, 127, 128 with 8 slots: the knot-pair kernels with both trees,
    the last padded horizon and the two with a knot on lane 63;
  * the facet slots: batches whose largest facet count per QP is exactly 2, 3, 4, 5, 6, 7 and 8;
    one batch in which a single knot of a single QP has 8 facets and every other knot 4; the
    unused slots filled with NaN, 1e300 and -1e300 (every reader masks them by the knot's count);
  * the failed passes' restore of the iterate: a batch in which at least half the QPs run three or
    more float passes and at least one runs two or more fp64 passes, at N = 99 and N = 101 (the
    last lane with a knot owns one knot, the lanes after it none: ownership differs inside a lane);
  * the other instances of as_passes: a warm shifted window and the phase-indexed cold solve at
    N = 100, a 16-slot cold solve at N = 50.

What a batch must contain is asserted from the oracle's outputs alone, before the device is asked
(the builders below), so a generated batch that misses its purpose fails on the CPU."""
import functools

import numpy as np
import pytest
import torch

from blf import native
from blf import problems as P
from test_gpu_qp_pass_loops import B, IN_KEYS, _check, _dev, _search, _solve_oracle

pytestmark = pytest.mark.gpu

SEED = 29
PUSH = 0.05      # the initial DCM's offset from the plan, per axis (m)
HARD_PUSH = 0.08  # the batches that must take several passes
FILLS = (np.nan, 1e300, -1e300)


def _plan(N, seed=SEED, push=PUSH, batch=B):
    prob = P.make_batch(batch, horizon=N, n_footsteps=6, seed=seed)
    rng = np.random.Generator(np.random.Philox(key=[seed, 99]))
    prob["xi_init"] = prob["xi_init"] + push * (rng.random((batch, 2)) * 2.0 - 1.0)
    return prob


def _ring(prob, where, k):
    """The polygons of the knots `where` ([B, N] bool) replaced by regular k-gons (radius 4 cm) about
    their references: k facets."""
    c, n = prob["corners"].copy(), prob["ncorners"].copy()
    ang = 2.0 * np.pi * np.arange(k) / k + 0.1
    ring = 0.04 * np.stack([np.cos(ang), np.sin(ang)], -1)
    N = where.shape[1]   # (the plan carries one more polygon than the window has knots)
    c[:, :N][where, :k] = prob["vrp_ref"][where][:, None, :] + ring[None]
    n[:, :N][where] = k
    return dict(prob, corners=c, ncorners=n)


def _assemble(prob, M=8):
    import oracle as O
    w = O.assemble_constraints(prob, max_facets=M)
    return {k: np.ascontiguousarray(w[k]) for k in IN_KEYS}


def _solved(w, M=8):
    ref = _solve_oracle(w, M)
    assert (ref["status"] == 0).all(), ref["status"]
    assert (ref["polished"] == 1).all() and (ref["passes"] > 0).all()
    return ref


@functools.lru_cache(maxsize=None)
def _cold(N, push=PUSH):
    w = _assemble(_plan(N, push=push))
    return w, _solved(w)


@functools.lru_cache(maxsize=None)
def _max_count(mx):
    """N = 100, every QP's largest facet count exactly mx.  mx <= 6: the plan's polygons (4 to 6
    facets) with the counts cut to mx, a relaxation that keeps every QP feasible; mx = 7, 8: a
    regular mx-gon on every third knot."""
    N = 100
    prob = _plan(N)
    if mx > 6:
        where = np.zeros((B, N), bool)
        where[:, ::3] = True
        prob = _ring(prob, where, mx)
    w = _assemble(prob)
    if mx <= 6:
        w["nfacets"] = np.minimum(w["nfacets"], mx).astype(np.int32)
    assert (w["nfacets"].max(1) == mx).all(), w["nfacets"].max(1)
    return w, _solved(w)


@functools.lru_cache(maxsize=None)
def _single_octagon():
    """N = 100: knot 37 of QP 7 has 8 facets, every other knot of the batch 4."""
    N = 100
    where = np.zeros((B, N), bool)
    where[7, 37] = True
    w = _assemble(_ring(_plan(N), where, 8))
    nf = np.minimum(w["nfacets"], 4)
    nf[7, 37] = 8
    w["nfacets"] = nf.astype(np.int32)
    assert (np.delete(w["nfacets"].ravel(), 7 * N + 37) == 4).all() and w["nfacets"][7, 37] == 8
    return w, _solved(w)


@functools.lru_cache(maxsize=None)
def _many_passes(N):
    """At least half the QPs run three or more float passes, at least one two or more fp64 passes."""
    w, ref = _cold(N, HARD_PUSH)
    _, np32, _ = _search(w)
    np.testing.assert_array_equal(ref["passes"], np32 + ref["passes64"])
    assert 2 * (np32 >= 3).sum() >= B, np32
    assert (ref["passes64"] >= 2).any(), ref["passes64"]
    return w, ref


def _dirty(w, fill):
    unused = np.arange(8)[None, None, :] >= w["nfacets"][..., None]
    assert unused.any()
    return dict(w, A=np.where(unused[..., None], fill, w["A"]), b=np.where(unused, fill, w["b"]))


def _solve(handle, w, N, M=8):
    return handle.dcm_mpc_solve(_dev(w), native.default_params(N, max_facets=M), lambda_out=True)


@pytest.mark.parametrize("N", [65, 100, 126, 127, 128])
def test_cold_knot_pairs_bitwise(handle, oracle, N):
    w, ref = _cold(N)
    _check(_solve(handle, w, N), ref, f"cold N={N}")


@pytest.mark.parametrize("mx", [2, 3, 4, 5, 6, 7, 8])
def test_largest_facet_count_bitwise(handle, oracle, mx):
    w, ref = _max_count(mx)
    _check(_solve(handle, w, 100), ref, f"largest facet count {mx}")


def test_single_octagon_bitwise(handle, oracle):
    w, ref = _single_octagon()
    _check(_solve(handle, w, 100), ref, "one knot with 8 facets among knots with 4")


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("batch", ["max5", "octagon"])
def test_unused_slots_bitwise(handle, oracle, batch, fill):
    """The slots past a knot's count hold NaN or huge values (+-inf as a float): the clean input's
    outputs.  max5: slots 5 to 7 are unused on every knot."""
    w, ref = _max_count(5) if batch == "max5" else _single_octagon()
    _check(_solve(handle, _dirty(w, fill), 100), ref, f"{batch}, unused slots = {fill}")


@pytest.mark.parametrize("N", [99, 101])
def test_many_passes_odd_horizon_bitwise(handle, oracle, N):
    w, ref = _many_passes(N)
    _check(_solve(handle, w, N), ref, f"cold N={N}, several passes")


def test_warm_shifted_window_bitwise(handle, oracle):
    """The next window (shift 1) of a longer plan at N = 100, warm-started from the oracle's cold solution."""
    import oracle as O
    N = 100
    full = O.assemble_constraints(_plan(N + 4, seed=SEED + 1), max_facets=8)
    prev = _solved(P.window(full, 0, N))
    w1 = P.window(full, 1, N, np.ascontiguousarray(prev["xi"][:, 1]))
    ref = _solve_oracle(w1, warm=(prev["vrp"], prev["lam"]))
    assert (ref["status"] == 0).all() and (ref["passes"] > 0).all()
    warm = dict(vrp=torch.from_numpy(prev["vrp"]).cuda(), lam=torch.from_numpy(prev["lam"]).cuda(), shift=1, floor=1e-2)
    got = handle.dcm_mpc_solve(_dev(w1), native.default_params(N), warm=warm, lambda_out=True)
    _check(got, ref, "warm N=100")


def test_phased_cold_bitwise(handle, oracle):
    """The phase-indexed entry point at N = 100 (rows gathered from the plan's phase table), cold."""
    O = oracle
    N = 100
    plan = _plan(N + 2)
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
        ref = _solved(w)
        got = handle.dcm_mpc_solve_phased(tab, s, d("xi_init"), omega[:, s:s + N], lambda_out=True)
        _check(got, ref, f"phased N={N} window {s}")


def test_sixteen_slots_cold_bitwise(handle, oracle):
    """N = 50 with 16 facet slots (one knot per lane, rows read from LDS): octagons
    on every third knot."""
    N = 50
    prob = _plan(N)
    where = np.zeros((B, N), bool)
    where[:, ::3] = True
    w = _assemble(_ring(prob, where, 8), M=16)
    assert {4, 6, 8} <= set(np.unique(w["nfacets"]))
    ref = _solved(w, M=16)
    _check(_solve(handle, w, N, M=16), ref, "cold N=50, 16 slots")
