"""The forms of the active-set kernels' LQ step (csrc/dcm_mpc_as.hip as_lq_step): the decoupled step
on one axis (the weights of the instantiated type equal on both axes), on two axes (any pair of
weights differs), and the general step it falls back to; in float (the cold search's start) and in
fp64 (the start point of a QP the passes hand to the interior point stage).  Cold solves of 37 QPs
per case, bit for bit against the oracle, which evaluates the general form alone: status, xi, vrp,
iterations, polish flag, active-set passes and multipliers.

Weights: the default (isotropic); every pair anisotropic; exactly one pair anisotropic (three
cases: the kernel's uniform test must then take the two-axis form); and a pair of doubles that
differ but round to one float (the float step is isotropic, the fp64 step is not).
Shapes: one lane and one pair (N = 1, 2), the knots-per-lane boundary (63, 64, 65), the bench's
100, the pad boundary (126, 127, 128), and N = 50 in a launch of 1 QP (the fused kernel, DPP tree),
of 37 (DPP tree) and of 1025 (one knot per lane in the Kogge-Stone tree).
Facet slots: 8, 6 (generic staging) and 16.
One shifted window warm-started from the oracle's cold solution at (100, 8) (the warm kernel shares
the passes with the cold one).  The first 37 windows of tests/golden/c5_failed_windows_r03.npz,
every one of which the passes hand over (iterations > 0): their start point is the fp64 LQ step.

The problems are those of tests/test_gpu_qp_staging.py: windows of one blf.problems.make_batch plan
per M from knot 5, so every window crosses the first lift-off.  The oracle alone reports status 0
on every QP of every case (asserted here), so no case passes by comparing two failures; many of
the anisotropic and 16-slot cases hand QPs over as well (iterations up to 27)."""
import functools
import os

import numpy as np
import pytest
import torch

from blf import native
from blf import problems as P

pytestmark = pytest.mark.gpu

B = 37
START = 5
PLAN_KNOTS = 136
IN_KEYS = ("xi_init", "omega", "xi_ref", "vrp_ref", "A", "b", "nfacets")
OUT_KEYS = ("status", "xi", "vrp", "iters", "polished", "passes", "lam")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

WEIGHTS = {
    "iso": {},
    "aniso": dict(w_xi=(10.0, 30.0), w_vrp=(2.0, 0.5), w_terminal=(100.0, 500.0), dt=0.015),
    "xi_only": dict(w_xi=(100.0, 130.0)),
    "vrp_only": dict(w_vrp=(1.0, 0.5)),
    "terminal_only": dict(w_terminal=(1000.0, 1500.0)),
    "same_float": dict(w_vrp=(1.0, 1.0 + 2.0 ** -30)),
}
# (N, QPs in the launch)
SHAPES = [(1, B), (2, B), (63, B), (64, B), (65, B), (100, B), (126, B), (127, B), (128, B), (50, 1), (50, B),
          (50, 1025)]
SLOTS = [8, 6, 16]


def test_same_float_weights_differ_in_double():
    a, b = WEIGHTS["same_float"]["w_vrp"]
    assert a != b and np.float32(a) == np.float32(b)


@functools.lru_cache(maxsize=None)
def _plan(M):
    import oracle as O
    full = O.assemble_constraints(P.make_batch(B, horizon=PLAN_KNOTS, n_footsteps=6, seed=700 + M), max_facets=M)
    assert (full["nfacets"] >= 3).all() and (full["nfacets"] <= M).all()
    return full


def _solve_oracle(w, N, M, kw, warm=None, device_batch=None):
    import oracle as O
    n = w["omega"].shape[0]
    pol = np.zeros(n, np.int32)
    pas = np.zeros(n, np.int32)
    args = () if warm is None else (warm[0], warm[1], 1, 1e-2)
    st, xi, vrp, it, lam = O.dcm_mpc_solve_batch_warm(w, *args, params=O.default_params(N, max_facets=M, **kw),
                                                      threads=8, polished=pol, passes=pas,
                                                      device_batch=device_batch)
    return dict(status=st, xi=xi, vrp=vrp, iters=it, polished=pol, passes=pas, lam=lam)


@functools.lru_cache(maxsize=None)
def _cold_case(N, batch, M, wname):
    """(window, the oracle's cold solution): a launch of 1 QP is the plan's first window, one of
    1025 the 37 windows repeated (the oracle solves the 37 as that launch evaluates them)."""
    w = P.window(_plan(M), START, N)
    if batch == 1:
        w = {k: np.ascontiguousarray(v[:1]) for k, v in w.items()}
    ref = _solve_oracle(w, N, M, WEIGHTS[wname], device_batch=batch)
    if batch > B:
        idx = np.arange(batch) % B
        w = {k: np.ascontiguousarray(v[idx]) for k, v in w.items()}
        ref = {k: np.ascontiguousarray(v[idx]) for k, v in ref.items()}
    return w, ref


@functools.lru_cache(maxsize=None)
def _warm_case(wname):
    """The next window of (100, 8), warm-started from the oracle's cold solution of this one."""
    N, M = 100, 8
    _, prev = _cold_case(N, B, M, wname)
    assert (prev["status"] == 0).all()
    w = P.window(_plan(M), START + 1, N, np.ascontiguousarray(prev["xi"][:, 1]))
    return w, prev, _solve_oracle(w, N, M, WEIGHTS[wname], warm=(prev["vrp"], prev["lam"]))


@functools.lru_cache(maxsize=None)
def _handover_case():
    """37 windows the active-set passes do not certify (uncapturable DCM states): the interior
    point stage starts from the fp64 LQ step."""
    d = np.load(os.path.join(GOLDEN, "c5_failed_windows_r03.npz"))
    w = {k: np.ascontiguousarray(d[k][:B]) for k in IN_KEYS}
    N, M = w["omega"].shape[1], w["b"].shape[2]
    return w, N, M, _solve_oracle(w, N, M, {})


def _dev(w):
    return {k: torch.from_numpy(np.ascontiguousarray(w[k])).cuda() for k in IN_KEYS}


def _check(got, ref, what):
    torch.cuda.synchronize()
    assert (ref["status"] == 0).all(), (what, ref["status"])
    assert (ref["passes"] > 0).all()   # the active-set kernels ran
    for k in OUT_KEYS:
        np.testing.assert_array_equal(got[k].cpu().numpy(), ref[k], err_msg=f"{k} {what}")


@pytest.mark.parametrize("M", SLOTS)
@pytest.mark.parametrize("N,batch", SHAPES)
@pytest.mark.parametrize("wname", list(WEIGHTS))
def test_cold_lq_forms_bitwise(handle, oracle, wname, N, batch, M):
    w, ref = _cold_case(N, batch, M, wname)
    got = handle.dcm_mpc_solve(_dev(w), native.default_params(N, max_facets=M, **WEIGHTS[wname]), lambda_out=True)
    _check(got, ref, f"cold {wname} N={N} B={batch} M={M}")


@pytest.mark.parametrize("wname", ["iso", "aniso"])
def test_warm_shifted_window_bitwise(handle, oracle, wname):
    w, prev, ref = _warm_case(wname)
    warm = dict(vrp=torch.from_numpy(prev["vrp"]).cuda(), lam=torch.from_numpy(prev["lam"]).cuda(),
                shift=1, floor=1e-2)
    got = handle.dcm_mpc_solve(_dev(w), native.default_params(100, max_facets=8, **WEIGHTS[wname]), warm=warm,
                               lambda_out=True)
    _check(got, ref, f"warm {wname}")


def test_handed_over_start_point_bitwise(handle, oracle):
    w, N, M, ref = _handover_case()
    assert (ref["iters"] > 0).all()   # every one handed over (and solved: _check asserts status 0)
    got = handle.dcm_mpc_solve(_dev(w), native.default_params(N, max_facets=M), lambda_out=True)
    _check(got, ref, "handed over")
