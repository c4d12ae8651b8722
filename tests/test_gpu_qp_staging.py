"""The facet rows' staging into LDS across its shapes (csrc/dcm_mpc_as.hip stage_rows_issue /
stage_rows_commit): the fast path (64 % (M KPL) == 0: a lane's facet index fixed, its LDS slot a
constant offset per round, rounds past N M skipped) and the generic path, at the sizes where the
rounds change: one partial round, N M = 64 exactly, one element more, the knots-per-lane boundary
(63, 64, 65), the bench's shape, the pad boundary (126, 127), a full sixteen rounds (128), and the
16-slot kernels' rounds with t0 > 0.  The cold per-knot solve at every shape and the warm solve of
one shifted window at two of them, 37 QPs each, bit for bit against the oracle: status, xi, vrp,
iterations, polish flag, active-set passes and multipliers (a row staged into the wrong slot, or
not at all, changes the active sets and with them every one of these).

The problems are windows of one blf.problems.make_batch plan per M, from knot 5 on, so even the
shortest window crosses the first lift-off (knot 10): double-support knots with 6 facets, single
support with 4, all below M = 8 and 16.  M = 4 takes the bounding boxes of the polygons, with one
facet fewer on every seventh knot (a relaxation, so the QP stays feasible); M = 6 the plan as it
is.  Every QP is feasible: the oracle alone reports status 0 on all 37 of every shape."""
import functools

import numpy as np
import pytest
import torch

from blf import native
from blf import problems as P

pytestmark = pytest.mark.gpu

B = 37
START = 5            # the windows' first knot: five knots before the first lift-off
PLAN_KNOTS = 136     # START + 128 knots + the warm window's shift, and a few to spare
IN_KEYS = ("xi_init", "omega", "xi_ref", "vrp_ref", "A", "b", "nfacets")
OUT_KEYS = ("status", "xi", "vrp", "iters", "polished", "passes", "lam")

COLD_SHAPES = [(1, 8), (7, 8), (8, 8), (9, 8), (63, 8), (64, 8), (65, 8), (100, 8), (126, 8), (127, 8),
               (128, 8), (100, 4), (100, 6), (50, 16), (100, 16)]
WARM_SHAPES = [(100, 8), (50, 16)]


def _bounding_boxes(prob):
    """Every knot's support polygon replaced by its axis-aligned bounding box (4 facets)."""
    c, n = prob["corners"], prob["ncorners"]
    inside = np.arange(c.shape[2])[None, None, :, None] < n[..., None, None]
    lo = np.where(inside, c, np.inf).min(2)
    hi = np.where(inside, c, -np.inf).max(2)
    box = np.zeros_like(c)
    box[:, :, 0] = lo
    box[:, :, 1] = np.stack([hi[..., 0], lo[..., 1]], -1)
    box[:, :, 2] = hi
    box[:, :, 3] = np.stack([lo[..., 0], hi[..., 1]], -1)
    return dict(prob, corners=box, ncorners=np.full_like(n, 4))


@functools.lru_cache(maxsize=None)
def _plan(M):
    import oracle as O
    prob = P.make_batch(B, horizon=PLAN_KNOTS, n_footsteps=6, seed=700 + M)
    if M == 4:
        prob = _bounding_boxes(prob)
    full = O.assemble_constraints(prob, max_facets=M)
    if M == 4:
        full["nfacets"][:, 3::7] -= 1
    nf = full["nfacets"]
    assert (nf >= 3).all() and (nf <= M).all()
    assert (nf < M).any() and len(np.unique(nf)) > 1
    return full


def _solve_oracle(w, N, M, warm=None):
    import oracle as O
    pol = np.zeros(B, np.int32)
    pas = np.zeros(B, np.int32)
    kw = dict(params=O.default_params(N, max_facets=M), threads=8, polished=pol, passes=pas)
    if warm is None:
        st, xi, vrp, it, lam = O.dcm_mpc_solve_batch_warm(w, **kw)
    else:
        st, xi, vrp, it, lam = O.dcm_mpc_solve_batch_warm(w, warm[0], warm[1], 1, 1e-2, **kw)
    return dict(status=st, xi=xi, vrp=vrp, iters=it, polished=pol, passes=pas, lam=lam)


@functools.lru_cache(maxsize=None)
def _cold_case(N, M):
    """(window, the oracle's cold solution), computed once per shape and shared."""
    w = P.window(_plan(M), START, N)
    return w, _solve_oracle(w, N, M)


def _dev(w):
    return {k: torch.from_numpy(np.ascontiguousarray(w[k])).cuda() for k in IN_KEYS}


def _check(got, ref, what):
    torch.cuda.synchronize()
    assert (ref["status"] == 0).all(), (what, ref["status"])
    for k in OUT_KEYS:
        np.testing.assert_array_equal(got[k].cpu().numpy(), ref[k], err_msg=f"{k} {what}")
    assert (ref["passes"] > 0).all()   # the active-set kernels ran


@pytest.mark.parametrize("N,M", COLD_SHAPES)
def test_cold_staging_shapes_bitwise(handle, oracle, N, M):
    w, ref = _cold_case(N, M)
    got = handle.dcm_mpc_solve(_dev(w), native.default_params(N, max_facets=M), lambda_out=True)
    _check(got, ref, f"cold N={N} M={M}")


@pytest.mark.parametrize("N,M", WARM_SHAPES)
def test_warm_staging_shapes_bitwise(handle, oracle, N, M):
    """The next window (shift 1), warm-started from the oracle's cold solution of this one."""
    _, prev = _cold_case(N, M)
    w = P.window(_plan(M), START + 1, N, np.ascontiguousarray(prev["xi"][:, 1]))
    ref = _solve_oracle(w, N, M, warm=(prev["vrp"], prev["lam"]))
    warm = dict(vrp=torch.from_numpy(prev["vrp"]).cuda(), lam=torch.from_numpy(prev["lam"]).cuda(),
                shift=1, floor=1e-2)
    got = handle.dcm_mpc_solve(_dev(w), native.default_params(N, max_facets=M), warm=warm, lambda_out=True)
    _check(got, ref, f"warm N={N} M={M}")
