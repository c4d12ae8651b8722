"""The windows of tests/golden/qp_bland_windows.npz (test infrastructure; made by
tests/golden/make_qp_bland_windows.py): per instance of the active-set QP kernels, the QPs whose
fp64 drop/add passes reach the anti-cycling rule (Bland's rule, oracle dcm_polish; the kernels'
as_passes), rebuilt here as the per-knot problems and phase tables the tests solve.

An instance is named m<M>_n<N> (facet slots, horizon; a trailing w: a second source at the same
M, N).  Two kinds of source:
  * "c5": rows of another fixture (tests/golden/c5_hard_windows.npz) truncated to their first N
    knots; the fixture holds the row indices only.  Cold rows are solved with the default
    parameters, warm rows (`warm_rows`) from the fixture's own warm start truncated alike
    (shift 1, floor 1e-3, tol_polish 1e-4);
  * "plan": rows of contact plans; the fixture holds their phase-table inputs (corners, counts,
    begin/end, references), xi_init, omega and dt.  Window 0 is the cold QP; these have no
    genuinely warm rows (make_qp_bland_windows.py says what was searched).
"""
import functools
import os

import numpy as np

import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "qp_bland_windows.npz")
KEYS = ("xi_init", "omega", "xi_ref", "vrp_ref", "A", "b", "nfacets")
PLAN_KEYS = ("nphases", "phase_begin", "phase_end", "phase_corners", "phase_ncorners", "phase_ref",
             "xi_init", "omega")
OUT_KEYS = ("status", "iters", "xi", "vrp", "polished", "passes")   # compared bit for bit (and lam)
BLAND_PASSES64 = 10   # the 10th fp64 pass is the first one that starts from a Bland move
WARM_SHIFT, WARM_FLOOR, WARM_TOL_POLISH = 1, 1e-3, 1e-4


def truncate(d, N, rows=None):
    """The first N knots of the per-knot problem arrays of `d` (rows: a subset of its problems)."""
    r = slice(None) if rows is None else rows
    out = {k: np.ascontiguousarray(d[k][r][:, :N]) for k in ("omega", "vrp_ref", "A", "b", "nfacets")}
    out["xi_ref"] = np.ascontiguousarray(d["xi_ref"][r][:, :N + 1])
    out["xi_init"] = np.ascontiguousarray(d["xi_init"][r])
    return out


def plan_table(plan, M):
    """The plan's phase table with the oracle's support-polygon H-reps (orc_hull2d_hrep)."""
    B, Pn, C, _ = plan["phase_corners"].shape
    A, b, nf = O.hull2d_hrep_batch(plan["phase_corners"].reshape(B * Pn, C, 2),
                                   plan["phase_ncorners"].reshape(B * Pn), M, threads=8)
    return dict(nphases=plan["nphases"], phase_begin=plan["phase_begin"], phase_end=plan["phase_end"],
                phase_A=A.reshape(B, Pn, M, 2), phase_b=b.reshape(B, Pn, M), phase_nf=nf.reshape(B, Pn),
                phase_ref=plan["phase_ref"])


def plan_window(otab, plan, s, N, xi_init=None):
    """Window s .. s + N of a plan as the per-knot problem (orc_dcm_phase_expand)."""
    w = O.dcm_phase_expand_batch(otab, s, float(plan["dt"]), N, threads=8)
    w["xi_init"] = np.ascontiguousarray(plan["xi_init"] if xi_init is None else xi_init)
    w["omega"] = np.ascontiguousarray(plan["omega"][:, s:s + N])
    return w


class Instance:
    def __init__(self, name, d):
        g = lambda k: d[f"{name}/{k}"]
        self.name = name
        self.kind = str(g("kind"))
        self.M, self.N = int(g("M")), int(g("N"))
        self.dt, self.tol_polish = float(g("dt")), float(g("tol_polish"))
        if self.kind == "c5":
            self.source = str(g("source"))
            self.rows = g("rows")
            self.warm_rows = g("warm_rows")
        else:
            self.warm_rows = np.zeros(0, np.int32)
            self.plan = {k: g(k) for k in PLAN_KEYS}
            self.plan["dt"] = self.dt
        # per cold row: certified by the active-set passes (else: handed to the interior point method)
        self.certified = g("certified").astype(bool)
        self.passes64 = g("passes64")
        self.n = len(self.certified)

    def params(self, mod, tol_polish=None):
        """default_params of `mod` (the oracle binding or blf.native) for this instance."""
        p = mod.default_params(self.N, max_facets=self.M, dt=self.dt)
        p.tol_polish = self.tol_polish if tol_polish is None else tol_polish
        return p

    def cold_problem(self):
        """The per-knot problems of the instance's cold Bland rows."""
        if self.kind == "c5":
            return truncate(_source(self.source), self.N, self.rows)
        return plan_window(plan_table(self.plan, self.M), self.plan, 0, self.N)

    def warm_problem(self):
        """(problem, vrp_ws, lam_ws, prev_status) of a c5 instance's genuinely warm Bland rows."""
        d, r, N = _source(self.source), self.warm_rows, self.N
        return (truncate(d, N, r), np.ascontiguousarray(d["vrp_ws"][r][:, :N]),
                np.ascontiguousarray(d["lam_ws"][r][:, :N]), np.ascontiguousarray(d["prev_status"][r]))


@functools.lru_cache(maxsize=None)
def _source(name):
    return dict(np.load(os.path.join(GOLDEN, name)))


@functools.lru_cache(maxsize=None)
def instances():
    d = np.load(FIXTURE)
    return {str(n): Instance(str(n), d) for n in d["instances"]}


def solve(prob, params, device_batch, warm=None, prev_status=None):
    """The oracle's batch solve as a launch of device_batch QPs evaluates it, every output the
    tests compare as a dict (warm: (vrp_ws, lam_ws), shift 1, floor 1e-3)."""
    B = prob["omega"].shape[0]
    pol, pas, p64 = (np.zeros(B, np.int32) for _ in range(3))
    kw = {}
    if warm is not None:
        kw = dict(vrp_ws=warm[0], lam_ws=warm[1], shift=WARM_SHIFT, floor=WARM_FLOOR, prev_status=prev_status)
    st, xi, vrp, it, lm = O.dcm_mpc_solve_batch_warm(
        {k: prob[k] for k in KEYS}, params=params, threads=8, polished=pol, passes=pas, passes64=p64,
        device_batch=device_batch, **kw)
    return dict(status=st, xi=xi, vrp=vrp, iters=it, lam=lm, polished=pol, passes=pas, passes64=p64)


def launch_batches(I):
    """The batches the GPU tests launch an instance's cold rows as: the rows alone, and for
    horizons <= 64 tiled to 1025 (past the DPP-tree limit: the Kogge-Stone tree)."""
    return (I.n, O.DPP_TREE_MAX_BATCH + 1) if I.N <= 64 else (I.n,)


@functools.lru_cache(maxsize=None)
def cold(name, device_batch):
    """(instance, per-knot problem, oracle result) of an instance's cold rows as a launch of
    device_batch QPs evaluates them.  Computed once and shared by the tests: read-only."""
    I = instances()[name]
    prob = I.cold_problem()
    return I, prob, solve(prob, I.params(O), device_batch)


@functools.lru_cache(maxsize=None)
def warm(name):
    """(instance, problem, vrp_ws, lam_ws, prev_status, oracle result) of the genuinely warm rows."""
    I = instances()[name]
    prob, v, l, ps = I.warm_problem()
    return I, prob, v, l, ps, solve(prob, I.params(O, WARM_TOL_POLISH), len(ps), warm=(v, l), prev_status=ps)
