"""Generates tests/golden/qp_bland_windows.npz: per instance of the active-set QP kernels
(csrc/dcm_mpc_as.hip launch_kpl: 8 | 16 facet slots, one knot per lane | knot pairs, scan tree), the
QPs whose fp64 drop/add passes reach the anti-cycling rule (Bland's rule from fp64 pass index 8 on:
oracle dcm_polish, the kernels' as_passes).  tests/test_qp_bland.py checks the rows on
the oracle, tests/test_gpu_qp_bland.py the device against the oracle on them, bit for bit.

A "Bland row" has oracle status 0 and at least 10 fp64 passes (orc_dcm_mpc_solve_warm64's passes64):
a QP that certifies at the 9th pass never applies a Bland move.  The sources, each evaluated whole
as one device launch (for horizons <= 64 under both scan trees; a row is kept only if it is a
Bland row with the same outcome under both):

  m8_n50, m8_n64, m8_n65, m8_n100   c5_hard_windows.npz truncated to its first N knots, default
                                    parameters; warm rows: its own warm start truncated alike
                                    (shift 1, floor 1e-3, tol_polish 1e-4, the previous status)
  m8_n127, m8_n128                  problems.make_batch(4096, horizon=128, n_footsteps=8, seed=SEED)
                                    with the initial DCM moved by up to 0.06 m per axis
                                    (default_rng(7)), window 0, tol_polish 1e-4.  (The plans of
                                    multi_contact.plan(4096, dt=0.04, knots=150, poses="identity",
                                    seed=11, xi_offset=0.05) have 823 Bland rows at either horizon,
                                    but every phase there is the same rectangle, each Bland pass
                                    has one knot and facet to choose from, and no mutation of the
                                    rule changes any output: not used.)
  m8_n64w, m8_n65w, m8_n100w        the same walking plans at the c5 instances' horizons: further
                                    rows where the c5 truncations have few that the active-set
                                    passes certify
  m16_n50, m16_n64                  problems.three_contact_plan(4096, dt=0.1, knots=75), seeds
                                    SEED .. SEED + 7 (SEED alone has two Bland rows), window 0
  m16_n100, m16_n128                problems.three_contact_plan(4096, dt=0.05, knots=150, seed=SEED),
                                    window 0; rows that end with status 1 or 2 are left out
  m16_n100w, m16_n128w              the same plans with xi_offset=0.065: rows whose Bland passes
                                    have changes in several lanes at once (the plans above have
                                    about one such row per 4096); 15-20 % of this source ends with
                                    status 1 or 2 and is left out

Warm rows (certified by the warm kernel's own passes, at least 10 of them) exist only in the c5
instances.  The plan sources were also searched as receding horizons, windows 1 .. 7 each
warm-started from the one before (shift 1, floor 1e-3) over the whole source: every window
certifies in fewer than 9 warm passes, so the plan instances have no genuinely warm rows.

Up to 64 cold rows per instance (48 certified by the active-set passes, 16 handed to the interior
point method, where both exist: only a certified row carries its Bland moves to the outputs) and up
to 16 warm rows.  c5 rows are stored as row indices,
plan rows as their phase-table inputs, xi_init, omega and dt.  The archive is written with fixed
time stamps, so a second run reproduces it byte for byte.

    python tests/golden/make_qp_bland_windows.py
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "bipedal-locomotion-framework_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle as O                  # noqa: E402
import qp_bland as QB               # noqa: E402
from blf import problems as P       # noqa: E402

MAX_COLD, MAX_WARM = 64, 16
SOURCE_BATCH = 4096
C5 = "c5_hard_windows.npz"
WALK_SEED, WALK_OFFSET = 7, 0.06
WIDE_OFFSET = 0.065


def trees(N, whole):
    """The device batches a source is evaluated as: the whole source, and for horizons <= 64 one
    batch on each side of the DPP-tree limit."""
    return (64, 1025) if N <= 64 else (whole,)


def pick(cert, cap):
    """Up to cap of the rows, in row order: three quarters of them rows the active-set passes certify
    (only there do the Bland moves reach the outputs; a handed-over row restores its start point),
    the rest handed-over rows, either share filled from the other where one runs short."""
    idx = np.arange(len(cert))
    a, b = idx[cert], idx[~cert]
    na = min(len(a), max(3 * cap // 4, cap - len(b)))
    nb = min(len(b), cap - na)
    return np.sort(np.concatenate([a[:na], b[:nb]]))


def cold_bland(prob, prm, N, whole):
    """(mask of the Bland rows, certified-by-the-active-set-passes, passes64) of a cold source."""
    res = [QB.solve(prob, prm, db) for db in trees(N, whole)]
    ok = np.ones(len(res[0]["status"]), bool)
    for r in res:
        ok &= (r["status"] == 0) & (r["passes64"] >= QB.BLAND_PASSES64)
        ok &= (r["iters"] == 0) == (res[0]["iters"] == 0)
    return ok, res[0]["iters"] == 0, res[0]["passes64"]


def warm_bland(prob, prm, N, whole, warm, prev):
    """Mask of the rows the warm passes certify with at least 10 of them (no cold re-solve: the
    passes reported are the fp64 passes alone), under every tree."""
    ok = None
    for db in trees(N, whole):
        r = QB.solve(prob, prm, db, warm=warm, prev_status=prev)
        m = (r["status"] == 0) & (r["iters"] == 0) & (r["passes"] == r["passes64"]) & \
            (r["passes64"] >= QB.BLAND_PASSES64)
        ok = m if ok is None else ok & m
    return ok


def c5_instance(N):
    d = dict(np.load(os.path.join(HERE, C5)))
    B = d["omega"].shape[0]
    prob = QB.truncate(d, N)
    ok, cert, p64 = cold_bland(prob, O.default_params(N), N, B)
    rows = np.nonzero(ok)[0]
    rows = rows[pick(cert[rows], MAX_COLD)]
    wprm = O.default_params(N, tol_polish=QB.WARM_TOL_POLISH)
    wok = warm_bland(prob, wprm, N, B, (np.ascontiguousarray(d["vrp_ws"][:, :N]),
                                        np.ascontiguousarray(d["lam_ws"][:, :N])), d["prev_status"])
    return dict(kind=np.array("c5"), source=np.array(C5), M=np.int32(8), N=np.int32(N), dt=np.float64(0.02),
                tol_polish=np.float64(O.default_params(N).tol_polish), rows=rows.astype(np.int32),
                certified=cert[rows].astype(np.int8), passes64=p64[rows].astype(np.int32),
                warm_rows=np.nonzero(wok)[0][:MAX_WARM].astype(np.int32)), int(ok.sum())


def plan_instance(M, N, plans):
    """plans: the source plans (dicts of make_batch's phase-table keys), concatenated in order."""
    keep = {k: [] for k in QB.PLAN_KEYS}
    cert, p64 = [], []
    for plan in plans:
        prm = O.default_params(N, max_facets=M, dt=plan["dt"], tol_polish=QB.WARM_TOL_POLISH)
        w0 = QB.plan_window(QB.plan_table(plan, M), plan, 0, N)
        ok, ce, ps = cold_bland(w0, prm, N, SOURCE_BATCH)
        sel = np.nonzero(ok)[0]
        for k in QB.PLAN_KEYS:
            keep[k].append(plan[k][sel])
        cert.append(ce[sel])
        p64.append(ps[sel])
    cert, p64 = np.concatenate(cert), np.concatenate(p64)
    rows = pick(cert, MAX_COLD)
    out = {k: np.ascontiguousarray(np.concatenate(v)[rows]) for k, v in keep.items()}
    out.update(kind=np.array("plan"), M=np.int32(M), N=np.int32(N), dt=np.float64(plans[0]["dt"]),
               tol_polish=np.float64(QB.WARM_TOL_POLISH), certified=cert[rows].astype(np.int8),
               passes64=p64[rows].astype(np.int32))
    return out, len(cert)


def pushed_walk():
    """Two-foot walking plans (8 footsteps) whose initial DCM is moved off the plan by up to
    WALK_OFFSET per axis: like the c5 windows, many start uncapturable."""
    plan = P.make_batch(SOURCE_BATCH, horizon=128, n_footsteps=8, seed=P.SEED)
    rng = np.random.default_rng(WALK_SEED)
    out = {k: plan[k] for k in QB.PLAN_KEYS}
    out["xi_init"] = plan["xi_init"] + rng.uniform(-WALK_OFFSET, WALK_OFFSET, plan["xi_init"].shape)
    out["dt"] = plan["dt"]
    return out


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
    inst = {}
    for N in (50, 64, 65, 100):
        inst[f"m8_n{N}"] = c5_instance(N)
    walk = pushed_walk()
    for N in (64, 65, 100):
        inst[f"m8_n{N}w"] = plan_instance(8, N, [walk])
    for N in (127, 128):
        inst[f"m8_n{N}"] = plan_instance(8, N, [walk])
    short = [P.three_contact_plan(SOURCE_BATCH, dt=0.1, knots=75, seed=P.SEED + j) for j in range(8)]
    for N in (50, 64):
        inst[f"m16_n{N}"] = plan_instance(16, N, short)
    long_ = [P.three_contact_plan(SOURCE_BATCH, dt=0.05, knots=150, seed=P.SEED)]
    for N in (100, 128):
        inst[f"m16_n{N}"] = plan_instance(16, N, long_)
    wide = [P.three_contact_plan(SOURCE_BATCH, dt=0.05, knots=150, seed=P.SEED, xi_offset=WIDE_OFFSET)]
    for N in (100, 128):
        inst[f"m16_n{N}w"] = plan_instance(16, N, wide)
    arrays = {"instances": np.array(list(inst))}
    print(f"{'instance':<10} {'Bland rows':>10} {'kept':>5} {'fp64 passes 10/11/12':>22} {'certified/IPM':>14} {'warm':>5}")
    for name, (a, nbland) in inst.items():
        for k, v in a.items():
            arrays[f"{name}/{k}"] = v
        hist = np.bincount(a["passes64"], minlength=13)[10:13].tolist()
        n, ce = len(a["certified"]), int(a["certified"].sum())
        nw = len(a["warm_rows"]) if "warm_rows" in a else 0
        print(f"{name:<10} {nbland:>10} {n:>5} {'/'.join(map(str, hist)):>22} {ce:>6} / {n - ce:<5} {nw:>5}")
    path = os.path.join(HERE, "qp_bland_windows.npz")
    write_npz(path, arrays)
    print(f"-> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
