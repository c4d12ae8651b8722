"""Timing of the swing-foot kernel at the configs[2] pipeline's count (diagnostics; not the driver's
bench.py).  HIP events around `reps` back-to-back calls after a warm-up, median of `rounds` rounds,
the variants alternating within a round.  One JSON line each:

  * swing_foot_eval for L = 2 x 65 536 feet (the workload's contact tables, problems.
    foot_contact_tables, tiled) x Q = 32 queries spread over the plan: time per call, algorithmic
    bytes (per query 8 B in and 200 B out, per list its table once) over time as a fraction of
    8 TB/s; beside it torch's fill_ (write only) and copy_ (half read, half written) of the same
    number of bytes, and quintic_eval_kernel at the same query count (its own bytes and fraction);
  * so3_eval at the same count.

  timeout -k 10 600 python tools/swing_bench.py [--problems 65536] [--queries 32] [--rounds 5]
(BLF_LIB=.../lib/libblf_<name>.so times a variant build, tools/build_variant.sh)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bipedal-locomotion-framework_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from blf import native  # noqa: E402
from blf import problems as P  # noqa: E402

PEAK = 8.0e12   # B/s
BASE = 1024     # distinct problems; tiled up to --problems


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps   # ms per call


def compare(variants, reps, rounds):
    """{name: fn} -> {name: [median ms, min ms, max ms]}, the variants alternating in every round."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, reps))
    return {k: [statistics.median(v), min(v), max(v)] for k, v in times.items()}


def tiled(a, n):
    return torch.from_numpy(np.ascontiguousarray(np.tile(a, (n,) + (1,) * (a.ndim - 1)))).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=65536)
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    assert args.problems % BASE == 0
    h = native.Handle(0)
    prov = native.build_provenance()
    print(json.dumps({"bench": "provenance", "lib_src_hash": prov["lib_src_hash"],
                      "lib": os.path.basename(prov["lib"]), "matches_tree": prov["matches"],
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    Q, rep = args.queries, args.problems // BASE
    prob = P.make_batch(BASE, horizon=100, n_footsteps=6)
    tabs = P.foot_contact_tables(prob)
    cp = tiled(np.concatenate([tabs[f]["contact_pose"] for f in ("left", "right")]), rep)
    ct = tiled(np.concatenate([tabs[f]["contact_time"] for f in ("left", "right")]), rep)
    nc = tiled(np.concatenate([tabs[f]["ncontacts"] for f in ("left", "right")]), rep)
    L, C = cp.shape[0], cp.shape[1]
    # queries over the plan (0 .. 2.6 s at the default schedule): stance and swing samples mixed
    t_end = max(lst[-1][0] for lst in prob["schedule"].values()) * prob["dt"] + 0.2
    tq = (torch.arange(Q, dtype=torch.float64, device="cuda") * (t_end / Q)).repeat(L, 1).contiguous()
    out = {k: torch.empty(s, dtype=d, device="cuda") for k, s, d in (
        ("pose", (L, Q, 12), torch.float64), ("twist", (L, Q, 6), torch.float64),
        ("accel", (L, Q, 6), torch.float64), ("contact_idx", (L, Q), torch.int32),
        ("in_contact", (L, Q), torch.int32))}
    nbytes = L * Q * (8 + 200) + L * (C * 14 * 8 + 4)

    # quintic_eval at the same query count: the workload's swing splines, tiled
    kt, kp, _ = P.swing_splines(prob, queries=Q)
    S0 = kt.shape[0]
    assert L % S0 == 0
    ktd, kpd = tiled(kt, L // S0), tiled(kp, L // S0)
    tqs = (ktd[:, :1] + (ktd[:, 2:] - ktd[:, :1]) *
           torch.linspace(0, 1, Q, dtype=torch.float64, device="cuda")[None, :]).contiguous()
    coeffs = h.quintic_fit(ktd, kpd)
    qbytes = L * Q * (8 + 72 + 4) + L * (3 * 8 + 2 * 3 * 6 * 8)

    src = torch.empty(nbytes // 16, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    fill = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    res = compare({"swing_foot_eval": lambda: h.swing_foot_eval(cp, ct, nc, tq, out=out),
                   "torch_fill": lambda: fill.fill_(1.0),
                   "torch_copy": lambda: dst.copy_(src),
                   "quintic_eval": lambda: h.quintic_eval(ktd, coeffs, tqs)},
                  reps=args.reps, rounds=args.rounds)
    frac = lambda b, k: b / (res[k][0] * 1e-3) / PEAK   # noqa: E731
    swing = int((out["in_contact"] == 0).sum().item())
    print(json.dumps({"bench": "swing_foot_eval", "lists": L, "max_contacts": C, "queries": Q,
                      "ms": res["swing_foot_eval"], "algorithmic_bytes": nbytes,
                      "hbm_fraction": frac(nbytes, "swing_foot_eval"),
                      "torch_fill_same_bytes_ms": res["torch_fill"],
                      "torch_fill_hbm_fraction": frac(nbytes, "torch_fill"),
                      "torch_copy_same_bytes_ms": res["torch_copy"],
                      "torch_copy_hbm_fraction": frac(nbytes, "torch_copy"),
                      "quintic_eval_same_queries_ms": res["quintic_eval"],
                      "quintic_eval_algorithmic_bytes": qbytes,
                      "quintic_eval_hbm_fraction": frac(qbytes, "quintic_eval"),
                      "queries_not_in_contact": swing / (L * Q),
                      "finite": bool(torch.isfinite(out["pose"]).all())}), flush=True)

    # so3_eval: one trajectory per list (its first swing's two rotations), the same queries
    R0, R1 = cp[:, 0, 3:].contiguous(), cp[:, 1, 3:].contiguous()
    dur = torch.full((L,), 0.6, dtype=torch.float64, device="cuda")
    tqo = (torch.linspace(0, 0.6, Q, dtype=torch.float64, device="cuda")).repeat(L, 1).contiguous()
    so = {k: torch.empty((L, Q, w), dtype=torch.float64, device="cuda")
          for k, w in (("rot", 9), ("omega", 3), ("alpha", 3))}
    sbytes = L * Q * (8 + 120) + L * 19 * 8
    r2 = compare({"so3_eval": lambda: h.so3_eval(R0, R1, dur, tqo, out=so)}, reps=args.reps,
                 rounds=args.rounds)
    print(json.dumps({"bench": "so3_eval", "trajectories": L, "queries": Q, "ms": r2["so3_eval"],
                      "algorithmic_bytes": sbytes,
                      "hbm_fraction": sbytes / (r2["so3_eval"][0] * 1e-3) / PEAK,
                      "finite": bool(torch.isfinite(so["rot"]).all())}), flush=True)
    h.close()


if __name__ == "__main__":
    main()
