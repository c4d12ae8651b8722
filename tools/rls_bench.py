"""Timing of the recursive-least-squares kernels at the closed loop's contact count (diagnostics;
not the driver's bench.py).  HIP events around `reps` back-to-back calls after a warm-up, median of
`rounds` rounds, the variants of one comparison alternating within a round.  One JSON line each:

  * rls_advance for (n, m) = (2, 6) and (8, 8) at T = 1 and T = 64: time per call, algorithmic
    bytes (every step's regressor and measurements in, state and covariance in and out) over time
    as a fraction of 8 TB/s, and torch's device copy of the same number of bytes (half read, half
    written) beside it;
  * contact_rls_advance (fused) against the unfused sequence (T blf_contact_model_eval calls that
    write the step's regressor, then one blf_rls_advance over the T steps), at T = 1 and T = 64.

  timeout -k 10 600 python tools/rls_bench.py [--batch 32768] [--rounds 5] [--only rls|contact]
(BLF_LIB=.../lib/libblf_<name>.so times a variant build, tools/build_variant.sh)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bipedal-locomotion-framework_amd"))

import torch  # noqa: E402
from blf import native  # noqa: E402

PEAK = 8.0e12   # B/s


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


def rnd(*shape, gen):
    return torch.randn(*shape, dtype=torch.float64, device="cuda", generator=gen)


def bench_rls(h, B, n, m, T, rounds, gen):
    H, Y = rnd(T, B, m, n, gen=gen), rnd(T, B, m, gen=gen)
    r = torch.full((m,), 0.5, dtype=torch.float64, device="cuda")
    x = torch.zeros(B, n, dtype=torch.float64, device="cuda")
    P = (10.0 * torch.eye(n, dtype=torch.float64, device="cuda")).repeat(B, 1, 1).contiguous()
    nbytes = 8 * B * (T * (m * n + m) + 2 * (n + n * n))
    src = torch.empty(nbytes // 16, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    res = compare({"rls_advance": lambda: h.rls_advance(H, Y, x, P, r),
                   "torch_copy": lambda: dst.copy_(src)},
                  reps=200 if T == 1 else 20, rounds=rounds)
    ms = res["rls_advance"][0]
    print(json.dumps({"bench": "rls_advance", "batch": B, "n": n, "m": m, "steps": T,
                      "ms": res["rls_advance"], "algorithmic_bytes": nbytes,
                      "hbm_fraction": nbytes / (ms * 1e-3) / PEAK,
                      "torch_copy_same_bytes_ms": res["torch_copy"],
                      "torch_copy_hbm_fraction": nbytes / (res["torch_copy"][0] * 1e-3) / PEAK,
                      "finite": bool(torch.isfinite(x).all())}), flush=True)


def bench_contact(h, B, T, rounds, gen):
    L = native.lib()
    vp = ctypes.c_void_p
    twist = torch.rand(T, B, 6, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    q = torch.linalg.qr(rnd(T, B, 3, 3, gen=gen))[0].contiguous()
    q0 = torch.linalg.qr(rnd(B, 3, 3, gen=gen))[0].contiguous()
    pose = torch.cat([0.02 * rnd(T, B, 3, gen=gen), q.reshape(T, B, 9)], dim=2).contiguous()
    null = torch.cat([0.02 * rnd(B, 3, gen=gen), q0.reshape(B, 9)], dim=1).contiguous()
    geometry = torch.tensor([0.12, 0.09], dtype=torch.float64, device="cuda")
    prm = torch.tensor([0.12, 0.09, 2000.0, 100.0], dtype=torch.float64, device="cuda")
    wrench = rnd(T, B, 6, gen=gen)
    r = torch.ones(6, dtype=torch.float64, device="cuda")
    reg = torch.empty(T, B, 6, 2, dtype=torch.float64, device="cuda")

    def state():
        return (torch.zeros(B, 2, dtype=torch.float64, device="cuda"),
                (1e6 * torch.eye(2, dtype=torch.float64, device="cuda")).repeat(B, 1, 1).contiguous())

    xf, Pf = state()
    xu, Pu = state()
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def fused():
        h.contact_rls_advance(geometry, twist, pose, null, wrench, xf, Pf, r)

    def unfused():
        for t in range(T):
            native._check(L.blf_contact_model_eval(
                h.ptr, vp(prm.data_ptr()), 1, vp(twist[t].data_ptr()), vp(pose[t].data_ptr()),
                vp(null.data_ptr()), B, None, None, None, vp(reg[t].data_ptr()), stream))
        h.rls_advance(reg, wrench, xu, Pu, r)

    res = compare({"fused": fused, "unfused": unfused}, reps=200 if T == 1 else 10, rounds=rounds)
    torch.cuda.synchronize()
    print(json.dumps({"bench": "contact_rls_advance", "batch": B, "steps": T, "fused_ms": res["fused"],
                      "unfused_ms": res["unfused"],
                      "speedup": res["unfused"][0] / res["fused"][0],
                      "bit_equal": bool(torch.equal(xf, xu) and torch.equal(Pf, Pu))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["rls", "contact"], default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    h = native.Handle(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    prov = native.build_provenance()
    print(json.dumps({"bench": "provenance", "lib_src_hash": prov["lib_src_hash"],
                      "lib": os.path.basename(prov["lib"]), "matches_tree": prov["matches"],
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    if args.only != "contact":
        for (n, m) in ((2, 6), (8, 8)):
            for T in (1, 64):
                bench_rls(h, args.batch, n, m, T, args.rounds, gen)
    if args.only != "rls":
        for T in (1, 64):
            bench_contact(h, args.batch, T, args.rounds, gen)
    h.close()


if __name__ == "__main__":
    main()
