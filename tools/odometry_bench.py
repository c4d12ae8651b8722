"""Timing of blf_legged_odometry_advance at the closed loop's period (diagnostics; not the driver's
bench.py): B humanoid24 robots, K = 2 soles, T = 20 steps of 1 ms in one launch, against the yardstick
of T blf_fb_frame_state calls for the same K frames on the same states -- the kinematics-only work
the estimator cannot avoid.  HIP events around `reps` back-to-back calls after a warm-up, the two
variants alternating within each of `rounds` rounds, median / min / max.  One JSON line:

  odometry_ms, frame_state_ms (each [median, min, max] per T steps), their ratio, the algorithmic bytes
  of the odometry call (the sample stream in: joint_pos, joint_vel, normal_force; the outputs out:
  base_pos, base_rot, base_vel, contact_out, fixed_out; the estimator state in and out) and that
  over the time as a fraction of 8 TB/s.

  timeout -k 10 300 python tools/odometry_bench.py [--batch 16384] [--steps 20] [--rounds 7]
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
from blf import native, robot  # noqa: E402

PEAK = 8.0e12   # B/s


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def compare(variants, reps, rounds):
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, reps))
    return {k: [statistics.median(v), min(v), max(v)] for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    B, T, K = args.batch, args.steps, 2
    h = native.Handle(0)
    model = robot.humanoid24()
    n = model["n"]
    dm = h.fb_model(model)
    st = robot.standing_states(model, B, seed=1)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in st.items()}
    frames = torch.arange(K, dtype=torch.int32, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    q = dev["joint_pos"][None] + 0.02 * torch.randn(T, B, n, dtype=torch.float64, device="cuda", generator=gen)
    qd = 0.5 * torch.randn(T, B, n, dtype=torch.float64, device="cuda", generator=gen)
    # alternating feet with a double-support overlap: every robot switches its fixed foot in the period
    force = torch.zeros(T, B, K, dtype=torch.float64, device="cuda")
    force[: T // 2 + 2, :, 0] = 300.0
    force[T // 2 - 2:, :, 1] = 300.0
    time = 0.001 * torch.arange(1, T + 1, dtype=torch.float64, device="cuda")
    prm = np.array([50.0, 20.0, 0.002, 0.002])
    est0 = robot.odometry_init(dm, dev, frames, 0, handle=h)
    est0["trig_state"][:, 0] = 1
    est = {k: v.clone() for k, v in est0.items()}
    spec = dict(base_pos=(T, B, 3), base_rot=(T, B, 3, 3), base_vel=(T, B, 6))
    out = {k: torch.empty(s, dtype=torch.float64, device="cuda") for k, s in spec.items()}
    out.update(contact_out=torch.empty((T, B, K), dtype=torch.int32, device="cuda"),
               fixed_out=torch.empty((T, B), dtype=torch.int32, device="cuda"),
               status=torch.empty((B,), dtype=torch.int32, device="cuda"))
    pose = torch.empty((B, K, 12), dtype=torch.float64, device="cuda")
    twist = torch.empty((B, K, 6), dtype=torch.float64, device="cuda")
    states = [dict(dev, joint_pos=q[t], joint_vel=qd[t]) for t in range(T)]

    def odometry():
        h.legged_odometry(dm, frames, prm, time, q, qd, force, est, out=out)

    def frame_state():
        for t in range(T):
            h.fb_frame_state(dm, states[t], frames, pose=pose, twist=twist)

    res = compare({"odometry": odometry, "frame_state": frame_state}, args.reps, args.rounds)
    torch.cuda.synchronize()
    nbytes = B * (T * (8 * (2 * n + K) + 8 * 18 + 4 * K + 4) + 2 * (4 * K + 16 * K + 4 + 96) + 4)
    ms = res["odometry"][0]
    prov = native.build_provenance()
    print(json.dumps({"bench": "legged_odometry_advance", "device": torch.cuda.get_device_name(0),
                      "lib_src_hash": prov["lib_src_hash"], "matches_tree": prov["matches"], "batch": B, "steps": T,
                      "contacts": K, "odometry_ms": res["odometry"], "frame_state_ms": res["frame_state"],
                      "odometry_over_frame_state": ms / res["frame_state"][0], "algorithmic_bytes": nbytes,
                      "hbm_fraction": nbytes / (ms * 1e-3) / PEAK,
                      "switched": int((out["fixed_out"][-1] == 1).sum()), "ok": bool((out["status"] == 0).all())}),
          flush=True)
    h.close()


if __name__ == "__main__":
    main()
