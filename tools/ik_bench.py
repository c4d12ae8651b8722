"""Timing of the whole-body IK kernel (csrc/fb_ik.hip) on the humanoid's standing task set
(diagnostics; not the driver's bench.py).  HIP events around `reps` back-to-back calls after a
warm-up, median of `rounds` rounds, the variants alternating within a round.  One JSON line each:

  * blf_fb_ik_solve at B robots: time per call, the counted flops per robot (below) over time as a
    fraction of the vector fp64 peak;
  * blf_fb_ik_integrate with steps = 20 (the state restored before every call by a device copy,
    timed on its own and reported), and the unfused sequence it replaces: 20 x { blf_fb_ik_solve;
    blf_fbk_euler_integrate(0, dT, dT) with that nu }; the fused / unfused ratio;
  * as yardsticks at the same B, the two existing kernels the IK is assembled from:
    blf_fb_frame_state (the forward kinematics alone, one robot per wavefront) and blf_fbd_dynamics
    with mass_reg = zeros and no contacts (kinematics, mass matrix, the same Cholesky and
    substitutions, two robots per wavefront);
  * with --hard, in the same rounds: blf_fb_ik_solve_hard and blf_fb_ik_integrate_hard (steps = 20)
    with robot.standing_ik_hard (both soles and the CoM's x, y: 14 hard rows), and their ratio to the
    soft figures of the same run;
  * with --limits (implies --hard), in the same rounds: blf_fb_ik_solve_limits and
    blf_fb_ik_integrate_limits (steps = 20) with robot.humanoid24_joint_limits (sampling_time = dT) on
    the same task set with the CoM target 2 cm above the nominal height, which straight legs cannot
    reach, so both knees end on their lower bound; the hard calls on that raised task set, the ratio
    limits / hard of the same run, the mean iters, and from these the time of one further iteration;
  * with --track, instead of the above: B walking humanoids (robot.walking_ik_schedule, one cycle of
    `steps` steps, half the robots half a cycle apart) through swing_foot_eval and blf_fb_ik_track
    (section 12d; joint_traj and status requested), and in the same rounds: blf_fb_ik_track with every
    robot in the same phase (one mask per step for the whole batch: what the per-robot masks add);
    blf_fb_ik_integrate_limits over `steps` steps with a uniform mask (both soles and the CoM's x, y)
    and held set points, the fused call a user had before; blf_fb_ik_track on exactly that problem (no
    contact array, step 0's set points at every step: bit for bit the same arithmetic, section 12d's P2,
    so the ratio is the track kernel's own overhead); and the unfused route to per-step set
    points a user had before, `steps` x { blf_fb_ik_solve_limits with step t's set points and that
    uniform mask; blf_fbk_euler_integrate }.
  * with --closed-loop, instead of the above: blf_fbd_euler_integrate_impedance_traj on B standing
    humanoids over 19 steps of 1 ms, (a) with 4 identical slices and neither qd_ref nor q_bias against
    blf_fbd_euler_integrate_impedance with that reference (the same arithmetic, bit for bit: the ratio
    is the cost of the slice logic) and (b) with 4 distinct slices, qd_ref and q_bias; then (c) one
    period of blf.closed_loop.ClosedLoop(reference="ik") against one posture-mode period, both over
    two stream groups (events from the first launch to each group's last, the slower group counts),
    and blf_dcm_com_reference, blf_fb_ik_track and the trajectory dynamics each alone at B robots as
    shares of the IK period (the groups overlap, so the shares need not add up to 1).

Counted flops per robot-step, NV = n + 6, M = the task rows of non-zero weight: H and g from the task
rows M (NV (NV + 1) + 2 NV), the Cholesky factorization NV^3 / 3, the two substitutions 2 NV^2.  The
kinematics and the task rows themselves are not counted.  Both calls stage the shared weight arrays
to the host and wait for that copy before they launch (blf_c.h section 12), so every call here
includes one stream synchronisation: the unfused sequence pays 20 of them, the fused call one.

  timeout -k 10 600 python tools/ik_bench.py [--robots 16384] [--steps 20] [--rounds 5] [--hard] [--limits]
  timeout -k 10 600 python tools/ik_bench.py --track [--robots 16384] [--steps 20] [--rounds 5]
  timeout -k 10 600 python tools/ik_bench.py --closed-loop [--robots 16384] [--rounds 5] [--reps 3]
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
from blf import native, robot  # noqa: E402

FP64_PEAK = 78.6e12   # MI355X vector fp64, flop/s
DT = 0.01


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


def counted_flops(NV, M):
    return M * (NV * (NV + 1) + 2 * NV) + NV ** 3 / 3.0 + 2 * NV ** 2


def track_bench(h, args):
    """--track: blf_fb_ik_track on walking humanoids against the fused and unfused calls of section 12c."""
    B, T = args.robots, args.steps
    model = robot.humanoid24()
    n, K = model["n"], 2
    host = robot.standing_states(model, B, seed=1, spread=0.2)
    tasks = robot.standing_ik_tasks(model, host)
    dm = h.fb_model(model)
    lim = h.ik_limits(**robot.humanoid24_joint_limits(model, sampling_time=DT))
    comxy = h.ik_hard(com=(True, True, False))
    feet = h.ik_hard(**robot.standing_ik_hard(model))
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    start = {k: dev(host[k]) for k in native.FB_STATE_KEYS}
    st = {k: v.clone() for k, v in start.items()}

    def restore():
        for k in native.FB_STATE_KEYS:
            st[k].copy_(start[k])

    def schedule(shift):
        w = robot.walking_ik_schedule(model, host, T, DT, shift=shift)
        sw = h.swing_foot_eval(dev(w["contact_pose"]), dev(w["contact_time"]), dev(w["ncontacts"], torch.int32),
                               dev(w["tq"]), step_height=w["step_height"], outputs=("pose", "twist", "in_contact"))
        return sw, w, h.ik_schedule(B, K, T, stance_rows=w["stance_rows"], contact=sw["in_contact"],
                                    se3_pose=sw["pose"], se3_twist=sw["twist"], com_pos=w["com_pos"])

    sw, w, sc = schedule(np.arange(B) % 2 * 0.5)
    _, _, sc_same = schedule(np.zeros(B))
    hold = lambda a: a[:, :, :1].expand(-1, -1, T, -1).contiguous()
    sc_held = h.ik_schedule(B, K, T, se3_pose=hold(sw["pose"].reshape(B, K, T, 12)),
                            se3_twist=hold(sw["twist"].reshape(B, K, T, 6)),
                            com_pos=dev(np.repeat(w["com_pos"][:, :1], T, axis=1)))
    tk = h.ik_tasks(B, n, **dict(tasks, se3_pose=None, com_pos=None))
    # the calls a user had before: set points of step t as [B, ...] arrays of their own
    pose = sw["pose"].reshape(B, K, T, 12)
    twist = sw["twist"].reshape(B, K, T, 6)
    com = dev(w["com_pos"])
    tks = [h.ik_tasks(B, n, **dict(tasks, se3_pose=pose[:, :, t].contiguous(), se3_twist=twist[:, :, t].contiguous(),
                                   com_pos=com[:, t].contiguous())) for t in range(T)]
    jt = torch.empty((T, B, n), dtype=torch.float64, device="cuda")
    status = torch.empty((B,), dtype=torch.int32, device="cuda")
    fail = torch.empty((B,), dtype=torch.int32, device="cuda")
    iters = torch.zeros((B,), dtype=torch.int32, device="cuda")
    active = torch.zeros((B, 2), dtype=torch.int64, device="cuda")
    nu = torch.empty((B, n + 6), dtype=torch.float64, device="cuda")
    bv = torch.empty((B, 6), dtype=torch.float64, device="cuda")
    jv = torch.empty((B, n), dtype=torch.float64, device="cuda")

    def track(s=sc, hard=comxy):
        restore()
        h.fb_ik_track(dm, st, tk, s, DT, hard=hard, limits=lim, joint_traj=jt, base_traj=False, nu_traj=False,
                      status=status, fail_step=fail, iters=iters, active=active)

    def fused_uniform():
        restore()
        h.fb_ik_integrate(dm, st, tks[0], T, DT, nu=nu, status=status, hard=feet, limits=lim, iters=iters,
                          active=active)

    def unfused_uniform():
        restore()
        for t in range(T):
            h.fb_ik_solve(dm, st, tks[t], nu=nu, status=status, hard=feet, limits=lim, iters=iters, active=active)
            bv.copy_(nu[:, :6])
            jv.copy_(nu[:, 6:])
            h.fbk_euler_integrate(dm.c.rho, st["base_pos"], st["base_rot"], st["joint_pos"], bv, jv, 0.0, DT, DT)
            jt[t].copy_(st["joint_pos"])

    res = compare({"restore": restore, "track": track, "track_same_phase": lambda: track(sc_same),
                   "track_held_uniform": lambda: track(sc_held, feet),
                   "fused_uniform": fused_uniform, "unfused_uniform": unfused_uniform},
                  reps=args.reps, rounds=args.rounds)
    track()
    ok_t, it_t = bool((status == 0).all()), float(iters.double().mean()) / T
    nfail = int((fail >= 0).sum())
    track(sc_same)
    it_s = float(iters.double().mean()) / T
    track(sc_held, feet)
    held_jp = st["joint_pos"].clone()
    fused_uniform()
    ok_f, it_f = bool((status == 0).all()), float(iters.double().mean()) / T
    same = torch.equal(held_jp, st["joint_pos"])
    restore()
    it_u = 0.0
    for t in range(T):
        h.fb_ik_solve(dm, st, tks[t], nu=nu, status=status, hard=feet, limits=lim, iters=iters, active=active)
        it_u += float(iters.double().mean()) / T
        h.fbk_euler_integrate(dm.c.rho, st["base_pos"], st["base_rot"], st["joint_pos"], nu[:, :6].contiguous(),
                              nu[:, 6:].contiguous(), 0.0, DT, DT)
    r0 = res["restore"][0]
    net = {k: res[k][0] - r0 for k in ("track", "track_same_phase", "track_held_uniform", "fused_uniform",
                                       "unfused_uniform")}
    print(json.dumps({"bench": "fb_ik_track", "robots": B, "steps": T, "track_ms": res["track"],
                      "track_same_phase_ms": res["track_same_phase"],
                      "track_held_uniform_ms": res["track_held_uniform"], "fused_uniform_ms": res["fused_uniform"],
                      "track_held_over_fused_uniform_net": net["track_held_uniform"] / net["fused_uniform"],
                      "track_held_equals_fused_uniform_bitwise": same,
                      "mean_iters_per_step_same_phase": it_s, "mean_iters_per_step_unfused_uniform": it_u,
                      "unfused_uniform_ms": res["unfused_uniform"], "restore_ms": res["restore"],
                      "track_ms_per_step_net": net["track"] / T,
                      "track_over_fused_uniform_net": net["track"] / net["fused_uniform"],
                      "track_over_same_phase_net": net["track"] / net["track_same_phase"],
                      "track_over_unfused_uniform_net": net["track"] / net["unfused_uniform"],
                      "mean_iters_per_step_track": it_t, "mean_iters_per_step_fused_uniform": it_f,
                      "all_status_ok_track": ok_t, "failed_robots_track": nfail, "all_status_ok_fused_uniform": ok_f,
                      "label": args.label}), flush=True)


def closed_loop_bench(h, args):
    """--closed-loop: the trajectory impedance against the held-reference call, and one IK-mode period of
    blf.closed_loop.ClosedLoop against one posture-mode period (two stream groups)."""
    from blf import closed_loop as DL, problems as P
    B, T = args.robots, 4
    model = robot.humanoid24()
    n = model["n"]
    host = robot.standing_states(model, B, seed=3)
    law = robot.posture_law_arrays(model)
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    dm = h.fb_model(model)
    start = {k: dev(host[k]) for k in native.FB_STATE_KEYS}
    st = {k: v.clone() for k, v in start.items()}
    contacts = dict(frame=dev(np.arange(2), torch.int32), params=dev(np.tile(np.asarray(DL.CONTACT_PARAMS), (2, 1))),
                    null_pose=dev(robot.sole_null_poses(model, host)))
    imp = h.joint_impedance(law["kp"], law["kd"])
    rng = np.random.default_rng(4)
    q0 = dev(rng.normal(size=(B, n)) * 0.02)
    same = h.joint_impedance_traj(imp, q0[None].expand(T, -1, -1).contiguous(), 5)
    full = h.joint_impedance_traj(imp, dev(rng.normal(size=(T, B, n)) * 0.02), 5,
                                  qd_ref=dev(rng.uniform(-0.1, 0.1, (T, B, 6 + n))), qd_offset=6,
                                  q_bias=dev(rng.uniform(-0.01, 0.01, (B, n))))
    t1, dT = 0.019, 0.001   # 19 steps: one control period of the closed loop

    def restore():
        for k in native.FB_STATE_KEYS:
            st[k].copy_(start[k])

    def held():
        restore()
        h.fbd_euler_integrate_impedance(dm, st, imp, q0, 0.0, t1, dT, contacts=contacts)

    def traj(tr):
        restore()
        h.fbd_euler_integrate_impedance_traj(dm, st, tr, 0.0, t1, dT, contacts=contacts)

    res = compare({"restore": restore, "held": held, "traj_same": lambda: traj(same), "traj_full": lambda: traj(full)},
                  reps=args.reps, rounds=args.rounds)
    held()
    a = st["joint_vel"].clone()
    traj(same)
    r0 = res["restore"][0]
    net = {k: res[k][0] - r0 for k in ("held", "traj_same", "traj_full")}
    print(json.dumps({"bench": "impedance_traj", "robots": B, "steps": 19, "slices": T, "held_ms": res["held"],
                      "traj_identical_slices_ms": res["traj_same"], "traj_distinct_qd_bias_ms": res["traj_full"],
                      "restore_ms": res["restore"], "traj_identical_over_held_net": net["traj_same"] / net["held"],
                      "traj_distinct_over_held_net": net["traj_full"] / net["held"],
                      "traj_identical_equals_held_bitwise": torch.equal(a, st["joint_vel"]),
                      "label": args.label}), flush=True)
    # one period of the loop, both modes, two stream groups; reps periods per timing
    periods = 3 + args.rounds * args.reps
    plan = P.make_batch(B, horizon=100 + periods, n_footsteps=8, seed=P.SEED, first_ds=periods + 10)
    loops = {m: DL.split_groups(h, model, plan, host, 2, reference=m) for m in ("posture", "ik")}

    def run(mode, reps):
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for g in loops[mode]:
            g.stream.wait_event(e0)
        for _ in range(reps):
            for g in loops[mode]:
                g.period()
        ends = []
        for g in loops[mode]:
            e = torch.cuda.Event(enable_timing=True)
            e.record(g.stream)
            ends.append(e)
        torch.cuda.synchronize()
        return max(e0.elapsed_time(e) for e in ends) / reps

    for m in loops:
        run(m, 3)
    times = {m: [] for m in loops}
    for _ in range(args.rounds):
        for m in loops:
            times[m].append(run(m, args.reps))
    med = {m: [statistics.median(v), min(v), max(v)] for m, v in times.items()}
    # the IK period's own pieces, each alone on the default stream at all B robots (the loop's buffers)
    one = DL.ClosedLoop(h, model, plan, host, reference="ik")
    one.period()
    out = one.bufs[0]
    pieces = compare({
        "com_reference": lambda: h.dcm_com_reference(one.xi, out["vrp"], one.omega, one.z_ref, one.c_ref, one.ik_steps,
                                                     one.ik_dT, column=1, com_pos=one.com_pos, com_vel=one.com_vel,
                                                     xi_end=one.xi_end),
        "fb_ik_track": lambda: h.fb_ik_track(one.dm, one.ik_state, one.ik_tasks, one.ik_schedule, one.ik_dT,
                                             hard=one.ik_hard, limits=one.ik_limits, joint_traj=one.joint_traj,
                                             base_traj=False, nu_traj=one.nu_traj, status=one.ik_status,
                                             fail_step=one.ik_fail_step, iters=one.ik_iters, active=one.ik_active),
        "dynamics_traj": lambda: h.fbd_euler_integrate_impedance_traj(one.dm, one.state, one.traj, 0.0, one.T, one.dT,
                                                                      contacts=one.contacts)},
        reps=1, rounds=args.rounds)
    ik_ok = all(bool((g.ik_status == 0).all()) for g in loops["ik"])
    finite = all(bool(torch.isfinite(g.state["joint_pos"]).all()) for g in loops["ik"])
    print(json.dumps({"bench": "closed_loop_ik_period", "robots": B, "groups": 2, "periods_per_mode": periods,
                      "posture_period_ms": med["posture"], "ik_period_ms": med["ik"],
                      "ik_over_posture": med["ik"][0] / med["posture"][0],
                      "alone_ms": {k: v for k, v in pieces.items()},
                      "share_of_ik_period": {k: v[0] / med["ik"][0] for k, v in pieces.items()},
                      "all_ik_status_ok": ik_ok, "states_finite": finite, "label": args.label}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--closed-loop", action="store_true",
                    help="time the trajectory impedance and the closed loop's IK period instead")
    ap.add_argument("--robots", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--hard", action="store_true", help="also time the hard-task calls (section 12b)")
    ap.add_argument("--limits", action="store_true", help="also time the joint-limit calls (section 12c)")
    ap.add_argument("--track", action="store_true", help="time blf_fb_ik_track (section 12d) instead")
    args = ap.parse_args()
    args.hard = args.hard or args.limits
    assert torch.cuda.is_available(), "needs a HIP device"
    h = native.Handle(0)
    prov = native.build_provenance()
    print(json.dumps({"bench": "provenance", "lib_src_hash": prov["lib_src_hash"],
                      "lib": os.path.basename(prov["lib"]), "matches_tree": prov["matches"],
                      "device": torch.cuda.get_device_name(0), "label": args.label}), flush=True)
    if args.track or args.closed_loop:
        (closed_loop_bench if args.closed_loop else track_bench)(h, args)
        h.close()
        return
    B, steps = args.robots, args.steps
    model = robot.humanoid24()
    n = model["n"]
    NV = n + 6
    host = robot.standing_states(model, B, seed=1, spread=0.2)
    host["joint_pos"] = host["joint_pos"] + np.random.default_rng(2).normal(size=(B, n)) * 0.05
    tasks = robot.standing_ik_tasks(model, host)
    M = int((tasks["se3_weight"] > 0).sum() + (tasks["com_weight"] > 0).sum())
    dm = h.fb_model(model)
    tk = h.ik_tasks(B, n, **tasks)
    start = {k: torch.from_numpy(np.ascontiguousarray(host[k])).cuda() for k in native.FB_STATE_KEYS}
    st = {k: v.clone() for k, v in start.items()}
    nu = torch.empty((B, NV), dtype=torch.float64, device="cuda")
    status = torch.empty((B,), dtype=torch.int32, device="cuda")
    twist = torch.empty((B, 6), dtype=torch.float64, device="cuda")
    jv = torch.empty((B, n), dtype=torch.float64, device="cuda")

    def restore():
        for k in native.FB_STATE_KEYS:
            st[k].copy_(start[k])

    def fused():
        restore()
        h.fb_ik_integrate(dm, st, tk, steps, DT, nu=nu, status=status)

    def unfused():
        restore()
        for _ in range(steps):
            h.fb_ik_solve(dm, st, tk, nu=nu, status=status)
            twist.copy_(nu[:, :6])
            jv.copy_(nu[:, 6:])
            h.fbk_euler_integrate(dm.c.rho, st["base_pos"], st["base_rot"], st["joint_pos"], twist, jv, 0.0, DT, DT)

    frames = torch.arange(len(model["frame_link"]), dtype=torch.int32, device="cuda")
    fpose = torch.empty((B, frames.shape[0], 12), dtype=torch.float64, device="cuda")
    ftwist = torch.empty((B, frames.shape[0], 6), dtype=torch.float64, device="cuda")
    tau = torch.zeros((B, n), dtype=torch.float64, device="cuda")
    reg = torch.zeros((NV, NV), dtype=torch.float64, device="cuda")
    variants = {"solve": lambda: h.fb_ik_solve(dm, start, tk, nu=nu, status=status), "restore": restore,
                "fused": fused, "unfused": unfused,
                "frame_state": lambda: h.fb_frame_state(dm, start, frames, pose=fpose, twist=ftwist),
                "fbd_dynamics_reg": lambda: h.fbd_dynamics(dm, start, tau, mass_reg=reg)}
    if args.hard:
        hard = h.ik_hard(**robot.standing_ik_hard(model))

        def fused_hard():
            restore()
            h.fb_ik_integrate(dm, st, tk, steps, DT, nu=nu, status=status, hard=hard)

        variants["solve_hard"] = lambda: h.fb_ik_solve(dm, start, tk, nu=nu, status=status, hard=hard)
        variants["fused_hard"] = fused_hard
    if args.limits:
        raised = dict(tasks, com_pos=tasks["com_pos"] + np.array([0.0, 0.0, 0.02]))
        tkr = h.ik_tasks(B, n, **raised)
        lim = h.ik_limits(**robot.humanoid24_joint_limits(model, sampling_time=DT))
        iters = torch.zeros((B,), dtype=torch.int32, device="cuda")
        active = torch.zeros((B, 2), dtype=torch.int64, device="cuda")

        def fused_raised(limits=None):
            restore()
            h.fb_ik_integrate(dm, st, tkr, steps, DT, nu=nu, status=status, hard=hard, limits=limits, iters=iters,
                              active=active)

        variants["solve_hard_raised"] = lambda: h.fb_ik_solve(dm, start, tkr, nu=nu, status=status, hard=hard)
        variants["solve_limits"] = lambda: h.fb_ik_solve(dm, start, tkr, nu=nu, status=status, hard=hard,
                                                         limits=lim, iters=iters, active=active)
        variants["fused_hard_raised"] = fused_raised
        variants["fused_limits"] = lambda: fused_raised(lim)
    res = compare(variants, reps=args.reps, rounds=args.rounds)
    fused()
    f_state = {k: v.clone() for k, v in st.items()}
    ok_f = bool((status == 0).all())
    unfused()
    same = all(torch.equal(f_state[k], st[k]) for k in ("base_pos", "base_rot", "joint_pos"))
    fl = counted_flops(NV, M)
    print(json.dumps({"bench": "fb_ik_solve", "robots": B, "ndof": n, "task_rows": M, "ms": res["solve"],
                      "counted_flops_per_robot_step": fl,
                      "fp64_fraction": B * fl / (res["solve"][0] * 1e-3) / FP64_PEAK,
                      "fb_frame_state_ms": res["frame_state"], "fbd_dynamics_mass_reg_ms": res["fbd_dynamics_reg"],
                      "label": args.label}), flush=True)
    f_ms = res["fused"][0] - res["restore"][0]
    u_ms = res["unfused"][0] - res["restore"][0]
    print(json.dumps({"bench": "fb_ik_integrate", "robots": B, "steps": steps, "fused_ms": res["fused"],
                      "unfused_ms": res["unfused"], "restore_ms": res["restore"],
                      "fused_ms_per_step_net": f_ms / steps, "fused_over_unfused_net": f_ms / u_ms,
                      "fp64_fraction_fused": B * steps * fl / (f_ms * 1e-3) / FP64_PEAK,
                      "fused_equals_unfused_bitwise": same, "all_status_ok": ok_f,
                      "label": args.label}), flush=True)
    if args.hard:
        fused_hard()
        ok_h = bool((status == 0).all())
        h_ms = res["fused_hard"][0] - res["restore"][0]
        print(json.dumps({"bench": "fb_ik_hard", "robots": B, "steps": steps,
                          "hard_rows": bin(hard.rows).count("1"), "solve_hard_ms": res["solve_hard"],
                          "fused_hard_ms": res["fused_hard"], "solve_hard_over_soft": res["solve_hard"][0] / res["solve"][0],
                          "fused_hard_over_soft_net": h_ms / f_ms, "fused_hard_ms_per_step_net": h_ms / steps,
                          "all_status_ok": ok_h, "label": args.label}), flush=True)
    if args.limits:
        variants["solve_limits"]()
        ok_s, it_s = bool((status == 0).all()), float(iters.double().mean())
        held = float(((active[:, 0] != 0) | (active[:, 1] != 0)).double().mean())
        variants["fused_limits"]()
        ok_l, it_l = bool((status == 0).all()), float(iters.double().mean()) / steps
        hr_ms = res["fused_hard_raised"][0] - res["restore"][0]
        l_ms = res["fused_limits"][0] - res["restore"][0]
        ds = res["solve_limits"][0] - res["solve_hard_raised"][0]
        print(json.dumps({"bench": "fb_ik_limits", "robots": B, "steps": steps,
                          "solve_hard_raised_ms": res["solve_hard_raised"], "solve_limits_ms": res["solve_limits"],
                          "fused_hard_raised_ms": res["fused_hard_raised"], "fused_limits_ms": res["fused_limits"],
                          "solve_limits_over_hard": res["solve_limits"][0] / res["solve_hard_raised"][0],
                          "fused_limits_over_hard_net": l_ms / hr_ms, "mean_iters_solve": it_s,
                          "mean_iters_per_fused_step": it_l, "robots_with_a_bound_active": held,
                          "ms_per_further_iteration_solve": ds / (it_s - 1.0) if it_s > 1.0 else None,
                          "ms_per_further_iteration_fused_step": ((l_ms - hr_ms) / steps / (it_l - 1.0)
                                                                  if it_l > 1.0 else None),
                          "all_status_ok": ok_s and ok_l, "label": args.label}), flush=True)
    h.close()


if __name__ == "__main__":
    main()
