"""Generates tests/golden/fb_refusals.json: what the 15 floating-base entry points of include/blf/blf_c.h
answer to calls they refuse before any HIP call, and to their accepted empty-batch calls.  Each row
holds the entry point, a label, the arguments that differ from the accepted empty-batch call (the
encoding of tests/fb_refusal_calls.py), the status and the complete blf_last_error() text of the library
the script ran against; `library` is that library's blf_version().  tests/test_fb_refusals.py holds every
later library to the table, text for text.

Per entry point: one row for every argument check with one defect (one per pointer where a check names
several), and rows with two defects at once for checks that follow each other, which fix the check
that reports first.  The checks behind a staged copy of device arrays (the weights' and limits'
values, hard and stance rows of weight 0, the outputs of the IK calls when batch > 0) need a device
and stay with the GPU tests.  The "model too large for one workgroup's LDS" refusals cannot be reached:
the largest model the size checks admit (48 joints, 8 contacts, 4 SE3 tasks) fits.

Run it against a library built from the commit whose behaviour is to be pinned:

    python tests/golden/make_fb_refusals.py
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "bipedal-locomotion-framework_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fb_refusal_calls as RC  # noqa: E402
from blf import native  # noqa: E402

PTR = "ptr"
STATE = ("base_vel", "joint_vel", "base_pos", "base_rot", "joint_pos")
POSITIONS = STATE[2:]
BAD_DT = (0.0, -0.01, "nan", "inf")


def join(*parts):
    out = {}
    for p in parts:
        out.update(p)
    return out


def model_state(ndof, before_arrays):
    """The handle / model / state / batch / ndof / model-array checks every entry point starts with.
    ndof(n): the arguments that give the model n joints (a law struct must agree).  before_arrays: the
    arguments whose checks come between the model / state pointers and the model arrays."""
    rows = [("null handle", {"handle": None}), ("null model", {"model": None}), ("null state", {"state": None}),
            ("ndof 0", ndof(0)), ("ndof 49", ndof(49)), ("ndof -1", ndof(-1)), ("negative batch", {"batch": -1})]
    rows += [(f"null model.{k}", {f"model.{k}": None}) for k in RC.MODEL_ARRAYS]
    rows += [("null handle + null model", {"handle": None, "model": None}),
             ("null handle + null state", {"handle": None, "state": None}),
             ("null handle + negative batch", {"handle": None, "batch": -1}),
             ("null handle + ndof 49", join({"handle": None}, ndof(49))),
             ("null state + negative batch", {"state": None, "batch": -1}),
             ("negative batch + ndof 49", join({"batch": -1}, ndof(49))),
             ("negative batch + null model array", {"batch": -1, "model.parent": None}),
             ("ndof 49 + null model array", join(ndof(49), {"model.link_inertia": None}))]
    for label, a in before_arrays:
        rows += [(f"{label} + negative batch", join(a, {"batch": -1})),
                 (f"{label} + ndof 49", join(a, ndof(49))),
                 (f"{label} + null model array", join(a, {"model.joint_axis": None}))]
    return rows


CONTACTS2 = {"contacts.ncontacts": 2, "contacts.frame": PTR, "contacts.params": PTR, "contacts.null_pose": PTR,
             "model.frame_link": PTR, "model.frame_pose": PTR, "model.nframes": 4}
CONTACT_BUFFERS = ("contacts.frame", "contacts.params", "contacts.null_pose", "model.frame_link", "model.frame_pose")


def contacts(ndof, running, after):
    """The contact block of the dynamics calls.  running: the arguments of a batch-of-2 call that passes
    every check before the contacts; after: (label, arguments) of the check that follows the block."""
    laws = join(running, CONTACTS2, {"contacts.law": PTR})
    rows = [("accepted: null contacts struct", {"contacts": None}),
            ("accepted: 2 contacts, empty batch", CONTACTS2),
            ("9 contacts", {"contacts.ncontacts": 9}), ("-1 contacts", {"contacts.ncontacts": -1})]
    rows += [(f"null {k}", join(CONTACTS2, {k: None})) for k in CONTACT_BUFFERS]
    rows += [("contacts, model without frames", join(CONTACTS2, {"model.nframes": 0})),
             ("laws without wrench", laws),
             ("accepted: laws without wrench, empty batch", join(CONTACTS2, {"contacts.law": PTR})),
             ("null model array + 9 contacts", {"model.parent": None, "contacts.ncontacts": 9}),
             ("null state buffer + 9 contacts", {"batch": 2, "contacts.ncontacts": 9}),
             ("null state buffer + -1 contacts", {"batch": 2, "contacts.ncontacts": -1}),
             ("-1 contacts + ndof 49", join({"contacts.ncontacts": -1}, ndof(49))),
             ("9 contacts + ndof 49", join({"contacts.ncontacts": 9}, ndof(49))),
             ("9 contacts + ndof 0", join({"contacts.ncontacts": 9}, ndof(0))),
             ("9 contacts + null contact buffer", {"contacts.ncontacts": 9, "contacts.frame": None}),
             ("-1 contacts + null contact buffer", {"contacts.ncontacts": -1, "contacts.frame": None}),
             ("null contact buffer + laws without wrench", join(laws, {"contacts.params": None})),
             (f"9 contacts + {after[0]}", join({"contacts.ncontacts": 9}, after[1])),
             (f"null contact buffer + {after[0]}", join(CONTACTS2, {"contacts.null_pose": None}, after[1])),
             (f"laws without wrench + {after[0]}", join(laws, after[1]))]
    return rows


def state_buffers(running, names, extra=()):
    """One null state buffer (or one of `extra`, the pointers the same check names) in a batch of 2."""
    return [(f"null {k}", join(running, {k: None})) for k in [f"state.{n}" for n in names] + list(extra)]


def schedule():
    """step_schedule's refusals, reached with an empty batch."""
    return [("final time before the initial one", {"initial_time": 1.0, "final_time": 0.5}),
            ("dT 0", {"dT": 0.0}), ("dT negative", {"dT": -0.001}), ("dT nan", {"dT": "nan"}),
            ("empty interval", {"initial_time": 0.25, "final_time": 0.25}),
            ("too many steps", {"final_time": 1.0e9, "dT": 1.0e-9}),
            ("initial time nan", {"initial_time": "nan"}),
            ("final time before + dT 0", {"initial_time": 1.0, "final_time": 0.5, "dT": 0.0}),
            ("dT 0 + empty interval", {"initial_time": 0.25, "final_time": 0.25, "dT": 0.0}),
            ("null handle + final time before", {"handle": None, "initial_time": 1.0, "final_time": 0.5}),
            ("negative batch + dT 0", {"batch": -1, "dT": 0.0})]


BACKWARDS = ("final time before the initial one", {"initial_time": 1.0, "final_time": 0.5})


def law_rows(name, traj, ndof):
    """The struct checks of the impedance, impedance-trajectory and computed-torque calls."""
    rows = [(f"null {name}", {name: None}), ("reserved 1", {f"{name}.reserved": 1}),
            ("null kp", {f"{name}.kp": None}), ("null kd", {f"{name}.kd": None}),
            ("null q_ref", {"batch": 2, "state.*": PTR}), ("law ndof 4", {f"{name}.ndof": 4}),
            ("model ndof 4", {"model.ndof": 4}),
            (f"null {name} + null handle", {name: None, "handle": None}),
            ("reserved 1 + null kp", {f"{name}.reserved": 1, f"{name}.kp": None}),
            ("reserved 1 + null handle", {f"{name}.reserved": 1, "handle": None}),
            ("null kd + law ndof 4", {f"{name}.kd": None, f"{name}.ndof": 4}),
            ("null q_ref + null model", {"batch": 2, "model": None}),
            ("law ndof 4 + null handle", {f"{name}.ndof": 4, "handle": None}),
            ("law ndof 4 + negative batch", {f"{name}.ndof": 4, "batch": -1})]
    if traj:
        rows += [("slices 0", {f"{name}.slices": 0}), ("steps_per_slice 0", {f"{name}.steps_per_slice": 0}),
                 ("qd_stride below ndof", {f"{name}.qd_ref": PTR, f"{name}.qd_stride": 2}),
                 ("accepted: qd_ref with qd_stride = ndof", {f"{name}.qd_ref": PTR, f"{name}.qd_stride": 3}),
                 ("reserved 1 + slices 0", {f"{name}.reserved": 1, f"{name}.slices": 0}),
                 ("slices 0 + null kp", {f"{name}.slices": 0, f"{name}.kp": None}),
                 ("law ndof 4 + qd_stride below ndof",
                  {f"{name}.ndof": 4, f"{name}.qd_ref": PTR, f"{name}.qd_stride": 2}),
                 ("qd_stride below ndof + null handle",
                  {f"{name}.qd_ref": PTR, f"{name}.qd_stride": 2, "handle": None}),
                 ("qd_stride below ndof + ndof 49",
                  join(ndof(49), {f"{name}.qd_ref": PTR, f"{name}.qd_stride": 2}))]
    return rows


def fbd(entry):
    """blf_fbd_dynamics and the four Euler integrations."""
    law = {"blf_fbd_euler_integrate_impedance": "impedance", "blf_fbd_euler_integrate_impedance_traj": "impedance",
           "blf_fbd_euler_integrate_computed_torque_traj": "law"}.get(entry)
    ctq = law == "law"
    ndof = (lambda n: {"model.ndof": n, f"{law}.ndof": n}) if law else (lambda n: {"model.ndof": n})
    running = {"batch": 2, "state.*": PTR}
    running.update({f"{law}.q_ref": PTR} if law else {"joint_torque": PTR})
    if entry == "blf_fbd_dynamics":
        after = ("null out", {"out": None})
    elif ctq:
        after = ("mass_reg", {"mass_reg": PTR})
    else:
        after = BACKWARDS
    rows = [("accepted: empty batch", {})]
    if law:
        rows += law_rows(law, entry != "blf_fbd_euler_integrate_impedance", ndof)
    if ctq:
        rows += [("qdd_stride below ndof", {"law.qdd_ref": PTR, "law.qdd_stride": 2}),
                 ("qd_stride + qdd_stride below ndof",
                  {"law.qd_ref": PTR, "law.qd_stride": 2, "law.qdd_ref": PTR, "law.qdd_stride": 1}),
                 ("qdd_stride below ndof + null handle", {"law.qdd_ref": PTR, "law.qdd_stride": 2, "handle": None})]
    rows += model_state(ndof, [])
    rows += state_buffers(running, STATE, () if law else ("joint_torque",))
    rows += [("null model array + null state buffer", {"batch": 2, "model.link_mass": None}),
             ("ndof 49 + null state buffer", join(ndof(49), {"batch": 2}))]
    rows += contacts(ndof, running, after)
    if entry == "blf_fbd_dynamics":
        rows += [("null out", {"out": None})]
        rows += [(f"null out.{k}", join(running, {"out.*": PTR, f"out.{k}": None})) for k in STATE]
        rows += [("null state buffer + null out", {"batch": 2, "out": None})]
    else:
        if ctq:
            rows += [("mass_reg", {"mass_reg": PTR}), ("mass_reg + ndof 49", join({"mass_reg": PTR}, ndof(49))),
                     ("mass_reg + null handle", {"mass_reg": PTR, "handle": None}),
                     ("mass_reg + final time before", join({"mass_reg": PTR}, BACKWARDS[1]))]
        rows += schedule()
    if law:
        # these calls require the law's q_ref whenever batch != 0, before every check of the shared rows:
        # the rows that are not about q_ref itself give it
        rows = [(label, a if a.get("batch", 0) == 0 or "null q_ref" in label else join({f"{law}.q_ref": PTR}, a))
                for label, a in rows]
    return rows


def inverse_dynamics():
    ndof = lambda n: {"model.ndof": n}
    running = {"batch": 2, "state.*": PTR}
    rows = [("accepted: empty batch", {}), ("reserved 1", {"reserved": 1}),
            ("reserved 1 + null handle", {"reserved": 1, "handle": None})]
    rows += model_state(ndof, [])
    rows += state_buffers(running, STATE)
    rows += [("null model array + null state buffer", {"batch": 2, "model.link_mass": None}),
             ("ndof 49 + null state buffer", join(ndof(49), {"batch": 2}))]
    rows += contacts(ndof, running, ("null joint_torque", join(running, {"base_acc_out": PTR})))
    rows += [("null joint_torque", join(running, {"base_acc_out": PTR, "base_wrench": PTR})),
             ("null joint_torque and outputs", running),
             ("null base_acc_out (free base)", join(running, {"joint_torque": PTR, "base_wrench": PTR})),
             ("null base_wrench (given base)", join(running, {"joint_torque": PTR, "base_acc": PTR,
                                                              "base_acc_out": PTR}))]
    return rows


def dcm():
    ndof = lambda n: {"model.ndof": n}
    running = {"batch": 2, "state.*": PTR, "com": PTR}
    rows = [("accepted: empty batch", {}), ("accepted: empty batch, xi with omega0", {"xi": PTR, "omega0": PTR})]
    rows += model_state(ndof, [])
    rows += state_buffers(running, STATE, ("com",))
    rows += [("xi without omega0", {"xi": PTR}), ("negative omega0 stride", {"omega0_stride": -1}),
             ("null model array + null state buffer", {"batch": 2, "model.link_mass": None}),
             ("null state buffer + xi without omega0", {"batch": 2, "xi": PTR}),
             ("xi without omega0 + negative omega0 stride", {"xi": PTR, "omega0_stride": -1})]
    return rows


def frame_state():
    ndof = lambda n: {"model.ndof": n}
    frames = {"nframes": 2, "frames": PTR, "model.frame_link": PTR, "model.frame_pose": PTR, "model.nframes": 4}
    running = join(frames, {"batch": 2, "state.*": PTR})
    rows = [("accepted: empty batch", {}), ("accepted: empty batch, 2 frames", frames),
            ("accepted: no frames, batch of 2", {"batch": 2})]
    rows += model_state(ndof, [("negative nframes", {"nframes": -1})])
    rows += [("negative nframes", {"nframes": -1})]
    rows += [(f"null {k}", join(frames, {k: None})) for k in ("frames", "model.frame_link", "model.frame_pose")]
    rows += [("frames, model without frames", join(frames, {"model.nframes": 0}))]
    rows += state_buffers(join(running, {"pose": PTR}), STATE)
    rows += [("null pose and twist", running),
             ("null model array + null frame buffer", join(frames, {"model.parent": None, "frames": None})),
             ("null frame buffer + null state buffer", join(frames, {"batch": 2, "frames": None}))]
    return rows


SE3 = {"tasks.nse3": 1, "tasks.frame": PTR, "tasks.se3_weight": PTR, "tasks.se3_kp": PTR, "model.frame_link": PTR,
       "model.frame_pose": PTR, "model.nframes": 4}
COM_ROWS = {"hard.rows": 1 << 24}


def ik(entry):
    ndof = lambda n: {"model.ndof": n}
    track = entry == "blf_fb_ik_track"
    hard = track or "hard" in entry or "limits" in entry
    limits = track or "limits" in entry
    stepped = "integrate" in entry
    rows = [("accepted: empty batch", {}), ("accepted: empty batch, one SE3 and a CoM task",
                                            join(SE3, {"tasks.com_weight": PTR, "tasks.com_kp": 2.0}))]
    first = []   # the checks in front of the shared ones
    if stepped:
        first = [("steps 0", {"steps": 0})] + [(f"dT {v}", {"dT": v}) for v in BAD_DT]
        rows += first + [("steps -1", {"steps": -1}), ("steps 0 + dT 0", {"steps": 0, "dT": 0.0})]
    if track:
        first = [("null schedule", {"schedule": None}), ("schedule steps 0", {"schedule.steps": 0}),
                 ("schedule reserved 1", {"schedule.reserved": 1}), ("schedule reserved2 1", {"schedule.reserved2": 1})]
        first += [(f"dT {v}", {"dT": v}) for v in BAD_DT]
        rows += first + [("schedule steps 0 + reserved 1", {"schedule.steps": 0, "schedule.reserved": 1}),
                         ("schedule reserved2 1 + dT 0", {"schedule.reserved2": 1, "dT": 0.0})]
    rows += [(f"{label} + null handle", join(a, {"handle": None})) for label, a in first[:1] + first[-1:]]
    rows += model_state(ndof, [("null tasks", {"tasks": None}), ("tasks reserved 1", {"tasks.reserved": 1})])
    rows += [("null tasks", {"tasks": None}), ("tasks reserved 1", {"tasks.reserved": 1}),
             ("nse3 -1", {"tasks.nse3": -1}), ("nse3 5", {"tasks.nse3": 5})]
    rows += [(f"null {k}", join(SE3, {k: None})) for k in SE3 if k not in ("tasks.nse3", "model.nframes")]
    rows += [("SE3 task, model without frames", join(SE3, {"model.nframes": 0})),
             ("null joint_weight", {"tasks.joint_weight": None}), ("null joint_kp", {"tasks.joint_kp": None})]
    rows += [(f"base_damping {v}", {"tasks.base_damping": v}) for v in (-1.0, "nan", "inf")]
    rows += [(f"com_kp {v}", {"tasks.com_weight": PTR, "tasks.com_kp": v}) for v in (-1.0, "nan", "inf")]
    rows += [("accepted: com_kp -1 without a CoM task", {"tasks.com_kp": -1.0}),
             ("null state + null tasks", {"state": None, "tasks": None}),
             ("null tasks + null handle", {"tasks": None, "handle": None}),
             ("tasks reserved 1 + null joint_weight", {"tasks.reserved": 1, "tasks.joint_weight": None}),
             ("ndof 49 + nse3 5", join(ndof(49), {"tasks.nse3": 5})),
             ("nse3 5 + null model array", {"tasks.nse3": 5, "model.parent": None}),
             ("null model array + null SE3 array", join(SE3, {"model.parent": None, "tasks.frame": None})),
             ("null SE3 array + null joint_weight", join(SE3, {"tasks.se3_kp": None, "tasks.joint_weight": None})),
             ("null joint_kp + base_damping -1", {"tasks.joint_kp": None, "tasks.base_damping": -1.0}),
             ("base_damping -1 + com_kp -1", {"tasks.base_damping": -1.0, "tasks.com_weight": PTR, "tasks.com_kp": -1.0})]
    # batch > 0: the pointers the checks want before the staged copy of the weights
    tasks = join(SE3, {"tasks.com_weight": PTR, "tasks.se3_pose": PTR, "tasks.com_pos": PTR, "tasks.joint_pos": PTR})
    running = join(tasks, {"batch": 2, "state.*": PTR})
    rows += state_buffers(running, POSITIONS)
    rows += [("null tasks.joint_pos", join(running, {"tasks.joint_pos": None})),
             ("com_kp -1 + null state buffer", join(running, {"tasks.com_kp": -1.0, "state.base_pos": None}))]
    if not track:
        rows += [("null se3_pose", join(running, {"tasks.se3_pose": None})),
                 ("null com_pos", join(running, {"tasks.com_pos": None})),
                 ("null state buffer + null se3_pose", join(running, {"state.joint_pos": None, "tasks.se3_pose": None})),
                 ("null se3_pose + null com_pos", join(running, {"tasks.se3_pose": None, "tasks.com_pos": None})),
                 ("null com_pos + null tasks.joint_pos", join(running, {"tasks.com_pos": None, "tasks.joint_pos": None}))]
    else:
        rows += [("null state buffer + null tasks.joint_pos",
                  join(running, {"state.base_rot": None, "tasks.joint_pos": None}))]
    if hard:
        ok = join(SE3, {"hard.rows": 0x3f})
        rows += [("accepted: empty batch, hard rows", ok),
                 ("hard reserved 1", join(ok, {"hard.reserved": 1}))]
        rows += [(f"rel_pivot_min {v}", join(ok, {"hard.rel_pivot_min": v})) for v in (-0.1, 1.0, "nan")]
        rows += [("hard rows above bit 26", {"hard.rows": 1 << 27}),
                 ("hard rows of an absent SE3 task", join(SE3, {"hard.rows": 1 << 6})),
                 ("hard CoM rows without a CoM task", COM_ROWS),
                 ("com_kp -1 + hard reserved 1", {"tasks.com_weight": PTR, "tasks.com_kp": -1.0, "hard.reserved": 1}),
                 ("hard reserved 1 + rel_pivot_min 1", {"hard.reserved": 1, "hard.rel_pivot_min": 1.0}),
                 ("rel_pivot_min 1 + rows above bit 26", {"hard.rel_pivot_min": 1.0, "hard.rows": 1 << 27}),
                 ("rows above bit 26 + absent SE3 task", {"hard.rows": (1 << 27) | 1}),
                 ("absent SE3 task + CoM rows without a CoM task", {"hard.rows": (1 << 24) | 1})]
    if limits:
        ok = {"limits.sampling_time": 0.01}
        rows += [("accepted: empty batch, limits", ok),
                 ("accepted: empty batch, hard rows and limits", join(SE3, {"hard.rows": 0x3f}, ok)),
                 ("limits reserved 1", join(ok, {"limits.reserved": 1}))]
        rows += [(f"sampling_time {v}", {"limits.sampling_time": v}) for v in BAD_DT]
        rows += [("max_iter -1", join(ok, {"limits.max_iter": -1})),
                 ("limits reserved 1 + sampling_time 0", {"limits.reserved": 1}),
                 ("sampling_time 0 + max_iter -1", {"limits.max_iter": -1}),
                 ("tasks reserved 1 + limits reserved 1", {"tasks.reserved": 1, "limits.reserved": 1})]
        if not track:
            rows += [("hard CoM rows + limits reserved 1", join(COM_ROWS, {"limits.reserved": 1}))]
        if stepped:
            rows += [("steps 0 + limits reserved 1", {"steps": 0, "limits.reserved": 1})]
    if track:
        rows += [("stance rows outside the SE3 tasks", join(SE3, {"schedule.stance_rows": 1 << 6})),
                 ("stance rows without SE3 tasks", {"schedule.stance_rows": 1}),
                 ("accepted: empty batch, stance rows", join(SE3, {"schedule.stance_rows": 0x3f})),
                 ("hard CoM rows + stance rows outside", join(COM_ROWS, {"schedule.stance_rows": 1})),
                 ("stance rows outside + limits reserved 1", {"schedule.stance_rows": 1, "limits.reserved": 1}),
                 ("dT 0 + limits reserved 1", {"dT": 0.0, "limits.reserved": 1})]
    return rows


def cases():
    out = []
    for entry in RC.ENTRY_POINTS:
        if entry.startswith("blf_fbd_"):
            rows = fbd(entry)
        elif entry == "blf_fb_inverse_dynamics":
            rows = inverse_dynamics()
        elif entry == "blf_fb_dcm":
            rows = dcm()
        elif entry == "blf_fb_frame_state":
            rows = frame_state()
        else:
            rows = ik(entry)
        labels = [label for label, _ in rows]
        assert len(set(labels)) == len(labels), (entry, sorted(l for l in labels if labels.count(l) > 1))
        out += [(entry, label, args) for label, args in rows]
    return out


# What a label promises: each defect it names (the parts around " + ") stands for a check, and the message
# of the row must be that of one of them.  (pattern of a defect, fragments of the messages of its check)
PROMISES = [
    (r"null handle", ["null handle"]),
    (r"null model array|null model\.(parent|joint_|link_)", ["null model array"]),
    (r"null model\.frame|null contacts\.|null contact buffer|model without frames|null frames|null frame buffer"
     r"|null tasks\.(frame|se3_weight|se3_kp)|null SE3 array",
     ["null contact buffer", "null frame buffer", "null SE3 task array"]),
    (r"null model$", ["null model / state", "!= model ndof -1"]),
    (r"null state buffer|null state\.", ["null state buffer", "null state / output buffer"]),
    (r"null state$", ["null model / state"]),
    (r"(law|model) ndof 4", ["!= model ndof"]),
    (r"ndof (0|49|-1)", ["ndof="]),
    (r"negative batch", ["negative batch", "negative size"]),
    (r"negative nframes", ["negative size"]),
    (r"^-?\d+ contacts", [" contacts"]),
    (r"laws without wrench", ["without the wrench buffer"]),
    (r"null out", ["null output buffer"]),
    (r"final time before", ["The final time has to be greater"]),
    (r"sampling_time", ["sampling_time="]),
    (r"steps_per_slice|slices", ["slices="]),
    (r"schedule steps|^steps ", ["steps="]),
    (r"^dT ", ["The sampling time must be", "dT="]),
    (r"empty interval", ["integrate(t, t)"]),
    (r"too many steps|initial time nan", ["too many integration steps"]),
    (r"null (impedance|law)$", ["null impedance", "null law"]),
    (r"schedule reserved", ["schedule->reserved must be 0"]),
    (r"tasks reserved", ["tasks->reserved must be 0"]),
    (r"hard reserved", ["hard->reserved must be 0"]),
    (r"limits reserved", ["limits->reserved must be 0"]),
    (r"^reserved 1", [": reserved must be 0"]),
    (r"null k[pd]$|null q_ref", ["null impedance array", "null law array"]),
    (r"negative omega0 stride", ["negative omega0 stride"]),
    (r"qdd?_stride", ["_stride="]),
    (r"mass_reg", ["mass_reg given"]),
    (r"null joint_torque", ["null joint_torque", "null state buffer"]),
    (r"null base_acc_out", ["null base_acc_out"]),
    (r"null base_wrench", ["null base_wrench"]),
    (r"null com_pos", ["com_weight given without com_pos"]),
    (r"null com$|null pose and twist", ["null state / output buffer"]),
    (r"xi without omega0", ["xi requested without omega0"]),
    (r"null schedule", ["null schedule"]),
    (r"null tasks\.joint_pos", ["null joint_pos set point"]),
    (r"null tasks$", ["null tasks"]),
    (r"nse3", ["nse3="]),
    (r"null joint_(weight|kp)", ["null joint task array"]),
    (r"base_damping", ["base_damping="]),
    (r"com_kp", ["com_kp="]),
    (r"null se3_pose", ["null se3_pose"]),
    (r"rel_pivot_min", ["rel_pivot_min="]),
    (r"above bit 26", ["has bits above 26"]),
    (r"absent SE3 task", ["names an SE3 task"]),
    (r"CoM rows", ["marks CoM rows without a CoM task"]),
    (r"max_iter", ["max_iter="]),
    (r"stance rows", ["stance_rows="]),
]


def promised(label):
    out = []
    for part in label.split(" + "):
        hit = next((frags for pat, frags in PROMISES if re.search(pat, part)), None)
        assert hit is not None, f"no promise known for '{part}' of '{label}'"
        out += hit
    return out


def main():
    rows = []
    for entry, label, args in cases():
        status, message = RC.invoke(entry, args)
        accepted = label.startswith("accepted")
        assert (status == 0) == accepted, (entry, label, status, message)
        assert accepted or any(f in message for f in promised(label)), (entry, label, message)
        assert status != 2, (entry, label, message)   # BLF_ERR_HIP: the call got past the argument checks
        rows.append(dict(entry=entry, case=label, args=args, status=status, message=message))
    path = os.path.join(HERE, "fb_refusals.json")
    with open(path, "w") as f:
        f.write('{\n"library": %s,\n"rows": [\n' % json.dumps(native.version()))
        f.write(",\n".join(json.dumps(r) for r in rows))
        f.write("\n]\n}\n")
    for entry in RC.ENTRY_POINTS:
        mine = [r for r in rows if r["entry"] == entry]
        print(f"{entry:46s} {len(mine):4d} rows, {len({r['message'] for r in mine if r['message']}):3d} distinct messages")
    print(f"wrote {path}: {len(rows)} rows, {os.path.getsize(path)} bytes, library {native.version()}")


if __name__ == "__main__":
    main()
