"""CPU test of the floating-base C boundary (include/blf/blf_c.h sections 8 to 12d): every refusal the 15
entry points make before any HIP call, and their accepted empty-batch calls, against the table
tests/golden/fb_refusals.json (tests/golden/make_fb_refusals.py wrote it from the library named in its
`library` member).  Status and blf_last_error() text are compared exactly, and the rows with two defects
fix which check reports first: the table is what "the boundary behaves as before" means.  The calls are
built by tests/fb_refusal_calls.py: a fake handle and fake array pointers that are never dereferenced."""
import json
import os

import pytest

import fb_refusal_calls as RC

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fb_refusals.json")) as _f:
    TABLE = json.load(_f)
ROWS = TABLE["rows"]

# Fragments of the messages the table must hold for an entry point: every check of the call that can
# refuse before a HIP call (the rest need a device; tests/golden/make_fb_refusals.py lists them).
EVERY = ["null handle", "null model / state", ": negative ", "ndof=", "null model array"]
CONTACTS = ["null state buffer", " contacts", "null contact buffer", "without the wrench buffer"]
SCHEDULE = ["The final time has to be greater", "The sampling time must be", "integrate(t, t)",
            "too many integration steps"]
LAW = [": reserved must be 0", " array", "!= model ndof"]
TRAJ = ["slices=", "qd_stride="]
IK = ["null tasks", "tasks->reserved must be 0", "nse3=", "null SE3 task array", "null joint task array",
      "base_damping=", "com_kp=", "null state buffer", "null joint_pos set point"]
SETPOINTS = ["null se3_pose", "com_weight given without com_pos"]
STEPS = ["steps=", "dT="]
HARD = ["hard->reserved must be 0", "rel_pivot_min=", "has bits above 26", "names an SE3 task",
        "marks CoM rows without a CoM task"]
LIMITS = ["limits->reserved must be 0", "sampling_time=", "max_iter="]
REQUIRED = {
    "blf_fbd_dynamics": EVERY + CONTACTS + ["null output buffer"],
    "blf_fbd_euler_integrate": EVERY + CONTACTS + SCHEDULE,
    "blf_fbd_euler_integrate_impedance": EVERY + CONTACTS + SCHEDULE + LAW + ["null impedance"],
    "blf_fbd_euler_integrate_impedance_traj": EVERY + CONTACTS + SCHEDULE + LAW + TRAJ + ["null impedance"],
    "blf_fbd_euler_integrate_computed_torque_traj": EVERY + CONTACTS + SCHEDULE + LAW + TRAJ
                                                    + ["null law", "qdd_stride=", "mass_reg given", ", at most 8"],
    "blf_fb_inverse_dynamics": EVERY + CONTACTS + [": reserved must be 0", "null joint_torque", "null base_acc_out",
                                                    "null base_wrench", ", at most 8"],
    "blf_fb_dcm": EVERY + ["null state / output buffer", "xi requested without omega0", "negative omega0 stride"],
    "blf_fb_frame_state": EVERY + ["negative size", "null frame buffer", "null state / output buffer"],
    "blf_fb_ik_solve": EVERY + IK + SETPOINTS,
    "blf_fb_ik_integrate": EVERY + IK + SETPOINTS + STEPS,
    "blf_fb_ik_solve_hard": EVERY + IK + SETPOINTS + HARD,
    "blf_fb_ik_integrate_hard": EVERY + IK + SETPOINTS + HARD + STEPS,
    "blf_fb_ik_solve_limits": EVERY + IK + SETPOINTS + HARD + LIMITS,
    "blf_fb_ik_integrate_limits": EVERY + IK + SETPOINTS + HARD + LIMITS + STEPS,
    "blf_fb_ik_track": EVERY + IK + HARD + LIMITS + STEPS + ["null schedule", "schedule->reserved must be 0",
                                                              "stance_rows="],
}


def test_table_covers_every_entry_point():
    assert " src " in TABLE["library"], TABLE["library"]   # blf_version() of the library the table was taken from
    assert set(REQUIRED) == set(RC.ENTRY_POINTS) == {r["entry"] for r in ROWS}
    for entry in RC.ENTRY_POINTS:
        mine = [r for r in ROWS if r["entry"] == entry]
        assert sum(r["status"] == 0 for r in mine) >= 1, entry          # the accepted empty-batch call
        assert all(r["status"] != 2 for r in mine), entry               # BLF_ERR_HIP: a HIP call was reached
        assert all((r["status"] == 0) == (r["message"] is None) for r in mine), entry
        messages = [r["message"] for r in mine if r["message"]]
        assert all(m.startswith(entry + ": ") or m in _schedule_text(messages) for m in messages), entry
        missing = [f for f in REQUIRED[entry] if not any(f in m for m in messages)]
        assert not missing, (entry, missing)


def _schedule_text(messages):
    """step_schedule's messages are the reference integrator's and do not name the entry point."""
    return [m for m in messages if any(f in m for f in SCHEDULE)]


@pytest.mark.parametrize("entry", RC.ENTRY_POINTS)
def test_refusals_match_the_table(entry):
    wrong = []
    for r in ROWS:
        if r["entry"] != entry:
            continue
        status, message = RC.invoke(entry, r["args"])
        if (status, message) != (r["status"], r["message"]):
            wrong.append(f"{r['case']}: got {status} {message!r}, the table holds {r['status']} {r['message']!r}")
    assert not wrong, "\n".join(wrong)
