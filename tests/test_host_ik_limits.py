"""Runs the C++17 adapter tests of IK::JointLimitsTask in IK::QPInverseKinematics
(bipedal-locomotion-framework_amd/host/tests/ik_limits_tests.cpp): on the CPU the task's keys and
refusals, the bookkeeping (priority 0 only, once, no weight) and blf::loadUrdf's joint limits, plain and
as the stand-alone ASan + UBSan binary; on a GPU finalize()'s refusals (sizes, "use_model_limits" on a
model without limits), advance() against blf_fb_ik_solve_limits with a bound active, and advance()
false on limits that leave the hard feet no solution.  And, on the CPU, that the two URDF loaders
(blf/urdf.py, blf::loadUrdf) read equal limits from one document."""
import subprocess

import numpy as np
import pytest

import host_binaries as HB

CPU_CASES = ("JointLimitsTask keys", "QPInverseKinematics limits task bookkeeping", "loadUrdf joint limits")
GPU_CASES = ("QPInverseKinematics limits finalize", "QPInverseKinematics limits on the device",
             "QPInverseKinematics infeasible limits")

URDF = """<?xml version="1.0"?>
<robot name="limits">
  <link name="base"><inertial><mass value="2.0"/><inertia ixx="0.1" iyy="0.1" izz="0.1"/></inertial></link>
  <link name="upper"/><link name="bracket"/><link name="wheel"/><link name="rail"/><link name="tip"/>
  <joint name="shoulder" type="revolute"><parent link="base"/><child link="upper"/><axis xyz="0 1 0"/>
    <limit lower="-0.75" upper="1.5" velocity="3.25" effort="40"/></joint>
  <joint name="weld" type="fixed"><parent link="upper"/><child link="bracket"/>
    <limit lower="-9" upper="9" velocity="9"/></joint>
  <joint name="spin" type="continuous"><parent link="bracket"/><child link="wheel"/><axis xyz="0 0 1"/>
    <limit lower="-1" upper="1" velocity="2.5"/></joint>
  <joint name="slide" type="prismatic"><parent link="wheel"/><child link="rail"/><axis xyz="1 0 0"/>
    <limit lower="0.0" upper="0.3"/></joint>
  <joint name="wrist" type="revolute"><parent link="rail"/><child link="tip"/><axis xyz="1 0 0"/></joint>
</robot>
"""


def test_ik_limits_adapter_bookkeeping():
    out, _ = HB.run("ik_limits_tests", "cpu")
    HB.assert_cases_ok(out, CPU_CASES)


def test_ik_limits_adapter_asan_cpu():
    """The instrumented stand-alone binary (make asan), host-only cases: leak detection on, every
    UBSan finding aborts."""
    HB.build_asan()
    out, _ = HB.run("ik_limits_tests", "cpu", asan=True)
    HB.assert_cases_ok(out, CPU_CASES)


def test_urdf_loaders_read_equal_limits(tmp_path):
    """A document with revolute, continuous, prismatic and fixed joints: the Python loader's
    load_urdf_limits and blf::loadUrdf's jointLower / jointUpper / jointVelocityLimit agree, joint by
    joint, after the fixed joint is merged; the continuous joint and the joint without <limit> have no
    range, the prismatic joint no velocity limit."""
    from blf import urdf
    HB.ensure_built("ik_limits_tests")
    path = tmp_path / "limits.urdf"
    path.write_text(URDF)
    model = urdf.load_urdf(str(path))
    lim = urdf.load_urdf_limits(str(path), model)
    r = subprocess.run([HB.binary("ik_limits_tests"), "urdf", str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [line.split() for line in r.stdout.splitlines()]
    assert [row[0] for row in rows] == list(model["names"][1:]) == ["shoulder", "spin", "slide", "wrist"]
    cpp = np.array([[float(v) for v in row[1:]] for row in rows])
    np.testing.assert_array_equal(cpp[:, 0], lim["pos_lower"])
    np.testing.assert_array_equal(cpp[:, 1], lim["pos_upper"])
    np.testing.assert_array_equal(cpp[:, 2], lim["vel_max"])
    np.testing.assert_array_equal(lim["pos_lower"], [-0.75, -np.inf, 0.0, -np.inf])
    np.testing.assert_array_equal(lim["pos_upper"], [1.5, np.inf, 0.3, np.inf])
    np.testing.assert_array_equal(lim["vel_max"], [3.25, 2.5, np.inf, np.inf])
    two = urdf.load_urdf(str(path), considered_joints=["shoulder", "slide"])
    np.testing.assert_array_equal(urdf.load_urdf_limits(str(path), two)["pos_upper"], [1.5, 0.3])


@pytest.mark.gpu
def test_ik_limits_adapter_on_device():
    out, _ = HB.run("ik_limits_tests", "gpu")
    HB.assert_cases_ok(out, GPU_CASES)
