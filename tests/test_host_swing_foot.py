"""Runs the C++17 adapter tests of Planners::SwingFootPlanner and Planners::SO3Planner
(bipedal-locomotion-framework_amd/host/tests/swing_tests.cpp): on the CPU every path on which
the adapters return false, plain and as the stand-alone ASan + UBSan binary; on a GPU a two-contact
list walked by advance() against blf_swing_foot_eval, and SO3Planner against blf_so3_eval."""
import pytest

import host_binaries as HB

CPU_CASES = ("SwingFootPlanner parameter handler", "SwingFootPlanner state machine")
GPU_CASES = ("SwingFootPlanner on the device", "SO3Planner on the device")


def test_swing_adapters_error_paths():
    out, _ = HB.run("swing_tests", "cpu")
    HB.assert_cases_ok(out, CPU_CASES)


def test_swing_adapters_asan_cpu():
    """The instrumented stand-alone binary (make asan), host-only cases: leak detection on, every
    UBSan finding aborts."""
    HB.build_asan()
    out, _ = HB.run("swing_tests", "cpu", asan=True)
    HB.assert_cases_ok(out, CPU_CASES)


@pytest.mark.gpu
def test_swing_adapters_on_device():
    out, _ = HB.run("swing_tests", "gpu")
    HB.assert_cases_ok(out, GPU_CASES)
