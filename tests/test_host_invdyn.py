"""Runs the C++17 adapter tests of System::FloatingBaseDynamicalSystem::inverseDynamics
(bipedal-locomotion-framework_amd/host/tests/invdyn_tests.cpp): on the CPU the refusal without a robot
model, plain and as the stand-alone ASan + UBSan binary; on a GPU the round trip (the torques of
inverseDynamics set as the control input, dynamics() returns the requested joint accelerations and the same
base acceleration), free fall, and the refusals of a wrong size and of a robot the device reports failed."""
import pytest

import host_binaries as HB

CPU_CASES = ("FloatingBaseDynamicalSystem inverseDynamics refusals",)
GPU_CASES = ("FloatingBaseDynamicalSystem inverseDynamics on the device",)
TAG = "[FloatingBaseDynamicalSystem::inverseDynamics] "


def _lines(err):
    return [l for l in err.splitlines() if l.startswith(TAG)]


def test_invdyn_adapter_refusals():
    out, err = HB.run("invdyn_tests", "cpu")
    HB.assert_cases_ok(out, CPU_CASES)
    assert any("setRobotModel" in l for l in _lines(err)), err


def test_invdyn_adapter_asan_cpu():
    """The instrumented stand-alone binary (make asan), host-only cases: leak detection on, every
    UBSan finding aborts."""
    HB.build_asan()
    out, _ = HB.run("invdyn_tests", "cpu", asan=True)
    HB.assert_cases_ok(out, CPU_CASES)


@pytest.mark.gpu
def test_invdyn_adapter_on_device():
    out, err = HB.run("invdyn_tests", "gpu")
    HB.assert_cases_ok(out, GPU_CASES)
    for word in ("Wrong size", "The device reports"):
        assert any(word in l for l in _lines(err)), (word, err)
