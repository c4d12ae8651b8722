"""Runs the C++17 tests of blf/robot_model.h, what the adapters over a blf_fb_model share
(bipedal-locomotion-framework_amd/host/tests/model_tests.cpp): on the CPU the one validation of a robot
model, its defects in their fixed order and the three adapters' refusals with the one text per defect, the
fixed-joint models FloatingBaseDynamicalSystem used to accept unmerged, and the state layout, plain and as
the stand-alone ASan + UBSan binary; on a GPU the device copy against a hand-uploaded model."""
import pytest

import host_binaries as HB

CPU_CASES = ("defect table", "the fixed-joint hole", "accepted models", "state layout")
TAGS = ("[FloatingBaseDynamicalSystem::setRobotModel] ", "[QPInverseKinematics::setRobotModel] ",
        "[LeggedOdometry::setRobotModel] ")
TEXTS = ("Corrupted robot model.", "The joints must be in topological order (parent[j] <= j).",
         "A frame is attached to a link the model does not have.", "Unknown joint type")
MARK = "model_tests row "


def assert_refusals(stderr):
    """Every row of the defect table (a MARK line that ends with describe()'s text, then what the three
    adapters print) has one line per adapter that begins with its tag and contains that text."""
    rows, lines = [], None
    for line in stderr.splitlines():
        if line.startswith("model_tests "):
            lines = []
            if line.startswith(MARK):
                rows.append((line[len(MARK):], lines))
        elif lines is not None:
            lines.append(line)
    assert len(rows) == 2 * 2 * 14, len(rows)   # chain and biped, plain and masked, the table's rows
    for row, printed in rows:
        name, _, text = row.partition(": ")
        assert text in TEXTS, row
        for tag in TAGS:
            assert any(p.startswith(tag) and text in p for p in printed), (name, tag, printed)
    assert {row.partition(": ")[2] for row, _ in rows} == set(TEXTS)
    # refused before any device work: no allocation, copy or handle was tried (blf/device.h reports those)
    assert "[blf::" not in stderr, stderr[-2000:]


def test_robot_model_validation_and_layout():
    out, err = HB.run("model_tests", "cpu")
    HB.assert_cases_ok(out, CPU_CASES)
    assert_refusals(err)


def test_robot_model_asan_cpu():
    """The instrumented stand-alone binary (make asan), host-only cases: leak detection on, every
    UBSan finding aborts."""
    HB.build_asan()
    out, err = HB.run("model_tests", "cpu", asan=True)
    HB.assert_cases_ok(out, CPU_CASES)
    assert_refusals(err)


@pytest.mark.gpu
def test_device_robot_model_on_device():
    out, _ = HB.run("model_tests", "gpu")
    HB.assert_cases_ok(out, ("device model",))
