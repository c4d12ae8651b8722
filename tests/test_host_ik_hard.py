"""Runs the C++17 adapter tests of IK::QPInverseKinematics' hard (priority 0) tasks
(bipedal-locomotion-framework_amd/host/tests/ik_hard_tests.cpp): on the CPU the bookkeeping (priority
0 accepted without a weight, refused with one and for the joint task, "hard_task_weight" out of
range, the mask the adapter builds), plain and as the stand-alone ASan + UBSan binary; on a GPU
advance() against blf_fb_ik_solve_hard for a biped with hard feet, and advance() false for two hard
tasks on one frame."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bipedal-locomotion-framework_amd")
BIN = os.path.join(PKG, "lib", "blf_ik_hard_tests")
BIN_ASAN = os.path.join(PKG, "lib", "blf_ik_hard_tests_asan")
CPU_CASES = ("QPInverseKinematics hard task bookkeeping",)
GPU_CASES = ("QPInverseKinematics hard feet on the device", "QPInverseKinematics dependent hard tasks")


def _run(binary, which, extra_env=None):
    env = dict(os.environ, **(extra_env or {}))
    r = subprocess.run([binary, which], capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "runtime error:" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "0 failed" in r.stdout, r.stdout
    return r.stdout


def _ok(out, name):
    return any(line.startswith(name) and line.rstrip().endswith("ok") for line in out.splitlines())


def test_ik_hard_adapter_bookkeeping():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-j8", "-C", PKG])
    out = _run(BIN, "cpu")
    for name in CPU_CASES:
        assert _ok(out, name), out


def test_ik_hard_adapter_asan_cpu():
    """The instrumented stand-alone binary (make asan), host-only cases: leak detection on, every
    UBSan finding aborts."""
    subprocess.check_call(["make", "-s", "-j8", "-C", PKG, "asan"])
    out = _run(BIN_ASAN, "cpu",
               dict(ASAN_OPTIONS="halt_on_error=1:exitcode=99:detect_leaks=1",
                    UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    for name in CPU_CASES:
        assert _ok(out, name), out


@pytest.mark.gpu
def test_ik_hard_adapter_on_device():
    out = _run(BIN, "gpu")
    for name in GPU_CASES:
        assert _ok(out, name), out
