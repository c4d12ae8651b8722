"""The test scaffolding under test: host/tests/test_harness.h through its self-test program
(host/tests/harness_selftest.cpp: a host case and a device-flagged case that touches no device; a
second argument makes the host case fail that many checks), and tests/host_binaries.py's reading of
the output.  All on the CPU."""
import subprocess

import pytest

import host_binaries as HB

NAME = "harness_selftest"


def _selftest(*args):
    HB.ensure_built(NAME)
    return subprocess.run([HB.binary(NAME), *args], capture_output=True, text=True, timeout=60)


def test_cpu_mode_runs_host_cases_only():
    out, _ = HB.run(NAME, "cpu")
    HB.assert_cases_ok(out, ("harness host case",))
    assert "device-flagged" not in out
    assert out.splitlines()[-1] == "1 checks, 0 failed"
    both, _ = HB.run(NAME, "all")
    HB.assert_cases_ok(both, ("harness host case", "harness device-flagged case"))


def test_one_failed_check_fails_the_run():
    r = _selftest("cpu", "1")
    assert r.returncode == 1
    lines = r.stdout.splitlines()
    assert lines[0].startswith("harness host case") and lines[0].endswith("FAILED")
    assert lines[-1] == "2 checks, 1 failed"
    assert "  FAILED host/tests/harness_selftest.cpp:" in r.stderr and ": i < 0" in r.stderr
    with pytest.raises(AssertionError):
        HB.assert_cases_ok(r.stdout, ("harness host case",))
    with pytest.raises(AssertionError):
        HB.run(NAME, ["cpu", "1"])


def test_256_failed_checks_still_exit_nonzero():
    r = _selftest("cpu", "256")
    assert r.returncode != 0
    assert r.stdout.splitlines()[-1] == "257 checks, 256 failed"
    with pytest.raises(AssertionError):
        HB.run(NAME, ["cpu", "256"])


def test_unknown_mode_is_refused():
    r = _selftest("cuda")
    assert r.returncode == 2
    assert r.stdout == "" and "unknown mode" in r.stderr


def test_summary_matcher():
    assert HB.summary_ok("a case ok\n10 checks, 0 failed\n")
    assert not HB.summary_ok("10 checks, 10 failed\n")
    assert not HB.summary_ok("0 checks, 0 failed\n")
    assert not HB.summary_ok("x 10 checks, 0 failed\n")
