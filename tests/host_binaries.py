"""The runner of the C++ test programs under bipedal-locomotion-framework_amd/host/tests/ (their
output format: host/tests/test_harness.h).  tests/test_host_*.py name a program, a mode and the cases
they expect; everything else about building and running one is here."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bipedal-locomotion-framework_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
SANITIZER_ENV = dict(ASAN_OPTIONS="halt_on_error=1:exitcode=99:detect_leaks=1",
                     UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
# the summary line of a run in which at least one check ran and none failed
SUMMARY_OK = re.compile(r"^[1-9]\d* checks, 0 failed$", re.MULTILINE)


def binary(name, asan=False):
    """lib/blf_<name>, or the stand-alone ASan + UBSan build of it."""
    return os.path.join(PKG, "lib", "blf_" + name + ("_asan" if asan else ""))


def ensure_built(name="host_tests"):
    if not os.path.exists(binary(name)):
        subprocess.check_call(["make", "-s", "-j8", "-C", PKG])


def build_asan():
    """`make asan`: the instrumented host adapters and every test program linked to them."""
    subprocess.check_call(["make", "-s", "-j8", "-C", PKG, "asan"])


def summary_ok(stdout):
    return SUMMARY_OK.search(stdout) is not None


def run(name, mode, asan=False, golden=False, timeout=600):
    """Runs blf_<name> <mode> and returns (stdout, stderr) of a run without a failed check or a
    sanitizer finding.  asan: the stand-alone instrumented binary (build_asan() first), leak detection
    on, every UBSan finding aborts.  golden: BLF_GOLDEN_DIR points at tests/golden.  mode: cpu, gpu or
    all, or a list of arguments that begins with it."""
    if not asan:
        ensure_built(name)
    env = dict(os.environ, **(SANITIZER_ENV if asan else {}))
    if golden:
        env["BLF_GOLDEN_DIR"] = GOLDEN
    args = [mode] if isinstance(mode, str) else list(mode)
    r = subprocess.run([binary(name, asan), *args], capture_output=True, text=True, timeout=timeout, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "runtime error:" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert summary_ok(r.stdout), r.stdout
    return r.stdout, r.stderr


def assert_cases_ok(stdout, names):
    """Every case of `names` has a line that starts with its name and ends with ok."""
    lines = stdout.splitlines()
    for name in names:
        assert any(line.startswith(name) and line.rstrip().endswith("ok") for line in lines), (name, stdout)
