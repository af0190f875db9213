"""The host side of converging accumulation (kifs_render_accumulate_converge_async: kifs_converge.cpp on top of the shared
check / check_jitter / enqueue of kifs_accumulate.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU:
`make asan-converge` compiles the seven host units, kifs_accumulate.cpp, kifs_progressive.cpp and kifs_converge.cpp as
plain C++ with -fsanitize=address,undefined and links them with tests/hip_stub/hip_stub.cpp (unchanged), a stand-in that
defines ALL THREE accumulate launchers and records a pass's ConvergeParams (accumulate_family_stub.cpp) and a stand-alone driver with
its own main (converge_driver.cpp): sequences of passes with and without restart, picture and counts, bands with padded
pitches on all three destinations, two streams and two contexts on one pair of planes, the counts zeroed before the launch,
every refusal with no HIP call made, a failure injected into every HIP call and the launch, an existing resume call and an
existing jittered call between passes, and a final leak census.  The four existing sanitizer targets must keep building
against their unchanged stand-ins.  Nothing sanitized is loaded into Python or run on a GPU."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kifs_raymarching_amd" / "csrc"


def test_converge_host_side_is_clean_under_asan_and_ubsan():
    make = subprocess.run(["make", "-C", str(CSRC), "asan-converge"], capture_output=True, text=True, timeout=900)
    assert make.returncode == 0, make.stderr[-3000:]
    assert "warning:" not in make.stderr, make.stderr[-3000:]
    run = subprocess.run([str(ROOT / "build" / "kifs_converge_asan")], capture_output=True, text=True, timeout=900,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1",
                              "PATH": "/usr/bin:/bin"})
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-4000:])
    assert "converge_driver:" in run.stdout and "checks ok" in run.stdout
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr


def test_the_existing_sanitizer_targets_still_build():
    """kifs_internal.hpp declares a launcher more: the four drivers that link stand-ins for today's launchers alone must
    build as before, without a warning.  Their own tests run them."""
    for target in ("asan", "asan-accumulate", "asan-jitter", "asan-progressive"):
        make = subprocess.run(["make", "-C", str(CSRC), target], capture_output=True, text=True, timeout=900)
        assert make.returncode == 0, (target, make.stderr[-3000:])
        assert "warning:" not in make.stderr and "undefined" not in make.stderr, (target, make.stderr[-3000:])
