"""The host side of progressive accumulation (kifs_render_accumulate_resume_async: kifs_progressive.cpp on top of the
shared check / check_jitter / enqueue of kifs_accumulate.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, on the
CPU: `make asan-progressive` compiles the seven host units, kifs_accumulate.cpp and kifs_progressive.cpp as plain C++ with
-fsanitize=address,undefined and links them with tests/hip_stub/hip_stub.cpp (unchanged), a stand-in that defines BOTH
accumulate launchers and records a pass's CarryParams (accumulate_family_stub.cpp) and a stand-alone driver with its own main
(progressive_driver.cpp): 1 x 1, 6 x 8, 8 x 64 and 13 x 5 views per pass as sequences of passes over one plane from prior 0,
1 and 2^24 - the frame's sub-frames, a picture from every pass, the last or none, bands with padded pitches on both
destinations, two streams, two contexts on one plane, an existing jittered and an existing unjittered call after every
pass, every refusal with nothing launched, a failure injected into every HIP call and the launch of an 8 x 64 pass, and a
final leak census.  The three existing sanitizer targets must keep building against their unchanged stand-ins, which
define launch_accumulate_render and nothing newer.  Nothing sanitized is loaded into Python or run on a GPU."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kifs_raymarching_amd" / "csrc"


def test_progressive_host_side_is_clean_under_asan_and_ubsan():
    make = subprocess.run(["make", "-C", str(CSRC), "asan-progressive"], capture_output=True, text=True, timeout=900)
    assert make.returncode == 0, make.stderr[-3000:]
    assert "warning:" not in make.stderr, make.stderr[-3000:]
    run = subprocess.run([str(ROOT / "build" / "kifs_progressive_asan")], capture_output=True, text=True, timeout=900,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1",
                              "PATH": "/usr/bin:/bin"})
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-4000:])
    assert "progressive_driver:" in run.stdout and "checks ok" in run.stdout
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr


def test_the_existing_sanitizer_targets_still_link():
    """kifs_accumulate.cpp takes its launch step as a parameter now: the drivers that link it with a stand-in for
    launch_accumulate_render alone (and `asan`, which links without it) must build as before.  Their own tests run them."""
    for target in ("asan", "asan-accumulate", "asan-jitter"):
        make = subprocess.run(["make", "-C", str(CSRC), target], capture_output=True, text=True, timeout=900)
        assert make.returncode == 0, (target, make.stderr[-3000:])
        assert "warning:" not in make.stderr and "undefined" not in make.stderr, (target, make.stderr[-3000:])
