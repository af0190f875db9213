"""The host side of jittered accumulated frames (kifs_render_accumulate_jittered_async in kifs_accumulate.cpp: its own
refusals, the cell of every view in pad[0] of its scene record, the grid as the launch's FrameParams::ssaa with the virtual
screen's 1 / height) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: `make asan-jitter` compiles the seven
host units and kifs_accumulate.cpp as plain C++ with -fsanitize=address,undefined and links them with
tests/hip_stub/hip_stub.cpp (unchanged), a stand-in for launch_accumulate_render that records what a launch carries
(accumulate_family_stub.cpp) and a stand-alone driver (accumulate_jitter_driver.cpp) that runs 1 x 1, 6 x 8, 8 x 64, 13 x 5
and 2 x 9 views at grids 1, 3 and 8 with cells given and NULL, options given and NULL, unjittered calls in between (zero
pad words, a grid of 1), every refusal, a failure injected into every HIP call of an 8 x 64 call, and a final leak census.
Nothing sanitized is loaded into Python or run on a GPU."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_jitter_host_side_is_clean_under_asan_and_ubsan():
    make = subprocess.run(["make", "-C", str(ROOT / "kifs_raymarching_amd" / "csrc"), "asan-jitter"], capture_output=True,
                          text=True, timeout=900)
    assert make.returncode == 0, make.stderr[-3000:]
    assert "warning:" not in make.stderr, make.stderr[-3000:]
    run = subprocess.run([str(ROOT / "build" / "kifs_jitter_asan")], capture_output=True, text=True, timeout=600,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1",
                              "PATH": "/usr/bin:/bin"})
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-4000:])
    assert "checks ok" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
