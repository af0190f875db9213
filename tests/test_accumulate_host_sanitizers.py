"""The host side of accumulated frames (kifs_accumulate.cpp: the checks, the sub-frames as views, the scene and view
rings it shares with the animated call) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU:
`make asan-accumulate` compiles the seven host units and kifs_accumulate.cpp as plain C++ with
-fsanitize=address,undefined and links them with tests/hip_stub/hip_stub.cpp (unchanged), a stand-in for
launch_accumulate_render (accumulate_family_stub.cpp, which stands in for all three accumulate launchers) and a stand-alone driver (accumulate_driver.cpp) that runs 1 x 1, 6 x 8,
8 x 64 and 13 x 5 views with and without options, bands, two streams, every refusal, a failure injected into every HIP
call of an 8 x 64 call, and a final leak census.  Nothing sanitized is loaded into Python or run on a GPU."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_accumulate_host_side_is_clean_under_asan_and_ubsan():
    make = subprocess.run(["make", "-C", str(ROOT / "kifs_raymarching_amd" / "csrc"), "asan-accumulate"], capture_output=True,
                          text=True, timeout=900)
    assert make.returncode == 0, make.stderr[-3000:]
    assert "warning:" not in make.stderr, make.stderr[-3000:]
    run = subprocess.run([str(ROOT / "build" / "kifs_accumulate_asan")], capture_output=True, text=True, timeout=600,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1",
                              "PATH": "/usr/bin:/bin"})
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-4000:])
    assert "checks ok" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
