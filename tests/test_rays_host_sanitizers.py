"""The host side of ray queries (kifs_trace_rays_async: kifs_rays.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer,
on the CPU: `make asan-rays` compiles the seven host units and kifs_rays.cpp as plain C++ with -fsanitize=address,undefined
and links them with tests/hip_stub/hip_stub.cpp (unchanged), a stand-in for launch_trace_rays that records what a launch
carries (rays_stub.cpp) and a stand-alone driver with its own main (rays_driver.cpp): every refusal with nothing launched,
no HIP call made and nothing written; both outputs and either alone; n at 0, 1, 255, 256, 257, 1000 and KIFS_MAX_RAYS with
the launch's grid; the frame constants on a context without screen or camera and on one with both and a supersampling
factor; a caller's stream; a failed launch; the existing render calls before, between and after traces; and a final leak
census.  The five existing sanitizer targets must keep building against their unchanged stand-ins, without the new file.
Nothing sanitized is loaded into Python or run on a GPU."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kifs_raymarching_amd" / "csrc"


def test_rays_host_side_is_clean_under_asan_and_ubsan():
    make = subprocess.run(["make", "-C", str(CSRC), "asan-rays"], capture_output=True, text=True, timeout=900)
    assert make.returncode == 0, make.stderr[-3000:]
    assert "warning:" not in make.stderr, make.stderr[-3000:]
    run = subprocess.run([str(ROOT / "build" / "kifs_rays_asan")], capture_output=True, text=True, timeout=900,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1",
                              "PATH": "/usr/bin:/bin"})
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-4000:])
    m = re.search(r"rays_driver: (\d+) checks ok", run.stdout)
    assert m, run.stdout[-1500:]
    print(f"rays_driver: {m.group(1)} checks")
    assert int(m.group(1)) >= 800  # (README quotes the count)
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr


def test_the_existing_sanitizer_targets_still_build():
    """kifs_internal.hpp declares a launcher more: the five drivers that link stand-ins for today's launchers alone must
    build as before, without a warning and without kifs_rays.cpp.  Their own tests run them."""
    text = (CSRC / "Makefile").read_text()
    for target in ("asan", "asan-accumulate", "asan-jitter", "asan-progressive", "asan-converge"):
        rule = re.search(rf"^{target}: \S+\n(?:.*\\\n)*.*\n(?:\t.*\\?\n)+", text, re.M).group(0)
        assert "kifs_rays" not in rule and "rays_" not in rule, target
        make = subprocess.run(["make", "-C", str(CSRC), target], capture_output=True, text=True, timeout=900)
        assert make.returncode == 0, (target, make.stderr[-3000:])
        assert "warning:" not in make.stderr and "undefined" not in make.stderr, (target, make.stderr[-3000:])
