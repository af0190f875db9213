"""The host side of kaleidoscopic IFS scenes (kifs_render_folded_async and kifs_eval_fold: kifs_fold.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: `make asan-fold` compiles the seven host units and kifs_fold.cpp
as plain C++ with -fsanitize=address,undefined and links them with tests/hip_stub/hip_stub.cpp (unchanged), a stand-in for
launch_folded and launch_eval_fold that records what a launch carries and models its stores (fold_stub.cpp) and a
stand-alone driver with its own main (fold_driver.cpp): every refusal with nothing launched and nothing written; one frame,
three and 64; bands; supersampling factors 1..4; a NULL light, a NULL term and both given; the system with the scaling
step's constants as the contract computes them, ALL THREE CULLS ZERO in the launched frame constants where the plain render
of the same context keeps them, the light as given and normalised, the views, the band's tile table and the fixed launch
shape of every launch; a caller's stream; a failed launch; the evaluation's refusals, values and allocations; the plain
render calls before, between and after the call with the same bytes, launch state and tile order; and a final leak census.
The existing sanitizer targets must keep building against their unchanged stand-ins, without the new file.  Nothing
sanitized is loaded into Python or run on a GPU."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kifs_raymarching_amd" / "csrc"


def test_fold_host_side_is_clean_under_asan_and_ubsan():
    make = subprocess.run(["make", "-C", str(CSRC), "asan-fold"], capture_output=True, text=True, timeout=900)
    assert make.returncode == 0, make.stderr[-3000:]
    assert "warning:" not in make.stderr, make.stderr[-3000:]
    run = subprocess.run([str(ROOT / "build" / "kifs_fold_asan")], capture_output=True, text=True, timeout=900,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1",
                              "PATH": "/usr/bin:/bin"})
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-4000:])
    m = re.search(r"fold_driver: (\d+) checks ok", run.stdout)
    assert m, run.stdout[-1500:]
    print(f"fold_driver: {m.group(1)} checks")
    assert int(m.group(1)) >= 350000  # (354029 when the call was added)
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr


def test_the_other_sanitizer_targets_link_without_the_new_unit():
    """kifs_internal.hpp declares two launchers more: the drivers that link stand-ins for the other launchers alone must
    build as before, the trapped call's among them.  Their own tests run them.  (`make asan` builds the new driver beside
    the first one; its rule names no fold source for the first.)"""
    text = (CSRC / "Makefile").read_text()
    for target in ("asan-accumulate", "asan-jitter", "asan-progressive", "asan-converge", "asan-rays", "asan-occlusion",
                   "asan-lighting", "asan-trap", "asan-tile-memory"):
        rule = re.search(rf"^{target}: \S+\n(?:.*\\\n)*.*\n(?:\t.*\\?\n)+", text, re.M).group(0)
        assert "fold" not in rule, target
    rule = re.search(r"^\$\(BUILD\)/kifs_host_asan:.*\n(?:\t.*\\?\n)+", text, re.M).group(0)
    assert "fold" not in rule
    assert re.search(r"^asan: asan-fold$", text, re.M)
    for name in ("HOSTSRC", "STUBSRC", "FAMILYSRC", "FAMILYDEPS", "OCCLSRC", "LIGHTSRC", "TRAPSRC"):
        assert "fold" not in re.search(rf"^{name}\s*:=.*(?:\\\n.*)*", text, re.M).group(0), name
    make = subprocess.run(["make", "-C", str(CSRC), "asan-trap"], capture_output=True, text=True, timeout=900)
    assert make.returncode == 0, make.stderr[-3000:]
    assert "warning:" not in make.stderr and "undefined" not in make.stderr, make.stderr[-3000:]
