"""The host side of orbit-trap colouring of folded scenes (kifs_render_folded_trapped_async and kifs_eval_fold_trap:
kifs_fold_trap.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: `make asan-fold-trap` compiles the seven
host units and kifs_fold_trap.cpp as plain C++ with -fsanitize=address,undefined and links them with
tests/hip_stub/hip_stub.cpp (unchanged), a stand-in for launch_folded_trapped and launch_eval_fold_trap that records what a
launch carries -- its Params and the record's contents as the copy left them at launch time -- and models its stores, the
plane included (fold_trap_stub.cpp), and a stand-alone driver with its own main (fold_trap_driver.cpp): every refusal with
nothing launched and nothing written; one frame, three and 64; bands; supersampling factors 1..4; the plane with and without
a term; all three culls zero in every launch; more calls than the scene-table ring is deep, each with a record of its own; a
failure injected at every HIP call and at the launch; animated batches interleaved on the same ring; the evaluation; the
plain render calls before, between and after the call; and a final leak census.  The existing sanitizer targets must keep
building against their unchanged stand-ins, without the new file -- kifs_animation.cpp, which they share, now exports the
ring's two steps.  Nothing sanitized is loaded into Python or run on a GPU."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kifs_raymarching_amd" / "csrc"


def test_fold_trap_host_side_is_clean_under_asan_and_ubsan():
    make = subprocess.run(["make", "-C", str(CSRC), "asan-fold-trap"], capture_output=True, text=True, timeout=900)
    assert make.returncode == 0, make.stderr[-3000:]
    assert "warning:" not in make.stderr, make.stderr[-3000:]
    run = subprocess.run([str(ROOT / "build" / "kifs_fold_trap_asan")], capture_output=True, text=True, timeout=900,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1",
                              "PATH": "/usr/bin:/bin"})
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-4000:])
    m = re.search(r"fold_trap_driver: (\d+) checks ok", run.stdout)
    assert m, run.stdout[-1500:]
    print(f"fold_trap_driver: {m.group(1)} checks")
    assert int(m.group(1)) >= 100000
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr


def test_the_other_sanitizer_targets_link_without_the_new_unit():
    """kifs_internal.hpp declares two launchers more and kifs_context.hpp the ring's two steps: the drivers that link
    stand-ins for the other launchers alone must build as before.  Their own tests run them.  (`make asan` builds the new
    driver beside the first one.)"""
    text = (CSRC / "Makefile").read_text()
    for target in ("asan-accumulate", "asan-jitter", "asan-progressive", "asan-converge", "asan-rays", "asan-occlusion",
                   "asan-lighting", "asan-trap", "asan-fold", "asan-tile-memory"):
        rule = re.search(rf"^{target}: \S+\n(?:.*\\\n)*.*\n(?:\t.*\\?\n)+", text, re.M).group(0)
        assert "fold_trap" not in rule, target
    assert re.search(r"^asan: asan-fold-trap$", text, re.M)
    for name in ("HOSTSRC", "STUBSRC", "FAMILYSRC", "FAMILYDEPS", "OCCLSRC", "LIGHTSRC", "TRAPSRC", "FOLDSRC"):
        assert "fold_trap" not in re.search(rf"^{name}\s*:=.*(?:\\\n.*)*", text, re.M).group(0), name
    make = subprocess.run(["make", "-C", str(CSRC), "asan-fold"], capture_output=True, text=True, timeout=900)
    assert make.returncode == 0, make.stderr[-3000:]
    assert "warning:" not in make.stderr and "undefined" not in make.stderr, make.stderr[-3000:]
