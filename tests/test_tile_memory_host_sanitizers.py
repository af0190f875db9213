"""The tile order's feedback on the host (kifs_schedule.cpp: feedback_before / feedback_after, tile_table, the sort with a
memory) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: `make asan-tile-memory` compiles the seven host
units as plain C++ with -fsanitize=address,undefined and links them with tests/hip_stub/hip_stub.cpp (unchanged), the
stand-in for launch_tile_order_remembering (tile_memory_stub.cpp) and a stand-alone driver with its own main
(tile_memory_driver.cpp): batches walked through record, sort and adopt over 22 periods with planted costs -- the table a
sort is handed, the memory word for word, the order, which order buffer every launch reads --, lone frames on the same
table, a failure injected at every HIP call of such a walk and at the sort's launch, and a final leak census.  Nothing
sanitized is loaded into Python or run on a GPU."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kifs_raymarching_amd" / "csrc"


def test_tile_order_feedback_host_side_is_clean_under_asan_and_ubsan():
    make = subprocess.run(["make", "-C", str(CSRC), "asan-tile-memory"], capture_output=True, text=True, timeout=900)
    assert make.returncode == 0, make.stderr[-3000:]
    assert "warning:" not in make.stderr, make.stderr[-3000:]
    run = subprocess.run([str(ROOT / "build" / "kifs_tile_memory_asan")], capture_output=True, text=True, timeout=900,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1",
                              "PATH": "/usr/bin:/bin"})
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-4000:])
    m = re.search(r"tile_memory_driver: (\d+) checks ok", run.stdout)
    assert m, run.stdout[-1500:]
    print(f"tile_memory_driver: {m.group(1)} checks")
    assert int(m.group(1)) >= 46000
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
