"""The throughput kernel's orbit trip in doubled coordinates (KIFS_FAST_TRIP_X2_ in kifs_scene.hpp) against the plain
trip it replaces, on the CPU: tests/orbit_x2_emulator.c runs both operation for operation, with -ffp-contract=off and
IEEE denormals, over 2 x 10^7 random orbits (KIFS_ORBIT_X2_ORBITS=N for a longer sweep; 10^8 takes ~13 s with hardware
fma, minutes with libm's software one) -- cfg2's constant, random constants, start points near the fractal, tiny and
zero start components, tiny and zero constants, near-cancelling real parts, constants at the edge of the host's
condition, far escape radii -- and compares |q|^2, dqs, the escape trip and the class test bit for bit.  Every
difference must come from a scene the host's orbit_x2_eligible() keeps on the plain trip, and the adversarial families
must produce some, or the comparison would prove nothing.  Tiny and zero start components are among the eligible
orbits: w_0^2 = 0.01 absorbs their squares, so the kernel tests nothing per step.  CPU only."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

SRC = Path(__file__).resolve().parent / "orbit_x2_emulator.c"


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler")
    exe = tmp_path_factory.mktemp("orbit_x2") / "orbit_x2_emulator"
    flags = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c99"]
    native = subprocess.run([cc, *flags, "-march=native", "-o", str(exe), str(SRC), "-lm"], capture_output=True, text=True)
    if native.returncode != 0:  # (a compiler without -march=native: libm's fmaf is exact either way)
        p = subprocess.run([cc, *flags, "-o", str(exe), str(SRC), "-lm"], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    return exe


def _run(exe, n, seed):
    p = subprocess.run([str(exe), str(n), str(seed)], capture_output=True, text=True, timeout=1800)
    m = re.search(r"orbits (\d+) differ (\d+) differ_eligible (\d+) ineligible (\d+)", p.stdout)
    assert m, p.stdout + p.stderr
    orbits, differ, eligible_diff, ineligible = map(int, m.groups())
    return p.returncode, orbits, differ, eligible_diff, ineligible, p.stderr


def test_the_doubled_trip_equals_the_plain_one_in_every_eligible_scene(emulator):
    n = int(os.environ.get("KIFS_ORBIT_X2_ORBITS", "20000000"))
    rc, orbits, differ, eligible_diff, ineligible, err = _run(emulator, n, 1)
    assert orbits == n
    assert eligible_diff == 0 and rc == 0, err
    # the adversarial families do reach the cases the host's condition exists for
    assert differ > n // 20000 and ineligible > differ
    # and most orbits run the doubled trip (the condition is not simply always off)
    assert ineligible < orbits // 2
