"""hipcc's resource report of every gfx950 kernel (`make -C kifs_raymarching_amd/csrc report`), parsed once per session:
{demangled name: {remark: value}}.  Shared by the resource ceilings and the kernel-form table's coverage test."""
import functools
import re
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "kifs_raymarching_amd" / "csrc"


@functools.lru_cache(maxsize=None)
def kernel_report():
    p = subprocess.run(["make", "-C", str(CSRC), "report"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    kernels, cur = {}, None
    for line in (p.stdout + p.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    names = subprocess.run(["c++filt"] + list(kernels), capture_output=True, text=True).stdout.split("\n")
    return {n.strip(): v for n, v in zip(names, kernels.values())}
