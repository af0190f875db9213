"""Resource ceilings of every gfx950 kernel, from hipcc's own report (`make -C csrc report`):
no scratch, no spills, VGPR budgets per pipeline.  The hand-written loops pin physical registers
(v30-v63, s74-s97: kifs_scene.hpp, kifs_julia_march_asm.hpp); after a toolchain bump or an edit
this is the test that notices a spill or a lost occupancy step.  CPU only (hipcc cross-compiles)."""
import re

import pytest

from kernel_report import kernel_report


@pytest.fixture(scope="module")
def report():
    return kernel_report()


def _budget(name):
    """(max VGPRs, min waves per SIMD) for a kernel by its demangled name."""
    m = re.search(r"render(?:_group|_wave)?_kernel<(\d+), (\d+)(?:, (\d+))?(?:, (true|false))?>", name)
    if "bunny_coop" in name:
        return 64, 6                       # weights as scalar operands; 24 KB of LDS allow six workgroups per CU
    if m and m.group(1) == "0" and m.group(2) == "5" and m.group(4) == "true":
        return 168, 3                      # the bunny with layer 2 of its network in LDS: the third wave per SIMD is the point
    if "bunny_quad" in name or (m and m.group(1) == "0" and m.group(2) == "5"):
        return 224, 2                      # the bunny keeps 156 weights per lane in registers
    if m:
        group, tiles = int(m.group(1)), int(m.group(3) or 0)
        vgprs = 80 if group in (1, 2) else 64   # Julia / gen-Julia: v30-v63 pinned + compiler's; KIFS: <= 64
        return vgprs, 6                         # (and 106 SGPRs allow six waves per SIMD, whatever the API says)
    return 64, 8                           # tile order, unpack, point and math evaluation


def test_every_kernel_is_reported(report):
    have = " ".join(report)
    for needle in ["render_kernel<1, 0>", "render_kernel<1, 1>", "render_kernel<2, 0>", "render_kernel<0, 4>",
                   "render_group_kernel<1, 1, 2, false>", "render_group_kernel<0, 4, 2, false>", "render_group_kernel<0, 5, 1, false>",
                   "render_group_kernel<0, 5, 2, true>",
                   "render_wave_kernel<1, 1>", "render_wave_kernel<0, 4>", "render_wave_kernel<2, 0>",
                   "render_bunny_quad_kernel", "render_bunny_coop_kernel<2>", "tile_order_kernel", "unpack_stripes_kernel"]:
        assert needle in have, needle
    assert len(report) >= 40


def test_no_scratch_no_spills_and_register_budgets(report):
    bad = []
    for name, r in report.items():
        vmax, occ_min = _budget(name)
        if int(r["ScratchSize [bytes/lane]"]) != 0 or int(r["VGPRs Spill"]) != 0:
            bad.append((name, "scratch/spill", r))
        # SGPR "spills" live in lanes of a VGPR (v_writelane / v_readlane), never in memory.  The frame
        # constants alone are ~70 SGPRs and the hand-written loops pin s74-s97, so the Julia kernels park
        # some constants that way outside their loops (21-44 today); everything else must not spill.
        # (render_bunny_coop_kernel: the frame constants plus sixteen weights at a time, 60 parked)
        sgpr_max = (48 if re.search(r"render(_group|_wave)?_kernel<[12], ", name) else 64 if "bunny_coop" in name
                    else 4 if "render" in name else 0)
        if int(r["SGPRs Spill"]) > sgpr_max:
            bad.append((name, f"SGPR spills {r['SGPRs Spill']} > {sgpr_max}", r))
        if r.get("Dynamic Stack") != "False":
            bad.append((name, "dynamic stack", r))
        if int(r["VGPRs"]) > vmax or int(r["AGPRs"]) != 0:
            bad.append((name, f"VGPRs {r['VGPRs']} > {vmax}", r))
        if int(r["Occupancy [waves/SIMD]"]) < occ_min:
            bad.append((name, f"occupancy {r['Occupancy [waves/SIMD]']} < {occ_min}", r))
    assert not bad, [b[:2] for b in bad]
