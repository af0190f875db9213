"""The form table (tests/kernel_forms.py) against what hipcc compiles: every render kernel instantiation `make report`
lists has a recipe, and every recipe names an instantiation that still exists.  A new template instantiation without a
recipe, or a recipe left behind by a removed one, fails here on the CPU, before any GPU run.  The recipes themselves are
checked for consistency with the launch plan the GPU test renders.  CPU only (hipcc cross-compiles)."""
import re
from pathlib import Path

import numpy as np
import pytest

import kernel_forms as F
from kernel_report import kernel_report

RENDER = re.compile(r"\bkifs::((ssaa|geom|adaptive|anim|accum|occl|light)::)?(jitter_|carry_)?render\w*_kernel\b")  # (not adaptive::classify_kernel: no render form)


def test_table_equals_the_compiled_render_instantiations():
    compiled = {n for n in kernel_report() if RENDER.search(n)}
    tables = [F.RENDER_FORMS, F.SSAA_FORMS, F.GEOMETRY_FORMS, F.ADAPTIVE_FORMS, F.ANIMATION_FORMS, F.ACCUMULATE_FORMS, F.JITTER_FORMS,
              F.CARRY_FORMS, F.OCCLUSION_FORMS, F.LIGHTING_FORMS]
    table = set().union(*tables)
    assert len(table) == sum(len(t) for t in tables)  # no instantiation in two tables
    assert not any("classify" in n for n in table) and any("adaptive::classify_kernel" in n for n in kernel_report())
    assert sorted(compiled - table) == [], "compiled, but no recipe in tests/kernel_forms.py"
    assert sorted(table - compiled) == [], "a recipe for an instantiation that is no longer compiled"
    assert len(F.ACCUMULATE_FORMS) == len(F.JITTER_FORMS) == len(F.CARRY_FORMS) == len(F.OCCLUSION_FORMS) == len(F.LIGHTING_FORMS) == 10
    # every extension table is claimed by a test file (test_extension_claims_name_cases_of_the_extension_tests runs per file)
    assert sorted(map(sorted, F.EXTENSION_FORMS.values())) == sorted(map(sorted, tables[2:]))


def test_ssaa_claims_name_cases_of_the_ssaa_test():
    text = (Path(__file__).resolve().parent / "test_gpu_ssaa.py").read_text()
    m = re.search(r'@pytest\.mark\.parametrize\("name", \[([^\]]*)\]\)\s*\n(?:@pytest\.mark\.parametrize\([^\n]*\n)*'
                  r'def test_aa_frame_bit_exact\(', text)
    assert m, "the parameter list of test_aa_frame_bit_exact"
    cases = set(re.findall(r'"([^"]+)"', m.group(1)))
    assert cases and set(F.SSAA_FORMS.values()) <= cases, sorted(set(F.SSAA_FORMS.values()) - cases)


@pytest.mark.parametrize("file", sorted(F.EXTENSION_FORMS))
def test_extension_claims_name_cases_of_the_extension_tests(file, kifs):
    """test_every_pipeline_bit_exact of the file runs every name of geometry_cases.PIPELINES, each claim names one of them,
    and the ten claims of a table name ten different pipelines: the (GROUP, PRIM) pair in the instantiation's name is the
    one dispatch_pipeline takes for that pipeline's scene in geometry_cases.cases."""
    from geometry_cases import PIPELINES, cases
    text = (Path(__file__).resolve().parent / file).read_text()
    assert re.search(r"^from geometry_cases import [^\n]*\bPIPELINES\b", text, re.M)
    assert re.search(r'@pytest\.mark\.parametrize\("name", PIPELINES\)\s*\n(?:@pytest\.mark\.parametrize\([^\n]*\n)*'
                     r'def test_every_pipeline_bit_exact\(', text), "the parameter list of test_every_pipeline_bit_exact"
    forms = F.EXTENSION_FORMS[file]
    assert len(forms) == 10 and sorted(forms.values()) == sorted(PIPELINES)
    scenes = cases(kifs, 64, 48)
    for name, pipeline in forms.items():
        _, _, gui, iters = scenes[pipeline]
        u = gui.into_buffer_data()
        group, prim = int(u.fractal_group_id), int(u.primitive_id)
        pair = (1, int(iters[0] <= 24)) if group == F.JULIA else (2, 0) if group == F.GENJULIA else (0, min(prim, F.PRIM_OTHER))
        assert re.search(r"\b(?:jitter_|carry_)?render_kernel<(\d+), (\d+)>", name).groups() == tuple(str(v) for v in pair), (name, pipeline)


@pytest.mark.parametrize("name", list(F.RENDER_FORMS))
def test_recipe_is_consistent_with_the_plan(name):
    """The recipe's configuration renders its scene in a batched launch, expects the recipe's tuple there, and that
    tuple maps back to this instantiation."""
    r = F.RENDER_FORMS[name]
    launches = [L for L in F.plan(r.config) if L.scene == r.scene and len(L.cams) == F.VIEWS and L.y1 is None]
    assert launches, (r.config, r.scene)
    for L in launches:
        assert F.expected_tuple(r.config, L) == r.tuple, (L.label, F.expected_tuple(r.config, L), r.tuple)
    assert F.instantiation(r.tuple, r.scene) == name


def test_the_plan_reaches_only_instantiations_of_the_table():
    reached = {F.instantiation(F.expected_tuple(c, L), L.scene) for c in F.CONFIGS for L in F.plan(c)}
    assert reached == set(F.RENDER_FORMS), (sorted(reached - set(F.RENDER_FORMS)), sorted(set(F.RENDER_FORMS) - reached))


def test_every_re_queuing_launch_re_queues():
    """The knobs force a form only where rounds run at all: every launch outside the block configuration re-queues, and
    the block configuration re-queues nothing."""
    for c in F.CONFIGS:
        for L in F.plan(c):
            t = F.expected_tuple(c, L)
            assert (t[3] == 0) == (c == "block"), (c, L.label, t)


def test_launch_geometry():
    w, h = F.FRAME
    n = F.tiles(w, h)
    assert (n, n % 2, w % F.TILE_W, h % F.TILE_H) == (209, 1, 10, 5)
    assert n * F.VIEWS >= F.REQUEUE_MIN_WORKGROUPS and F.tiles(w, h, *F.BAND) * F.VIEWS >= F.REQUEUE_MIN_WORKGROUPS
    assert F.BAND[0] % F.TILE_H and F.BAND[1] % F.TILE_H and (F.BAND[1] - F.BAND[0]) % F.TILE_H
    assert F.tiles(*F.LONE) >= F.REQUEUE_MIN_WORKGROUPS and F.BIG_VIEWS > F.MAX_BATCH_INLINE
    assert F.VIEWS >= 20 and F.VIEWS % len(F.CAMERAS) == 0
    for c in ("group1", "group2", "wave"):
        labels = [L.label for L in F.plan(c)]
        assert any(x.endswith("/band") for x in labels) and any(x.endswith("/shuffled") for x in labels)
        assert sum(x.endswith("/lone") for x in labels) == 2 and any(x.endswith(f"/views{F.BIG_VIEWS}") for x in labels)


def test_julia_variants_and_encodes():
    """The four Julia builds with constants far from the doubled trip's window edges, sdf_iters 24 and 25 on both
    sides of the divide / square root switch, and both encodes on every form for at least two pipelines."""
    slots = {F.prim_slot(s): s for s, v in F.SCENES.items() if v.group == F.JULIA}
    assert sorted(slots) == [0, 1, 2, 3]
    for s in slots.values():
        c = F.SCENES[s].constant
        assert (0.0 in c) != all(0.1 <= abs(x) <= 1.0 for x in c), c
        assert F.SCENES[s].iters[0] in (24, 25)
    for c in F.CONFIGS:
        both = {L.scene for L in F.plan(c) if L.encode == 0} & {L.scene for L in F.plan(c) if L.encode == 1}
        assert len({F.SCENES[s].group * 10 + min(F.SCENES[s].prim, 6) for s in both}) >= (1 if c.startswith("bunny") else 2), c


def test_child_environment_drops_every_kifs_variable():
    env = F.child_env({"PATH": "/bin", "KIFS_GROUP_TILES": "2", "KIFS_DEBUG": "1", "KIFS_TUNING": "0"}, "group1")
    assert env == {"PATH": "/bin", "KIFS_TUNING": "1", "KIFS_GROUP_TILES": "1"}


SHADOW_SCENES = [s for s, v in F.SCENES.items() if v.shadow]


@pytest.mark.parametrize("scene", SHADOW_SCENES)
def test_shadow_scene_has_occluded_and_unoccluded_hits(scene, oracle, kifs):
    """A `*_shadow` scene cannot pass vacuously: over the table's cameras the oracle's frame with the soft-shadow
    extension differs from its frame without it in some hit pixel (a secondary ray met the fractal) and equals it in
    some hit pixel (one did not, or none was cast).  From the oracle alone."""
    K, O = kifs, oracle
    assert scene.endswith("_shadow") and len(SHADOW_SCENES) == 5
    s, ub, ext = F.SCENES[scene], K.uniform_bytes, F.extensions(scene)

    def frame(cam, shadow):
        return O.render(O.from_bytes(O.Screen, ub(K.ScreenData(*F.FRAME).into_buffer_data())),
                        O.from_bytes(O.Camera, ub(F.camera(K, scene, cam).into_buffer_data())),
                        O.from_bytes(O.Options, ub(F.options(K, scene))), O.iters(*s.iters), encode=s.encodes[0],
                        ext=O.Ext(1, ext["shadow_steps"], ext["shadow_k"], ext["shadow_t0"], ext["shadow_max_t"])
                        if shadow else None)

    background = frame(len(F.CAMERAS) - 1, False)[0, 0]  # a corner of the far view
    differ = equal = 0
    for cam in range(len(F.CAMERAS)):
        plain, shadowed = frame(cam, False), frame(cam, True)
        hit = (plain != background).any(-1)
        changed = (plain != shadowed).any(-1)
        differ += int(np.count_nonzero(hit & changed))
        equal += int(np.count_nonzero(hit & ~changed))
    assert differ > 0 and equal > 0, (scene, differ, equal)
