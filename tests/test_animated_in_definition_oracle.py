"""Animated shapes inside object instance definitions (CPU checker, no GPU).

`Shape` under an animated CTM inside ObjectBegin ... ObjectEnd (BasicSceneBuilder::Shape, scene.cpp:277-290) is an AnimatedPrimitive among the
definition's primitives (scene.cpp:1530-1551): a ray passes two transformations, the use of the definition and the moving entity, each static
or interpolated at the ray's time (cpu/primitive.cpp:112-158).  The goldens are pbrt_ref --wavefront renders (tools/make_golden.sh)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, WF_CPU, read_pfm, run_wf_cpu

SCENES = ["animated_in_definition", "animated_in_definition_general", "animated_in_definition_media", "animated_in_definition_sss"]
PBRT_REF = os.path.join(ROOT, "oracle", "_ref", "pbrt_ref")
INSTANCING_WARNING = "Area lights not supported with object instancing"
ANIMATED_LIGHT_ERROR = "Animated area lights are not supported."


@pytest.mark.parametrize("scene", SCENES)
def test_scene_loader_admits_animated_shapes_inside_definitions(wfpt, scene):
    """the loader builds the scenes (it stopped with a fatal error at every one of them before)"""
    text = open(os.path.join(GOLDEN, scene + ".pbrt")).read()
    assert _nested_sections(text) > 0
    s = wfpt.Scene(path=os.path.join(GOLDEN, scene + ".pbrt"), spp=4)
    assert s.width > 0 and s.height > 0


@pytest.mark.parametrize("scene", SCENES)
def test_cpu_checker_renders_nested_animated_shapes_like_the_reference(built, tmp_path, scene):
    """oracle/wf_cpu against pbrt_ref --wavefront (tests/golden/<scene>_ref.pfm): bit-identical"""
    ref = read_pfm(os.path.join(GOLDEN, scene + "_ref.pfm"))
    out = str(tmp_path / "cpu.pfm")
    j = run_wf_cpu(os.path.join(GOLDEN, scene + ".pbrt"), out, 4)
    img = read_pfm(out)
    assert img.shape == ref.shape
    assert j["camera_rays"] == 4 * img.shape[0] * img.shape[1]
    assert (img.view(np.uint32) == ref.view(np.uint32)).all(), "fraction identical: %f" % (img == ref).mean()


def _frozen_twin(text):
    """the scene with the motion of every shape INSIDE a definition frozen at its start: each `ActiveTransform EndTime ... ActiveTransform All`
    section between ObjectBegin and ObjectEnd (which moves the end transformation only) removed; the uses of the definitions keep theirs"""
    out, skipping, inside = [], False, False
    for line in text.splitlines():
        key = line.strip()
        if key.startswith("ObjectBegin"):
            inside = True
        elif key == "ObjectEnd":
            inside = False
        if inside and key == "ActiveTransform EndTime":
            skipping = True
            continue
        if inside and skipping and key == "ActiveTransform All":
            skipping = False
            continue
        if not skipping:
            out.append(line)
    return "\n".join(out) + "\n"


def _nested_sections(text):
    n, inside = 0, False
    for line in text.splitlines():
        key = line.strip()
        if key.startswith("ObjectBegin"):
            inside = True
        elif key == "ObjectEnd":
            inside = False
        n += inside and key == "ActiveTransform EndTime"
    return n


@pytest.mark.parametrize("scene", SCENES)
def test_the_goldens_depend_on_the_nested_motion(built, tmp_path, scene):
    """the parity test above cannot pass on a scene that lost its point: with the nested shapes frozen at their start (still inside their
    definitions, the uses still moving) at least 5 % of the pixels differ from the golden (the reference's own margin: 12 % or more)"""
    text = open(os.path.join(GOLDEN, scene + ".pbrt")).read()
    frozen = _frozen_twin(text)
    assert frozen != text and _nested_sections(frozen) == 0 and frozen.count("Shape") == text.count("Shape")
    path = tmp_path / (scene + "_frozen.pbrt")
    path.write_text(frozen)
    out = str(tmp_path / "frozen.pfm")
    run_wf_cpu(str(path), out, 4)
    img, ref = read_pfm(out), read_pfm(os.path.join(GOLDEN, scene + "_ref.pfm"))
    differ = (img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).mean()
    print("%s: %.1f %% of the pixels differ from the golden with the nested motion frozen" % (scene, 100 * differ))
    assert differ >= 0.05


HEAD = """LookAt 0 -8 3.5  0 0 0.8  0 0 1
Camera "perspective" "float fov" [ 40 ] "float shutteropen" [ 0 ] "float shutterclose" [ 1 ]
Sampler "zsobol" "integer pixelsamples" [ 4 ]
Integrator "volpath" "integer maxdepth" [ 3 ]
Film "rgb" "string filename" [ "x.pfm" ] "integer xresolution" [ 48 ] "integer yresolution" [ 32 ] "bool savefp16" [ false ]
WorldBegin
LightSource "distant" "point3 from" [ 2 -4 6 ] "point3 to" [ 0 0 0 ] "rgb L" [ 2.5 2.4 2.2 ]
LightSource "infinite" "rgb L" [ 0.3 0.35 0.45 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -7 -7 0  7 -7 0  7 7 0  -7 7 0 ]
"""
MOVING_BLADE = """  AttributeBegin
    Material "diffuse" "rgb reflectance" [ 0.8 0.3 0.2 ]
    Translate 0 0 0.6
    ActiveTransform EndTime
    Translate 0.8 0 0.4
    Rotate 50 0 0 1
    ActiveTransform All
    %s
    Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -0.8 -0.5 0  0.8 -0.5 0  0.8 0.5 0.3  -0.8 0.5 0 ]
  AttributeEnd
"""
USES = """AttributeBegin
  Translate -1.5 0.5 0.1
  ObjectInstance "part"
AttributeEnd
AttributeBegin
  Translate 1.6 -0.5 0.2
  ActiveTransform EndTime
  Translate 0.4 0.6 0.5
  ActiveTransform All
  ObjectInstance "part"
AttributeEnd
"""


def test_area_light_on_a_nested_animated_shape_warns_then_fails_like_the_reference(built, tmp_path):
    """scene.cpp:1484-1487: the instancing warning, then ErrorExit("Animated area lights are not supported.")"""
    path = tmp_path / "light.pbrt"
    path.write_text(HEAD + 'ObjectBegin "part"\n' + MOVING_BLADE % 'AreaLightSource "diffuse" "rgb L" [ 4 4 4 ]' + "ObjectEnd\n" + USES)
    p = subprocess.run([WF_CPU, "--quiet", "--spp", "4", "--outfile", str(tmp_path / "x.pfm"), str(path)], capture_output=True, text=True)
    assert p.returncode != 0
    assert INSTANCING_WARNING in p.stderr and ANIMATED_LIGHT_ERROR in p.stderr, p.stderr
    assert p.stderr.index(INSTANCING_WARNING) < p.stderr.index(ANIMATED_LIGHT_ERROR)
    warning = [l for l in p.stderr.splitlines() if INSTANCING_WARNING in l][0]
    assert warning.startswith("Warning: ") and "light.pbrt" in warning


@pytest.mark.parametrize("case", ["only_a_moving_entity", "definition_never_used"])
def test_degenerate_definitions_load_and_render(built, tmp_path, case):
    """a definition whose only content is one moving entity; a definition with a moving entity that no ObjectInstance names"""
    if case == "only_a_moving_entity":
        text = HEAD + 'ObjectBegin "part"\n' + MOVING_BLADE % "" + "ObjectEnd\n" + USES
    else:
        text = (HEAD + 'ObjectBegin "unused"\n' + MOVING_BLADE % "" + "ObjectEnd\n" +
                'ObjectBegin "part"\n  Shape "trianglemesh" "integer indices" [ 0 1 2 ] "point3 P" [ -0.5 0 0  0.5 0 0  0 0 1.2 ]\nObjectEnd\n' + USES)
    path = tmp_path / (case + ".pbrt")
    path.write_text(text)
    out = str(tmp_path / "cpu.pfm")
    j = run_wf_cpu(str(path), out, 4)
    img = read_pfm(out)
    assert img.shape == (32, 48, 3) and np.isfinite(img).all() and img.mean() > 0.01 and j["camera_rays"] == 4 * 32 * 48
    if case == "only_a_moving_entity":
        # the entity is seen, and seen moving: the frozen twin renders another image
        frozen = tmp_path / "frozen.pbrt"
        frozen.write_text(_frozen_twin(text))
        out_f = str(tmp_path / "frozen.pfm")
        run_wf_cpu(str(frozen), out_f, 4)
        assert (read_pfm(out_f) != img).any(axis=2).mean() > 0.01
    if os.path.exists(PBRT_REF):
        ref_out = str(tmp_path / "ref.pfm")
        subprocess.run([PBRT_REF, "--wavefront", "--quiet", "--seed", "0", "--spp", "4", "--outfile", ref_out, str(path)], check=True, capture_output=True)
        ref = read_pfm(ref_out)
        assert (ref.view(np.uint32) == img.view(np.uint32)).all(), "fraction identical: %f" % (ref == img).mean()


def test_table_cache_serves_a_scene_with_nested_placements(wfpt, tmp_path, monkeypatch):
    """WF_TABLE_CACHE: the second load comes from the table file written by the first, with the same counts (the GPU suite renders from it)"""
    path = os.path.join(GOLDEN, "animated_in_definition.pbrt")
    monkeypatch.setenv("WF_TABLE_CACHE", str(tmp_path))
    a = wfpt.Scene(path=path, spp=4)
    files = [f for f in os.listdir(tmp_path) if f.endswith(".wftab")]
    assert len(files) == 1
    mtime = os.path.getmtime(os.path.join(tmp_path, files[0]))
    b = wfpt.Scene(path=path, spp=4)
    assert os.path.getmtime(os.path.join(tmp_path, files[0])) == mtime and len(os.listdir(tmp_path)) == 1
    for f in ("width", "height", "spp", "n_triangles", "n_bvh_nodes", "n_lights", "max_depth"):
        assert getattr(a.info, f) == getattr(b.info, f)
    a.close(); b.close()


# per scene: uses of the definition, moving entities inside it, quadrics / patches in the whole scene (from the scene files)
LAYOUT = {"animated_in_definition": (3, 2, 0), "animated_in_definition_general": (3, 4, 3),
          "animated_in_definition_media": (2, 1, 0), "animated_in_definition_sss": (2, 1, 0)}


@pytest.mark.parametrize("scene", SCENES)
def test_bvh_prims_holds_a_nested_placement_once_per_definition(wfpt, scene):
    """The length of bvh_prims that wf_scene_upload copies is what the trees' leaves index: every triangle / quadric once, every use of the
    definition once, every moving entity ONCE — while `instances` repeats the entity's record per use.  (Sized as n_triangles + n_quadrics
    + n_instances the copy read (uses - 1) x entities ints past the end of the table: 4 on animated_in_definition, 8 on _general.)
    wf_scene_check_instances also range-checks the nested-placement words of every record; it runs without a device."""
    uses, entities, quadrics = LAYOUT[scene]
    text = open(os.path.join(GOLDEN, scene + ".pbrt")).read()
    assert text.count("ObjectInstance") == uses and _nested_sections(text) <= entities
    s = wfpt.Scene(path=os.path.join(GOLDEN, scene + ".pbrt"), spp=4)
    c = s.check_instances()
    n_geom = s.info.n_triangles + quadrics
    s.close()
    assert c["top_level_instances"] == uses and c["nested_entries"] == entities and c["nested_records"] == uses * entities
    assert c["bvh_prims"] == n_geom + uses + entities
    assert c["bvh_prims"] == n_geom + c["top_level_instances"] + c["nested_records"] - (uses - 1) * entities


@pytest.mark.parametrize("scene", ["instances", "instances_quadrics", "media_instances", "animated", "animated_interface", "cornell64"])
def test_instance_table_check_passes_on_scenes_without_nested_placements(wfpt, scene):
    """... and there the length is the one it always was: every primitive and every instance record once"""
    s = wfpt.Scene(path=os.path.join(GOLDEN, scene + ".pbrt"), spp=4)
    c = s.check_instances()
    n_tri = s.info.n_triangles
    s.close()
    assert c["nested_records"] == 0 and c["nested_entries"] == 0
    assert c["bvh_prims"] >= n_tri + c["top_level_instances"]
    if scene == "cornell64":
        assert c["top_level_instances"] == 0 and c["bvh_prims"] == n_tri


def test_reference_order_stack_stays_inline_in_the_device_code(built, tmp_path):
    """LdsStack::push / pop must not exist as out-of-line device functions: one that touches g_sstack changes how every LDS array of the
    traversal unit is lowered (LdsStackT::push then looks g_tstack up in a per-kernel table), in the static scenes' kernels too — which is
    how a change to the ANIM walks once reached them.  Also runs tools/isa_compare.py, the comparison that shows a change ISA-neutral for
    the functions it is not meant to touch, on the unit against itself."""
    import isa_compare
    import isa_dump
    obj = os.path.join(ROOT, "pbrt-v4_amd", "_build", "wf_backend.o")
    assert os.path.exists(obj), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    out = str(tmp_path / "isa")
    isa_dump.main(obj, out)
    names = os.listdir(out)
    assert any(n.startswith("_Z19k_intersect_closestILb0ELb1EE") for n in names), "the ANIM reference-order kernel is in this unit"
    assert [n for n in names if "8LdsStack" in n] == []
    assert isa_compare.compare(out, out) == ([], [], [])
    # a body that differs in more than a pc-relative literal is reported; one that differs in the literal alone is not
    other = tmp_path / "isa2"
    other.mkdir()
    victim = sorted(n for n in names if n.startswith("_Z19k_intersect_closest"))[0]
    for n in names:
        t = open(os.path.join(out, n)).read()
        if n == victim:
            t = t.replace("s_endpgm", "s_nop 0\n\ts_endpgm", 1)
        else:
            t = isa_compare._LITERAL.sub(r"\1 \2, \3, 0x1234", t)
        (other / n).write_text(t)
    assert isa_compare.compare(out, str(other)) == ([], [], [victim[:-2]])
