"""The lean shade kernels' planned loads (DESIGN.md 4.2 "Load fronts"): k_mat_shade<type, 0 | 1> fetch an item's inputs in fronts and
park what they need late in LDS columns, one per lane.  Only when and how operands arrive may differ: every film stays what it was, bit
for bit, and so does every ray and item count.

Golden cases: matrix_lean / matrix_lean_tex (all ten types, variants 0 and 1), instances (object instances; its checkerboard cut-out makes
every type general, so it pins the untouched kernels beside the new code), media_instances (lean types through instances in a scene with
media: wo of a medium-stage item is not transformed), each under five legs: the default, WF_STAGE_GRID_CAP=1 and =3 (many grid-stride
iterations per workgroup: the parked columns are reused and the last batch is partial), WF_SHADE_TRIS=0 (the indexed vertex tables) and
WF_LEAN_SHADE=0 (the general kernels).  The film of every leg is the golden's committed reference render, bit for bit; ray counts per
depth and item counts per type are the default leg's; no queue or stack overflows.

Boundary cases: wall scenes (tests/test_stage_grids_gpu.py's construction: orthographic camera, one material stage, W x 1 pixels at 1 spp)
whose diffuse queue holds exactly 1, 63, 64, 65, 255, 256 and 257 items — a lane, a wave and a workgroup, one short and one over — as
  plain  one quad with (u, v) and vertex normals,
  bare   a mesh with neither,
  inst   a quad behind and, in front of its right part, a second one inside an ObjectInstance with a rotation, a translation and a
         non-uniform scale: the waves around the slanted edge mix inst = -1 and inst >= 0.
Witness: the CPU port's render of the same file, bit for bit, and the WF_LEAN_SHADE=0 leg — never the lean kernels' own earlier output.

Variant 1 through instances: matrix_lean_tex with each of its ten material quads moved into an object definition and placed by an
ObjectInstance under the quad's own transformation and a non-uniform scale — the footprint / bump block and the normal map of every
type's variant 1 kernel on interactions that came through InstanceInteraction on fetched rows.  Same legs' worth of witnesses: the CPU
port and the general kernels.

(No torch in this module: DESIGN 8, renderer creation after torch initialises.)"""
import contextlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, read_pfm, run_wf_cpu
from suite_helpers import assert_image_parity

pytestmark = pytest.mark.gpu

SWITCHES = ("WF_STAGE_GRID_CAP", "WF_SHADE_TRIS", "WF_LEAN_SHADE", "WF_LEAN_PER_TYPE", "WF_VISIBLE_SURFACE", "WF_STAGE_ROUNDS")
LEGS = {"default": {}, "cap1": {"WF_STAGE_GRID_CAP": "1"}, "cap3": {"WF_STAGE_GRID_CAP": "3"}, "indexed": {"WF_SHADE_TRIS": "0"},
        "general": {"WF_LEAN_SHADE": "0"}}
DIFFUSE = 1
# scene -> the shade variant its own plan gives the types with items (tests/variant_matrix_cases.py), None: not asserted per type
GOLDENS = {"matrix_lean": 0, "matrix_lean_tex": 1, "instances": 2, "media_instances": 0}


@contextlib.contextmanager
def switches(env):
    """the environment of one leg (the switches are read at upload), put back afterwards"""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def render(wfpt, path, spp, env):
    with switches(env):
        s = wfpt.Scene(path=path, spp=spp)
        try:
            s.create_renderer(0)
            variants = {t: s.query("shade_variant_%d" % t) for t in range(1, 11)}
            cap = s.query("stage_grid_cap")
            tris = s.query("shade_tris")
            s.debug_counters(reset=True)
            s.clear_film()
            s.render(0, spp, 1)
            img = s.image()
            dbg = s.debug_counters(reset=True)
            return dict(img=img, stats=s.stats(), items=s.material_items(), overflow=dbg["overflow"], variants=variants, cap=cap, shade_tris=tris)
        finally:
            s.close()


@pytest.fixture(scope="module")
def default_leg(wfpt):
    """scene -> the default leg's render, made once and shared by the scene's legs"""
    cache = {}

    def get(scene):
        if scene not in cache:
            cache[scene] = render(wfpt, os.path.join(GOLDEN, scene + ".pbrt"), 4, {})
            cache[scene]["img"].setflags(write=False)
        return cache[scene]
    return get


@pytest.mark.parametrize("leg", list(LEGS))
@pytest.mark.parametrize("scene", list(GOLDENS))
def test_golden_films_and_counts_under_every_leg(wfpt, default_leg, scene, leg):
    base = default_leg(scene)
    r = base if leg == "default" else render(wfpt, os.path.join(GOLDEN, scene + ".pbrt"), 4, LEGS[leg])
    used = [t for t in range(1, 11) if base["items"][t] > 0]
    assert used, scene
    if scene.startswith("matrix_lean"):
        assert used == list(range(1, 11)), (scene, base["items"])   # all ten types have items
    assert r["shade_tris"] == (0 if leg == "indexed" else 1), (scene, leg)   # the indexed leg really runs without the de-indexed records
    want = 2 if leg == "general" else GOLDENS[scene]
    assert {t: r["variants"][t] for t in used} == {t: want for t in used}, (scene, leg, r["variants"])
    assert r["cap"] == int(LEGS[leg].get("WF_STAGE_GRID_CAP", 0))
    assert r["overflow"] == 0
    assert r["stats"] == base["stats"], (scene, leg)   # camera rays, indirect and shadow rays per depth
    assert r["items"] == base["items"], (scene, leg)
    ref = read_pfm(os.path.join(GOLDEN, scene + "_ref.pfm"))   # the reference's own CPU wavefront render
    assert_image_parity(scene, r["img"], ref)                  # bit-identical: NOT_BIT_IDENTICAL is empty


HEAD = """
LookAt 0 0 0  0 0 1  0 1 0
Camera "orthographic" "float screenwindow" [ -1 1 -1 1 ]
Sampler "zsobol" "integer pixelsamples" [ 1 ]
Integrator "volpath" "integer maxdepth" [ 1 ]
Film "rgb" "string filename" [ "wall.pfm" ] "integer xresolution" [ %d ] "integer yresolution" [ 1 ] "bool savefp16" [ false ]
WorldBegin
LightSource "point" "point3 from" [ 0.3 0.4 0 ] "rgb I" [ 5 5 5 ]
Material "diffuse" "rgb reflectance" [ 0.6 0.5 0.4 ]
"""
QUAD_UV_N = """Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ %s ]
  "point2 uv" [ 0 0  1 0  1 1  0 1 ] "normal N" [ 0.1 0.05 -1  -0.1 0.05 -1  -0.1 -0.05 -1  0.1 -0.05 -1 ]
"""
WALLS = {
    "plain": HEAD + QUAD_UV_N % "-5 -5 2  5 -5 2  5 5 2  -5 5 2",
    "bare": HEAD + 'Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -5 -5 2  5 -5 2  5 5 2  -5 5 2 ]\n',
    # the instanced quad: x in [-1.5, 1.5], y in [-3, 3] after the scale, turned 20 degrees about z, moved to x = 1.6 — its left edge
    # crosses the view between x = -0.15 and 0.55 — and to z = 1.996, a hair in front of the wall at z = 2 and parallel to it: a bounce
    # off the wall would have to leave within 0.004 tan(theta) of the edge to meet the panel's back, and none of these does (the
    # item counts below are asserted), so the queue holds the camera rays' hits only
    "inst": HEAD + QUAD_UV_N % "-5 -5 2  5 -5 2  5 5 2  -5 5 2" + """ObjectBegin "panel"
  Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -1 -1 0  1 -1 0  1 1 0  -1 1 0 ]
    "point2 uv" [ 0 0  1 0  1 1  0 1 ] "normal N" [ 0 0 -1  0 0 -1  0 0 -1  0 0 -1 ]
ObjectEnd
AttributeBegin
  Translate 1.6 0 1.996
  Rotate 20 0 0 1
  Scale 1.5 3 0.8
  ObjectInstance "panel"
AttributeEnd
""",
}
SIZES = (1, 63, 64, 65, 255, 256, 257)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", list(WALLS))
def test_wall_queues_of_boundary_sizes(wfpt, tmp_path, kind, n):
    path = str(tmp_path / ("wall_%s_%d.pbrt" % (kind, n)))
    with open(path, "w") as f:
        f.write(WALLS[kind] % n)
    out = str(tmp_path / "cpu.pfm")
    j = run_wf_cpu(path, out, 1)
    cpu = read_pfm(out)
    assert np.isfinite(cpu).all() and cpu.mean() > 0
    lean, general = render(wfpt, path, 1, {}), render(wfpt, path, 1, {"WF_LEAN_SHADE": "0"})
    assert lean["variants"][DIFFUSE] == 0 and general["variants"][DIFFUSE] == 2
    for r in (lean, general):
        assert r["overflow"] == 0
        assert r["stats"]["camera_rays"] == n == j["camera_rays"]
        # the diffuse queue holds exactly n items, read back from the material stage's counts
        assert {t: v for t, v in enumerate(r["items"][t] for t in range(11)) if v} == {DIFFUSE: n}, (kind, n, r["items"])
        assert [r["items"][t] for t in range(11)] == j["material_items"]
        assert r["stats"]["shadow_rays"] == lean["stats"]["shadow_rays"]
    assert lean["img"].shape == cpu.shape
    assert (lean["img"].view(np.uint32) == cpu.view(np.uint32)).all(), (kind, n)
    assert (general["img"].view(np.uint32) == cpu.view(np.uint32)).all(), (kind, n)


def instanced_matrix_tex():
    """matrix_lean_tex.pbrt with every material quad (the blocks that have a Translate) inside an object definition of its own"""
    text = open(os.path.join(GOLDEN, "matrix_lean_tex.pbrt")).read()
    for name in ("png_rgb8.png", "png_rgb16.png", "png_pal8.png", "png_grey8.png", "png_normal.png", "measured_iso.bsdf"):
        text = text.replace('"%s"' % name, '"%s"' % os.path.join(GOLDEN, name))
    out, n = [], 0
    for block in text.split("AttributeBegin\n"):
        lines = block.split("\n")
        if lines[0].lstrip().startswith("Translate"):
            place = [l for l in lines if l.lstrip().startswith(("Translate", "Rotate"))]
            material = [l for l in lines if l.lstrip().startswith("Material")]
            shape = [l for l in lines if l.lstrip().startswith("Shape")]
            rest = lines[lines.index("AttributeEnd") + 1:]
            assert len(material) == 1 and len(shape) == 1, block
            name = "quad%d" % n
            n += 1
            lines = material + ['  ObjectBegin "%s"' % name] + shape + ["  ObjectEnd", "AttributeEnd", "AttributeBegin"] + place + \
                    ["  Scale 1.1 0.9 1.2", '  ObjectInstance "%s"' % name, "AttributeEnd"] + rest
        out.append("\n".join(lines))
    assert n == 10
    return "AttributeBegin\n".join(out)


def test_variant_1_kernels_through_instances(wfpt, tmp_path):
    path = str(tmp_path / "matrix_lean_tex_instanced.pbrt")
    with open(path, "w") as f:
        f.write(instanced_matrix_tex())
    out = str(tmp_path / "cpu.pfm")
    j = run_wf_cpu(path, out, 4)
    cpu = read_pfm(out)
    assert all(v > 0 for v in j["material_items"][1:11]), j["material_items"]   # every type's queue holds items
    lean, general = render(wfpt, path, 4, {}), render(wfpt, path, 4, {"WF_LEAN_SHADE": "0"})
    assert lean["variants"] == {t: 1 for t in range(1, 11)} and general["variants"] == {t: 2 for t in range(1, 11)}
    for r in (lean, general):
        assert r["overflow"] == 0
        assert [r["items"][t] for t in range(11)] == j["material_items"]
        assert r["stats"]["camera_rays"] == j["camera_rays"] and r["stats"] == lean["stats"]
        assert r["img"].shape == cpu.shape and (r["img"].view(np.uint32) == cpu.view(np.uint32)).all()
