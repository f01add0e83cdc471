"""Frame scheduling of the fused render pass (wf_render_pass): the shadow stage of depth d on a stream of its own beside
the first half of depth d + 1 (WF_FRAME_OVERLAP = 0 serial | 1 every depth | 2 thin depths only), and no ray samples drawn at the last depth, where
nothing is shaded (WF_SAMPLES_SHADED = 1 | 0).  Neither may change a bit of the film or a ray count: escaped rays and emitter hits add
into the same pixels' L as the shadow stage before them, so a missing join shows as a float sum taken in another order."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, read_pfm

pytestmark = pytest.mark.gpu

# a Cornell-like box crossed by two "interface" quads: rays are re-pushed at the same depth (intersect.h:93-101), so a ray's path depth
# lags the pass's loop index, and a ray of the last loop index may still be shaded
INTERFACE_BOX = """
LookAt 0 -3.4 1  0 0 1  0 0 1
Camera "perspective" "float fov" [ 45 ]
Sampler "zsobol" "integer pixelsamples" [ 4 ]
Integrator "volpath" "integer maxdepth" [ 5 ]
Film "rgb" "string filename" [ "interface_box.pfm" ] "integer xresolution" [ 48 ] "integer yresolution" [ 48 ] "bool savefp16" [ false ]
WorldBegin
LightSource "infinite" "rgb L" [ 0.05 0.06 0.08 ]
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ 12 11 9 ]
  Shape "trianglemesh" "integer indices" [ 0 2 1 0 3 2 ] "point3 P" [ -0.3 -0.3 1.98  0.3 -0.3 1.98  0.3 0.3 1.98  -0.3 0.3 1.98 ]
AttributeEnd
Material "diffuse" "rgb reflectance" [ 0.7 0.7 0.7 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -1 -1 0  1 -1 0  1 1 0  -1 1 0 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -1 1 0  1 1 0  1 1 2  -1 1 2 ]
Material "diffuse" "rgb reflectance" [ 0.6 0.1 0.1 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -1 -1 0  -1 1 0  -1 1 2  -1 -1 2 ]
Material "conductor" "float roughness" [ 0.1 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ 1 -1 0  1 1 0  1 1 2  1 -1 2 ]
Material "interface"
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -1 -1 1.2  1 -1 1.2  1 1 1.2  -1 1 1.2 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -1 -0.5 0  1 -0.5 0  1 -0.5 2  -1 -0.5 2 ]
"""


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """name -> (path or None, inline text or None, spp, golden .pfm or None)"""
    from conftest import bench_small_scene
    sm, sm_spp = bench_small_scene("sanmiguel_like_small", tmp_path_factory.mktemp("sm"))
    g = lambda n: os.path.join(GOLDEN, n)
    return {
        "cornell64": (g("cornell64.pbrt"), None, 4, g("cornell64_ref.pfm")),
        "sanmiguel_like_small": (sm, None, sm_spp, g("sanmiguel_like_small_ref.pfm")),
        "instances": (g("instances.pbrt"), None, 4, g("instances_ref.pfm")),
        "spheres": (g("spheres.pbrt"), None, 4, g("spheres_ref.pfm")),
        "instances_quadrics": (g("instances_quadrics.pbrt"), None, 4, g("instances_quadrics_ref.pfm")),
        "media_box": (g("media_box.pbrt"), None, 4, None),
        "subsurface": (g("subsurface.pbrt"), None, 4, None),
        "interface_box": (None, INTERFACE_BOX, 4, None),
    }


class Env:
    def __init__(self, **env):
        self.env = {k: str(v) for k, v in env.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


_renders = {}


def render(wfpt, scenes, name, overlap=1, shaded=1, spp=None, repeats=1, **env):
    """One render per (scene, switches), shared by the tests: a renderer created anew under the two variables (they are read when the
    context is created) -> dict(film, image, stats, queries)"""
    key = (name, overlap, shaded, spp, repeats, tuple(sorted(env.items())))
    if key in _renders:
        return _renders[key]
    path, text, default_spp, _ = scenes[name]
    with Env(WF_FRAME_OVERLAP=overlap, WF_SAMPLES_SHADED=shaded, **env):
        s = wfpt.Scene(path=path, text=text, spp=default_spp if spp is None else spp)
        s.create_renderer(0)
        films = []
        for k in range(repeats):
            if k:
                s.clear_film()
            s.render()
            films.append(s.film().copy())
        r = dict(film=films[0], films=films, image=s.film_to_rgb(films[0]), stats=s.stats(),
                 q={k: s.query(k) for k in ("frame_overlap_active", "frame_overlap_mode", "skip_last_samples", "gen_mode", "fast_ok", "defer_general")})
        s.close()
    assert np.isfinite(r["film"]).all() and r["film"][..., :3].mean() > 0
    _renders[key] = r
    return r


def same_bits(a, b):
    return a.shape == b.shape and bool((np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all())


def differing(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


@pytest.mark.parametrize("name", ["cornell64", "sanmiguel_like_small", "instances"])
def test_overlap_modes_render_the_serial_film(wfpt, scenes, name):
    """serial (0), every depth (1), thin depths only (2): one film, one set of ray counts per stage and depth; the serial one is the
    committed golden (the reference's own render), bit for bit.  sanmiguel_like_small is the case the join is for: sky, sun and emitters
    add into the pixels the shadow stage of the depth before adds into."""
    base = render(wfpt, scenes, name, overlap=0)
    assert base["q"]["frame_overlap_active"] == 0 and base["q"]["frame_overlap_mode"] == 0
    ref = read_pfm(scenes[name][3])
    assert same_bits(base["image"], ref), (name, "serial vs golden", differing(base["image"], ref))
    for mode in (1, 2):
        r = render(wfpt, scenes, name, overlap=mode)
        assert r["q"]["frame_overlap_active"] == 1 and r["q"]["frame_overlap_mode"] == mode, (name, mode, r["q"])
        assert same_bits(r["film"], base["film"]), (name, mode, differing(r["film"], base["film"]))
        assert r["stats"] == base["stats"], (name, mode)


def test_overlap_beside_the_near_tie_retrace(wfpt, scenes):
    """a general-primitive scene: the near-tie re-trace of depth d + 1 on its stream and the shadow stage of depth d on its own are
    in flight together"""
    base = render(wfpt, scenes, "spheres", overlap=0)
    r = render(wfpt, scenes, "spheres", overlap=1)
    assert r["q"]["gen_mode"] >= 2 and r["q"]["fast_ok"] == 1 and r["q"]["frame_overlap_active"] == 1, r["q"]
    assert same_bits(r["film"], base["film"]), differing(r["film"], base["film"])
    assert r["stats"] == base["stats"]
    ref = read_pfm(scenes["spheres"][3])
    assert same_bits(base["image"], ref), differing(base["image"], ref)


def test_two_class_shadow_walk_aside(wfpt, scenes):
    """the two-class traversal (WF_DEFER_GENERAL=1): the any-hit triangle walk hands rays to a list of the shadow side's own
    (deferQShadow) while the next depth's closest-hit walk fills ws.deferQ"""
    base = render(wfpt, scenes, "instances_quadrics", overlap=0, WF_DEFER_GENERAL=1)
    r = render(wfpt, scenes, "instances_quadrics", overlap=1, WF_DEFER_GENERAL=1)
    assert r["q"]["defer_general"] == 1 and base["q"]["defer_general"] == 1 and r["q"]["frame_overlap_active"] == 1, r["q"]
    assert same_bits(r["film"], base["film"]), differing(r["film"], base["film"])
    assert r["stats"] == base["stats"]
    ref = read_pfm(scenes["instances_quadrics"][3])
    assert same_bits(base["image"], ref), differing(base["image"], ref)


@pytest.mark.parametrize("name", ["media_box", "subsurface"])
def test_media_and_subsurface_scenes_stay_serial(wfpt, scenes, name):
    base = render(wfpt, scenes, name, overlap=0)
    r = render(wfpt, scenes, name, overlap=1)
    assert r["q"]["frame_overlap_active"] == 0 and r["q"]["skip_last_samples"] == 0, r["q"]
    assert render(wfpt, scenes, "cornell64", overlap=1)["q"]["frame_overlap_active"] == 1
    assert same_bits(r["film"], base["film"]), (name, differing(r["film"], base["film"]))
    assert r["stats"] == base["stats"]


def test_overlapped_renders_repeat(wfpt, scenes):
    """six renders by one context with the overlap at every depth: one film (a race between the two streams would move a pixel sum),
    the serial context's"""
    r = render(wfpt, scenes, "sanmiguel_like_small", overlap=1, spp=16, repeats=6)
    for k, f in enumerate(r["films"][1:]):
        assert same_bits(f, r["films"][0]), (k + 1, differing(f, r["films"][0]))
    base = render(wfpt, scenes, "sanmiguel_like_small", overlap=0, spp=16)
    assert same_bits(r["film"], base["film"]), differing(r["film"], base["film"])


@pytest.mark.parametrize("name", ["cornell64", "sanmiguel_like_small", "interface_box", "spheres"])
def test_no_samples_at_the_last_depth(wfpt, scenes, name):
    """the pass without its last depth's sample launch (nothing is shaded there) against the pass that draws at every depth: one film.
    `interface_box` re-pushes rays at the same depth, so a ray of the last loop index is not at its path's last depth: the switch must
    leave such a scene (haveMedia) on the launch at every depth."""
    every = render(wfpt, scenes, name, overlap=0, shaded=0)
    only = render(wfpt, scenes, name, overlap=0, shaded=1)
    # (an "interface" material anywhere sets the scene's haveMedia, as in the reference: integrator.cpp:91-111 — such a scene keeps the
    #  launch at every depth, and its shadow stage stays serial)
    assert every["q"]["skip_last_samples"] == 0 and only["q"]["skip_last_samples"] == (0 if name == "interface_box" else 1)
    assert same_bits(only["film"], every["film"]), (name, differing(only["film"], every["film"]))
    assert only["stats"] == every["stats"]
    both = render(wfpt, scenes, name, overlap=1, shaded=1)
    assert same_bits(both["film"], every["film"]), (name, differing(both["film"], every["film"]))
    if scenes[name][3]:
        ref = read_pfm(scenes[name][3])
        assert same_bits(only["image"], ref), (name, differing(only["image"], ref))
