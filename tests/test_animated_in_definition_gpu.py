"""Animated shapes inside object instance definitions on the MI355X: the renders, the walk they take, the timed boundary entry points and the
product binary.  (Scenes and goldens: tests/test_animated_in_definition_oracle.py.)

Such scenes are walked by the reference-order kernels' ANIM variants (k_intersect_closest<*, true>, k_intersect_shadow<*, true>,
k_shadow_tr<true>, k_intersect_one_random<true>), which take the third level — use of the definition, then the moving entity — from the
shared walk code; the production tree has no entry form for a nested placement yet, so `anim_fast` is 0 whenever `nested_animated` > 0."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, WF_CPU, read_pfm
from suite_helpers import _check_image_vs_oracle_and_reference

pytestmark = pytest.mark.gpu

SCENES = ["animated_in_definition", "animated_in_definition_general", "animated_in_definition_media", "animated_in_definition_sss"]
# per scene, from the scene files: uses of its one definition (ObjectInstance), moving entities inside it (Shape under an animated CTM)
LAYOUT = {"animated_in_definition": (3, 2), "animated_in_definition_general": (3, 4), "animated_in_definition_media": (2, 1), "animated_in_definition_sss": (2, 1)}
# nested placements: one record of `instances` per (use, moving entity)
NESTED = {name: uses * entities for name, (uses, entities) in LAYOUT.items()}


def _open(wfpt, name):
    s = wfpt.Scene(path=os.path.join(GOLDEN, name + ".pbrt"), spp=4)
    s.create_renderer(0)
    return s


def _query(wfpt, name, keys):
    s = _open(wfpt, name)
    r = {k: s.query(k) for k in keys}
    s.close()
    return r


def _nested_mask(scene, name, instance):
    """which hit records name a nested placement.  The layout is the documented one (include/wf_abi.h wf_instance): every use of a definition
    is followed in `instances` by one record per moving entity of the definition; these scenes hold one definition and nothing else that is
    an instance, so with the scene file's own counts the records are exactly `uses` groups of 1 + `entities`, each led by the use."""
    uses, entities = LAYOUT[name]
    text = open(os.path.join(GOLDEN, name + ".pbrt")).read()
    assert text.count("ObjectBegin") == 1 and text.count("ObjectInstance") == uses
    assert scene.query("instances") == uses * (1 + entities) and scene.query("nested_animated") == uses * entities
    assert (instance < uses * (1 + entities)).all()
    return (instance >= 0) & (instance % (1 + entities) != 0)


@pytest.mark.parametrize("name", SCENES)
def test_nested_animated_shapes_render_like_the_reference(wfpt, tmp_path, monkeypatch, name):
    """bit-identical with wf_cpu and with pbrt_ref --wavefront, equal ray counts, on the default walk and with WF_ANIM_FAST=0"""
    assert _query(wfpt, name, ["nested_animated"])["nested_animated"] == NESTED[name]
    _check_image_vs_oracle_and_reference(wfpt, tmp_path, name)
    monkeypatch.setenv("WF_ANIM_FAST", "0")
    assert _query(wfpt, name, ["anim_fast"])["anim_fast"] == 0
    _check_image_vs_oracle_and_reference(wfpt, tmp_path, name)


def test_scenes_with_nested_placements_take_the_reference_order_walks(wfpt, monkeypatch):
    """the path the renders above took: nested placements present, and every walk in reference order (the production tree does not hold
    nested placements; their un-nested counterparts `animated_tris` / `animated_interface` stay on the production walk)"""
    for name in SCENES:
        assert _query(wfpt, name, ["anim_fast", "fast_ok", "nested_animated"]) == {"anim_fast": 0, "fast_ok": 0, "nested_animated": NESTED[name]}, name
    assert _query(wfpt, "animated_interface", ["anim_fast", "fast_ok", "nested_animated"]) == {"anim_fast": 1, "fast_ok": 1, "nested_animated": 0}
    assert _query(wfpt, "instances", ["nested_animated"]) == {"nested_animated": 0}
    monkeypatch.setenv("WF_ANIM_FAST", "0")
    for name in SCENES:
        assert _query(wfpt, name, ["anim_fast"]) == {"anim_fast": 0}, name


def test_table_cache_round_trips_nested_placements(wfpt, tmp_path, monkeypatch):
    """WF_TABLE_CACHE: the scene served from the table file (second load) renders the golden too"""
    monkeypatch.setenv("WF_TABLE_CACHE", str(tmp_path / "cache"))
    os.makedirs(str(tmp_path / "cache"))
    for _ in range(2):
        _check_image_vs_oracle_and_reference(wfpt, tmp_path, "animated_in_definition")
        assert len([f for f in os.listdir(str(tmp_path / "cache")) if f.endswith(".wftab")]) == 1


def _camera(name):
    for line in open(os.path.join(GOLDEN, name + ".pbrt")):
        if line.startswith("LookAt"):
            return np.array([float(v) for v in line.split()[1:4]], dtype=np.float32)
    raise AssertionError("no LookAt")


def _aimed_rays(name, n, seed, centres, reach):
    """rays from around the scene THROUGH the neighbourhood of the definition's uses (world space -> rendering space, "cameraworld": the
    world translated by minus the camera's position)"""
    rng = np.random.default_rng(seed)
    cam = _camera(name)
    centres = np.asarray(centres, dtype=np.float32)
    c = centres[rng.integers(0, len(centres), size=n)]
    target = c + rng.uniform([-reach, -reach, 0], [reach, reach, 1.6], size=(n, 3)).astype(np.float32)
    origin = c + rng.uniform([-4, -4, 0.1], [4, 4, 4], size=(n, 3)).astype(np.float32)
    o = (origin - cam).astype(np.float32)
    d = (target - origin).astype(np.float32)
    return o, d, np.full(n, 2.0, dtype=np.float32)


def test_timed_trace_entry_points_walk_nested_placements(wfpt, tmp_path):
    """wf_trace_closest_host_t / wf_trace_any_host_t on animated_in_definition_general (sphere, alpha-tested mesh, cylinder + patch moving
    inside a definition used statically, mirrored and animated): bit-identical with the CPU build of the same walk, whose render of the scene
    is pinned to the reference's; at least 200 of the CPU checker's own hits name a nested placement"""
    name = "animated_in_definition_general"
    path = os.path.join(GOLDEN, name + ".pbrt")
    s = _open(wfpt, name)
    n = 20000
    o, d, tmax = _aimed_rays(name, n, 21, [(-2.6, 0.5, 0.1), (0, 1.5, 0.1), (2.6, -0.2, 0.4)], 1.1)
    time = np.random.default_rng(6).uniform(0, 1, size=n).astype(np.float32)
    with pytest.raises(wfpt.WfError, match="animated"):
        s.trace_closest(o, d, tmax)
    with pytest.raises(wfpt.WfError, match="animated"):
        s.trace_any(o, d, tmax, reference_order=False)
    got = s.trace_timed(o, d, tmax, time)
    occ = s.trace_timed(o, d, tmax, time, any_hit=True)
    at0 = s.trace_timed(o, d, tmax, np.zeros(n, dtype=np.float32))
    rays = np.concatenate([o, d, tmax[:, None], time[:, None]], axis=1).astype(np.float32)
    rays.tofile(tmp_path / "rays8.bin")
    subprocess.run([WF_CPU, "--quiet", "--trace-timed", str(tmp_path / "rays8.bin"), str(tmp_path / "hits.bin"), path], check=True)
    ref = np.fromfile(tmp_path / "hits.bin", dtype=got.dtype)
    nested = _nested_mask(s, name, ref["instance"])
    s.close()
    print("hits %d, inside the definition %d, inside nested placements %d" % ((ref["prim"] >= 0).sum(), (ref["instance"] >= 0).sum(), nested.sum()))
    assert 0.1 < (ref["prim"] >= 0).mean() < 1.0
    assert nested.sum() >= 200
    for f in ("prim", "instance"):
        assert (got[f] == ref[f]).all(), f
    for f in ("t", "b0", "b1", "b2"):
        assert (got[f].view(np.uint32) == ref[f].view(np.uint32)).all(), f
    assert ((occ != 0) == (ref["prim"] >= 0)).all()
    # the time matters: the same rays at time 0 meet the moving primitives elsewhere
    assert ((at0["prim"] != got["prim"]) | (at0["t"] != got["t"])).mean() > 0.005


def _shadow_rays(o, d, seed, n_media):
    n = len(o)
    rng = np.random.RandomState(seed)
    tmax = np.full(n, 0.9999, dtype=np.float32)
    medium = rng.randint(-1, n_media, size=n).astype(np.int32)
    lam = np.sort(rng.uniform(380, 780, size=(n, 4)), axis=1).astype(np.float32)
    Ld = rng.uniform(0.1, 2, size=(n, 4)).astype(np.float32)
    ones = np.ones((n, 4), dtype=np.float32)
    return o, d, tmax, medium, lam, Ld, ones, ones.copy()


def test_shadow_tr_host_t_walks_a_nested_moving_interface(wfpt):
    """wf_trace_shadow_tr_host_t on animated_in_definition_media (a moving `interface` shell around a medium inside the definition): the
    untimed call is refused, the results are finite, and time 0 and time 1 give different transmittances (its arithmetic is pinned by the
    image parity above: the render's shadow rays take this walk)"""
    name = "animated_in_definition_media"
    s = _open(wfpt, name)
    lo, hi = s.bounds()
    n = 20000
    rng = np.random.RandomState(4)
    o = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = (rng.uniform(lo, hi, size=(n, 3)).astype(np.float32) - o).astype(np.float32)
    rays = _shadow_rays(o, d, 4, 1)
    with pytest.raises(wfpt.WfError, match="animated"):
        s.trace_shadow_tr(*rays)
    at0 = s.trace_shadow_tr(*rays, time=np.zeros(n, dtype=np.float32))
    at1 = s.trace_shadow_tr(*rays, time=np.ones(n, dtype=np.float32))
    s.close()
    assert np.isfinite(at0).all() and np.isfinite(at1).all()
    print("shadow rays whose radiance differs between time 0 and time 1: %.2f %%" % (100 * (at0 != at1).any(axis=1).mean()))
    assert (at0 != at1).any(axis=1).mean() > 0.01


def test_one_random_host_t_walks_a_nested_moving_subsurface_block(wfpt):
    """wf_trace_one_random_host_t on animated_in_definition_sss: the untimed call is refused, the records are finite, time 0 and time 1
    differ, and some records name a nested placement (the moving block inside the definition)"""
    name = "animated_in_definition_sss"
    s = _open(wfpt, name)
    lo, hi = s.bounds()
    n = 20000
    rng = np.random.RandomState(12)
    p0 = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    p1 = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    with pytest.raises(wfpt.WfError, match="animated"):
        s.trace_one_random(p0, p1, np.zeros(n, dtype=np.int32))
    differ, nested = 0.0, 0
    for m in range(16):
        mat = np.full(n, m, dtype=np.int32)
        r0, pdf0 = s.trace_one_random(p0, p1, mat, time=np.zeros(n, dtype=np.float32))
        r1, pdf1 = s.trace_one_random(p0, p1, mat, time=np.ones(n, dtype=np.float32))
        assert np.isfinite(pdf0).all() and np.isfinite(pdf1).all()
        for r, pdf in ((r0, pdf0), (r1, pdf1)):
            hit = pdf > 0
            assert (r["prim"][~hit] == -1).all() and (r["prim"][hit] >= 0).all()
            assert all(np.isfinite(r[f][hit]).all() for f in ("t", "b0", "b1", "b2"))
            nested += int(_nested_mask(s, name, r["instance"][hit]).sum())
        differ = max(differ, float(((r0["prim"] != r1["prim"]) | (r0["t"] != r1["t"])).mean()))
    s.close()
    print("probe segments that end elsewhere at time 1 (best material): %.2f %%; records naming a nested placement: %d" % (100 * differ, nested))
    assert differ > 0.01
    assert nested > 0


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_product_binary_renders_the_golden(tmp_path, devices):
    """pbrt_amd --spp 4 on animated_in_definition.pbrt: the reference's image bit for bit, from one context and from two contexts on one device"""
    exe = os.path.join(ROOT, "pbrt-v4_amd", "_build", "pbrt_amd")
    out = str(tmp_path / "out.pfm")
    cmd = [exe, "--quiet", "--spp", "4"] + (["--gpu-devices", devices] if devices else []) + ["--outfile", out, os.path.join(GOLDEN, "animated_in_definition.pbrt")]
    subprocess.run(cmd, check=True, timeout=600)
    img, ref = read_pfm(out), read_pfm(os.path.join(GOLDEN, "animated_in_definition_ref.pfm"))
    assert img.shape == ref.shape and (img.view(np.uint32) == ref.view(np.uint32)).all()
