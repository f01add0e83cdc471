"""Interface, mix and subsurface materials on AnimatedPrimitives on the MI355X, and the timed boundary entry points of the transmittance
walk and the subsurface probe (wf_trace_shadow_tr_host_t, wf_trace_one_random_host_t)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from suite_helpers import _check_image_vs_oracle_and_reference

pytestmark = pytest.mark.gpu

SCENES = ["animated_interface", "animated_interface_sphere", "animated_mix", "animated_subsurface", "animated_light"]


def _query(wfpt, name, keys):
    s = wfpt.Scene(path=os.path.join(GOLDEN, name + ".pbrt"), spp=4)
    s.create_renderer(0)
    r = {k: s.query(k) for k in keys}
    s.close()
    return r


@pytest.mark.parametrize("name", SCENES)
def test_animated_materials_render_like_the_reference_on_both_walks(wfpt, tmp_path, monkeypatch, name):
    """bit-identical with wf_cpu and with pbrt_ref --wavefront, equal ray counts: on the default walk (the production walk's ANIM variants
    for the triangle-only scenes: k_route_hits<true, true>, k_resolve_mix<true>, k_medium_route<true>) and with WF_ANIM_FAST=0 (the
    reference-order walks: KAfterClosestHit<true>)"""
    _check_image_vs_oracle_and_reference(wfpt, tmp_path, name)
    monkeypatch.setenv("WF_ANIM_FAST", "0")
    assert _query(wfpt, name, ["anim_fast"])["anim_fast"] == 0
    _check_image_vs_oracle_and_reference(wfpt, tmp_path, name)


def test_triangle_scenes_take_the_production_walk(wfpt):
    """the ANIM routing of the production walk is what animated_interface / animated_mix / animated_subsurface cover"""
    for name in ("animated_interface", "animated_mix", "animated_subsurface"):
        assert _query(wfpt, name, ["anim_fast", "fast_ok"]) == {"anim_fast": 1, "fast_ok": 1}, name
    assert _query(wfpt, "animated_interface_sphere", ["anim_fast"]) == {"anim_fast": 0}


def _shadow_rays(lo, hi, n, seed, n_media):
    rng = np.random.RandomState(seed)
    o = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    to = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = (to - o).astype(np.float32)
    tmax = np.full(n, 0.9999, dtype=np.float32)
    medium = rng.randint(-1, n_media, size=n).astype(np.int32)
    lam = np.sort(rng.uniform(380, 780, size=(n, 4)), axis=1).astype(np.float32)
    Ld = rng.uniform(0.1, 2, size=(n, 4)).astype(np.float32)
    ones = np.ones((n, 4), dtype=np.float32)
    return o, d, tmax, medium, lam, Ld, ones, ones.copy()


def test_shadow_tr_host_t_at_time_zero_is_the_untimed_call_on_a_static_scene(wfpt):
    s = wfpt.Scene(path=os.path.join(GOLDEN, "media_box.pbrt"), spp=4)
    s.create_renderer(0)
    lo, hi = s.bounds()
    n = 20000
    rays = _shadow_rays(lo, hi, n, 3, 2)
    untimed = s.trace_shadow_tr(*rays)
    timed = s.trace_shadow_tr(*rays, time=np.zeros(n, dtype=np.float32))
    s.close()
    assert np.isfinite(untimed).all() and (untimed > 0).any(axis=1).mean() > 0.1 and (untimed == 0).all(axis=1).mean() > 0.05
    assert (timed.view(np.uint32) == untimed.view(np.uint32)).all()


def test_shadow_tr_host_t_takes_ray_times_on_an_animated_scene(wfpt):
    s = wfpt.Scene(path=os.path.join(GOLDEN, "animated_interface.pbrt"), spp=4)
    s.create_renderer(0)
    lo, hi = s.bounds()
    n = 20000
    rays = _shadow_rays(lo, hi, n, 4, 2)
    with pytest.raises(wfpt.WfError, match="animated"):
        s.trace_shadow_tr(*rays)
    at0 = s.trace_shadow_tr(*rays, time=np.zeros(n, dtype=np.float32))
    at1 = s.trace_shadow_tr(*rays, time=np.ones(n, dtype=np.float32))
    s.close()
    assert np.isfinite(at0).all() and np.isfinite(at1).all()
    assert (at0 != at1).any(axis=1).mean() > 0.01   # the moving media boundaries and the moving metal wedge are elsewhere at time 1


def test_one_random_host_t_matches_the_timed_closest_hit_on_a_moving_surface(wfpt):
    """Vertical probe segments from above the scene down to the middle height of animated_subsurface's moving block AT THE SEGMENT'S TIME:
    the block's top face is the only surface on such a segment, so wherever the block lies under it the reservoir holds that one hit
    (pdf 1) and it is the closest hit of the probe's first ray — SpawnRayTo(p0, p1) from an interaction with a zero normal: origin p0,
    direction p1 - p0, tMax 1 — walked at the same time (wf_trace_closest_host_t)."""
    s = wfpt.Scene(path=os.path.join(GOLDEN, "animated_subsurface.pbrt"), spp=4)
    s.create_renderer(0)
    n = 4000
    rng = np.random.RandomState(9)
    time = rng.uniform(0, 1, size=n).astype(np.float32)
    xy = rng.uniform([-1.9, -1.0], [1.1, 1.0], size=(n, 2)).astype(np.float32)
    # (in world space; the segments are given in rendering space, "cameraworld" by default: the world translated by minus the camera's
    #  position, LookAt 0 -6 3.5)
    camera = np.array([0, -6, 3.5], dtype=np.float32)
    p0 = (np.concatenate([xy, np.full((n, 1), 3.5, np.float32)], axis=1) - camera).astype(np.float32)
    # the block spans z = 1.2 + 0.5 t .. 1.8 + 0.5 t at time t (its translation is interpolated linearly; the rotation is about z)
    p1 = (np.concatenate([xy, (1.5 + 0.5 * time)[:, None]], axis=1) - camera).astype(np.float32)
    with pytest.raises(wfpt.WfError, match="animated"):
        s.trace_one_random(p0, p1, np.zeros(n, dtype=np.int32))
    # the block's material id: the one material these segments meet
    found = {}
    for m in range(16):
        rec, pdf = s.trace_one_random(p0, p1, np.full(n, m, dtype=np.int32), time=time)
        if (pdf > 0).any():
            found[m] = (rec, pdf)
    assert len(found) == 1, sorted(found)
    (m, (rec, pdf)), = found.items()
    mat = np.full(n, m, dtype=np.int32)
    hit = pdf > 0
    assert 0.05 < hit.mean() < 0.9
    assert (pdf[hit] == 1).all() and (rec["prim"][~hit] == -1).all()
    d = (p1 - p0).astype(np.float32)
    ref = s.trace_timed(p0, d, np.ones(n, dtype=np.float32), time)
    assert (ref["prim"] >= 0).tolist() == hit.tolist()
    for f in ("prim", "instance"):
        assert (rec[f][hit] == ref[f][hit]).all(), f
    for f in ("t", "b0", "b1", "b2"):
        assert (rec[f][hit].view(np.uint32) == ref[f][hit].view(np.uint32)).all(), f
    # the segments' time matters: at time 0 and at time 1 the block lies under different segments
    r0, p_0 = s.trace_one_random(p0, p1, mat, time=np.zeros(n, dtype=np.float32))
    r1, p_1 = s.trace_one_random(p0, p1, mat, time=np.ones(n, dtype=np.float32))
    s.close()
    assert ((p_0 > 0) != (p_1 > 0)).mean() > 0.05
    assert ((r0["prim"] != r1["prim"]) | (r0["t"] != r1["t"])).mean() > 0.05
