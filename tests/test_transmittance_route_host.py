"""Which route a scene's transmittance stage takes (ScenePlan::trRoute), asked on the HOST (no GPU) through Scene.plan("tr_route") ->
wf_scene_plan_query: -1 the scene has no media, 0 the reference-order walk per lane (k_shadow_tr), 1 the per-lane production walk
(k_shadow_tr_fast), 2 the transmittance wavefront (k_tr_begin / k_tr_trace / k_tr_segment / k_tr_rest).  Scenes whose animated primitives
the production walks' ANIM variants carry (anim_fast) take the wavefront under the rule of the static scenes; the render's stage and
wf_trace_shadow_tr_device both read the plan.  Also the golden of the scene written for those variants, on the CPU checker."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, read_pfm, run_wf_cpu

STATIC_MEDIA = ["media_box", "media_instances", "media_preset", "cloud_medium", "rgbgrid_medium", "tempgrid_medium"]
ANIM_FAST_MEDIA = ["animated_interface", "animated_tr_routes"]


def plan(wfpt, name, keys):
    s = wfpt.Scene(path=os.path.join(GOLDEN, name + ".pbrt"), spp=4)
    try:
        return {k: s.plan(k) for k in keys}
    finally:
        s.close()


def route(wfpt, name):
    return plan(wfpt, name, ["tr_route"])["tr_route"]


@pytest.mark.parametrize("name", ANIM_FAST_MEDIA)
def test_anim_fast_scenes_with_media_take_the_wavefront(wfpt, monkeypatch, name):
    monkeypatch.delenv("WF_TR_WAVEFRONT", raising=False)
    assert route(wfpt, name) == 2
    monkeypatch.setenv("WF_TR_WAVEFRONT", "1")
    assert route(wfpt, name) == 2
    # the switch takes it off: there is no per-lane production ANIM kernel, so the reference-order walk
    monkeypatch.setenv("WF_TR_WAVEFRONT", "0")
    assert route(wfpt, name) == 0


@pytest.mark.parametrize("name", ANIM_FAST_MEDIA)
def test_without_the_anim_walks_the_reference_order_walk_answers(wfpt, monkeypatch, name):
    monkeypatch.delenv("WF_TR_WAVEFRONT", raising=False)
    monkeypatch.setenv("WF_ANIM_FAST", "0")
    assert plan(wfpt, name, ["anim_fast", "fast_ok", "tr_route"]) == {"anim_fast": 0, "fast_ok": 0, "tr_route": 0}
    monkeypatch.setenv("WF_TR_WAVEFRONT", "1")
    assert route(wfpt, name) == 0


def test_nested_placements_keep_the_reference_order_walk(wfpt, monkeypatch):
    monkeypatch.delenv("WF_TR_WAVEFRONT", raising=False)
    assert plan(wfpt, "animated_in_definition_media", ["fast_ok", "tr_route"]) == {"fast_ok": 0, "tr_route": 0}
    monkeypatch.setenv("WF_TR_WAVEFRONT", "1")
    assert route(wfpt, "animated_in_definition_media") == 0


def test_scene_without_media_has_no_route(wfpt, monkeypatch):
    for sw in (None, "1", "0"):
        if sw is None:
            monkeypatch.delenv("WF_TR_WAVEFRONT", raising=False)
        else:
            monkeypatch.setenv("WF_TR_WAVEFRONT", sw)
        assert route(wfpt, "cornell64") == -1


def _static_rule(p, sw):
    """the rule of wf_intersect_shadow_tr before the route moved into the plan, from the plan's other keys (sw: the switch, -1 = unset)"""
    if p["fast_ok"] and p["gen_mode"] <= 1 and (sw == 1 or (sw < 0 and (p["instances"] > 0 or p["medium_lean"]))):
        return 2
    if p["fast_ok"] and p["instances"] == 0:
        return 1
    return 0


@pytest.mark.parametrize("name", STATIC_MEDIA)
def test_static_media_scenes_keep_their_routes(wfpt, monkeypatch, name):
    seen = {}
    for sw in (-1, 1, 0):
        if sw < 0:
            monkeypatch.delenv("WF_TR_WAVEFRONT", raising=False)
        else:
            monkeypatch.setenv("WF_TR_WAVEFRONT", str(sw))
        p = plan(wfpt, name, ["fast_ok", "gen_mode", "instances", "medium_lean", "anim_fast", "tr_route"])
        assert p["anim_fast"] == 0
        assert p["tr_route"] == _static_rule(p, sw), (sw, p)
        seen[sw] = p["tr_route"]
    # the switch takes the wavefront off everywhere, and the scenes with lean media or object instances have it by default
    assert seen[0] != 2
    if name in ("media_box", "media_instances", "media_preset"):
        assert seen[-1] == 2 and seen[1] == 2, seen


def test_the_routes_scene_asks_for_the_variants_it_was_written_for(wfpt, monkeypatch):
    monkeypatch.delenv("WF_TR_WAVEFRONT", raising=False)
    p = plan(wfpt, "animated_tr_routes", ["anim_fast", "fast_ok", "gen_mode", "medium_lean", "instances", "nested_animated", "tr_route"])
    assert p["anim_fast"] == 1 and p["fast_ok"] == 1 and p["gen_mode"] == 1 and p["medium_lean"] == 0 and p["nested_animated"] == 0, p
    assert p["instances"] > 0 and p["tr_route"] == 2, p
    # ... and animated_interface for the others: GEN 0, lean media
    q = plan(wfpt, "animated_interface", ["anim_fast", "gen_mode", "medium_lean"])
    assert q == {"anim_fast": 1, "gen_mode": 0, "medium_lean": 1}


def test_cpu_checker_renders_the_routes_scene_like_the_reference(built, tmp_path):
    """oracle/wf_cpu against pbrt_ref --wavefront (tests/golden/animated_tr_routes_ref.pfm): bit-identical"""
    ref = read_pfm(os.path.join(GOLDEN, "animated_tr_routes_ref.pfm"))
    out = str(tmp_path / "cpu.pfm")
    j = run_wf_cpu(os.path.join(GOLDEN, "animated_tr_routes.pbrt"), out, 4)
    img = read_pfm(out)
    assert img.shape == ref.shape == (64, 96, 3)
    assert j["camera_rays"] == 4 * img.shape[0] * img.shape[1]
    assert np.isfinite(img).all() and img.mean() > 0.01
    assert (img.view(np.uint32) == ref.view(np.uint32)).all(), "fraction identical: %f" % (img == ref).mean()
