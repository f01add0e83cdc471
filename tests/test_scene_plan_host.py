"""Which kernel variants a scene gets, asked on the HOST (no GPU): Scene.plan -> wf_scene_plan_query (include/wf_abi.h) runs the planning
step of wf_scene_upload — every check of the description, the classification, the production trees — without a context or a device.
The expected values are the ones the GPU suite asserts through wf_ctx_query on the uploaded scenes (test_variant_selection_queries,
test_lean_medium_kernels_selected_and_bit_identical, test_animated_primitives_on_the_production_walk,
test_triangle_scenes_take_the_production_walk, test_animated_in_definition_gpu.py); test_variant_selection_queries checks on the device
that the two entry points agree."""
import ctypes
import os

import pytest

from conftest import GOLDEN

# per scene, from the scene files: uses of its one definition (ObjectInstance), moving entities inside it (tests/test_animated_in_definition_gpu.py)
NESTED_LAYOUT = {"animated_in_definition": (3, 2), "animated_in_definition_general": (3, 4), "animated_in_definition_media": (2, 1), "animated_in_definition_sss": (2, 1)}


def plan(wfpt, name, keys):
    s = wfpt.Scene(path=os.path.join(GOLDEN, name + ".pbrt"), spp=4)
    try:
        return {k: s.plan(k) for k in keys}
    finally:
        s.close()


def test_triangle_scene_takes_the_lean_production_kernels(wfpt):
    assert plan(wfpt, "cornell64", ["fast_ok", "gen_mode", "lean_shade", "defer_general"]) == {"fast_ok": 1, "gen_mode": 0, "lean_shade": 1, "defer_general": 0}


def test_two_class_traversal_follows_its_switch(wfpt, monkeypatch):
    monkeypatch.setenv("WF_DEFER_GENERAL", "1")
    r = plan(wfpt, "instances_quadrics", ["fast_ok", "gen_mode", "defer_general", "instances"])
    assert r["fast_ok"] == 1 and r["gen_mode"] >= 2 and r["defer_general"] == 1 and r["instances"] > 0, r
    monkeypatch.setenv("WF_DEFER_GENERAL", "0")
    assert plan(wfpt, "instances_quadrics", ["defer_general"]) == {"defer_general": 0}


def test_anim_fast_switch_sends_an_animated_scene_to_the_reference_order_walks(wfpt, monkeypatch):
    monkeypatch.setenv("WF_ANIM_FAST", "0")
    assert plan(wfpt, "animated_sss", ["fast_ok", "anim_fast"]) == {"fast_ok": 0, "anim_fast": 0}


@pytest.mark.parametrize("name,lean", [("media_box", 1), ("media_instances", 1), ("cloud_medium", 0), ("rgbgrid_medium", 0), ("tempgrid_medium", 0)])
def test_lean_medium_kernels(wfpt, monkeypatch, name, lean):
    assert plan(wfpt, name, ["medium_lean"]) == {"medium_lean": lean}
    if lean:
        monkeypatch.setenv("WF_MEDIUM_LEAN", "0")
        assert plan(wfpt, name, ["medium_lean"]) == {"medium_lean": 0}


@pytest.mark.parametrize("name", ["animated_tris", "animated_tris_alpha", "animated_interface", "animated_mix", "animated_subsurface"])
def test_animated_triangle_scenes_take_the_production_walk(wfpt, name):
    assert plan(wfpt, name, ["anim_fast", "fast_ok"]) == {"anim_fast": 1, "fast_ok": 1}


@pytest.mark.parametrize("name", ["animated", "animated_sss"])
def test_animated_scenes_with_quadrics_keep_the_reference_order_walks(wfpt, name):
    r = plan(wfpt, name, ["anim_fast", "fast_ok"])
    assert not (r["anim_fast"] == 1 and r["fast_ok"] == 1), r


def test_animated_sphere_keeps_the_reference_order_walks(wfpt):
    assert plan(wfpt, "animated_interface_sphere", ["anim_fast"]) == {"anim_fast": 0}


@pytest.mark.parametrize("name", sorted(NESTED_LAYOUT))
def test_nested_placements_are_counted_and_keep_the_reference_order_walks(wfpt, name):
    uses, entities = NESTED_LAYOUT[name]
    assert plan(wfpt, name, ["nested_animated", "instances", "fast_ok"]) == {"nested_animated": uses * entities, "instances": uses * (1 + entities), "fast_ok": 0}


def test_unknown_key_is_an_error(wfpt):
    with pytest.raises(wfpt.WfError, match="unknown key"):
        plan(wfpt, "cornell64", ["frame_overlap_active"])   # (a key of the context, not of the plan)


def test_rejected_description_fails_in_the_planning_step(wfpt):
    """abi_version is the first int32 of wf_scene_desc: a description the upload would reject is rejected by the step that owns no
    device memory, with the upload's message"""
    host, _ = wfpt.libs()
    s = wfpt.Scene(path=os.path.join(GOLDEN, "cornell64.pbrt"), spp=4)
    try:
        word = ctypes.c_int32.from_address(host.wfh_scene_desc(s.h))
        good = word.value
        word.value = good + 1
        try:
            with pytest.raises(wfpt.WfError, match="ABI version mismatch"):
                s.plan("fast_ok")
        finally:
            word.value = good
        assert s.plan("fast_ok") == 1
    finally:
        s.close()
