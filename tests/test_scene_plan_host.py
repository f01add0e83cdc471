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


# ---- the stage kernels' variants: "shade_variant_<t>", "route_variant", "camera_anim" (ScenePlan::shadeVariant, routeVariant, cameraAnim) ----
# Each expected value is worked out here with the rule the launch site applied while the choice was still made there (EvalMaterial's `v`,
# the three-way choice around "Route hits", the `?:` of "Generate camera rays"), from facts read off the scene file — not read back from
# the plan.  The variants of a material kernel agree bit for bit (every one of them is rendered and compared on the device by
# tests/test_material_matrix_gpu.py), so a wrong rule would be a slowdown no parity test sees.
DIFFUSE, CONDUCTOR, DIELECTRIC, THIN_DIELECTRIC, DIFFUSE_TRANSMISSION, COATED_DIFFUSE, COATED_CONDUCTOR = range(1, 8)   # wf_material_type


def _shade_rule(gbuffer, moving_camera, animated, alpha_curves, lean, footprint):
    """EvalMaterial: 3 the visible-surface variant (any of its four conditions), else 2 general, else the lean kernel with (1) or without (0) the texture footprint"""
    if gbuffer or moving_camera or animated or alpha_curves:
        return 3
    return 2 if not lean else (1 if footprint else 0)


def _route_rule(animated, general, instanced):
    """wf_intersect_closest: k_route_hits<true, true> for animated primitives, <true> for general primitives (genMode > 1) or instances, else <false>"""
    return 2 if animated else (1 if general or instanced else 0)


# scene -> the material types it uses, which condition of the visible-surface variant it meets (if any), whether a texture needs a
# footprint (an image map, a displacement), and the types that are lean under the default switches: none of their materials on a shape
# that is not a triangle, every texture of the scene a constant, an image map or a bilerp, nothing animated
SHADE_SCENES = {
    # triangles, constant reflectances only
    "cornell64": dict(types=[DIFFUSE], lean=[DIFFUSE]),
    # triangles; image-map reflectance / roughness and image-map displacement
    "image_textures": dict(types=[DIFFUSE, CONDUCTOR], lean=[DIFFUSE, CONDUCTOR], footprint=True),
    # disks and cylinders only
    "quadrics": dict(types=[DIFFUSE, CONDUCTOR, DIELECTRIC], lean=[]),
    # Film "gbuffer" (its "scale" / "mix" textures would make it general otherwise)
    "gbuffer_film": dict(types=[DIFFUSE, CONDUCTOR, DIELECTRIC, THIN_DIELECTRIC, DIFFUSE_TRANSMISSION, COATED_DIFFUSE, COATED_CONDUCTOR], lean=[], gbuffer=True),
    # image_textures under a camera with two transformations (ActiveTransform StartTime / EndTime before Camera)
    "camera_motion": dict(types=[DIFFUSE, CONDUCTOR], lean=[DIFFUSE, CONDUCTOR], footprint=True, moving_camera=True),
    # triangle meshes under two transformations
    "animated_tris": dict(types=[DIFFUSE, CONDUCTOR, COATED_DIFFUSE], lean=[], animated=True),
    # curves, some with "texture alpha" / "float alpha"
    "curves_alpha": dict(types=[DIFFUSE, DIELECTRIC, COATED_DIFFUSE], lean=[], alpha_curves=True),
    # WF_LEAN_PER_TYPE, a lean type beside general ones (instances_quadrics does not qualify: its checkerboard texture makes every type
    # general): diffuse on triangle meshes only, coated diffuse and conductor on spheres; constant textures
    "portal_light": dict(types=[DIFFUSE, CONDUCTOR, COATED_DIFFUSE], lean=[DIFFUSE]),
    # ... and with a footprint: coated diffuse (with a normal map) on triangles only, diffuse on a bilinear patch and a sphere too, conductor on a sphere; image maps
    "png_textures": dict(types=[DIFFUSE, CONDUCTOR, COATED_DIFFUSE], lean=[COATED_DIFFUSE], footprint=True),
}
# what the rule comes to, scene by scene (the scenes not named: 3 for every type, each by a different one of the four conditions)
SHADE_EXPECTED = {"cornell64": {DIFFUSE: 0}, "image_textures": {DIFFUSE: 1, CONDUCTOR: 1}, "quadrics": {DIFFUSE: 2, CONDUCTOR: 2, DIELECTRIC: 2},
                  "portal_light": {DIFFUSE: 0, CONDUCTOR: 2, COATED_DIFFUSE: 2}, "png_textures": {DIFFUSE: 2, CONDUCTOR: 2, COATED_DIFFUSE: 1}}
VISIBLE_SURFACE = ["gbuffer_film", "camera_motion", "animated_tris", "curves_alpha"]


def _check_shade_variants(wfpt, name, lean_types):
    f = SHADE_SCENES[name]
    types = f["types"]
    p = plan(wfpt, name, ["lean_type_%d" % t for t in types] + ["shade_variant_%d" % t for t in types])
    # the scene is in the class it is listed for (the lean types are the plan's older keys, pinned before this one existed)
    lean = {t: int(t in lean_types) for t in types}
    assert {t: p["lean_type_%d" % t] for t in types} == lean, p
    want = {t: _shade_rule(f.get("gbuffer", False), f.get("moving_camera", False), f.get("animated", False), f.get("alpha_curves", False), lean[t], f.get("footprint", False))
            for t in types}
    assert {t: p["shade_variant_%d" % t] for t in types} == want, p
    return want


@pytest.mark.parametrize("name", sorted(SHADE_SCENES))
def test_shade_variant_follows_the_launch_site_rule(wfpt, name):
    want = _check_shade_variants(wfpt, name, SHADE_SCENES[name]["lean"])
    assert want == SHADE_EXPECTED.get(name, {t: 3 for t in SHADE_SCENES[name]["types"]}), want
    assert (name in VISIBLE_SURFACE) == (name not in SHADE_EXPECTED)


@pytest.mark.parametrize("name", sorted(SHADE_SCENES))
def test_shade_variant_without_the_lean_kernels(wfpt, monkeypatch, name):
    monkeypatch.setenv("WF_LEAN_SHADE", "0")
    want = _check_shade_variants(wfpt, name, [])
    assert set(want.values()) == {3 if name in VISIBLE_SURFACE else 2}, want


@pytest.mark.parametrize("name", ["portal_light", "png_textures"])
def test_shade_variant_without_the_per_type_lean_kernels(wfpt, monkeypatch, name):
    monkeypatch.setenv("WF_LEAN_PER_TYPE", "0")
    assert set(_check_shade_variants(wfpt, name, []).values()) == {2}


@pytest.mark.parametrize("name", sorted(SHADE_SCENES))
def test_visible_surface_switch_forces_variant_3_and_only_on(wfpt, monkeypatch, name):
    """WF_VISIBLE_SURFACE=1: every type takes the superset kernel, whatever the scene (the lean classification itself is untouched);
    =0 is "unset": a scene that needs variant 3 keeps it, every other scene its own plan"""
    types = SHADE_SCENES[name]["types"]
    keys = ["lean_type_%d" % t for t in types] + ["rare_lights"]
    before = plan(wfpt, name, keys)
    monkeypatch.setenv("WF_VISIBLE_SURFACE", "1")
    assert plan(wfpt, name, ["shade_variant_%d" % t for t in range(1, 11)]) == {"shade_variant_%d" % t: 3 for t in range(1, 11)}
    assert plan(wfpt, name, keys) == before
    monkeypatch.setenv("WF_VISIBLE_SURFACE", "0")
    want = _check_shade_variants(wfpt, name, SHADE_SCENES[name]["lean"])
    assert want == SHADE_EXPECTED.get(name, {t: 3 for t in types}), want


# cornell64: one triangle emitter; portal_light: a portal infinite light; bilinear_lights: emissive bilinear patches; arealight_alpha:
# alpha-masked triangle emitters — the last three are RARE by themselves
@pytest.mark.parametrize("name,rare,portal", [("cornell64", 0, 0), ("image_textures", 0, 0), ("portal_light", 1, 1), ("bilinear_lights", 1, 0), ("arealight_alpha", 1, 0)])
def test_rare_lights_switch_forces_the_rare_kernels_and_only_on(wfpt, monkeypatch, name, rare, portal):
    """WF_RARE_LIGHTS=1: k_mat_nee<t, true>, k_medium_scatter<true> ("rare_lights") and k_handle_escaped<true> ("portal_lights") whatever the scene's lights;
    =0 is "unset": a scene with such lights keeps them.  The shade variants do not depend on it."""
    keys = ["shade_variant_%d" % t for t in range(1, 11)]
    before = plan(wfpt, name, keys)
    assert plan(wfpt, name, ["rare_lights", "portal_lights"]) == {"rare_lights": rare, "portal_lights": portal}
    monkeypatch.setenv("WF_RARE_LIGHTS", "1")
    assert plan(wfpt, name, ["rare_lights", "portal_lights"]) == {"rare_lights": 1, "portal_lights": 1}
    assert plan(wfpt, name, keys) == before
    monkeypatch.setenv("WF_RARE_LIGHTS", "0")
    assert plan(wfpt, name, ["rare_lights", "portal_lights"]) == {"rare_lights": rare, "portal_lights": portal}


# cornell64: triangles only, no ObjectInstance; media_instances: plain triangle meshes under ObjectInstance; quadrics: disks and cylinders
# (gen_mode 2), no instances; instances: ObjectInstance and a checkerboard alpha cut-out (a texture graph: gen_mode 2) — both conditions
# of <true> at once; animated_tris: moving meshes (each an instance)
@pytest.mark.parametrize("name,animated,general,instanced,variant", [("cornell64", False, False, False, 0), ("media_instances", False, False, True, 1), ("quadrics", False, True, False, 1),
                                                                      ("instances", False, True, True, 1), ("animated_tris", True, False, True, 2)])
def test_route_variant_follows_the_launch_site_rule(wfpt, name, animated, general, instanced, variant):
    p = plan(wfpt, name, ["gen_mode", "instances", "anim_fast", "route_variant"])
    assert (p["gen_mode"] > 1, p["instances"] > 0) == (general, instanced), p
    assert p["route_variant"] == _route_rule(animated, general, instanced) == variant, p
    assert p["anim_fast"] == animated


def test_camera_anim(wfpt):
    """camera_motion: ActiveTransform StartTime / EndTime give the camera two transformations; cornell64: one LookAt"""
    assert plan(wfpt, "camera_motion", ["camera_anim"]) == {"camera_anim": 1}
    assert plan(wfpt, "cornell64", ["camera_anim"]) == {"camera_anim": 0}


@pytest.mark.parametrize("key", ["shade_variant_", "shade_variant_x", "shade_variant_1x", "shade_variant_-1", "shade_variant_11", "lean_type_", "lean_type_x"])
def test_a_type_key_needs_a_type_in_digits(wfpt, key):
    """(a key without a number used to answer for type 0)"""
    with pytest.raises(wfpt.WfError, match="unknown key"):
        plan(wfpt, "cornell64", [key])
