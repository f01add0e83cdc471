"""The case table of the material-kernel matrix: which (scene, environment) runs which of the 60 separately compiled material kernels —
k_mat_shade<type, variant> (ten types x variants 0 lean, 1 lean + footprint, 2 general, 3 general + visible surface) and
k_mat_nee<type, rare> (ten types x two).  tests/test_variant_census_host.py checks the table against the planner on the host (and that
it covers every cell); tests/test_material_matrix_gpu.py renders every case on the device.

A case CLAIMS cells only for material types whose queues hold items in that scene (the census checks this with the CPU port's item
counts): `shade` maps each such type to the shade variant the case plans for it, `rare` is the NEE kernels' template argument.  The
values are written down from the scene files and the planner's rule (wf_plan.cpp ClassifyScene: 3 if the scene — or
WF_VISIBLE_SURFACE=1 — asks for the visible surface, else 2 for a type that is not lean, else 1 / 0 with / without a texture footprint;
a type is lean when WF_LEAN_SHADE is not 0, every texture of the scene is a constant, an image map or a bilerp, nothing is animated and
none of the type's materials sits on a shape that is not a triangle — with WF_LEAN_PER_TYPE=0: no such shape in the whole scene), not
read back from the plan."""
from collections import namedtuple

DIFFUSE, CONDUCTOR, DIELECTRIC, THIN_DIELECTRIC, DIFFUSE_TRANSMISSION, COATED_DIFFUSE, COATED_CONDUCTOR, SUBSURFACE, HAIR, MEASURED = range(1, 11)   # wf_material_type
TYPES = tuple(range(1, 11))     # the types with a queue and kernels of their own (0, the interface, has none)
SHADE_CELLS = {(t, v) for t in TYPES for v in range(4)}     # kMatShade[type][variant]
NEE_CELLS = {(t, r) for t in TYPES for r in range(2)}       # kMatNee[type][rare]

# The item floor of the two matrix scenes, per type over the render: two full 256-thread workgroups, so every queue spans several blocks
ITEM_FLOOR = 512
BLOCK = 256

Case = namedtuple("Case", "id scene env shade rare")


def _case(scene, env, shade, rare):
    tag = ",".join("%s=%s" % (k[3:].lower(), v) for k, v in sorted(env.items())) or "default"
    return Case("%s-%s" % (scene, tag), scene, dict(env), dict(shade), int(rare))


def _all(variant, types=TYPES):
    return {t: variant for t in types}


CASES = []

# ---- the two matrix scenes: all ten types on triangle quads, one triangle emitter and a point light (RARE = false by themselves).
# matrix_lean: constant textures (variant 0); matrix_lean_tex: image maps, bilerps, a normal map and displacements (variant 1).
# x {default, WF_LEAN_SHADE=0 (2), WF_VISIBLE_SURFACE=1 (3)} x {default, WF_RARE_LIGHTS=1}: all 40 shade cells and all 20 NEE cells.
for _scene, _lean in (("matrix_lean", 0), ("matrix_lean_tex", 1)):
    for _env, _variant in (({}, _lean), ({"WF_LEAN_SHADE": "0"}, 2), ({"WF_VISIBLE_SURFACE": "1"}, 3)):
        for _rare in (0, 1):
            CASES.append(_case(_scene, dict(_env, **({"WF_RARE_LIGHTS": "1"} if _rare else {})), _all(_variant), _rare))

# ---- the per-type lean kernels taken away from the two goldens that plan them beside general types (tests/test_scene_plan_host.py):
# portal_light (diffuse lean, conductor and coated diffuse on spheres; a portal light: RARE), png_textures (coated diffuse lean)
CASES.append(_case("portal_light", {"WF_LEAN_PER_TYPE": "0"}, _all(2, (DIFFUSE, CONDUCTOR, COATED_DIFFUSE)), 1))
CASES.append(_case("png_textures", {"WF_LEAN_PER_TYPE": "0"}, _all(2, (DIFFUSE, CONDUCTOR, COATED_DIFFUSE)), 0))

# ---- existing goldens under each of the two forcing switches: the superset kernels meet what the matrix scenes lack (quadrics, patches,
# curves with alpha, instances, texture graphs, media, an environment map, emitters that are not triangles).
# scene: (the types whose queues hold items -> the variant its own plan gives them, whether its own lights are RARE)
_EXISTING = {
    # disks and cylinders only, two of them emitters
    "quadrics": (_all(2, (DIFFUSE, CONDUCTOR, DIELECTRIC)), 1),
    # curves with alpha textures: the visible-surface variant already (the switch changes nothing: the case pins that too)
    "curves_alpha": (_all(3, (DIFFUSE, DIELECTRIC, COATED_DIFFUSE)), 0),
    # bilinear patches and spheres only, four of them emitters
    "bilinear_lights": (_all(2, (DIFFUSE, CONDUCTOR, COATED_DIFFUSE)), 1),
    # object instances, a checkerboard alpha cut-out (a texture graph: no lean type)
    "instances": (_all(2, (DIFFUSE, CONDUCTOR, DIELECTRIC, DIFFUSE_TRANSMISSION, COATED_DIFFUSE)), 0),
    # hair on spheres, a cylinder and a mesh; the diffuse ground is a triangle mesh: lean
    "hair": ({DIFFUSE: 0, HAIR: 2}, 0),
    # measured BRDFs on spheres, a cylinder and meshes; a checkerboard displacement (a texture graph: no lean type); the emitter is diffuse
    "measured": (_all(2, (DIFFUSE, MEASURED)), 0),
    # triangle meshes, constant textures
    "subsurface": (_all(0, (DIFFUSE, SUBSURFACE)), 0),
    # procedural textures on spheres and meshes
    "textures_noise": (_all(2, (DIFFUSE, CONDUCTOR, COATED_DIFFUSE)), 0),
    # triangles in homogeneous and grid media: k_medium_scatter<RARE>
    "media_box": (_all(0, (DIFFUSE, CONDUCTOR, DIELECTRIC)), 0),
    # triangles under an image infinite light: k_handle_escaped<RARE>
    "envmap": (_all(0, (DIFFUSE, CONDUCTOR, DIELECTRIC, COATED_DIFFUSE)), 0),
}
# (mix_materials is left out: the reference's MixMaterial choice hashes heap pointers, so its golden is compared in 8x8 block means at
# 64 spp — test_gpu_parity.py test_mix_material — not bit for bit, which is what every case here is held to.)
for _scene, (_shade, _rare) in _EXISTING.items():
    CASES.append(_case(_scene, {"WF_VISIBLE_SURFACE": "1"}, _all(3, tuple(_shade)), _rare))
    CASES.append(_case(_scene, {"WF_RARE_LIGHTS": "1"}, _shade, 1))

MATRIX_SCENES = ("matrix_lean", "matrix_lean_tex")
SWITCHES = ("WF_LEAN_SHADE", "WF_LEAN_PER_TYPE", "WF_VISIBLE_SURFACE", "WF_RARE_LIGHTS")   # a test clears these before it sets a case's


def shade_cells(case):
    return {(t, v) for t, v in case.shade.items()}


def nee_cells(case):
    return {(t, case.rare) for t in case.shade}
