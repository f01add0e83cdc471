// wf_scene_view.h — how a wf_scene_desc (include/wf_abi.h) becomes a SceneView (wf_scene.h), written down once.  Host code only, no HIP
// header: the planner (csrc/hip/wf_plan.cpp) takes the scene's facts from here, the upload (csrc/hip/wf_backend.hip UploadTables) walks
// the table list with devUpload and assigns the scalar block, and the CPU oracle and the stand-alone checkers (oracle/wf_cpu, tools/)
// get their host view from HostSceneView — so the views the GPU tests' expected values are computed on cannot drift from the device's.
// A NEW SCENE TABLE is added here: a member of SceneView, one line of WF_SCENE_TABLES (or, for a scalar, of SetSceneScalars).
#pragma once
#include <cstddef>
#include <cstdint>
#include "wf_scene.h"

namespace wf {

// The tables of SceneView that are copies of wf_scene_desc arrays, in the order the upload allocates them (the order fixes the context's
// allocation list and with it the device addresses a scene gets): T(view member, description member, elements).  The element counts are
// read by the upload alone; they are written for a scope with `const wf_scene_desc *d` and `nBvhPrims` (planning::BvhPrimCount: what the
// leaves of the trees index).  ALSO(member) marks the place of a table with a condition or a derivation of its own — S, and the
// device-only shadeTris, lightBvhX, gridCorners / gridCornerBase and sobol — which its user spells out (UploadTables; HostSceneView).
#define WF_SCENE_TABLES(T, ALSO)                                                                              \
    T(P, P, (size_t)3 * d->n_vertices)                                                                        \
    T(N, N, (size_t)3 * d->n_vertices)                                                                        \
    T(UV, UV, (size_t)2 * d->n_vertices)                                                                      \
    ALSO(S)                                                                                                   \
    T(triIndices, tri_indices, (size_t)3 * d->n_triangles)                                                    \
    T(triMesh, tri_mesh, (size_t)d->n_triangles + d->n_quadrics)                                              \
    ALSO(shadeTris)                                                                                           \
    T(quadrics, quadrics, (size_t)d->n_quadrics)                                                              \
    T(sobolMatrices, sobol_matrices, d->sobol_matrices ? (size_t)1024 * 52 : (size_t)0)                       \
    T(vdcSobol, vdc_sobol, d->vdc_sobol ? (size_t)25 * 52 : (size_t)0)                                        \
    T(vdcSobolInv, vdc_sobol_inv, d->vdc_sobol_inv ? (size_t)26 * 52 : (size_t)0)                             \
    T(haltonPrimes, halton_primes, d->halton_primes ? (size_t)1000 : (size_t)0)                               \
    T(haltonPermOffsets, halton_perm_offsets, d->halton_perm_offsets ? (size_t)1000 : (size_t)0)              \
    T(haltonPerms, halton_perms, (size_t)d->n_halton_perms)                                                   \
    T(meshes, meshes, (size_t)d->n_meshes)                                                                    \
    T(bvhNodes, bvh_nodes, (size_t)d->n_bvh_nodes)                                                            \
    T(bvhPrims, bvh_prims, (size_t)nBvhPrims)                                                                 \
    T(instances, instances, (size_t)d->n_instances)                                                           \
    T(instanceDefs, instance_defs, (size_t)d->n_instance_defs)                                                \
    T(animated, animated, (size_t)d->n_animated)                                                              \
    T(spectra, spectra, (size_t)d->n_spectra)                                                                 \
    T(spectrumData, spectrum_data, (size_t)d->n_spectrum_floats)                                              \
    T(textures, textures, (size_t)d->n_textures)                                                              \
    T(materials, materials, (size_t)d->n_materials)                                                           \
    T(lights, lights, (size_t)d->n_lights)                                                                    \
    T(infiniteLights, infinite_lights, (size_t)d->n_infinite_lights)                                          \
    T(lightBvh, light_bvh_nodes, (size_t)d->n_light_bvh_nodes)                                                \
    ALSO(lightBvhX)                                                                                           \
    T(lightXforms, light_transforms, (size_t)d->n_light_transforms)                                           \
    T(powerAlias, power_alias, d->light_sampler == WF_LS_POWER ? (size_t)3 * d->n_lights : (size_t)0)         \
    T(imageLights, image_lights, (size_t)d->n_image_lights)                                                   \
    T(texImages, tex_images, (size_t)d->n_tex_images)                                                         \
    T(tableData, table_data, (size_t)d->n_table_floats)                                                       \
    T(rgb2specCoeffs, rgb2spec_coeffs, d->rgb2spec_coeffs ? (size_t)3 * 64 * 64 * 64 * 3 : (size_t)0)         \
    T(rgb2specZNodes, rgb2spec_znodes, (size_t)64)                                                            \
    T(noisePerm, noise_perm, d->noise_perm ? (size_t)512 : (size_t)0)                                         \
    T(media, media, (size_t)d->n_media)                                                                       \
    T(mediumData, medium_data, (size_t)d->n_medium_floats)                                                    \
    ALSO(gridCorners)                                                                                         \
    T(filterData, filter_data, (size_t)d->n_filter_floats)                                                    \
    ALSO(sobol)
// A member added to SceneView changes this size: give it its line in WF_SCENE_TABLES above or in SetSceneScalars below.
static_assert(sizeof(SceneView) == 1776, "SceneView changed: add the new member to WF_SCENE_TABLES or SetSceneScalars (wf_scene_view.h)");

// What a description holds, as far as the view and the plan record it (ScenePlan derives from this: csrc/hip/wf_plan.h).
struct SceneFacts {
    int nInstances = 0;
    bool haveAlpha = false, texNeedsFootprint = false, haveMix = false, haveSubsurface = false, haveQuadricAlpha = false, haveCurves = false, haveAnimated = false;
    int matTypeMask = 0;
    bool matPresent[WF_MAT_NTYPES] = {};
};
// (the description has passed the planner's checks, or comes from BuildSceneTables: every material is a mix or of a known type)
inline SceneFacts SceneFactsOf(const wf_scene_desc &d) {
    SceneFacts f;
    f.nInstances = d.n_instances;
    f.haveAnimated = d.n_animated > 0;
    for (int i = 0; i < d.n_meshes; ++i)
        if (d.meshes[i].alpha_tex >= 0) f.haveAlpha = true;
    for (int i = 0; i < d.n_textures; ++i)
        if (d.textures[i].type >= WF_TEX_FLOAT_IMAGE) f.texNeedsFootprint = true;
    for (int i = 0; i < d.n_materials; ++i)
        if (d.materials[i].displacement >= 0 || d.materials[i].normalmap >= 0) f.texNeedsFootprint = true;
    for (int i = 0; i < d.n_quadrics; ++i) {
        if (d.meshes[d.quadrics[i].mesh].alpha_tex >= 0) f.haveQuadricAlpha = true;
        if (d.quadrics[i].type == WF_QUADRIC_CURVE) f.haveCurves = true;
    }
    for (int i = 0; i < d.n_materials; ++i) {
        const int t = d.materials[i].type;
        if (t == WF_MAT_MIX) { f.haveMix = true; continue; }
        f.matPresent[t] = true;
        f.matTypeMask |= 1 << t;
        if (t == WF_MAT_SUBSURFACE) f.haveSubsurface = true;
    }
    return f;
}

// The scalars of SceneView: the description's, and the facts
inline void SetSceneScalars(SceneView *sv, const wf_scene_desc &d, const SceneFacts &f) {
    sv->nTriangles = d.n_triangles;
    sv->nBvhNodes = d.n_bvh_nodes;
    sv->nQuadrics = d.n_quadrics;
    sv->nLights = d.n_lights;
    sv->nInfiniteLights = d.n_infinite_lights;
    sv->nLightBvhNodes = d.n_light_bvh_nodes;
    sv->lightSampler = d.light_sampler;
    for (int i = 0; i < 6; ++i) sv->allLightBounds[i] = d.all_light_bounds[i];
    sv->camera = d.camera;
    sv->film = d.film;
    sv->filter = d.filter;
    sv->sampler = d.sampler;
    sv->csIlluminantOffset = d.cs_illuminant_offset;
    sv->maxDepth = d.max_depth;
    sv->regularize = d.regularize;
    sv->haveMedia = d.have_media;
    sv->options = d.options;
    sv->nInstances = f.nInstances;
    sv->haveAnimated = f.haveAnimated;
    sv->haveAlpha = f.haveAlpha;
    sv->texNeedsFootprint = f.texNeedsFootprint;
    sv->haveMix = f.haveMix;
    sv->haveSubsurface = f.haveSubsurface;
    sv->haveQuadricAlpha = f.haveQuadricAlpha;
    sv->haveCurves = f.haveCurves;
    sv->matTypeMask = f.matTypeMask;
}

// The view of a description on the host: every table aliases the description's array, the scalars are the device's.  The device-only
// tables (shadeTris, lightBvhX, gridCorners / gridCornerBase) stay null; `sobol` is the caller's FillSobol2D table (or null: no ZSobol
// sample is drawn); self and fatal are the caller's to set, once the view has its address.
inline SceneView HostSceneView(const wf_scene_desc &desc, const uint32_t *sobol) {
    SceneView sv{};
    const wf_scene_desc *d = &desc;
#define WF_ALIAS(member, table, count) sv.member = d->table;
#define WF_NOTHING(member)
    WF_SCENE_TABLES(WF_ALIAS, WF_NOTHING)
#undef WF_ALIAS
#undef WF_NOTHING
    sv.S = d->S;
    sv.sobol = sobol;
    SetSceneScalars(&sv, desc, SceneFactsOf(desc));
    return sv;
}

}  // namespace wf
