// wf_plan.cpp — the scene's plan: the checks that reject a description, its classification, and PlanScene, which puts them and the tree
// builder (wf_fastbvh_build.cpp) together; with the error text of the library (wf_last_error) and the two boundary calls that need no
// context, wf_scene_check_instances and wf_scene_plan_query.  Plain C++: no HIP header, no device.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include "wf_plan.h"

using namespace wf;
using namespace wf::planning;

// ---------------------------------------------------------------------------------------------
// errors
static thread_local char g_err[512] = "";
int wf::planning::fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code ? code : -1;
}
extern "C" const char *wf_last_error(void) { return g_err; }

// Nested placements (wf_abi.h wf_instance) exist in scenes with animated primitives only; without any, the two words that describe them are
// never read (callers that predate them may have left them unset).
int wf::planning::NestedPlacements(const wf_scene_desc *d) {
    int n = 0;
    if (d->n_animated > 0)
        for (int i = 0; i < d->n_instances; ++i) n += d->instances[i].outer_plus1 != 0;
    return n;
}
// Entries of bvh_prims: what the leaves of the trees index.  Every triangle / quadric once, every top-level instance once, and every nested
// placement ONCE PER DEFINITION (its records in `instances` repeat per use, its entry in the definition's leaves does not) — so this is
// n_triangles + n_quadrics + n_instances only while no definition with a nested placement is used more than once.
int64_t wf::planning::BvhPrimCount(const wf_scene_desc *d) {
    int64_t n = 0;
    for (int i = 0; i < d->n_bvh_nodes; ++i)
        if (d->bvh_nodes[i].nprims > 0) n = std::max(n, (int64_t)d->bvh_nodes[i].offset + d->bvh_nodes[i].nprims);
    return n;
}
extern "C" int wf_scene_check_instances(const wf_scene_desc *d, int64_t out[4]) {
    if (!d) return fail(-1, "wf_scene_check_instances: null argument");
    const int nGeom = d->n_triangles + d->n_quadrics, nI = d->n_instances, nD = d->n_instance_defs;
    const int64_t nPrims = BvhPrimCount(d);
    for (int i = 0; i < d->n_bvh_nodes; ++i) {
        const wf_bvh_node &n = d->bvh_nodes[i];
        if (n.offset < 0 || (n.nprims == 0 && n.offset >= d->n_bvh_nodes)) return fail(-1, "bvh_nodes[%d]: offset %d out of range", i, n.offset);
    }
    const int64_t nTop = nI > 0 ? d->n_top_prims : nPrims;
    if (nTop < 0 || nTop > nPrims) return fail(-1, "n_top_prims %d outside bvh_prims (%lld entries)", d->n_top_prims, (long long)nPrims);
    const bool anim = d->n_animated > 0;   // (the nested-placement words are read in such scenes only)
    int64_t nNestedRecords = 0, nNestedEntries = 0;
    // per definition: its range of bvh_prims, and how many nested placements its leaves name (entries nGeom + 0 .. nGeom + c - 1)
    std::vector<int> defNested((size_t)std::max(nD, 0), 0);
    for (int k = 0; k < nD; ++k) {
        const wf_instance_def &def = d->instance_defs[k];
        if (def.n_prims < 0 || def.first_prim < 0 || (int64_t)def.first_prim + def.n_prims > nPrims) return fail(-1, "instance_defs[%d]: bvh_prims range %d + %d outside the %lld entries", k, def.first_prim, def.n_prims, (long long)nPrims);
        if (def.bvh_root >= d->n_bvh_nodes) return fail(-1, "instance_defs[%d]: bvh_root %d out of range", k, def.bvh_root);
        int c = 0, hi = -1;
        for (int j = def.first_prim; j < def.first_prim + def.n_prims; ++j) {
            const int t = d->bvh_prims[j];
            if (t < 0) return fail(-1, "bvh_prims[%d] = %d", j, t);
            if (t >= nGeom) { ++c; hi = std::max(hi, t - nGeom); }
        }
        if (c > 0 && !anim) return fail(-1, "instance_defs[%d] names an instance in its leaves: only a scene with animated primitives can hold nested placements", k);
        if (hi >= c) return fail(-1, "instance_defs[%d]: nested placement %d named, %d present", k, hi, c);
        defNested[k] = c;
        nNestedEntries += c;
    }
    for (int64_t j = 0; j < nTop; ++j) {
        const int t = d->bvh_prims[j];
        if (t < 0 || t >= nGeom + nI) return fail(-1, "bvh_prims[%lld] = %d outside the primitives and instances", (long long)j, t);
        if (anim && t >= nGeom && d->instances[t - nGeom].outer_plus1 != 0) return fail(-1, "bvh_prims[%lld]: a nested placement's record among the top-level primitives", (long long)j);
    }
    for (int i = 0; i < nI; ++i) {
        const wf_instance &in = d->instances[i];
        if (in.def < 0 || in.def >= nD) return fail(-1, "instances[%d]: def %d out of range", i, in.def);
        if (in.anim_plus1 < 0 || in.anim_plus1 > d->n_animated) return fail(-1, "instances[%d]: anim_plus1 %d out of range", i, in.anim_plus1);
        if (!anim) continue;
        if (in.outer_plus1 != 0) {
            // a nested placement: animated, holds none itself, and belongs to the group of the use it names
            ++nNestedRecords;
            const int o = in.outer_plus1 - 1;
            if (o < 0 || o >= nI || d->instances[o].outer_plus1 != 0) return fail(-1, "instances[%d]: outer_plus1 %d does not name a use of a definition", i, in.outer_plus1);
            const int first = d->instances[o].nested_first, c = defNested[d->instances[o].def];
            if (first <= 0 || i < first || i >= first + c) return fail(-1, "instances[%d]: not among the %d nested records of instances[%d] (nested_first %d)", i, c, o, first);
            if (in.anim_plus1 == 0 || in.nested_first != 0 || defNested[in.def] != 0) return fail(-1, "instances[%d]: a nested placement is an animated primitive around a definition without nested placements", i);
        } else {
            const int c = defNested[in.def];
            if (c == 0) continue;   // (nested_first is not read)
            if (in.nested_first <= 0 || (int64_t)in.nested_first + c > nI) return fail(-1, "instances[%d]: nested_first %d + %d nested placements outside instances", i, in.nested_first, c);
            for (int k = 0; k < c; ++k)
                if (d->instances[in.nested_first + k].outer_plus1 != i + 1) return fail(-1, "instances[%d]: record %d is not nested placement %d of this use", i, in.nested_first + k, k);
        }
    }
    if (out) { out[0] = nPrims; out[1] = nI - nNestedRecords; out[2] = nNestedRecords; out[3] = nNestedEntries; }
    return 0;
}
// ---- the scene's plan (ScenePlan) ------------------------------------------------------------------------------------------------
// PlanScene, in its order: check the description, classify it, build the production trees, decide the walks.  Host code without a HIP
// call: wf_scene_upload runs it before it allocates anything (a rejected description leaves the context as it was), and
// wf_scene_plan_query runs it without a context.

// Every array the five interpolants of measured material i point to must lie inside table_data (the kernels index them unchecked)
static int CheckMeasuredTable(const wf_scene_desc *d, int i) {
    const int64_t nT = d->n_table_floats, h = d->materials[i].measured_table;
    if (h < 0 || h + WF_MEASURED_HEADER_WORDS > nT) return fail(-1, "measured material %d: header outside table_data", i);
    auto word = [&](int64_t k) { int32_t v; memcpy(&v, &d->table_data[h + k], 4); return (int64_t)v; };
    static const int nParams[5] = {0, 0, 2, 2, 3};
    static const bool hasCdf[5] = {false, false, true, true, false};
    for (int k = 0; k < 5; ++k) {
        const int64_t b = 16 + 16 * k, sx = word(b), sy = word(b + 1);
        if (sx < 2 || sy < 2 || sx > (1 << 20) || sy > (1 << 20)) return fail(-1, "measured material %d: interpolant %d has size %lld x %lld", i, k, (long long)sx, (long long)sy);
        int64_t slices = 1;
        for (int p = nParams[k] - 1; p >= 0; --p) {
            const int64_t ps = word(b + 2 + p), st = word(b + 5 + p), po = word(b + 8 + p);
            if (ps < 1 || ps > (1 << 20) || po < 0 || po + ps > nT || st != (ps > 1 ? slices : 0)) return fail(-1, "measured material %d: interpolant %d, parameter %d invalid", i, k, p);
            slices *= ps;
            if (slices > nT) return fail(-1, "measured material %d: interpolant %d larger than table_data", i, k);
        }
        const int64_t dataOff = word(b + 11), margOff = word(b + 12), condOff = word(b + 13);
        if (dataOff < 0 || dataOff + slices * sx * sy > nT) return fail(-1, "measured material %d: interpolant %d data outside table_data", i, k);
        if (hasCdf[k] && (margOff < 0 || margOff + slices * sy > nT || condOff < 0 || condOff + slices * sx * sy > nT))
            return fail(-1, "measured material %d: interpolant %d cdf outside table_data", i, k);
    }
    return 0;
}
// Step 1: everything that rejects a description, before anything indexes through its tables (on the host or on the device).
// counts: wf_scene_check_instances' out.
int wf::planning::CheckAbi(const wf_scene_desc *d) {
    return d->abi_version == WF_ABI_VERSION ? 0 : fail(-1, "ABI version mismatch: desc %d, library %d", d->abi_version, WF_ABI_VERSION);
}
static int CheckScene(const wf_scene_desc *d, int64_t counts[4]) {
    if (int e = CheckAbi(d)) return e;
    if (d->sampler.type == WF_SAMPLER_SOBOL && (!d->sobol_matrices || !d->vdc_sobol || !d->vdc_sobol_inv)) return fail(-1, "the Sobol sampler needs the sobol_matrices / vdc_sobol tables");
    if (int e = wf_scene_check_instances(d, counts)) return e;
    if (d->sampler.type < WF_SAMPLER_ZSOBOL || d->sampler.type > WF_SAMPLER_SOBOL) return fail(-1, "unknown sampler type %d", d->sampler.type);
    if (d->sampler.type == WF_SAMPLER_HALTON && (!d->halton_primes || (d->sampler.randomize == WF_RAND_PERMUTE_DIGITS && (!d->halton_perm_offsets || !d->halton_perms))))
        return fail(-1, "Halton sampler without its prime / digit-permutation tables");
    for (int i = 0; i < d->n_materials; ++i) {
        const wf_material &m = d->materials[i];
        if (m.type == WF_MAT_MIX) {
            if (m.mix[0] < 0 || m.mix[0] >= d->n_materials || m.mix[1] < 0 || m.mix[1] >= d->n_materials || m.mix[0] >= i || m.mix[1] >= i)
                return fail(-1, "mix material %d must name two earlier materials", i);
            continue;
        }
        if (m.type < 0 || m.type >= WF_MAT_NTYPES) return fail(-1, "material %d has unknown type %d", i, m.type);
        if (m.type == WF_MAT_SUBSURFACE && (m.sss_table < 0 || (size_t)m.sss_table + BSSRDF_TABLE_FLOATS > (size_t)d->n_table_floats))
            return fail(-1, "subsurface material %d: BSSRDF table outside table_data", i);
        if (m.type == WF_MAT_MEASURED)
            if (int e = CheckMeasuredTable(d, i)) return e;
    }
    if (d->film.type == WF_FILM_SPECTRAL && (d->film.n_buckets < 1 || d->film.n_buckets > 4096 || !(d->film.lambda_max > d->film.lambda_min)))
        return fail(-1, "spectral film: bad bucket count / wavelength range");
    return 0;
}
// Step 2: what the scene holds, and which variants of the stage and walk kernels that asks for.
static void ClassifyScene(const wf_scene_desc *d, const Switches &sw, ScenePlan *plan) {
    static_cast<SceneFacts &>(*plan) = SceneFactsOf(*d);
    plan->nestedAnimated = NestedPlacements(d);
    // the lean delta-tracking kernel (k_medium_sample<true>): no procedural cloud, NanoVDB, RGB grid or emissive grid in the scene (WF_MEDIUM_LEAN=0: off)
    plan->mediumLean = d->n_media > 0 && sw.mediumLean;
    for (int m = 0; m < d->n_media; ++m)
        if (!(d->media[m].type == WF_MEDIUM_HOMOGENEOUS || (d->media[m].type == WF_MEDIUM_GRID && !d->media[m].is_emissive))) plan->mediumLean = false;
    // the lean shade kernels (wf_scene.h "LEAN DEVICE VARIANTS"): no quadrics / patches / curves, every texture a constant, an image map or a
    // bilerp (WF_LEAN_SHADE=0 turns them off)
    bool simpleTextures = true;
    for (int i = 0; i < d->n_textures && simpleTextures; ++i)
        if (!wf::IsSimpleFloatTexture(d->textures[i].type) && !wf::IsSimpleSpectrumTexture(d->textures[i].type)) simpleTextures = false;
    plan->leanShade = d->n_quadrics == 0 && d->n_animated == 0 && sw.leanShade && simpleTextures;
    {
        // the material types met on shapes that are not triangles (through MixMaterials, whose hits join the queue of the chosen material's type)
        bool onGeneral[WF_MAT_NTYPES] = {};
        std::vector<int> todo;
        for (int i = 0; i < d->n_quadrics; ++i) {
            const int m = d->meshes[d->quadrics[i].mesh].material;
            if (m >= 0 && m < d->n_materials) todo.push_back(m);
        }
        std::vector<char> seen((size_t)std::max(d->n_materials, 1), 0);
        while (!todo.empty()) {
            const int m = todo.back();
            todo.pop_back();
            if (m < 0 || m >= d->n_materials || seen[m]) continue;
            seen[m] = 1;
            const int t = d->materials[m].type;
            if (t == WF_MAT_MIX) { todo.push_back(d->materials[m].mix[0]); todo.push_back(d->materials[m].mix[1]); }
            else if (t >= 0 && t < WF_MAT_NTYPES) onGeneral[t] = true;
        }
        const bool wanted = sw.leanShade && sw.leanPerType;
        for (int t = 0; t < WF_MAT_NTYPES; ++t) plan->leanType[t] = plan->leanShade || (wanted && simpleTextures && d->n_animated == 0 && !onGeneral[t]);
    }
    // ... and, since round 5, emitters that are not triangles (sphere / disk / cylinder / patch / curve lights: an out-of-line sampler of
    // 214 VGPRs) and emitters with an alpha texture (the texture-graph evaluator): LightSampleLi<RARE>, AreaLightL<ALPHA> (wf_lights.h)
    // (WF_RARE_LIGHTS=1 forces both: the RARE kernels are supersets, they sample every light type)
    if (sw.rareLights) plan->rareLights = plan->portalLights = true;
    bool emitterAlpha = sw.rareLights;
    for (int i = 0; i < d->n_lights; ++i) {
        const wf_light &l = d->lights[i];
        if (l.type == WF_LIGHT_PORTAL_INFINITE) plan->rareLights = plan->portalLights = true;
        if (l.type == WF_LIGHT_DIFFUSE_AREA && (l.tri >= d->n_triangles || l.alpha_tex_plus1 != 0)) plan->rareLights = true;
        if (l.type == WF_LIGHT_DIFFUSE_AREA && l.alpha_tex_plus1 != 0) emitterAlpha = true;
    }
    // the emission kernel of the device-buffer boundary (ScenePlan::emittedVariant)
    plan->emittedVariant = EmittedVariant(plan->portalLights, emitterAlpha, plan->rareLights);
    plan->nLights = d->n_lights;
    plan->nInfiniteLights = d->n_infinite_lights;
    plan->nMedia = d->n_media;
    plan->cameraMedium = d->n_media > 0 && d->camera.medium >= 0 && d->camera.medium < d->n_media ? d->camera.medium : -1;
    plan->nMaterials = d->n_materials;
    if (d->n_quadrics > 0) plan->genMode = (plan->haveCurves || plan->haveQuadricAlpha) ? 3 : 2;
    {
        // the hit-interaction kernel of the device-buffer boundary (ScenePlan::intrVariant): allocated what the scene can make it reach
        bool curveAlpha = false;
        for (int i = 0; i < d->n_quadrics; ++i)
            if (d->quadrics[i].type == WF_QUADRIC_CURVE && d->meshes[d->quadrics[i].mesh].alpha_tex >= 0) curveAlpha = true;
        plan->intrVariant = IntrVariant(d->n_quadrics > 0, curveAlpha, d->n_animated > 0);
    }
    int alphaGen = 0;   // what the TRIANGLES of the scene ask of the walk: 0 nothing, 1 simple alpha cut-outs, 2 texture-graph alpha
    for (int i = 0; i < d->n_meshes && alphaGen < 2; ++i)
        if (d->meshes[i].alpha_tex >= 0) {
            const int tt = d->textures[d->meshes[i].alpha_tex].type;
            // the inline test looks an image map up without a footprint (MIPFilterFloatZeroP): uv-mapped, not EWA-filtered
            const wf_texture &at = d->textures[d->meshes[i].alpha_tex];
            const bool lean = tt == WF_TEX_FLOAT_CONSTANT || (at.mapping == WF_TEXMAP_UV && (tt != WF_TEX_FLOAT_IMAGE || d->tex_images[at.i0].filter != WF_MIP_EWA));
            alphaGen = std::max(alphaGen, ((tt == WF_TEX_FLOAT_CONSTANT || tt == WF_TEX_FLOAT_IMAGE || tt == WF_TEX_FLOAT_BILERP) && lean) ? 1 : 2);
        }
    plan->genMode = std::max(plan->genMode, alphaGen);
    // TWO-CLASS TRAVERSAL: the scene's quadrics / patches / curves are few beside its triangles, and the triangles themselves need no
    // more than the simple alpha test — the triangle kernels walk first, the general kernels only the rays handed over
    // (WF_DEFER_GENERAL=1 | 0 forces / forbids it for any scene with such shapes)
    plan->genTri = std::min(alphaGen, 1);
    if (d->n_quadrics > 0 && alphaGen <= 1 && plan->genMode >= 2) {
        const bool few = (int64_t)d->n_quadrics * 16 <= (int64_t)d->n_triangles;
        plan->deferGeneral = sw.deferGeneral >= 0 ? sw.deferGeneral != 0 : few;
    }
    // the stage kernels' remaining variants (genMode is final here)
    plan->cameraAnim = d->camera.anim.actually_animated;
    plan->trFastAlpha = plan->haveAlpha || d->n_quadrics > 0;
    plan->routeVariant = plan->haveAnimated ? 2 : (plan->genMode > 1 || plan->nInstances > 0) ? 1 : 0;
    // (WF_VISIBLE_SURFACE=1 forces it: variant 3 is a superset of the others, and its visible-surface store is guarded by the film's type)
    const bool visibleSurface = sw.visibleSurface || d->film.type == WF_FILM_GBUFFER || plan->cameraAnim || plan->haveAnimated || (plan->haveCurves && plan->haveQuadricAlpha);
    for (int t = 0; t < WF_MAT_NTYPES; ++t) plan->shadeVariant[t] = visibleSurface ? 3 : !plan->leanType[t] ? 2 : plan->texNeedsFootprint ? 1 : 0;
}
// levels of the reference's binary tree under `root`
static int RefTreeDepth(const wf_scene_desc *d, int root) {
    int best = 0;
    if (root < 0 || root >= d->n_bvh_nodes) return best;
    std::vector<std::pair<int, int>> st{{root, 1}};
    while (!st.empty()) {
        auto [i, dep] = st.back();
        st.pop_back();
        best = std::max(best, dep);
        if (d->bvh_nodes[i].nprims == 0) { st.push_back({i + 1, dep + 1}); st.push_back({d->bvh_nodes[i].offset, dep + 1}); }
    }
    return best;
}
int wf::planning::PlanScene(const wf_scene_desc *d, const Switches &sw, ScenePlan *plan, FastTrees *trees) {
    *plan = ScenePlan{};
    int64_t counts[4];
    if (int e = CheckScene(d, counts)) return e;
    plan->nBvhPrims = counts[0];
    ClassifyScene(d, sw, plan);
    // Step 3: the production trees, and the traversal stacks behind them.
    FastDepths fdep;
    plan->fastBuilt = BuildFastBVH(d, sw, trees, &fdep);
    {
        // LDS entries per lane + rows of `stackSpill` behind them, sized from the trees' ACTUAL depths: the
        // reference-order walk pushes one sibling per level of the reference's binary trees (top level, then an instance
        // definition's on top); the four-wide production walk up to three per level of ITS collapsed trees (BuildFastBVH records
        // their depths: the greedy largest-area collapse does not halve the depth of an unbalanced tree), one entry per instance
        // of a leaf, and the two instance markers.  A push past the rows is dropped and flagged (LdsStackT, wf_sync).
        int depthTop = d->n_bvh_nodes > 0 ? RefTreeDepth(d, 0) : 0, depthDef = 0;
        for (int k = 0; k < d->n_instance_defs; ++k) depthDef = std::max(depthDef, RefTreeDepth(d, d->instance_defs[k].bvh_root));
        // (a definition with nested placements carries a third level: a moving entity's tree on top of the definition's)
        const int needRef = depthTop + (plan->nestedAnimated > 0 ? 2 : 1) * depthDef + 4;
        const int needFast = 3 * fdep.top + fdep.maxLeafInstances + 3 * fdep.def + 6;
        plan->spillRows = std::max(std::max(needRef - std::min(STACK_LDS, TSTACK), needFast - TSTACK), STACK_MAX - std::min(STACK_LDS, TSTACK));
        if (plan->spillRows > 2048) return fail(-1, "BVH too deep for the traversal stacks (depth %d + %d)", depthTop, depthDef);
    }
    // Step 4: which walks use the trees.
    plan->fastOk = plan->fastBuilt && !sw.noFast;
    if (plan->fastBuilt) {
        // rays of a scene whose trees do not fit the caches walk long enough for one cursor fetch per 64 rays (measured: -3 % on
        // the 10 M-triangle scene); a cache-resident scene traces so fast that the cursor's atomics would bound it (see cursorChunk)
        const bool big = trees->nodes.size() * sizeof(QNode) + trees->tris.size() * sizeof(LeafTri) > ((size_t)256 << 20);
        plan->cursorChunk = big ? 3 : 2;
        plan->cursorChunkShadow = big ? 1 : 2;
    }
    // AnimatedPrimitive: the production walks' ANIM variants (triangles + simple alpha cut-outs, two-level: an animated shape entity is an
    // instance) interpolate the transformation per ray since round 6; scenes that also hold quadrics / curves / texture-graph alpha keep the
    // reference-order walks (WF_ANIM_FAST=0: every animated scene does)
    plan->animFast = d->n_animated > 0 && plan->fastOk && plan->genMode <= 1 && plan->nInstances > 0 && sw.animFast;
    if (d->n_animated > 0 && !plan->animFast) plan->fastOk = false;
    // Step 5: the transmittance stage's route (ScenePlan::trRoute).  The wavefront walks with k_tr_trace, which exists for the variants
    // that resolve their near ties inside the walk, static and ANIM; the per-lane production walk has neither a two-level nor an ANIM variant.
    if (d->have_media) {   // (what SceneView::haveMedia is: the scenes whose shadow stage is IntersectShadowTr)
        const bool wavefront = sw.trWavefront == 1 || (sw.trWavefront < 0 && (plan->nInstances > 0 || plan->mediumLean));
        if (plan->fastOk && RetraceInline(plan->genMode) && wavefront) plan->trRoute = 2;
        else if (plan->fastOk && !plan->animFast && plan->nInstances == 0) plan->trRoute = 1;
        else plan->trRoute = 0;
    }
    return 0;
}
// "<prefix><t>" with t a material type written in digits alone -> t; any other key -> -1
static int TypeKey(const std::string &k, const char *prefix) {
    const size_t n = strlen(prefix);
    if (k.compare(0, n, prefix) != 0 || k.size() == n || k.size() > n + 2 || k.find_first_not_of("0123456789", n) != std::string::npos) return -1;
    const int t = atoi(k.c_str() + n);
    return t < WF_MAT_NTYPES ? t : -1;
}
// The answers of wf_ctx_query / wf_scene_plan_query that the plan alone gives; false: not one of its keys.
bool wf::planning::PlanValue(const ScenePlan &plan, const char *key, int64_t *value) {
    const std::string k = key;
    if (k == "fast_ok") *value = plan.fastOk;
    else if (k == "gen_mode") *value = plan.genMode;
    else if (k == "gen_tri") *value = plan.genTri;
    else if (k == "defer_general") *value = plan.deferGeneral;
    else if (k == "anim_fast") *value = plan.animFast;
    else if (k == "lean_shade") *value = plan.leanShade;
    else if (k == "rare_lights") *value = plan.rareLights;     // k_mat_nee<t, RARE>, k_medium_scatter<RARE>
    else if (k == "portal_lights") *value = plan.portalLights; // k_handle_escaped<RARE>
    else if (k == "medium_lean") *value = plan.mediumLean;   // k_medium_sample<true> / k_tr_segment<true>: every medium is homogeneous or a non-emissive uniform grid
    else if (TypeKey(k, "lean_type_") >= 0) *value = plan.leanType[TypeKey(k, "lean_type_")];
    else if (k == "instances") *value = plan.nInstances;
    else if (k == "nested_animated") *value = plan.nestedAnimated;
    else if (k == "intr_variant") *value = plan.intrVariant;   // k_hit_interaction<GENERAL, CURVE_ALPHA, ANIM> (IntrVariant, wf_plan.h)
    else if (k == "light_sample_rare") *value = plan.rareLights;          // k_light_sample<RARE> (wf_boundary_light.hip)
    else if (k == "light_emitted_variant") *value = plan.emittedVariant;  // k_light_emitted<PORTAL, ALPHA, AREA_RARE> (EmittedVariant, wf_plan.h)
    else if (k == "lights") *value = plan.nLights;
    else if (k == "infinite_lights") *value = plan.nInfiniteLights;
    else if (k == "medium_sample_variant") *value = plan.mediumLean;   // k_medium_track<LEAN> (wf_boundary_medium.hip): chosen as k_medium_sample<LEAN> is
    else if (k == "media") *value = plan.nMedia;
    else if (k == "camera_medium") *value = plan.cameraMedium;
    else if (k == "bsdf_planes") *value = WF_BSDF_PLANES;          // the planes of a wf_bsdf_make_device record
    else if (k == "material_types") *value = plan.matTypeMask;     // bit t: the scene holds a material of type t — the k_bsdf_make / k_bsdf_eval launches of a call (wf_boundary_bsdf.hip)
    else if (k == "tr_route") *value = plan.trRoute;  // -1 no media, 0 k_shadow_tr, 1 k_shadow_tr_fast, 2 the transmittance wavefront
    else if (k == "camera_anim") *value = plan.cameraAnim;   // k_gen_camera_rays<ANIM>
    else if (k == "route_variant") *value = plan.routeVariant;   // 0 k_route_hits<false>, 1 <true>, 2 <true, true>
    else if (TypeKey(k, "shade_variant_") >= 0) *value = plan.shadeVariant[TypeKey(k, "shade_variant_")];   // k_mat_shade's variant for material type t
    else if (k.compare(0, 11, "stage_grid:") == 0) {
        // the grid rule itself (StageGrid, wf_plan.h), whatever the scene: "stage_grid:<n_max>:<block>:<per CU>:<CUs>:<rounds>:<cap>"
        long long n = 0;
        int block = 0, perCU = 0, nCU = 0, rounds = 0, cap = 0, used = 0;
        if (sscanf(k.c_str() + 11, "%lld:%d:%d:%d:%d:%d%n", &n, &block, &perCU, &nCU, &rounds, &cap, &used) != 6 || k.size() != (size_t)(11 + used) || n < 0 || block < 1) return false;
        *value = StageGrid(n, block, perCU, nCU, rounds, cap);
    }
    else return false;
    return true;
}


extern "C" int wf_scene_plan_query(const wf_scene_desc *d, const char *key, int64_t *value) {
    if (!d || !key || !value) return fail(-1, "wf_scene_plan_query: null argument");
    ScenePlan plan;
    FastTrees trees;
    if (int e = PlanScene(d, Switches::FromEnv(), &plan, &trees)) return e;
    if (!PlanValue(plan, key, value)) return fail(-1, "wf_scene_plan_query: unknown key '%s'", key);
    return 0;
}
