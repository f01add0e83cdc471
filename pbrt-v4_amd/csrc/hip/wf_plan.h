// wf_plan.h — what libwfhip.so decides about a scene on the host before anything is uploaded: the environment switches (Switches), the
// scene's plan (ScenePlan, PlanScene) and the production traversal layout as it is built (FastTrees, BuildFastBVH).  The definitions are
// plain C++ without a HIP call — wf_plan.cpp, wf_fastbvh_build.cpp — so they are compiled once, not per pass of the kernel unit, and a
// stand-alone host program can link them (tools/plan_dump.cpp).  wf_ctx.h includes this for the upload, the queries and the boundary calls.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <algorithm>
#include <vector>
#include "../common/wf_fastbvh.h"
#include "../common/wf_scene_view.h"

// (hidden: these names are shared by the library's units, not exported from it)
namespace wf { namespace planning __attribute__((visibility("hidden"))) {

// the message of wf_last_error (per thread); returns `code`, or -1 for 0
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// STAGE GRIDS.  A stage kernel is a grid-stride loop whose workgroups all run the same number of iterations, so a launch
// proceeds in rounds of `perCU * nCU` workgroups — as many as the chip keeps resident of that kernel — and a grid that is no whole
// number of rounds leaves part of the chip idle through its last one.  The workgroups of a launch over at most nMax items:
//   min(ceil(nMax / block), rounds * perCU * nCU)     rounds > 0 and the kernel's occupancy is known (perCU > 0)
//   min(ceil(nMax / block), STAGE_GRID_BOUND)         otherwise: the fixed bound of every round before this rule
// and in both cases at most `cap`, if one is set.  Never less than one workgroup.
constexpr int STAGE_GRID_BOUND = 256 * 8;    // 256 CUs x up to 8 resident 256-thread workgroups (wf_ctx.h: MAX_GRID)
constexpr int STAGE_ROUNDS_DEFAULT = 4;     // chosen from {1, 2, 4} on the flagship: profiles/stage_rounds_parent_vs_change.txt
inline int StageGrid(int64_t nMax, int block, int perCU, int nCU, int rounds, int cap) {
    const int64_t need = std::max<int64_t>(1, (nMax + block - 1) / std::max(1, block));
    int64_t most = rounds > 0 && perCU > 0 && nCU > 0 ? (int64_t)rounds * perCU * nCU : (int64_t)STAGE_GRID_BOUND;
    if (cap > 0) most = std::min<int64_t>(most, cap);
    return (int)std::min(need, most);
}

// The environment switches of context creation, scene upload (tree building included) and queue allocation, read in one place.  Each of those three calls takes a
// fresh copy when it runs (the tests set switches between calls); the code they steer sees values, not the environment.
struct Switches {
    bool shadeTris = true;        // WF_SHADE_TRIS=0: the indexed vertex tables only (wf_scene.h ShadeTri)
    bool gridCorners = true;      // WF_GRID_CORNERS=0: no corner-packed copies of the density grids
    double gridCornersGB = 32.0;  // WF_GRID_CORNERS_GB: tables beyond this many gigabytes in all are left out
    bool mediumLean = true;       // WF_MEDIUM_LEAN=0
    bool leanShade = true;        // WF_LEAN_SHADE=0
    bool leanPerType = true;      // WF_LEAN_PER_TYPE=0
    bool visibleSurface = false;  // WF_VISIBLE_SURFACE=1: every material type takes shade variant 3, whatever the scene (on only: a scene that needs it keeps it)
    bool rareLights = false;      // WF_RARE_LIGHTS=1: the RARE kernels (k_mat_nee<t, true>, k_medium_scatter<true>, k_handle_escaped<true>), whatever the scene's lights (on only)
    int deferGeneral = -1;        // WF_DEFER_GENERAL=1 | 0 forces / forbids the two-class traversal; -1 (unset): by the scene's counts
    bool noFast = false;          // WF_NO_FAST (set to anything): the reference-order walks only
    bool animFast = true;         // WF_ANIM_FAST=0
    bool pixelMajor = true;       // WF_PIXEL_MAJOR=0: items of a pass ordered sample by sample
    bool noSampleTops = false;    // WF_NO_SAMPLE_TOPS (set to anything)
    int trWavefront = -1;         // WF_TR_WAVEFRONT=1 | 0 forces / forbids the transmittance wavefront; -1 (unset): by the scene (ScenePlan::trRoute)
    int frameOverlap = 1;         // WF_FRAME_OVERLAP: 0 | 1 | 2 (wf_ctx::frameOverlap)
    int stageRounds = STAGE_ROUNDS_DEFAULT;   // WF_STAGE_ROUNDS: 0 | 1 .. 16, the stage kernels' grids in whole resident rounds (StageGrid); 0: the fixed bound only
    int stageGridCap = 0;         // WF_STAGE_GRID_CAP=<workgroups> (tests): no stage grid above this many workgroups, so that a tiny scene runs many grid-stride iterations; 0: none
    bool samplesShaded = true;    // WF_SAMPLES_SHADED=0
    bool traceLaunch = false;     // WF_TRACE_LAUNCH (set to anything)
    bool scratchPrime = true;     // WF_SCRATCH_PRIME=0
    // the tree builder's (BuildFastBVH)
    int leafCollapse = 1;         // WF_LEAF_COLLAPSE: 1..16 primitives a reference subtree may hold to become one leaf
    int braidMax = 2;             // WF_BRAID: 0..256, most entries one instance is opened into (measured on the spec scene, profiles/r06_rebraid_ab_sm16.txt: 2 is the optimum — DESIGN 4.1)
    bool tightInstances = true;   // WF_TIGHT_INSTANCES=0
    double braidMinFrac = 1.0 / 64;   // WF_BRAID_MIN_FRAC: an entry smaller than this fraction of the instance's own box is not opened further
    bool braidVerbose = false;    // WF_BRAID_VERBOSE=1: one line on stderr per re-braided tree
    static Switches FromEnv() {
        auto isSet = [](const char *name) { return getenv(name) != nullptr; };
        auto on = [](const char *name) { const char *e = getenv(name); return !(e && atoi(e) == 0); };   // on unless set to 0
        auto number = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
        Switches s;
        s.shadeTris = on("WF_SHADE_TRIS");
        s.gridCorners = on("WF_GRID_CORNERS");
        if (const char *e = getenv("WF_GRID_CORNERS_GB")) s.gridCornersGB = atof(e);
        s.mediumLean = on("WF_MEDIUM_LEAN");
        s.leanShade = on("WF_LEAN_SHADE");
        s.leanPerType = on("WF_LEAN_PER_TYPE");
        s.visibleSurface = number("WF_VISIBLE_SURFACE", 0) != 0;
        s.rareLights = number("WF_RARE_LIGHTS", 0) != 0;
        if (isSet("WF_DEFER_GENERAL")) s.deferGeneral = number("WF_DEFER_GENERAL", 0) != 0;
        s.noFast = isSet("WF_NO_FAST");
        s.animFast = on("WF_ANIM_FAST");
        s.pixelMajor = on("WF_PIXEL_MAJOR");
        s.noSampleTops = isSet("WF_NO_SAMPLE_TOPS");
        s.trWavefront = number("WF_TR_WAVEFRONT", -1);
        s.frameOverlap = std::min(2, std::max(0, number("WF_FRAME_OVERLAP", 1)));
        s.stageRounds = std::min(16, std::max(0, number("WF_STAGE_ROUNDS", STAGE_ROUNDS_DEFAULT)));
        s.stageGridCap = std::max(0, number("WF_STAGE_GRID_CAP", 0));
        s.samplesShaded = on("WF_SAMPLES_SHADED");
        s.traceLaunch = isSet("WF_TRACE_LAUNCH");
        s.scratchPrime = on("WF_SCRATCH_PRIME");
        s.leafCollapse = std::min(16, std::max(1, number("WF_LEAF_COLLAPSE", 1)));
        s.braidMax = std::min(256, std::max(0, number("WF_BRAID", 2)));
        s.tightInstances = on("WF_TIGHT_INSTANCES");
        if (const char *e = getenv("WF_BRAID_MIN_FRAC")) s.braidMinFrac = atof(e);
        s.braidVerbose = number("WF_BRAID_VERBOSE", 0) != 0;
        return s;
    }
};

// Everything decided about a scene: a pure function of the description and the switches (PlanScene), made before anything is uploaded.
// wf_ctx::plan is the one copy; wf_scene_plan_query gives the same answers without a context.
struct ScenePlan : SceneFacts {
    // what the description holds: SceneFacts (wf_scene_view.h SceneFactsOf; the upload copies these into SceneView) — nInstances, haveAlpha,
    // texNeedsFootprint, haveMix, haveSubsurface, haveQuadricAlpha, haveCurves, haveAnimated, matTypeMask, matPresent — and
    int64_t nBvhPrims = 0;       // entries of bvh_prims the trees index (wf_scene_check_instances)
    int nestedAnimated = 0;      // records of `instances` that are nested placements (animated shapes inside instance definitions); such scenes keep the reference-order walks
    // the stage kernels' variants
    bool mediumLean = false;     // every medium is homogeneous or a non-emissive uniform grid: k_medium_sample<true>
    bool portalLights = false;   // the scene has a portal infinite light (k_handle_escaped<RARE>)
    bool leanShade = false;      // the scene qualifies for the lean shade kernels (SceneLean)
    // ... per MATERIAL TYPE since round 6: a type none of whose materials sits on a quadric / patch / curve keeps its lean shade kernel
    // when such shapes appear elsewhere in the scene (their hits are items of other types' queues)
    bool leanType[WF_MAT_NTYPES] = {};
    bool rareLights = false;     // the scene has a light type only the VARIANT 2 material kernels sample (portal infinite lights)
    bool cameraAnim = false;     // the camera moves: k_gen_camera_rays<ANIM>
    // The shade kernel of each material type (k_mat_shade's variant): 0 / 1 the LEAN kernels (leanType), without / with the texture
    // footprint and bump block; 2 general; 3 general + what fills the visible surface (GBuffer film), differentiates a moving camera
    // and meets animated primitives or alpha-textured curves.  The variants agree bit for bit: a wrong rule here only costs time.
    int shadeVariant[WF_MAT_NTYPES] = {};
    int routeVariant = 0;        // the routing pass of the production closest-hit walk: 0 k_route_hits<false>, 1 <true> (general primitives or instances), 2 <true, true> (animated primitives)
    bool trFastAlpha = false;    // k_shadow_tr_fast<ALPHA>: alpha cut-outs or quadrics (wins over its MLEAN variant: there is no <true, true>)
    // the walk kernels' variants (PickWalkKernels turns these into template instantiations)
    int genMode = 0;             // general-primitive strength of the traversal kernels: 0 triangles only, 1 simple alpha, 2 anything but curves and alpha on quadrics, 3 anything (see GeneralPrims)
    bool deferGeneral = false;   // TWO-CLASS TRAVERSAL (see WalkKernels)
    int genTri = 0;
    bool fastBuilt = false;      // BuildFastBVH gave a production layout (FastTrees): it is uploaded, in use or not
    bool fastOk = false;         // ... and the scene's walks use it; false (leaf sizes > 16, nested placements, WF_NO_FAST, ...): the reference-order kernels only
    bool animFast = false;       // the scene's AnimatedPrimitives are walked by the production kernels' ANIM variants (round 6; genMode <= 1 only)
    int cursorChunk = 2;         // 64-ray batches a closest-hit wave takes per cursor fetch (chosen from the tree size)
    int cursorChunkShadow = 2;   // ... an any-hit wave (round 6, with the descent scheduling, 10 M-triangle scene: closest-hit 27.7 ms at 1, 26.7 at 3, 27.0 at 4, 27.4 at 8, 29.9 at 16;
                                 // any-hit 12.15 at 1, 12.16 at 3, 12.4 at 4, 13.0 at 8: profiles/r06_cursor_chunk_ab_sm16.txt)
                                 // (-3 %), but on a 30 k-triangle scene one fetch per 64 rays is 83 atomics/us on one counter: the kernel's bound
    int spillRows = 0;           // rows of wf_ctx::stackSpill behind the LDS stack entries, from the trees' depths
    // The transmittance stage (IntersectShadowTr) of the render and of wf_trace_shadow_tr_device: -1 the scene has no media, 0 the
    // reference-order walk per lane (k_shadow_tr), 1 the per-lane production walk (k_shadow_tr_fast: one-level static scenes), 2 the
    // transmittance wavefront (k_tr_begin / k_tr_trace / k_tr_segment / k_tr_rest).  WF_TR_WAVEFRONT: -1 (unset) = the wavefront for
    // two-level scenes and for scenes whose media are all lean, 1 = wherever its walk exists, 0 = never.  Measured on the cloud-like spec
    // scene (14 triangles, 512^3 grid, round 3): per-lane loop 27.9 ms per 16 spp, wavefront 31.4 ms (begin
    // 3.3 + trace 3.7 + segment 24.1 + rest 0.3) — the time is the ratio tracking through the grid, not the walk, and the per-lane loop
    // keeps its state in registers; with object instances the per-lane alternative is the reference-order walk (1 wave / SIMD).  Round 6,
    // one-level scenes whose media are all lean: k_tr_segment<true> runs at 3 waves (162 VGPRs) where the per-lane kernel is one wave of
    // 366 + 110 registers per SIMD — cloud scene 17.3 against 18.5 ms, profiles/r06_transmittance_lean_wavefront_ab_cloud16.txt.
    int trRoute = -1;
    // The kernel of wf_hit_interaction_device (wf_boundary_intr.hip), k_hit_interaction<GENERAL, CURVE_ALPHA, ANIM>, as IntrVariant() below
    // encodes it: GENERAL — the scene has quadrics / patches / curves; CURVE_ALPHA — one of its curves carries an alpha texture; ANIM — it
    // has animated primitives (nested placements included).  0: the lean triangle kernel.
    int intrVariant = 0;
    // The kernels of wf_light_sample_device / wf_light_emitted_device (wf_boundary_light.hip): k_light_sample<RARE> follows rareLights
    // (k_mat_nee's predicate); k_light_emitted<PORTAL, ALPHA, AREA_RARE> is encoded as EmittedVariant() below: PORTAL — portalLights
    // (LightLe<RARE>), ALPHA — an emitter carries an alpha texture (AreaLightL<ALPHA>), AREA_RARE — rareLights (the PDF of an emitter that
    // is not a triangle).  WF_RARE_LIGHTS=1 forces the general ones.
    int emittedVariant = 0;
    int nLights = 0, nInfiniteLights = 0;   // the sizes of the light table and of the list of infinite lights ("lights", "infinite_lights")
    int nMaterials = 0;                     // the size of the material table: what wf_bsdf_make_device / wf_bsdf_eval_device check a row's material id against
    int nMedia = 0, cameraMedium = -1;      // the size of the medium table (what wf_medium_sample_device checks a row's medium id against) and the camera's medium ("media", "camera_medium")
};
constexpr int EMITTED_PORTAL = 1, EMITTED_ALPHA = 2, EMITTED_AREA_RARE = 4;
constexpr int EmittedVariant(bool portal, bool alpha, bool areaRare) {
    return (portal ? EMITTED_PORTAL : 0) | (alpha ? EMITTED_ALPHA : 0) | (areaRare ? EMITTED_AREA_RARE : 0);
}
// The encoding of ScenePlan::intrVariant ("intr_variant"): the one place it is written down — the planner builds the value with it, the
// launcher of wf_boundary_intr.hip switches on it.  CURVE_ALPHA exists only with GENERAL (a curve is a general primitive).
constexpr int INTR_GENERAL = 1, INTR_CURVE_ALPHA = 2, INTR_ANIM = 4;
constexpr int IntrVariant(bool general, bool curveAlpha, bool anim) {
    return (general ? INTR_GENERAL : 0) | (general && curveAlpha ? INTR_CURVE_ALPHA : 0) | (anim ? INTR_ANIM : 0);
}
// which walk kernel variants resolve their near ties themselves (the others mark them for a re-trace launch)
constexpr bool RetraceInline(int gen) { return gen <= 1; }
// The production traversal layout as BuildFastBVH leaves it on the host: what the upload copies once PlanScene has succeeded.
struct FastTrees {
    std::vector<QNode> nodes;
    std::vector<LeafTri> tris;
    std::vector<FastDef> defs;
    std::vector<SubEntry> subs;
    FastBVH header{};
};
struct FastDepths { int top = 0, def = 0, maxLeafInstances = 0; };   // levels of the four-wide trees (top level / deepest definition), most instances in one leaf

int NestedPlacements(const wf_scene_desc *d);   // records of `instances` that are nested placements
int64_t BvhPrimCount(const wf_scene_desc *d);   // entries of bvh_prims the trees index
// wf_fastbvh_build.cpp; false: the scene has no production layout (leaves over 16 primitives, nested placements, ...)
bool BuildFastBVH(const wf_scene_desc *d, const Switches &sw, FastTrees *trees, FastDepths *depths);
// wf_plan.cpp
int CheckAbi(const wf_scene_desc *d);
int PlanScene(const wf_scene_desc *d, const Switches &sw, ScenePlan *plan, FastTrees *trees);
bool PlanValue(const ScenePlan &plan, const char *key, int64_t *value);

}}  // namespace wf::planning
