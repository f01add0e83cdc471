// wf_ctx.h — libwfhip.so's internal header: the context behind the C ABI's opaque wf_ctx and the launch plumbing, for the units that hold
// the entry points of include/wf_abi.h — wf_backend.hip (the render and every kernel of it), wf_boundary.hip (the boundary calls),
// wf_results.hip (what a caller reads back) and wf_probe.hip (the tests' probe kernels).  Each thing is defined once, here; the few
// functions of wf_backend.hip that the other units call are declared at the end.  All four units are compiled with the same flags
// (Makefile: BACKENDFLAGS, EXTRA): they must agree on wf_ctx, and the probe kernels keep the instructions they had inside wf_backend.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

// These units are compiled with -ftrivial-auto-var-init=zero (Makefile, BACKENDFLAGS; DESIGN 4.1 "Locals that start as undef"): the walk
// loops of wf_backend.hip and wf_traverse.h spill a third less when no local starts as undef.  The shared stage code keeps the default: its
// out-of-line shape / texture functions grow by 15 VGPRs when initialised, which takes the general-primitive walk kernels (GEN = 2)
// from 165 to 180 registers and from 3 waves to 2 (-9 / -12 % on the spec scene plus one sphere).
#pragma clang attribute push(__attribute__((uninitialized)), apply_to = variable(is_local))
#include "../common/wf_kernels.h"
#include "../common/wf_kat.h"
#pragma clang attribute pop
#include "wf_traverse.h"
#include "wf_plan.h"
#include "wf_film_develop.h"
#include "wf_boundary_intr.h"
#include "wf_film_add.h"
#include "wf_boundary_light.h"

using namespace wf;
using namespace wf::planning;

// ---------------------------------------------------------------------------------------------
// errors: fail() of wf_plan.h sets the text of wf_last_error
#define HIPCHK(call)                                                                                        \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess) return fail((int)e_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// ---------------------------------------------------------------------------------------------
constexpr int BLOCK = 256;
constexpr int MAX_GRID = 256 * 8;  // 256 CUs x up to 8 resident 256-thread workgroups

struct SpillArea { int *base; int rows; int *dbg; };   // the context's stackSpill rows + the debug words (kernel argument of the production traversal)

// The production walk kernels of the uploaded scene and their resident grids: filled once, by PickWalkKernels in the traversal step of
// wf_scene_upload, the only place that turns the plan's (genMode, genTri, deferGeneral, animFast, nInstances) into template instantiations.
// Every launch below goes through these pointers, so the kernel whose occupancy sized a grid is the kernel launched on it.
// (every instantiation of a walk kernel template has the signature of its pointer type)
using ClosestWalkFn = void (*)(const SceneView, WorkState, FastBVH, int, SpillArea, int *, int, const int *);   // k_closest_fast
using ShadowWalkFn = void (*)(const SceneView, WorkState, FastBVH, SpillArea, int *, int, const int *);         // k_shadow_fast
using TrTraceFn = void (*)(const SceneView, WorkState, FastBVH, int, SpillArea);                                // k_tr_trace
using TraceClosestFn = void (*)(const SceneView, FastBVH, int, const float *, wf_hit_record *, SpillArea);      // k_trace_closest_fast
using TraceAnyFn = void (*)(const SceneView, FastBVH, int, const float *, int32_t *, SpillArea);                // k_trace_any_fast
struct WalkKernels {
    ClosestWalkFn closest = nullptr;   // the launch every ray goes through
    ShadowWalkFn shadow = nullptr;
    // TWO-CLASS TRAVERSAL (round 6): `closest` / `shadow` are then the triangle kernels (genTri = 0 | 1) in their handing-over variants, and
    // these the general kernels (genMode >= 2) that walk only the rays handed to deferQ; null otherwise
    ClosestWalkFn closestGen = nullptr;
    ShadowWalkFn shadowGen = nullptr;
    int grid = 1024, gridShadow = 1024, gridGen = 1024, gridShadowGen = 1024;   // resident workgroups of the four, each from its own kernel's occupancy
    // The kernels below are launched on `grid`, the closest-hit walk's, and k_shadow_tr_fast with them, not on grids of their own: an
    // occupancy query per kernel would change their launches and so their times — a measurement of its own, left as it is here.
    TrTraceFn trTrace = nullptr;       // the transmittance wavefront's walk (genMode <= 1 only: null otherwise)
    TraceClosestFn traceClosest = nullptr;   // wf_trace_closest_device / wf_trace_any_device
    TraceAnyFn traceAny = nullptr;
    // wf_trace_closest_device_t / wf_trace_any_device_t (rays8): the same variants reading eight floats per ray, or — plan.animFast — the
    // ANIM variants the render walks the scene's AnimatedPrimitives with, at every ray's own time
    TraceClosestFn traceClosest8 = nullptr;
    TraceAnyFn traceAny8 = nullptr;
};
// ... and the stage kernels that have variants, the same way: filled once, by PickStageKernels beside PickWalkKernels, the only function
// that names a template argument of a stage kernel.  What a launch site may still choose is an index of run-time state: a counting pass
// (ctx->countTraversal), items that carry times.
using StageFn = void (*)(const SceneView, WorkState, int);                  // (sv, ws, cur)
using StageSpillFn = void (*)(const SceneView, WorkState, int *);           // (sv, ws, stackSpill): the reference-order any-hit / transmittance / probe walks
using StageCurSpillFn = void (*)(const SceneView, WorkState, int, int *);   // (sv, ws, cur, stackSpill): k_intersect_closest, k_tr_rest
using CameraRaysFn = void (*)(const SceneView, WorkState, int, int, int, int);
using ShadowTrFastFn = void (*)(const SceneView, WorkState, FastBVH, SpillArea);
using TraceOneRandomFn = void (*)(const SceneView, int, const float *, int, const int32_t *, const float *, int, wf_hit_record *, float *, int *);
// the boundary calls' reference-order walks over a caller's rays (sv, n, rays, rayStride, [times, timeStride,] results ..., stackSpill [, mode | counts])
using TraceClosestRefFn = void (*)(const SceneView, int, const float *, int, wf_hit_record *, int *, int);                                // k_trace_closest
using TraceAnyRefFn = void (*)(const SceneView, int, const float *, int, int32_t *, int32_t *, int32_t *, int *);                        // k_trace_any
using TraceClosestTimedFn = void (*)(const SceneView, int, const float *, int, const float *, int, wf_hit_record *, int *, int);         // k_trace_closest_timed
using TraceAnyTimedFn = void (*)(const SceneView, int, const float *, int, const float *, int, int32_t *, int *);                        // k_trace_any_timed
using PackShadowItemsFn = void (*)(int, const float *, F4 *, F4 *, F4 *, float *, F4 *, int32_t *);                                       // k_pack_shadow_items
// the two halves of the material stage (wf_mat.hip): shade variant 0 | 1 (lean) | 2 | 3, next-event estimation variant 0 | 1
using MatShadeFn = void (*)(hipStream_t, int, const SceneView *, const WorkState *, int);
using MatNeeFn = void (*)(hipStream_t, int, const SceneView *, const WorkState *);
struct StageKernels {
    CameraRaysFn genCameraRays = nullptr;
    StageCurSpillFn intersectClosest[2] = {};   // the reference-order walks, [counting pass]
    StageSpillFn intersectShadow[2] = {}, intersectOneRandom = nullptr;   // ... and the subsurface probe's
    StageFn routeHits = nullptr;
    int routeBlock = 0;                         // ... and the threads of its workgroups (RouteBlock)
    StageFn resolveMix = nullptr, mediumSample = nullptr, mediumRoute = nullptr, mediumScatter = nullptr, handleEscaped = nullptr, trSegment = nullptr;
    StageCurSpillFn trRest = nullptr;           // (with trSegment the transmittance wavefront's; its walk: WalkKernels::trTrace)
    StageSpillFn shadowTr[2] = {};              // the reference-order transmittance walk, [items carry times]
    ShadowTrFastFn shadowTrFast = nullptr, shadowTrFastWitness = nullptr;   // the per-lane production transmittance walk: of plan.trRoute == 1, of the host-array calls (LaunchHostTr)
    TraceOneRandomFn traceOneRandom[2] = {};    // [segments carry times]
    // the kernels only the boundary calls launch (wf_boundary.hip), which have no variants: here so that no other unit names a kernel of wf_backend.hip
    TraceClosestRefFn traceClosestRef = nullptr;
    TraceAnyRefFn traceAnyRef = nullptr;
    TraceClosestTimedFn traceClosestTimed = nullptr;
    TraceAnyTimedFn traceAnyTimed = nullptr;
    PackShadowItemsFn packShadowItems = nullptr;
    MatShadeFn shade[WF_MAT_NTYPES] = {};       // the rows of kMatShade / kMatNee the plan chose; [0]: WF_MAT_INTERFACE has no kernel
    MatNeeFn nee[WF_MAT_NTYPES] = {};
};
// STAGE GRIDS (wf_plan.h StageGrid): the launch sites of the render pass whose kernels are grid-stride loops over a queue, and
// what PickStageGrids found out about the kernel each of them launches for this scene.  ("stage_grid_<site>" of wf_ctx_query counts in
// this order.)  Not among them: k_reset (one workgroup), the production walks (WalkKernels: resident grids of their own), the near-tie
// re-trace and the transmittance wavefront's rest (128 workgroups), the film update, and the reference-order walks of a counting pass.
enum StageSite {
    SITE_SAMPLE_TOPS, SITE_CAMERA_RAYS, SITE_RAY_SAMPLES, SITE_ROUTE_HITS, SITE_RESOLVE_MIX, SITE_INTERSECT_CLOSEST, SITE_MEDIUM_SAMPLE, SITE_MEDIUM_ROUTE,
    SITE_MEDIUM_SCATTER, SITE_TR_BEGIN, SITE_TR_SEGMENT, SITE_SHADOW_TR, SITE_HANDLE_ESCAPED, SITE_HANDLE_EMISSIVE, SITE_INTERSECT_SHADOW,
    SITE_SUBSURFACE_PROBE, SITE_INTERSECT_ONE_RANDOM, SITE_SUBSURFACE_SCATTER,
    SITE_SHADE0,                              // + material type
    SITE_NEE0 = SITE_SHADE0 + WF_MAT_NTYPES,   // + material type
    SITE_COUNT = SITE_NEE0 + WF_MAT_NTYPES
};
struct StageGrids {
    struct Site {
        bool used = false;      // the scene launches a kernel here
        int block = 0;          // threads of its workgroups
        int perCU = 0;          // workgroups of it one CU keeps resident; 0: the query failed, the site keeps the fixed bound
        bool spillRows = false; // a reference-order walk: indexes wf_ctx::stackSpill by global thread, so its grid stays within MAX_GRID
    } site[SITE_COUNT];
    int rounds = 0, cap = 0;    // WF_STAGE_ROUNDS, WF_STAGE_GRID_CAP as the upload read them
    int nCU = 0;
    int fallbacks = 0;          // sites in use whose query failed
};

struct wf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<void *> allocs;
    SceneView svHost{};          // device pointers inside; passed to every kernel by value (kernarg)
    const SceneView *svDev = nullptr;  // the same struct in device memory, for the out-of-line callbacks of the traversal kernels
    WorkState ws{};
    int maxQueueSize = 0;
    int *stackSpill = nullptr;   // [plan.spillRows][MAX_GRID*BLOCK]
    int *dbgWords = nullptr;     // [4] spilled stack entries, stack-overflow flag, inline near-tie re-traces, cursor path taken (wf_debug_counters)
    SpillArea spillArea() const { return SpillArea{stackSpill, plan.spillRows, dbgWords}; }
    FastBVH fast{};              // production traversal layout (wf_traverse.h); built at upload
    hipStream_t stream2 = nullptr;   // the near-tie re-trace runs here, beside the routing pass and the next stage's sample generation
    hipEvent_t evFork = nullptr, evJoin = nullptr;
    bool retracePending = false, deferJoin = false;
    // FRAME SCHEDULING (wf_render_pass): the shadow stage of depth d — the any-hit launch(es) and "Reset shadowRayQueue" — runs on stream3
    // beside the reset, closest-hit walk, routing and sample generation of depth d + 1.  WF_FRAME_OVERLAP: 0 serial, 1 at every depth,
    // 2 from depth FRAME_OVERLAP_THIN_DEPTH on (read once, at wf_ctx_create).  A third stream and not stream2: the near-tie re-trace of
    // depth d + 1 (genMode >= 2) is then ordered behind nothing but its own closest-hit launch, as before.
    hipStream_t stream3 = nullptr;
    hipEvent_t evShadowFork = nullptr, evShadowJoin = nullptr;
    int frameOverlap = 1;
    bool shadowPending = false;   // a shadow stage on stream3 the main stream has not waited for yet (JoinShadow)
    int *stackSpill2 = nullptr;   // the spill rows of the walk on stream3 (stackSpill's size; allocated when the scene qualifies: FrameOverlapOk)
    int32_t *deferQShadow = nullptr;   // ... and its hand-over list of the two-class walk (ws.deferQ is the closest-hit side's)
    // WF_SAMPLES_SHADED (default 1; 0: at every depth, as the stand-alone entry point): the fused pass draws no ray samples at the last
    // depth, where it leaves before the material stage that would read them (scenes without media and subsurface)
    bool samplesShaded = true;
    bool cursorDirty[2] = {false, false};   // the closest-hit / any-hit work cursor has been used since a k_reset last zeroed it
    ScenePlan plan;              // what the uploaded scene runs: written by PlanScene, read by PickWalkKernels / PickStageKernels, the launch sites and wf_queues_alloc
    WalkKernels walk;
    StageKernels stage;
    StageGrids grids;            // written by PickStageGrids behind PickStageKernels, read by StageGridOf at the launch sites
    // The scratch of wf_trace_shadow_tr_device: the packed shadow-queue items of the call (k_pack_shadow_items), its counter block and —
    // on a scene whose plan routes transmittance through the wavefront (plan.trRoute == 2) — the wavefront's per-item state, index
    // queues and hit records: a call's n has nothing to do with the render's queue size, and the call works without wf_queues_alloc, so
    // it borrows none of ctx->ws's arrays.  Owned by the context and grown geometrically (GrowTrScratch: the only place a call may
    // synchronise or allocate), freed in DestroyCtx.  The next call overwrites it without waiting: every launch that reads it is on the
    // context's in-order stream, ahead of the pack kernel that rewrites it.
    struct TrScratch {
        F4 *o = nullptr, *d = nullptr, *lambdaPdf = nullptr;
        float *pathTime = nullptr;
        F4 *trO = nullptr, *trD = nullptr, *trT = nullptr, *trRu = nullptr, *trRl = nullptr, *hit = nullptr;   // (the wavefront's: null on the other routes)
        I4 *trRng = nullptr;
        int32_t *trQ[2] = {nullptr, nullptr}, *hitInst = nullptr;
        int32_t *counters = nullptr;
        size_t capacity = 0;   // items
        // every per-item array with its element size (the counter block is not one of them)
        struct Slot { void **p; size_t elem; bool wavefront; };
        std::vector<Slot> slots() {
            return {{(void **)&o, sizeof(F4), false}, {(void **)&d, sizeof(F4), false}, {(void **)&lambdaPdf, sizeof(F4), false}, {(void **)&pathTime, sizeof(float), false},
                    {(void **)&trO, sizeof(F4), true}, {(void **)&trD, sizeof(F4), true}, {(void **)&trT, sizeof(F4), true}, {(void **)&trRu, sizeof(F4), true},
                    {(void **)&trRl, sizeof(F4), true}, {(void **)&hit, sizeof(F4), true}, {(void **)&trRng, sizeof(I4), true},
                    {(void **)&trQ[0], sizeof(int32_t), true}, {(void **)&trQ[1], sizeof(int32_t), true}, {(void **)&hitInst, sizeof(int32_t), true}};
        }
    } trScratch;
    int32_t *probeCursor = nullptr;
    unsigned long long *developNaN = nullptr;   // wf_film_develop_*_device's NaN counter (allocated by the first call that asks for the count)
    int32_t *filmStamps = nullptr;   // wf_film_add_samples_device: per film pixel, the epoch of the last call that added to it (allocated by the scene's first call)
    int32_t filmEpoch = 0;           // ... the last call's epoch, 1 .. INT32_MAX (then the stamps are zeroed and the epochs start over)
    int32_t *bsdfRoute = nullptr;    // wf_bsdf_make_device: per row, the material the routing pass resolved (-1: no BSDF), read by the types' launches of the same call
    size_t bsdfRouteCap = 0;         // ... its rows (grown by doubling; an outgrown array stays in `allocs`: launches in flight may still read it)
    int W = 0, H = 0;
    int maxDepth = 5;
    float sceneBounds[6] = {};
    bool sceneLoaded = false, queuesAllocated = false;
    // profiling (gpu/util.cpp:136-209)
    int profile = 0;             // 0 off, 1 every launch, 2 traversal kernels only
    struct Ev { std::string name; hipEvent_t a, b; };
    std::vector<Ev> events;
    std::vector<hipEvent_t> eventPool;
    int passY0 = INT_MIN;        // first scanline of the band of the last wf_gen_camera_rays
    int passStep = 1, passSamples = 1;  // wf_set_pass_samples: sample-index stride and sample slots used by the current pass
    bool pixelMajor = true;      // items of a pass ordered pixel by pixel (WorkState::slotStride); WF_PIXEL_MAJOR=0: sample by sample
    bool countTraversal = false;
    bool traceLaunch = false;    // WF_TRACE_LAUNCH=1: print every launch and synchronise after it (debugging)
};

template <typename T>
int devAlloc(wf_ctx *c, T **p, size_t n) {
    void *d = nullptr;
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    HIPCHK(hipMalloc(&d, bytes));
    c->allocs.push_back(d);
    HIPCHK(hipMemsetAsync(d, 0, bytes, c->stream));
    *p = (T *)d;
    return 0;
}
template <typename T>
int devUpload(wf_ctx *c, const T **p, const T *src, size_t n) {
    T *d = nullptr;
    if (int e = devAlloc(c, &d, n)) return e;
    if (n && src) HIPCHK(hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *p = d;
    return 0;
}

template <typename T>
int devUpload(wf_ctx *c, wf::GPtr<const T> *p, const T *src, size_t n) {   // (a SceneView table pointer, wf_scene.h)
    const T *d = nullptr;
    if (int e = devUpload(c, &d, src, n)) return e;
    *p = d;
    return 0;
}

// The device scratch of one boundary call (wf_trace_*_host, the probes): freed when the call returns, on whichever path.
struct DeviceScratch {
    hipStream_t stream;
    std::vector<void *> ptrs;
    explicit DeviceScratch(hipStream_t s) : stream(s) {}
    DeviceScratch(const DeviceScratch &) = delete;
    DeviceScratch &operator=(const DeviceScratch &) = delete;
    ~DeviceScratch() { for (void *p : ptrs) (void)hipFree(p); }   // (hipFree waits for the work that uses the memory)
    template <typename T>
    int alloc(T **dst, size_t n) {
        void *p = nullptr;
        HIPCHK(hipMalloc(&p, n * sizeof(T)));
        ptrs.push_back(p);
        *dst = (T *)p;
        return 0;
    }
    template <typename T>
    int zeroed(T **dst, size_t n) {
        if (int e = alloc(dst, n)) return e;
        HIPCHK(hipMemsetAsync(*dst, 0, n * sizeof(T), stream));
        return 0;
    }
    template <typename T, typename S>
    int upload(T **dst, const S *src, size_t n) {   // n elements of T from src (S: T, or void for a caller's untyped array)
        if (int e = alloc(dst, n)) return e;
        HIPCHK(hipMemcpyAsync(*dst, src, n * sizeof(T), hipMemcpyHostToDevice, stream));
        return 0;
    }
};
// n rays as the trace kernels read them: (o, d, tmax), seven floats each
inline std::vector<float> PackRays7(const float *o, const float *d, const float *tmax, int n) {
    std::vector<float> rays((size_t)n * 7);
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) { rays[(size_t)i * 7 + k] = o[3 * i + k]; rays[(size_t)i * 7 + 3 + k] = d[3 * i + k]; }
        rays[(size_t)i * 7 + 6] = tmax[i];
    }
    return rays;
}

// the `mode` argument of k_trace_closest (StageKernels::traceClosestRef)
// mode & TRACE_ONLY_MARKED: the re-trace pass after k_trace_closest_fast — only the records it marked as near-ties (nodes_visited == -1)
// mode & TRACE_NO_COUNTS: nodes_visited / tris_tested = 0 (the records of the device-buffer calls with times carry none, on any walk)
constexpr int TRACE_ONLY_MARKED = 1, TRACE_NO_COUNTS = 2;

// ---------------------------------------------------------------------------------------------
// launches
inline int gridFor(int n) {
    int g = (n + BLOCK - 1) / BLOCK;
    if (g < 1) g = 1;
    return g > MAX_GRID ? MAX_GRID : g;
}

struct Prof {
    wf_ctx *c;
    hipEvent_t a = nullptr, b = nullptr;
    const char *name;
    bool on;
    hipStream_t s;
    Prof(wf_ctx *c, const char *name, hipStream_t onStream = nullptr) : c(c), name(name), s(onStream ? onStream : c->stream) {
        if (c->traceLaunch) { fprintf(stderr, "[wf] launch %s\n", name); fflush(stderr); }
        on = c->profile == 1 || (c->profile == 2 && (strncmp(name, "Intersect", 9) == 0 || strcmp(name, "Route hits") == 0 || strstr(name, "Material") != nullptr ||
                                                      strncmp(name, "Sample medium", 13) == 0));   // (2: the stages bench.py prices against a roofline)
        if (!on) return;
        auto get = [&]() {
            hipEvent_t e;
            if (!c->eventPool.empty()) { e = c->eventPool.back(); c->eventPool.pop_back(); }
            else (void)hipEventCreate(&e);
            return e;
        };
        a = get(); b = get();
        (void)hipEventRecord(a, s);
    }
    ~Prof() {
        if (c->traceLaunch) {
            hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) { fprintf(stderr, "[wf] %s: %s\n", name, hipGetErrorString(e)); fflush(stderr); }
        }
        if (!on) return;
        (void)hipEventRecord(b, s);
        c->events.push_back({name, a, b});
    }
};

// (the _ON forms name the stream: the shadow stage of the fused pass runs on ctx->stream3, and its HIP-event times are taken there;
//  LAUNCHB_ON names the workgroup's threads too)
#define LAUNCHB_ON(strm, name, kernel, grid, block, ...)                                   \
    do {                                                                                   \
        Prof prof_(ctx, name, strm);                                                       \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, strm, __VA_ARGS__);         \
    } while (0)
#define LAUNCH_ON(strm, name, kernel, grid, ...) LAUNCHB_ON(strm, name, kernel, grid, BLOCK, __VA_ARGS__)
#define LAUNCH(name, kernel, grid, ...) LAUNCH_ON(ctx->stream, name, kernel, grid, __VA_ARGS__)
// a walk kernel (workgroups of TBLOCK threads), usually one of ctx->walk on its resident grid
#define LAUNCHT_ON(strm, name, kernel, grid, ...) LAUNCHB_ON(strm, name, kernel, grid, TBLOCK, __VA_ARGS__)
#define LAUNCHT(name, kernel, grid, ...) LAUNCHT_ON(ctx->stream, name, kernel, grid, __VA_ARGS__)

// wf_render_stats carries 64 per-depth slots (indirect_rays[64], shadow_rays[64]); deeper bounces (volumetric scenes
// set maxdepth 100 and more) accumulate in the last slot instead of running past the array
inline int statDepth(int depth) { return depth < STAT_DEPTHS - 1 ? depth : STAT_DEPTHS - 1; }

// HIP's current device is a property of the calling host thread: a context may be driven from any thread (pbrt_amd --gpus N runs one
// host thread per device, SURVEY 8(b) "multi-GPU = one host thread per device"), so every stage entry makes the context's device current
// — unconditionally: other entry points of this library (wf_ctx_create, wf_build_bvh_sah, ...) and the application itself (torch in the
// same thread) change the current device too, so a cached "current" would go stale; hipSetDevice on the current device is a TLS write
inline void useDevice(const wf_ctx *ctx) { (void)hipSetDevice(ctx->device); }
inline int checkReady(wf_ctx *ctx) {
    if (!ctx) return fail(-1, "null context");
    if (!ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    if (!ctx->queuesAllocated) return fail(-1, "queues not allocated (wf_queues_alloc)");
    useDevice(ctx);
    return 0;
}
inline bool Aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// ---------------------------------------------------------------------------------------------
// What wf_boundary.hip calls of wf_backend.hip, where these are defined beside the render's own use of them
namespace wf::backend {
// the band's camera rays into the ray queue; countStats = false (wf_camera_rays_device): the rays are a caller's, not the render's
int GenCameraRays(wf_ctx *ctx, int y0, int sample_index, bool countStats);
// the transmittance stage's launches over `ws` (n items) by `route` (ScenePlan::trRoute), under the caller's launch names
struct TrNames { const char *reset, *begin, *trace, *segment, *rest, *perLane; };
void LaunchTransmittance(wf_ctx *ctx, const WorkState &ws, int n, int route, bool timed, const TrNames &names);
}  // namespace wf::backend
using namespace wf::backend;
