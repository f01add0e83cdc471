// wf_backend.hip — libwfhip.so: the HIP/CDNA4 (gfx950) back end behind include/wf_abi.h.
//
// What the reference does with one generic kernel template instantiated per lambda (gpu/util.h:77-114)
// plus OptiX programs (gpu/optix/optix.cu), this file does with named, hand-written kernels:
//   k_gen_camera_rays / k_gen_ray_samples / k_handle_escaped / k_handle_emissive / k_mat_shade<M> / k_mat_nee<M> /
//   k_update_film            grid-stride "for all queued" kernels (sizes are read on the device; the host
//                            never reads a queue size, as in wavefront/workqueue.h:118-137)
//   k_intersect_closest      BVH closest hit, replaces OptiX __raygen__findClosest + closest-hit programs
//   k_intersect_shadow       BVH any hit + RecordShadowRayResult, replaces __raygen__shadow
//   k_reset                  the one-thread "Reset queues" / stats kernels of integrator.cpp:357-397
// Traversal keeps the node stack in LDS (one column per lane, STACK_LDS entries; deeper levels spill to a
// per-lane HBM column) — no private-memory (scratch) arrays anywhere in the hot loop.
// Queue pushes are wave-aggregated (wf_kernels.h: QueueAlloc): one atomic per wave per destination queue.
//
// The library's host-only part — the environment switches, the scene's plan, the builder of the production traversal layout and its
// self-check — is plain C++ beside this unit: wf_plan.h, wf_plan.cpp, wf_fastbvh_build.cpp.  The context and the launch plumbing are
// wf_ctx.h, shared with the units that hold the rest of the C ABI and no kernel of the render: wf_boundary.hip (the boundary calls),
// wf_results.hip (what a caller reads back) and wf_probe.hip (the tests' probe kernels).  This unit is the render: every kernel of it and
// of the boundary's walks, PickWalkKernels / PickStageKernels / PickStageGrids, the context's life, the uploads, the stage entry points
// and the render pass.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (the only fused operations are the explicit
// fma calls of the restated arithmetic, as in the reference's CPU build).
#include "wf_ctx.h"
// FRAME SCHEDULING: the scenes whose shadow stage may run beside the next depth (the part of the condition that is fixed at upload).
// Media and subsurface scenes stay serial: the transmittance walk and the second shadow stage after SampleSubsurface share more state
// (the transmittance queues; ws.sq refilled between the two stages).  Scenes with animated primitives too: their closest-hit walk
// stores the path's time (ws.pathTime) that the any-hit walk's rays read.  The reference-order walks (!fastOk) are not worth it.
static bool FrameOverlapScene(const wf_ctx *ctx) {
    return ctx->frameOverlap > 0 && ctx->plan.fastOk && !ctx->svHost.haveMedia && !ctx->svHost.haveSubsurface && !ctx->svHost.haveAnimated;
}
// ... and the context has the second set of spill rows that walk needs (a profiling / tracing / counting pass is serial all the same)
static bool FrameOverlapActive(const wf_ctx *ctx) { return FrameOverlapScene(ctx) && ctx->stackSpill2 != nullptr; }
// The fused pass draws no ray samples at the last depth, where it leaves before the material stage, their only reader (media and
// subsurface scenes keep the launch: their scatter stages are not that loop's material stage)
static bool SkipLastSamples(const wf_ctx *ctx) { return ctx->samplesShaded && !ctx->svHost.haveMedia && !ctx->svHost.haveSubsurface; }
constexpr int FRAME_OVERLAP_THIN_DEPTH = 2;   // WF_FRAME_OVERLAP=2: the depths from here on (8 % of the spec scene's rays) are the "thin" ones

// ---------------------------------------------------------------------------------------------
// kernels
// Round 4: a kernel may read the scene view through the pointer to its device-resident copy (sv.self) instead of from its by-value
// argument — what took 100 spilled SGPRs out of the material kernels (wf_mat.hip, WF_MAT_SV_PTR).  Measured per kernel on the spec scene
// (gpurun_out/r04ad, 16 spp, same box): camera rays 4.03 -> 3.32 ms, route hits 1.81 -> 1.71; closest-hit 36.8 -> 39.0 (worse: it hardly
// touches the view, and the indirection costs), escaped 3.02 -> 3.16, the others unchanged — so only the first two use it.
template <bool VIA_SELF>
__device__ inline const SceneView &SvOf(const SceneView &a) { return VIA_SELF ? *a.self : a; }
__global__ void __launch_bounds__(BLOCK) k_reset(WorkState ws, unsigned mask, int statSlot, int statCounter) {
    // mask bit i: zero counters[(i) * CNT_STRIDE].  statSlot >= 0: stats[statSlot] += counters[(statCounter) * CNT_STRIDE] first.
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (statSlot >= 0) ws.stats[statSlot] += (unsigned long long)ws.counters[(statCounter) * CNT_STRIDE];
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x < CNT_COUNT && ((mask >> threadIdx.x) & 1u)) {
        // the items a material queue held go to stats[STAT_ITEMS + type] before the counter is zeroed (wf_material_items_download: the item
        // counts of the material stage's roofline) — the same for the medium-sample queue at stats[STAT_ITEMS + WF_MAT_NTYPES]
        const int t = (int)threadIdx.x;
        if (t >= CNT_MAT0 && t <= CNT_MEDIUM_SAMPLE) ws.stats[STAT_ITEMS + (t - CNT_MAT0)] += (unsigned long long)ws.counters[t * CNT_STRIDE];
        ws.counters[t * CNT_STRIDE] = 0;
    }
}

__global__ void __launch_bounds__(BLOCK) k_sample_tops(const SceneView svArg, WorkState ws, int y0, int dim0) {
    const SceneView &sv = SvOf<false>(svArg);
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < 5 * ws.pixelsPerPass; i += gridDim.x * BLOCK) KSampleTops(sv, ws, i, y0, dim0);
}
// ANIM: the instance for a moving camera (AnimatedTransform::Interpolate per ray); scenes with a static camera launch the other one
template <bool ANIM>
__global__ void __launch_bounds__(BLOCK) k_gen_camera_rays(const SceneView svArg, WorkState ws, int y0, int sampleBase, int sampleStep, int nSamples) {
    const SceneView &sv = SvOf<true>(svArg);
    if (sv.camera.type != WF_CAMERA_REALISTIC && blockIdx.x == 0 && threadIdx.x == 0) ws.counters[(CNT_RAY0) * CNT_STRIDE] = KCameraRayCount(sv, ws, y0, nSamples);
    const bool useTops = ws.sampleTops != nullptr;
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < ws.maxQueueSize; i += gridDim.x * BLOCK)
        KGenerateCameraRay<ANIM>(sv, ws, i, y0, sampleBase, sampleStep, nSamples, useTops);
}

__global__ void __launch_bounds__(BLOCK) k_gen_ray_samples(const SceneView svArg, WorkState ws, int cur, int sampleBase, int sampleStep, int topsDepth) {
    const SceneView &sv = SvOf<false>(svArg);
    const int n = ws.counters[(CNT_RAY0 + cur) * CNT_STRIDE];
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) KGenerateRaySamples(sv, ws, cur, i, sampleBase, sampleStep, topsDepth);
}

// LDS short stack with HBM spill: one column per lane ([entry][lane] so a wave's same-depth accesses hit
// 64 consecutive banks).  The array lives at file scope so every access is a ds_read/ds_write (LDS address
// space), never a flat access.
__shared__ int g_sstack[STACK_LDS * BLOCK];
struct LdsStack {
    int *spill;   // &stackSpill[global thread], stride = total threads
    int spillStride;
    int n;
    // always inline: the three-level walks of the ANIM kernels have enough call sites for the inliner to leave push / pop out of line, and an
    // out-of-line function that touches g_sstack moves EVERY LDS array of the unit that such functions reach (g_tstack: LdsStackT::push) from a
    // fixed address to a per-kernel table look-up — in the static scenes' kernels too
    __device__ __forceinline__ void push(int v) {
        if (n < STACK_LDS) g_sstack[n * BLOCK + threadIdx.x] = v;
        else spill[(size_t)(n - STACK_LDS) * spillStride] = v;
        ++n;
    }
    __device__ __forceinline__ int pop() {
        --n;
        int v = g_sstack[(n < STACK_LDS ? n : 0) * BLOCK + threadIdx.x];  // always a ds_read
        if (__builtin_expect(n >= STACK_LDS, 0)) v = spill[(size_t)(n - STACK_LDS) * spillStride];
        return v;
    }
    __device__ bool empty() const { return n == 0; }
};

__device__ inline unsigned long long waveSum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// ANIM: the scene has animated shapes / instances (AnimatedPrimitive, round 5): the walk interpolates their transformation at the ray's time.
// Such scenes are walked by these reference-order kernels only (no production tree: ctx->plan.fastOk is false for them).
template <bool COUNT, bool ANIM = false>
__global__ void __launch_bounds__(BLOCK) k_intersect_closest(const SceneView sv, WorkState ws, int cur, int *stackSpill) {
    const int n = ws.counters[(CNT_RAY0 + cur) * CNT_STRIDE];
    const int gtid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
    LdsStack st{stackSpill + gtid, stride, 0};
    unsigned long long nv = 0, nt = 0, nh = 0, nr = 0;
    for (int i = gtid; i < n; i += stride) {
        F4 o = ws.rq[cur].o[i], d = ws.rq[cur].d[i];
        // the path's time, for the shadow rays this depth spawns (a subsurface exit continues at time 0: subsurface.cpp:70)
        if (ANIM) ws.pathTime[ws.rq[cur].meta[i].x] = o.w;
        ClosestHit ch;
        st.n = 0;
        bool found = BVHIntersectClosest<ANIM>(sv, V3{o.x, o.y, o.z}, V3{d.x, d.y, d.z}, WF_INFINITY, st, &ch, o.w);
        KAfterClosestHit<ANIM>(sv, ws, cur, i, found, ch.prim, ch.inst, ch.h.t, ch.h.b0, ch.h.b1, ch.h.b2);
        if (COUNT) { nv += ch.nodesVisited; nt += ch.trisTested; nh += found; nr += 1; }
    }
    if (COUNT) {
        nv = waveSum(nv); nt = waveSum(nt); nh = waveSum(nh); nr = waveSum(nr);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&ws.trav[0], nr); atomicAdd(&ws.trav[1], nv); atomicAdd(&ws.trav[2], nt); atomicAdd(&ws.trav[3], nh);
        }
    }
}

template <bool COUNT, bool ANIM = false>
__global__ void __launch_bounds__(BLOCK) k_intersect_shadow(const SceneView sv, WorkState ws, int *stackSpill) {
    const int n = ws.counters[(CNT_SHADOW) * CNT_STRIDE];
    const int gtid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
    LdsStack st{stackSpill + gtid, stride, 0};
    unsigned long long nv = 0, nt = 0, nu = 0, nr = 0;
    for (int i = gtid; i < n; i += stride) {
        F4 o = ws.sq.o[i], d = ws.sq.d[i];
        int v = 0, t = 0;
        st.n = 0;
        const float time = ShadowTime<ANIM>(ws, d.w);
        bool occluded = BVHIntersectAny<ANIM>(sv, V3{o.x, o.y, o.z}, V3{d.x, d.y, d.z}, o.w, st, &v, &t, time);
        KRecordShadowRay(ws, i, occluded);
        if (COUNT) { nv += v; nt += t; nu += !occluded; nr += 1; }
    }
    if (COUNT) {
        nv = waveSum(nv); nt = waveSum(nt); nu = waveSum(nu); nr = waveSum(nr);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&ws.trav[4], nr); atomicAdd(&ws.trav[5], nv); atomicAdd(&ws.trav[6], nt); atomicAdd(&ws.trav[7], nu);
        }
    }
}

// ---- production traversal: persistent waves over QNode/LeafTri (wf_traverse.h) ----
__shared__ int g_tstack[TSTACK * TBLOCK];
// the render-space ray of every lane (o.xyz, d.xyz), for the instance transitions and the alpha test of the two-level / general
// variants: re-reading it from the queue (round 2) put an L2 round trip in front of every transition — eight per ray on the spec scene
__shared__ float g_ray[6 * TBLOCK];
__device__ inline void StoreWorldRay(V3 o, V3 d) {
    g_ray[0 * TBLOCK + threadIdx.x] = o.x; g_ray[1 * TBLOCK + threadIdx.x] = o.y; g_ray[2 * TBLOCK + threadIdx.x] = o.z;
    g_ray[3 * TBLOCK + threadIdx.x] = d.x; g_ray[4 * TBLOCK + threadIdx.x] = d.y; g_ray[5 * TBLOCK + threadIdx.x] = d.z;
}
// the ray's time, for the kernels of scenes with animated primitives (written by their fetch functors, read at instance entries)
__shared__ float g_time[TBLOCK];
__device__ inline V3 WorldRayO() { return V3{g_ray[0 * TBLOCK + threadIdx.x], g_ray[1 * TBLOCK + threadIdx.x], g_ray[2 * TBLOCK + threadIdx.x]}; }
__device__ inline V3 WorldRayD() { return V3{g_ray[3 * TBLOCK + threadIdx.x], g_ray[4 * TBLOCK + threadIdx.x], g_ray[5 * TBLOCK + threadIdx.x]}; }
// the HBM spill path of the stack is out of line so that the compiler cannot merge it with the LDS path
// into a pointer select (which turns every pop into a flat load)
__device__ __attribute__((noinline)) int SpillRead(const int *p) { return *p; }
__device__ __attribute__((noinline)) void SpillWrite(int *p, int v) { *p = v; }
// The node stack of the production walk: a ring of TSTACK entries per lane in LDS holding the NEWEST entries; when it is full the
// OLDEST entry moves to the lane's HBM column (round 3).  Until round 2 the entries above TSTACK went to HBM instead: a walk deep in
// a two-level tree (20-30 entries) then paid an HBM store and an HBM load on nearly every push / pop — rocprofv3 WRITE_SIZE showed
// 230 B per closest-hit ray and 394 B per shadow ray for kernels whose results are 28 B and 16 B.  With the bottom of the stack
// spilled, an entry crosses the LDS / HBM boundary at most once in each direction, and the entries that do are the ones pushed near
// the root, which are popped last.
// dbg (null = off): [0] += entries spilled, [1] |= 1 when a push would have run past the lane's spill rows (the entry is dropped and
// wf_sync reports the overflow: ADVICE r2, "the traversal spill stack can overflow on unbalanced trees").
struct LdsStackT {
    int *spill;   // &stackSpill[global thread], stride = total threads
    int spillStride;
    int n;        // entries on the stack
    int lo;       // entries [0, lo) are in the HBM column, [lo, n) in the LDS ring (n - lo <= TSTACK)
    int rows;     // capacity of the HBM column
    int *dbg;
    static constexpr int MASK = TSTACK - 1;
    static_assert((TSTACK & (TSTACK - 1)) == 0, "WF_TSTACK must be a power of two (ring indexing)");
    __device__ void reset() { n = 0; lo = 0; }
    __device__ void push(int v) {
        if (__builtin_expect(n - lo == TSTACK, 0)) {
            if (__builtin_expect(lo >= rows, 0)) { if (dbg) atomicOr(dbg + 1, 1); return; }
            SpillWrite(&spill[(size_t)lo * spillStride], g_tstack[(lo & MASK) * TBLOCK + threadIdx.x]);
            if (dbg) atomicAdd(dbg, 1);
            ++lo;
        }
        g_tstack[(n & MASK) * TBLOCK + threadIdx.x] = v;
        ++n;
    }
    __device__ int pop() {
        --n;
        int v = g_tstack[(n & MASK) * TBLOCK + threadIdx.x];  // always a ds_read
        if (__builtin_expect(n < lo, 0)) { lo = n; v = SpillRead(&spill[(size_t)n * spillStride]); }
        return v;
    }
    __device__ bool empty() const { return n == 0; }
};

// a node's 16-byte words: a plain global load.  (Rounds 1-5 copied the top of the tree into LDS per workgroup, and a node was then fetched
// through a pointer into either LDS or global memory, which the compiler can only issue as FLAT loads.  Measured and dropped in round 6:
// closest-hit 31.3 -> 28.4 ms, any-hit 13.5 -> 12.5 ms per 16 spp on the spec scene, profiles/r06_tree_top_global_loads_and_knobs_ab_sm16.txt.)
__device__ inline void FetchNode(const FastBVH &bvh, int node, U4 *n) {
    const U4 *p = reinterpret_cast<const U4 *>(bvh.nodes + node);
    for (int k = 0; k < QNODE_U4; ++k) n[k] = p[k];
}

// One batch of TBLOCK rays per workgroup iteration: ray index = thread index within the batch (no cursor
// atomic).  Waves walk independently ("while-while": all lanes descend interior nodes until every one of
// them sits at a leaf or is done, then the leaves are processed together); `finish` runs once per batch for
// the whole workgroup, so its queue pushes are block-aggregated (BlockAlloc).
// what the general-primitive traversal variants call back into (wf_traverse.h LeafStep): the alpha test and the spheres
// The general-primitive work of the traversal kernels comes in two strengths (template parameter GEN of the kernels):
//   GEN = 1  "simple alpha": every alpha texture of the scene is a constant, a uv-mapped image map (not EWA-filtered) or a bilerp
//            (no texture graph: EvalFloatTextureSimple) and there are no quadrics.  The test is a real call into a small out-of-line function
//            that reads the device-resident SceneView: the walk keeps its registers, the call is paid only when an
//            alpha-tested triangle is actually hit.  (Foliage cut-outs are image maps: this is the san-miguel case.)
//   GEN = 2  anything else (texture graphs as alpha, spheres / disks / cylinders): evaluated inline as before — an
//            out-of-line callee for the full texture graph needs 194 VGPRs, which would become the kernel's own count.
// The ray is NOT kept in registers for either: the origin of the space being walked is w.o, the direction is re-fetched
// from the queue (and taken into the instance's space) when such a primitive is hit.
__device__ __attribute__((noinline)) bool AlphaTestSimpleP(const SceneView *svp, int tri, float b0, float b1, float b2, float ox, float oy, float oz,
                                                            float dx, float dy, float dz) {
    // AlphaTestPasses (common/wf_shapes.h) for the alpha textures genMode 1 admits: a constant, or a uv-mapped bilerp / image map
    // looked up without a footprint.  The same arithmetic as EvalFloatTextureSimple on those inputs (UVMapping::Map, textures.h:76-98;
    // FloatImageTexture::Evaluate, FloatBilerpTexture::Evaluate), without the interaction point the other mappings need and without
    // the calls into the general filter: the test runs for every candidate hit of a cut-out triangle.
    const SceneView &sv = *svp;
    const wf_mesh &mesh = sv.meshes[sv.triMesh[tri]];
    if (mesh.alpha_tex < 0) return true;
    const wf_texture &t = sv.textures[mesh.alpha_tex];
    float a;
    if (t.type == WF_TEX_FLOAT_CONSTANT) a = t.f0;
    else {
        const auto v = sv.triIndices + 3 * (size_t)tri;
        V2 uv0{0, 0}, uv1{1, 0}, uv2{1, 1};
        if (mesh.flags & WF_MESH_HAS_UV) {
            if ((const ShadeTri *)sv.shadeTris != nullptr) {   // the triangle's de-indexed record (wf_scene.h): one 24-byte gather instead of an index triple + three
                const float *q = sv.shadeTris[tri].uv;
                uv0 = V2{q[0], q[1]}; uv1 = V2{q[2], q[3]}; uv2 = V2{q[4], q[5]};
            } else { uv0 = LoadUV(sv, v[0]); uv1 = LoadUV(sv, v[1]); uv2 = LoadUV(sv, v[2]); }
        }
        const V2 uv{b0 * uv0.x + b1 * uv1.x + b2 * uv2.x, b0 * uv0.y + b1 * uv1.y + b2 * uv2.y};
        const V2 st{t.map[0] * uv.x + t.map[2], t.map[1] * uv.y + t.map[3]};
        if (t.type == WF_TEX_FLOAT_IMAGE) {
            const float val = t.f0 * MIPFilterFloatZeroP(sv.tableData, sv.texImages + t.i0, st.x, 1 - st.y);
            a = t.f1 != 0 ? fmax(0.f, 1 - val) : val;
        } else {
            const float v00 = t.f0, v01 = t.f1, v10 = t.map[10], v11 = t.map[11];
            a = (1 - st.x) * (1 - st.y) * v00 + st.x * (1 - st.y) * v10 + (1 - st.x) * st.y * v01 + st.x * st.y * v11;
        }
    }
    if (!(a < 1)) return true;
    float u = (a <= 0) ? 1.f : HashToFloat(Hash6f(V3{ox, oy, oz}, V3{dx, dy, dz}));
    return !(u > a);
}
// ---- TWO-CLASS TRAVERSAL (round 6) ----------------------------------------------------------------------------------------------
// Until round 5 ONE quadric, patch or curve anywhere in a scene moved every ray onto the general-primitive walk kernels (GEN >= 2: the
// shape intersectors inline, 165-260 VGPRs, a separate near-tie re-trace launch): the 10 M-triangle scene plus one sphere rendered 1.56x
// slower.  Now the triangle kernels (GEN 0 / 1) walk such a scene first in their DEFER variants (template value 4 + GEN): a walk that
// meets a leaf entry of the other class (LeafTri c.z == 3) stops and hands its ray to `deferQ`; a second, small launch of the general
// kernel walks only those rays, from the start.  A ray that is not handed over never had such a primitive's leaf box within its
// pruning bound — a superset of the primitives that could have been its hit or a near-tie partner of its hit (the wide band of a pair
// that involves such a shape only matters to candidates NEARER than the triangle hit: wf_traverse.h) — so both classes of rays end
// with the result the general kernel alone computes.  The reference keeps such shapes in acceleration structures of their own too
// (gpu/optix/aggregate.cpp:916-1025: one GAS per shape class under the root IAS).
// (kernel template value = strength 0 .. 3 | 4: hands general primitives over | 8: ANIMATED instances, see EnterInstance<ANIM>)
constexpr int GenBase(int g) { return g & 3; }
constexpr bool GenDefer(int g) { return (g & 4) != 0; }
constexpr bool GenAnim(int g) { return (g & 8) != 0; }
constexpr int GenX(int gen, bool defer, bool anim) { return gen | (defer ? 4 : 0) | (anim ? 8 : 0); }   // (the host packs a template value here only: PickWalkKernels)
template <typename Fetch, int GEN, bool DEFER = false, bool ANIM = false>
struct GeneralPrims {
    static constexpr bool pairBands = GEN >= 2;   // quadrics / patches / curves in the scene: the near-tie band depends on the pair (wf_traverse.h)
    static constexpr bool deferGeneral = DEFER;
    const SceneView &sv;
    const FastBVH &bvh;
    const RayWalk &w;
    const Fetch &fetch;
    int idx;
    __device__ V3 dir() const {
        V3 d = WorldRayD();
        if (w.curInst >= 0) {
            wf_instance moving;
            d = XfVector3(InstanceAt<ANIM>(*bvh.sv, bvh.instances[w.curInst], g_time[threadIdx.x], &moving).render_from_instance.mInv, d);  // = InstanceRay's direction
        }
        return d;
    }
    __device__ bool accept(int prim, float b0, float b1, float b2) const {
        const V3 d = dir();
        if constexpr (GEN == 1) return AlphaTestSimpleP(bvh.sv, prim, b0, b1, b2, w.o.x, w.o.y, w.o.z, d.x, d.y, d.z);
        else return AlphaTestPasses(sv, prim, b0, b1, b2, w.o, d);
    }
    __device__ bool sphere(int prim, float tMax, QuadricHit *qh) const {
        if constexpr (GEN == 1) return false;
        else return QuadricIntersect<GEN == 3>(sv, prim, w.o, dir(), tMax, qh);
    }
};
struct DeferOnlyPrims {   // the triangle walk of a scene that also holds primitives of the other class
    static constexpr bool pairBands = false;
    static constexpr bool deferGeneral = true;
    __device__ bool accept(int, float, float, float) const { return true; }
    __device__ bool sphere(int, float, QuadricHit *) const { return false; }
};
// The part of a "while-while" iteration that follows the interior descent: every lane sits at a leaf run, at an instance transition
// (an instance entry popped from the stack, or the NODE_EXIT marker) or is done.  Leaves are processed first; the transitions —
// ~400 instructions each (the reference's interval-arithmetic ray transform, two WalkSetRay with three IEEE divisions each), eight
// per ray on the spec scene, about half of the walk's VALU work — are PARKED until WF_TRANS_BATCH lanes of the wave wait for one, or
// until no lane has anything else to do: a parked lane loses nothing (its wave-mates' steps would have been issued with its lane
// masked anyway), and the expensive code then runs with several times the lanes.  (0: run every transition in the iteration it is
// popped in, as in round 2.)
#ifndef WF_WALK_STATS
#define WF_WALK_STATS 0   // (diagnostic builds: WalkStats below)
#endif
#ifndef WF_TRANS_Q
#define WF_TRANS_Q 2   // spec scene, 16 spp, same box (profiles/r06_transition_parking_ab_sm16.txt): closest / any-hit 28.2 / 12.4 ms at 0, 27.6 / 12.1 at 2, 28.0 / 12.2 at 4
#endif
#ifndef WF_TRANS_BATCH
#define WF_TRANS_BATCH 6   // spec scene, 16 spp, same box (gpurun_out/r3f_ab_sm16.txt): closest / any-hit 60.1 / 22.0 ms at 0, 56.5 / 20.2 at 6, 58.4 / 20.5 at 12, 62.4 / 21.1 at 24
#endif
__device__ inline bool AtTransition(int node) { return node < 0 && node != NODE_NONE && (node == NODE_EXIT || (int)((~(unsigned)node) >> 4) >= INST_FIRST); }
template <bool ANY, int GENX, bool INST, typename Fetch>
__device__ inline int LeafPhase(const SceneView &sv, const FastBVH &bvh, RayWalk &w, LdsStackT &st, const Fetch &fetch, int idx) {
    constexpr int GEN = GenBase(GENX);
    constexpr bool DF = GenDefer(GENX), ANIM = GenAnim(GENX);
    if constexpr (INST) {
        bool tr = AtTransition(w.node);
        if (w.node < 0 && w.node != NODE_NONE && !tr) {   // (w.node >= 0: a lane the descent left at an interior node, WF_SCHED_Q)
            if constexpr (GEN > 0) LeafStep<ANY, true, true>(bvh, w, st, GeneralPrims<Fetch, GEN, DF, ANIM>{sv, bvh, w, fetch, idx});
            else if constexpr (DF) LeafStep<ANY, false, true>(bvh, w, st, DeferOnlyPrims{});
            else LeafStep<ANY, false, true>(bvh, w, st);
        }
        if constexpr (WF_TRANS_BATCH > 0) {
            tr = AtTransition(w.node);
            const int nT = __popcll(__ballot(tr));
            if (nT == 0) return 0;
#if WF_TRANS_Q > 0
            {
                // (round 6) ... and, like the descent (WalkDescend), until the lanes that wait for a transition are at least WF_TRANS_Q / 4 of
                // the lanes that have nodes and leaves to visit: the transition is the walk's most expensive code (~400 instructions)
                const int nO = __popcll(__ballot(w.node != NODE_NONE && !tr));
                if (nO > 0 && (nT < WF_TRANS_BATCH || 4 * nT < WF_TRANS_Q * nO)) return 0;
            }
#else
            if (nT < WF_TRANS_BATCH && __any(w.node != NODE_NONE && !tr)) return 0;   // parked: the others still have nodes and leaves to visit
#endif
        } else tr = AtTransition(w.node);
        if (tr) {
            const V3 o = WorldRayO(), d = WorldRayD();
            if (w.node == NODE_EXIT) ExitInstance(bvh, w, st, o, d);
            if (IsInstanceEntry(w.node)) EnterInstance<ANIM>(bvh, w, st, o, d, (int)((~(unsigned)w.node) >> 4) - INST_FIRST, ANIM ? g_time[threadIdx.x] : 0.f);   // (also the entry an exit has just popped)
        }
        return WF_WALK_STATS ? __popcll(__ballot(tr)) : 0;
    } else if (w.node < 0 && w.node != NODE_NONE) {
        if constexpr (GEN > 0) LeafStep<ANY, true>(bvh, w, st, GeneralPrims<Fetch, GEN, DF>{sv, bvh, w, fetch, idx});
        else if constexpr (DF) LeafStep<ANY, false, false>(bvh, w, st, DeferOnlyPrims{});
        else LeafStep<ANY>(bvh, w, st);
    }
    return 0;
}

// ---- near-tie resolution inside the production walk (round 3) -------------------------------------------------------------------
// A ray the production walk marked as a near-tie (wf_traverse.h) is walked once more in the REFERENCE's order — BVHAggregate::Intersect
// over the reference-layout 32-byte nodes (cpu/aggregates.cpp:529-579), the exact Bounds3::IntersectP, the reference's accept rule —
// starting from tMax = t* + twice the band instead of infinity (see k_closest_retrace).  Until round 2 this was a separate launch whose
// duration was the latency of its longest single walk on a 388-VGPR kernel (1.5-3 ms per depth on the 10 M-triangle scene: a tenth
// of the closest-hit stage); now the lane does it itself at the end of its batch, in this out-of-line function — triangles, simple
// alpha cut-outs and object instances only (the GEN <= 1 kernels; scenes with quadrics / curves / texture-graph alpha keep the second
// launch), so that it fits the walk's own register budget.  Cost: the few waves that hold a marked lane run one short walk at 1/64
// lane utilisation (a marked ray's bound is tight: it descends to its hit and little else).
struct RefHit { int prim, inst; float t, b0, b1, b2; uint32_t route; };
template <int GEN, bool TOP, bool ANIM = false>
__device__ inline __attribute__((always_inline)) bool RefOrderTree(const SceneView *svp, int root, V3 o, V3 d, float *tMaxIO, LdsStackT &st, RefHit *out, float time = 0) {
    const SceneView &sv = *svp;
    float tMax = *tMaxIO;
    bool hitAny = false;
    const int base = st.n;
    const V3 invDir{1 / d.x, 1 / d.y, 1 / d.z};
    const int negMask = int(invDir.x < 0) | (int(invDir.y < 0) << 1) | (int(invDir.z < 0) << 2);
    const RayShear sh = MakeRayShear(d);
    int cur = root;
    while (true) {
        const wf_bvh_node *node = &sv.bvhNodes[cur];
        if (BoxIntersectP(node->bmin, node->bmax, o, tMax, invDir, negMask)) {
            if (node->nprims > 0) {
                for (int i = 0; i < node->nprims; ++i) {
                    const int tri = sv.bvhPrims[node->offset + i];
                    if constexpr (TOP) {
                        if (tri >= sv.nTriangles + sv.nQuadrics) {  // TransformedPrimitive::Intersect (cpu/primitive.cpp:112-125)
                            const int inst = tri - sv.nTriangles - sv.nQuadrics;
                            wf_instance moving;
                            const wf_instance &in = InstanceAt<ANIM>(sv, sv.instances[inst], time, &moving);   // (AnimatedPrimitive::Intersect, cpu/primitive.cpp:140-153)
                            float tI = tMax;
                            V3 oI, dI;
                            InstanceRay(in, o, d, &tI, &oI, &dI);
                            if (RefOrderTree<GEN, false>(svp, sv.instanceDefs[in.def].bvh_root, oI, dI, &tI, st, out)) {
                                out->inst = inst;
                                tMax = tI;
                                hitAny = true;
                            }
                            continue;
                        }
                    }
                    // (a quadric / patch / curve — only in the scenes of the two-class traversal — cannot decide a near tie between the
                    //  triangles of a ray that was not handed to the general walk: it lies beyond their band)
                    if (tri >= sv.nTriangles) continue;
                    V3 p0, p1, p2;
                    TriVerts(sv, tri, &p0, &p1, &p2);
                    TriHit h;
                    if (IntersectTriangleSheared(o, sh, tMax, p0, p1, p2, &h, true)) {
                        if (GEN == 0 || AlphaTestSimpleP(svp, tri, h.b0, h.b1, h.b2, o.x, o.y, o.z, d.x, d.y, d.z)) {
                            out->prim = tri;
                            if (TOP) out->inst = -1;
                            out->t = h.t; out->b0 = h.b0; out->b1 = h.b1; out->b2 = h.b2;
                            tMax = h.t;
                            hitAny = true;
                        }
                    }
                }
                if (st.n == base) break;
                cur = st.pop();
            } else if ((negMask >> node->axis) & 1) {
                st.push(cur + 1);
                cur = node->offset;
            } else {
                st.push(node->offset);
                cur = cur + 1;
            }
        } else {
            if (st.n == base) break;
            cur = st.pop();
        }
    }
    *tMaxIO = tMax;
    return hitAny;
}
template <int GEN, bool ANIM = false>
__device__ inline __attribute__((always_inline)) RefHit RetraceRefOrder(const SceneView *svp, float ox, float oy, float oz, float dx, float dy, float dz, float tBound,
                                                           int *spill, int spillStride, int rows, int *dbg, float time = 0) {
    LdsStackT st{spill, spillStride, 0, 0, rows, dbg};
    RefHit out{-1, -1, 0, 0, 0, 0, 0};
    float tMax = tBound;
    RefOrderTree<GEN, true, ANIM>(svp, 0, V3{ox, oy, oz}, V3{dx, dy, dz}, &tMax, st, &out, time);
    if (out.prim >= 0) {
        // the routing code BuildFastBVH stores per LeafTri (EnqueueWorkAfterIntersection, intersect.h:48-156)
        const wf_mesh &mesh = svp->meshes[svp->triMesh[out.prim]];
        out.route = mesh.material >= 0 ? (uint32_t)svp->materials[mesh.material].type | (mesh.first_light >= 0 ? 16u : 0u) : 32u;
    }
    if (dbg) atomicAdd(dbg + 2, 1);
    return out;
}
// (which kernel variants resolve their near ties themselves: RetraceInline, wf_plan.h — the plan's transmittance route asks it too)

// -DWF_WALK_STATS (diagnostic builds only): per-phase counts of the closest-hit (slot 0) and any-hit (slot 1) production walks — how often a
// wave ran the interior step / the leaf step / an instance transition / a refill, and how many lanes were active each time — summed
// over the launch into 64-bit words behind the debug words (wf_sync prints them under WF_DEBUG_DRAIN).  What the round-6 scheduling
// decisions were checked against: profiles/r06_walk_phase_stats.txt.
struct WalkStats {
    unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // iterations / lanes of: interior, leaf, transition, refill
    __device__ void add(int phase, bool active) {
#if WF_WALK_STATS
        const int n = __popcll(__ballot(active));
        if (n) { c[2 * phase] += 1; c[2 * phase + 1] += (unsigned long long)n; }
#endif
    }
    __device__ void flush(int *dbg, int slot) {
#if WF_WALK_STATS
        if (dbg && (threadIdx.x & 63) == 0)
            for (int k = 0; k < 8; ++k) atomicAdd(reinterpret_cast<unsigned long long *>(dbg + 8) + slot * 8 + k, c[k]);
#endif
    }
};
// Does the wave take another interior step?  WF_SCHED_Q = 0: while ANY lane sits at an interior node (the "while-while" loop of rounds
// 1-5: the descent ends when its LAST lane has reached a leaf, the other lanes wait masked off).  WF_SCHED_Q = q > 0 (round 6): only while
// the lanes at interior nodes are at least q/4 of the lanes that wait at a leaf — otherwise the leaves are processed
// first and the few lanes still descending go on in the next round, together with the lanes whose leaves sent them back into the tree.
// Which lanes step when changes no result: every lane's own sequence of visits is the same.
#ifndef WF_SCHED_Q
#define WF_SCHED_Q 3   // spec scene, 16 spp, same box (profiles/r06_descent_scheduling_ab_sm16.txt): closest / any-hit 35.9 / 16.4 ms at 0, 31.5 / 13.4 at 2, 31.6 / 13.4 at 4, 31.9 / 13.8 at 8; second box (r06_tree_top_global_loads_and_knobs_ab_sm16.txt): 31.6 / 13.9 at 1, 31.0 / 13.4 at 3, 31.3 / 13.5 at 4
#endif
#ifndef WF_SCHED_Q_ANY
#define WF_SCHED_Q_ANY WF_SCHED_Q   // the any-hit walks' own threshold (measured: see DESIGN 4.1)
#endif
template <bool INST, bool ANY = false>
__device__ inline bool WalkDescend(const RayWalk &w) {
    constexpr int Q = ANY ? WF_SCHED_Q_ANY : WF_SCHED_Q;
    if constexpr (Q == 0) return __any(w.node >= 0);
    const int nI = __popcll(__ballot(w.node >= 0));
    if (nI == 0) return false;
    // (lanes at an instance transition do not count: LeafPhase may leave them parked, and a round must always make progress)
    const int nL = __popcll(__ballot(w.node < 0 && w.node != NODE_NONE && !(INST && AtTransition(w.node))));
    return 4 * nI >= Q * nL;
}
template <bool ANY, int GEN, bool INST = false, typename Fetch, typename Finish>
__device__ inline void BatchTrace(const SceneView &sv, const FastBVH &bvh, int n, LdsStackT &st, Fetch fetch, Finish finish, int *cursor = nullptr, int chunk = 4) {
    // cursor != nullptr (only when `finish` has no workgroup barrier): every wave takes its next `chunk` x 64 rays from a shared
    // cursor, so a wave with short walks serves more of the queue and the launch ends without a tail of waves that drew long ones
    // (one returning atomic per chunk x 64 rays: a counter sustains ~88 of them per microsecond)
    // (a queue shorter than two rounds of the resident grid is dealt statically: every wave starts at once, no atomics)
    if (n < 2 * (int)gridDim.x * TBLOCK) cursor = nullptr;
    if (cursor && st.dbg && threadIdx.x == 0 && blockIdx.x == 0) atomicOr(st.dbg + 3, 1);
    int chunkBase = 0, chunkSub = chunk;
    for (int base = blockIdx.x * TBLOCK; true; base += gridDim.x * TBLOCK) {
        int idx;
        if (cursor) {
            if (chunkSub == chunk) {
                int b = 0;
                if ((threadIdx.x & 63) == 0) b = atomicAdd(cursor, 64 * chunk);
                chunkBase = __shfl(b, 0);
                chunkSub = 0;
            }
            if (chunkBase + chunkSub * 64 >= n) break;
            idx = chunkBase + chunkSub * 64 + (threadIdx.x & 63);
            ++chunkSub;
        } else {
            if (base >= n) break;
            idx = base + threadIdx.x;
        }
        const bool valid = idx < n;
        RayWalk w;
        w.node = NODE_NONE;
        w.prim = -1;
        w.route = 0;
        w.tMax = 0;
        w.b0 = w.b1 = w.b2 = 0;
        w.inst = w.curInst = -1;
        if (valid) {
            V3 o, d;
            float tMax;
            fetch(idx, &o, &d, &tMax);
            WalkInit(bvh, w, o, d, tMax);
            if constexpr (INST || GEN > 0) StoreWorldRay(o, d);
            st.reset();
        }
        // (Measured and dropped: parking a lane's first leaf and descending on speculatively — 11 % slower; continuous
        // per-lane refill ("streaming": idle lanes take the next rays of the wave's run, leaf / interior step chosen per
        // iteration) — 28 % fewer VALU instructions at 53 % instead of 31 % active lanes, but 5x the vector-L1 line
        // accesses (7.2e8 vs 1.45e8 per 8.5 M-ray launch): lanes at unrelated depths of the tree no longer share
        // cache lines, and the walk becomes L1-bound: 33 ms vs 27 ms per 16 spp.  DESIGN.md §4.)
        while (__any(w.node != NODE_NONE)) {
            while (WalkDescend<INST, ANY>(w)) {
                if (w.node >= 0) {
                    U4 nd[QNODE_U4];
                    FetchNode(bvh, w.node, nd);
                    InteriorStep<!ANY>(bvh, w, st, nd);
                }
            }
            LeafPhase<ANY, GEN, INST>(sv, bvh, w, st, fetch, idx);
        }
        if constexpr (!ANY && RetraceInline(GenBase(GEN))) {
            static_assert(ANY || !GenDefer(GEN), "the inline re-walk's `w.route = rh.route` would drop WALK_DEFER: the handing-over variants must walk with BatchTraceRefill");
            if (valid && WalkAmbiguous(w)) {
                V3 o, d;
                float t0;
                fetch(idx, &o, &d, &t0);
                const float tB = __builtin_fminf(2 * WalkBound(bvh, WalkT(w)) - WalkT(w), t0);
                const RefHit rh = RetraceRefOrder<GenBase(GEN), GenAnim(GEN)>(bvh.sv, o.x, o.y, o.z, d.x, d.y, d.z, tB, st.spill, st.spillStride, st.rows, st.dbg, GenAnim(GEN) ? g_time[threadIdx.x] : 0.f);
                w.prim = rh.prim; w.inst = rh.inst; w.route = rh.route;
                w.tMax = rh.t; w.b0 = rh.b0; w.b1 = rh.b1; w.b2 = rh.b2;
            }
        }
        finish(idx, valid, w);
    }
}

// ---- the same walk with wave-level replacement of finished rays (round 3) ---------------------------------------------------------
// BatchTrace keeps a wave on its 64 rays until the LAST of them is done: on the 10 M-triangle scene the SQ counters showed 24 % of
// the lanes active over a wave's lifetime — walk lengths within a wave differ by an order of magnitude.  Here a wave whose active
// lanes drop to WF_REFILL_AT or fewer retires its finished lanes (`finish` is a per-lane store in every caller that uses this
// variant: no workgroup barrier) and deals them the next rays of the wave's private run of the queue (runs of chunk x 64 rays, taken
// from the shared cursor with one returning atomic each, or dealt statically when the queue is short).  Between refills the loop is
// the same "while-while" as before, so the lanes of one refill — neighbours in the queue — descend the top of the tree together
// (the same cache lines), which is what the continuous per-lane refill measured in round 2 lost (5x the L1 line accesses).
#ifndef WF_REFILL_AT
#define WF_REFILL_AT 40
#endif
#ifndef WF_GUIDED_CHUNK
#define WF_GUIDED_CHUNK 6   // 0: fixed runs of `chunk` x 64 rays; > 0: the any-hit walks take guided runs of at most this many x 64
#endif
#ifndef WF_GUIDED_DIV
#define WF_GUIDED_DIV 4
#endif
template <bool ANY, int GEN, bool INST = false, bool DRAIN = false, typename Fetch, typename Finish>
__device__ inline void BatchTraceRefill(const SceneView &sv, const FastBVH &bvh, int n, LdsStackT &st, Fetch fetch, Finish finish, int *cursor = nullptr, int chunk = 4,
                                        int workBlocks = 0) {
    if (workBlocks <= 0) workBlocks = (int)gridDim.x;   // (the first workBlocks workgroups of the grid walk rays; the rest, if any, have another job)
    if (n < 2 * workBlocks * TBLOCK) cursor = nullptr;
    if (cursor && st.dbg && threadIdx.x == 0 && blockIdx.x == 0) atomicOr(st.dbg + 3, 1);
    const int lane = threadIdx.x & 63;
    const int waveId = (blockIdx.x * TBLOCK + threadIdx.x) >> 6, nWaves = (workBlocks * TBLOCK) >> 6;
    const int runRays = cursor ? 64 * chunk : 64;
    int next = 0, end = 0, staticJ = 0;   // the wave's private run [next, end) of ray indices (uniform)
    int lastB = 0;                        // the cursor's value at the wave's last fetch (WF_GUIDED_CHUNK)
    bool exhausted = false;
    int idx = -1;
#if WF_WALK_ZERO
    RayWalk w{};
#else
    RayWalk w;
#endif
    w.node = NODE_NONE;
    w.prim = -1;
    w.route = 0;
    w.tMax = 0;
    w.b0 = w.b1 = w.b2 = 0;
    w.inst = w.curInst = -1;
    WalkStats ws_;
    auto retire = [&]() {
        // (a closest-hit walk here never re-walks a near tie itself: with DRAIN `finish` queues the ray and the kernel resolves it after its
        //  walks (DrainRetrace), otherwise the separate re-trace launch does.  The reference-order walk inlined HERE cost the closest-hit
        //  kernel 37 %: 76.9 vs 56.0 ms per 16 spp on the spec scene; without it the refill gains 28 %, 40.3 ms)
        finish(idx, true, w);
        idx = -1;
    };
    while (true) {
        const unsigned long long act = __ballot(w.node != NODE_NONE);
        const int nAct = __popcll(act);
        if (nAct <= WF_REFILL_AT && !exhausted) {
            const bool idle = w.node == NODE_NONE;
            if (idle && idx >= 0) retire();
            const int need = 64 - nAct;
            const int rank = __popcll(~act & ((1ull << lane) - 1ull));
            int served = 0;
            while (served < need) {
                if (next >= end) {
                    int b;
                    int rr = runRays;
                    if (cursor) {
#if WF_GUIDED_CHUNK
                        // guided self-scheduling (any-hit walks): long runs (neighbouring rays, refill after refill) while the queue is long,
                        // short ones towards its end, where a wave that still owns a long run would be the launch's tail.  Spec scene, 16 spp,
                        // same box, three runs (profiles/r06_guided_chunk_ab_sm16.txt): any-hit 12.2 -> 11.95 ms; the closest-hit walk
                        // LOSES with it (26.9 -> 28.4) and keeps its fixed runs of 3 x 64
                        // (triangle kernels only: with it k_shadow_fast<2, false> spilled an SGPR-spill carrier — tools/check_spill_carriers.py)
                        if constexpr (ANY && GenBase(GEN) <= 1) { int c = (n - lastB) / (nWaves * 64 * WF_GUIDED_DIV); c = c < 1 ? 1 : (c > WF_GUIDED_CHUNK ? WF_GUIDED_CHUNK : c); rr = 64 * c; }
#endif
                        b = 0;
                        if (lane == 0) b = atomicAdd(cursor, rr);
                        b = __builtin_amdgcn_readfirstlane(b);
                        lastB = b < n ? b : n;
                    } else {
                        b = (staticJ * nWaves + waveId) * 64;
                        ++staticJ;
                    }
                    next = b;
                    end = b + rr < n ? b + rr : n;
                    if (next >= n) { exhausted = true; break; }
                }
                const int take = need - served < end - next ? need - served : end - next;
                if (idle && rank >= served && rank < served + take) idx = next + (rank - served);
                next += take;
                served += take;
            }
            ws_.add(3, idle && idx >= 0);
            if (idle && idx >= 0) {
                V3 o, d;
                float tMax;
                fetch(idx, &o, &d, &tMax);
                WalkInit(bvh, w, o, d, tMax);
                if constexpr (INST || GEN > 0) StoreWorldRay(o, d);
                st.reset();
            }
            if (exhausted && !__any(w.node != NODE_NONE)) break;
        } else if (nAct == 0) break;
        while (WalkDescend<INST, ANY>(w)) {
            ws_.add(0, w.node >= 0);
            if (w.node >= 0) {
                U4 nd[QNODE_U4];
                FetchNode(bvh, w.node, nd);
                InteriorStep<!ANY>(bvh, w, st, nd);
            }
        }
        if constexpr (WF_WALK_STATS != 0) ws_.add(1, w.node < 0 && w.node != NODE_NONE && !(INST && AtTransition(w.node)));
        const int ranT = LeafPhase<ANY, GEN, INST>(sv, bvh, w, st, fetch, idx);
        if constexpr (WF_WALK_STATS != 0) { if (ranT) { ws_.c[4] += 1; ws_.c[5] += (unsigned long long)ranT; } }
    }
    ws_.flush(st.dbg, ANY ? 1 : 0);
    if (idx >= 0) retire();   // the rays still held when the queue ran out
}
// Which walk a launch takes (`finish` is a per-lane store in every caller: no workgroup barrier).  A walk whose near ties are resolved
// outside its loop walks with refill:
//   any-hit (no near ties): spec scene, 16 spp, same box (round 3): 30.1 -> 25.2 ms at a threshold of 40 lanes, 26.2 at 24, 27.5 at 12;
//   closest-hit with DRAIN (the caller queues near-tie rays in `finish` and drains the queue itself after this returns, DrainRetrace):
//   56.0 -> see DESIGN 4.1;
//   closest-hit of scenes with general primitives (GEN >= 2, whose near ties go to the separate re-trace launch): spec scene + one
//   sphere, 73.4 -> 64.6 ms (profiles/r04_one_sphere_refill_ab_sm16.txt).
// What remains — a closest-hit walk of triangles (GEN <= 1) whose caller does not drain: k_tr_trace, k_trace_closest_fast — walks with
// BatchTrace, which re-walks near ties inline.
template <bool ANY, int GEN, bool INST, bool DRAIN = false, typename Fetch, typename Finish>
__device__ inline void TraceQueue(const SceneView &sv, const FastBVH &bvh, int n, LdsStackT &st, Fetch fetch, Finish finish, int *cursor = nullptr, int chunk = 4,
                                  int workBlocks = 0) {
    if constexpr (ANY || DRAIN || !RetraceInline(GenBase(GEN))) BatchTraceRefill<ANY, GEN, INST, DRAIN>(sv, bvh, n, st, fetch, finish, cursor, chunk, workBlocks);
    else BatchTrace<ANY, GEN, INST>(sv, bvh, n, st, fetch, finish, cursor, chunk);
}
// The near-tie rays of a closest-hit launch, resolved inside the launch (round 3, second step).  A walk that ends on a near-tie publishes
// (ray index | starting bound) with ONE 64-bit atomic into retraceQ64 (slots are ~0 until written).  The reference-order walks of the
// queued rays are long single-lane walks (the old re-trace launch: 1.4-2 ms for its longest one), so they must run BESIDE the production
// walks, not after them: the last WF_SERVICE_BLOCKS workgroups of the grid walk no rays — they poll the queue (s_sleep between polls),
// take up to 64 entries per wave at a time, one walk per lane, until every worker wave has signed off and the queue is empty.  A worker
// wave that runs out of rays also takes what is queued at that moment before it signs off.  The wave that signs off last rewinds the
// counters for the next launch.  Nothing waits for a wave that is not resident: workers never wait, and the service workgroups occupy a
// fixed handful of slots.  (Grids too small to spare service workgroups: the worker that signs off last takes the rest.)
#ifndef WF_SERVICE_BLOCKS
#define WF_SERVICE_BLOCKS 16   // spec scene, 16 spp, same box: closest-hit 54.6 ms at 4, 48.0 at 8, 42.5 at 16, 44.4 at 32, 48.1 at 64 (gpurun_out/r3t_, r3u_ab_sm16.txt)
#endif
__device__ inline int ServiceBlocks() { return (int)gridDim.x >= 8 * WF_SERVICE_BLOCKS ? WF_SERVICE_BLOCKS : 0; }
template <int GEN, bool INST, bool ANIM = false>
__device__ inline void DrainRetrace(const SceneView &sv, const WorkState &ws, const FastBVH &bvh, int cur, LdsStackT &st, bool service) {
    int *cnt = ws.counters + CNT_RETRACE * CNT_STRIDE, *head = ws.counters + CNT_RETRACE_HEAD * CNT_STRIDE, *done = ws.counters + CNT_WAVES_DONE * CNT_STRIDE;
    const int lane = threadIdx.x & 63;
    const int totalWaves = (int)gridDim.x * (TBLOCK / 64), workerWaves = ((int)gridDim.x - ServiceBlocks()) * (TBLOCK / 64);
    const RayQueueV &q = ws.rq[cur];
    auto takeSome = [&]() -> bool {
        int base = 0, take = 0;
        if (lane == 0) {
            while (true) {
                const int h = __hip_atomic_load(head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), c = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (h >= c) break;
                const int t = c - h < 64 ? c - h : 64;
                if (atomicCAS(head, h, h + t) == h) { base = h; take = t; break; }
            }
        }
        base = __builtin_amdgcn_readfirstlane(base);
        take = __builtin_amdgcn_readfirstlane(take);
        if (take == 0) return false;
        if (lane < take) {
            // a slot is published when its tag is THIS launch's epoch (no sentinel to restore, nothing a stale slot could be mistaken for);
            // the bound lies in a word of its own, written before the tag (release) and read after it (acquire)
            unsigned long long e;
            while ((uint32_t)((e = __hip_atomic_load(&ws.retraceQ64[base + lane], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != (uint32_t)ws.drainEpoch) {}   // reserved, store in flight
            const int i = (int)(uint32_t)(e & 0xffffffffull);
            const float tB = BitsToFloat((uint32_t)__hip_atomic_load(&ws.retraceQ[base + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const F4 o = q.o[i], d = q.d[i];
            // A queued ray HAS a hit inside its bound (the production walk accepted one at t < tB with the same triangle and alpha tests), so a
            // re-walk that returns none is a fault, not an answer.  Round 3 measured exactly that on the 10 M-triangle scene: 2-6 of 4443
            // re-walks per frame came back empty in about half of the runs (gpurun_out/det3_sm16.txt; never with the re-walk inlined in the
            // worker, never once this check was compiled in) — a pixel sample lost per occurrence.  The walk is repeated; what it costs is
            // counted (dbg + 5), and a ray that stays without a hit raises wf_sync's error (dbg + 6) instead of a silently wrong pixel.
            RefHit rh;
            int tries = 0;
            do { rh = RetraceRefOrder<GEN, ANIM>(bvh.sv, o.x, o.y, o.z, d.x, d.y, d.z, tB, st.spill, st.spillStride, st.rows, st.dbg, o.w); } while (rh.prim < 0 && ++tries < 4);
            if (st.dbg && tries) { atomicAdd(st.dbg + 5, tries); if (rh.prim < 0) atomicOr(st.dbg + 6, 1); }
            // ... and the entry itself is validated instead of trusted: the ray index lies inside this launch's queue, the
            // re-walk's hit lies inside the entry's bound, and the slot still carries this launch's tag after the walk.  A violation is
            // wf_sync's error like an unresolved ray: wrong inputs that happen to yield SOME hit must not pass silently.
            if (st.dbg) {
                const bool badIndex = i < 0 || i >= ws.counters[(CNT_RAY0 + cur) * CNT_STRIDE];
                const bool badHit = rh.prim >= 0 && !(rh.t <= tB);
                const bool badTag = (uint32_t)(__hip_atomic_load(&ws.retraceQ64[base + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32) != (uint32_t)ws.drainEpoch;
                if (badIndex || badHit || badTag) atomicOr(st.dbg + 6, 2);
            }
            ws.routeCode[i] = rh.route;
            ws.hit[i] = F4{BitsToFloat((uint32_t)rh.prim), rh.b0, rh.b1, rh.b2};
            if (INST) ws.hitInst[i] = rh.prim >= 0 ? rh.inst : -1;
            if (sv.haveMedia) ws.hitT[i] = rh.prim >= 0 ? rh.t : WF_INFINITY;
        }
        return true;
    };
    auto signOff = [&]() -> int {
        int prev = 0;
        if (lane == 0) { __threadfence(); prev = atomicAdd(done, 1); }
        return __builtin_amdgcn_readfirstlane(prev);
    };
    bool last;
    if (!service) {
        while (takeSome()) {}
        last = signOff() == totalWaves - 1;   // (only without service workgroups can a worker be the last)
        if (last) while (takeSome()) {}
    } else {
        while (true) {
            if (takeSome()) continue;
            int dn = 0;
            if (lane == 0) dn = __hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            dn = __builtin_amdgcn_readfirstlane(dn);
            if (dn >= workerWaves) {      // no more pushes: one last look
                if (takeSome()) continue;
                break;
            }
            __builtin_amdgcn_s_sleep(64);
        }
        last = signOff() == totalWaves - 1;
    }
    if (last && lane == 0) {
        __hip_atomic_store(head, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a second launch without the stage reset must not find stale entries)
        __hip_atomic_store(done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The walk only records the hit (ws.hit, hitInst, hitT, routeCode) and k_route_hits pushes the queue entries afterwards in one streaming
// pass; waves never meet, so a wave whose 64 walks are done moves on to its next 64 rays while the others still walk.
constexpr uint32_t ROUTE_SKIP = 0x80000000u;   // near-tie: the re-trace routes this ray
// The occupancy target of a walk kernel.  The general-primitive variants (GEN >= 2) cannot reach the triangle kernels' 4-5 waves, but the
// target still matters: the allocator spills towards it before the callees' frames are added (asked for 3 / 2 waves, which they could
// reach, GEN = 2 / 3 ended at 2 / 1; asked for the triangle kernels' 4-5 they end at 3 / 2).  GEN = 2 takes the triangle kernels' target.
// (GEN = 3, the curve kernels: at the one-level kernels' 5-wave target they were the only kernels of the library that spilled an SGPR-spill
//  carrier register — tools/check_spill_carriers.py; at the two-level kernels' 4 they do not)
// (round 5: with alpha textures on curves the GEN = 3 kernels reach the curve intersector through the alpha recursion as well — a chain of
//  out-of-line callees the compiler gives 200+ VGPRs; it reported "final occupancy is 2" for every target above, and at a target of 4 the
//  kernels spilled carriers again: their target is what they get)
constexpr int TWavesFor(int gen, int triangleWaves) { return gen == 3 ? 2 : triangleWaves; }
// GENX: 0 - 3 as above; 4 / 5 = GEN 0 / 1 handing rays that meet a quadric / patch / curve to `deferQ` (TWO-CLASS TRAVERSAL).
// list != nullptr: walk the rays list[0 .. counters[CNT_DEFER]) of the queue instead of all of it (the second launch of that scheme).
template <int GENX, bool INST = false>
__global__ void __launch_bounds__(TBLOCK, TWavesFor(GenBase(GENX), INST ? WF_TWAVES_INST : WF_TWAVES_CLOSEST)) k_closest_fast(const SceneView svArg, WorkState ws, FastBVH bvh, int cur, SpillArea sp, int *cursor = nullptr, int chunk = 4, const int *list = nullptr) {
    constexpr int GEN = GenBase(GENX);
    const SceneView &sv = SvOf<false>(svArg);
    const int n = list ? ws.counters[(CNT_DEFER) * CNT_STRIDE] : ws.counters[(CNT_RAY0 + cur) * CNT_STRIDE];
    const int gtid = blockIdx.x * TBLOCK + threadIdx.x, stride = gridDim.x * TBLOCK;
    LdsStackT st{sp.base + gtid, stride, 0, 0, sp.rows, sp.dbg};
    const RayQueueV q = ws.rq[cur];
    // near-ties resolved by this launch itself: the kernels that would otherwise inline the reference-order walk (RetraceInline), walking with refill
    constexpr bool DRAIN = RetraceInline(GEN);
    const int workBlocks = DRAIN ? (int)gridDim.x - ServiceBlocks() : (int)gridDim.x;
    if (DRAIN && (int)blockIdx.x >= workBlocks) { DrainRetrace<GEN, INST, GenAnim(GENX)>(sv, ws, bvh, cur, st, true); return; }   // a service workgroup
    TraceQueue<false, GENX, INST, DRAIN>(
        sv, bvh, n, st,
        [&](int i0, V3 *o, V3 *d, float *tMax) {
            const int i = list ? list[i0] : i0;
            F4 o4 = q.o[i], d4 = q.d[i];
            *o = V3{o4.x, o4.y, o4.z}; *d = V3{d4.x, d4.y, d4.z}; *tMax = WF_INFINITY;
            if constexpr (GenAnim(GENX)) {
                g_time[threadIdx.x] = o4.w;
                ws.pathTime[q.meta[i].x] = o4.w;   // the path's time, for the shadow rays this depth spawns (k_intersect_closest<.., ANIM>)
            }
        },
        [&](int i0, bool valid, const RayWalk &w) {
            const int i = (list && valid) ? list[i0] : i0;
            if constexpr (GenDefer(GENX))
                if (valid && (w.route & WALK_DEFER)) {   // the general-primitive launch walks this ray (and writes its record)
                    ws.deferQ[QueueAlloc(&ws.counters[(CNT_DEFER) * CNT_STRIDE])] = i;
                    ws.routeCode[i] = ROUTE_SKIP;
                    return;
                }
            // near-tie seen (wf_traverse.h): the reference-order walk decides (k_closest_retrace)
            const bool amb = valid && WalkAmbiguous(w);
            if (amb) {
                const int slot = atomicAdd(&ws.counters[(CNT_RETRACE) * CNT_STRIDE], 1);
                const float bound = 2 * WalkBound(bvh, WalkT(w)) - WalkT(w);   // the re-trace's starting bound, see k_closest_retrace
                if constexpr (DRAIN) {
                    if (sp.dbg) atomicAdd(sp.dbg + 4, 1);
                    __hip_atomic_store(&ws.retraceQ[slot], (int)FloatToBits(bound), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&ws.retraceQ64[slot], (unsigned long long)(uint32_t)i | ((unsigned long long)(uint32_t)ws.drainEpoch << 32), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    return;   // DrainRetrace writes the ray's record
                } else {
                    ws.retraceQ[slot] = i;
                    ws.hit[i] = F4{0, bound, 0, 0};
                }
            }
            if (!valid) return;
            ws.routeCode[i] = amb ? ROUTE_SKIP : (uint32_t)w.route;
            if (amb) return;
            ws.hit[i] = F4{BitsToFloat((uint32_t)w.prim), w.b0, w.b1, w.b2};
            if (INST) ws.hitInst[i] = w.prim >= 0 ? w.inst : -1;
            if (sv.haveMedia) ws.hitT[i] = w.prim >= 0 ? WalkT(w) : WF_INFINITY;
        }, cursor, chunk, workBlocks);
    if constexpr (DRAIN) DrainRetrace<GEN, INST, GenAnim(GENX)>(sv, ws, bvh, cur, st, false);
}
// the routing pass of the closest-hit traversal: EnqueueWorkAfterIntersection / Miss for every ray of the queue (block-aggregated pushes)
// (1024 threads per workgroup: one returning atomic per destination queue per 1024 rays — a queue counter sustains ~88 of them per
// microsecond, which at 256 rays per workgroup was the whole cost of this pass)
constexpr int RBLOCK = 1024;
// ANIM: the scene has animated primitives (the interface skip rebuilds the hit's interaction at the ray's time).  That variant takes
// workgroups of BLOCK threads: the interpolation is an out-of-line callee shared with the ANIM walk kernels, and a 1024-thread caller
// would cap its registers at 128 for all of them (measured: k_closest_fast<8, true> 162 -> 128 VGPRs, its spills 104 -> 183).
constexpr int RouteBlock(bool anim) { return anim ? BLOCK : RBLOCK; }
template <bool GENERAL, bool ANIM = false>
__global__ void __launch_bounds__(RouteBlock(ANIM)) k_route_hits(const SceneView svArg, WorkState ws, int cur) {
    constexpr int RB = RouteBlock(ANIM);
    const SceneView &sv = SvOf<true>(svArg);
    const int n = ws.counters[(CNT_RAY0 + cur) * CNT_STRIDE];
    for (int base = blockIdx.x * RB; base < n; base += gridDim.x * RB) {
        const int i = base + threadIdx.x;
        bool valid = i < n;
        uint32_t route = 0;
        F4 h{0, 0, 0, 0};
        int inst = -1;
        float tHit = 0;
        if (valid) {
            route = ws.routeCode[i];
            if (route & ROUTE_SKIP) valid = false;
            else {
                h = ws.hit[i];
                if (sv.nInstances > 0) inst = ws.hitInst[i];
                if (sv.haveMedia) tHit = ws.hitT[i];
            }
        }
        KRouteHitBlock<GENERAL, ANIM>(sv, ws, cur, i, valid, (int)FloatToBits(h.x), route, tHit, h.y, h.z, h.w, inst);
    }
}
// the rays k_closest_fast marked as near-ties, in the reference's own traversal order (rare: coplanar overlapping geometry)
__global__ void __launch_bounds__(BLOCK) k_closest_retrace(const SceneView sv, WorkState ws, int cur, int *stackSpill) {
    const int n = ws.counters[(CNT_RETRACE) * CNT_STRIDE];
    const int gtid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
    LdsStack st{stackSpill + gtid, stride, 0};
    for (int qi = gtid; qi < n; qi += stride) {
        const int i = ws.retraceQ[qi];
        F4 o = ws.rq[cur].o[i], d = ws.rq[cur].d[i];
        ClosestHit ch;
        st.n = 0;
        // The walk starts from tMax = t* + twice the near-tie band instead of infinity (t* = the production walk's hit): every
        // candidate that can end up as the reference's hit lies inside the band around t*, a candidate beyond the starting
        // bound could only have been a temporary hit that the band's members replace — the result is the reference's, and
        // the walk visits a fraction of the nodes (the latency of this launch is one ray's dependent chain).
        bool found = BVHIntersectClosest(sv, V3{o.x, o.y, o.z}, V3{d.x, d.y, d.z}, ws.hit[i].y, st, &ch);
        KAfterClosestHit(sv, ws, cur, i, found, ch.prim, ch.inst, ch.h.t, ch.h.b0, ch.h.b1, ch.h.b2);
    }
}
// K12 (wavefront/subsurface.cpp): probe segment, one random intersection of it with the same material, out-scattering
__global__ void __launch_bounds__(BLOCK) k_subsurface_probe(const SceneView sv, WorkState ws) {
    const int n = ws.counters[(CNT_BSSRDF) * CNT_STRIDE];
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) KSubsurfaceProbe(sv, ws, i);
}
template <bool ANIM>
__global__ void __launch_bounds__(BLOCK) k_intersect_one_random(const SceneView sv, WorkState ws, int *stackSpill) {
    const int n = ws.counters[(CNT_SSS) * CNT_STRIDE];
    const int gtid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
    LdsStack st{stackSpill + gtid, stride, 0};
    for (int i = gtid; i < n; i += stride) KIntersectOneRandom<ANIM>(sv, ws, i, st);
}
// IntersectOneRandom on caller-supplied probe segments (the boundary adapter's path): segs = p0.xyz p1.xyz at the head of every
// segStride floats (6: the packed host arrays; 7: the caller's device segments {p0, p1, time}, wf_trace_one_random_device)
// ANIM: walked at times[timeStride * i] (the host call's array of times, or the seventh float of the device segments); otherwise at
// time 0 on a static scene
template <bool ANIM>
__global__ void __launch_bounds__(BLOCK) k_trace_one_random(const SceneView sv, int n, const float *segs, int segStride, const int32_t *material, const float *times,
                                                            int timeStride, wf_hit_record *out, float *pdf, int *stackSpill) {
    const int gtid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
    LdsStack st{stackSpill + gtid, stride, 0};
    for (int i = gtid; i < n; i += stride) {
        const float *s = segs + (size_t)segStride * i;
        ClosestHit ch;
        SurfIntr si;
        float p = IntersectOneRandom<ANIM>(sv, V3{s[0], s[1], s[2]}, V3{s[3], s[4], s[5]}, material[i], st, &ch, &si, ANIM ? times[(size_t)timeStride * i] : 0.f);
        wf_hit_record h{};
        h.prim = p != 0 ? ch.prim : -1;
        if (p != 0) { h.t = ch.h.t; h.b0 = ch.h.b0; h.b1 = ch.h.b1; h.b2 = ch.h.b2; h.instance = ch.inst; } else h.instance = -1;
        out[i] = h;
        pdf[i] = p;
    }
}
__global__ void __launch_bounds__(BLOCK) k_subsurface_scatter(const SceneView sv, WorkState ws, int cur) {
    const int n = ws.counters[(CNT_SSS) * CNT_STRIDE];
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) KSubsurfaceScatter(sv, ws, cur, i);
}
template <int GEN, bool INST = false>
__global__ void __launch_bounds__(TBLOCK, TWavesFor(GenBase(GEN), INST ? WF_TWAVES_INST_SHADOW : WF_TWAVES)) k_shadow_fast(const SceneView svArg, WorkState ws, FastBVH bvh, SpillArea sp, int *cursor = nullptr, int chunk = 4, const int *list = nullptr) {
    const SceneView &sv = SvOf<false>(svArg);
    const int n = list ? ws.counters[(CNT_DEFER_SHADOW) * CNT_STRIDE] : ws.counters[(CNT_SHADOW) * CNT_STRIDE];
    const int gtid = blockIdx.x * TBLOCK + threadIdx.x, stride = gridDim.x * TBLOCK;
    LdsStackT st{sp.base + gtid, stride, 0, 0, sp.rows, sp.dbg};
    TraceQueue<true, GEN, INST>(
        sv, bvh, n, st,
        [&](int i0, V3 *o, V3 *d, float *tMax) {
            const int i = list ? list[i0] : i0;
            F4 o4 = ws.sq.o[i], d4 = ws.sq.d[i];
            *o = V3{o4.x, o4.y, o4.z}; *d = V3{d4.x, d4.y, d4.z}; *tMax = o4.w;
            if constexpr (GenAnim(GEN)) g_time[threadIdx.x] = ShadowTime<true>(ws, d4.w);
        },
        [&](int i0, bool valid, const RayWalk &w) {
            if (!valid) return;
            const int i = list ? list[i0] : i0;
            if constexpr (GenDefer(GEN))
                if (w.route & WALK_DEFER) {   // (the walk stops at its first occluder: a ray handed over has none among the triangles before the leaf it met)
                    ws.deferQ[QueueAlloc(&ws.counters[(CNT_DEFER_SHADOW) * CNT_STRIDE])] = i;
                    return;
                }
            KRecordShadowRay(ws, i, w.prim >= 0);
        }, cursor, chunk);
}

// A ray of the stand-alone walks.  STRIDE 7: {o[3], d[3], tMax} (wf_trace_*_device).  STRIDE 8: {o[3], d[3], tMax, time}, aligned to 16
// bytes and read as two 16-byte loads (wf_trace_*_device_t); the ANIM variants (GenAnim) leave the time where the instance entries of
// the walk read it, as k_shadow_fast does — a static scene's variants ignore it.
template <int GEN, int STRIDE>
__device__ inline void FetchTraceRay(const float *rays, int i, V3 *o, V3 *d, float *tMax) {
    static_assert(STRIDE == 7 || STRIDE == 8, "rays7 or rays8");
    static_assert(STRIDE == 8 || !GenAnim(GEN), "a ray of an animated scene needs its time");
    if constexpr (STRIDE == 8) {
        const F4 *r = reinterpret_cast<const F4 *>(rays) + (size_t)2 * i;
        const F4 a = r[0], b = r[1];
        *o = V3{a.x, a.y, a.z}; *d = V3{a.w, b.x, b.y}; *tMax = b.z;
        if constexpr (GenAnim(GEN)) g_time[threadIdx.x] = b.w;
    } else {
        const float *r = rays + (size_t)7 * i;
        *o = V3{r[0], r[1], r[2]}; *d = V3{r[3], r[4], r[5]}; *tMax = r[6];
    }
}
// GENERAL: the scene has alpha-tested triangles or quadrics (the variant the render uses then)
template <int GEN, bool INST, int STRIDE = 7>
__global__ void __launch_bounds__(TBLOCK) k_trace_closest_fast(const SceneView sv, FastBVH bvh, int n, const float *rays, wf_hit_record *out, SpillArea sp) {
    const int gtid = blockIdx.x * TBLOCK + threadIdx.x, stride = gridDim.x * TBLOCK;
    LdsStackT st{sp.base + gtid, stride, 0, 0, sp.rows, sp.dbg};
    TraceQueue<false, GEN, INST>(
        sv, bvh, n, st,
        [&](int i, V3 *o, V3 *d, float *tMax) { FetchTraceRay<GEN, STRIDE>(rays, i, o, d, tMax); },
        [&](int i, bool valid, const RayWalk &w) {
            if (!valid) return;
            wf_hit_record h;
            bool found = w.prim >= 0;
            h.prim = w.prim;
            h.t = found ? WalkT(w) : 0; h.b0 = w.b0; h.b1 = w.b1; h.b2 = w.b2;
            h.nodes_visited = WalkAmbiguous(w) ? -1 : 0;  // -1: near-tie, re-traced in reference order by the pass that follows
            h.tris_tested = 0; h.instance = (INST && found) ? w.inst : -1;
            out[i] = h;
        });
}
template <int GEN, bool INST, int STRIDE = 7>
__global__ void __launch_bounds__(TBLOCK) k_trace_any_fast(const SceneView sv, FastBVH bvh, int n, const float *rays, int32_t *occluded, SpillArea sp) {
    const int gtid = blockIdx.x * TBLOCK + threadIdx.x, stride = gridDim.x * TBLOCK;
    LdsStackT st{sp.base + gtid, stride, 0, 0, sp.rows, sp.dbg};
    TraceQueue<true, GEN, INST>(
        sv, bvh, n, st,
        [&](int i, V3 *o, V3 *d, float *tMax) { FetchTraceRay<GEN, STRIDE>(rays, i, o, d, tMax); },
        [&](int i, bool valid, const RayWalk &w) { if (valid) occluded[i] = w.prim >= 0; });
}

// ANIM: the scene has animated primitives (the amount textures are evaluated on the interaction at the ray's time)
template <bool ANIM>
__global__ void __launch_bounds__(BLOCK) k_resolve_mix(const SceneView sv, WorkState ws, int cur) {
    const int n = ws.counters[(CNT_MIX) * CNT_STRIDE];
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) KResolveMix<ANIM>(sv, ws, cur, i);
}
// K5 / K6 / K11: participating media (wf_media.h, wf_kernels.h)
// (round 5) the delta-tracking loop alone: the routing of the items that reach their surface — interaction rebuild of interface hits,
// MixMaterial resolve — is the kernel after it (219 VGPRs / 604 B of scratch -> 207 / 0 for the loop; WF_MEDIUM_WAVES sets its occupancy target)
#ifndef WF_MEDIUM_WAVES
#define WF_MEDIUM_WAVES 2
#endif
// (round 6, measured and dropped: a persistent form of this kernel with wave-level refill of the delta-tracking loop, VERDICT r5 item 8 —
//  a wave whose active lanes dropped below a threshold took new items for its idle lanes from a shared work cursor)
// LEAN: every medium of the scene is homogeneous or a non-emissive uniform grid (ctx->plan.mediumLean, set at upload): the kernel is built without the
// procedural cloud, NanoVDB, RGB-grid and blackbody code and compiled for WF_MEDIUM_WAVES_LEAN waves
#ifndef WF_MEDIUM_WAVES_LEAN
#define WF_MEDIUM_WAVES_LEAN 3
#endif
template <bool LEAN>
__global__ void __launch_bounds__(BLOCK, LEAN ? WF_MEDIUM_WAVES_LEAN : WF_MEDIUM_WAVES) k_medium_sample(const SceneView sv, WorkState ws, int cur) {
    const int n = ws.counters[(CNT_MEDIUM_SAMPLE) * CNT_STRIDE];
    // (the nested-loop form of rounds 1-5 measured 43.2 ms against this form's 36.5 on the cloud scene, same box: profiles/r06_medium_nested_vs_state_machine_ab_cloud16.txt)
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) KSampleMediumInteraction<LEAN>(sv, ws, cur, i);
}
// ANIM: the scene has animated primitives (interface / MixMaterial hits are rebuilt at the ray's time)
template <bool ANIM>
__global__ void __launch_bounds__(BLOCK) k_medium_route(const SceneView sv, WorkState ws, int cur) {
    const int n = ws.counters[(CNT_MEDIUM_ROUTE) * CNT_STRIDE];
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) KMediumRoute<ANIM>(sv, ws, cur, i);
}
template <bool RARE>
__global__ void __launch_bounds__(BLOCK) k_medium_scatter(const SceneView sv, WorkState ws, int cur) {
    const int n = ws.counters[(CNT_MEDIUM_SCATTER) * CNT_STRIDE];
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) KSampleMediumScattering<RARE>(sv, ws, cur, i);
}
// reference-order variant (no production BVH, or WF_NO_FAST)
template <bool ANIM>
__global__ void __launch_bounds__(BLOCK) k_shadow_tr(const SceneView sv, WorkState ws, int *stackSpill) {
    const int n = ws.counters[(CNT_SHADOW) * CNT_STRIDE];
    const int gtid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
    LdsStack st{stackSpill + gtid, stride, 0};
    for (int i = gtid; i < n; i += stride) {
        const float time = ShadowTime<ANIM>(ws, ws.sq.d[i].w);
        KTraceTransmittance<ANIM>(sv, ws, i, [&](V3 o, V3 d, float tMax, int *prim, int *inst, float *b0, float *b1, float *b2) {
            ClosestHit ch;
            st.n = 0;
            bool found = BVHIntersectClosest<ANIM>(sv, o, d, tMax, st, &ch, time);
            if (found) { *prim = ch.prim; *inst = ch.inst; *b0 = ch.h.b0; *b1 = ch.h.b1; *b2 = ch.h.b2; }
            return found;
        });
    }
}
// production layout, one independent walk per lane (a transmittance ray alternates between tracing and
// ratio tracking, so there is no batch to share)
struct TrPrims {  // the same callbacks for the transmittance walk, whose ray is a local of its loop
    static constexpr bool pairBands = true;   // (a per-lane loop over whole scenes, general shapes included)
    static constexpr bool deferGeneral = false;
    const SceneView &sv;
    V3 o, d;
    __device__ bool accept(int prim, float b0, float b1, float b2) const { return AlphaTestPasses(sv, prim, b0, b1, b2, o, d); }
    __device__ bool sphere(int prim, float tMax, QuadricHit *qh) const { return QuadricIntersect(sv, prim, o, d, tMax, qh); }
};
// MLEAN: the lean medium code (ctx->plan.mediumLean, as k_medium_sample<true>)
template <bool ALPHA, bool MLEAN = false>
__global__ void __launch_bounds__(TBLOCK) k_shadow_tr_fast(const SceneView sv, WorkState ws, FastBVH bvh, SpillArea sp) {
    const int n = ws.counters[(CNT_SHADOW) * CNT_STRIDE];
    const int gtid = blockIdx.x * TBLOCK + threadIdx.x, stride = gridDim.x * TBLOCK;
    LdsStackT st{sp.base + gtid, stride, 0, 0, sp.rows, sp.dbg};
    for (int i = gtid; i < n; i += stride)
        KTraceTransmittance<false, MLEAN>(sv, ws, i, [&](V3 o, V3 d, float tMax, int *prim, int *inst, float *b0, float *b1, float *b2) {
            RayWalk w;
            WalkInit(bvh, w, o, d, tMax);
            st.reset();
            while (w.node != NODE_NONE) {
                if (w.node >= 0) {
                    U4 nd[QNODE_U4];
                    FetchNode(bvh, w.node, nd);
                    InteriorStep(bvh, w, st, nd);
                } else if constexpr (ALPHA) LeafStep<false, true>(bvh, w, st, TrPrims{sv, o, d});
                else LeafStep<false>(bvh, w, st);
            }
            if (WalkAmbiguous(w)) {  // near-tie (wf_traverse.h): the reference-order walk decides
                ClosestHit ch;
                st.reset();
                bool found = BVHIntersectClosest(sv, o, d, tMax, st, &ch);
                if (found) { *prim = ch.prim; *inst = ch.inst; *b0 = ch.h.b0; *b1 = ch.h.b1; *b2 = ch.h.b2; }
                return found;
            }
            if (w.prim >= 0) { *prim = w.prim; *b0 = w.b0; *b1 = w.b1; *b2 = w.b2; }
            return w.prim >= 0;
        });
}

// ---- the transmittance wavefront (round 3): TraceTransmittance as launches instead of one loop per lane ------------------------------
// k_tr_begin sets up the state of every shadow ray (TrBegin) and the first index queue; per segment k_tr_trace walks the live rays
// with the production closest-hit traversal (two-level scenes included; near ties resolved inside the walk: the scenes of the
// GEN <= 1 variants) and records the hits in ws.hit / ws.hitInst — free at this point of the depth — and k_tr_segment runs the rest
// of the loop body (interaction, ratio tracking along the segment, respawn behind an interface), finishing rays or queuing them for
// the next segment.  After WF_TR_SEGMENTS rounds k_tr_rest finishes what is still alive with the per-lane loop (reference-order walk).
#ifndef WF_TR_SEGMENTS
#define WF_TR_SEGMENTS 4
#endif
__global__ void __launch_bounds__(BLOCK) k_tr_begin(const SceneView sv, WorkState ws) {
    const int n = ws.counters[(CNT_SHADOW) * CNT_STRIDE];
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        TrState st;
        TrBegin(ws, i, &st);
        if (st.rd.x == 0 && st.rd.y == 0 && st.rd.z == 0) { TrFinish(ws, i, st); continue; }
        TrStore(ws, i, st);
        ws.trQ[0][QueueAlloc(&ws.counters[(CNT_TR0) * CNT_STRIDE])] = i;
    }
}
template <int GEN, bool INST>
__global__ void __launch_bounds__(TBLOCK, INST ? WF_TWAVES_INST : WF_TWAVES_CLOSEST) k_tr_trace(const SceneView sv, WorkState ws, FastBVH bvh, int cur, SpillArea sp) {
    const int n = ws.counters[(CNT_TR0 + cur) * CNT_STRIDE];
    const int gtid = blockIdx.x * TBLOCK + threadIdx.x, stride = gridDim.x * TBLOCK;
    LdsStackT st{sp.base + gtid, stride, 0, 0, sp.rows, sp.dbg};
    const int32_t *q = ws.trQ[cur];
    TraceQueue<false, GEN, INST>(
        sv, bvh, n, st,
        [&](int j, V3 *o, V3 *d, float *tMax) {
            const int i = q[j];
            F4 o4 = ws.trO[i], d4 = ws.trD[i];
            *o = V3{o4.x, o4.y, o4.z}; *d = V3{d4.x, d4.y, d4.z}; *tMax = ws.sq.o[i].w;
            // (the time of the ORIGINAL shadow item: every segment of one ray, the ones respawned behind an interface included, is walked
            //  at the same time; the walk fetches a near-tie ray a second time, which stores the same value again)
            if constexpr (GenAnim(GEN)) g_time[threadIdx.x] = ShadowTime<true>(ws, ws.sq.d[i].w);
        },
        [&](int j, bool valid, const RayWalk &w) {
            if (!valid) return;
            const int i = q[j];
            ws.hit[i] = F4{BitsToFloat((uint32_t)w.prim), w.b0, w.b1, w.b2};
            if (INST) ws.hitInst[i] = w.prim >= 0 ? w.inst : -1;
        });
}
// MLEAN: the lean medium code.  ANIM: the scene has animated primitives (the interaction of a hit through one is rebuilt at the ray's
// time; workgroups of BLOCK threads, like every caller of the interpolation: see RouteBlock)
template <bool MLEAN, bool ANIM = false>
__global__ void __launch_bounds__(BLOCK) k_tr_segment(const SceneView sv, WorkState ws, int cur) {
    const int n = ws.counters[(CNT_TR0 + cur) * CNT_STRIDE];
    for (int j = blockIdx.x * BLOCK + threadIdx.x; j < n; j += gridDim.x * BLOCK) {
        const int i = ws.trQ[cur][j];
        TrState st;
        TrLoad(ws, i, &st);
        const F4 h = ws.hit[i];
        const int prim = (int)FloatToBits(h.x);
        if (TrSegment<ANIM, MLEAN>(sv, ws, i, &st, prim >= 0, prim, HitInst(sv, ws, i), h.y, h.z, h.w)) {
            TrStore(ws, i, st);
            ws.trQ[cur ^ 1][QueueAlloc(&ws.counters[(CNT_TR0 + (cur ^ 1)) * CNT_STRIDE])] = i;
        } else TrFinish(ws, i, st);
    }
}
// ANIM: the reference-order walk at the shadow item's time, as k_shadow_tr<true>
template <bool ANIM>
__global__ void __launch_bounds__(BLOCK) k_tr_rest(const SceneView sv, WorkState ws, int cur, int *stackSpill) {
    const int n = ws.counters[(CNT_TR0 + cur) * CNT_STRIDE];
    if (n == 0) return;
    const int gtid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
    LdsStack st{stackSpill + gtid, stride, 0};
    for (int j = gtid; j < n; j += stride) {
        const int i = ws.trQ[cur][j];
        TrState ts;
        TrLoad(ws, i, &ts);
        const float time = ShadowTime<ANIM>(ws, ws.sq.d[i].w);
        KTraceTransmittanceFrom<ANIM>(sv, ws, i, ts, [&](V3 o, V3 d, float tMax, int *prim, int *inst, float *b0, float *b1, float *b2) {
            ClosestHit ch;
            st.n = 0;
            bool found = BVHIntersectClosest<ANIM>(sv, o, d, tMax, st, &ch, time);
            if (found) { *prim = ch.prim; *inst = ch.inst; *b0 = ch.h.b0; *b1 = ch.h.b1; *b2 = ch.h.b2; }
            return found;
        });
    }
}

// RARE = false: no portal infinite light (k_handle_escaped: 328 VGPRs + 72 AGPRs — one wave per SIMD — with the portal callees and the area
// lights' PDFs reachable; round 5)
template <bool RARE>
__global__ void __launch_bounds__(BLOCK) k_handle_escaped(const SceneView svArg, WorkState ws, int cur) {
    const SceneView &sv = SvOf<false>(svArg);
    const int n = ws.counters[(CNT_ESCAPED) * CNT_STRIDE];
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) KHandleEscaped<RARE>(sv, ws, cur, i);
}
__global__ void __launch_bounds__(BLOCK) k_handle_emissive(const SceneView svArg, WorkState ws, int cur) {
    const SceneView &sv = SvOf<false>(svArg);
    const int n = ws.counters[(CNT_HITLIGHT) * CNT_STRIDE];
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) KHandleEmissive(sv, ws, cur, i);
}
// the material kernels live in wf_mat.hip (one translation unit per material type)
// the material types that have kernels (wf_material_type 1 .. WF_MAT_NTYPES - 1): the one list the declarations and tables below are made from
#define WF_MAT_TYPES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10)
extern "C" {
#define WF_MAT_DECL(n) void wf_launch_mat_shade_##n##_0(hipStream_t, int, const SceneView *, const WorkState *, int); \
                       void wf_launch_mat_shade_##n##_1(hipStream_t, int, const SceneView *, const WorkState *, int); \
                       void wf_launch_mat_shade_##n##_2(hipStream_t, int, const SceneView *, const WorkState *, int); \
                       void wf_launch_mat_shade_##n##_3(hipStream_t, int, const SceneView *, const WorkState *, int); \
                       void wf_launch_mat_nee_##n##_0(hipStream_t, int, const SceneView *, const WorkState *); \
                       void wf_launch_mat_nee_##n##_1(hipStream_t, int, const SceneView *, const WorkState *);
WF_MAT_TYPES(WF_MAT_DECL)
}
#define WF_MAT_SHADE_ROW(n) {wf_launch_mat_shade_##n##_0, wf_launch_mat_shade_##n##_1, wf_launch_mat_shade_##n##_2, wf_launch_mat_shade_##n##_3},
#define WF_MAT_NEE_ROW(n) {wf_launch_mat_nee_##n##_0, wf_launch_mat_nee_##n##_1},
static const MatShadeFn kMatShade[WF_MAT_NTYPES][4] = {{}, WF_MAT_TYPES(WF_MAT_SHADE_ROW)};   // [type][shade variant]; row 0: WF_MAT_INTERFACE has no kernel
static const MatNeeFn kMatNee[WF_MAT_NTYPES][2] = {{}, WF_MAT_TYPES(WF_MAT_NEE_ROW)};         // [type][rare lights]
// ... and the launchers' siblings, which answer for their units' kernels: resident workgroups per CU (STAGE GRIDS)
using MatResidentFn = int (*)(int *);
extern "C" {
#define WF_MAT_RESIDENT_DECL(n) int wf_resident_mat_shade_##n##_0(int *); int wf_resident_mat_shade_##n##_1(int *); int wf_resident_mat_shade_##n##_2(int *); \
                                int wf_resident_mat_shade_##n##_3(int *); int wf_resident_mat_nee_##n##_0(int *); int wf_resident_mat_nee_##n##_1(int *);
WF_MAT_TYPES(WF_MAT_RESIDENT_DECL)
}
#define WF_MAT_SHADE_RESIDENT_ROW(n) {wf_resident_mat_shade_##n##_0, wf_resident_mat_shade_##n##_1, wf_resident_mat_shade_##n##_2, wf_resident_mat_shade_##n##_3},
#define WF_MAT_NEE_RESIDENT_ROW(n) {wf_resident_mat_nee_##n##_0, wf_resident_mat_nee_##n##_1},
static const MatResidentFn kMatShadeResident[WF_MAT_NTYPES][4] = {{}, WF_MAT_TYPES(WF_MAT_SHADE_RESIDENT_ROW)};
static const MatResidentFn kMatNeeResident[WF_MAT_NTYPES][2] = {{}, WF_MAT_TYPES(WF_MAT_NEE_RESIDENT_ROW)};
// bytes of one NeeItem's BxDF (wf_kernels.h) -> 16-byte planes of the record between the two kernels (wf_mat.hip: NeeIO)
template <int MAT> constexpr int NeePlanesOf() { return 10 + (int)((sizeof(typename MatBxDF<MAT>::T) + 15) / 16); }
static int NeePlanes(int m) {
    switch (m) {
#define WF_MAT_PLANES(n) case n: return NeePlanesOf<n>();
    WF_MAT_TYPES(WF_MAT_PLANES)
    }
    return 0;
}
__global__ void __launch_bounds__(BLOCK) k_update_film(const SceneView sv, WorkState ws, int nSamples) {
    for (int p = blockIdx.x * BLOCK + threadIdx.x; p < ws.pixelsPerPass; p += gridDim.x * BLOCK) KUpdateFilm(sv, ws, p, nSamples);
}
// The RGB film under the pixel-major item order (WorkState::slotStride = nSamples): a pixel's samples are neighbours, so the workgroup
// reads FILM_PIX pixels x nSamples items with coalesced loads, one item per thread and round, leaves each item's four addends in LDS, and
// one thread per pixel then adds its samples in slot order into the double accumulators — the order KUpdateFilm adds them in.
constexpr int FILM_PIX = 32, FILM_MAX_SLOTS = 64;
__global__ void __launch_bounds__(BLOCK) k_update_film_pm(const SceneView sv, WorkState ws, int nSamples) {
    __shared__ float add[FILM_PIX * FILM_MAX_SLOTS][4];
    __shared__ unsigned long long filmIdx[FILM_PIX];
    const int nItems = FILM_PIX * nSamples;
    for (int p0 = blockIdx.x * FILM_PIX; p0 < ws.pixelsPerPass; p0 += gridDim.x * FILM_PIX) {
        if (threadIdx.x < FILM_PIX) filmIdx[threadIdx.x] = ~0ull;
        __syncthreads();
        for (int j = threadIdx.x; j < nItems; j += BLOCK) {
            const int pl = j / nSamples;
            if (p0 + pl >= ws.pixelsPerPass) break;
            size_t idx;
            float v[4];
            if (FilmSampleRGBW(sv, ws, p0 * nSamples + j, v, &idx)) {
                add[j][0] = v[0]; add[j][1] = v[1]; add[j][2] = v[2]; add[j][3] = v[3];
                if (j - pl * nSamples == 0) filmIdx[pl] = idx;
            }
        }
        __syncthreads();
        if (threadIdx.x < FILM_PIX && filmIdx[threadIdx.x] != ~0ull) {
            double *px = ws.film + 4 * filmIdx[threadIdx.x];
            double a0 = px[0], a1 = px[1], a2 = px[2], a3 = px[3];
            for (int s = 0; s < nSamples; ++s) {
                const float *v = add[threadIdx.x * nSamples + s];
                a0 += v[0]; a1 += v[1]; a2 += v[2]; a3 += v[3];
            }
            px[0] = a0; px[1] = a1; px[2] = a2; px[3] = a3;
        }
        __syncthreads();
    }
}

// stand-alone traversal for parity tests / counters: rays as {o[3], d[3], tMax} at the head of every rayStride floats (7: packed;
// 8: the rays8 of wf_trace_*_device_t on a static scene, whose eighth float — the time — is not read); mode: TRACE_* of wf_ctx.h
__global__ void __launch_bounds__(BLOCK) k_trace_closest(const SceneView sv, int n, const float *rays, int rayStride, wf_hit_record *out, int *stackSpill, int mode) {
    const int gtid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
    LdsStack st{stackSpill + gtid, stride, 0};
    const bool onlyMarked = (mode & TRACE_ONLY_MARKED) != 0, counts = mode == 0;
    for (int i = gtid; i < n; i += stride) {
        if (onlyMarked && out[i].nodes_visited != -1) continue;
        const float *r = rays + (size_t)rayStride * i;
        ClosestHit ch;
        st.n = 0;
        bool found = BVHIntersectClosest(sv, V3{r[0], r[1], r[2]}, V3{r[3], r[4], r[5]}, r[6], st, &ch);
        wf_hit_record h;
        h.prim = found ? ch.prim : -1;
        h.t = found ? ch.h.t : 0; h.b0 = found ? ch.h.b0 : 0; h.b1 = found ? ch.h.b1 : 0; h.b2 = found ? ch.h.b2 : 0;
        h.nodes_visited = counts ? ch.nodesVisited : 0; h.tris_tested = counts ? ch.trisTested : 0; h.instance = found ? ch.inst : -1;
        out[i] = h;
    }
}
// ... and at the rays' own TIMES (AnimatedPrimitive, cpu/primitive.cpp:132-158: the reference's WavefrontAggregate reads ray.time): the
// reference-order walks with the per-ray interpolation of the animated transformations.  Ray i at rays + rayStride i, its time at
// times[timeStride i]: (7, 1) the host call's packed rays with the n times behind them (wf_trace_*_host_t), (8, 8) the caller's rays8
// with times = rays8 + 7 (wf_trace_*_device_t on the animated scenes the production walk does not take).  counts = 0: no visit counts
__global__ void __launch_bounds__(BLOCK) k_trace_closest_timed(const SceneView sv, int n, const float *rays, int rayStride, const float *times, int timeStride,
                                                               wf_hit_record *out, int *stackSpill, int counts) {
    const int gtid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
    LdsStack st{stackSpill + gtid, stride, 0};
    for (int i = gtid; i < n; i += stride) {
        const float *r = rays + (size_t)rayStride * i;
        ClosestHit ch;
        st.n = 0;
        bool found = BVHIntersectClosest<true>(sv, V3{r[0], r[1], r[2]}, V3{r[3], r[4], r[5]}, r[6], st, &ch, times[(size_t)timeStride * i]);
        wf_hit_record h;
        h.prim = found ? ch.prim : -1;
        h.t = found ? ch.h.t : 0; h.b0 = found ? ch.h.b0 : 0; h.b1 = found ? ch.h.b1 : 0; h.b2 = found ? ch.h.b2 : 0;
        h.nodes_visited = counts ? ch.nodesVisited : 0; h.tris_tested = counts ? ch.trisTested : 0; h.instance = found ? ch.inst : -1;
        out[i] = h;
    }
}
__global__ void __launch_bounds__(BLOCK) k_trace_any_timed(const SceneView sv, int n, const float *rays, int rayStride, const float *times, int timeStride,
                                                           int32_t *occluded, int *stackSpill) {
    const int gtid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
    LdsStack st{stackSpill + gtid, stride, 0};
    for (int i = gtid; i < n; i += stride) {
        const float *r = rays + (size_t)rayStride * i;
        int v = 0, t = 0;
        st.n = 0;
        occluded[i] = BVHIntersectAny<true>(sv, V3{r[0], r[1], r[2]}, V3{r[3], r[4], r[5]}, r[6], st, &v, &t, times[(size_t)timeStride * i]);
    }
}
// IntersectShadowTr on the caller's DEVICE items (wf_trace_shadow_tr_device): the per-item arrays of the scratch WorkState that the
// transmittance kernels read and the caller does not supply — the shadow queue's (o, tMax) and (d, pixelIndex = i), the wavelengths' pdf
// (1), the item's path time (animated scenes: pathTime != nullptr) — the zeroed result, and the counter block with CNT_SHADOW = n
__global__ void __launch_bounds__(BLOCK) k_pack_shadow_items(int n, const float *rays8, F4 *o, F4 *d, F4 *lambdaPdf, float *pathTime, F4 *L, int32_t *counters) {
    if (blockIdx.x == 0 && threadIdx.x < CNT_COUNT) counters[threadIdx.x * CNT_STRIDE] = threadIdx.x == CNT_SHADOW ? n : 0;
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const F4 *r = reinterpret_cast<const F4 *>(rays8) + (size_t)2 * i;
        const F4 a = r[0], b = r[1];
        o[i] = F4{a.x, a.y, a.z, b.z};
        d[i] = F4{a.w, b.x, b.y, BitsToFloat((uint32_t)i)};
        lambdaPdf[i] = F4{1, 1, 1, 1};
        if (pathTime) pathTime[i] = b.w;
        L[i] = F4{0, 0, 0, 0};
    }
}
__global__ void __launch_bounds__(BLOCK) k_trace_any(const SceneView sv, int n, const float *rays, int rayStride, int32_t *occluded, int32_t *nodes, int32_t *tris, int *stackSpill) {
    const int gtid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
    LdsStack st{stackSpill + gtid, stride, 0};
    for (int i = gtid; i < n; i += stride) {
        const float *r = rays + (size_t)rayStride * i;
        int v = 0, t = 0;
        st.n = 0;
        bool occ = BVHIntersectAny(sv, V3{r[0], r[1], r[2]}, V3{r[3], r[4], r[5]}, r[6], st, &v, &t);
        occluded[i] = occ;
        if (nodes) nodes[i] = v;
        if (tris) tris[i] = t;
    }
}

// ---------------------------------------------------------------------------------------------
// SceneView::gridCorners: cell (cx, cy, cz) of the (nx + 1)(ny + 1)(nz + 1) table <- the eight values a trilinear lookup with
// floor(p * res - .5) = (cx - 1, cy - 1, cz - 1) reads (wf_media.h: GridLookupPacked), zeros outside the grid
__global__ void k_pack_grid_corners(const float *v, int nx, int ny, int nz, float *out) {
    const size_t cells = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (size_t)gridDim.x * blockDim.x) {
        const int cx = (int)(c % (size_t)(nx + 1)), cy = (int)((c / (size_t)(nx + 1)) % (size_t)(ny + 1)), cz = (int)(c / ((size_t)(nx + 1) * (ny + 1)));
        const int ix = cx - 1, iy = cy - 1, iz = cz - 1;
        float *o = out + 8 * wf::GridCornerIndex(nx, ny, cx, cy, cz);
        o[0] = wf::GridLookupI(v, nx, ny, nz, ix, iy, iz);         o[1] = wf::GridLookupI(v, nx, ny, nz, ix + 1, iy, iz);
        o[2] = wf::GridLookupI(v, nx, ny, nz, ix, iy + 1, iz);     o[3] = wf::GridLookupI(v, nx, ny, nz, ix + 1, iy + 1, iz);
        o[4] = wf::GridLookupI(v, nx, ny, nz, ix, iy, iz + 1);     o[5] = wf::GridLookupI(v, nx, ny, nz, ix + 1, iy, iz + 1);
        o[6] = wf::GridLookupI(v, nx, ny, nz, ix, iy + 1, iz + 1); o[7] = wf::GridLookupI(v, nx, ny, nz, ix + 1, iy + 1, iz + 1);
    }
}

// ---- the scene's walk kernels (WalkKernels) --------------------------------------------------------------------------------------
// the walk kernel templates as types, so that one function maps run-time values onto their instantiations
struct ClosestWalk { using Fn = ClosestWalkFn; template <int G, bool I> static Fn of() { return k_closest_fast<G, I>; } };
struct ShadowWalk { using Fn = ShadowWalkFn; template <int G, bool I> static Fn of() { return k_shadow_fast<G, I>; } };
struct TrTraceWalk { using Fn = TrTraceFn; template <int G, bool I> static Fn of() { return k_tr_trace<G, I>; } };
struct TraceClosestWalk { using Fn = TraceClosestFn; template <int G, bool I> static Fn of() { return k_trace_closest_fast<G, I>; } };
struct TraceAnyWalk { using Fn = TraceAnyFn; template <int G, bool I> static Fn of() { return k_trace_any_fast<G, I>; } };
struct TraceClosestWalk8 { using Fn = TraceClosestFn; template <int G, bool I> static Fn of() { return k_trace_closest_fast<G, I, 8>; } };   // (rays8)
struct TraceAnyWalk8 { using Fn = TraceAnyFn; template <int G, bool I> static Fn of() { return k_trace_any_fast<G, I, 8>; } };
// K<G, inst> for the G of the pack that equals genx; null if there is none.  The packs handed in are the variants the library holds —
// a pair that appears nowhere here is not compiled.  The ANIM variants (GenAnim) exist two-level only: an animated shape is an instance.
template <typename K, bool INST, int G>
static typename K::Fn WalkVariant() {
    if constexpr (GenAnim(G) && !INST) return nullptr;
    else return K::template of<G, INST>();
}
template <typename K, int... G>
static typename K::Fn PickWalk(int genx, bool inst, std::integer_sequence<int, G...>) {
    typename K::Fn f = nullptr;
    ((genx == G ? (void)(f = inst ? WalkVariant<K, true, G>() : WalkVariant<K, false, G>()) : (void)0), ...);
    return f;
}
static int PickWalkKernels(wf_ctx *ctx) {
    using QueueWalks = std::integer_sequence<int, 0, 1, 2, 3, GenX(0, true, false), GenX(1, true, false), GenX(0, false, true), GenX(1, false, true)>;
    const bool inst = ctx->svHost.nInstances > 0;
    const int gen = ctx->plan.genMode;
    // what every ray of a queue walks through: the triangle kernel that hands general primitives over, or the scene's one kernel
    const int first = ctx->plan.deferGeneral ? GenX(ctx->plan.genTri, true, false) : GenX(gen, false, ctx->plan.animFast);
    WalkKernels k;
    k.closest = PickWalk<ClosestWalk>(first, inst, QueueWalks{});
    k.shadow = PickWalk<ShadowWalk>(first, inst, QueueWalks{});
    if (ctx->plan.deferGeneral) {
        k.closestGen = PickWalk<ClosestWalk>(gen, inst, QueueWalks{});
        k.shadowGen = PickWalk<ShadowWalk>(gen, inst, QueueWalks{});
    }
    k.traceClosest = PickWalk<TraceClosestWalk>(gen, inst, std::integer_sequence<int, 0, 1, 2, 3>{});
    k.traceAny = PickWalk<TraceAnyWalk>(gen, inst, std::integer_sequence<int, 0, 1, 2, 3>{});
    {
        // the timed boundary calls: a static scene's rays through the variants above, an animFast scene's (genMode <= 1: near ties are
        // resolved inside the walk — RetraceInline — at the ray's time) through the ANIM variants of the render's walks
        using TimedWalks = std::integer_sequence<int, 0, 1, 2, 3, GenX(0, false, true), GenX(1, false, true)>;
        k.traceClosest8 = PickWalk<TraceClosestWalk8>(GenX(gen, false, ctx->plan.animFast), inst, TimedWalks{});
        k.traceAny8 = PickWalk<TraceAnyWalk8>(GenX(gen, false, ctx->plan.animFast), inst, TimedWalks{});
    }
    // (resolves its near ties inside the walk; an animFast scene's at the shadow item's time, through the ANIM variants)
    if (RetraceInline(gen)) k.trTrace = PickWalk<TrTraceWalk>(GenX(gen, false, ctx->plan.animFast), inst, std::integer_sequence<int, 0, 1, GenX(0, false, true), GenX(1, false, true)>{});
    if (!k.closest || !k.shadow || !k.traceClosest || !k.traceAny || !k.traceClosest8 || !k.traceAny8 || (ctx->plan.deferGeneral && (!k.closestGen || !k.shadowGen)) || (RetraceInline(gen) && !k.trTrace))
        return fail(-1, "no walk kernel for this scene (genMode %d, genTri %d, two-class %d, animated %d, instances %d)", gen, ctx->plan.genTri, (int)ctx->plan.deferGeneral, (int)ctx->plan.animFast, (int)inst);
    // resident workgroups of the queue walks (closest-hit and shadow differ in registers)
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, ctx->device));
    const int maxG = MAX_GRID * BLOCK / TBLOCK;  // stackSpill is sized for MAX_GRID * BLOCK threads
    auto residentGrid = [&](auto kernel, int *out) {
        int perCU = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, (const void *)kernel, TBLOCK, 0));
        *out = std::min(maxG, std::max(1, perCU) * prop.multiProcessorCount);
        return 0;
    };
    int e;
    if ((e = residentGrid(k.closest, &k.grid)) || (e = residentGrid(k.shadow, &k.gridShadow))) return e;
    if (ctx->plan.deferGeneral && ((e = residentGrid(k.closestGen, &k.gridGen)) || (e = residentGrid(k.shadowGen, &k.gridShadowGen)))) return e;
    ctx->walk = k;
    return 0;
}
// ---- the scene's stage kernels (StageKernels): the plan's values onto instantiations, each named here and nowhere else.  Only what the
// library has always compiled: no k_route_hits<false, true> (an animated primitive is an instance), no k_shadow_tr_fast<true, true> (ALPHA
// wins over MLEAN).  The order of the statements means nothing to the result: any order picks the same kernels (it only moves them in the code object).
static void PickStageKernels(wf_ctx *ctx) {
    const ScenePlan &p = ctx->plan;
    const bool anim = p.haveAnimated;   // the reference-order walks' ANIM: every scene with animated primitives (p.animFast: those the production walks take)
    StageKernels &k = ctx->stage;
    k.genCameraRays = p.cameraAnim ? k_gen_camera_rays<true> : k_gen_camera_rays<false>;
    k.intersectClosest[1] = anim ? k_intersect_closest<true, true> : k_intersect_closest<true, false>;   // <COUNT, ANIM>
    if (p.routeVariant == 2) k.routeHits = k_route_hits<true, true>;   // (animated primitives: two-level)
    else k.routeHits = p.routeVariant == 1 ? k_route_hits<true> : k_route_hits<false>;
    k.routeBlock = RouteBlock(p.routeVariant == 2);
    k.resolveMix = anim ? k_resolve_mix<true> : k_resolve_mix<false>;
    k.intersectClosest[0] = anim ? k_intersect_closest<false, true> : k_intersect_closest<false, false>;
    k.mediumSample = p.mediumLean ? k_medium_sample<true> : k_medium_sample<false>;
    k.mediumRoute = anim ? k_medium_route<true> : k_medium_route<false>;
    k.mediumScatter = p.rareLights ? k_medium_scatter<true> : k_medium_scatter<false>;
    if (p.animFast) k.trSegment = p.mediumLean ? k_tr_segment<true, true> : k_tr_segment<false, true>;   // <MLEAN, ANIM>
    else k.trSegment = p.mediumLean ? k_tr_segment<true> : k_tr_segment<false>;
    k.trRest = p.animFast ? k_tr_rest<true> : k_tr_rest<false>;
    k.shadowTrFast = p.trFastAlpha ? k_shadow_tr_fast<true> : p.mediumLean ? k_shadow_tr_fast<false, true> : k_shadow_tr_fast<false>;   // <ALPHA, MLEAN>
    k.shadowTrFastWitness = p.trFastAlpha ? k_shadow_tr_fast<true> : k_shadow_tr_fast<false>;
    k.shadowTr[1] = k_shadow_tr<true>; k.shadowTr[0] = k_shadow_tr<false>;
    k.handleEscaped = p.portalLights ? k_handle_escaped<true> : k_handle_escaped<false>;
    k.intersectShadow[1] = anim ? k_intersect_shadow<true, true> : k_intersect_shadow<true, false>;
    k.intersectShadow[0] = anim ? k_intersect_shadow<false, true> : k_intersect_shadow<false, false>;
    k.intersectOneRandom = anim ? k_intersect_one_random<true> : k_intersect_one_random<false>;
    k.traceOneRandom[1] = k_trace_one_random<true>; k.traceOneRandom[0] = k_trace_one_random<false>;
    k.traceClosestRef = k_trace_closest; k.traceAnyRef = k_trace_any; k.traceClosestTimed = k_trace_closest_timed; k.traceAnyTimed = k_trace_any_timed;
    k.packShadowItems = k_pack_shadow_items;
    for (int t = 1; t < WF_MAT_NTYPES; ++t) { k.shade[t] = kMatShade[t][p.shadeVariant[t]]; k.nee[t] = kMatNee[t][p.rareLights]; }
}
// ---- STAGE GRIDS: the resident workgroups of the kernels PickStageKernels chose and of those the pass names itself, asked once per
// process, device and kernel (the answer is a property of the code object and the chip).  Only the kernels this scene launches are
// asked about: a query loads the kernel's code object.  A query that fails — see DESIGN 8 on occupancy queries behind torch's
// initialisation — fails nothing: its error is taken off the thread's state, the site keeps the fixed bound, and "stage_grid_fallbacks"
// of wf_ctx_query counts it.  (Failures are not cached: the next upload asks again.)
static int ResidentPerCU(int device, const void *key, int block, MatResidentFn sibling) {
    static std::mutex mutex;
    static std::map<std::pair<int, const void *>, int> known;
    std::lock_guard<std::mutex> lock(mutex);
    const auto it = known.find({device, key});
    if (it != known.end()) return it->second;
    int perCU = 0;
    const hipError_t e = sibling ? (hipError_t)sibling(&perCU) : hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, key, block, 0);
    if (e != hipSuccess || perCU < 1) { (void)hipGetLastError(); return 0; }
    known[{device, key}] = perCU;
    return perCU;
}
static void PickStageGrids(wf_ctx *ctx, const Switches &sw) {
    const ScenePlan &p = ctx->plan;
    const SceneView &sv = ctx->svHost;
    const StageKernels &k = ctx->stage;
    StageGrids g;
    g.rounds = sw.stageRounds;
    g.cap = sw.stageGridCap;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess) g.nCU = prop.multiProcessorCount;
    else (void)hipGetLastError();
    // a site the scene launches `kernel` at (or, for a material kernel, the kernel `sibling` answers for)
    auto use = [&](int site, bool launched, auto kernel, int block = BLOCK, bool spillRows = false, MatResidentFn sibling = nullptr) {
        if (!launched) return;
        StageGrids::Site &s = g.site[site];
        s.used = true;
        s.block = block;
        s.spillRows = spillRows;
        if (g.rounds > 0 && g.nCU > 0) s.perCU = ResidentPerCU(ctx->device, sibling ? (const void *)sibling : (const void *)kernel, block, sibling);
        if (g.rounds > 0 && s.perCU == 0) ++g.fallbacks;
    };
    // (the condition under which wf_queues_alloc allocates ws.sampleTops)
    use(SITE_SAMPLE_TOPS, sv.sampler.type == WF_SAMPLER_ZSOBOL && 2 * sv.sampler.nBase4Digits <= 32 && !sw.noSampleTops && !sv.haveSubsurface, k_sample_tops);
    use(SITE_CAMERA_RAYS, true, k.genCameraRays);
    use(SITE_RAY_SAMPLES, true, k_gen_ray_samples);
    use(SITE_ROUTE_HITS, p.fastOk, k.routeHits, k.routeBlock);
    use(SITE_RESOLVE_MIX, p.fastOk && sv.haveMix, k.resolveMix);
    use(SITE_INTERSECT_CLOSEST, !p.fastOk, k.intersectClosest[0], BLOCK, true);
    use(SITE_MEDIUM_SAMPLE, sv.haveMedia, k.mediumSample);
    use(SITE_MEDIUM_ROUTE, sv.haveMedia, k.mediumRoute);
    use(SITE_MEDIUM_SCATTER, sv.haveMedia, k.mediumScatter);
    use(SITE_TR_BEGIN, p.trRoute == 2, k_tr_begin);
    use(SITE_TR_SEGMENT, p.trRoute == 2, k.trSegment);
    use(SITE_SHADOW_TR, p.trRoute == 0, k.shadowTr[p.haveAnimated], BLOCK, true);
    use(SITE_HANDLE_ESCAPED, sv.nInfiniteLights > 0, k.handleEscaped);
    use(SITE_HANDLE_EMISSIVE, true, k_handle_emissive);
    use(SITE_INTERSECT_SHADOW, !p.fastOk && !sv.haveMedia, k.intersectShadow[0], BLOCK, true);
    use(SITE_SUBSURFACE_PROBE, sv.haveSubsurface, k_subsurface_probe);
    use(SITE_INTERSECT_ONE_RANDOM, sv.haveSubsurface, k.intersectOneRandom, BLOCK, true);
    use(SITE_SUBSURFACE_SCATTER, sv.haveSubsurface, k_subsurface_scatter);
    for (int t = 1; t < WF_MAT_NTYPES; ++t) {
        use(SITE_SHADE0 + t, p.matPresent[t], (const void *)nullptr, BLOCK, false, kMatShadeResident[t][p.shadeVariant[t]]);
        use(SITE_NEE0 + t, p.matPresent[t], (const void *)nullptr, BLOCK, false, kMatNeeResident[t][p.rareLights]);
    }
    ctx->grids = g;
}
// The workgroups of a launch at `site` over at most n items (StageGrid, wf_plan.h).  `asPicked` = false: the launch is not of the kernel
// PickStageGrids asked about (a counting pass's walk) and takes the fixed bound.
static int StageGridOf(const wf_ctx *ctx, int site, int n, bool asPicked = true) {
    const StageGrids &g = ctx->grids;
    const StageGrids::Site &s = g.site[site];
    const int grid = StageGrid(n, s.block > 0 ? s.block : BLOCK, asPicked ? s.perCU : 0, g.nCU, g.rounds, g.cap);
    return s.spillRows || !asPicked ? std::min(grid, MAX_GRID) : grid;
}
static_assert(STAGE_GRID_BOUND == MAX_GRID, "the fixed bound of StageGrid is this unit's MAX_GRID");

// ---- what the boundary calls (wf_boundary.hip) share with the stage entry points below: declared in wf_ctx.h
namespace wf::backend {
// countStats = false (wf_camera_rays_device): the band's rays are a caller's, not the render's — they stay out of stats->cameraRays
int GenCameraRays(wf_ctx *ctx, int y0, int sample_index, bool countStats) {
    if (int e = checkReady(ctx)) return e;
    ctx->passY0 = y0;
    if (ctx->ws.sampleTops) LAUNCH("Sampler index prefixes", k_sample_tops, StageGridOf(ctx, SITE_SAMPLE_TOPS, 5 * ctx->ws.pixelsPerPass), ctx->svHost, ctx->ws, y0, 0);
    if (ctx->svHost.camera.type == WF_CAMERA_REALISTIC)  // rays blocked by the lenses leave no queue entry: the kernel appends
        LAUNCH("Reset ray queue", k_reset, 1, ctx->ws, 1u << CNT_RAY0, -1, 0);
    LAUNCH("Generate camera rays", ctx->stage.genCameraRays, StageGridOf(ctx, SITE_CAMERA_RAYS, ctx->maxQueueSize), ctx->svHost, ctx->ws, y0, sample_index, ctx->passStep, ctx->passSamples);
    if (countStats) LAUNCH("Update camera ray stats", k_reset, 1, ctx->ws, 0u, STAT_CAMERA, CNT_RAY0);
    return 0;
}
// The transmittance stage's launches over `ws` (n items) by `route` (ScenePlan::trRoute): 2 the wavefront (see k_tr_begin), 1 the per-lane
// production walk (static one-level scenes), 0 the reference-order walk per lane, at the items' times if they carry them (`timed`).
// The one copy of the sequence: the render's stage and wf_trace_shadow_tr_device run it, each over its WorkState and under its own names.
void LaunchTransmittance(wf_ctx *ctx, const WorkState &ws, int n, int route, bool timed, const TrNames &names) {
    if (route == 2) {
        LAUNCH(names.reset, k_reset, 1, ws, (1u << CNT_TR0) | (1u << CNT_TR1), -1, 0);
        LAUNCH(names.begin, k_tr_begin, StageGridOf(ctx, SITE_TR_BEGIN, n), ctx->svHost, ws);
        for (int seg = 0; seg < WF_TR_SEGMENTS; ++seg) {
            const int cur = seg & 1;
            LAUNCHT(names.trace, ctx->walk.trTrace, ctx->walk.grid, ctx->svHost, ws, ctx->fast, cur, ctx->spillArea());
            LAUNCH(names.segment, ctx->stage.trSegment, StageGridOf(ctx, SITE_TR_SEGMENT, n), ctx->svHost, ws, cur);
            LAUNCH(names.reset, k_reset, 1, ws, 1u << (CNT_TR0 + cur), -1, 0);
        }
        LAUNCH(names.rest, ctx->stage.trRest, 128, ctx->svHost, ws, WF_TR_SEGMENTS & 1, ctx->stackSpill);
    } else if (route == 1) LAUNCHT(names.perLane, ctx->stage.shadowTrFast, ctx->walk.grid, ctx->svHost, ws, ctx->fast, ctx->spillArea());
    else LAUNCH(names.perLane, ctx->stage.shadowTr[timed], StageGridOf(ctx, SITE_SHADOW_TR, n, ctx->plan.trRoute == 0 && timed == ctx->plan.haveAnimated), ctx->svHost, ws, ctx->stackSpill);
}
}  // namespace wf::backend

extern "C" {

int wf_abi_version(void) { return WF_ABI_VERSION; }

// The stream's scratch (private segment) grows whenever a kernel needs more per lane than any kernel before it; on about a third of the
// pool's boxes every such growth costs the launch that triggers it 20-30 ms (round 4: the first frame of a process took 200 ms instead of
// 112: "Handle escaped rays" 1264 B, "Handle emitters" 1424 B, conductor 1468 B, coated diffuse 1500 B per lane — four steps in launch
// order).  One launch of a kernel whose private segment is at least the largest of the library's (round 4: the one-kernel material stage of type 7, 3372 B) pays for
// the growth once, when the context is created.  WF_SCRATCH_PRIME=0 skips it.
constexpr int SCRATCH_PRIME_WORDS = 896;   // 3584 B per lane
__global__ void k_scratch_prime(int *out, int n) {
    volatile int buf[SCRATCH_PRIME_WORDS];
    for (int i = 0; i < n; ++i) buf[(i * 131) % SCRATCH_PRIME_WORDS] = i;
    out[threadIdx.x] = buf[(n * 7) % SCRATCH_PRIME_WORDS];
}
// (what wf_ctx_create made so far, or a whole context: null members are skipped)
static void DestroyCtx(wf_ctx *ctx) {
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->stream3) (void)hipStreamSynchronize(ctx->stream3);
    for (void *p : ctx->allocs) (void)hipFree(p);
    for (const wf_ctx::TrScratch::Slot &sl : ctx->trScratch.slots())
        if (*sl.p) (void)hipFree(*sl.p);
    if (ctx->trScratch.counters) (void)hipFree(ctx->trScratch.counters);
    for (auto &e : ctx->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto e : ctx->eventPool) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream3) (void)hipStreamDestroy(ctx->stream3);
    if (ctx->evShadowFork) (void)hipEventDestroy(ctx->evShadowFork);
    if (ctx->evShadowJoin) (void)hipEventDestroy(ctx->evShadowJoin);
    if (ctx->evFork) (void)hipEventDestroy(ctx->evFork);
    if (ctx->evJoin) (void)hipEventDestroy(ctx->evJoin);
    delete ctx;
}
static int InitCtx(wf_ctx *c, const Switches &sw) {
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->evJoin, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->evShadowFork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->evShadowJoin, hipEventDisableTiming));
    c->frameOverlap = sw.frameOverlap;
    c->samplesShaded = sw.samplesShaded;
    c->traceLaunch = sw.traceLaunch;
    if (sw.scratchPrime) {
        DeviceScratch tmp(c->stream);
        int *out = nullptr;
        if (int e = tmp.alloc(&out, (size_t)64)) return e;
        hipLaunchKernelGGL(k_scratch_prime, dim3(1), dim3(64), 0, c->stream, out, 8);
        hipLaunchKernelGGL(k_scratch_prime, dim3(1), dim3(64), 0, c->stream2, out, 8);
        hipLaunchKernelGGL(k_scratch_prime, dim3(1), dim3(64), 0, c->stream3, out, 8);
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipStreamSynchronize(c->stream2));
        HIPCHK(hipStreamSynchronize(c->stream3));
    }
    return 0;
}
int wf_ctx_create(int device, wf_ctx **out) {
    if (!out) return fail(-1, "null out");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(-1, "no HIP device visible: libwfhip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(-1, "device %d out of range (0..%d)", device, ndev - 1);
    HIPCHK(hipSetDevice(device));
    wf_ctx *c = new wf_ctx();
    c->device = device;
    if (int e = InitCtx(c, Switches::FromEnv())) { DestroyCtx(c); return e; }   // (g_err keeps the failing call's message)
    *out = c;
    return 0;
}

int wf_ctx_destroy(wf_ctx *ctx) {
    if (ctx) DestroyCtx(ctx);
    return 0;
}

int wf_sync(wf_ctx *ctx) {
    if (!ctx) return fail(-1, "null context");
    useDevice(ctx);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    if (ctx->dbgWords) {
        int overflow = 0;
        HIPCHK(hipMemcpy(&overflow, ctx->dbgWords + 1, sizeof(int), hipMemcpyDeviceToHost));
        if (overflow) return fail(-1, "traversal stack overflow: a walk needed more than %d + %d node-stack entries (results are incomplete)", TSTACK, ctx->plan.spillRows);
        int unresolved = 0;
        HIPCHK(hipMemcpy(&unresolved, ctx->dbgWords + 6, sizeof(int), hipMemcpyDeviceToHost));
        if (unresolved & 1) return fail(-1, "a near-tie re-walk found no hit where the production walk had one (results are incomplete)");
        if (unresolved & 2) return fail(-1, "a near-tie queue entry failed its validation (ray index, bound or launch tag): results are incomplete");
        int fatal = 0;
        HIPCHK(hipMemcpy(&fatal, ctx->dbgWords + 7, sizeof(int), hipMemcpyDeviceToHost));
        // the reference's LOG_FATAL / CHECK inside a kernel body (wf_scene.h: WF_FATAL_*), e.g. a sample drawn from an emissive curve
        if (fatal) return fail(-1, "%s", FatalMessage(fatal));
        if (getenv("WF_DEBUG_DRAIN")) {
            int h[8];
            HIPCHK(hipMemcpy(h, ctx->dbgWords, sizeof(h), hipMemcpyDeviceToHost));
            fprintf(stderr, "[drain] spilled %d, re-walks %d, pushes %d, repeated re-walks %d, unresolved %d\n", h[0], h[2], h[4], h[5], h[6]);
#if WF_WALK_STATS
            unsigned long long c[16];
            HIPCHK(hipMemcpy(c, ctx->dbgWords + 8, sizeof(c), hipMemcpyDeviceToHost));
            const char *ph[4] = {"interior", "leaf", "transition", "refill"};
            for (int k = 0; k < 2; ++k)
                for (int q = 0; q < 4; ++q)
                    fprintf(stderr, "[walk stats] %s %-26s wave iterations %llu, lanes %llu (%.1f per iteration)\n", k ? "any-hit" : "closest", ph[q], c[k * 8 + 2 * q], c[k * 8 + 2 * q + 1],
                            c[k * 8 + 2 * q] ? (double)c[k * 8 + 2 * q + 1] / (double)c[k * 8 + 2 * q] : 0.0);
#endif
        }
    }
    return 0;
}
void *wf_stream(wf_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

// The first step of the upload after PlanScene: the description's tables, the ones derived from them, and the scalars of SceneView.
// The tables that are copies of the description's arrays are the list WF_SCENE_TABLES (csrc/common/wf_scene_view.h), uploaded in its
// order; the tables with a condition or a derivation of their own are the Upload_<member> steps here, run where the list marks them.
static int Upload_S(wf_ctx *ctx, const wf_scene_desc *d, const Switches &) {
    // (null in a scene without shading tangents)
    return d->n_tangents > 0 ? devUpload(ctx, &ctx->svHost.S, d->S, (size_t)3 * d->n_tangents) : 0;
}
static int Upload_shadeTris(wf_ctx *ctx, const wf_scene_desc *d, const Switches &sw) {
    // the de-indexed per-triangle vertex records of the material stage (wf_scene.h ShadeTri); WF_SHADE_TRIS=0: the indexed tables only
    SceneView &sv = ctx->svHost;
    sv.shadeTris = nullptr;
    if (d->n_triangles > 0 && sw.shadeTris) {
        std::vector<ShadeTri> st((size_t)d->n_triangles);
        for (size_t t = 0; t < (size_t)d->n_triangles; ++t) {
            const int32_t *ix = d->tri_indices + 3 * t;
            const int flags = d->meshes[d->tri_mesh[t]].flags;
            ShadeTri r{};
            for (int k = 0; k < 3; ++k) {
                for (int a = 0; a < 3; ++a) r.p[3 * k + a] = d->P[3 * (size_t)ix[k] + a];
                if ((flags & WF_MESH_HAS_N) && d->N) for (int a = 0; a < 3; ++a) r.n[3 * k + a] = d->N[3 * (size_t)ix[k] + a];
                if ((flags & WF_MESH_HAS_UV) && d->UV) for (int a = 0; a < 2; ++a) r.uv[2 * k + a] = d->UV[2 * (size_t)ix[k] + a];
            }
            st[t] = r;
        }
        const ShadeTri *dst = nullptr;
        if (int e = devUpload(ctx, &dst, st.data(), st.size())) return e;
        HIPCHK(hipStreamSynchronize(ctx->stream));   // (the staging vector dies here)
        sv.shadeTris = dst;
    }
    return 0;
}
static int Upload_lightBvhX(wf_ctx *ctx, const wf_scene_desc *d, const Switches &) {
    // the light BVH's nodes with their per-node constants expanded (wf_lights.h ExpandLightNode: the reference's own expressions, evaluated
    // once here instead of at every visit of every descent)
    std::vector<wf::LightNodeX> xs((size_t)d->n_light_bvh_nodes);
    for (int i = 0; i < d->n_light_bvh_nodes; ++i) xs[i] = wf::ExpandLightNode(d->all_light_bounds, d->light_bvh_nodes[i]);
    return devUpload(ctx, &ctx->svHost.lightBvhX, xs.data(), xs.size());
}
static int Upload_gridCorners(wf_ctx *ctx, const wf_scene_desc *d, const Switches &sw) {
    // the corner-packed copies of the GridMedium density grids (SceneView::gridCorners), built on the device from the dense grids
    // just uploaded.  WF_GRID_CORNERS=0: none (A/B); tables beyond WF_GRID_CORNERS_GB (default 32) gigabytes in all are left out
    SceneView &sv = ctx->svHost;
    int e = 0;
    sv.gridCorners = nullptr;
    sv.gridCornerBase = nullptr;
    if (d->n_media > 0 && sw.gridCorners) {
        const double budget = sw.gridCornersGB * 1024.0 * 1024.0 * 1024.0;
        std::vector<long long> base(d->n_media, -1);
        size_t total = 0;
        for (int m = 0; m < d->n_media; ++m) {
            const wf_medium &M = d->media[m];
            if (M.type != WF_MEDIUM_GRID || M.density_offset < 0 || M.nx < 1 || M.ny < 1 || M.nz < 1) continue;
            const size_t cells = wf::GridCornerCells(M.nx, M.ny, M.nz);
            if ((double)(total + 8 * cells) * sizeof(float) > budget) continue;
            base[m] = (long long)total;
            total += 8 * cells;
        }
        if (total > 0) {
            float *corners = nullptr;
            const long long *dbase = nullptr;
            if ((e = devAlloc(ctx, &corners, total))) return e;
            if ((e = devUpload(ctx, &dbase, base.data(), (size_t)d->n_media))) return e;
            for (int m = 0; m < d->n_media; ++m) {
                if (base[m] < 0) continue;
                const wf_medium &M = d->media[m];
                const size_t cells = (size_t)(M.nx + 1) * (M.ny + 1) * (M.nz + 1);
                const int grid = (int)std::min<size_t>((cells + BLOCK - 1) / BLOCK, (size_t)MAX_GRID * 16);
                LAUNCH("Pack grid corners", k_pack_grid_corners, grid, sv.mediumData + M.density_offset, M.nx, M.ny, M.nz, corners + base[m]);
            }
            sv.gridCorners = corners;
            sv.gridCornerBase = dbase;
        }
    }
    return 0;
}
static int Upload_sobol(wf_ctx *ctx, const wf_scene_desc *, const Switches &) {
    // (filled once per process: uploads of several contexts run on several threads)
    static const std::vector<uint32_t> sobol = [] { std::vector<uint32_t> t(WF_SOBOL_WORDS); FillSobol2D(t.data()); return t; }();
    return devUpload(ctx, &ctx->svHost.sobol, sobol.data(), sobol.size());
}
static int UploadTables(wf_ctx *ctx, const wf_scene_desc *d, const Switches &sw) {
    SceneView &sv = ctx->svHost;
    const int64_t nBvhPrims = ctx->plan.nBvhPrims;
    int e = 0;
#define UPLOAD(member, table, count) if ((e = devUpload(ctx, &sv.member, d->table, count))) return e;
#define STEP(member) if ((e = Upload_##member(ctx, d, sw))) return e;
    WF_SCENE_TABLES(UPLOAD, STEP)
#undef UPLOAD
#undef STEP
    SetSceneScalars(&sv, *d, ctx->plan);
    return 0;
}
// ... then the traversal stacks, the production trees and the kernels that walk them
static int UploadTraversal(wf_ctx *ctx, const FastTrees &trees, const Switches &sw) {
    const ScenePlan &plan = ctx->plan;
    int e = 0;
    if ((e = devAlloc(ctx, &ctx->stackSpill, (size_t)plan.spillRows * MAX_GRID * BLOCK))) return e;
    if ((e = devAlloc(ctx, &ctx->dbgWords, (size_t)8 + 32))) return e;   // [8..39]: -DWF_WALK_STATS builds: sixteen 64-bit phase counters (WalkStats)   // [4..7]: near-tie queue diagnostics (pushes, re-walks without a hit, -, -)
    HIPCHK(hipMemset(ctx->dbgWords, 0, (8 + 32) * sizeof(int)));
    ctx->fast = trees.header;
    if (plan.fastBuilt) {
        if ((e = devUpload(ctx, &ctx->fast.nodes, trees.nodes.data(), trees.nodes.size()))) return e;
        if ((e = devUpload(ctx, &ctx->fast.tris, trees.tris.data(), trees.tris.size()))) return e;
        if ((e = devUpload(ctx, &ctx->fast.defs, trees.defs.data(), trees.defs.size()))) return e;
        if ((e = devUpload(ctx, &ctx->fast.subs, trees.subs.data(), trees.subs.size()))) return e;
        ctx->fast.instances = ctx->svHost.instances;
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    if ((e = PickWalkKernels(ctx))) return e;
    PickStageKernels(ctx);
    PickStageGrids(ctx, sw);
    if ((e = devAlloc(ctx, &ctx->probeCursor, (size_t)1))) return e;
    // the walk on stream3 pushes into spill rows of its own: a column is indexed by the global thread, which both walks have
    if (FrameOverlapScene(ctx) && (e = devAlloc(ctx, &ctx->stackSpill2, (size_t)plan.spillRows * MAX_GRID * BLOCK))) return e;
    return 0;
}
// ... and the film, the counters and the device copy of SceneView
static int UploadFilmAndView(wf_ctx *ctx, const wf_scene_desc *d) {
    int e = 0;
    ctx->W = d->film.pixel_max[0] - d->film.pixel_min[0];
    ctx->H = d->film.pixel_max[1] - d->film.pixel_min[1];
    ctx->maxDepth = d->max_depth;
    for (int i = 0; i < 6; ++i) ctx->sceneBounds[i] = d->scene_bounds[i];
    if ((e = devAlloc(ctx, &ctx->ws.film, (size_t)ctx->W * ctx->H * 4))) return e;
    ctx->ws.filmSpectral = nullptr;
    ctx->ws.filmGBuffer = nullptr;
    if (d->film.type == WF_FILM_GBUFFER && (e = devAlloc(ctx, &ctx->ws.filmGBuffer, (size_t)ctx->W * ctx->H))) return e;
    if (d->film.type == WF_FILM_SPECTRAL && (e = devAlloc(ctx, &ctx->ws.filmSpectral, (size_t)ctx->W * ctx->H * 2 * d->film.n_buckets))) return e;
    if ((e = devAlloc(ctx, &ctx->ws.stats, (size_t)STAT_COUNT))) return e;
    if ((e = devAlloc(ctx, &ctx->ws.trav, (size_t)8))) return e;
    if ((e = devAlloc(ctx, &ctx->ws.counters, (size_t)CNT_COUNT * CNT_STRIDE))) return e;
    SceneView *dev = nullptr;
    if ((e = devAlloc(ctx, &dev, (size_t)1))) return e;
    ctx->svHost.self = dev;  // the device copy points at itself: the address the out-of-line device functions are given
    ctx->svHost.fatal = ctx->dbgWords + 7;   // RaiseFatal (wf_scene.h): reported by wf_sync
    HIPCHK(hipMemcpyAsync(dev, &ctx->svHost, sizeof(SceneView), hipMemcpyHostToDevice, ctx->stream));
    ctx->svDev = dev;
    ctx->fast.sv = ctx->svDev;
    HIPCHK(hipStreamSynchronize(ctx->stream));  // (the copies above read host memory that the caller and this call own)
    return 0;
}
int wf_scene_upload(wf_ctx *ctx, const wf_scene_desc *d) {
    if (!ctx || !d) return fail(-1, "null argument");
    if (int e = CheckAbi(d)) return e;   // (before the context's own state: a foreign description is reported as such)
    if (ctx->sceneLoaded) return fail(-1, "a scene is already uploaded to this context");
    const Switches sw = Switches::FromEnv();
    ScenePlan plan;
    FastTrees trees;
    if (int e = PlanScene(d, sw, &plan, &trees)) return e;   // (nothing is allocated before the description has passed)
    HIPCHK(hipSetDevice(ctx->device));
    // a step that fails below takes back what this call allocated and puts the scene state back to its defaults (W, H, maxDepth and
    // sceneBounds keep what UploadFilmAndView wrote: nothing reads them while sceneLoaded is false, and the next upload sets them)
    struct Rollback {
        wf_ctx *ctx;
        size_t nAllocs;
        bool done = false;
        ~Rollback() {
            if (done) return;
            (void)hipStreamSynchronize(ctx->stream);
            for (size_t i = nAllocs; i < ctx->allocs.size(); ++i) (void)hipFree(ctx->allocs[i]);
            ctx->allocs.resize(nAllocs);
            ctx->svHost = SceneView{};
            ctx->svDev = nullptr;
            ctx->ws = WorkState{};
            ctx->fast = FastBVH{};
            ctx->walk = WalkKernels{};
            ctx->stage = StageKernels{};
            ctx->grids = StageGrids{};
            ctx->plan = ScenePlan{};
            ctx->stackSpill = ctx->stackSpill2 = ctx->dbgWords = nullptr;
            ctx->probeCursor = nullptr;
        }
    } rollback{ctx, ctx->allocs.size()};
    ctx->plan = plan;
    int e;
    if ((e = UploadTables(ctx, d, sw)) || (e = UploadTraversal(ctx, trees, sw)) || (e = UploadFilmAndView(ctx, d))) return e;
    rollback.done = true;
    ctx->sceneLoaded = true;
    return 0;
}
int wf_ctx_query(wf_ctx *ctx, const char *key, int64_t *value) {
    if (!ctx || !key || !value) return fail(-1, "wf_ctx_query: null argument");
    if (!ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    const std::string k = key;
    if (PlanValue(ctx->plan, key, value)) return 0;
    if (k == "frame_overlap_active") *value = FrameOverlapActive(ctx);
    else if (k == "frame_overlap_mode") *value = ctx->frameOverlap;
    else if (k == "skip_last_samples") *value = SkipLastSamples(ctx);
    else if (k == "pixels_per_pass") *value = ctx->queuesAllocated ? ctx->ws.pixelsPerPass : 0;   // the rays a band holds per sample index (wf_camera_rays_device's n_max)
    else if (k == "shade_tris") *value = (const ShadeTri *)ctx->svHost.shadeTris != nullptr;   // the de-indexed vertex records are uploaded (0: WF_SHADE_TRIS=0, the indexed tables only)
    else if (k == "stage_rounds") *value = ctx->grids.rounds;
    else if (k == "stage_grid_cap") *value = ctx->grids.cap;
    else if (k == "stage_grid_fallbacks") *value = ctx->grids.fallbacks;
    else if (k == "stage_grid_sites") *value = SITE_COUNT;
    else if (k.compare(0, 6, "stage_") == 0 && k.find_first_of("0123456789") != std::string::npos && k.find_first_not_of("0123456789", k.find_first_of("0123456789")) == std::string::npos) {
        // per launch site of the render pass (StageSite's order; -1: the scene launches nothing there): "stage_grid_<site>" the workgroups
        // of its launches, "stage_need_<site>" one workgroup per `block` items of the full queue, "stage_resident_<site>" the workgroups
        // the chip keeps resident of its kernel (0: not known, the site keeps the fixed bound)
        const size_t digits = k.find_first_of("0123456789");
        const std::string what = k.substr(0, digits);
        const int site = atoi(k.c_str() + digits);
        if (site < 0 || site >= SITE_COUNT || (what != "stage_grid_" && what != "stage_need_" && what != "stage_resident_")) return fail(-1, "wf_ctx_query: unknown key '%s'", key);
        const StageGrids::Site &s = ctx->grids.site[site];
        const int n = site == SITE_SAMPLE_TOPS ? 5 * ctx->ws.pixelsPerPass : ctx->maxQueueSize;
        if (!s.used || (site == SITE_SAMPLE_TOPS && ctx->queuesAllocated && !ctx->ws.sampleTops)) *value = -1;
        else if (what == "stage_resident_") *value = (int64_t)s.perCU * ctx->grids.nCU;
        else if (!ctx->queuesAllocated) *value = 0;
        else if (what == "stage_grid_") *value = StageGridOf(ctx, site, n);
        else *value = (n + s.block - 1) / s.block;
    }
    else return fail(-1, "wf_ctx_query: unknown key '%s'", key);
    return 0;
}

int wf_aggregate_bounds(wf_ctx *ctx, float out_bounds[6]) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    for (int i = 0; i < 6; ++i) out_bounds[i] = ctx->sceneBounds[i];
    return 0;
}

static int allocRayQueue(wf_ctx *c, RayQueueV *q, size_t n) {
    int e;
    if ((e = devAlloc(c, &q->o, n)) || (e = devAlloc(c, &q->d, n)) || (e = devAlloc(c, &q->beta, n)) || (e = devAlloc(c, &q->r_u, n)) ||
        (e = devAlloc(c, &q->r_l, n)) || (e = devAlloc(c, &q->ctx0, n)) || (e = devAlloc(c, &q->ctx1, n)) || (e = devAlloc(c, &q->ctx2, n)) ||
        (e = devAlloc(c, &q->meta, n)))
        return e;
    return 0;
}

int wf_queues_alloc(wf_ctx *ctx, int pixels_per_pass, int samples_per_pass) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    if (ctx->queuesAllocated) return fail(-1, "queues already allocated");
    if (pixels_per_pass <= 0 || samples_per_pass <= 0) return fail(-1, "pixels_per_pass and samples_per_pass must be positive");
    if ((long long)pixels_per_pass * samples_per_pass > (1ll << 30)) return fail(-1, "queue capacity %lld too large", (long long)pixels_per_pass * samples_per_pass);
    if (pixels_per_pass % ctx->W != 0) return fail(-1, "pixels_per_pass must be a whole number of scanlines (width %d)", ctx->W);
    HIPCHK(hipSetDevice(ctx->device));
    const int max_queue_size = pixels_per_pass * samples_per_pass;
    const size_t n = (size_t)max_queue_size;
    WorkState &ws = ctx->ws;
    ws.maxQueueSize = max_queue_size;
    ws.pixelsPerPass = pixels_per_pass;
    ws.samplesPerPass = samples_per_pass;
    if (ws.stripCount < 1) { ws.stripRank = 0; ws.stripCount = 1; ws.stripHeight = 1; ws.localRows = ctx->H; }
    ctx->passSamples = 1;
    const Switches sw = Switches::FromEnv();
    // (pixelMajor is set by its switch alone, and an unset switch gives wf_ctx's own default)
    ctx->pixelMajor = sw.pixelMajor;
    ctx->ws.slotStride = ctx->pixelMajor ? 1 : 0;
    ctx->passStep = 1;
    int e;
    if ((e = devAlloc(ctx, &ws.filterWeight, n)) || (e = devAlloc(ctx, &ws.pPixel, n)) || (e = devAlloc(ctx, &ws.lambda, n)) ||
        (e = devAlloc(ctx, &ws.lambdaPdf, n)) || (e = devAlloc(ctx, &ws.L, n)) || (e = devAlloc(ctx, &ws.cameraRayWeight, n)) ||
        (e = devAlloc(ctx, &ws.samples0, n)) || (e = devAlloc(ctx, &ws.samples1, n)))
        return e;
    if (ctx->svHost.film.type == WF_FILM_GBUFFER &&
        ((e = devAlloc(ctx, &ws.vsP, n)) || (e = devAlloc(ctx, &ws.vsN, n)) || (e = devAlloc(ctx, &ws.vsNs, n)) || (e = devAlloc(ctx, &ws.vsDpdx, n)) ||
         (e = devAlloc(ctx, &ws.vsDpdy, n)) || (e = devAlloc(ctx, &ws.vsAlbedo, n))))
        return e;
    // pixel-only sample-index digits (wf_camera.h TopDigits): usable while the permuted index fits 32 bits
    ws.sampleTops = nullptr;
    if (ctx->svHost.sampler.type == WF_SAMPLER_ZSOBOL && 2 * ctx->svHost.sampler.nBase4Digits <= 32 && !sw.noSampleTops &&
        !ctx->svHost.haveSubsurface)  // (K12 scenes draw 10 dimensions per depth, not 7)
        if ((e = devAlloc(ctx, &ws.sampleTops, (size_t)5 * pixels_per_pass))) return e;
    if ((e = allocRayQueue(ctx, &ws.rq[0], n)) || (e = allocRayQueue(ctx, &ws.rq[1], n))) return e;
    if (ctx->svHost.haveMedia) {
        if ((e = devAlloc(ctx, &ws.trO, n)) || (e = devAlloc(ctx, &ws.trD, n)) || (e = devAlloc(ctx, &ws.trT, n)) || (e = devAlloc(ctx, &ws.trRu, n)) ||
            (e = devAlloc(ctx, &ws.trRl, n)) || (e = devAlloc(ctx, &ws.trRng, n)) || (e = devAlloc(ctx, &ws.trQ[0], n)) || (e = devAlloc(ctx, &ws.trQ[1], n)))
            return e;
        if ((e = devAlloc(ctx, &ws.hitT, n)) || (e = devAlloc(ctx, &ws.mediumSampleQ, n)) || (e = devAlloc(ctx, &ws.mediumScatterQ, n)) || (e = devAlloc(ctx, &ws.mediumRouteQ, n)) ||
            (e = devAlloc(ctx, &ws.scatterP, n)) || (e = devAlloc(ctx, &ws.sq.medium, n)))
            return e;
    }
    if (ctx->svHost.haveMix && ((e = devAlloc(ctx, &ws.mixMat, n)) || (e = devAlloc(ctx, &ws.mixQ, n)))) return e;
    if (ctx->svHost.haveSubsurface && ((e = devAlloc(ctx, &ws.samples2, n)) || (e = devAlloc(ctx, &ws.bssrdfQ, n)) || (e = devAlloc(ctx, &ws.sssQ, n)))) return e;
    if ((e = devAlloc(ctx, &ws.hit, n)) || (e = devAlloc(ctx, &ws.escapedQ, n)) || (e = devAlloc(ctx, &ws.hitLightQ, n)) || (e = devAlloc(ctx, &ws.retraceQ, n)) || (e = devAlloc(ctx, &ws.retraceQ64, n))) return e;
    if ((e = devAlloc(ctx, &ws.deferQ, n))) return e;
    if (ctx->stackSpill2 && ctx->walk.shadowGen && (e = devAlloc(ctx, &ctx->deferQShadow, n))) return e;
    HIPCHK(hipMemset(ws.retraceQ64, 0xff, (size_t)n * sizeof(unsigned long long)));   // every slot "not yet written"
    if (ctx->svHost.nInstances > 0 && (e = devAlloc(ctx, &ws.hitInst, n))) return e;
    for (int m = 0; m < WF_MAT_NTYPES; ++m)
        if ((e = devAlloc(ctx, &ws.matQ[m], ctx->plan.matPresent[m] ? n : (size_t)1))) return e;  // workqueue.h:152-155
    if ((e = devAlloc(ctx, &ws.sq.o, n)) || (e = devAlloc(ctx, &ws.sq.d, n)) || (e = devAlloc(ctx, &ws.sq.Ld, n)) ||
        (e = devAlloc(ctx, &ws.sq.r_u, n)) || (e = devAlloc(ctx, &ws.sq.r_l, n)))
        return e;
    if (ctx->svHost.haveAnimated && (e = devAlloc(ctx, &ws.pathTime, n))) return e;   // the paths' times, for the shadow rays (AnimatedPrimitive)
    {
        // the NeeItems between the material stage's two kernels: as many 16-byte planes as the widest record of the material types present
        int planes = 0;
        for (int m = 1; m < WF_MAT_NTYPES; ++m) if (ctx->plan.matPresent[m]) planes = std::max(planes, NeePlanes(m));
        if (planes > 0 && (e = devAlloc(ctx, &ws.neeRec, n * (size_t)planes))) return e;
    }
    if ((e = devAlloc(ctx, &ws.routeCode, n))) return e;
    ctx->maxQueueSize = max_queue_size;
    ctx->queuesAllocated = true;
    return 0;
}

// sample indices carried by the following passes: sample_index, sample_index + sample_step, ... (n_samples of
// them, n_samples <= samples_per_pass of wf_queues_alloc)
int wf_set_pass_samples(wf_ctx *ctx, int sample_step, int n_samples) {
    if (int e = checkReady(ctx)) return e;
    if (n_samples < 1 || n_samples > ctx->ws.samplesPerPass) return fail(-1, "n_samples %d outside 1..%d", n_samples, ctx->ws.samplesPerPass);
    if (sample_step < 1) return fail(-1, "sample_step must be >= 1");
    ctx->passStep = sample_step;
    ctx->passSamples = n_samples;
    ctx->ws.slotStride = ctx->pixelMajor ? n_samples : 0;
    return 0;
}

int wf_set_strips(wf_ctx *ctx, int rank, int count, int height, int *local_rows) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    if (count < 1 || rank < 0 || rank >= count || height < 1) return fail(-1, "wf_set_strips: rank %d of %d, height %d", rank, count, height);
    int rows = 0;
    for (int y = 0; y < ctx->H; ++y) rows += (y / height) % count == rank;
    ctx->ws.stripRank = rank; ctx->ws.stripCount = count; ctx->ws.stripHeight = height; ctx->ws.localRows = count > 1 ? rows : ctx->H;
    if (local_rows) *local_rows = ctx->ws.localRows;
    return 0;
}

int wf_film_clear(wf_ctx *ctx) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    HIPCHK(hipMemsetAsync(ctx->ws.film, 0, (size_t)ctx->W * ctx->H * 4 * sizeof(double), ctx->stream));
    if (ctx->ws.filmGBuffer) HIPCHK(hipMemsetAsync(ctx->ws.filmGBuffer, 0, (size_t)ctx->W * ctx->H * sizeof(wf_gbuffer_pixel), ctx->stream));
    if (ctx->ws.filmSpectral) HIPCHK(hipMemsetAsync(ctx->ws.filmSpectral, 0, (size_t)ctx->W * ctx->H * 2 * ctx->svHost.film.n_buckets * sizeof(double), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->ws.stats, 0, STAT_COUNT * sizeof(unsigned long long), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->ws.trav, 0, 8 * sizeof(unsigned long long), ctx->stream));
    return 0;
}

int wf_reset_ray_queue(wf_ctx *ctx, int which) {
    if (int e = checkReady(ctx)) return e;
    LAUNCH("Reset ray queue", k_reset, 1, ctx->ws, 1u << (CNT_RAY0 + (which & 1)), -1, 0);
    return 0;
}
int wf_reset_stage_queues(wf_ctx *ctx, int depth) {
    if (int e = checkReady(ctx)) return e;
    const int cur = depth & 1;
    constexpr unsigned matBits = ((1u << WF_MAT_NTYPES) - 1u) << CNT_MAT0;   // every material queue
    constexpr unsigned stageMask = (1u << CNT_ESCAPED) | (1u << CNT_HITLIGHT) | matBits |
        (1u << CNT_MEDIUM_SAMPLE) | (1u << CNT_MEDIUM_SCATTER) | (1u << CNT_MIX) | (1u << CNT_RETRACE) | (1u << CNT_BSSRDF) | (1u << CNT_SSS) |
        (1u << CNT_RETRACE_HEAD) | (1u << CNT_WAVES_DONE) | (1u << CNT_CURSOR) | (1u << CNT_MEDIUM_ROUTE) | (1u << CNT_DEFER) | (1u << CNT_CURSOR_MEDIUM);
    static_assert((stageMask & ((1u << CNT_SHADOW) | (1u << CNT_CURSOR_SHADOW) | (1u << CNT_DEFER_SHADOW))) == 0 && CNT_SHADOW != CNT_RAY0 && CNT_SHADOW != CNT_RAY1,
                  "the stage reset must not zero a counter of the shadow stage, which may be running beside it");
    const unsigned mask = stageMask | (1u << (CNT_RAY0 + (cur ^ 1)));
    // (NOT in the mask, and not to be: CNT_SHADOW, CNT_CURSOR_SHADOW, CNT_DEFER_SHADOW — in the fused pass the previous depth's shadow stage
    //  may still be running on stream3 when this launch executes; it owns those three and zeroes them itself ("Reset shadowRayQueue").
    //  The stats slots differ too: [STAT_INDIRECT + depth] here, [STAT_SHADOW + depth] there, [STAT_ITEMS ..] here only.)
    // stats->indirectRays[depth] += queue size (integrator.cpp:411-414)
    LAUNCH("Reset queues before tracing rays", k_reset, 1, ctx->ws, mask, STAT_INDIRECT + statDepth(depth), CNT_RAY0 + cur);
    ctx->cursorDirty[0] = false;
    return 0;
}
int wf_gen_camera_rays(wf_ctx *ctx, int y0, int sample_index) { return GenCameraRays(ctx, y0, sample_index, true); }
int wf_gen_ray_samples(wf_ctx *ctx, int depth, int sample_index) {
    if (int e = checkReady(ctx)) return e;
    // the pixel-only digits of the sample-index permutation, once per pixel and dimension instead of once per ray
    // (needs the band of the pass: the y0 of the last wf_gen_camera_rays)
    const bool tops = ctx->ws.sampleTops != nullptr && ctx->passY0 != INT_MIN;
    if (tops) LAUNCH("Sampler index prefixes", k_sample_tops, StageGridOf(ctx, SITE_SAMPLE_TOPS, 5 * ctx->ws.pixelsPerPass), ctx->svHost, ctx->ws, ctx->passY0, 6 + 7 * depth);
    LAUNCH("Generate ray samples - ZSobolSampler", k_gen_ray_samples, StageGridOf(ctx, SITE_RAY_SAMPLES, ctx->maxQueueSize), ctx->svHost, ctx->ws, depth & 1, sample_index, ctx->passStep,
           tops ? depth : -1);
    return 0;
}
static int JoinRetrace(wf_ctx *ctx) {
    if (!ctx->retracePending) return 0;
    HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->evJoin, 0));
    ctx->retracePending = false;
    return 0;
}
int wf_intersect_closest(wf_ctx *ctx, int depth) {
    if (int e = checkReady(ctx)) return e;
    // counting on: the reference-order walk (its visit counts define the algorithmic bytes); otherwise the production traversal (wf_traverse.h)
    if (!ctx->countTraversal && ctx->plan.fastOk) {
        const WalkKernels &k = ctx->walk;
        // the work cursor starts at 0: zeroed by the stage's "Reset queues" launch (wf_reset_stage_queues) — a memset node of its own
        // cost a launch's latency per traversal launch (139 fillBuffer launches, 6 ms, in three renders of the spec scene, round 4);
        // only a caller that launches twice without that reset in between pays for one here
        int *cursor = ctx->ws.counters + CNT_CURSOR * CNT_STRIDE;
        if (ctx->cursorDirty[0]) HIPCHK(hipMemsetAsync(cursor, 0, sizeof(int), ctx->stream));
        ctx->cursorDirty[0] = true;
        ctx->ws.drainEpoch = (ctx->ws.drainEpoch + 1) & 0x7fffffff;   // tag of this launch's near-tie queue entries (DrainRetrace)
        if (ctx->ws.drainEpoch == 0) ctx->ws.drainEpoch = 1;
        if (k.closestGen) {
            // TWO-CLASS TRAVERSAL: every ray through the triangle kernel; the rays it hands over (deferQ) through the general kernel
            // (the triangle kernels know one near-tie band: the triangles' own, 2^-20 — the scene-wide band of FastBVH is the wide one of
            //  the pairs that involve a quadric, which only the general kernel's rays can meet)
            FastBVH triFast = ctx->fast;
            triFast.absBand = triFast.absBandTri; triFast.tieRel = triFast.tieRelTri;
            LAUNCHT("Intersect closest", k.closest, k.grid, ctx->svHost, ctx->ws, triFast, depth & 1, ctx->spillArea(), cursor, ctx->plan.cursorChunk, (const int *)nullptr);
            LAUNCHT("Intersect closest: rays that met a general primitive", k.closestGen, k.gridGen, ctx->svHost, ctx->ws, ctx->fast, depth & 1, ctx->spillArea(), (int *)nullptr, ctx->plan.cursorChunk, (const int *)ctx->ws.deferQ);
        } else
            LAUNCHT("Intersect closest", k.closest, k.grid, ctx->svHost, ctx->ws, ctx->fast, depth & 1, ctx->spillArea(), cursor, ctx->plan.cursorChunk, (const int *)nullptr);
        // The near-tie re-trace of the scenes whose walk does not resolve its ties itself (genMode >= 2: quadrics, curves, texture-graph
        // alpha; RetraceInline) is a handful of long single walks: it runs on a second stream beside the routing pass (and, in the
        // fused pass, the next sample-generation launch) — they touch disjoint rays and share only the queue counters, through
        // atomics — and the main stream waits for it before anything consumes the queues.
        const bool overlap = !RetraceInline(ctx->plan.genMode) && ctx->profile != 1 && !ctx->traceLaunch;   // (the full per-stage profile times every launch on the main stream)
        if (overlap) {
            HIPCHK(hipEventRecord(ctx->evFork, ctx->stream));
            HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->evFork, 0));
            hipLaunchKernelGGL(k_closest_retrace, dim3(128), dim3(BLOCK), 0, ctx->stream2, ctx->svHost, ctx->ws, depth & 1, ctx->stackSpill);   // (beside it no walk uses these rows: its own closest-hit launch is done, and the previous depth's any-hit walk, which may still run on stream3, pushes into stackSpill2 — FRAME SCHEDULING)
            HIPCHK(hipEventRecord(ctx->evJoin, ctx->stream2));
            ctx->retracePending = true;
        }
        const int rb = ctx->stage.routeBlock;
        LAUNCHB_ON(ctx->stream, "Route hits", ctx->stage.routeHits, StageGridOf(ctx, SITE_ROUTE_HITS, ctx->maxQueueSize), rb, ctx->svHost, ctx->ws, depth & 1);
        if (ctx->retracePending) {
            if (ctx->deferJoin) return 0;   // the fused pass joins after its sample-generation launch (JoinRetrace)
            if (int e = JoinRetrace(ctx)) return e;
        } else if (!RetraceInline(ctx->plan.genMode))
            LAUNCH("Intersect closest: near-tie re-trace", k_closest_retrace, 128, ctx->svHost, ctx->ws, depth & 1, ctx->stackSpill);
        if (ctx->svHost.haveMix) LAUNCH("Resolve MixMaterial hits", ctx->stage.resolveMix, StageGridOf(ctx, SITE_RESOLVE_MIX, ctx->maxQueueSize), ctx->svHost, ctx->ws, depth & 1);
    } else
        LAUNCH("Intersect closest", ctx->stage.intersectClosest[ctx->countTraversal], StageGridOf(ctx, SITE_INTERSECT_CLOSEST, ctx->maxQueueSize, !ctx->countTraversal), ctx->svHost, ctx->ws, depth & 1, ctx->stackSpill);
    return 0;
}
// SampleMediumInteraction (wavefront/media.cpp:22-257): K5, then K6 for the Henyey-Greenstein phase function
int wf_medium_sample(wf_ctx *ctx, int depth) {
    if (int e = checkReady(ctx)) return e;
    if (!ctx->svHost.haveMedia) return 0;
    LAUNCH("Sample medium interaction", ctx->stage.mediumSample, StageGridOf(ctx, SITE_MEDIUM_SAMPLE, ctx->maxQueueSize), ctx->svHost, ctx->ws, depth & 1);
    LAUNCH("Sample medium interaction: route surface hits", ctx->stage.mediumRoute, StageGridOf(ctx, SITE_MEDIUM_ROUTE, ctx->maxQueueSize), ctx->svHost, ctx->ws, depth & 1);
    if (depth == ctx->maxDepth) return 0;
    LAUNCH("Sample direct/indirect - Henyey-Greenstein", ctx->stage.mediumScatter, StageGridOf(ctx, SITE_MEDIUM_SCATTER, ctx->maxQueueSize), ctx->svHost, ctx->ws, depth & 1);
    return 0;
}
// TraceShadowRays with media: IntersectShadowTr (wavefront/aggregate.cpp:70-88, intersect.h:165-274)
int wf_intersect_shadow_tr(wf_ctx *ctx, int depth) {
    if (int e = checkReady(ctx)) return e;
    if (!ctx->svHost.haveMedia) return fail(-1, "wf_intersect_shadow_tr: the scene has no media (use wf_intersect_shadow)");
    LaunchTransmittance(ctx, ctx->ws, ctx->maxQueueSize, ctx->countTraversal ? 0 : ctx->plan.trRoute, ctx->plan.haveAnimated,   // (a counting pass keeps the reference-order walk)
                        {"Reset transmittance queues", "Intersect shadow (Tr): begin", "Intersect shadow (Tr): trace", "Intersect shadow (Tr): segment",
                         "Intersect shadow (Tr): rest", "Intersect shadow (Tr)"});
    LAUNCH("Reset shadowRayQueue", k_reset, 1, ctx->ws, (1u << CNT_SHADOW), STAT_SHADOW + statDepth(depth), CNT_SHADOW);
    return 0;
}
int wf_handle_escaped(wf_ctx *ctx, int depth) {
    if (int e = checkReady(ctx)) return e;
    if (ctx->svHost.nInfiniteLights == 0) return 0;  // escapedRayQueue == nullptr (integrator.cpp:496-497)
    LAUNCH("Handle escaped rays", ctx->stage.handleEscaped, StageGridOf(ctx, SITE_HANDLE_ESCAPED, ctx->maxQueueSize), ctx->svHost, ctx->ws, depth & 1);
    return 0;
}
int wf_handle_emissive(wf_ctx *ctx, int depth) {
    if (int e = checkReady(ctx)) return e;
    LAUNCH("Handle emitters hit by indirect rays", k_handle_emissive, StageGridOf(ctx, SITE_HANDLE_EMISSIVE, ctx->maxQueueSize), ctx->svHost, ctx->ws, depth & 1);
    return 0;
}
static int EvalMaterial(wf_ctx *ctx, int material_type, int depth) {
    const int cur = depth & 1;
    static const char *names[WF_MAT_NTYPES] = {"", "DiffuseMaterial + BxDF eval (Basic tex)", "ConductorMaterial + BxDF eval (Basic tex)",
                                               "DielectricMaterial + BxDF eval (Basic tex)", "ThinDielectricMaterial + BxDF eval (Basic tex)",
                                               "DiffuseTransmissionMaterial + BxDF eval (Basic tex)", "CoatedDiffuseMaterial + BxDF eval (Basic tex)",
                                               "CoatedConductorMaterial + BxDF eval (Basic tex)", "SubsurfaceMaterial + BxDF eval (Basic tex)", "HairMaterial + BxDF eval (Basic tex)",
                                               "MeasuredMaterial + BxDF eval (Basic tex)"};
    if (material_type == WF_MAT_INTERFACE) return 0;
    if (material_type < 0 || material_type >= WF_MAT_NTYPES) return fail(-1, "material type %d has no HIP kernel", material_type);
    // the two halves (wf_kernels.h MatShade / MatNee; the items' NeeItems stay in ws.neeRec between them), in the plan's variants (shadeVariant, rareLights)
    { Prof prof_(ctx, names[material_type]); ctx->stage.shade[material_type](ctx->stream, StageGridOf(ctx, SITE_SHADE0 + material_type, ctx->maxQueueSize), &ctx->svHost, &ctx->ws, cur); }
    static const char *neeNames[WF_MAT_NTYPES] = {"", "DiffuseMaterial: next-event estimation", "ConductorMaterial: next-event estimation", "DielectricMaterial: next-event estimation",
                                                  "ThinDielectricMaterial: next-event estimation", "DiffuseTransmissionMaterial: next-event estimation",
                                                  "CoatedDiffuseMaterial: next-event estimation", "CoatedConductorMaterial: next-event estimation",
                                                  "SubsurfaceMaterial: next-event estimation", "HairMaterial: next-event estimation", "MeasuredMaterial: next-event estimation"};
    { Prof prof_(ctx, neeNames[material_type]); ctx->stage.nee[material_type](ctx->stream, StageGridOf(ctx, SITE_NEE0 + material_type, ctx->maxQueueSize), &ctx->svHost, &ctx->ws); }
    return 0;
}
int wf_eval_material(wf_ctx *ctx, int material_type, int depth) {
    if (int e = checkReady(ctx)) return e;
    return EvalMaterial(ctx, material_type, depth);
}
// The material stage of one depth: every type present, one after the other on the render stream.  (Measured and dropped, round 5: each
// type's pair of kernels on a stream of its own — 0.111-0.112 s per render against 0.108 s, profiles/r05_material_split_ab_sm16.txt.
// And again at the thin depths only, depth >= 2, where no launch fills the chip, pairs round-robin on four streams: 438.1 / 443.7 / 438.8
// against 442.0 / 443.8 / 442.8 Msamples/s at K = 20, profiles/r07_thin_material_streams_ab_sm20.txt.)
static int EvalMaterials(wf_ctx *ctx, int depth) {
    for (int m = 1; m < WF_MAT_NTYPES; ++m)
        if (ctx->plan.matPresent[m])
            if (int e = EvalMaterial(ctx, m, depth)) return e;
    return 0;
}
// The shadow stage of one depth on `strm` with the spill rows `spill`: the main stream and the context's own rows for the per-stage entry
// point; stream3 and stackSpill2 where the fused pass runs it beside the next depth (IssueShadowAside).
static int ShadowStage(wf_ctx *ctx, int depth, hipStream_t strm, int *spill) {
    if (!ctx->countTraversal && ctx->plan.fastOk) {
        const WalkKernels &k = ctx->walk;
        const SpillArea area{spill, ctx->plan.spillRows, ctx->dbgWords};   // (the debug words are shared: every update of them is an atomic)
        int *cursor = ctx->ws.counters + CNT_CURSOR_SHADOW * CNT_STRIDE;   // (zeroed by the "Reset shadowRayQueue" launch that follows every any-hit launch)
        if (ctx->cursorDirty[1]) HIPCHK(hipMemsetAsync(cursor, 0, sizeof(int), strm));
        ctx->cursorDirty[1] = true;
        // TWO-CLASS TRAVERSAL: aside, the rays handed over go to a list of the shadow side's own (ws.deferQ may be filling with the next
        // depth's closest-hit rays); the kernels take the list from the WorkState they are given
        WorkState ws = ctx->ws;
        if (strm != ctx->stream && ctx->deferQShadow) ws.deferQ = ctx->deferQShadow;
        LAUNCHT_ON(strm, "Intersect shadow", k.shadow, k.gridShadow, ctx->svHost, ws, ctx->fast, area, cursor, ctx->plan.cursorChunkShadow, (const int *)nullptr);
        if (k.shadowGen)
            LAUNCHT_ON(strm, "Intersect shadow: rays that met a general primitive", k.shadowGen, k.gridShadowGen, ctx->svHost, ws, ctx->fast, area, (int *)nullptr, ctx->plan.cursorChunkShadow, (const int *)ws.deferQ);
    } else
        LAUNCH_ON(strm, "Intersect shadow", ctx->stage.intersectShadow[ctx->countTraversal], StageGridOf(ctx, SITE_INTERSECT_SHADOW, ctx->maxQueueSize, !ctx->countTraversal), ctx->svHost, ctx->ws, spill);
    // "Reset shadowRayQueue": stats->shadowRays[depth] += size; Reset (integrator.cpp:581-585)
    LAUNCH_ON(strm, "Reset shadowRayQueue", k_reset, 1, ctx->ws, (1u << CNT_SHADOW) | (1u << CNT_CURSOR_SHADOW) | (1u << CNT_DEFER_SHADOW), STAT_SHADOW + statDepth(depth), CNT_SHADOW);
    ctx->cursorDirty[1] = false;
    return 0;
}
int wf_intersect_shadow(wf_ctx *ctx, int depth) {
    if (int e = checkReady(ctx)) return e;
    return ShadowStage(ctx, depth, ctx->stream, ctx->stackSpill);
}
// FRAME SCHEDULING: the shadow stage of `depth` on stream3, behind everything the main stream has been given so far (the material stage
// that filled ws.sq).  It reads ws.sq, the scene and its own counters and adds into the pixels' L; the main stream goes on with the
// stages of depth + 1 that touch none of these and waits (JoinShadow) before the first that does: escaped rays and emitter hits add
// into the same pixels' L, after shadow(depth) in the reference's order, so the float sums keep their order and their bits; the
// material stage of depth + 1, which refills ws.sq and CNT_SHADOW, comes later still.
static int IssueShadowAside(wf_ctx *ctx, int depth) {
    HIPCHK(hipEventRecord(ctx->evShadowFork, ctx->stream));
    HIPCHK(hipStreamWaitEvent(ctx->stream3, ctx->evShadowFork, 0));
    if (int e = ShadowStage(ctx, depth, ctx->stream3, ctx->stackSpill2)) return e;
    HIPCHK(hipEventRecord(ctx->evShadowJoin, ctx->stream3));
    ctx->shadowPending = true;
    return 0;
}
static int JoinShadow(wf_ctx *ctx) {
    if (!ctx->shadowPending) return 0;
    HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->evShadowJoin, 0));
    ctx->shadowPending = false;
    return 0;
}
// K12: SampleSubsurface (wavefront/subsurface.cpp:18-203) in its three launches
int wf_subsurface_probe(wf_ctx *ctx, int depth) {
    if (int e = checkReady(ctx)) return e;
    if (!ctx->svHost.haveSubsurface) return 0;
    (void)depth;
    LAUNCH("Get BSSRDF and enqueue probe ray", k_subsurface_probe, StageGridOf(ctx, SITE_SUBSURFACE_PROBE, ctx->maxQueueSize), ctx->svHost, ctx->ws);
    return 0;
}
int wf_intersect_one_random(wf_ctx *ctx) {
    if (int e = checkReady(ctx)) return e;
    if (!ctx->svHost.haveSubsurface) return 0;
    // reference-order walk (the chain of probe hits is a dependent sequence per item; the subsurface path is a side path)
    LAUNCH("Intersect one random (subsurface probe)", ctx->stage.intersectOneRandom, StageGridOf(ctx, SITE_INTERSECT_ONE_RANDOM, ctx->maxQueueSize), ctx->svHost, ctx->ws, ctx->stackSpill);
    return 0;
}
int wf_subsurface_scatter(wf_ctx *ctx, int depth) {
    if (int e = checkReady(ctx)) return e;
    if (!ctx->svHost.haveSubsurface) return 0;
    LAUNCH("Handle out-scattering after SSS", k_subsurface_scatter, StageGridOf(ctx, SITE_SUBSURFACE_SCATTER, ctx->maxQueueSize), ctx->svHost, ctx->ws, depth & 1);
    return 0;
}
int wf_update_film(wf_ctx *ctx) {
    if (int e = checkReady(ctx)) return e;
    if (ctx->ws.slotStride > 0 && ctx->ws.slotStride == ctx->passSamples && ctx->passSamples <= FILM_MAX_SLOTS && ctx->svHost.film.type == WF_FILM_RGB)
        LAUNCH("Update film", k_update_film_pm, std::min(4096, (ctx->ws.pixelsPerPass + FILM_PIX - 1) / FILM_PIX), ctx->svHost, ctx->ws, ctx->passSamples);
    else
        LAUNCH("Update film", k_update_film, gridFor(ctx->ws.pixelsPerPass), ctx->svHost, ctx->ws, ctx->passSamples);
    return 0;
}

// integrator.cpp:357-434 for one (y0, sampleIndex): everything is enqueued, nothing synchronises
static int RenderPass(wf_ctx *ctx, int y0, int sample_index) {
    int e;
    // FRAME SCHEDULING (see IssueShadowAside).  Serial, as the per-stage entry points are: the full per-stage profile (it times every launch
    // on the main stream), launch tracing, traversal counting (ws.trav, the reference-order walks on ctx->stackSpill), and the scenes
    // FrameOverlapScene leaves out.
    const bool aside = FrameOverlapActive(ctx) && ctx->profile != 1 && !ctx->traceLaunch && !ctx->countTraversal;
    const bool skipLastSamples = SkipLastSamples(ctx);
    if ((e = wf_reset_ray_queue(ctx, 0))) return e;
    if ((e = wf_gen_camera_rays(ctx, y0, sample_index))) return e;
    for (int depth = 0; true; ++depth) {
        if ((e = wf_reset_stage_queues(ctx, depth))) return e;
        // (GenerateRaySamples does not depend on the intersections: it is issued after the closest-hit launch so that it runs beside
        // the re-trace; the per-stage entry points keep the reference's order)
        ctx->deferJoin = ctx->plan.fastOk && !ctx->countTraversal && !ctx->svHost.haveMix;
        if ((e = wf_intersect_closest(ctx, depth))) { ctx->deferJoin = false; return e; }
        ctx->deferJoin = false;
        // no samples at the last depth: the loop leaves before the material stage, the only reader.  (Measured and dropped, round 7: at
        // the other depths a launch over the material queues' rays only — 30 % fewer items, 12 % less kernel time, nothing in the frame:
        // profiles/r07_samples_shaded_only_ab_sm20.txt.)
        if (!(skipLastSamples && depth == ctx->maxDepth) && (e = wf_gen_ray_samples(ctx, depth, sample_index))) return e;
        if ((e = JoinRetrace(ctx))) return e;
        if ((e = JoinShadow(ctx))) return e;   // shadow(depth - 1): before the first launch that adds into L
        if ((e = wf_medium_sample(ctx, depth))) return e;
        if ((e = wf_handle_escaped(ctx, depth))) return e;
        if ((e = wf_handle_emissive(ctx, depth))) return e;
        if (depth == ctx->maxDepth) break;
        if ((e = EvalMaterials(ctx, depth))) return e;
        if (aside && (ctx->frameOverlap == 1 || depth >= FRAME_OVERLAP_THIN_DEPTH)) {
            if ((e = IssueShadowAside(ctx, depth))) return e;
            continue;
        }
        if ((e = ctx->svHost.haveMedia ? wf_intersect_shadow_tr(ctx, depth) : wf_intersect_shadow(ctx, depth))) return e;
        if (ctx->svHost.haveSubsurface) {  // SampleSubsurface (integrator.cpp:431) ends with its own TraceShadowRays
            if ((e = wf_subsurface_probe(ctx, depth)) || (e = wf_intersect_one_random(ctx)) || (e = wf_subsurface_scatter(ctx, depth))) return e;
            if ((e = ctx->svHost.haveMedia ? wf_intersect_shadow_tr(ctx, depth) : wf_intersect_shadow(ctx, depth))) return e;
        }
    }
    // (the last depth's shadow stage was joined above, before its escaped rays: maxDepth >= 1 iterations end in the join; maxDepth = 0
    //  issues no shadow stage at all)
    if ((e = JoinShadow(ctx))) return e;
    return wf_update_film(ctx);
}
int wf_render_pass(wf_ctx *ctx, int y0, int sample_index) {
    if (int e = checkReady(ctx)) return e;
    const int e = RenderPass(ctx, y0, sample_index);
    if (e) {
        // a pass that failed half way leaves nothing in flight that wf_sync or a film download (the main stream's) would not cover
        (void)hipStreamSynchronize(ctx->stream3);
        ctx->shadowPending = false;
    }
    return e;
}

}  // extern "C"
