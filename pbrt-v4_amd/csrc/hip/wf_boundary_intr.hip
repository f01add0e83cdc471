// wf_boundary_intr.hip — the device-buffer boundary between a hit record and a SurfaceInteraction, and between the context's camera-ray
// queue and a caller's ray buffer (wf_hit_interaction_device / wf_camera_rays_device, include/wf_abi.h).  A translation unit of its own:
// its kernels share no device code object with the render's, so no existing kernel's register allocation or ISA can move with it.
//   k_hit_interaction<GENERAL, CURVE_ALPHA, ANIM>  what WavefrontAggregate::IntersectClosest hands EnqueueWorkAfterIntersection
//                                                  (wavefront/intersect.h:72-162): the SurfaceInteraction of every hit record, built by
//                                                  the functions the material kernels build it with (HitInteraction / IntrWo, wf_shapes.h)
//   k_pack_camera_rays                             ray queue 0 after "Generate camera rays", as rays8 + pixel + wavelengths
//   k_pack_camera_samples                          ... plus the wavelengths' PDF, the camera-ray weight and the filter weight (wf_camera_samples_device)
#include <hip/hip_runtime.h>

#include "../common/wf_kernels.h"
#include "wf_boundary_intr.h"
#include "wf_plan.h"

using namespace wf;

constexpr int BLOCK = 256;
constexpr int MAX_GRID = 256 * 8;   // 256 CUs x up to 8 resident 256-thread workgroups

static int GridFor(int n) {
    int g = (n + BLOCK - 1) / BLOCK;
    return g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g);
}

// Plane-major output, the queues' own idiom: item i of plane p is the 16 bytes at out[p * n + i], so every store of a wave is one
// coalesced 1 KiB.  A kernel is allocated what it can reach: GENERAL — the quadric / patch / curve interactions, CURVE_ALPHA — the replay
// of an alpha-textured curve's recursion (the texture evaluator), ANIM — the interpolation of animated transformations, nested
// placements included (outer_plus1: both transformations at the ray's time).  The lean variant applies an instance's transformation in
// line (WF_LEAN_INLINE_INSTANCE, wf_shapes.h): the SurfIntr goes from registers to the planes.
template <bool GENERAL, bool CURVE_ALPHA, bool ANIM>
__global__ void __launch_bounds__(BLOCK) k_hit_interaction(const SceneView *__restrict__ svp, int n, const F4 *__restrict__ rays, const I4 *__restrict__ hits,
                                                            F4 *__restrict__ outF, I4 *__restrict__ outI) {
    static_assert(GENERAL || !CURVE_ALPHA, "a curve is a general primitive");
    const SceneView &sv = *svp;
    const size_t N = (size_t)n;
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const F4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];   // o.xyz d.x | d.yz tMax time
        const I4 h0 = hits[2 * (size_t)i], h1 = hits[2 * (size_t)i + 1];   // prim t b0 b1 | b2 - - instance
        const int prim = h0.x, inst = h1.w;
        const float time = r1.w, tHit = BitsToFloat((uint32_t)h0.y);
        // a caller's stale buffer must not walk the tables: two compares per item
        int valid = prim >= 0 ? 1 : 0;
        if (valid && ((uint32_t)prim >= (uint32_t)(sv.nTriangles + sv.nQuadrics) || (uint32_t)(inst + 1) > (uint32_t)sv.nInstances)) valid = -1;
        F4 f[WF_INTR_FPLANES];
#pragma unroll
        for (int p = 0; p < WF_INTR_FPLANES; ++p) f[p] = F4{0, 0, 0, 0};
        I4 ids{-1, -1, -1, -1}, info{-1, valid, 0, 0};
        if (valid == 1) {
            const V3 ro{r0.x, r0.y, r0.z}, rd{r0.w, r1.x, r1.y};
            SurfIntr si;
            HitInteraction<GENERAL, CURVE_ALPHA, ANIM>(sv, prim, inst, BitsToFloat((uint32_t)h0.z), BitsToFloat((uint32_t)h0.w), BitsToFloat((uint32_t)h1.x), &si, ro, rd, time);
            // intr.wo: the Interaction constructor normalises -ray.d (interaction.h:40-43), in every space the interaction passes through
            const V3 wo = IntrWo<GENERAL, ANIM>(sv, prim, inst, V3{-rd.x, -rd.y, -rd.z}, time);
            const wf_mesh &mesh = sv.meshes[si.mesh];
            f[0] = F4{si.pi.lo.x, si.pi.lo.y, si.pi.lo.z, si.uv.x};
            f[1] = F4{si.pi.hi.x, si.pi.hi.y, si.pi.hi.z, si.uv.y};
            f[2] = F4{si.n.x, si.n.y, si.n.z, time};
            f[3] = F4{si.ns.x, si.ns.y, si.ns.z, tHit};
            f[4] = F4{wo.x, wo.y, wo.z, 0};
            f[5] = F4{si.dpdu.x, si.dpdu.y, si.dpdu.z, 0};
            f[6] = F4{si.dpdv.x, si.dpdv.y, si.dpdv.z, 0};
            f[7] = F4{si.dpdus.x, si.dpdus.y, si.dpdus.z, 0};
            f[8] = F4{si.dpdvs.x, si.dpdvs.y, si.dpdvs.z, 0};
            f[9] = F4{si.dndus.x, si.dndus.y, si.dndus.z, 0};
            f[10] = F4{si.dndvs.x, si.dndvs.y, si.dndvs.z, 0};
            // the emitter of a hit as the emissive-hit stage finds it (KHandleEmissive): first_light + (primitive id - first_tri)
            ids = I4{mesh.material, mesh.first_light >= 0 ? mesh.first_light + (prim - mesh.first_tri) : -1, mesh.medium_inside, mesh.medium_outside};
            info = I4{si.mesh, 1, mesh.flags, 0};
        }
#pragma unroll
        for (int p = 0; p < WF_INTR_FPLANES; ++p) outF[p * N + i] = f[p];
        outI[i] = ids;
        outI[N + i] = info;
    }
}

// Ray queue 0 as "Generate camera rays" left it -> the caller's arrays: the ray with tMax = infinity and the time of o.w, the pixel and
// the wavelengths of the item's pixel sample state.  The count is clamped to the caller's capacity (the entry point has checked that the
// band fits).
__global__ void __launch_bounds__(BLOCK) k_pack_camera_rays(WorkState ws, int nMax, F4 *__restrict__ rays, I2 *__restrict__ pixel, F4 *__restrict__ lambda4,
                                                             int32_t *__restrict__ nOut) {
    int n = ws.counters[CNT_RAY0 * CNT_STRIDE];
    if (n > nMax) n = nMax;
    if (n > ws.maxQueueSize) n = ws.maxQueueSize;
    if (blockIdx.x == 0 && threadIdx.x == 0) *nOut = n;
    const RayQueueV &q = ws.rq[0];
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const F4 o = q.o[i], d = q.d[i];
        const int pixelIndex = q.meta[i].x;
        rays[2 * (size_t)i] = F4{o.x, o.y, o.z, d.x};
        rays[2 * (size_t)i + 1] = F4{d.y, d.z, WF_INFINITY, o.w};
        pixel[i] = ws.pPixel[pixelIndex];
        lambda4[i] = ws.lambda[pixelIndex];
    }
}

// ... and with the three weights of the item's pixel sample (wf_camera_samples_device): the wavelengths' PDF as the camera-ray stage
// sampled it, the camera-ray weight and the filter weight — what UpdateFilm reads beside the radiance.  A kernel of its own, so that
// k_pack_camera_rays stays the code it was.
__global__ void __launch_bounds__(BLOCK) k_pack_camera_samples(WorkState ws, int nMax, F4 *__restrict__ rays, I2 *__restrict__ pixel, F4 *__restrict__ lambda4,
                                                                F4 *__restrict__ lambdaPdf4, F4 *__restrict__ cameraWeight4, float *__restrict__ filterWeight,
                                                                int32_t *__restrict__ nOut) {
    int n = ws.counters[CNT_RAY0 * CNT_STRIDE];
    if (n > nMax) n = nMax;
    if (n > ws.maxQueueSize) n = ws.maxQueueSize;
    if (blockIdx.x == 0 && threadIdx.x == 0) *nOut = n;
    const RayQueueV &q = ws.rq[0];
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const F4 o = q.o[i], d = q.d[i];
        const int pixelIndex = q.meta[i].x;
        rays[2 * (size_t)i] = F4{o.x, o.y, o.z, d.x};
        rays[2 * (size_t)i + 1] = F4{d.y, d.z, WF_INFINITY, o.w};
        pixel[i] = ws.pPixel[pixelIndex];
        lambda4[i] = ws.lambda[pixelIndex];
        lambdaPdf4[i] = ws.lambdaPdf[pixelIndex];
        cameraWeight4[i] = ws.cameraRayWeight[pixelIndex];
        filterWeight[i] = ws.filterWeight[pixelIndex];
    }
}

using IntrFn = void (*)(const SceneView *, int, const F4 *, const I4 *, F4 *, I4 *);
static IntrFn IntrKernel(int variant) {
    using wf::planning::IntrVariant;
    switch (variant) {
    case IntrVariant(false, false, false): return k_hit_interaction<false, false, false>;
    case IntrVariant(true, false, false): return k_hit_interaction<true, false, false>;
    case IntrVariant(true, true, false): return k_hit_interaction<true, true, false>;
    case IntrVariant(false, false, true): return k_hit_interaction<false, false, true>;
    case IntrVariant(true, false, true): return k_hit_interaction<true, false, true>;
    case IntrVariant(true, true, true): return k_hit_interaction<true, true, true>;
    }
    return nullptr;
}

int wf::boundary::LaunchHitInteraction(hipStream_t stream, int variant, const SceneView *svDev, int n, const float *rays8, const wf_hit_record *hits, float *outF,
                                       int32_t *outI) {
    static_assert(sizeof(wf_hit_record) == 2 * sizeof(I4) && sizeof(F4) == 16 && sizeof(I4) == 16, "a ray and a record are read as two 16-byte loads each");
    const IntrFn k = IntrKernel(variant);
    if (!k) return -1;
    hipLaunchKernelGGL(k, dim3(GridFor(n)), dim3(BLOCK), 0, stream, svDev, n, reinterpret_cast<const F4 *>(rays8), reinterpret_cast<const I4 *>(hits),
                       reinterpret_cast<F4 *>(outF), reinterpret_cast<I4 *>(outI));
    return (int)hipGetLastError();
}

int wf::boundary::LaunchPackCameraRays(hipStream_t stream, const WorkState &ws, int nMax, float *rays8, int32_t *pixelXY, float *lambda4, int32_t *nOut) {
    static_assert(sizeof(I2) == 8, "pixel_xy holds two ints per ray");
    hipLaunchKernelGGL(k_pack_camera_rays, dim3(GridFor(nMax)), dim3(BLOCK), 0, stream, ws, nMax, reinterpret_cast<F4 *>(rays8), reinterpret_cast<I2 *>(pixelXY),
                       reinterpret_cast<F4 *>(lambda4), nOut);
    return (int)hipGetLastError();
}

int wf::boundary::LaunchPackCameraSamples(hipStream_t stream, const WorkState &ws, int nMax, float *rays8, int32_t *pixelXY, float *lambda4, float *lambdaPdf4,
                                          float *cameraWeight4, float *filterWeight, int32_t *nOut) {
    hipLaunchKernelGGL(k_pack_camera_samples, dim3(GridFor(nMax)), dim3(BLOCK), 0, stream, ws, nMax, reinterpret_cast<F4 *>(rays8), reinterpret_cast<I2 *>(pixelXY),
                       reinterpret_cast<F4 *>(lambda4), reinterpret_cast<F4 *>(lambdaPdf4), reinterpret_cast<F4 *>(cameraWeight4), filterWeight, nOut);
    return (int)hipGetLastError();
}
