// wf_boundary_light.hip — the scene's lights on a caller's device items (gfx950): the kernels behind wf_light_sample_device and
// wf_light_emitted_device (include/wf_abi.h).  One row per lane, 256-thread workgroups; the per-row bodies are wf_boundary_light.h's, and
// through them the render's own (the light samplers, SampleLi, PDF_Li, L, Le: -ffp-contract=off, no fast-math).  A unit of its own: its
// kernels share no device code object with the render's.  The C ABI entry points are in wf_boundary.hip; they call the launchers below.
//   k_light_sample<RARE>                       lightSampler.Sample + light.SampleLi for a whole workgroup (SampleLightForBlock: the
//                                              requests sorted by light class through 21.5 KB of LDS, whole waves of one class — as
//                                              k_mat_nee runs it), then the shadow ray of each usable row.  RARE as k_mat_nee's
//   k_light_emitted<PORTAL, ALPHA, AREA_RARE>  AreaLightL of a hit row, LightLe of a miss row, with the sampler's PMF and PDF_Li from
//                                              the previous vertex where the caller passes one
// Every output row is whole 16-byte vector stores, and no row past the count is written.
#include <hip/hip_runtime.h>

#include "wf_boundary_light.h"
#include "wf_plan.h"

namespace wf {
namespace blight {

constexpr int BLOCK = 256;   // SampleLightForBlock's NT

// the rows of the call: min(n, *nDevice).  Uniform over the launch (one scalar load)
__device__ inline int RowCount(int n, const int32_t *nDevice) {
    if (nDevice == nullptr) return n;
    const int m = *nDevice;
    return m < n ? (m < 0 ? 0 : m) : n;
}

// BARRIERS.  SampleLightForBlock synchronises the workgroup four times, so every thread of every launched workgroup calls it exactly
// once: the kernel has no return and no loop before or around the call, and a thread without a usable row — past the count, in the
// partial last block, a miss, an invalid record — goes in with want = false (SampleRequest of a default SampleItem).  Only the loads
// before the call and the stores after it are predicated on the row.
template <bool RARE>
__global__ void __launch_bounds__(BLOCK) k_light_sample(const SceneView *__restrict__ svp, int n, const int32_t *__restrict__ nDevice, const F4 *__restrict__ planesF,
                                                         const I4 *__restrict__ planesI, const F4 *__restrict__ lambda4, const F4 *__restrict__ u4,
                                                         const int32_t *__restrict__ side, F4 *__restrict__ rays, F4 *__restrict__ L4, F4 *__restrict__ wiPdf4,
                                                         I4 *__restrict__ light4) {
    const SceneView &sv = *svp;
    const size_t N = (size_t)n;   // the planes' stride is the caller's n, whatever the device count says
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool row = (long long)i < (long long)RowCount(n, nDevice);
    SampleItem it;   // valid = 0
    if (row) it = LoadSampleItem(planesF, planesI, N, i, lambda4, u4, side);
    const NeeRequest rq = SampleRequest(it);
    const LightPick pick = SampleLightForBlock<RARE>(sv, rq.want, rq.ctx, rq.u0, rq.u, rq.lambda);   // every thread: see BARRIERS
    if (row) {
        const SampleRow out = SampleFinish(sv, it, pick);
        rays[2 * i] = out.ray0;
        rays[2 * i + 1] = out.ray1;
        L4[i] = out.L;
        wiPdf4[i] = out.wiPdf;
        light4[i] = out.light;
    }
}

template <bool PORTAL, bool ALPHA, bool AREA_RARE>
__global__ void __launch_bounds__(BLOCK) k_light_emitted(const SceneView *__restrict__ svp, int n, const int32_t *__restrict__ nDevice, const F4 *__restrict__ rays,
                                                          const F4 *__restrict__ planesF, const I4 *__restrict__ planesI, const F4 *__restrict__ lambda4,
                                                          int infiniteIndex, const F4 *__restrict__ prevF, F4 *__restrict__ Le4, F4 *__restrict__ pmfPdf4) {
    const SceneView &sv = *svp;
    const size_t N = (size_t)n;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if ((long long)i >= (long long)RowCount(n, nDevice)) return;   // (no barrier in this kernel)
    const EmittedRow out = EmittedItem<PORTAL, ALPHA, AREA_RARE>(sv, rays, planesF, planesI, N, i, lambda4, infiniteIndex, prevF);
    Le4[i] = out.Le;
    pmfPdf4[i] = out.pmfPdf;
}

static dim3 GridFor(int n) { return dim3((unsigned)(((size_t)n + BLOCK - 1) / BLOCK)); }

int LaunchLightSample(void *stream, bool rare, const SceneView *svDev, const SampleArgs &a) {
    static_assert(sizeof(F4) == 16 && sizeof(I4) == 16, "a plane item and an output row are 16 bytes");
    if (a.n <= 0) return 0;
    auto k = rare ? k_light_sample<true> : k_light_sample<false>;
    hipLaunchKernelGGL(k, GridFor(a.n), dim3(BLOCK), 0, (hipStream_t)stream, svDev, a.n, a.nDevice, reinterpret_cast<const F4 *>(a.planesF),
                       reinterpret_cast<const I4 *>(a.planesI), reinterpret_cast<const F4 *>(a.lambda4), reinterpret_cast<const F4 *>(a.u4), a.side,
                       reinterpret_cast<F4 *>(a.rays8), reinterpret_cast<F4 *>(a.L4), reinterpret_cast<F4 *>(a.wiPdf4), reinterpret_cast<I4 *>(a.light4));
    return (int)hipGetLastError();
}

using EmittedFn = void (*)(const SceneView *, int, const int32_t *, const F4 *, const F4 *, const I4 *, const F4 *, int, const F4 *, F4 *, F4 *);
// (a portal light or an emitter's alpha texture makes rareLights true: five of the eight combinations exist)
static EmittedFn EmittedKernel(int variant) {
    using wf::planning::EmittedVariant;
    switch (variant) {
    case EmittedVariant(false, false, false): return k_light_emitted<false, false, false>;
    case EmittedVariant(false, false, true): return k_light_emitted<false, false, true>;
    case EmittedVariant(true, false, true): return k_light_emitted<true, false, true>;
    case EmittedVariant(false, true, true): return k_light_emitted<false, true, true>;
    case EmittedVariant(true, true, true): return k_light_emitted<true, true, true>;
    }
    return nullptr;
}

int LaunchLightEmitted(void *stream, int variant, const SceneView *svDev, const EmittedArgs &a) {
    const EmittedFn k = EmittedKernel(variant);
    if (!k) return -1;
    if (a.n <= 0) return 0;
    hipLaunchKernelGGL(k, GridFor(a.n), dim3(BLOCK), 0, (hipStream_t)stream, svDev, a.n, a.nDevice, reinterpret_cast<const F4 *>(a.rays8),
                       reinterpret_cast<const F4 *>(a.planesF), reinterpret_cast<const I4 *>(a.planesI), reinterpret_cast<const F4 *>(a.lambda4), a.infiniteIndex,
                       reinterpret_cast<const F4 *>(a.prevF), reinterpret_cast<F4 *>(a.Le4), reinterpret_cast<F4 *>(a.pmfPdf4));
    return (int)hipGetLastError();
}

}  // namespace blight
}  // namespace wf
