// wf_boundary_medium.hip — the scene's media and phase functions on a caller's device items (gfx950): the kernels behind
// wf_medium_sample_device and wf_phase_device (include/wf_media.h).  One row per lane, 256-thread workgroups; the per-row bodies are
// wf_boundary_medium.h's, and through them the render's own medium functions (csrc/common/wf_media.h: -ffp-contract=off, no fast-math).
// A unit of its own: its kernels share no device code object with the render's.  The C ABI entry points are in wf_boundary.hip; they
// call the launchers below.
//   k_medium_track<LEAN>   the delta tracking of SampleMediumInteraction along each row's ray: RowBegin, RowStep until the row is
//                          finished, RowEnd.  LEAN as k_medium_sample's (the scene's plan.mediumLean): homogeneous and non-emissive
//                          uniform-grid media only.
//   k_phase                HGPhaseFunction p / PDF for a given direction and Sample_p with the next ray: straight-line code
// WHY THE LOOP ENDS, for every kind of row: wf_boundary_medium.h, TERMINATION.  In short: rows that must not be walked (an id outside the
// medium table, a non-finite origin, a direction without a finite positive length, a NaN or negative tMax, no medium) never enter it;
// the majorant iterator yields one segment (homogeneous, also for an infinite tMax) or at most res.x + res.y + res.z (the DDA, whose
// first line is the NaN guard `!(tMin < tMax)`); a zero-majorant segment takes no collision; and the tentative collisions of a row are
// counted and capped at WF_MEDIUM_ROW_MAX_STEPS.
// THE LESSON OF DESIGN 4.3 (the render's delta-tracking kernel was bound by an atomic taken inside the loop, where every lane arrives in
// its own iteration): nothing shared is touched inside the loop — there is no queue, no counter and no atomic in this unit at all — and
// every store of a row sits after the loop, where the wave's lanes meet again.  Every output row is whole 16-byte vector stores, written
// exactly once, and no row past the count is written.
#include <hip/hip_runtime.h>

#include "wf_boundary_medium.h"

namespace wf {
namespace bmedium {

constexpr int BLOCK = 256;
// the occupancy targets of the render's k_medium_sample (wf_backend.hip: WF_MEDIUM_WAVES / WF_MEDIUM_WAVES_LEAN), taken as they are:
// the loop is the same code, without the queue write-back (DESIGN 4.4 has the registers each variant came out with)
#ifndef WF_MEDIUM_ROW_WAVES
#define WF_MEDIUM_ROW_WAVES 2
#endif
#ifndef WF_MEDIUM_ROW_WAVES_LEAN
#define WF_MEDIUM_ROW_WAVES_LEAN 3
#endif

// the rows of the call: min(n, *nDevice).  Uniform over the launch (one scalar load)
__device__ inline int RowCount(int n, const int32_t *nDevice) {
    if (nDevice == nullptr) return n;
    const int m = *nDevice;
    return m < n ? (m < 0 ? 0 : m) : n;
}

template <bool LEAN>
__global__ void __launch_bounds__(BLOCK, LEAN ? WF_MEDIUM_ROW_WAVES_LEAN : WF_MEDIUM_ROW_WAVES)
k_medium_track(const SceneView *__restrict__ svp, int n, const int32_t *__restrict__ nDevice, int nMedia, const F4 *rays, const int32_t *__restrict__ medium,
               const F4 *__restrict__ lambda4, const F4 *beta4, const F4 *ru4, const F4 *rl4, const int32_t *__restrict__ flags, I4 *__restrict__ event4,
               F4 *__restrict__ pG4, F4 *outBeta4, F4 *outRu4, F4 *outRl4, F4 *__restrict__ L4) {
    const SceneView &sv = *svp;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool row = (long long)i < (long long)RowCount(n, nDevice);
    TrackItem it;   // kind = KIND_NONE: a lane without a row walks nothing
    // (beta4 / r_u4 / r_l4 may be the output arrays: the row is read here, once, and written once at the end)
    if (row) it = LoadTrackItem(nMedia, rays, medium, lambda4, beta4, ru4, rl4, flags, i);
    TrackRow out;
    if (it.kind < 0) {
        RowTrack s;
        RowBegin<LEAN>(sv, it, s);
        while (RowStep<LEAN>(sv, s)) {}   // no store, no atomic, nothing shared: see the header
        out = RowEnd(s, it.r_l);
    } else out = UnwalkedRow(it);
    if (row) {
        event4[i] = out.event;
        pG4[i] = out.pG;
        outBeta4[i] = out.beta;
        outRu4[i] = out.r_u;
        outRl4[i] = out.r_l;
        L4[i] = out.L;
    }
}

// WI / U: the half is asked for (its arrays are given).  A half that is not asked for is neither computed nor written.
template <bool WI, bool U>
__global__ void __launch_bounds__(BLOCK) k_phase(int n, const int32_t *__restrict__ nDevice, const F4 *__restrict__ rays, const F4 *__restrict__ pG4,
                                                  const F4 *__restrict__ wi4, const F4 *__restrict__ u4, F4 *__restrict__ pPdf4, F4 *__restrict__ sample4,
                                                  F4 *__restrict__ nextRays) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if ((long long)i >= (long long)RowCount(n, nDevice)) return;   // (no barrier in this kernel)
    const PhaseRow out = PhaseItem(rays, pG4, WI ? wi4 : nullptr, U ? u4 : nullptr, i);
    if (WI) pPdf4[i] = out.pPdf;
    if (U) {
        sample4[i] = out.sample;
        nextRays[2 * i] = out.ray0;
        nextRays[2 * i + 1] = out.ray1;
    }
}

static dim3 GridFor(int n) { return dim3((unsigned)(((size_t)n + BLOCK - 1) / BLOCK)); }

int LaunchMediumTrack(void *stream, bool lean, const SceneView *svDev, const TrackArgs &a) {
    static_assert(sizeof(F4) == 16 && sizeof(I4) == 16, "a ray half and an output row are 16 bytes");
    if (a.n <= 0) return 0;
    auto k = lean ? k_medium_track<true> : k_medium_track<false>;
    hipLaunchKernelGGL(k, GridFor(a.n), dim3(BLOCK), 0, (hipStream_t)stream, svDev, a.n, a.nDevice, a.nMedia, reinterpret_cast<const F4 *>(a.rays8), a.medium,
                       reinterpret_cast<const F4 *>(a.lambda4), reinterpret_cast<const F4 *>(a.beta4), reinterpret_cast<const F4 *>(a.ru4),
                       reinterpret_cast<const F4 *>(a.rl4), a.flags, reinterpret_cast<I4 *>(a.event4), reinterpret_cast<F4 *>(a.pG4),
                       reinterpret_cast<F4 *>(a.outBeta4), reinterpret_cast<F4 *>(a.outRu4), reinterpret_cast<F4 *>(a.outRl4), reinterpret_cast<F4 *>(a.L4));
    return (int)hipGetLastError();
}

int LaunchPhase(void *stream, const PhaseArgs &a) {
    if (a.n <= 0) return 0;
    const bool wi = a.wi4 != nullptr, u = a.u4 != nullptr;
    if (!wi && !u) return 0;
    auto k = wi && u ? k_phase<true, true> : wi ? k_phase<true, false> : k_phase<false, true>;
    hipLaunchKernelGGL(k, GridFor(a.n), dim3(BLOCK), 0, (hipStream_t)stream, a.n, a.nDevice, reinterpret_cast<const F4 *>(a.rays8), reinterpret_cast<const F4 *>(a.pG4),
                       reinterpret_cast<const F4 *>(a.wi4), reinterpret_cast<const F4 *>(a.u4), reinterpret_cast<F4 *>(a.pPdf4), reinterpret_cast<F4 *>(a.sample4),
                       reinterpret_cast<F4 *>(a.nextRays8));
    return (int)hipGetLastError();
}

}  // namespace bmedium
}  // namespace wf
