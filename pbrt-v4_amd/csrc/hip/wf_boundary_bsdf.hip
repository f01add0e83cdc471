// wf_boundary_bsdf.hip — the scene's BSDFs on a caller's device items (gfx950): the kernels behind wf_bsdf_make_device and
// wf_bsdf_eval_device (include/wf_abi.h).  One translation unit per material type, compiled with -DWF_MAT_INSTANCE=<wf_material_type> as
// wf_mat.hip is: a code object per type (a kernel is allocated what it can reach, DESIGN 4.0 — no kernel switches over ten BxDFs) and a
// parallel build.  Its kernels share no device code object with the render's.  The per-row bodies are wf_boundary_bsdf.h's, and through
// them the render's own (the texture evaluator, MatBxDF<type>::Get, BSDF<BxDF>::f / PDF / Sample_f: -ffp-contract=off, no fast-math).
//   WF_MAT_INSTANCE 0        k_bsdf_route       the type-independent first kernel of a make call: which rows have a BSDF and of which
//                                               material (the MixMaterial resolve) -> the context's route words; the zero rows
//                            k_bsdf_eval_zero   ... of an eval call: the rows whose record names no BSDF of this scene
//   WF_MAT_INSTANCE 1 - 10   k_bsdf_make<type, CAMANIM>   the record and bsdf4 of the rows routed to a material of this type
//                            k_bsdf_eval<type>            f / PDF / Sample_f of the rows whose record is of this type
// ROUTING: every present type's launch scans all rows and skips the foreign ones (DESIGN 4.4 says why).  One row per lane, 256-thread
// workgroups, no barrier, no atomic of its own, no LDS.  Every row below the count is written by exactly one kernel of a call, as whole
// 16-byte stores, and no row past the count is written.  The C ABI entry points are in wf_boundary.hip; they call the launchers below.
#include <hip/hip_runtime.h>

#if !defined(WF_MAT_INSTANCE)
#error "compile with -DWF_MAT_INSTANCE=<0 | wf_material_type>"
#endif

#include "wf_boundary_bsdf.h"

using namespace wf;
using namespace wf::bbsdf;

constexpr int BLOCK = 256;
// minimum waves per SIMD of every kernel here (2 -> 256 VGPRs): the layered and hair types want the registers, and nobody has measured
// these kernels yet — a type's occupancy goes up only with a compile that shows no spills at the higher setting
#ifndef WF_BSDF_WAVES
#define WF_BSDF_WAVES 2
#endif

// the rows of the call: min(n, *nDevice).  Uniform over the launch (one scalar load)
__device__ inline int RowCount(int n, const int32_t *nDevice) {
    if (nDevice == nullptr) return n;
    const int m = *nDevice;
    return m < n ? (m < 0 ? 0 : m) : n;
}
static dim3 GridFor(int n) { return dim3((unsigned)(((size_t)n + BLOCK - 1) / BLOCK)); }

#if WF_MAT_INSTANCE == 0
__global__ void __launch_bounds__(BLOCK, WF_BSDF_WAVES) k_bsdf_route(const SceneView *__restrict__ svp, int n, int nMaterials, const int32_t *__restrict__ nDevice,
                                                                      const F4 *__restrict__ rays, const F4 *__restrict__ planesF, const I4 *__restrict__ planesI,
                                                                      int32_t *__restrict__ route, F4 *__restrict__ rec, I4 *__restrict__ bsdf4) {
    const SceneView &sv = *svp;
    const size_t N = (size_t)n;   // the planes' stride is the caller's n, whatever the device count says
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if ((long long)i >= (long long)RowCount(n, nDevice)) return;
    const int matId = RouteRow(sv, nMaterials, rays, planesF, planesI, N, i);
    route[i] = matId;
    if (matId < 0) {
#pragma unroll
        for (int p = 0; p < REC_PLANES; ++p) rec[p * N + i] = F4{0, 0, 0, 0};
        bsdf4[i] = I4{0, 0, 0, 0};
    }
}
__global__ void __launch_bounds__(BLOCK, WF_BSDF_WAVES) k_bsdf_eval_zero(const SceneView *__restrict__ svp, int n, int nMaterials, const int32_t *__restrict__ nDevice,
                                                                          const F4 *__restrict__ rec, F4 *__restrict__ f4, F4 *__restrict__ pdf4, F4 *__restrict__ nextRays,
                                                                          F4 *__restrict__ sampleF4, F4 *__restrict__ samplePdf4, I4 *__restrict__ sampleI4) {
    const SceneView &sv = *svp;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if ((long long)i >= (long long)RowCount(n, nDevice)) return;
    int matId;
    if (RecordType(sv, nMaterials, rec[i], &matId) != 0) return;   // (its type's kernel writes the row)
    const F4 z{0, 0, 0, 0};
    if (f4 != nullptr) { f4[i] = z; pdf4[i] = z; }
    if (sampleF4 != nullptr) {
        nextRays[2 * i] = z; nextRays[2 * i + 1] = z;
        sampleF4[i] = z; samplePdf4[i] = z;
        sampleI4[i] = I4{0, 0, 0, 0};
    }
}
extern "C" int wf_launch_bsdf_make_0(void *stream, const SceneView *svDev, const MakeArgs *a) {
    static_assert(sizeof(F4) == 16 && sizeof(I4) == 16, "a plane item and an output row are 16 bytes");
    if (a->n <= 0) return 0;
    hipLaunchKernelGGL(k_bsdf_route, GridFor(a->n), dim3(BLOCK), 0, (hipStream_t)stream, svDev, a->n, a->nMaterials, a->nDevice, reinterpret_cast<const F4 *>(a->rays8),
                       reinterpret_cast<const F4 *>(a->planesF), reinterpret_cast<const I4 *>(a->planesI), a->route, reinterpret_cast<F4 *>(a->rec),
                       reinterpret_cast<I4 *>(a->bsdf4));
    return (int)hipGetLastError();
}
extern "C" int wf_launch_bsdf_eval_0(void *stream, const SceneView *svDev, const EvalArgs *a) {
    if (a->n <= 0) return 0;
    hipLaunchKernelGGL(k_bsdf_eval_zero, GridFor(a->n), dim3(BLOCK), 0, (hipStream_t)stream, svDev, a->n, a->nMaterials, a->nDevice, reinterpret_cast<const F4 *>(a->rec),
                       reinterpret_cast<F4 *>(a->f4), reinterpret_cast<F4 *>(a->pdf4), reinterpret_cast<F4 *>(a->nextRays8), reinterpret_cast<F4 *>(a->sampleF4),
                       reinterpret_cast<F4 *>(a->samplePdf4), reinterpret_cast<I4 *>(a->sampleI4));
    return (int)hipGetLastError();
}
#else
static_assert(WF_MAT_INSTANCE >= WF_MAT_DIFFUSE && WF_MAT_INSTANCE < WF_MAT_NTYPES, "WF_MAT_INSTANCE is a material type with a BxDF");

template <int MAT, bool CAMANIM>
__global__ void __launch_bounds__(BLOCK, WF_BSDF_WAVES) k_bsdf_make(const SceneView *__restrict__ svp, int n, const int32_t *__restrict__ nDevice,
                                                                     const F4 *__restrict__ planesF, const F4 *__restrict__ lambda4,
                                                                     const int32_t *__restrict__ regularize, const int32_t *__restrict__ route, F4 *__restrict__ rec,
                                                                     I4 *__restrict__ bsdf4) {
    const SceneView &sv = *svp;
    const size_t N = (size_t)n;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if ((long long)i >= (long long)RowCount(n, nDevice)) return;
    const int matId = route[i];   // (k_bsdf_route's: in the scene's table, or -1)
    if (matId < 0 || sv.materials[matId].type != MAT) return;
    MakeRowOut out;
    MakeRow<MAT, CAMANIM>(sv, matId, planesF, N, i, lambda4[i], regularize != nullptr && regularize[i] != 0, &out);
#pragma unroll
    for (int p = 0; p < REC_PLANES; ++p) rec[p * N + i] = out.rec[p];
    bsdf4[i] = out.bsdf4;
}

template <int MAT>
__global__ void __launch_bounds__(BLOCK, WF_BSDF_WAVES) k_bsdf_eval(const SceneView *__restrict__ svp, int n, int nMaterials, const int32_t *__restrict__ nDevice,
                                                                     const F4 *__restrict__ rec, const F4 *__restrict__ planesF, const I4 *__restrict__ planesI,
                                                                     const F4 *__restrict__ wi4, const F4 *__restrict__ u4, F4 *__restrict__ f4, F4 *__restrict__ pdf4,
                                                                     F4 *__restrict__ nextRays, F4 *__restrict__ sampleF4, F4 *__restrict__ samplePdf4,
                                                                     I4 *__restrict__ sampleI4) {
    const SceneView &sv = *svp;
    const size_t N = (size_t)n;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if ((long long)i >= (long long)RowCount(n, nDevice)) return;
    int matId;
    if (RecordType(sv, nMaterials, rec[i], &matId) != MAT) return;   // (the header is checked against the scene before anything is indexed by it)
    EvalRowOut out;
    EvalRow<MAT>(sv, matId, rec, planesF, planesI, N, i, wi4, u4, &out);
    if (wi4 != nullptr) { f4[i] = out.f; pdf4[i] = out.pdf; }
    if (u4 != nullptr) {
        nextRays[2 * i] = out.ray0; nextRays[2 * i + 1] = out.ray1;
        sampleF4[i] = out.sf; samplePdf4[i] = out.spdf;
        sampleI4[i] = out.si;
    }
}

#define WF_CAT2_(a, b) a##b
#define WF_CAT2(a, b) WF_CAT2_(a, b)
extern "C" int WF_CAT2(wf_launch_bsdf_make_, WF_MAT_INSTANCE)(void *stream, const SceneView *svDev, const MakeArgs *a) {
    if (a->n <= 0) return 0;
    auto k = a->cameraAnim ? k_bsdf_make<WF_MAT_INSTANCE, true> : k_bsdf_make<WF_MAT_INSTANCE, false>;
    hipLaunchKernelGGL(k, GridFor(a->n), dim3(BLOCK), 0, (hipStream_t)stream, svDev, a->n, a->nDevice, reinterpret_cast<const F4 *>(a->planesF),
                       reinterpret_cast<const F4 *>(a->lambda4), a->regularize, (const int32_t *)a->route, reinterpret_cast<F4 *>(a->rec), reinterpret_cast<I4 *>(a->bsdf4));
    return (int)hipGetLastError();
}
extern "C" int WF_CAT2(wf_launch_bsdf_eval_, WF_MAT_INSTANCE)(void *stream, const SceneView *svDev, const EvalArgs *a) {
    if (a->n <= 0) return 0;
    hipLaunchKernelGGL((k_bsdf_eval<WF_MAT_INSTANCE>), GridFor(a->n), dim3(BLOCK), 0, (hipStream_t)stream, svDev, a->n, a->nMaterials, a->nDevice,
                       reinterpret_cast<const F4 *>(a->rec), reinterpret_cast<const F4 *>(a->planesF), reinterpret_cast<const I4 *>(a->planesI),
                       reinterpret_cast<const F4 *>(a->wi4), reinterpret_cast<const F4 *>(a->u4), reinterpret_cast<F4 *>(a->f4), reinterpret_cast<F4 *>(a->pdf4),
                       reinterpret_cast<F4 *>(a->nextRays8), reinterpret_cast<F4 *>(a->sampleF4), reinterpret_cast<F4 *>(a->samplePdf4),
                       reinterpret_cast<I4 *>(a->sampleI4));
    return (int)hipGetLastError();
}
#endif
