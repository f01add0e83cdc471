// wf_film_add.hip — Film::AddSample on a caller's device items (gfx950): the kernel behind wf_film_add_samples_device.  One item per
// lane, 256-thread blocks; the per-item arithmetic is wf_film_add.h's (the render's, operation for operation: -ffp-contract=off).  A unit
// of its own: its kernels share no device code object with the render's.  The C ABI entry point is in wf_boundary.hip; it calls the
// launcher below.
//   loads per item   8 bytes of pixel, 16 each of L4 / lambda4 / lambda_pdf4, 4 of filter weight; one returning 4-byte atomic on the
//                    pixel's stamp; the film record as two 16-byte loads and two 16-byte stores
// In camera order neighbouring lanes touch neighbouring 32-byte records, so nothing is staged through LDS.
#include <hip/hip_runtime.h>
#include "wf_film_add.h"

namespace wf {
namespace filmadd {

constexpr int BLOCK = 256;

// rejected items of a wave -> the counter: one non-returning atomic from one lane, and only from a wave that rejected one (the ballot
// is wave-uniform, so is the branch; every lane of the wave gets here), as k_film_develop_* count NaNs
__device__ inline void CountRejected(int rej, uint32_t *counter) {
    if (counter == nullptr) return;
    if (__ballot(rej != 0) == 0) return;
    for (int d = 32; d > 0; d >>= 1) rej += __shfl_xor(rej, d);
    if ((threadIdx.x & 63) == 0) atomicAdd(counter, (uint32_t)rej);
}

template <bool SPECTRAL>
__global__ void __launch_bounds__(BLOCK) k_film_add(const SceneView *__restrict__ svp, double *film, double *spectral, int32_t *stamps, int32_t epoch, int n,
                                                    const int32_t *__restrict__ nDevice, const I2 *__restrict__ pixel, const F4 *__restrict__ L4,
                                                    const F4 *__restrict__ lambda4, const F4 *__restrict__ lambdaPdf4, const float *__restrict__ filterWeight,
                                                    uint32_t *rejected) {
    const SceneView &sv = *svp;
    if (nDevice != nullptr) {   // the count a kernel before this one left on the device (wf_camera_samples_device's n_out_device)
        const int m = *nDevice;
        n = m < n ? m : n;
    }
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    int rej = 0;
    if ((long long)i < (long long)n) {
        const I2 pp = pixel[i];
        size_t idx;
        if (FilmIndex(sv.film, pp, &idx)) {
            const F4 L = L4[i], lam = lambda4[i], pdf = lambdaPdf4[i];
            const float fw = filterWeight[i];
            if (ClaimPixel(stamps + idx, epoch)) {
                Wavelengths w;
                w.lambda[0] = lam.x; w.lambda[1] = lam.y; w.lambda[2] = lam.z; w.lambda[3] = lam.w;
                w.pdf[0] = pdf.x; w.pdf[1] = pdf.y; w.pdf[2] = pdf.z; w.pdf[3] = pdf.w;
                double2 *rec = reinterpret_cast<double2 *>(film) + 2 * idx;
                const double2 a = rec[0], b = rec[1];
                double px[4] = {a.x, a.y, b.x, b.y};
                AddSample<SPECTRAL>(sv, px, SPECTRAL ? spectral + (size_t)2 * sv.film.n_buckets * idx : nullptr, toS4(L), w, fw);
                rec[0] = double2{px[0], px[1]};
                rec[1] = double2{px[2], px[3]};
            } else rej = 1;
        }
    }
    CountRejected(rej, rejected);
}

int LaunchFilmAdd(void *stream, const SceneView *svDev, const Args &a) {
    static_assert(sizeof(I2) == 8 && sizeof(F4) == 16, "a pixel is one 8-byte load, L4 / lambda4 / lambda_pdf4 one 16-byte load each");
    if (a.n <= 0) return 0;
    const dim3 grid((unsigned)(((size_t)a.n + BLOCK - 1) / BLOCK)), block(BLOCK);
    const I2 *pixel = reinterpret_cast<const I2 *>(a.pixelXY);
    const F4 *L4 = reinterpret_cast<const F4 *>(a.L4), *lambda4 = reinterpret_cast<const F4 *>(a.lambda4), *pdf4 = reinterpret_cast<const F4 *>(a.lambdaPdf4);
    if (a.spectral)
        hipLaunchKernelGGL(k_film_add<true>, grid, block, 0, (hipStream_t)stream, svDev, a.film, a.spectral, a.stamps, a.epoch, a.n, a.nDevice, pixel, L4, lambda4, pdf4,
                           a.filterWeight, a.rejected);
    else
        hipLaunchKernelGGL(k_film_add<false>, grid, block, 0, (hipStream_t)stream, svDev, a.film, a.spectral, a.stamps, a.epoch, a.n, a.nDevice, pixel, L4, lambda4, pdf4,
                           a.filterWeight, a.rejected);
    return (int)hipGetLastError();
}

}  // namespace filmadd
}  // namespace wf
