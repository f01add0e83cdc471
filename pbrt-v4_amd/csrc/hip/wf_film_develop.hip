// wf_film_develop.hip — the film's GetImage step on the device (gfx950): from the accumulators wf_update_film leaves in HBM to the final
// float32 [H][W][C] image in a caller-owned device buffer.  One pixel per lane, 256-thread blocks; the per-pixel arithmetic is
// wf_film_develop.h's, the restatement of image_io.cpp's host loops (bit-identical: -ffp-contract=off, IEEE division and sqrt).
// The C ABI entry points (wf_film_develop_device, ...) are in wf_results.hip; they call the launchers below.
#include <hip/hip_runtime.h>
#include "wf_film_develop.h"

namespace wf {
namespace develop {

constexpr int BLOCK = 256;

// NaN values of a wave -> the counter: one non-returning atomic from one lane, and only from a wave that saw one (every lane of the wave
// gets here: the ballot is wave-uniform, so is the branch).  A per-lane returning atomic is what DESIGN 4.3 took out of the medium stage.
__device__ inline void CountNaN(int nan, unsigned long long *counter) {
    if (counter == nullptr) return;
    if (__ballot(nan != 0) == 0) return;
    for (int d = 32; d > 0; d >>= 1) nan += __shfl_xor(nan, d);
    if ((threadIdx.x & 63) == 0) atomicAdd(counter, (unsigned long long)nan);
}

// the [pixels][4] double film: two 16-byte loads per lane
__device__ inline void LoadFilmPixel(const double *film, size_t i, double px[4]) {
    const double2 a = reinterpret_cast<const double2 *>(film)[2 * i], b = reinterpret_cast<const double2 *>(film)[2 * i + 1];
    px[0] = a.x; px[1] = a.y; px[2] = b.x; px[3] = b.y;
}

__global__ void __launch_bounds__(BLOCK) k_film_develop_rgb(const double *__restrict__ film, float *__restrict__ dst, size_t pixels, RGBMatrix M, int saveFP16,
                                                            unsigned long long *nanCount) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    int nan = 0;
    if (i < pixels) {
        double px[4];
        LoadFilmPixel(film, i, px);
        float o[3];
        nan = DevelopRGB(M, px, saveFP16 != 0, saveFP16 != 0, o);
        dst[3 * i] = o[0]; dst[3 * i + 1] = o[1]; dst[3 * i + 2] = o[2];
    }
    CountNaN(nan, nanCount);
}

__global__ void __launch_bounds__(BLOCK) k_film_develop_spectral(const double *__restrict__ film, const double *__restrict__ spectral, float *__restrict__ dst,
                                                                 size_t pixels, int nBuckets, RGBMatrix M, int saveFP16, unsigned long long *nanCount) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    int nan = 0;
    if (i < pixels) {
        double px[4];
        LoadFilmPixel(film, i, px);
        float *o = dst + i * (size_t)(3 + nBuckets);
        float rgb[3];
        nan = DevelopRGB(M, px, saveFP16 != 0, saveFP16 != 0, rgb);
        o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
        const double *sp = spectral + i * (size_t)(2 * nBuckets);   // bucketSums[nBuckets], weightSums[nBuckets]
        for (int b = 0; b < nBuckets; ++b) nan += DevelopBucket(sp[b], sp[nBuckets + b], saveFP16 != 0, &o[3 + b]);
    }
    CountNaN(nan, nanCount);
}

// GBuffer: the 136-byte wf_gbuffer_pixel record in and the 25 floats out are per-lane accesses (7 x 16-byte + 2 narrower loads, 6 x 16-byte
// + one 4-byte stores: neighbouring lanes fill each other's cache lines).  Staging both through LDS for coalesced rows was measured and is
// 13 % slower at 3840 x 2160 (34 KB of LDS halves the occupancy, two more barriers): DESIGN 4.4.
__global__ void __launch_bounds__(BLOCK) k_film_develop_gbuffer(const double *__restrict__ film, const wf_gbuffer_pixel *__restrict__ gb, float *__restrict__ dst,
                                                                size_t pixels, RGBMatrix M, int saveFP16, unsigned long long *nanCount) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    int nan = 0;
    if (i < pixels) {
        double px[4];
        LoadFilmPixel(film, i, px);
        const wf_gbuffer_pixel g = gb[i];
        float ch[GBUFFER_CHANNELS];
        nan = DevelopGBuffer(M, px, g, saveFP16 != 0, ch);
        float *o = dst + i * GBUFFER_CHANNELS;
#pragma unroll
        for (int c = 0; c < GBUFFER_CHANNELS; ++c) o[c] = ch[c];
    }
    CountNaN(nan, nanCount);
}

static unsigned GridFor(size_t pixels) { return (unsigned)((pixels + BLOCK - 1) / BLOCK); }

int LaunchDevelopRGB(void *stream, const double *film, size_t pixels, const wf_film &F, bool saveFP16, float *dst, unsigned long long *nanCount) {
    if (pixels == 0) return 0;
    hipLaunchKernelGGL(k_film_develop_rgb, dim3(GridFor(pixels)), dim3(BLOCK), 0, (hipStream_t)stream, film, dst, pixels, OutputMatrix(F), saveFP16 ? 1 : 0, nanCount);
    return (int)hipGetLastError();
}
int LaunchDevelopSpectral(void *stream, const double *film, const double *spectral, size_t pixels, const wf_film &F, bool saveFP16, float *dst,
                          unsigned long long *nanCount) {
    if (pixels == 0) return 0;
    hipLaunchKernelGGL(k_film_develop_spectral, dim3(GridFor(pixels)), dim3(BLOCK), 0, (hipStream_t)stream, film, spectral, dst, pixels, (int)F.n_buckets,
                       OutputMatrix(F), saveFP16 ? 1 : 0, nanCount);
    return (int)hipGetLastError();
}
int LaunchDevelopGBuffer(void *stream, const double *film, const wf_gbuffer_pixel *gb, size_t pixels, const wf_film &F, bool saveFP16, float *dst,
                         unsigned long long *nanCount) {
    if (pixels == 0) return 0;
    hipLaunchKernelGGL(k_film_develop_gbuffer, dim3(GridFor(pixels)), dim3(BLOCK), 0, (hipStream_t)stream, film, gb, dst, pixels,
                       OutputMatrix(F), saveFP16 ? 1 : 0, nanCount);
    return (int)hipGetLastError();
}

}  // namespace develop
}  // namespace wf
