// wf_film_add.h — the per-item bodies of wf_film_add_samples_device (include/wf_abi.h), host + device (WF_HD): Film::AddSample for a
// caller's sample, what UpdateFilm (wavefront/film.cpp:14-38) does for a pixel sample of the render.  The kernels of wf_film_add.hip run
// them one item per lane; tools/film_add_check.cpp compiles this header for the host and runs them against KUpdateFilm (wf_kernels.h),
// accumulators compared byte for byte.
//   RGB part       FilmSensorRGBW (wf_kernels.h), the value-taking core FilmSampleRGBW calls too: SafeDiv by the PDF, the three sensor
//                  products times imaging_ratio, the max_component_value rescale; then the four fp64 adds, as KUpdateFilm writes them
//   spectral part  SpectralFilm::AddSample beside the RGB accumulators (film.h:432-457), restated from KUpdateFilm line for line
// A GBuffer film gets the RGB part only: AddSample with a null VisibleSurface, KUpdateFilm's vp.w == 0 branch.
#pragma once
#include "../common/wf_kernels.h"

namespace wf {
namespace filmadd {

// UpdateFilm's InsideExclusive test and the pixel's record in the [pixels][4] film
WF_HD bool FilmIndex(const wf_film &F, I2 pp, size_t *idx) {
    if (!(pp.x >= F.pixel_min[0] && pp.x < F.pixel_max[0] && pp.y >= F.pixel_min[1] && pp.y < F.pixel_max[1])) return false;
    const int width = F.pixel_max[0] - F.pixel_min[0];
    *idx = (size_t)(pp.y - F.pixel_min[1]) * width + (pp.x - F.pixel_min[0]);
    return true;
}

// One sample per pixel and call: the item writes the call's epoch over the pixel's stamp and gets the stamp's old value back.  The old
// value is the epoch itself only if another item of the same call came first; that item owns the pixel, this one adds nothing.  One
// returning 4-byte atomic per lane, every lane at an address of its own (not the one-counter pattern of DESIGN 4.3).
WF_HD bool ClaimPixel(int32_t *stamp, int32_t epoch) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicExch(stamp, epoch) != epoch;
#else
    return __atomic_exchange_n(stamp, epoch, __ATOMIC_RELAXED) != epoch;
#endif
}

// The epoch of the call after the one of epoch `last` (0: none yet).  Epochs run 1 .. INT32_MAX and then over again from 1; *clear says
// that the stamps must be zeroed before this call's items, or a pixel last stamped in the earlier cycle's call of the same number would
// reject its first item.  The entry point's bookkeeping (wf_boundary.hip); the host program walks it across the wrap.
inline int32_t NextEpoch(int32_t last, bool *clear) {
    *clear = last == INT32_MAX;
    return *clear ? 1 : last + 1;
}

// The adds of one item that owns its pixel.  px: the pixel's rgbSum[3], weightSum (the caller loads and stores the record); sp: the
// pixel's bucketSums[n_buckets], weightSums[n_buckets] (SPECTRAL only).  Lw = the radiance times the camera-ray weight.
template <bool SPECTRAL>
WF_HD void AddSample(const SceneView &sv, double px[4], double *sp, S4 Lw, const Wavelengths &lambda, float filterWeight) {
    float v[4];
    FilmSensorRGBW(sv, Lw, lambda, filterWeight, v);
    px[0] += v[0];
    px[1] += v[1];
    px[2] += v[2];
    px[3] += v[3];
    if (SPECTRAL) {
        const wf_film &F = sv.film;
        S4 Ls = Lw;
        const float lm = Ls.MaxComponentValue();
        if (lm > F.max_component_value) Ls = Ls * (F.max_component_value / lm);
        Ls = Ls * (filterWeight * 106.856895f);
        for (int i = 0; i < 4; ++i) {
            int b = (int)(F.n_buckets * (lambda.lambda[i] - F.lambda_min) / (F.lambda_max - F.lambda_min));
            b = b < 0 ? 0 : (b > F.n_buckets - 1 ? F.n_buckets - 1 : b);
            sp[b] += Ls[i];
            sp[F.n_buckets + b] += filterWeight;
        }
    }
}

// The whole item on plain arrays (the host program's loop; the kernel does the same steps with 16-byte loads and stores of the record).
// Returns 1 for an item rejected as a second sample of its pixel, else 0 (added, or outside the pixel bounds and skipped).
template <bool SPECTRAL>
WF_HD int AddItem(const SceneView &sv, double *film, double *spectral, int32_t *stamps, int32_t epoch, I2 pp, F4 L, F4 lam, F4 pdf, float filterWeight) {
    size_t idx;
    if (!FilmIndex(sv.film, pp, &idx)) return 0;
    if (!ClaimPixel(stamps + idx, epoch)) return 1;
    Wavelengths w;
    w.lambda[0] = lam.x; w.lambda[1] = lam.y; w.lambda[2] = lam.z; w.lambda[3] = lam.w;
    w.pdf[0] = pdf.x; w.pdf[1] = pdf.y; w.pdf[2] = pdf.z; w.pdf[3] = pdf.w;
    double *px = film + 4 * idx;
    double a[4] = {px[0], px[1], px[2], px[3]};
    AddSample<SPECTRAL>(sv, a, SPECTRAL ? spectral + (size_t)2 * sv.film.n_buckets * idx : nullptr, toS4(L), w, filterWeight);
    px[0] = a[0]; px[1] = a[1]; px[2] = a[2]; px[3] = a[3];
    return 0;
}

// the launcher of wf_film_add.hip (hidden: shared by the library's units, not exported from it): k_film_add<spectral != null> over
// the items, one per lane.  svDev: the scene view's device-resident copy.  Returns a hipError_t (0: launched).
struct Args {
    double *film, *spectral;   // spectral: null unless the film is a spectral film
    int32_t *stamps;           // one per film pixel
    int32_t epoch;
    int n;
    const int32_t *nDevice;    // null, or the device word that caps n
    const int32_t *pixelXY;
    const float *L4, *lambda4, *lambdaPdf4, *filterWeight;
    uint32_t *rejected;        // null, or the device counter the rejected items are added to
};
__attribute__((visibility("hidden"))) int LaunchFilmAdd(void *stream, const SceneView *svDev, const Args &a);

}  // namespace filmadd
}  // namespace wf
