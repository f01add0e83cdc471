// wf_film_develop.h — the per-pixel bodies of the film's GetImage step, host + device (WF_HD): what the kernels of wf_film_develop.hip
// run per lane, restating csrc/host/image_io.cpp's FilmToRGB / SpectralFilmImage / GBufferFilmImage operation for operation (those host
// loops stay as they are: they are the witness tests/test_film_develop_gpu.py compares the kernels with, bit for bit).
// tools/film_develop_check.cpp compiles this header for the host: RoundToHalf below against image_io.cpp's over every float.
// Every function returns the number of channel values that were NaN and were stored as 0 (Image::SetChannel, util/image.h:425-432).
#pragma once
#include "../common/wf_math.h"
#include "../../../include/wf_abi.h"

namespace wf {
namespace develop {

constexpr int GBUFFER_CHANNELS = 25;   // R G B Albedo.RGB P.XYZ dzdx dzdy N.XYZ Ns.XYZ u v Variance.RGB RelativeVariance.RGB

WF_HD uint32_t Bits(float f) { uint32_t x; __builtin_memcpy(&x, &f, 4); return x; }
WF_HD float FromBits(uint32_t x) { float f; __builtin_memcpy(&f, &x, 4); return f; }

// float -> half -> float, round to nearest even (the twin of image_io.cpp's RoundToHalf, util/float.h Half(float))
WF_HD float RoundToHalf(float f) {
    const uint32_t x = Bits(f), sign = x & 0x80000000u, mag = x & 0x7fffffffu;
    if (mag >= 0x7f800000u) return f;  // inf / nan
    const float a = FromBits(mag);
    if (a >= 65520.f) return FromBits(sign | 0x7f800000u);
    float r;
    if (a < 6.103515625e-05f) {  // half subnormal range: quantum 2^-24
        const float q = a * 16777216.f;               // exact
        const float rq = __builtin_nearbyintf(q);     // RN-even (v_rndne_f32 on the device)
        r = rq / 16777216.f;
    } else {
        const uint32_t rem = mag & 0x1fffu;
        uint32_t base = mag & ~0x1fffu;
        if (rem > 0x1000u || (rem == 0x1000u && (base & 0x2000u))) base += 0x2000u;
        r = FromBits(base);
    }
    return FromBits(Bits(r) | sign);
}

// the film's outputRGBFromSensorRGB, by value (a kernel argument)
struct RGBMatrix { float m[3][3]; };
WF_HD RGBMatrix OutputMatrix(const wf_film &F) {
    RGBMatrix M;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) M.m[r][k] = F.outputRGBFromSensorRGB[r][k];
    return M;
}

// RGBFilm::GetPixelRGB + GetImage of one pixel (FilmToRGB): px = rgbSum[3], weightSum.  clamp: values above 65504 become 65504;
// round: RoundToHalf.  (FilmToRGB clamps, zeroes the NaNs and rounds; the spectral and GBuffer images zero the NaNs first — the same
// values either way: a NaN is not above 65504.)
WF_HD int DevelopRGB(const RGBMatrix &M, const double px[4], bool clamp, bool round, float o[3]) {
    float c[3] = {(float)px[0], (float)px[1], (float)px[2]};
    const float weightSum = (float)px[3];
    if (weightSum != 0) { c[0] /= weightSum; c[1] /= weightSum; c[2] /= weightSum; }
    int nan = 0;
    for (int r = 0; r < 3; ++r) {
        float v = 0;
        for (int k = 0; k < 3; ++k) v += M.m[r][k] * c[k];
        if (clamp && v > 65504.f) v = 65504.f;
        if (v != v) { ++nan; v = 0; }
        o[r] = round ? RoundToHalf(v) : v;
    }
    return nan;
}

// one bucket of SpectralFilm::GetImage (SpectralFilmImage)
WF_HD int DevelopBucket(double sum, double weight, bool saveFP16, float *out) {
    float c = 0;
    int nan = 0;
    if (weight > 0) {
        c = (float)(sum / weight);
        if (c != c) { nan = 1; c = 0; }
        if (saveFP16) { if (c > 65504.f) c = 65504.f; c = RoundToHalf(c); }
    }
    *out = c;
    return nan;
}

WF_HD void NormalizedOrZero(const float v[3], float n[3]) {
    const float l2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    if (!(l2 > 0)) { n[0] = n[1] = n[2] = 0; return; }
    const float l = __builtin_sqrtf(l2);
    n[0] = v[0] / l; n[1] = v[1] / l; n[2] = v[2] / l;
}

// GBufferFilm::GetImage of one pixel (GBufferFilmImage): only R, G and B are clamped, every channel is rounded
WF_HD int DevelopGBuffer(const RGBMatrix &M, const double px[4], const wf_gbuffer_pixel &g, bool saveFP16, float ch[GBUFFER_CHANNELS]) {
    int nan = DevelopRGB(M, px, saveFP16, saveFP16, ch);
    float alb[3] = {(float)g.rgb_albedo_sum[0], (float)g.rgb_albedo_sum[1], (float)g.rgb_albedo_sum[2]};
    const float weightSum = (float)px[3], gws = (float)g.gbuffer_weight_sum;
    float pt[3] = {g.p_sum[0], g.p_sum[1], g.p_sum[2]}, uv[2] = {g.uv_sum[0], g.uv_sum[1]}, dzdx = g.dzdx_sum, dzdy = g.dzdy_sum;
    if (weightSum != 0) for (int c = 0; c < 3; ++c) alb[c] /= weightSum;
    if (gws != 0) {
        for (int c = 0; c < 3; ++c) pt[c] /= gws;
        uv[0] /= gws; uv[1] /= gws;
        dzdx /= gws; dzdy /= gws;
    }
    float n[3], ns[3];
    NormalizedOrZero(g.n_sum, n);
    NormalizedOrZero(g.ns_sum, ns);
    float var[3], rel[3];
    for (int c = 0; c < 3; ++c) {
        var[c] = g.var_n[c] > 1 ? g.var_s[c] / (g.var_n[c] - 1) : 0.f;
        rel[c] = (g.var_n[c] < 1 || g.var_mean[c] == 0) ? 0.f : var[c] / g.var_mean[c];
    }
    const float rest[GBUFFER_CHANNELS - 3] = {alb[0], alb[1], alb[2], pt[0], pt[1], pt[2], __builtin_fabsf(dzdx), __builtin_fabsf(dzdy), n[0], n[1], n[2],
                                              ns[0], ns[1], ns[2], uv[0], uv[1], var[0], var[1], var[2], rel[0], rel[1], rel[2]};
    for (int c = 3; c < GBUFFER_CHANNELS; ++c) {
        float v = rest[c - 3];
        if (v != v) { ++nan; v = 0; }
        ch[c] = saveFP16 ? RoundToHalf(v) : v;
    }
    return nan;
}

// The launchers of wf_film_develop.hip (host): one kernel each on `stream`, no synchronisation.  dst = float32 [pixels][channels];
// nanCount = a device counter the kernel adds its NaN values to, or null.  Return hipError_t values (0 = launched).
int LaunchDevelopRGB(void *stream, const double *film, size_t pixels, const wf_film &F, bool saveFP16, float *dst, unsigned long long *nanCount);
int LaunchDevelopSpectral(void *stream, const double *film, const double *spectral, size_t pixels, const wf_film &F, bool saveFP16, float *dst,
                          unsigned long long *nanCount);
int LaunchDevelopGBuffer(void *stream, const double *film, const wf_gbuffer_pixel *gb, size_t pixels, const wf_film &F, bool saveFP16, float *dst,
                         unsigned long long *nanCount);

}  // namespace develop
}  // namespace wf
