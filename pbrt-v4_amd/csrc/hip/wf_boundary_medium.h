// wf_boundary_medium.h — the per-row bodies of wf_medium_sample_device / wf_phase_device (include/wf_media.h) and the launchers of
// wf_boundary_medium.hip.  The bodies are host + device: the kernels run them one row per lane, tools/medium_check.cpp compiles them
// for the host and runs them against the render's own KSampleMediumInteraction / KSampleMediumScattering on a one-slot WorkState.
//
// The medium row is the render's delta-tracking sequence — MediumTrackBegin / Step / Event / End of csrc/common/wf_kernels.h — restated
// beside it WITHOUT the WorkState: the render's bodies read and write the ray queue slot, the pixel's L and the scatter / route /
// escaped queues, and a change to them would be a change to the render's device code.  What is shared is everything below them:
// MediumSpectra, MediumSampleRay<LEAN>, MajorantIter::Next, SampleExponential, MediumSamplePoint<LEAN>, SampleDiscreteN, FastExp
// (csrc/common/wf_media.h).  The arithmetic of an event is MediumTrackEvent's, expression for expression; `depth < maxDepth` is the
// caller's flag bit 0.
//
// TERMINATION (a row is a lane of a kernel on a machine other people use).  A row runs RowBegin, then RowStep until it returns false.
//   * Rows that are not walked at all are filtered in LoadTrackItem, before the loop: a medium id that is not in the table (kind 0), an
//     origin that is not finite, a direction whose squared length is not a finite positive number (a zero, an underflowing, an
//     overflowing, an infinite or a NaN direction: Normalize would produce a zero or non-finite vector), a NaN or negative tMax — and a
//     row in no medium (medium < 0, kind 1).  The tables are indexed by the id only after that check.
//   * The OUTER sequence (one majorant segment per RowStep with inSeg false) is MajorantIter::Next.  A homogeneous medium and the cloud
//     give ONE segment (`called`), whatever tMax is — an infinite tMax is one segment [0, inf).  The DDA iterator moves one voxel towards
//     voxelLimit per call or sets tMin = tMax: at most res.x + res.y + res.z calls from a voxel inside the grid, and RowBegin ends the
//     iteration of a row whose first voxel is not inside it (a non-finite grid coordinate; the render's rays never have one).  Its first
//     line is the NaN guard `!(tMin < tMax)` that the golden scene nan_ray_grid_medium pins: a NaN interval ends the iteration at once.
//     A segment whose majorant is zero takes no tentative collision: it multiplies T_maj and the next RowStep fetches the next segment.
//   * The INNER sequence (tentative collisions inside one segment) ends when t = tMin + SampleExponential(u, sigma_maj[0]) reaches the
//     segment's tMax, or at an absorption or a real scatter, or at a null collision that leaves beta or r_u black.  In a homogeneous
//     medium sigma_maj = sigma_a + sigma_s, so the null probability is a rounding error and sigma_n is 0 or one ulp: a collision ends
//     the row, also with tMax = inf.  In a grid the segment is finite and t grows by a positive exponential step, but nothing in the
//     arithmetic bounds the count (a majorant of 1e30 in an empty voxel would step by less than an ulp of t for ever), so the count
//     itself is bounded: after WF_MEDIUM_ROW_MAX_STEPS = 2^20 tentative collisions the row ends where it stands as kind 2.  (The most a
//     row took so far: 15 among tools/medium_check --self's rows on nine scenes, 19 among the 2^18 of profiles/medium_device.txt.)
// Nothing shared is touched inside the loop (no queue, no atomic, no store): a row's outputs are written once, after it.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../common/wf_kernels.h"

namespace wf {
namespace bmedium {

constexpr int WF_MEDIUM_ROW_MAX_STEPS = 1 << 20;
constexpr int KIND_NONE = 0, KIND_ARRIVED = 1, KIND_ENDED = 2, KIND_SCATTER = 3;
constexpr int FLAG_EMISSION = 1;

// what a row writes: six 16-byte rows
struct TrackRow {
    I4 event{0, 0, 0, 0};   // kind, tentative collisions taken, 0, 0
    F4 pG{0, 0, 0, 0};      // the scattering point and the phase function's g (kind 3)
    F4 beta{0, 0, 0, 0}, r_u{0, 0, 0, 0}, r_l{0, 0, 0, 0}, L{0, 0, 0, 0};
};
// what a row reads.  kind: KIND_NONE — no row; KIND_ARRIVED — in no medium, the spectra go through; -1 — walk it
struct TrackItem {
    int kind = KIND_NONE, medium = -1, flags = 0;
    V3 o{0, 0, 0}, d{0, 0, 0};
    float tMax = 0;
    F4 lambda{0, 0, 0, 0}, beta{0, 0, 0, 0}, r_u{0, 0, 0, 0}, r_l{0, 0, 0, 0};
};
WF_HD TrackItem LoadTrackItem(int nMedia, const F4 *rays, const int32_t *medium, const F4 *lambda4, const F4 *beta4, const F4 *ru4, const F4 *rl4,
                              const int32_t *flags, size_t i) {
    TrackItem it;
    it.medium = medium[i];
    if (it.medium >= nMedia) return it;
    const F4 r0 = rays[2 * i], r1 = rays[2 * i + 1];   // o.xyz d.x | d.yz tMax time
    it.o = V3{r0.x, r0.y, r0.z}; it.d = V3{r0.w, r1.x, r1.y}; it.tMax = r1.z;
    it.beta = beta4[i]; it.r_u = ru4[i]; it.r_l = rl4[i];
    if (it.medium < 0) { it.kind = KIND_ARRIVED; return it; }
    const float l2 = LengthSquared(it.d);
    if (!(IsFinite(it.o.x) && IsFinite(it.o.y) && IsFinite(it.o.z)) || !(l2 > 0 && IsFinite(l2)) || !(it.tMax >= 0)) return it;
    it.lambda = lambda4[i];
    it.flags = flags != nullptr ? flags[i] : FLAG_EMISSION;
    it.kind = -1;
    return it;
}

// MediumTrack (wf_kernels.h) without the ray slot, the pixel and the depth; `steps` counts the tentative collisions
struct RowTrack {
    int medium, steps;
    bool emission;
    V3 o, d;             // origin, NORMALISED direction
    MediumAtLambda ml;
    MajorantIter iter;
    MajorantSeg seg;
    float tMin;
    bool inSeg, scattered, stopped, usable;   // usable: the scatter left beta and r_u non-black (the render pushes a MediumScatterWorkItem)
    S4 T_maj, beta, r_u, r_l, L;
    F4 pG;
    RNG rng;
    float u, uMode;
};
// MediumTrackBegin
template <bool LEAN>
WF_HD void RowBegin(const SceneView &sv, const TrackItem &it, RowTrack &s) {
    s.medium = it.medium; s.steps = 0;
    s.emission = (it.flags & FLAG_EMISSION) != 0;
    float tMax = it.tMax;
    Wavelengths lambda;
    lambda.lambda[0] = it.lambda.x; lambda.lambda[1] = it.lambda.y; lambda.lambda[2] = it.lambda.z; lambda.lambda[3] = it.lambda.w;
    for (int k = 0; k < 4; ++k) lambda.pdf[k] = 0;   // (the media read the wavelengths only)
    s.beta = toS4(it.beta); s.r_u = toS4(it.r_u); s.r_l = toS4(it.r_l);
    s.L = S4c(0.f);
    s.pG = F4{0, 0, 0, 0};
    s.rng = RNG(Hash3f1(it.o, tMax), Hash3f(it.d));
    s.scattered = false;
    s.stopped = false;
    s.usable = false;
    s.u = s.rng.UniformFloat();
    s.uMode = s.rng.UniformFloat();
    // SampleT_maj's preamble (media.h:728-741)
    const wf_medium &M = sv.media[s.medium];
    tMax *= Length(it.d);
    s.o = it.o;
    s.d = Normalize(it.d);
    s.ml = MediumSpectra(sv, M, lambda);
    s.iter = MediumSampleRay<LEAN>(sv, M, s.ml, s.o, s.d, tMax);
    // (see TERMINATION: the DDA walk starts from a voxel of the grid, or not at all)
    if (!s.iter.homogeneous && s.iter.tMin < s.iter.tMax)
        for (int a = 0; a < 3; ++a)
            if (!(s.iter.voxel[a] >= 0 && s.iter.voxel[a] < s.iter.res[a])) s.iter.tMin = s.iter.tMax;
    s.T_maj = S4c(1.f);
    s.inSeg = false;
    s.tMin = 0;
}
// MediumTrackEvent: the callback of SampleMediumInteraction (wavefront/media.cpp:60-140) at a tentative collision; false = the walk ends here
WF_HD bool RowEvent(RowTrack &s, V3 p, const MediumProps &mp, S4 sigma_maj, S4 T_maj) {
    // emission, scaled by sigma_a / sigma_maj at every event (media.cpp:72-83)
    if (s.emission && mp.Le) {
        float pr = sigma_maj[0] * T_maj[0];
        S4 r_e = s.r_u * sigma_maj * T_maj / pr;
        if (r_e) s.L = s.L + s.beta * mp.sigma_a * T_maj * mp.Le / (pr * r_e.Average());
    }
    float pAbsorb = mp.sigma_a[0] / sigma_maj[0];
    float pScatter = mp.sigma_s[0] / sigma_maj[0];
    float pNull = fmax(0.f, 1 - pAbsorb - pScatter);
    const float w3[3] = {pAbsorb, pScatter, pNull};
    int mode = SampleDiscreteN(w3, 3, s.uMode);
    if (mode == 0) {
        s.beta = S4c(0.f);
        return false;
    } else if (mode == 1) {
        float pr = T_maj[0] * mp.sigma_s[0];
        s.beta = s.beta * (T_maj * mp.sigma_s / pr);
        s.r_u = s.r_u * (T_maj * mp.sigma_s / pr);
        if (s.beta && s.r_u) {
            s.pG = F4{p.x, p.y, p.z, mp.g};
            s.usable = true;
        }
        s.scattered = true;
        return false;
    } else {
        S4 sigma_n = ClampZero(sigma_maj - mp.sigma_a - mp.sigma_s);
        float pr = T_maj[0] * sigma_n[0];
        s.beta = s.beta * (T_maj * sigma_n / pr);
        if (pr == 0) s.beta = S4c(0.f);
        s.r_u = s.r_u * (T_maj * sigma_n / pr);
        s.r_l = s.r_l * (T_maj * sigma_maj / pr);
        s.uMode = s.rng.UniformFloat();
        return bool(s.beta) && bool(s.r_u);
    }
}
// MediumTrackStep: at most one majorant segment fetched and one tentative collision taken; false = the row is finished
template <bool LEAN>
WF_HD bool RowStep(const SceneView &sv, RowTrack &s) {
    if (!s.inSeg) {
        if (!s.iter.Next(&s.seg)) return false;
        if (s.seg.sigma_maj[0] == 0) {
            float dt = s.seg.tMax - s.seg.tMin;
            if (IsInf(dt)) dt = WF_FLT_MAX;
            s.T_maj = s.T_maj * FastExp(-dt * s.seg.sigma_maj);
            return true;
        }
        s.tMin = s.seg.tMin;
        s.inSeg = true;
    }
    float t = s.tMin + SampleExponential(s.u, s.seg.sigma_maj[0]);
    s.u = s.rng.UniformFloat();
    if (t < s.seg.tMax) {
        s.T_maj = s.T_maj * FastExp(-(t - s.tMin) * s.seg.sigma_maj);
        V3 p = s.o + s.d * t;
        const wf_medium &M = sv.media[s.medium];
        MediumProps mp = MediumSamplePoint<LEAN>(sv, M, s.ml, p);
        ++s.steps;
        if (!RowEvent(s, p, mp, s.seg.sigma_maj, s.T_maj) || s.steps >= WF_MEDIUM_ROW_MAX_STEPS) {
            s.stopped = true;
            return false;
        }
        s.T_maj = S4c(1.f);
        s.tMin = t;
    } else {
        float dt = s.seg.tMax - s.tMin;
        if (IsInf(dt)) dt = WF_FLT_MAX;
        s.T_maj = s.T_maj * FastExp(-dt * s.seg.sigma_maj);
        s.inSeg = false;
    }
    return true;
}
// MediumTrackEnd without the queues: what the render writes back into the ray slot (kinds 1 and 3) or holds when it drops the item (kind 2).
// entry_r_l: a scattered row keeps the r_l it came with — the render's scatter item carries none, the next ray's is r_u / pdf
WF_HD TrackRow RowEnd(const RowTrack &s, F4 entry_r_l) {
    TrackRow row;
    const S4 T_maj = s.stopped ? S4c(1.f) : s.T_maj;
    S4 beta = s.beta, r_u = s.r_u, r_l = s.r_l;
    if (!s.scattered && beta) {
        beta = beta * (T_maj / T_maj[0]);
        r_u = r_u * (T_maj / T_maj[0]);
        r_l = r_l * (T_maj / T_maj[0]);
    }
    const bool capped = s.steps >= WF_MEDIUM_ROW_MAX_STEPS;
    const int kind = s.scattered ? (s.usable ? KIND_SCATTER : KIND_ENDED) : (!capped && beta && r_u ? KIND_ARRIVED : KIND_ENDED);
    row.event = I4{kind, s.steps, 0, 0};
    row.pG = s.pG;
    row.beta = toF4(beta); row.r_u = toF4(r_u);
    row.r_l = kind == KIND_SCATTER ? entry_r_l : toF4(r_l);
    row.L = toF4(s.L);
    return row;
}
// a row that is not walked: zeros, or the spectra of a ray in no medium as they came
WF_HD TrackRow UnwalkedRow(const TrackItem &it) {
    TrackRow row;
    if (it.kind != KIND_ARRIVED) return row;
    row.event.x = KIND_ARRIVED;
    row.beta = it.beta; row.r_u = it.r_u; row.r_l = it.r_l;
    return row;
}
// the whole row, as the host runs it (the kernel runs the same pieces with its stores behind the loop)
template <bool LEAN>
WF_HD TrackRow TrackItemRow(const SceneView &sv, const TrackItem &it) {
    if (it.kind >= 0) return UnwalkedRow(it);
    RowTrack s;
    RowBegin<LEAN>(sv, it, s);
    while (RowStep<LEAN>(sv, s)) {}
    return RowEnd(s, it.r_l);
}

// ---- wf_phase_device: the phase-function half of SampleMediumScattering (wavefront/media.cpp:270-348), Henyey-Greenstein -----------------
struct PhaseRow {
    F4 pPdf{0, 0, 0, 0};                       // phase.p(wo, wi), phase.PDF(wo, wi), 0, 0
    F4 sample{0, 0, 0, 0};                     // Sample_p: p, pdf, 0, 0
    F4 ray0{0, 0, 0, 0}, ray1{0, 0, 0, 0};     // the next ray: o.xyz d.x | d.yz tMax time
};
WF_HD PhaseRow PhaseItem(const F4 *rays, const F4 *pG4, const F4 *wi4, const F4 *u4, size_t i) {
    PhaseRow row;
    const F4 r0 = rays[2 * i], r1 = rays[2 * i + 1], sp = pG4[i];
    const V3 wo{-r0.w, -r1.x, -r1.y};   // unnormalised, as KSampleMediumScattering carries it
    const float g = sp.w;
    if (wi4 != nullptr) {
        const F4 w = wi4[i];
        const V3 wi{w.x, w.y, w.z};
        // HGPhaseFunction::p and ::PDF are the same function of the same arguments (media.h:50-66)
        row.pPdf = F4{HenyeyGreenstein(Dot(wo, wi), g), HenyeyGreenstein(Dot(wo, wi), g), 0, 0};
    }
    if (u4 != nullptr) {
        const F4 u = u4[i];
        float pdf = 0;
        const V3 wi = SampleHenyeyGreenstein(wo, g, V2{u.x, u.y}, &pdf);
        if (pdf != 0) {
            row.sample = F4{pdf, pdf, 0, 0};   // phaseSample->p == phaseSample->pdf
            row.ray0 = F4{sp.x, sp.y, sp.z, wi.x};
            row.ray1 = F4{wi.y, wi.z, WF_INFINITY, r1.w};
        }
    }
    return row;
}

// The launchers of wf_boundary_medium.hip (hidden: shared by the library's units, not exported from it).  svDev: the scene view's
// device-resident copy.  Return a hipError_t (0: launched).
struct TrackArgs {
    int n = 0, nMedia = 0;
    const int32_t *nDevice = nullptr;
    const float *rays8 = nullptr, *lambda4 = nullptr, *beta4 = nullptr, *ru4 = nullptr, *rl4 = nullptr;
    const int32_t *medium = nullptr, *flags = nullptr;
    int32_t *event4 = nullptr;
    float *pG4 = nullptr, *outBeta4 = nullptr, *outRu4 = nullptr, *outRl4 = nullptr, *L4 = nullptr;
};
struct PhaseArgs {
    int n = 0;
    const int32_t *nDevice = nullptr;
    const float *rays8 = nullptr, *pG4 = nullptr, *wi4 = nullptr, *u4 = nullptr;
    float *pPdf4 = nullptr, *sample4 = nullptr, *nextRays8 = nullptr;
};
__attribute__((visibility("hidden"))) int LaunchMediumTrack(void *stream, bool lean, const SceneView *svDev, const TrackArgs &a);
__attribute__((visibility("hidden"))) int LaunchPhase(void *stream, const PhaseArgs &a);

}  // namespace bmedium
}  // namespace wf
