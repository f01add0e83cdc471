// wf_boundary_light.h — the per-row bodies of wf_light_sample_device / wf_light_emitted_device (include/wf_abi.h) and the launchers of
// wf_boundary_light.hip.  The bodies are host + device: the kernels run them one row per lane, tools/light_sample_check.cpp compiles
// them for the host and runs them against the render's own functions.  They add no arithmetic of their own: a row's light sample is
// SampleLightDirect's (through SampleLightForBlock on the device), its shadow ray is MatNeeFinish's, its emission is KHandleEscaped's /
// KHandleEmissive's — what is left out is the BSDF, the path state and the queues.
//
// The planes are wf_hit_interaction_device's: item i of plane p is the 16 bytes at planes[p * n + i].
//   planes_f  0  pi lower | uv[0]    1  pi upper | uv[1]    2  n | time    3  ns | t    4  wo | 0
//   planes_i  0  material, area light, medium inside, medium outside        1  mesh, valid, mesh flags, 0
#pragma once
#include <cstddef>
#include <cstdint>
#include "../common/wf_kernels.h"

namespace wf {
namespace blight {

// ---- wf_light_sample_device ---------------------------------------------------------------------------------------------------------
// what a row reads.  valid != 1: nothing else is meaningful (the row asks for no light)
struct SampleItem {
    P3i pi{V3{0, 0, 0}, V3{0, 0, 0}};
    N3 n{0, 0, 0}, ns{0, 0, 0};
    V3 wo{0, 0, 0};
    float time = 0;
    int valid = 0, mediumInside = -1, mediumOutside = -1, side = 0;
    float u0 = 0;
    V2 u{0, 0};
    float lambda[4] = {0, 0, 0, 0};
};
// what a row writes: five 16-byte rows
struct SampleRow {
    F4 ray0{0, 0, 0, 0}, ray1{0, 0, 0, 0};   // o.xyz d.x | d.yz tMax time
    F4 L{0, 0, 0, 0}, wiPdf{0, 0, 0, 0};
    I4 light{-1, 0, 0, -1};                  // light id, bits of the PMF, flags, the shadow ray's medium
};
constexpr int LIGHT_FLAG_DELTA = 1;

WF_HD SampleItem LoadSampleItem(const F4 *planesF, const I4 *planesI, size_t N, size_t i, const F4 *lambda4, const F4 *u4, const int32_t *side) {
    SampleItem it;
    it.valid = planesI[N + i].y;
    if (it.valid != 1) return it;
    const F4 f0 = planesF[i], f1 = planesF[N + i], f2 = planesF[2 * N + i], f3 = planesF[3 * N + i], f4 = planesF[4 * N + i];
    const I4 ids = planesI[i];
    const F4 lam = lambda4[i], uu = u4[i];
    it.pi = P3i{V3{f0.x, f0.y, f0.z}, V3{f1.x, f1.y, f1.z}};
    it.n = N3{f2.x, f2.y, f2.z}; it.time = f2.w;
    it.ns = N3{f3.x, f3.y, f3.z};
    it.wo = V3{f4.x, f4.y, f4.z};
    it.mediumInside = ids.z; it.mediumOutside = ids.w;
    it.u0 = uu.x; it.u = V2{uu.y, uu.z};
    it.lambda[0] = lam.x; it.lambda[1] = lam.y; it.lambda[2] = lam.z; it.lambda[3] = lam.w;
    if (side != nullptr) { const int s = side[i]; it.side = s == 1 || s == -1 ? s : 0; }
    return it;
}
// The LightSampleContext of the row (MatShade's rule for the NeeItem, wf_kernels.h; surfscatter.cpp:256-261, with the side in the
// caller's hands) and the request of the workgroup's light sampling, as MatNeeRequest builds it
WF_HD NeeRequest SampleRequest(const SampleItem &it) {
    NeeRequest r;
    r.want = it.valid == 1;
    if (!r.want) return r;
    P3i pi = it.pi;
    if (it.side > 0) pi = MakeP3i(OffsetRayOrigin(it.pi, it.n, it.wo));
    else if (it.side < 0) pi = MakeP3i(OffsetRayOrigin(it.pi, it.n, -it.wo));
    r.ctx = LightCtx{pi, it.n, it.ns};
    r.u0 = it.u0; r.u = it.u;
    for (int k = 0; k < 4; ++k) { r.lambda.lambda[k] = it.lambda[k]; r.lambda.pdf[k] = 0; }   // (the lights read the wavelengths only)
    return r;
}
// ... and what MatNeeFinish does with the sample before and after its BSDF: the test for going on, the shadow ray, its medium
WF_HD SampleRow SampleFinish(const SceneView &sv, const SampleItem &it, const LightPick &pick) {
    SampleRow row;
    if (it.valid != 1 || pick.lightId < 0) return row;
    const wf_light &light = sv.lights[pick.lightId];
    row.light = I4{pick.lightId, (int32_t)FloatToBits(pick.pmf), IsDeltaLight(light) ? LIGHT_FLAG_DELTA : 0, -1};
    const LightLiSample &ls = pick.ls;
    if (!(ls.valid && ls.L && ls.pdf != 0)) return row;
    // a row without a normal is a point in a medium (include/wf_abi.h; wfpt.Scene.medium_light_planes): its shadow ray is
    // SampleMediumScattering's, Ray(p, pLight.p() - p) (wavefront/media.cpp:300) — no offset at either end; p = the interval's midpoint
    const bool inMedium = it.n.x == 0 && it.n.y == 0 && it.n.z == 0;
    const RayOD sr = inMedium ? RayOD{it.pi.mid(), ls.pLightPi.mid() - it.pi.mid()} : SpawnRayTo(it.pi, it.n, ls.pLightPi, ls.pLightN);
    if (sv.haveMedia) row.light.w = Dot(sr.d, it.n) > 0 ? it.mediumOutside : it.mediumInside;   // SurfaceMedium
    row.ray0 = F4{sr.o.x, sr.o.y, sr.o.z, sr.d.x};
    row.ray1 = F4{sr.d.y, sr.d.z, 1 - ShadowEpsilon, it.time};
    row.L = toF4(ls.L);
    row.wiPdf = F4{ls.wi.x, ls.wi.y, ls.wi.z, ls.pdf};
    return row;
}

// ---- wf_light_emitted_device --------------------------------------------------------------------------------------------------------
struct EmittedRow {
    F4 Le{0, 0, 0, 0}, pmfPdf{0, 0, 0, 0};   // pmf, pdf, 0, 0
};
// planes 0 - 3 of the vertex the ray left, as LoadCtx reads the ray queue's copy
WF_HD LightCtx LoadPrevCtx(const F4 *prevF, size_t N, size_t i) {
    const F4 a = prevF[i], b = prevF[N + i], c = prevF[2 * N + i], d = prevF[3 * N + i];
    return LightCtx{P3i{V3{a.x, a.y, a.z}, V3{b.x, b.y, b.z}}, N3{c.x, c.y, c.z}, N3{d.x, d.y, d.z}};
}
// PORTAL: the scene has a portal infinite light (LightLe<RARE>, LightPDF_Li<false, RARE>); ALPHA: an emitter with an alpha texture
// (AreaLightL<ALPHA>); AREA_RARE: an emitter that is not a triangle (LightPDF_Li<true, RARE> of a hit).  A kernel is allocated what
// it can reach; the variants agree bit for bit on the scenes the lean ones serve.
template <bool PORTAL, bool ALPHA, bool AREA_RARE>
WF_HD EmittedRow EmittedItem(const SceneView &sv, const F4 *rays, const F4 *planesF, const I4 *planesI, size_t N, size_t i, const F4 *lambda4, int infiniteIndex,
                             const F4 *prevF) {
    EmittedRow row;
    const int valid = planesI[N + i].y;
    if (valid != 0 && valid != 1) return row;
    const F4 lam = lambda4[i];
    Wavelengths lambda;
    lambda.lambda[0] = lam.x; lambda.lambda[1] = lam.y; lambda.lambda[2] = lam.z; lambda.lambda[3] = lam.w;
    for (int k = 0; k < 4; ++k) lambda.pdf[k] = 0;   // (the lights read the wavelengths only)
    if (valid == 1) {
        // HandleEmissiveIntersection (KHandleEmissive): the hit's own emission, once — with the first infinite light's term
        const int lightId = planesI[i].y;
        if (infiniteIndex != 0 || lightId < 0 || lightId >= sv.nLights) return row;   // (a stale buffer does not walk the tables)
        const wf_light &light = sv.lights[lightId];
        if (light.type != WF_LIGHT_DIFFUSE_AREA) return row;
        const F4 f0 = planesF[i], f1 = planesF[N + i], f2 = planesF[2 * N + i], f4 = planesF[4 * N + i];
        const P3i pi{V3{f0.x, f0.y, f0.z}, V3{f1.x, f1.y, f1.z}};
        const V3 wo{f4.x, f4.y, f4.z};
        const S4 Le = AreaLightL<ALPHA>(sv, light, pi.mid(), N3{f2.x, f2.y, f2.z}, V2{f0.w, f1.w}, wo, lambda);
        if (!Le) return row;
        row.Le = toF4(Le);
        if (prevF != nullptr) {
            const LightCtx ctx = LoadPrevCtx(prevF, N, i);
            row.pmfPdf.x = LightSamplerPMF(sv, ctx, lightId);
            row.pmfPdf.y = LightPDF_Li<true, AREA_RARE>(sv, light, ctx, -wo, true);
        }
        return row;
    }
    // HandleEscapedRays (KHandleEscaped): one infinite light's term
    if (infiniteIndex < 0 || infiniteIndex >= sv.nInfiniteLights) return row;
    const F4 r0 = rays[2 * i], r1 = rays[2 * i + 1];   // o.xyz d.x | d.yz tMax time
    const V3 rayo{r0.x, r0.y, r0.z}, rayd{r0.w, r1.x, r1.y};
    const int lightId = sv.infiniteLights[infiniteIndex];
    const wf_light &light = sv.lights[lightId];
    const S4 Le = LightLe<PORTAL>(sv, light, rayo, rayd, lambda);
    if (!Le) return row;
    row.Le = toF4(Le);
    if (prevF != nullptr) {
        const LightCtx ctx = LoadPrevCtx(prevF, N, i);
        row.pmfPdf.x = LightSamplerPMF(sv, ctx, lightId);
        row.pmfPdf.y = LightPDF_Li<false, PORTAL>(sv, light, ctx, rayd, true);   // (infinite lights only)
    }
    return row;
}

// The launchers of wf_boundary_light.hip (hidden: shared by the library's units, not exported from it).  svDev: the scene view's
// device-resident copy.  Return a hipError_t (0: launched); -1: no such variant.
struct SampleArgs {
    int n = 0;
    const int32_t *nDevice = nullptr;
    const float *planesF = nullptr, *lambda4 = nullptr, *u4 = nullptr;
    const int32_t *planesI = nullptr, *side = nullptr;
    float *rays8 = nullptr, *L4 = nullptr, *wiPdf4 = nullptr;
    int32_t *light4 = nullptr;
};
struct EmittedArgs {
    int n = 0, infiniteIndex = 0;
    const int32_t *nDevice = nullptr;
    const float *rays8 = nullptr, *planesF = nullptr, *lambda4 = nullptr, *prevF = nullptr;
    const int32_t *planesI = nullptr;
    float *Le4 = nullptr, *pmfPdf4 = nullptr;
};
__attribute__((visibility("hidden"))) int LaunchLightSample(void *stream, bool rare, const SceneView *svDev, const SampleArgs &a);
__attribute__((visibility("hidden"))) int LaunchLightEmitted(void *stream, int variant, const SceneView *svDev, const EmittedArgs &a);

}  // namespace blight
}  // namespace wf
