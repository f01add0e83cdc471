// tools/light_sample_check.cpp — the per-row bodies of wf_light_sample_device / wf_light_emitted_device
// (pbrt-v4_amd/csrc/hip/wf_boundary_light.h) compiled for the host, and the render's own light functions composed directly
// (SampleLightDirect<true>, SpawnRayTo, LightSamplerPMF, LightPDF_Li, LightLe, AreaLightL: csrc/common/wf_kernels.h, wf_lights.h) on a
// scene file's light tables.  Stand-alone: the parser and BuildSceneTables, no device, neither library.
//
//   light_sample_check [--datadir DIR] --self SCENE N
//       N pseudo-random rows for each call — contexts inside the scene's bounds, every side, misses and invalid rows between them,
//       emitter rows on the emitters' own triangles seen from a previous vertex that faces them, escaped rays, every infinite index —
//       through the new bodies and through the direct composition; every output word must be equal.  Exits non-zero otherwise.
//   light_sample_check [--datadir DIR] --eval SCENE in.bin out.bin
//       the DIRECT COMPOSITION's outputs for the rows of in.bin (not the new header's): the expected values of the GPU tests.
//       in.bin   int32 {magic 0x4c534331, call (0 sample, 1 emitted), n, infinite_index, has_side, has_prev, 0, 0}
//                planes_f [11][n][4] f32, planes_i [2][n][4] i32, lambda4 [n][4]
//                call 0: u4 [n][4], side [n] if has_side        call 1: rays8 [n][8], prev_planes_f [4][n][4] if has_prev
//       out.bin  call 0: shadow_rays8 [n][8], L4 [n][4], wi_pdf4 [n][4], light4 [n][4] i32      call 1: Le4 [n][4], pmf_pdf4 [n][4]
// Built with -fsanitize=address,undefined it is how that code is run under the sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../pbrt-v4_amd/csrc/hip/wf_boundary_light.h"
#include "check_common.h"

using namespace wf;

namespace {

constexpr int32_t MAGIC = 0x4c534331;

struct Rows {
    int call = 0, n = 0, infiniteIndex = 0;
    std::vector<F4> planesF, lambda4, u4, rays, prev;
    std::vector<I4> planesI;
    std::vector<int32_t> side;
    bool hasSide = false, hasPrev = false;
};

// ---- the direct composition: the render's functions, called as its stages call them ---------------------------------------------
void DirectSample(const SceneView &sv, const Rows &r, size_t i, F4 out[4], I4 *light) {
    const size_t N = (size_t)r.n;
    out[0] = out[1] = out[2] = out[3] = F4{0, 0, 0, 0};
    *light = I4{-1, 0, 0, -1};
    if (r.planesI[N + i].y != 1) return;
    const F4 lo = r.planesF[i], hi = r.planesF[N + i], nn = r.planesF[2 * N + i], sn = r.planesF[3 * N + i], w = r.planesF[4 * N + i];
    const P3i pi{V3{lo.x, lo.y, lo.z}, V3{hi.x, hi.y, hi.z}};
    const N3 n{nn.x, nn.y, nn.z}, ns{sn.x, sn.y, sn.z};
    const V3 wo{w.x, w.y, w.z};
    const int s = r.hasSide ? r.side[i] : 0;
    // surfscatter.cpp:256-261
    LightCtx ctx{pi, n, ns};
    if (s == 1) ctx.pi = MakeP3i(OffsetRayOrigin(pi, n, wo));
    else if (s == -1) ctx.pi = MakeP3i(OffsetRayOrigin(pi, n, -wo));
    Wavelengths lambda{};
    memcpy(lambda.lambda, &r.lambda4[i], 16);
    const LightPick pk = SampleLightDirect<true>(sv, ctx, r.u4[i].x, V2{r.u4[i].y, r.u4[i].z}, lambda);
    if (pk.lightId < 0) return;
    *light = I4{pk.lightId, (int32_t)FloatToBits(pk.pmf), IsDeltaLight(sv.lights[pk.lightId]) ? 1 : 0, -1};
    if (!pk.ls.valid || !pk.ls.L || pk.ls.pdf == 0) return;
    // (a row without a normal is a point in a medium: KSampleMediumScattering's shadow ray, p to the light's point as it is)
    const RayOD ray = n.x == 0 && n.y == 0 && n.z == 0 ? RayOD{pi.mid(), pk.ls.pLightPi.mid() - pi.mid()} : SpawnRayTo(pi, n, pk.ls.pLightPi, pk.ls.pLightN);
    if (sv.haveMedia) light->w = Dot(ray.d, n) > 0 ? r.planesI[i].w : r.planesI[i].z;
    out[0] = F4{ray.o.x, ray.o.y, ray.o.z, ray.d.x};
    out[1] = F4{ray.d.y, ray.d.z, 1 - ShadowEpsilon, nn.w};
    out[2] = toF4(pk.ls.L);
    out[3] = F4{pk.ls.wi.x, pk.ls.wi.y, pk.ls.wi.z, pk.ls.pdf};
}

void DirectEmitted(const SceneView &sv, const Rows &r, size_t i, F4 out[2]) {
    const size_t N = (size_t)r.n;
    out[0] = out[1] = F4{0, 0, 0, 0};
    const int valid = r.planesI[N + i].y;
    Wavelengths lambda{};
    memcpy(lambda.lambda, &r.lambda4[i], 16);
    LightCtx prev{};
    if (r.hasPrev) {
        const F4 a = r.prev[i], b = r.prev[N + i], c = r.prev[2 * N + i], d = r.prev[3 * N + i];
        prev = LightCtx{P3i{V3{a.x, a.y, a.z}, V3{b.x, b.y, b.z}}, N3{c.x, c.y, c.z}, N3{d.x, d.y, d.z}};
    }
    if (valid == 1) {
        const int id = r.planesI[i].y;
        if (r.infiniteIndex != 0 || id < 0 || id >= sv.nLights || sv.lights[id].type != WF_LIGHT_DIFFUSE_AREA) return;
        const wf_light &light = sv.lights[id];
        const F4 lo = r.planesF[i], hi = r.planesF[N + i], nn = r.planesF[2 * N + i], w = r.planesF[4 * N + i];
        const P3i pi{V3{lo.x, lo.y, lo.z}, V3{hi.x, hi.y, hi.z}};
        const V3 wo{w.x, w.y, w.z};
        // KHandleEmissive
        const S4 Le = AreaLightL(sv, light, pi.mid(), N3{nn.x, nn.y, nn.z}, V2{lo.w, hi.w}, wo, lambda);
        if (!Le) return;
        out[0] = toF4(Le);
        if (r.hasPrev) {
            out[1].x = LightSamplerPMF(sv, prev, id);
            out[1].y = LightPDF_Li(sv, light, prev, -wo, true);
        }
    } else if (valid == 0) {
        if (r.infiniteIndex >= sv.nInfiniteLights) return;
        // KHandleEscaped
        const int id = sv.infiniteLights[r.infiniteIndex];
        const wf_light &light = sv.lights[id];
        const F4 r0 = r.rays[2 * i], r1 = r.rays[2 * i + 1];
        const V3 o{r0.x, r0.y, r0.z}, d{r0.w, r1.x, r1.y};
        const S4 Le = LightLe(sv, light, o, d, lambda);
        if (!Le) return;
        out[0] = toF4(Le);
        if (r.hasPrev) {
            out[1].x = LightSamplerPMF(sv, prev, id);
            out[1].y = LightPDF_Li<false, true>(sv, light, prev, d, true);
        }
    }
}

// ---- the new bodies, as the kernels run them -------------------------------------------------------------------------------------
void BodySample(const SceneView &sv, const Rows &r, size_t i, F4 out[4], I4 *light) {
    const blight::SampleItem it = blight::LoadSampleItem(r.planesF.data(), r.planesI.data(), (size_t)r.n, i, r.lambda4.data(), r.u4.data(), r.hasSide ? r.side.data() : nullptr);
    const NeeRequest rq = blight::SampleRequest(it);
    const LightPick pick = SampleLightForBlock<true>(sv, rq.want, rq.ctx, rq.u0, rq.u, rq.lambda);   // (on the host: SampleLightDirect, or nothing)
    const blight::SampleRow row = blight::SampleFinish(sv, it, pick);
    out[0] = row.ray0; out[1] = row.ray1; out[2] = row.L; out[3] = row.wiPdf;
    *light = row.light;
}
void BodyEmitted(const SceneView &sv, const Rows &r, size_t i, F4 out[2]) {
    const blight::EmittedRow row = blight::EmittedItem<true, true, true>(sv, r.rays.data(), r.planesF.data(), r.planesI.data(), (size_t)r.n, i, r.lambda4.data(), r.infiniteIndex,
                                                                         r.hasPrev ? r.prev.data() : nullptr);
    out[0] = row.Le; out[1] = row.pmfPdf;
}

// ---- --self: fabricated rows ---------------------------------------------------------------------------------------------------------
struct Gen {
    std::mt19937 rng;
    std::uniform_real_distribution<float> uni{0.f, 1.f};
    float lo[3], hi[3];
    explicit Gen(uint32_t seed, const wf_scene_desc &d) : rng(seed) {
        for (int k = 0; k < 3; ++k) { lo[k] = -1; hi[k] = 1; }
        if (d.n_bvh_nodes > 0)
            for (int k = 0; k < 3; ++k) { lo[k] = d.bvh_nodes[0].bmin[k]; hi[k] = d.bvh_nodes[0].bmax[k]; }
        for (int k = 0; k < 3; ++k) { const float e = 0.05f * (hi[k] - lo[k]) + 1e-3f; lo[k] -= e; hi[k] += e; }
    }
    float u() { return uni(rng); }
    V3 point() { return V3{lo[0] + u() * (hi[0] - lo[0]), lo[1] + u() * (hi[1] - lo[1]), lo[2] + u() * (hi[2] - lo[2])}; }
    V3 dir() { return SampleUniformSphere(V2{u(), u()}); }
    F4 lambda() { return check::RotatedWavelengths(u()); }
};

// planes 0 - 4 and the two id planes of a row at p: a small position interval, a normal that is zero on every eighth row
void FillVertex(Gen &g, std::vector<F4> &pf, std::vector<I4> &pi, size_t N, size_t i, V3 p, V3 wo, int valid, int areaLight, bool zeroN) {
    const float e = 1e-5f * (1 + fabsf(p.x) + fabsf(p.y) + fabsf(p.z)) * g.u();
    const V3 n = zeroN ? V3{0, 0, 0} : g.dir();
    V3 ns = n;
    if (!zeroN && g.u() < 0.5f) ns = Normalize(n + 0.2f * g.dir());
    pf[i] = F4{p.x - e, p.y - e, p.z - e, g.u()};
    pf[N + i] = F4{p.x + e, p.y + e, p.z + e, g.u()};
    pf[2 * N + i] = F4{n.x, n.y, n.z, g.u()};
    pf[3 * N + i] = F4{ns.x, ns.y, ns.z, 1.f + g.u()};
    pf[4 * N + i] = F4{wo.x, wo.y, wo.z, 0};
    pi[i] = I4{0, areaLight, (int)(g.u() * 3) - 1, (int)(g.u() * 3) - 1};
    pi[N + i] = I4{0, valid, 0, 0};
}

int Self(const SceneView &sv, const wf_scene_desc &d, int n) {
    const size_t N = (size_t)n;
    long mismatches = 0, usable = 0, chosen = 0, lit = 0, weighted = 0;
    // the sample call
    {
        Gen g(7, d);
        Rows r;
        r.call = 0; r.n = n; r.hasSide = true;
        r.planesF.assign(WF_INTR_FPLANES * N, F4{0, 0, 0, 0}); r.planesI.assign(WF_INTR_IPLANES * N, I4{0, 0, 0, 0});
        r.lambda4.resize(N); r.u4.resize(N); r.side.resize(N);
        for (size_t i = 0; i < N; ++i) {
            const int valid = i % 11 == 5 ? 0 : i % 13 == 7 ? -1 : 1;
            FillVertex(g, r.planesF, r.planesI, N, i, g.point(), g.dir(), valid, -1, i % 8 == 3);
            r.lambda4[i] = g.lambda();
            r.u4[i] = F4{g.u(), g.u(), g.u(), g.u()};
            r.side[i] = (int)(i % 3) - 1;
            if (i % 97 == 0) r.side[i] = 5;   // (read as 0)
        }
        Rows asZero = r;   // what "any other value is read as 0" means for the direct composition
        for (int32_t &s : asZero.side) if (s != 1 && s != -1) s = 0;
        for (size_t i = 0; i < N; ++i) {
            F4 a[4], b[4];
            I4 la, lb;
            DirectSample(sv, asZero, i, a, &la);
            BodySample(sv, r, i, b, &lb);
            if (memcmp(a, b, sizeof a) != 0 || memcmp(&la, &lb, sizeof la) != 0) {
                if (mismatches++ < 5) fprintf(stderr, "sample row %zu: direct light %d pdf %a, bodies light %d pdf %a\n", i, la.x, a[3].w, lb.x, b[3].w);
            }
            chosen += la.x >= 0; usable += a[3].w != 0;
        }
    }
    // the emitted call, for every infinite index, with and without the previous vertex
    std::vector<int> emitters;
    for (int k = 0; k < d.n_lights; ++k) if (d.lights[k].type == WF_LIGHT_DIFFUSE_AREA) emitters.push_back(k);
    const int nIdx = d.n_infinite_lights > 0 ? d.n_infinite_lights : 1;
    for (int idx = 0; idx < nIdx; ++idx)
        for (int withPrev = 0; withPrev < 2; ++withPrev) {
            Gen g(19 + idx, d);
            Rows r;
            r.call = 1; r.n = n; r.infiniteIndex = idx; r.hasPrev = withPrev != 0;
            r.planesF.assign(WF_INTR_FPLANES * N, F4{0, 0, 0, 0}); r.planesI.assign(WF_INTR_IPLANES * N, I4{0, 0, 0, 0});
            r.lambda4.resize(N); r.rays.resize(2 * N); r.prev.assign(5 * N, F4{0, 0, 0, 0});   // (FillVertex writes plane 4 too; the bodies read 0 - 3)
            std::vector<I4> prevI(2 * N);
            for (size_t i = 0; i < N; ++i) {
                int valid = i % 3 == 0 ? 0 : i % 17 == 4 ? -1 : 1;
                V3 p = g.point(), wo = g.dir();
                int area = -1;
                if (valid == 1 && !emitters.empty() && i % 5 != 1) {
                    area = emitters[(size_t)(g.u() * emitters.size()) % emitters.size()];
                    const int tri = d.lights[area].tri;
                    if (tri < d.n_triangles) {   // a point of the emitter's triangle
                        float b0 = g.u(), b1 = g.u();
                        if (b0 + b1 > 1) { b0 = 1 - b0; b1 = 1 - b1; }
                        const int32_t *v = &d.tri_indices[3 * (size_t)tri];
                        const float *p0 = &d.P[3 * (size_t)v[0]], *p1 = &d.P[3 * (size_t)v[1]], *p2 = &d.P[3 * (size_t)v[2]];
                        const float b2 = 1 - b0 - b1;
                        p = V3{b0 * p0[0] + b1 * p1[0] + b2 * p2[0], b0 * p0[1] + b1 * p1[1] + b2 * p2[1], b0 * p0[2] + b1 * p1[2] + b2 * p2[2]};
                    }
                }
                FillVertex(g, r.planesF, r.planesI, N, i, p, wo, valid, area, false);
                if (area >= 0 && d.lights[area].tri < d.n_triangles && i % 2 == 0) {
                    // the geometric normal on the side of wo, as a hit seen from there has it (a one-sided emitter then emits)
                    const int32_t *v = &d.tri_indices[3 * (size_t)d.lights[area].tri];
                    const float *p0 = &d.P[3 * (size_t)v[0]], *p1 = &d.P[3 * (size_t)v[1]], *p2 = &d.P[3 * (size_t)v[2]];
                    V3 n = Cross(V3{p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, V3{p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]});
                    if (LengthSquared(n) > 0) {
                        n = Normalize(n);
                        if (Dot(n, wo) < 0) n = -n;
                        r.planesF[2 * N + i].x = n.x; r.planesF[2 * N + i].y = n.y; r.planesF[2 * N + i].z = n.z;
                    }
                }
                r.lambda4[i] = g.lambda();
                // the ray that ends at the row: from the previous vertex, which lies along wo
                const float t = 0.05f + g.u() * (g.hi[0] - g.lo[0]);
                const V3 o = valid == 1 ? p + wo * t : g.point(), dd = valid == 1 ? -wo * (0.5f + g.u()) : g.dir() * (0.5f + g.u());
                r.rays[2 * i] = F4{o.x, o.y, o.z, dd.x};
                r.rays[2 * i + 1] = F4{dd.y, dd.z, WF_INFINITY, g.u()};
                FillVertex(g, r.prev, prevI, N, i, o, g.dir(), 1, -1, i % 8 == 3);
            }
            for (size_t i = 0; i < N; ++i) {
                F4 a[2], b[2];
                DirectEmitted(sv, r, i, a);
                BodyEmitted(sv, r, i, b);
                if (memcmp(a, b, sizeof a) != 0) {
                    if (mismatches++ < 5) fprintf(stderr, "emitted row %zu (index %d, prev %d): direct Le %a pdf %a, bodies Le %a pdf %a\n", i, idx, withPrev, a[0].x, a[1].y, b[0].x, b[1].y);
                }
                lit += (a[0].x != 0 || a[0].y != 0 || a[0].z != 0 || a[0].w != 0); weighted += a[1].y != 0;
            }
        }
    printf("{\"rows\": %d, \"mismatches\": %ld, \"lights_chosen\": %ld, \"usable\": %ld, \"emitting\": %ld, \"with_pdf\": %ld, \"lights\": %d, \"infinite_lights\": %d}\n", n,
           mismatches, chosen, usable, lit, weighted, d.n_lights, d.n_infinite_lights);
    return mismatches == 0 ? 0 : 1;
}

// ---- --eval -------------------------------------------------------------------------------------------------------------------------
using check::ReadVec;
int Eval(const SceneView &sv, const char *inPath, const char *outPath) {
    FILE *f = fopen(inPath, "rb");
    if (!f) { perror(inPath); return 1; }
    int32_t h[8];
    if (fread(h, 4, 8, f) != 8 || h[0] != MAGIC || h[1] < 0 || h[1] > 1 || h[2] < 0 || h[2] > (1 << 24)) { fprintf(stderr, "%s: not an input file of this program\n", inPath); fclose(f); return 1; }
    Rows r;
    r.call = h[1]; r.n = h[2]; r.infiniteIndex = h[3]; r.hasSide = h[4] != 0; r.hasPrev = h[5] != 0;
    const size_t N = (size_t)r.n;
    bool ok = ReadVec(f, r.planesF, WF_INTR_FPLANES * N) && ReadVec(f, r.planesI, WF_INTR_IPLANES * N) && ReadVec(f, r.lambda4, N);
    if (r.call == 0) ok = ok && ReadVec(f, r.u4, N) && ReadVec(f, r.side, r.hasSide ? N : 0);
    else ok = ok && ReadVec(f, r.rays, 2 * N) && ReadVec(f, r.prev, r.hasPrev ? 4 * N : 0);
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short file\n", inPath); return 1; }
    if (r.call == 1 && (r.infiniteIndex < 0 || r.infiniteIndex >= (sv.nInfiniteLights > 0 ? sv.nInfiniteLights : 1))) { fprintf(stderr, "infinite_index %d out of range\n", r.infiniteIndex); return 1; }
    if (r.hasSide) for (int32_t &s : r.side) if (s != 1 && s != -1) s = 0;
    FILE *g = fopen(outPath, "wb");
    if (!g) { perror(outPath); return 1; }
    if (r.call == 0) {
        std::vector<F4> rays(2 * N), L(N), wiPdf(N);
        std::vector<I4> light(N);
        for (size_t i = 0; i < N; ++i) {
            F4 o[4];
            DirectSample(sv, r, i, o, &light[i]);
            rays[2 * i] = o[0]; rays[2 * i + 1] = o[1]; L[i] = o[2]; wiPdf[i] = o[3];
        }
        fwrite(rays.data(), 16, 2 * N, g); fwrite(L.data(), 16, N, g); fwrite(wiPdf.data(), 16, N, g); fwrite(light.data(), 16, N, g);
    } else {
        std::vector<F4> Le(N), pp(N);
        for (size_t i = 0; i < N; ++i) {
            F4 o[2];
            DirectEmitted(sv, r, i, o);
            Le[i] = o[0]; pp[i] = o[1];
        }
        fwrite(Le.data(), 16, N, g); fwrite(pp.data(), 16, N, g);
    }
    if (fclose(g) != 0) { perror(outPath); return 1; }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    std::string dataDir, mode, scene;
    std::vector<std::string> rest;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--datadir" && i + 1 < argc) dataDir = argv[++i];
        else if ((a == "--self" || a == "--eval") && mode.empty()) mode = a;
        else if (!mode.empty() && scene.empty()) scene = a;
        else rest.push_back(a);
    }
    if (scene.empty() || (mode == "--self" && rest.size() != 1) || (mode == "--eval" && rest.size() != 2)) {
        fprintf(stderr, "usage: light_sample_check [--datadir <dir>] --self scene.pbrt N | --eval scene.pbrt in.bin out.bin\n");
        return 2;
    }
    return check::Guarded(scene, [&] {
        check::InitData(dataDir, argv[0], "/../data");   // (the binary's usual location: pbrt-v4_amd/_build/light_sample_check)
        RenderOptions opt = check::QuietOptions();
        const check::HostScene hs(scene, &opt);
        const int rc = mode == "--self" ? Self(hs.sv, hs.T.desc, atoi(rest[0].c_str())) : Eval(hs.sv, rest[0].c_str(), rest[1].c_str());
        if (hs.fatalWord != 0) { fprintf(stderr, "a light function raised the scene's fatal word (%d)\n", hs.fatalWord); return 1; }
        return rc;
    });
}
