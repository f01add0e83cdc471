// tools/bsdf_check.cpp — the per-row bodies of wf_bsdf_make_device / wf_bsdf_eval_device (pbrt-v4_amd/csrc/hip/wf_boundary_bsdf.h)
// compiled for the host, and the render's own material functions composed directly (ResolveMix, the footprint / normal-map / bump-map
// lines of MatShade, MatBxDF<T>::Get, Regularize, BSDF<T>::f / PDF / Sample_f: csrc/common/wf_kernels.h, wf_bxdf.h) on a scene file's
// tables.  The direct side keeps every BxDF as the struct the render holds — it never goes through a record.  Stand-alone: the parser
// and BuildSceneTables, no device, neither library.
//
//   bsdf_check [--datadir DIR] [--spp S] --self SCENE N
//       N rows from the scene's own first hits (rays from the camera's position through the scene's bounds, walked by the
//       reference-order BVH walk, their interactions by HitInteraction), with misses and invalid rows between them, seeded wavelengths,
//       directions and sample values, every other row regularised — through the new bodies and through the direct composition; every
//       output word must be equal.  Prints one JSON line with counters per material type and per outcome; exits non-zero on a mismatch.
//   bsdf_check [--datadir DIR] [--spp S] --eval SCENE in.bin out.bin
//       the DIRECT COMPOSITION's outputs for the rows of in.bin (not the new header's bodies): the expected values of the GPU tests.
//       in.bin   int32 {magic 0x42534431, n, has_regularize, has_wi, has_u, 0, 0, 0}
//                rays8 [n][8] f32, planes_f [11][n][4] f32, planes_i [2][n][4] i32, lambda4 [n][4],
//                regularize [n] i32 if has_regularize, wi4 [n][4] if has_wi, u4 [n][4] if has_u
//       out.bin  bsdf_rec [10][n][4], bsdf4 [n][4] i32, then f4 [n][4], pdf4 [n][4] if has_wi, then next_rays8 [n][8], sample_f4 [n][4],
//                sample_pdf4 [n][4], sample_i4 [n][4] i32 if has_u
//   --spp S: the pixel samples, in place of the scene file's (as a renderer opened with that many has them: the texture footprint of
//   Approximate_dp_dxy scales with 1 / sqrt(spp))
// Built with -fsanitize=address,undefined it is how that code is run under the sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../pbrt-v4_amd/csrc/hip/wf_boundary_bsdf.h"
#include "check_common.h"

using namespace wf;

namespace {

constexpr int32_t MAGIC = 0x42534431;

struct Rows {
    int n = 0;
    bool hasReg = false, hasWi = false, hasU = false;
    std::vector<F4> rays, planesF, lambda4, wi4, u4;
    std::vector<I4> planesI;
    std::vector<int32_t> reg;
    // --self only: the hit each row came from (prim < 0: none), for the render's own ResolveMix
    std::vector<int> prim, inst;
    std::vector<F4> bary;
};
struct Outs {
    std::vector<F4> rec, f4, pdf4, next, sf, spdf;
    std::vector<I4> bsdf4, si;
    void Size(size_t N) {
        rec.assign(WF_BSDF_PLANES * N, F4{0, 0, 0, 0}); f4.assign(N, F4{0, 0, 0, 0}); pdf4 = f4; sf = f4; spdf = f4; next.assign(2 * N, F4{0, 0, 0, 0});
        bsdf4.assign(N, I4{0, 0, 0, 0}); si = bsdf4;
    }
};

// ---- the direct composition: the render's functions, called as MatShade / MatNeeFinish call them ------------------------------------
struct Vertex {   // the SurfaceInteraction of a row, from its planes
    SurfIntr si{};
    V3 wo{0, 0, 0};
    float time = 0;
    int material = -1, medIn = -1, medOut = -1;
};
Vertex LoadVertex(const Rows &r, size_t i) {
    const size_t N = (size_t)r.n;
    auto P = [&](int p) { return r.planesF[p * N + i]; };
    auto v3 = [](F4 q) { return V3{q.x, q.y, q.z}; };
    auto n3 = [](F4 q) { return N3{q.x, q.y, q.z}; };
    Vertex v;
    v.si.pi = P3i{v3(P(0)), v3(P(1))};
    v.si.uv = V2{P(0).w, P(1).w};
    v.si.n = n3(P(2)); v.time = P(2).w;
    v.si.ns = n3(P(3));
    v.wo = v3(P(4));
    v.si.dpdu = v3(P(5)); v.si.dpdv = v3(P(6)); v.si.dpdus = v3(P(7)); v.si.dpdvs = v3(P(8));
    v.si.dndus = n3(P(9)); v.si.dndvs = n3(P(10));
    const I4 ids = r.planesI[i];
    v.material = ids.x; v.medIn = ids.z; v.medOut = ids.w;
    return v;
}
// MixMaterial::ChooseMaterial until the material is no mix (intersect.h:92-97, materials.h:284-294)
int DirectResolveMix(const SceneView &sv, int matId, const TexCtx &tc, V3 wo) {
    while (sv.materials[matId].type == WF_MAT_MIX) {
        const wf_material &m = sv.materials[matId];
        const float amt = EvalFloatTexture(sv, m.tex[WF_MT_AMOUNT], tc);
        int pick;
        if (amt <= 0) pick = 0;
        else if (amt >= 1) pick = 1;
        else {
            uint32_t w[8] = {FloatToBits(tc.p.x), FloatToBits(tc.p.y), FloatToBits(tc.p.z), FloatToBits(wo.x), FloatToBits(wo.y), FloatToBits(wo.z),
                             (uint32_t)m.mix[0], (uint32_t)m.mix[1]};
            pick = amt < HashToFloat(HashWords(w, 8)) ? 0 : 1;
        }
        matId = m.mix[pick];
    }
    return matId;
}
// what the direct side keeps of a row's BSDF: the struct itself
template <int MAT>
struct DirectBsdf {
    typename MatBxDF<MAT>::T bxdf{};
    N3 ns{0, 0, 0};
    V3 dpdus{0, 0, 0};
    bool terminated = false;
};
// surfscatter.cpp:73-145 as MatShade restates it (wf_kernels.h), on the vertex
template <int MAT>
DirectBsdf<MAT> DirectMake(const SceneView &sv, const Vertex &v, int matId, F4 lam, bool regularize) {
    const SurfIntr &si = v.si;
    const wf_material &mat = sv.materials[matId];
    TexCtx tc;
    tc.p = si.pi.mid(); tc.n = si.n; tc.uv = si.uv;
    if (!sv.options.disable_texture_filtering) {
        ApproximateDpDxy<true>(sv, tc.p, si.n, &tc.dpdx, &tc.dpdy, v.time);
        V3 dpdu = si.dpdu, dpdv = si.dpdv;
        float ata00 = Dot(dpdu, dpdu), ata01 = Dot(dpdu, dpdv), ata11 = Dot(dpdv, dpdv);
        float invDet = 1 / DifferenceOfProducts(ata00, ata11, ata01, ata01);
        invDet = IsFinite(invDet) ? invDet : 0.f;
        float atb0x = Dot(dpdu, tc.dpdx), atb1x = Dot(dpdv, tc.dpdx);
        float atb0y = Dot(dpdu, tc.dpdy), atb1y = Dot(dpdv, tc.dpdy);
        float dudx = DifferenceOfProducts(ata11, atb0x, ata01, atb1x) * invDet;
        float dvdx = DifferenceOfProducts(ata00, atb1x, ata01, atb0x) * invDet;
        float dudy = DifferenceOfProducts(ata11, atb0y, ata01, atb1y) * invDet;
        float dvdy = DifferenceOfProducts(ata00, atb1y, ata01, atb0y) * invDet;
        tc.dudx = IsFinite(dudx) ? Clamp(dudx, -1e8f, 1e8f) : 0.f;
        tc.dvdx = IsFinite(dvdx) ? Clamp(dvdx, -1e8f, 1e8f) : 0.f;
        tc.dudy = IsFinite(dudy) ? Clamp(dudy, -1e8f, 1e8f) : 0.f;
        tc.dvdy = IsFinite(dvdy) ? Clamp(dvdy, -1e8f, 1e8f) : 0.f;
        tc.dpdx = tc.dpdy = V3{0, 0, 0};
    }
    DirectBsdf<MAT> b;
    b.ns = si.ns; b.dpdus = si.dpdus;
    if (mat.normalmap >= 0) {
        V3 nm;
        NormalMapTexelP(sv.tableData, sv.texImages + mat.normalmap, tc.uv.x, tc.uv.y, &nm.x, &nm.y, &nm.z);
        nm = Normalize(nm);
        Frame frame = Frame::FromXZ(Normalize(si.dpdus), toV(si.ns));
        nm = frame.FromLocal(nm);
        float ulen = Length(si.dpdus), vlen = Length(si.dpdvs);
        b.dpdus = Normalize(GramSchmidt(si.dpdus, nm)) * ulen;
        V3 dpdvs = Normalize(Cross(nm, b.dpdus)) * vlen;
        b.ns = toN(Normalize(Cross(b.dpdus, dpdvs)));
        b.ns = FaceForward(b.ns, si.n);
    } else if (mat.displacement >= 0) {
        TexCtx bc = tc;
        bc.n = N3{0, 0, 0};
        TexCtx sh = bc;
        float du = .5f * (wf::abs(tc.dudx) + wf::abs(tc.dudy));
        if (du == 0) du = .0005f;
        sh.p = tc.p + du * si.dpdus;
        sh.uv = V2{tc.uv.x + du, tc.uv.y + 0.f};
        float uDisplace = EvalFloatTexture(sv, mat.displacement, sh);
        float dv = .5f * (wf::abs(tc.dvdx) + wf::abs(tc.dvdy));
        if (dv == 0) dv = .0005f;
        sh.p = tc.p + dv * si.dpdvs;
        sh.uv = V2{tc.uv.x + 0.f, tc.uv.y + dv};
        float vDisplace = EvalFloatTexture(sv, mat.displacement, sh);
        float displace = EvalFloatTexture(sv, mat.displacement, bc);
        b.dpdus = si.dpdus + (uDisplace - displace) / du * toV(si.ns) + displace * toV(si.dndus);
        V3 dpdvs = si.dpdvs + (vDisplace - displace) / dv * toV(si.ns) + displace * toV(si.dndvs);
        b.ns = toN(Normalize(Cross(b.dpdus, dpdvs)));
        b.ns = FaceForward(b.ns, si.n);
    }
    Wavelengths lambda;
    lambda.lambda[0] = lam.x; lambda.lambda[1] = lam.y; lambda.lambda[2] = lam.z; lambda.lambda[3] = lam.w;
    for (int k = 0; k < 4; ++k) lambda.pdf[k] = 1;
    b.bxdf = MatBxDF<MAT>::Get(sv, mat, lambda, tc);
    b.terminated = lambda.SecondaryTerminated();
    if (regularize) { BSDF<typename MatBxDF<MAT>::T> bsdf(b.ns, b.dpdus, b.bxdf); bsdf.Regularize(); b.bxdf = bsdf.bxdf; }
    return b;
}
struct Counters {
    long rows = 0, mismatches = 0, zeroRows = 0, typeRows[WF_MAT_NTYPES] = {}, validSamples = 0, transmitted = 0, specular = 0, proportional = 0, fNonzero = 0,
         mixRows = 0, mixChild[2] = {0, 0}, mixAgainstRender = 0, terminated = 0, regularized = 0, regularizedDiffer = 0;
};
template <int MAT>
void DirectRow(const SceneView &sv, const Rows &r, size_t i, const Vertex &v, int matId, Outs *o, Counters *c) {
    using BxDF = typename MatBxDF<MAT>::T;
    const size_t N = (size_t)r.n;
    const bool reg = r.hasReg && r.reg[i] != 0;
    const DirectBsdf<MAT> b = DirectMake<MAT>(sv, v, matId, r.lambda4[i], reg);
    const BSDF<BxDF> bsdf(b.ns, b.dpdus, b.bxdf);
    const int flags = bsdf.Flags();
    int side = 0;
    if (IsNonSpecular(flags)) side = (IsReflective(flags) && !IsTransmissive(flags)) ? 1 : (IsReflective(flags) && IsTransmissive(flags)) ? -1 : 0;
    o->bsdf4[i] = I4{flags | (b.terminated ? 256 : 0), side, matId, MAT};
    // the record the GPU tests expect: the documented header and frame, the BxDF's numbers in the header's order
    float w[bbsdf::BX_WORDS] = {};
    bbsdf::Pack(w, b.bxdf);
    o->rec[i] = bbsdf::IntsAsF4(MAT, flags, matId, 0);
    o->rec[N + i] = F4{b.ns.x, b.ns.y, b.ns.z, 0};
    o->rec[2 * N + i] = F4{b.dpdus.x, b.dpdus.y, b.dpdus.z, 0};
    for (int p = 0; p < bbsdf::BX_PLANES; ++p) o->rec[(3 + p) * N + i] = F4{w[4 * p], w[4 * p + 1], w[4 * p + 2], w[4 * p + 3]};
    if (c) {
        ++c->typeRows[MAT];
        c->terminated += b.terminated;
        if (reg) {
            ++c->regularized;
            const DirectBsdf<MAT> plain = DirectMake<MAT>(sv, v, matId, r.lambda4[i], false);
            float w0[bbsdf::BX_WORDS] = {};
            bbsdf::Pack(w0, plain.bxdf);
            c->regularizedDiffer += memcmp(w, w0, sizeof w) != 0;
        }
    }
    if (r.hasWi) {
        const V3 wi{r.wi4[i].x, r.wi4[i].y, r.wi4[i].z};
        const S4 f = bsdf.f(v.wo, wi);   // MatNeeFinish
        o->f4[i] = toF4(f);
        o->pdf4[i] = F4{bsdf.PDF(v.wo, wi), AbsDot(wi, b.ns), 0, 0};
        if (c && f) ++c->fNonzero;
    }
    if (r.hasU) {
        const BSDFSample bs = bsdf.Sample_f(v.wo, r.u4[i].x, V2{r.u4[i].y, r.u4[i].z});   // MatShade
        if (bs.valid) {
            const V3 wi = bs.wi;
            const float pdfMis = bs.pdfIsProportional ? bsdf.PDF(v.wo, bs.wi) : bs.pdf;
            const V3 ro = OffsetRayOrigin(v.si.pi, v.si.n, wi);
            const int medium = sv.haveMedia ? (Dot(wi, v.si.n) > 0 ? v.medOut : v.medIn) : -1;
            o->sf[i] = toF4(bs.f);
            o->spdf[i] = F4{bs.pdf, pdfMis, AbsDot(wi, b.ns), bs.eta};
            o->si[i] = I4{1, bs.flags, medium, bs.pdfIsProportional ? 1 : 0};
            o->next[2 * i] = F4{ro.x, ro.y, ro.z, wi.x};
            o->next[2 * i + 1] = F4{wi.y, wi.z, WF_INFINITY, v.time};
            if (c) { ++c->validSamples; c->transmitted += bs.IsTransmission(); c->specular += bs.IsSpecularS(); c->proportional += bs.pdfIsProportional; }
        }
    }
}
void Direct(const SceneView &sv, int nMaterials, const Rows &r, size_t i, Outs *o, Counters *c) {
    const size_t N = (size_t)r.n;
    if (c) ++c->rows;
    // (the outputs start as zeros: a row without a BSDF stays that way)
    if (r.planesI[N + i].y != 1) { if (c) ++c->zeroRows; return; }
    const Vertex v = LoadVertex(r, i);
    int matId = v.material;
    if (matId < 0 || matId >= nMaterials) { if (c) ++c->zeroRows; return; }
    if (sv.materials[matId].type == WF_MAT_MIX) {
        const wf_material &top = sv.materials[matId];
        TexCtx tc;
        tc.p = v.si.pi.mid(); tc.n = v.si.n; tc.uv = v.si.uv;
        const V3 wo{-r.rays[2 * i].w, -r.rays[2 * i + 1].x, -r.rays[2 * i + 1].y};
        const int resolved = DirectResolveMix(sv, matId, tc, wo);
        if (c) {
            ++c->mixRows;
            ++c->mixChild[resolved == top.mix[0] ? 0 : 1];   // (a nested mix counts under its second child)
            // ... and the render's own resolve, from the hit the row came from
            if (!r.prim.empty() && r.prim[i] >= 0) {
                const F4 r0 = r.rays[2 * i], r1 = r.rays[2 * i + 1], b = r.bary[i];
                const int m = ResolveMix<true>(sv, matId, r.prim[i], r.inst[i], b.x, b.y, b.z, wo, V3{r0.x, r0.y, r0.z}, r1.w);
                if (m != resolved) { ++c->mismatches; fprintf(stderr, "row %zu: ResolveMix gives material %d, the planes' resolve %d\n", i, m, resolved); }
                ++c->mixAgainstRender;
            }
        }
        matId = resolved;
    }
    switch (sv.materials[matId].type) {
#define CASE(T) case T: DirectRow<T>(sv, r, i, v, matId, o, c); break;
        CASE(WF_MAT_DIFFUSE) CASE(WF_MAT_CONDUCTOR) CASE(WF_MAT_DIELECTRIC) CASE(WF_MAT_THIN_DIELECTRIC) CASE(WF_MAT_DIFFUSE_TRANSMISSION)
        CASE(WF_MAT_COATED_DIFFUSE) CASE(WF_MAT_COATED_CONDUCTOR) CASE(WF_MAT_SUBSURFACE) CASE(WF_MAT_HAIR) CASE(WF_MAT_MEASURED)
#undef CASE
    default: if (c) ++c->zeroRows; break;
    }
}

// ---- the new bodies, as the kernels run them: the routing pass, every type's make pass, the zero pass and every type's eval pass ----
template <int MAT>
void BodyMakeType(const SceneView &sv, const Rows &r, const std::vector<int32_t> &route, Outs *o) {
    const size_t N = (size_t)r.n;
    for (size_t i = 0; i < N; ++i) {
        const int matId = route[i];
        if (matId < 0 || sv.materials[matId].type != MAT) continue;
        bbsdf::MakeRowOut out;
        bbsdf::MakeRow<MAT, true>(sv, matId, r.planesF.data(), N, i, r.lambda4[i], r.hasReg && r.reg[i] != 0, &out);
        for (int p = 0; p < WF_BSDF_PLANES; ++p) o->rec[p * N + i] = out.rec[p];
        o->bsdf4[i] = out.bsdf4;
    }
}
template <int MAT>
void BodyEvalType(const SceneView &sv, int nMaterials, const Rows &r, Outs *o) {
    const size_t N = (size_t)r.n;
    for (size_t i = 0; i < N; ++i) {
        int matId;
        if (bbsdf::RecordType(sv, nMaterials, o->rec[i], &matId) != MAT) continue;
        bbsdf::EvalRowOut out;
        bbsdf::EvalRow<MAT>(sv, matId, o->rec.data(), r.planesF.data(), r.planesI.data(), N, i, r.hasWi ? r.wi4.data() : nullptr, r.hasU ? r.u4.data() : nullptr, &out);
        if (r.hasWi) { o->f4[i] = out.f; o->pdf4[i] = out.pdf; }
        if (r.hasU) { o->next[2 * i] = out.ray0; o->next[2 * i + 1] = out.ray1; o->sf[i] = out.sf; o->spdf[i] = out.spdf; o->si[i] = out.si; }
    }
}
void Bodies(const SceneView &sv, int nMaterials, const Rows &r, Outs *o) {
    const size_t N = (size_t)r.n;
    // (every output starts as a sentinel, so that a row no pass writes shows)
    const F4 sf{BitsToFloat(0x7fc12345u), -1.f, 2.f, 3.f};
    const I4 sI{-77, -77, -77, -77};
    o->rec.assign(WF_BSDF_PLANES * N, sf); o->f4.assign(N, sf); o->pdf4 = o->f4; o->sf = o->f4; o->spdf = o->f4; o->next.assign(2 * N, sf);
    o->bsdf4.assign(N, sI); o->si = o->bsdf4;
    std::vector<int32_t> route(N, -2);
    for (size_t i = 0; i < N; ++i) {
        route[i] = bbsdf::RouteRow(sv, nMaterials, r.rays.data(), r.planesF.data(), r.planesI.data(), N, i);
        if (route[i] < 0) { for (int p = 0; p < WF_BSDF_PLANES; ++p) o->rec[p * N + i] = F4{0, 0, 0, 0}; o->bsdf4[i] = I4{0, 0, 0, 0}; }
    }
#define EACH(F) F(WF_MAT_DIFFUSE) F(WF_MAT_CONDUCTOR) F(WF_MAT_DIELECTRIC) F(WF_MAT_THIN_DIELECTRIC) F(WF_MAT_DIFFUSE_TRANSMISSION) \
                F(WF_MAT_COATED_DIFFUSE) F(WF_MAT_COATED_CONDUCTOR) F(WF_MAT_SUBSURFACE) F(WF_MAT_HAIR) F(WF_MAT_MEASURED)
#define MAKE(T) BodyMakeType<T>(sv, r, route, o);
    EACH(MAKE)
#undef MAKE
    for (size_t i = 0; i < N; ++i) {
        int matId;
        if (bbsdf::RecordType(sv, nMaterials, o->rec[i], &matId) != 0) continue;
        const F4 z{0, 0, 0, 0};
        o->f4[i] = o->pdf4[i] = o->sf[i] = o->spdf[i] = o->next[2 * i] = o->next[2 * i + 1] = z;
        o->si[i] = I4{0, 0, 0, 0};
    }
#define EVAL(T) BodyEvalType<T>(sv, nMaterials, r, o);
    EACH(EVAL)
#undef EVAL
#undef EACH
}

// ---- --self: rows from the scene's own first hits ------------------------------------------------------------------------------------
int Self(const SceneView &sv, const wf_scene_desc &d, int n) {
    const size_t N = (size_t)n;
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> uni(0.f, 1.f);
    auto u = [&] { return uni(rng); };
    float lo[3] = {-1, -1, -1}, hi[3] = {1, 1, 1};
    if (d.n_bvh_nodes > 0) for (int k = 0; k < 3; ++k) { lo[k] = d.bvh_nodes[0].bmin[k]; hi[k] = d.bvh_nodes[0].bmax[k]; }
    const V3 eye{d.camera.renderFromCamera.m[0][3], d.camera.renderFromCamera.m[1][3], d.camera.renderFromCamera.m[2][3]};
    Rows r;
    r.n = n; r.hasReg = r.hasWi = r.hasU = true;
    r.rays.assign(2 * N, F4{0, 0, 0, 0}); r.planesF.assign(WF_INTR_FPLANES * N, F4{0, 0, 0, 0}); r.planesI.assign(WF_INTR_IPLANES * N, I4{-1, -1, -1, -1});
    r.lambda4.resize(N); r.wi4.resize(N); r.u4.resize(N); r.reg.resize(N); r.prim.assign(N, -1); r.inst.assign(N, -1); r.bary.assign(N, F4{0, 0, 0, 0});
    long hits = 0;
    for (size_t i = 0; i < N; ++i) {
        const V3 target{lo[0] + u() * (hi[0] - lo[0]), lo[1] + u() * (hi[1] - lo[1]), lo[2] + u() * (hi[2] - lo[2])};
        V3 dir = target - eye;
        if (LengthSquared(dir) == 0) dir = V3{0, 0, 1};
        dir = Normalize(dir) * (0.5f + u());   // (not normalised: the mix hash takes the ray's own -d)
        const float time = u();
        r.rays[2 * i] = F4{eye.x, eye.y, eye.z, dir.x};
        r.rays[2 * i + 1] = F4{dir.y, dir.z, WF_INFINITY, time};
        r.lambda4[i] = check::RotatedWavelengths(u());
        r.u4[i] = F4{u(), u(), u(), u()};
        r.reg[i] = (int32_t)(i & 1);
        ArrayStack st;
        ClosestHit ch;
        const bool found = i % 19 != 7 && BVHIntersectClosest<true>(sv, eye, dir, WF_INFINITY, st, &ch, time);   // (every 19th row: a miss whatever the scene says)
        r.planesI[N + i] = I4{-1, found ? 1 : 0, 0, 0};
        V3 n{0, 0, 1}, wo = Normalize(-dir);
        if (found) {
            ++hits;
            SurfIntr si;
            HitInteraction<true, true, true>(sv, ch.prim, ch.inst, ch.h.b0, ch.h.b1, ch.h.b2, &si, eye, dir, time);
            wo = IntrWo<true, true>(sv, ch.prim, ch.inst, -dir, time);
            const wf_mesh &mesh = sv.meshes[si.mesh];
            auto f3 = [](V3 q, float w) { return F4{q.x, q.y, q.z, w}; };
            r.planesF[i] = f3(si.pi.lo, si.uv.x); r.planesF[N + i] = f3(si.pi.hi, si.uv.y);
            r.planesF[2 * N + i] = F4{si.n.x, si.n.y, si.n.z, time}; r.planesF[3 * N + i] = F4{si.ns.x, si.ns.y, si.ns.z, ch.h.t};
            r.planesF[4 * N + i] = f3(wo, 0); r.planesF[5 * N + i] = f3(si.dpdu, 0); r.planesF[6 * N + i] = f3(si.dpdv, 0);
            r.planesF[7 * N + i] = f3(si.dpdus, 0); r.planesF[8 * N + i] = f3(si.dpdvs, 0);
            r.planesF[9 * N + i] = F4{si.dndus.x, si.dndus.y, si.dndus.z, 0}; r.planesF[10 * N + i] = F4{si.dndvs.x, si.dndvs.y, si.dndvs.z, 0};
            r.planesI[i] = I4{mesh.material, -1, mesh.medium_inside, mesh.medium_outside};
            r.planesI[N + i] = I4{si.mesh, 1, mesh.flags, 0};
            r.prim[i] = ch.prim; r.inst[i] = ch.inst; r.bary[i] = F4{ch.h.b0, ch.h.b1, ch.h.b2, 0};
            n = toV(si.n);
            // between the hits: a record the interaction kernel calls invalid, an interface surface, a material id past the table
            if (i % 23 == 3) r.planesI[N + i].y = -1;
            else if (i % 29 == 5) r.planesI[i].x = -1;
            else if (i % 31 == 6) r.planesI[i].x = d.n_materials + (int)(i % 7);
        }
        // wi: any direction, or one in the hemisphere of wo / against it (so that f is not black for want of a hemisphere)
        V3 wi = SampleUniformSphere(V2{u(), u()});
        if (i % 3 == 1) { if (Dot(wi, n) * Dot(wo, n) < 0) wi = -wi; }
        else if (i % 3 == 2) { if (Dot(wi, n) * Dot(wo, n) > 0) wi = -wi; }
        r.wi4[i] = F4{wi.x, wi.y, wi.z, u()};
    }
    Outs a, b;
    a.Size(N);
    Counters c;
    for (size_t i = 0; i < N; ++i) Direct(sv, d.n_materials, r, i, &a, &c);
    Bodies(sv, d.n_materials, r, &b);
    auto differ = [&](size_t i) {
        for (int p = 0; p < WF_BSDF_PLANES; ++p) if (memcmp(&a.rec[p * N + i], &b.rec[p * N + i], 16) != 0) return "bsdf_rec";
        if (memcmp(&a.bsdf4[i], &b.bsdf4[i], 16) != 0) return "bsdf4";
        if (memcmp(&a.f4[i], &b.f4[i], 16) != 0) return "f4";
        if (memcmp(&a.pdf4[i], &b.pdf4[i], 16) != 0) return "pdf4";
        if (memcmp(&a.next[2 * i], &b.next[2 * i], 32) != 0) return "next_rays8";
        if (memcmp(&a.sf[i], &b.sf[i], 16) != 0) return "sample_f4";
        if (memcmp(&a.spdf[i], &b.spdf[i], 16) != 0) return "sample_pdf4";
        if (memcmp(&a.si[i], &b.si[i], 16) != 0) return "sample_i4";
        return (const char *)nullptr;
    };
    for (size_t i = 0; i < N; ++i)
        if (const char *what = differ(i)) {
            if (c.mismatches++ < 8) fprintf(stderr, "row %zu (type %d): %s differs — direct f %a pdf %a sample pdf %a, bodies f %a pdf %a sample pdf %a\n", i, a.bsdf4[i].w, what,
                                            a.f4[i].x, a.pdf4[i].x, a.spdf[i].x, b.f4[i].x, b.pdf4[i].x, b.spdf[i].x);
        }
    printf("{\"rows\": %ld, \"mismatches\": %ld, \"hits\": %ld, \"zero_rows\": %ld, \"type_rows\": [", c.rows, c.mismatches, hits, c.zeroRows);
    for (int t = 0; t < WF_MAT_NTYPES; ++t) printf("%s%ld", t ? ", " : "", c.typeRows[t]);
    printf("], \"valid_samples\": %ld, \"transmitted\": %ld, \"specular\": %ld, \"proportional\": %ld, \"f_nonzero\": %ld, \"mix_rows\": %ld, \"mix_child\": [%ld, %ld], "
           "\"mix_against_render\": %ld, \"terminated\": %ld, \"regularized\": %ld, \"regularized_differ\": %ld}\n",
           c.validSamples, c.transmitted, c.specular, c.proportional, c.fNonzero, c.mixRows, c.mixChild[0], c.mixChild[1], c.mixAgainstRender, c.terminated, c.regularized,
           c.regularizedDiffer);
    return c.mismatches == 0 ? 0 : 1;
}

// ---- --eval -------------------------------------------------------------------------------------------------------------------------
using check::ReadVec;
int Eval(const SceneView &sv, int nMaterials, const char *inPath, const char *outPath) {
    FILE *f = fopen(inPath, "rb");
    if (!f) { perror(inPath); return 1; }
    int32_t h[8];
    if (fread(h, 4, 8, f) != 8 || h[0] != MAGIC || h[1] < 0 || h[1] > (1 << 24)) { fprintf(stderr, "%s: not an input file of this program\n", inPath); fclose(f); return 1; }
    Rows r;
    r.n = h[1]; r.hasReg = h[2] != 0; r.hasWi = h[3] != 0; r.hasU = h[4] != 0;
    const size_t N = (size_t)r.n;
    const bool ok = ReadVec(f, r.rays, 2 * N) && ReadVec(f, r.planesF, WF_INTR_FPLANES * N) && ReadVec(f, r.planesI, WF_INTR_IPLANES * N) && ReadVec(f, r.lambda4, N) &&
                    ReadVec(f, r.reg, r.hasReg ? N : 0) && ReadVec(f, r.wi4, r.hasWi ? N : 0) && ReadVec(f, r.u4, r.hasU ? N : 0);
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short file\n", inPath); return 1; }
    Outs o;
    o.Size(N);
    for (size_t i = 0; i < N; ++i) Direct(sv, nMaterials, r, i, &o, nullptr);
    FILE *g = fopen(outPath, "wb");
    if (!g) { perror(outPath); return 1; }
    fwrite(o.rec.data(), 16, o.rec.size(), g); fwrite(o.bsdf4.data(), 16, N, g);
    if (r.hasWi) { fwrite(o.f4.data(), 16, N, g); fwrite(o.pdf4.data(), 16, N, g); }
    if (r.hasU) { fwrite(o.next.data(), 16, 2 * N, g); fwrite(o.sf.data(), 16, N, g); fwrite(o.spdf.data(), 16, N, g); fwrite(o.si.data(), 16, N, g); }
    if (fclose(g) != 0) { perror(outPath); return 1; }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    std::string dataDir, mode, scene;
    std::vector<std::string> rest;
    int spp = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--datadir" && i + 1 < argc) dataDir = argv[++i];
        else if (a == "--spp" && i + 1 < argc) spp = atoi(argv[++i]);
        else if ((a == "--self" || a == "--eval") && mode.empty()) mode = a;
        else if (!mode.empty() && scene.empty()) scene = a;
        else rest.push_back(a);
    }
    if (scene.empty() || (mode == "--self" && rest.size() != 1) || (mode == "--eval" && rest.size() != 2)) {
        fprintf(stderr, "usage: bsdf_check [--datadir <dir>] [--spp <pixel samples>] --self scene.pbrt N | --eval scene.pbrt in.bin out.bin\n");
        return 2;
    }
    return check::Guarded(scene, [&] {
        check::InitData(dataDir, argv[0], "/../data");   // (the binary's usual location: pbrt-v4_amd/_build/bsdf_check)
        RenderOptions opt = check::QuietOptions(spp);
        const check::HostScene hs(scene, &opt);
        const int rc = mode == "--self" ? Self(hs.sv, hs.T.desc, atoi(rest[0].c_str())) : Eval(hs.sv, hs.T.desc.n_materials, rest[0].c_str(), rest[1].c_str());
        if (hs.fatalWord != 0) fprintf(stderr, "note: a material function raised the scene's fatal word (%d), as the render would\n", hs.fatalWord);
        return rc;
    });
}
