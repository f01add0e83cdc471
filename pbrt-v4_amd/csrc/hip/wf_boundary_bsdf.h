// wf_boundary_bsdf.h — the per-row bodies of wf_bsdf_make_device / wf_bsdf_eval_device (include/wf_abi.h) and the launchers of
// wf_boundary_bsdf.hip.  The bodies are host + device: the kernels run them one row per lane, tools/bsdf_check.cpp compiles them for the
// host and runs them against a direct composition of the render's functions.  They add no arithmetic of their own: a row's BSDF is
// MatShade's (wf_kernels.h; surfscatter.cpp:57-145) from the texture context to bsdf.Regularize(), on the row's planes instead of on
// (primitive, barycentrics); its evaluation and its sample are BSDF<BxDF>::f / PDF / Sample_f and the lines of MatShade / MatNeeFinish
// around them.  MatShade's lines are RESTATED here and not shared with it: nothing the render's kernels include changes with this file.
//
// The planes are wf_hit_interaction_device's: item i of plane p is the 16 bytes at planes[p * n + i].
//   planes_f  0  pi lower | uv[0]    1  pi upper | uv[1]    2  n | time    3  ns | t    4  wo | 0    5, 6  dpdu, dpdv
//             7, 8  shading dpdu, dpdv    9, 10  shading dndu, dndv
//   planes_i  0  material, area light, medium inside, medium outside        1  mesh, valid, mesh flags, 0
// The record (bsdf_rec, WF_BSDF_PLANES planes of the same stride):
//   0  {type, flags, material, 0} as int bits    1  the final ns | 0    2  the final shading dpdu | 0    3 - 9  the BxDF's numbers
// The BxDF is stored FIELD BY FIELD (Pack / Unpack below), not as the bytes of the struct: a record holds no address and no padding, so
// it is the same words on the host and on the device, and a kernel cannot be led anywhere by it.  What a BxDF points to (the scene's
// fatal word, the measured tables) and what bounds its loops (a layered BxDF's depth and sample count) come back from the scene.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../common/wf_kernels.h"

namespace wf {
namespace bbsdf {

constexpr int REC_PLANES = WF_BSDF_PLANES;
constexpr int BX_PLANE0 = 3, BX_PLANES = REC_PLANES - BX_PLANE0, BX_WORDS = 4 * BX_PLANES;
constexpr int FLAG_TERMINATED = 1 << 8;   // bsdf4 word 0: Get terminated the secondary wavelengths

template <int MAT> struct FitsRecord {
    static constexpr bool value = sizeof(typename MatBxDF<MAT>::T) <= (size_t)BX_PLANES * 16;
};
static_assert(FitsRecord<WF_MAT_DIFFUSE>::value && FitsRecord<WF_MAT_CONDUCTOR>::value && FitsRecord<WF_MAT_DIELECTRIC>::value &&
              FitsRecord<WF_MAT_THIN_DIELECTRIC>::value && FitsRecord<WF_MAT_DIFFUSE_TRANSMISSION>::value && FitsRecord<WF_MAT_COATED_DIFFUSE>::value &&
              FitsRecord<WF_MAT_COATED_CONDUCTOR>::value && FitsRecord<WF_MAT_SUBSURFACE>::value && FitsRecord<WF_MAT_HAIR>::value &&
              FitsRecord<WF_MAT_MEASURED>::value, "every BxDF fits the record's seven planes (the coated conductor is the largest)");

// ---- a BxDF's numbers as words of the record, and back -------------------------------------------------------------------------------
// Pack returns the words it wrote; Unpack reads the same words in the same order.
WF_HD int PackS4(float *w, const S4 &s) { for (int k = 0; k < 4; ++k) w[k] = s[k]; return 4; }
WF_HD int UnpackS4(const float *w, S4 *s) { for (int k = 0; k < 4; ++k) (*s)[k] = w[k]; return 4; }
WF_HD int PackTR(float *w, const TrowbridgeReitz &d) { w[0] = d.alpha_x; w[1] = d.alpha_y; return 2; }
WF_HD int UnpackTR(const float *w, TrowbridgeReitz *d) { d->alpha_x = w[0]; d->alpha_y = w[1]; return 2; }   // (as they are: the constructor's clamp has happened)

WF_HD int Pack(float *w, const DiffuseBxDF &b) { return PackS4(w, b.R); }
WF_HD int Unpack(const float *w, const SceneView &, const wf_material &, DiffuseBxDF *b) { return UnpackS4(w, &b->R); }
WF_HD int Pack(float *w, const DiffuseTransmissionBxDF &b) { PackS4(w, b.R); PackS4(w + 4, b.T); return 8; }
WF_HD int Unpack(const float *w, const SceneView &, const wf_material &, DiffuseTransmissionBxDF *b) { UnpackS4(w, &b->R); UnpackS4(w + 4, &b->T); return 8; }
WF_HD int Pack(float *w, const DielectricBxDF &b) { w[0] = b.eta; PackTR(w + 1, b.mfDistrib); return 3; }
WF_HD int Unpack(const float *w, const SceneView &sv, const wf_material &, DielectricBxDF *b) {
    b->eta = w[0]; UnpackTR(w + 1, &b->mfDistrib);
    b->fatal = sv.fatal;   // (where the render's own BxDF reports the reference's CHECK)
    return 3;
}
WF_HD int Pack(float *w, const ThinDielectricBxDF &b) { w[0] = b.eta; return 1; }
WF_HD int Unpack(const float *w, const SceneView &, const wf_material &, ThinDielectricBxDF *b) { b->eta = w[0]; return 1; }
WF_HD int Pack(float *w, const ConductorBxDF &b) { PackTR(w, b.mfDistrib); PackS4(w + 2, b.eta); PackS4(w + 6, b.k); return 10; }
WF_HD int Unpack(const float *w, const SceneView &, const wf_material &, ConductorBxDF *b) { UnpackTR(w, &b->mfDistrib); UnpackS4(w + 2, &b->eta); UnpackS4(w + 6, &b->k); return 10; }
WF_HD int Pack(float *w, const HairBxDF &b) {
    int k = 0;
    w[k++] = b.h; w[k++] = b.eta;
    k += PackS4(w + k, b.sigma_a);
    w[k++] = b.beta_m; w[k++] = b.beta_n;
    for (int p = 0; p <= HairBxDF::pMax; ++p) w[k++] = b.v[p];
    w[k++] = b.s;
    for (int p = 0; p < HairBxDF::pMax; ++p) w[k++] = b.sin2kAlpha[p];
    for (int p = 0; p < HairBxDF::pMax; ++p) w[k++] = b.cos2kAlpha[p];
    return k;
}
WF_HD int Unpack(const float *w, const SceneView &, const wf_material &, HairBxDF *b) {
    int k = 0;
    b->h = w[k++]; b->eta = w[k++];
    k += UnpackS4(w + k, &b->sigma_a);
    b->beta_m = w[k++]; b->beta_n = w[k++];
    for (int p = 0; p <= HairBxDF::pMax; ++p) b->v[p] = w[k++];
    b->s = w[k++];
    for (int p = 0; p < HairBxDF::pMax; ++p) b->sin2kAlpha[p] = w[k++];
    for (int p = 0; p < HairBxDF::pMax; ++p) b->cos2kAlpha[p] = w[k++];
    return k;
}
WF_HD int Pack(float *w, const MeasuredBxDF &b) { for (int k = 0; k < 4; ++k) w[k] = b.lambda[k]; return 4; }
WF_HD int Unpack(const float *w, const SceneView &sv, const wf_material &m, MeasuredBxDF *b) {
    b->table = sv.tableData; b->hdr = m.measured_table;   // (the scene's, by the row's material: never the record's)
    for (int k = 0; k < 4; ++k) b->lambda[k] = w[k];
    return 4;
}
template <typename Top, typename Bottom, bool TS>
WF_HD int Pack(float *w, const LayeredBxDF<Top, Bottom, TS> &b) {
    int k = Pack(w, b.top);
    k += Pack(w + k, b.bottom);
    w[k++] = b.thickness; w[k++] = b.g;
    k += PackS4(w + k, b.albedo);
    return k;
}
template <typename Top, typename Bottom, bool TS>
WF_HD int Unpack(const float *w, const SceneView &sv, const wf_material &m, LayeredBxDF<Top, Bottom, TS> *b) {
    int k = Unpack(w, sv, m, &b->top);
    k += Unpack(w + k, sv, m, &b->bottom);
    b->thickness = w[k++]; b->g = w[k++];
    k += UnpackS4(w + k, &b->albedo);
    b->maxDepth = m.maxdepth; b->nSamples = m.nsamples; b->seed = sv.options.seed;   // (GetCoated*BxDF's own sources: the loops' bounds are the scene's)
    return k;
}

// ---- which rows have a BSDF ----------------------------------------------------------------------------------------------------------
WF_HD bool IsBsdfType(int t) { return t >= WF_MAT_DIFFUSE && t < WF_MAT_NTYPES; }

// ResolveMix (wf_kernels.h; intersect.h:92-97, materials.h:284-294) on a row's planes: the texture context is (pi.mid(), n, uv) of the
// interaction, the hash takes wo = -ray.d as the ray carries it (not normalised)
WF_HD int ResolveMixRow(const SceneView &sv, int matId, const TexCtx &tc, V3 wo) {
    while (sv.materials[matId].type == WF_MAT_MIX) {
        const wf_material &m = sv.materials[matId];
        float amt = EvalFloatTexture(sv, m.tex[WF_MT_AMOUNT], tc);
        int pick;
        if (amt <= 0) pick = 0;
        else if (amt >= 1) pick = 1;
        else {
            uint32_t w[8] = {FloatToBits(tc.p.x), FloatToBits(tc.p.y), FloatToBits(tc.p.z), FloatToBits(wo.x), FloatToBits(wo.y), FloatToBits(wo.z),
                             (uint32_t)m.mix[0], (uint32_t)m.mix[1]};
            float u = HashToFloat(HashWords(w, 8));
            pick = (amt < u) ? 0 : 1;
        }
        matId = m.mix[pick];
    }
    return matId;
}
// The routing pass's answer for row i: the resolved material id of a row with a BSDF, -1 for a row without one (valid != 1, an
// interface surface, an id outside the scene's table — a stale buffer does not walk the tables)
WF_HD int RouteRow(const SceneView &sv, int nMaterials, const F4 *rays, const F4 *planesF, const I4 *planesI, size_t N, size_t i) {
    if (planesI[N + i].y != 1) return -1;
    int matId = planesI[i].x;
    if (matId < 0 || matId >= nMaterials) return -1;
    if (sv.materials[matId].type == WF_MAT_MIX) {
        const F4 f0 = planesF[i], f1 = planesF[N + i], f2 = planesF[2 * N + i];
        const F4 r0 = rays[2 * i], r1 = rays[2 * i + 1];   // o.xyz d.x | d.yz tMax time
        const P3i pi{V3{f0.x, f0.y, f0.z}, V3{f1.x, f1.y, f1.z}};
        TexCtx tc;
        tc.p = pi.mid(); tc.n = N3{f2.x, f2.y, f2.z}; tc.uv = V2{f0.w, f1.w};
        matId = ResolveMixRow(sv, matId, tc, V3{-r0.w, -r1.x, -r1.y});
        if (matId < 0 || matId >= nMaterials) return -1;
    }
    return IsBsdfType(sv.materials[matId].type) ? matId : -1;
}

// ---- wf_bsdf_make_device -------------------------------------------------------------------------------------------------------------
struct MakeRowOut {
    F4 rec[REC_PLANES];
    I4 bsdf4{0, 0, 0, 0};
};
WF_HD void ZeroMakeRow(MakeRowOut *out) {
    for (int p = 0; p < REC_PLANES; ++p) out->rec[p] = F4{0, 0, 0, 0};
    out->bsdf4 = I4{0, 0, 0, 0};
}
WF_HD F4 IntsAsF4(int a, int b, int c, int d) { return F4{BitsToFloat((uint32_t)a), BitsToFloat((uint32_t)b), BitsToFloat((uint32_t)c), BitsToFloat((uint32_t)d)}; }

// MatShade from the texture context to bsdf.Regularize() for a row of material matId (of type MAT).  CAMANIM: the camera moves
// (ApproximateDpDxy at the row's time); the footprint block always runs, as in the render's general variants.
template <int MAT, bool CAMANIM>
WF_HD void MakeRow(const SceneView &sv, int matId, const F4 *planesF, size_t N, size_t i, F4 lam, bool regularize, MakeRowOut *out) {
    using BxDF = typename MatBxDF<MAT>::T;
    const wf_material &mat = sv.materials[matId];
    const F4 f0 = planesF[i], f1 = planesF[N + i], f2 = planesF[2 * N + i], f3 = planesF[3 * N + i], f4 = planesF[4 * N + i];
    const P3i pi{V3{f0.x, f0.y, f0.z}, V3{f1.x, f1.y, f1.z}};
    const N3 sin{f2.x, f2.y, f2.z}, sins{f3.x, f3.y, f3.z};
    const V3 wo{f4.x, f4.y, f4.z};
    const float time = f2.w;
    // differentials of position and (u, v) at the intersection (surfscatter.cpp:73-104)
    TexCtx tc;
    tc.p = pi.mid(); tc.n = sin; tc.uv = V2{f0.w, f1.w};
    if (!sv.options.disable_texture_filtering) {
        const F4 f5 = planesF[5 * N + i], f6 = planesF[6 * N + i];
        ApproximateDpDxy<CAMANIM>(sv, tc.p, sin, &tc.dpdx, &tc.dpdy, time);
        V3 dpdu{f5.x, f5.y, f5.z}, dpdv{f6.x, f6.y, f6.z};
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
        // (the wavefront path hands the (u, v) differentials to the textures and leaves ctx.dpdx / dpdy at zero: reproduced, as MatShade does)
        tc.dpdx = tc.dpdy = V3{0, 0, 0};
    }
    N3 ns = sins;
    const F4 f7 = planesF[7 * N + i];
    const V3 sidpdus{f7.x, f7.y, f7.z};
    V3 dpdus = sidpdus;
    if (mat.normalmap >= 0) {
        // NormalMap (materials.h:86-106) and the shading frame rebuilt from it (surfscatter.cpp:111-118)
        const F4 f8 = planesF[8 * N + i];
        const V3 sidpdvs{f8.x, f8.y, f8.z};
        V3 nm;
        NormalMapTexelP(sv.tableData, sv.texImages + mat.normalmap, tc.uv.x, tc.uv.y, &nm.x, &nm.y, &nm.z);
        nm = Normalize(nm);
        Frame frame = Frame::FromXZ(Normalize(sidpdus), toV(sins));
        nm = frame.FromLocal(nm);
        float ulen = Length(sidpdus), vlen = Length(sidpdvs);
        dpdus = Normalize(GramSchmidt(sidpdus, nm)) * ulen;
        V3 dpdvs = Normalize(Cross(nm, dpdus)) * vlen;
        ns = toN(Normalize(Cross(dpdus, dpdvs)));
        ns = FaceForward(ns, sin);
    } else if (mat.displacement >= 0) {
        // BumpMap (materials.h:109-138) and the shading frame rebuilt from it (surfscatter.cpp:120-130); the three displacement lookups
        // see n = 0 (workitems.h:268-285), reproduced
        const F4 f8 = planesF[8 * N + i], f9 = planesF[9 * N + i], f10 = planesF[10 * N + i];
        const V3 sidpdvs{f8.x, f8.y, f8.z};
        const N3 sidndus{f9.x, f9.y, f9.z}, sidndvs{f10.x, f10.y, f10.z};
        TexCtx bc = tc;
        bc.n = N3{0, 0, 0};
        TexCtx sh = bc;
        float du = .5f * (abs(tc.dudx) + abs(tc.dudy));
        if (du == 0) du = .0005f;
        sh.p = tc.p + du * sidpdus;
        sh.uv = V2{tc.uv.x + du, tc.uv.y + 0.f};
        float uDisplace = EvalFloatTexture(sv, mat.displacement, sh);
        float dv = .5f * (abs(tc.dvdx) + abs(tc.dvdy));
        if (dv == 0) dv = .0005f;
        sh.p = tc.p + dv * sidpdvs;
        sh.uv = V2{tc.uv.x + 0.f, tc.uv.y + dv};
        float vDisplace = EvalFloatTexture(sv, mat.displacement, sh);
        float displace = EvalFloatTexture(sv, mat.displacement, bc);
        dpdus = sidpdus + (uDisplace - displace) / du * toV(sins) + displace * toV(sidndus);
        V3 dpdvs = sidpdvs + (vDisplace - displace) / dv * toV(sins) + displace * toV(sidndvs);
        ns = toN(Normalize(Cross(dpdus, dpdvs)));
        ns = FaceForward(ns, sin);
    }
    // the BxDF.  The caller's wavelength PDFs are not here: every secondary wavelength counts as alive, so that Get's
    // TerminateSecondary shows (the caller repeats it on its own PDFs)
    Wavelengths lambda;
    lambda.lambda[0] = lam.x; lambda.lambda[1] = lam.y; lambda.lambda[2] = lam.z; lambda.lambda[3] = lam.w;
    for (int k = 0; k < 4; ++k) lambda.pdf[k] = 1;
    BxDF bxdf = MatBxDF<MAT>::Get(sv, mat, lambda, tc);
    if (regularize) bxdf.Regularize();
    const int flags = bxdf.Flags();
    // the side of the light sample context (surfscatter.cpp:256-261), where next-event estimation takes place at all
    int side = 0;
    if (IsNonSpecular(flags)) {
        if (IsReflective(flags) && !IsTransmissive(flags)) side = 1;
        else if (IsTransmissive(flags) && IsReflective(flags)) side = -1;
    }
    float w[BX_WORDS];
    for (int k = 0; k < BX_WORDS; ++k) w[k] = 0;
    Pack(w, bxdf);
    out->rec[0] = IntsAsF4(MAT, flags, matId, 0);
    out->rec[1] = F4{ns.x, ns.y, ns.z, 0};
    out->rec[2] = F4{dpdus.x, dpdus.y, dpdus.z, 0};
    for (int p = 0; p < BX_PLANES; ++p) out->rec[BX_PLANE0 + p] = F4{w[4 * p], w[4 * p + 1], w[4 * p + 2], w[4 * p + 3]};
    out->bsdf4 = I4{flags | (lambda.SecondaryTerminated() ? FLAG_TERMINATED : 0), side, matId, MAT};
}

// ---- wf_bsdf_eval_device -------------------------------------------------------------------------------------------------------------
// The type of a record's header if it names a BSDF of this scene (type in range, material in the scene's table and of that type), else 0:
// checked before any table is indexed by what the record says.
WF_HD int RecordType(const SceneView &sv, int nMaterials, F4 header, int *matId) {
    const int type = (int)FloatToBits(header.x), m = (int)FloatToBits(header.z);
    *matId = m;
    if (!IsBsdfType(type) || m < 0 || m >= nMaterials) return 0;
    return sv.materials[m].type == type ? type : 0;
}
struct EvalRowOut {
    F4 f{0, 0, 0, 0}, pdf{0, 0, 0, 0};                                              // the wi half
    F4 ray0{0, 0, 0, 0}, ray1{0, 0, 0, 0}, sf{0, 0, 0, 0}, spdf{0, 0, 0, 0};        // the u half
    I4 si{0, 0, 0, 0};
};
// BSDF<BxDF> rebuilt from the record of row i (of type MAT, material matId: RecordType's answer), then f / PDF for wi4[i] and
// Sample_f for u4[i] (either may be null), as MatNeeFinish and MatShade call them
template <int MAT>
WF_HD void EvalRow(const SceneView &sv, int matId, const F4 *rec, const F4 *planesF, const I4 *planesI, size_t N, size_t i, const F4 *wi4, const F4 *u4,
                   EvalRowOut *out) {
    using BxDF = typename MatBxDF<MAT>::T;
    const wf_material &mat = sv.materials[matId];
    const F4 r1 = rec[N + i], r2 = rec[2 * N + i];
    float w[BX_WORDS];
    for (int p = 0; p < BX_PLANES; ++p) {
        const F4 q = rec[(BX_PLANE0 + p) * N + i];
        w[4 * p] = q.x; w[4 * p + 1] = q.y; w[4 * p + 2] = q.z; w[4 * p + 3] = q.w;
    }
    BxDF bxdf{};
    Unpack(w, sv, mat, &bxdf);
    const N3 ns{r1.x, r1.y, r1.z};
    const BSDF<BxDF> bsdf(ns, V3{r2.x, r2.y, r2.z}, bxdf);
    const F4 f4 = planesF[4 * N + i];
    const V3 wo{f4.x, f4.y, f4.z};
    if (wi4 != nullptr) {
        const F4 q = wi4[i];
        const V3 wi{q.x, q.y, q.z};
        out->f = toF4(bsdf.f(wo, wi));
        out->pdf = F4{bsdf.PDF(wo, wi), AbsDot(wi, ns), 0, 0};
    }
    if (u4 != nullptr) {
        const F4 u = u4[i];
        const BSDFSample bs = bsdf.Sample_f(wo, u.x, V2{u.y, u.z});
        if (bs.valid) {
            const F4 f0 = planesF[i], f1 = planesF[N + i], f2 = planesF[2 * N + i];
            const P3i pi{V3{f0.x, f0.y, f0.z}, V3{f1.x, f1.y, f1.z}};
            const N3 n{f2.x, f2.y, f2.z};
            const V3 wi = bs.wi;
            const float pdfMis = bs.pdfIsProportional ? bsdf.PDF(wo, wi) : bs.pdf;   // what the render divides r_u by
            const V3 o = OffsetRayOrigin(pi, n, wi);
            int medium = -1;
            if (sv.haveMedia) { const I4 ids = planesI[i]; medium = Dot(wi, n) > 0 ? ids.w : ids.z; }
            out->sf = toF4(bs.f);
            out->spdf = F4{bs.pdf, pdfMis, AbsDot(wi, ns), bs.eta};
            out->si = I4{1, bs.flags, medium, bs.pdfIsProportional ? 1 : 0};
            out->ray0 = F4{o.x, o.y, o.z, wi.x};
            out->ray1 = F4{wi.y, wi.z, WF_INFINITY, f2.w};
        }
    }
}

// The launchers of wf_boundary_bsdf.hip, one pair per material type's code object plus the type-independent pair (hidden: shared by the
// library's units, not exported from it).  svDev: the scene view's device-resident copy; route: the context's scratch of n words
// between the routing pass and the types' launches.  Return a hipError_t (0: launched).
struct MakeArgs {
    int n = 0, nMaterials = 0;
    bool cameraAnim = false;
    const int32_t *nDevice = nullptr;
    const float *rays8 = nullptr, *planesF = nullptr, *lambda4 = nullptr;
    const int32_t *planesI = nullptr, *regularize = nullptr;
    int32_t *route = nullptr;
    float *rec = nullptr;
    int32_t *bsdf4 = nullptr;
};
struct EvalArgs {
    int n = 0, nMaterials = 0;
    const int32_t *nDevice = nullptr;
    const float *rec = nullptr, *planesF = nullptr, *wi4 = nullptr, *u4 = nullptr;
    const int32_t *planesI = nullptr;
    float *f4 = nullptr, *pdf4 = nullptr, *nextRays8 = nullptr, *sampleF4 = nullptr, *samplePdf4 = nullptr;
    int32_t *sampleI4 = nullptr;
};

}  // namespace bbsdf
}  // namespace wf
// type 0: the type-independent first kernels (k_bsdf_route: the mix resolve, the route words and the zero rows of a make call;
// k_bsdf_eval_zero: the zero rows of an eval call); types 1 - 10: that type's k_bsdf_make / k_bsdf_eval
#define WF_BSDF_LAUNCHERS(T)                                                                                                                   \
    extern "C" __attribute__((visibility("hidden"))) int wf_launch_bsdf_make_##T(void *stream, const wf::SceneView *svDev, const wf::bbsdf::MakeArgs *a); \
    extern "C" __attribute__((visibility("hidden"))) int wf_launch_bsdf_eval_##T(void *stream, const wf::SceneView *svDev, const wf::bbsdf::EvalArgs *a);
WF_BSDF_LAUNCHERS(0) WF_BSDF_LAUNCHERS(1) WF_BSDF_LAUNCHERS(2) WF_BSDF_LAUNCHERS(3) WF_BSDF_LAUNCHERS(4) WF_BSDF_LAUNCHERS(5)
WF_BSDF_LAUNCHERS(6) WF_BSDF_LAUNCHERS(7) WF_BSDF_LAUNCHERS(8) WF_BSDF_LAUNCHERS(9) WF_BSDF_LAUNCHERS(10)
