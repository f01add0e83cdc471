// tools/medium_check.cpp — the per-row bodies of wf_medium_sample_device / wf_phase_device (pbrt-v4_amd/csrc/hip/wf_boundary_medium.h)
// compiled for the host, and the render's own medium stages (MediumTrackBegin / Step / End = KSampleMediumInteraction, and
// KSampleMediumScattering: csrc/common/wf_kernels.h) run on a ONE-SLOT WorkState over a scene file's tables.  Stand-alone: the parser
// and BuildSceneTables, no device, neither library.
//
//   medium_check [--datadir DIR] --self SCENE N
//       N pseudo-random rows — origins inside the scene's bounds (the grids' boxes included), every medium id from -1 to two past the
//       table, hit distances and infinite rays, non-unit spectra, alternating flags, a handful of rows that must not be walked —
//       through the new bodies (lean and full where the scene allows both) and through the render's stage on a one-slot WorkState: the
//       slot's beta / r_u / r_l, the scatter point, the pixel's L, the next ray and the shadow item must be equal word for word.
//       Prints one JSON line; exits non-zero on a mismatch.
//   medium_check [--datadir DIR] --eval SCENE in.bin out.bin
//       the bodies' outputs for the rows of in.bin: the expected values of the GPU tests.
//       in.bin   int32 {magic 0x4d444331, call (0 medium sample, 1 phase), n, has_flags, has_wi, has_u, 0, 0}
//                call 0: rays8 [n][8] f32, medium [n] i32, lambda4, beta4, r_u4, r_l4 [n][4], flags [n] if has_flags
//                call 1: rays8 [n][8], p_g4 [n][4], wi4 [n][4] if has_wi, u4 [n][4] if has_u
//       out.bin  call 0: event4 [n][4] i32, p_g4, beta4, r_u4, r_l4, L4 [n][4]
//                call 1: p_pdf4 [n][4] if has_wi; sample4 [n][4], next_rays8 [n][8] if has_u
// Built with -fsanitize=address,undefined it is how that code is run under the sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../pbrt-v4_amd/csrc/hip/wf_boundary_light.h"
#include "../pbrt-v4_amd/csrc/hip/wf_boundary_medium.h"
#include "check_common.h"

using namespace wf;

namespace {

constexpr int32_t MAGIC = 0x4d444331;

struct Rows {
    int n = 0;
    std::vector<F4> rays, lambda4, beta4, ru4, rl4, pG4, wi4, u4;
    std::vector<int32_t> medium, flags;
    bool hasFlags = false, hasWi = false, hasU = false;
};

bool MediaAllLean(const wf_scene_desc &d) {
    for (int m = 0; m < d.n_media; ++m)
        if (!(d.media[m].type == WF_MEDIUM_HOMOGENEOUS || (d.media[m].type == WF_MEDIUM_GRID && !d.media[m].is_emissive))) return false;
    return d.n_media > 0;
}

template <bool LEAN>
bmedium::TrackRow BodyTrack(const SceneView &sv, int nMedia, const Rows &r, size_t i) {
    const bmedium::TrackItem it = bmedium::LoadTrackItem(nMedia, r.rays.data(), r.medium.data(), r.lambda4.data(), r.beta4.data(), r.ru4.data(), r.rl4.data(),
                                                         r.hasFlags ? r.flags.data() : nullptr, i);
    return bmedium::TrackItemRow<LEAN>(sv, it);
}

// ---- the render's stages on a one-slot WorkState ------------------------------------------------------------------------------------------
struct OneSlot {
    WorkState ws{};
    F4 q[2][9];          // the two ray queues' planes: o, d, beta, r_u, r_l, ctx0, ctx1, ctx2 (+ one spare)
    I4 meta[2];
    F4 hit, scatterP, L, lambda, lambdaPdf, samples0, samples1, sq[5];
    float hitT = 0;
    int32_t hitInst = -1, mixMat = 0, sqMedium = -1, qs[8 + WF_MAT_NTYPES];
    int32_t counters[CNT_COUNT * CNT_STRIDE];
    OneSlot() {
        for (int c = 0; c < 2; ++c) {
            RayQueueV &v = ws.rq[c];
            v.o = &q[c][0]; v.d = &q[c][1]; v.beta = &q[c][2]; v.r_u = &q[c][3]; v.r_l = &q[c][4]; v.ctx0 = &q[c][5]; v.ctx1 = &q[c][6]; v.ctx2 = &q[c][7];
            v.meta = &meta[c];
        }
        ws.maxQueueSize = 1; ws.pixelsPerPass = 1; ws.samplesPerPass = 1;
        ws.hit = &hit; ws.hitInst = &hitInst; ws.hitT = &hitT; ws.scatterP = &scatterP; ws.L = &L; ws.lambda = &lambda; ws.lambdaPdf = &lambdaPdf;
        ws.samples0 = &samples0; ws.samples1 = &samples1; ws.mixMat = &mixMat;
        ws.escapedQ = &qs[0]; ws.hitLightQ = &qs[1]; ws.mediumSampleQ = &qs[2]; ws.mediumScatterQ = &qs[3]; ws.mediumRouteQ = &qs[4]; ws.mixQ = &qs[5];
        for (int t = 0; t < WF_MAT_NTYPES; ++t) ws.matQ[t] = &qs[8 + t];
        ws.sq.o = &sq[0]; ws.sq.d = &sq[1]; ws.sq.Ld = &sq[2]; ws.sq.r_u = &sq[3]; ws.sq.r_l = &sq[4]; ws.sq.medium = &sqMedium;
        ws.counters = counters;
    }
    void Reset() {
        memset(q, 0, sizeof q); memset(meta, 0, sizeof meta); memset(qs, 0, sizeof qs); memset(counters, 0, sizeof counters); memset(sq, 0, sizeof sq);
        hit = scatterP = L = samples0 = samples1 = F4{0, 0, 0, 0};
        lambdaPdf = F4{1, 1, 1, 1};
        hitInst = -1; mixMat = 0; sqMedium = -1;
    }
    int Count(int c) const { return counters[c * CNT_STRIDE]; }
};

// what the render's medium-sample stage leaves for one item.  depth 0, or maxDepth where the row's flag is clear
// fromQueues: the kind was read off what the stage left in its queues, not off the tracking state
struct Witness { int kind; bool fromQueues; F4 beta, r_u, r_l, pG, L; };
Witness RenderTrack(const SceneView &sv, OneSlot &S, const Rows &r, size_t i, int depth, int routePrim) {
    S.Reset();
    const F4 r0 = r.rays[2 * i], r1 = r.rays[2 * i + 1];
    S.q[0][0] = F4{r0.x, r0.y, r0.z, r1.w};
    S.q[0][1] = F4{r0.w, r1.x, r1.y, 1.f};
    S.q[0][2] = r.beta4[i]; S.q[0][3] = r.ru4[i]; S.q[0][4] = r.rl4[i];
    S.meta[0] = I4{0, depth, 0, r.medium[i]};
    S.hitT = r1.z;
    S.hit = F4{BitsToFloat((uint32_t)routePrim), 1.f / 3, 1.f / 3, 1.f / 3};
    S.lambda = r.lambda4[i];
    S.qs[2] = 0;   // mediumSampleQ[0] = slot 0
    MediumTrack s;
    // KSampleMediumInteraction, with the state looked at between the loop and the write-back
    MediumTrackBegin<false>(sv, S.ws, 0, 0, s);
    while (MediumTrackStep<false>(sv, S.ws, 0, s)) {}
    Witness w{};
    const S4 T = s.stopped ? S4c(1.f) : s.T_maj;
    S4 beta = s.beta, r_u = s.r_u, r_l = s.r_l;
    if (!s.scattered && beta) { beta = beta * (T / T[0]); r_u = r_u * (T / T[0]); r_l = r_l * (T / T[0]); }
    w.kind = s.scattered ? (s.pushScatter ? 3 : 2) : (beta && r_u ? 1 : 2);
    MediumTrackEnd(sv, S.ws, 0, s);
    w.L = S.L;
    // The kind as the stage's QUEUES show it: a scatter item pushed (3); the ray routed on — to a material queue, through an interface
    // into the next ray queue, to the emitter or the escaped queue (1); neither (2).  Not visible where the stage routes nothing: at
    // depth == maxDepth, and for a ray that leaves a scene without infinite lights.
    if (depth < sv.maxDepth && (!IsInf(r1.z) || sv.nInfiniteLights > 0)) {
        int routed = S.Count(CNT_RAY1) + S.Count(CNT_ESCAPED) + S.Count(CNT_HITLIGHT);
        for (int t = 0; t < WF_MAT_NTYPES; ++t) routed += S.Count(CNT_MAT0 + t);
        const int queueKind = S.Count(CNT_MEDIUM_SCATTER) == 1 ? 3 : routed > 0 ? 1 : 2;
        if (queueKind != w.kind) { w.kind = -1; return w; }
        w.fromQueues = true;
    }
    if (w.kind == 2) { w.beta = toF4(beta); w.r_u = toF4(r_u); w.r_l = toF4(r_l); return w; }
    // kinds 1 and 3: what the stage wrote back into the ray slot (at depth == maxDepth it drops an arriving item without the write-back)
    w.beta = S.q[0][2]; w.r_u = S.q[0][3]; w.r_l = S.q[0][4];
    if (w.kind == 3) { w.pG = S.scatterP; if (S.Count(CNT_MEDIUM_SCATTER) != 1) w.kind = -1; }
    return w;
}

// ---- --self ------------------------------------------------------------------------------------------------------------------------------
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
    F4 spectrum() { return F4{0.25f + 1.5f * u(), 0.25f + 1.5f * u(), 0.25f + 1.5f * u(), 0.25f + 1.5f * u()}; }
};

bool Same(const F4 &a, const F4 &b) { return memcmp(&a, &b, 16) == 0; }
bool SameRow(const bmedium::TrackRow &a, const bmedium::TrackRow &b) {
    return memcmp(&a.event, &b.event, 16) == 0 && Same(a.pG, b.pG) && Same(a.beta, b.beta) && Same(a.r_u, b.r_u) && Same(a.r_l, b.r_l) && Same(a.L, b.L);
}

int Self(const SceneView &sv, const wf_scene_desc &d, int n) {
    const size_t N = (size_t)n;
    const int nMedia = d.n_media;
    const bool lean = MediaAllLean(d);
    if (nMedia <= 0) { fprintf(stderr, "the scene has no media\n"); return 1; }
    Gen g(11, d);
    Rows r;
    r.n = n; r.hasFlags = true;
    r.rays.resize(2 * N); r.lambda4.resize(N); r.beta4.resize(N); r.ru4.resize(N); r.rl4.resize(N); r.medium.resize(N); r.flags.resize(N);
    const float extent = Length(V3{g.hi[0] - g.lo[0], g.hi[1] - g.lo[1], g.hi[2] - g.lo[2]});
    const float nan = BitsToFloat(0x7fc00000u);
    for (size_t i = 0; i < N; ++i) {
        V3 o = g.point(), dd = g.dir() * (0.5f + g.u());
        float tMax = i % 4 == 1 ? WF_INFINITY : g.u() * extent;
        r.medium[i] = (int)(g.u() * (nMedia + 3)) - 1;
        if (r.medium[i] > nMedia + 1) r.medium[i] = nMedia + 1;
        // the rows that must not be walked
        switch (i % 61) {
        case 7: o.x = nan; break;
        case 13: o.y = WF_INFINITY; break;
        case 19: dd = V3{0, 0, 0}; break;
        case 23: dd.z = nan; break;
        case 29: dd.x = -WF_INFINITY; break;
        case 31: tMax = nan; break;
        case 37: tMax = -1.f; break;
        case 41: dd = V3{1e-30f, 0, 0}; break;
        case 43: dd = V3{1e30f, 1e30f, 0}; break;
        default: break;
        }
        const float time = g.u();
        r.rays[2 * i] = F4{o.x, o.y, o.z, dd.x};
        r.rays[2 * i + 1] = F4{dd.y, dd.z, tMax, time};
        r.lambda4[i] = check::RotatedWavelengths(g.u());
        r.beta4[i] = g.spectrum(); r.ru4[i] = g.spectrum(); r.rl4[i] = g.spectrum();
        r.flags[i] = (int)(i & 1);
    }
    OneSlot S;
    long skipped = 0, queueKinds = 0, mismatches = 0, kinds[4] = {0, 0, 0, 0}, nullCollisions = 0, multi = 0, emitting = 0, phaseRows = 0, shadowRows = 0;
    int maxSteps = 0;
    auto bad = [&](size_t i, const char *what) { if (mismatches++ < 8) fprintf(stderr, "row %zu (medium %d): %s\n", i, r.medium[i], what); };
    for (size_t i = 0; i < N; ++i) {
        const bmedium::TrackRow full = BodyTrack<false>(sv, nMedia, r, i);
        if (lean && !SameRow(full, BodyTrack<true>(sv, nMedia, r, i))) bad(i, "the lean and the full bodies differ");
        const int kind = full.event.x, steps = full.event.y;
        if (kind < 0 || kind > 3) { bad(i, "kind out of range"); continue; }
        ++kinds[kind];
        if (steps > maxSteps) maxSteps = steps;
        multi += steps > 1;
        nullCollisions += kind == 1 ? steps : (steps > 0 ? steps - 1 : 0);
        emitting += (full.L.x != 0 || full.L.y != 0 || full.L.z != 0 || full.L.w != 0);
        const bmedium::TrackItem it = bmedium::LoadTrackItem(nMedia, r.rays.data(), r.medium.data(), r.lambda4.data(), r.beta4.data(), r.ru4.data(), r.rl4.data(), r.flags.data(), i);
        if (it.kind >= 0) {
            // not walked: zeros, or the spectra as they came
            bmedium::TrackRow want;
            if (r.medium[i] < 0) { want.event.x = 1; want.beta = r.beta4[i]; want.r_u = r.ru4[i]; want.r_l = r.rl4[i]; }
            if ((r.medium[i] < 0) != (it.kind == 1) || !SameRow(full, want)) bad(i, "an unwalked row is not zeros / a copy");
            continue;
        }
        if (sv.nTriangles == 0 && !IsInf(r.rays[2 * i + 1].z)) { ++skipped; continue; }   // (the stage's routing of an arriving ray needs a triangle to route to: reported)
        const bool flag = (r.flags[i] & 1) != 0;
        // the event, the spectra and the scatter point from the stage at depth 0, where it routes; the pixel's L from the stage at the
        // depth the flag stands for (at maxDepth it collects no emission and drops an arriving item without the write-back)
        const Witness sp = RenderTrack(sv, S, r, i, 0, 0);
        if (sp.kind != kind) { bad(i, "the event differs from the render's"); continue; }
        queueKinds += sp.fromQueues;
        if (!Same(sp.pG, full.pG)) bad(i, "the scatter point differs");
        if (!Same(sp.beta, full.beta) || !Same(sp.r_u, full.r_u) || !Same(sp.r_l, full.r_l)) bad(i, "the spectra differ from the ray slot's");
        const Witness w = flag ? sp : RenderTrack(sv, S, r, i, sv.maxDepth, 0);
        if (!Same(w.L, full.L)) bad(i, "L differs from the pixel's");
        if (!flag && kind == 3 && (w.kind != 3 || !Same(w.pG, full.pG) || !Same(w.beta, full.beta) || !Same(w.r_u, full.r_u))) bad(i, "the scatter at maxDepth differs");
        if (kind != 3) continue;
        // the scatter: KSampleMediumScattering on the slot, with unit throughput so that the queues show the phase values themselves
        Rows p;
        p.n = 1; p.hasWi = true; p.hasU = true;
        p.rays = {r.rays[2 * i], r.rays[2 * i + 1]};
        p.pG4 = {full.pG};
        const F4 s0{g.u(), g.u(), g.u(), g.u()}, s1{g.u(), g.u(), g.u(), g.u()};
        p.u4 = {F4{s1.x, s1.y, 0, 0}};
        S.Reset();
        S.q[0][0] = F4{r.rays[2 * i].x, r.rays[2 * i].y, r.rays[2 * i].z, r.rays[2 * i + 1].w};
        S.q[0][1] = F4{r.rays[2 * i].w, r.rays[2 * i + 1].x, r.rays[2 * i + 1].y, 1.f};
        S.q[0][2] = F4{1, 1, 1, 1}; S.q[0][3] = F4{1, 1, 1, 1};
        S.meta[0] = I4{0, 0, 0, r.medium[i]};
        S.scatterP = full.pG; S.lambda = r.lambda4[i]; S.samples0 = s0; S.samples1 = s1;
        S.qs[3] = 0;
        KSampleMediumScattering<true>(sv, S.ws, 0, 0);
        // the light the stage sampled, for the direction of the wi half
        Wavelengths lambda{};
        memcpy(lambda.lambda, &r.lambda4[i], 16);
        const V3 pp{full.pG.x, full.pG.y, full.pG.z};
        const LightCtx ctx{MakeP3i(pp), N3{0, 0, 0}, N3{0, 0, 0}};
        float pmf = 0;
        const int lightId = LightSamplerSample(sv, ctx, s0.x, &pmf);
        LightLiSample ls{};
        bool lit = false;
        if (lightId >= 0) { ls = LightSampleLi<true>(sv, sv.lights[lightId], ctx, V2{s0.y, s0.z}, lambda, true); lit = ls.valid && ls.L && ls.pdf > 0; }
        p.wi4 = {lit ? F4{ls.wi.x, ls.wi.y, ls.wi.z, 0} : F4{0, 0, 1, 0}};
        const bmedium::PhaseRow ph = bmedium::PhaseItem(p.rays.data(), p.pG4.data(), p.wi4.data(), p.u4.data(), 0);
        ++phaseRows;
        if ((S.Count(CNT_SHADOW) == 1) != lit) bad(i, "the shadow item's presence differs");
        if (lit) {
            ++shadowRows;
            const S4 beta = S4c(1.f) * ph.pPdf.x;
            const F4 Ld = toF4(beta * ls.L), ru = toF4(S4c(1.f) * (IsDeltaLight(sv.lights[lightId]) ? 0.f : ph.pPdf.y));
            if (!Same(Ld, S.sq[2]) || !Same(ru, S.sq[3])) bad(i, "phase.p / phase.PDF differ from the shadow item's");
            // the vertex's light sample through the light boundary's bodies on the planes of a medium point (Scene.medium_light_planes):
            // its shadow ray is the stage's
            blight::SampleItem li;
            li.pi = MakeP3i(pp); li.time = r.rays[2 * i + 1].w; li.valid = 1; li.mediumInside = li.mediumOutside = r.medium[i];
            li.u0 = s0.x; li.u = V2{s0.y, s0.z};
            memcpy(li.lambda, &r.lambda4[i], 16);
            const NeeRequest rq = blight::SampleRequest(li);
            const blight::SampleRow lr = blight::SampleFinish(sv, li, SampleLightForBlock<true>(sv, rq.want, rq.ctx, rq.u0, rq.u, rq.lambda));
            const F4 so = S.sq[0], sd = S.sq[1];
            const F4 e0{so.x, so.y, so.z, sd.x}, e1{sd.y, sd.z, so.w, li.time};
            if (!Same(e0, lr.ray0) || !Same(e1, lr.ray1) || lr.light.w != S.sqMedium || !Same(lr.L, toF4(ls.L))) bad(i, "the light boundary's shadow ray of a medium point differs from the stage's");
        }
        const bool pushed = S.Count(CNT_RAY1) == 1;
        if (pushed != (ph.sample.y != 0)) { bad(i, "the next ray's presence differs"); continue; }
        if (pushed) {
            const F4 o = S.q[1][0], dd = S.q[1][1];
            const F4 e0{o.x, o.y, o.z, dd.x}, e1{dd.y, dd.z, WF_INFINITY, o.w};
            const F4 rl = toF4(S4c(1.f) / ph.sample.y), be = toF4(S4c(1.f) * ph.sample.x / ph.sample.y);
            if (!Same(e0, ph.ray0) || !Same(e1, ph.ray1) || !Same(rl, S.q[1][4]) || !Same(be, S.q[1][2])) bad(i, "Sample_p differs from the next ray's");
        } else if (!Same(ph.ray0, F4{0, 0, 0, 0}) || !Same(ph.ray1, F4{0, 0, 0, 0})) bad(i, "a sample with pdf 0 is not zeros");
    }
    printf("{\"rows\": %d, \"mismatches\": %ld, \"kinds\": [%ld, %ld, %ld, %ld], \"null_collisions\": %ld, \"multi_collision_rows\": %ld, \"emitting\": %ld, "
           "\"max_steps\": %d, \"phase_rows\": %ld, \"shadow_rows\": %ld, \"media\": %d, \"medium_lean\": %d, \"skipped\": %ld, \"kinds_from_queues\": %ld}\n",
           n, mismatches, kinds[0], kinds[1], kinds[2], kinds[3], nullCollisions, multi, emitting, maxSteps, phaseRows, shadowRows, nMedia, lean ? 1 : 0, skipped, queueKinds);
    return mismatches == 0 ? 0 : 1;
}

// ---- --eval ------------------------------------------------------------------------------------------------------------------------------
using check::ReadVec;
int Eval(const SceneView &sv, const wf_scene_desc &d, const char *inPath, const char *outPath) {
    FILE *f = fopen(inPath, "rb");
    if (!f) { perror(inPath); return 1; }
    int32_t h[8];
    if (fread(h, 4, 8, f) != 8 || h[0] != MAGIC || h[1] < 0 || h[1] > 1 || h[2] < 0 || h[2] > (1 << 24)) { fprintf(stderr, "%s: not an input file of this program\n", inPath); fclose(f); return 1; }
    Rows r;
    const int call = h[1];
    r.n = h[2]; r.hasFlags = h[3] != 0; r.hasWi = h[4] != 0; r.hasU = h[5] != 0;
    const size_t N = (size_t)r.n;
    bool ok = ReadVec(f, r.rays, 2 * N);
    if (call == 0) ok = ok && ReadVec(f, r.medium, N) && ReadVec(f, r.lambda4, N) && ReadVec(f, r.beta4, N) && ReadVec(f, r.ru4, N) && ReadVec(f, r.rl4, N) && ReadVec(f, r.flags, r.hasFlags ? N : 0);
    else ok = ok && ReadVec(f, r.pG4, N) && ReadVec(f, r.wi4, r.hasWi ? N : 0) && ReadVec(f, r.u4, r.hasU ? N : 0);
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short file\n", inPath); return 1; }
    if (call == 1 && !r.hasWi && !r.hasU) { fprintf(stderr, "neither wi4 nor u4\n"); return 1; }
    if (d.n_media <= 0) { fprintf(stderr, "the scene has no media\n"); return 1; }
    FILE *g = fopen(outPath, "wb");
    if (!g) { perror(outPath); return 1; }
    if (call == 0) {
        std::vector<I4> ev(N);
        std::vector<F4> pG(N), beta(N), ru(N), rl(N), L(N);
        long steps = 0;
        for (size_t i = 0; i < N; ++i) {
            const bmedium::TrackRow row = BodyTrack<false>(sv, d.n_media, r, i);
            ev[i] = row.event; pG[i] = row.pG; beta[i] = row.beta; ru[i] = row.r_u; rl[i] = row.r_l; L[i] = row.L;
            steps += row.event.y;
        }
        fwrite(ev.data(), 16, N, g); fwrite(pG.data(), 16, N, g); fwrite(beta.data(), 16, N, g); fwrite(ru.data(), 16, N, g); fwrite(rl.data(), 16, N, g); fwrite(L.data(), 16, N, g);
        printf("{\"rows\": %zu, \"steps\": %ld}\n", N, steps);
    } else {
        std::vector<F4> pp(N), sm(N), nx(2 * N);
        for (size_t i = 0; i < N; ++i) {
            const bmedium::PhaseRow row = bmedium::PhaseItem(r.rays.data(), r.pG4.data(), r.hasWi ? r.wi4.data() : nullptr, r.hasU ? r.u4.data() : nullptr, i);
            pp[i] = row.pPdf; sm[i] = row.sample; nx[2 * i] = row.ray0; nx[2 * i + 1] = row.ray1;
        }
        if (r.hasWi) fwrite(pp.data(), 16, N, g);
        if (r.hasU) { fwrite(sm.data(), 16, N, g); fwrite(nx.data(), 16, 2 * N, g); }
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
        fprintf(stderr, "usage: medium_check [--datadir <dir>] --self scene.pbrt N | --eval scene.pbrt in.bin out.bin\n");
        return 2;
    }
    return check::Guarded(scene, [&] {
        check::InitData(dataDir, argv[0], "/../data");   // (the binary's usual location: pbrt-v4_amd/_build/medium_check)
        RenderOptions opt = check::QuietOptions();
        const check::HostScene hs(scene, &opt);
        const int rc = mode == "--self" ? Self(hs.sv, hs.T.desc, atoi(rest[0].c_str())) : Eval(hs.sv, hs.T.desc, rest[0].c_str(), rest[1].c_str());
        if (hs.fatalWord != 0) { fprintf(stderr, "a scene function raised the scene's fatal word (%d)\n", hs.fatalWord); return 1; }
        return rc;
    });
}
