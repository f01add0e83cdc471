// wf_traverse.h — the production BVH traversal for CDNA4 (device only; included through wf_ctx.h, walked by wf_backend.hip).  The records it walks (QNode, LeafTri,
// FastBVH, FastDef, SubEntry) are declared in common/wf_fastbvh.h, which the host-only tree builder (wf_fastbvh_build.cpp) shares.
//
// The reference-order walk in common/wf_shapes.h (BVHIntersectClosest/Any) visits one 32-byte
// LinearBVHNode per step and chases three levels of indirection per triangle (bvh_prims -> tri_indices
// -> P); it stays as the *counting* variant, because SURVEY.md §8(d) defines the roofline's algorithmic
// bytes on exactly those visit counts.  The kernels that render use the layout and loop below instead.
//
// What bounds traversal on MI355X (profiles/r01_*pmc*): not HBM.  With launches of millions of rays the walk is
// bounded by VALU issue (56-75 % busy at ~30 % active lanes) and by the latency of the dependent node fetches, so
// the design minimises instructions and fetches per visited node:
//
//  * QNode (64 B, four dwordx4): an interior node carries FOUR children's bounds (the reference's binary tree with every
//    second level collapsed), quantised to 16 bits per plane on the tree's grid, with build-time outward margins.  One fetch
//    feeds four slab tests and halves the dependent fetches per ray (the two-child 32-byte layout of round 1 was measured and dropped).
//  * the slab test runs in grid coordinates: WalkInit folds the grid (base, cell), the ray (o, 1/d), the
//    reference's (1 + 2 gamma(3)) factor and an evaluation-error slack into per-ray constants, so a plane costs one
//    v_cvt (SDWA half-word select) and half a v_pk_fma; near/far planes are swapped per ray with v_perm; min/max
//    are v_max3/v_min3.  No branches inside the step.  The test is a superset of Bounds3::IntersectP on the exact
//    box (it passes whenever the reference's test passes); WHICH triangle is hit is decided only by the exact,
//    float triangle test, so results are the reference's.
//  * every node fetch is a plain global load; the top of the tree lives in the vector L1 / L2 (rounds 1-5 copied it into LDS per
//    workgroup, measured and dropped in round 6: see FetchNode in wf_backend.hip).
//  * LeafTri (48 B, three dwordx4): the three vertices of each triangle in BVH leaf order — the
//    "3 indices + 3 Point3f" of the §8(d) formula as one contiguous record, no index chase — plus the triangle's
//    routing code (material type / emissive / interface), so the end-of-batch routing gathers nothing.
//  * children are visited nearest-entry first; the node stack lives in LDS, one column per lane.
//  * "while-while": all lanes of a wave descend interior nodes until every lane sits at a leaf, leaves are
//    processed together, a workgroup finishes a batch of TBLOCK rays together (block-aggregated queue pushes).
//
// Near-ties in t (coplanar overlapping geometry, e.g. a glass box standing on the floor seen from inside) are the one
// case where the visiting order decides the result: IntersectTriangle (shapes.cpp:234-237) accepts a triangle while
// tScaled <= fl(tMax * det), so among candidates whose t agree to ~3 * 2^-24 the reference keeps the LAST one its own
// depth-first order accepts.  This walk visits nearest-entry first, so it cannot know; instead it tests and prunes
// against tMax * (1 + 2^-20) + 2^-20 of the scene extent (one fma), and a candidate that lands inside that band of the
// current best marks the ray (sign bit of RayWalk::tMax).  Marked rays are re-traced by the reference-order walk
// (k_closest_retrace / BVHIntersectClosest).  The band has to cover more than the acceptance test's own rounding: the
// computed t of two coplanar triangles differ by their evaluation errors (absolute: a few ulps of the vertex
// coordinates, not of t), and the reference prunes subtrees with the EXACT tMax against box entries that carry errors
// of the same size — a flat leaf box coplanar with the current hit is skipped or not by a hair.  Size of the band: inside a
// triangle t = sum b_i z_i with b_i in [0, 1], so its rounding error is a few ulps of max |z_i|, the sheared depth of the
// farthest vertex, which is at most sqrt(3) x (scene extent + |o|) for any triangle; 2^-20 = 16 ulps of t plus 16 ulps of the
// scene extent covers that with a margin (measured on the coplanar floor / glass-box golden: ~1e-5 at extent 16).  A wider band
// only re-traces more rays (2^-16 re-traced 1 ray in 40 on the 100-unit san-miguel-like scene: every blob resting on the ground).
// (Measured and dropped: deciding marks by the triangles' own deltaT bounds of shapes.cpp:252-266 in a slow branch —
// sound by pbrt's error analysis, but deltaT grows as distance^2 / triangle size, which forces a 2^-8 pruning band:
// +24 % closest-hit time on the bench scene.)
//
// Object instances (two-level BVH): an instance definition's tree lives in the same QNode / LeafTri arrays with its own
// quantisation grid (FastDef); a top-level leaf entry marked c.z == 4 is an instance.  The walk pushes it as a leaf
// reference with first >= INST_FIRST, and when that reference is popped it switches the lane to the instance's space
// (InstanceRay = the reference's Transform::ApplyInverse(Ray, &tMax), per-ray constants recomputed for the definition's
// grid), with the world tMax and a NODE_EXIT marker underneath on the stack; popping the marker switches back.
#pragma once
#include "../common/wf_fastbvh.h"

namespace wf {

#ifndef WF_TWAVES
#define WF_TWAVES 5   // __launch_bounds__ second argument (minimum waves per SIMD) of the traversal kernels
#endif
#ifndef WF_TWAVES_CLOSEST
#define WF_TWAVES_CLOSEST WF_TWAVES   // the one-level closest-hit walk (it carries the hit record and the near-tie code)
#endif
#ifndef WF_TWAVES_INST
#define WF_TWAVES_INST 4   // the same for the two-level (object instance) variants, which carry the render-space ray as well
#endif
#ifndef WF_TWAVES_INST_SHADOW
#define WF_TWAVES_INST_SHADOW 4   // round 3: 5 waves (96 VGPRs, 28 spilled) beat 4 by 3 %; round 4, after the zero-initialised locals: 4 waves (122 VGPRs, NOTHING spilled) 17.4 vs 18.5 ms per 16 spp (gpurun_out/r04aa)
#endif

typedef float f2 __attribute__((ext_vector_type(2)));

struct RayWalk {
    V3 o;
    RayShear sh;   // per-ray part of the triangle test (MakeRayShear)
    float tMax;    // |tMax| = nearest hit so far; sign bit set = a near-tie was seen (see above): re-trace in reference order
    // slab test in grid coordinates: entry t of an axis = fma(qNear, a, bn), exit t = fma(qFar, af, bf)
    V3 a, bn, af, bf;
    uint32_t selx, sely, selz;  // v_perm selectors: put the near plane in the low half, the far plane in the high half
    // (round 4: deriving them from the sign of `a` at every node instead frees three registers on paper; the two-level closest-hit kernel
    //  still spills the same 192 VGPRs at compile time — not pursued)
    int node;  // current ref; NODE_NONE = finished
    int prim;
    uint32_t route;  // routing code of the hit triangle (LeafTri.c.w)
    float b0, b1, b2;
    int inst;        // instance the hit primitive was reached through (-1: top level); only the INST kernel variants use it
    int curInst;     // instance whose definition is being walked (-1: top level)
};

// Per-ray constants of the box test.  Bounds3::IntersectP (util/vecmath.h:1574-1608) computes, per axis,
// tNear = (pNear - o) * invDir and tFar = (pFar - o) * invDir * (1 + 2 gamma(3)).  With pNear = base + q * cell
// that is q * (cell * invDir) + (base - o) * invDir: one fma per plane.  The evaluation error of that form is
// bounded by a few ulps of (65535 |a| + |b|); SLACK times that bound is folded into the constants (subtracted on
// the near side, added on the far side) so that the test passes whenever the reference's test on the exact
// box would: a superset of visited nodes, while the hit itself is decided by the exact triangle test.
// the slab constants from the per-axis products a = cell / d and bk = (base - o) / d
__device__ inline void WalkSlabFromAB(RayWalk &w, const float a[3], const float bk[3]) {
    constexpr float SLACK = 0x1p-20f;            // 16 ulp
    constexpr float G = 1 + 2 * gamma(3);        // the reference's tMax factor
    float bn[3], af[3], bf[3];
    uint32_t sel[3];
    for (int k = 0; k < 3; ++k) {
        const float delta = SLACK * fma(65535.f, fabsf(a[k]), fabsf(bk[k]));
        bn[k] = bk[k] - delta;
        af[k] = a[k] * G; bf[k] = fma(bk[k], G, delta * 1.001f);
        sel[k] = (FloatToBits(a[k]) >> 31) ? 0x01000302u : 0x03020100u;  // negative direction (incl. -0: the sign of 1/d, kept by the clamp): swap halves
    }
    w.a = V3{a[0], a[1], a[2]}; w.bn = V3{bn[0], bn[1], bn[2]};
    w.af = V3{af[0], af[1], af[2]}; w.bf = V3{bf[0], bf[1], bf[2]};
    w.selx = sel[0]; w.sely = sel[1]; w.selz = sel[2];
}
__device__ inline void WalkSetSlab(const float base[3], const float cell[3], RayWalk &w, V3 o, V3 d) {
    constexpr float INV_MAX = 1e28f;             // |1/d| clamp: keeps every product finite (no 0 * inf NaNs)
    const float dd[3] = {d.x, d.y, d.z}, oo[3] = {o.x, o.y, o.z};
    float a[3], bk[3];
    for (int k = 0; k < 3; ++k) {
        // v_rcp_f32 (1 ulp) instead of the IEEE division (ten instructions): the constants feed the conservative slab test only, and
        // the 16-ulp SLACK covers one more ulp in a and b (the exact triangle test keeps its IEEE divisions, MakeRayShear)
        float inv = __builtin_amdgcn_rcpf(dd[k]);
        if (!(fabsf(inv) <= INV_MAX)) inv = copysignf(INV_MAX, dd[k]);
        a[k] = cell[k] * inv; bk[k] = (base[k] - oo[k]) * inv;
    }
    WalkSlabFromAB(w, a, bk);
}
__device__ inline void WalkSetRay(const float base[3], const float cell[3], RayWalk &w, V3 o, V3 d) {
    w.o = o;
    w.sh = MakeRayShear(d);
    WalkSetSlab(base, cell, w, o, d);
}
__device__ inline void WalkInit(const FastBVH &bvh, RayWalk &w, V3 o, V3 d, float tMax) {
    WalkSetRay(bvh.base, bvh.cell, w, o, d);
    w.tMax = tMax;
    w.node = 0;
    w.prim = -1;
    w.route = 0;
    w.b0 = w.b1 = w.b2 = 0;
    w.inst = -1;
    w.curInst = -1;
}
// Switch the lane into / out of an object instance (see the header comment).  oW, dW: the ray in render space.
// Returns false when the instance is skipped.  (Measured and dropped: a cheap conservative pre-test of the definition's root box before
// the reference's ray transform — the entries it saves are too few to pay for the test: closest 56.8 vs 56.5 ms, any-hit 22.9 vs 21.7 ms
// per 16 spp on the spec scene, round 3; a LAZY transition that makes the ray exact only when a leaf holds a primitive — closest / any-hit
// 49.4 / 26.1 ms against 45.0 / 23.0, round 4.)
// ANIM (round 6): the instance may be an AnimatedPrimitive (cpu/primitive.cpp:132-158) — its transformation is interpolated at the ray's
// `time` (wf_animated.h: the reference's AnimatedTransform::Interpolate restated), as the reference-order walks do (InstanceAt<true>, wf_shapes.h).
// An animated instance is one entry of the top-level tree, bounded by the reference's motion bounds; the walk inside is the static one.
// Only the kernels of scenes that have such primitives are built with ANIM: the interpolation is an out-of-line callee whose registers
// every kernel that can reach it is allocated.
template <bool ANIM = false, typename Stack>
__device__ inline bool EnterInstance(const FastBVH &bvh, RayWalk &w, Stack &st, V3 oW, V3 dW, int entry, float time = 0) {
    const SubEntry se = bvh.subs[entry];
    const int inst = se.inst;
    if (se.node == NODE_NONE) {   // an instance of an empty definition
        WalkSetRay(bvh.base, bvh.cell, w, oW, dW);   // (a fused exit may have left the previous instance's constants: ExitInstance)
        w.node = st.empty() ? NODE_NONE : st.pop();
        return false;
    }
    wf_instance moving;
    const wf_instance &in = InstanceAt<ANIM>(*bvh.sv, bvh.instances[inst], time, &moving);
    const FastDef fd = bvh.defs[in.def];
    float tI = __builtin_fabsf(w.tMax);
    V3 oI, dI;
    InstanceRay(in, oW, dW, &tI, &oI, &dI);
    st.push((int)FloatToBits(w.tMax));
    st.push(NODE_EXIT);
    WalkSetRay(fd.base, fd.cell, w, oI, dI);
    w.tMax = (FloatToBits(w.tMax) >> 31) ? -tI : tI;
    // (a re-braided instance is entered once per subtree the ray meets: the best hit so far may lie in THIS instance from an earlier
    //  visit — marked stale, so that ExitInstance can tell a hit found during this visit, whose t becomes the render-space tMax as it
    //  is, from none, after which the saved tMax is restored)
    if (w.inst == inst) w.inst = inst | INST_STALE;
    w.curInst = inst;
    w.node = se.node;
    return true;
}
// an instance ENTRY on the stack / in a child slot (not the exit marker)
__device__ inline bool IsInstanceEntry(int node) { return node < 0 && node != NODE_NONE && node != NODE_EXIT && (int)((~(unsigned)node) >> 4) >= INST_FIRST; }
// ExitInstance recomputes the render-space walk constants.  (Measured and dropped, round 6: saving them when the ray starts and reloading
// them here — through HBM, profiles/r06_walk_constants_reload_ab_sm16.txt, or nine of them in LDS, r06_walk_constants_lds_ab_sm16.txt.)
// A lane that leaves an instance and pops another instance's entry enters it in the same step, and the render-space shear / slab
// constants in between are not rebuilt (three IEEE divisions, three v_rcp).
template <typename Stack>
__device__ inline void ExitInstance(const FastBVH &bvh, RayWalk &w, Stack &st, V3 oW, V3 dW) {
    const float saved = BitsToFloat((uint32_t)st.pop());
    // a hit found inside: its t (the instance ray's parameter) becomes the world tMax as it is, like the reference's
    // si->tHit (cpu/primitive.cpp:112-125); otherwise the world tMax is restored.  Near-tie marks are kept either way.
    const float tW = (w.inst == w.curInst) ? __builtin_fabsf(w.tMax) : __builtin_fabsf(saved);
    const bool mark = ((FloatToBits(w.tMax) | FloatToBits(saved)) >> 31) != 0;
    const int next = st.empty() ? NODE_NONE : st.pop();
    // the next entry on the stack is another subtree of the SAME instance (re-braided instances): the lane stays in the instance's space
    // and walks on there — one visit for the reference too, whose tMax runs through the whole definition
    if (IsInstanceEntry(next)) {
        const SubEntry se = bvh.subs[(int)((~(unsigned)next) >> 4) - INST_FIRST];
        if (se.inst == w.curInst && se.node != NODE_NONE) {
            st.push((int)FloatToBits(saved));
            st.push(NODE_EXIT);
            w.node = se.node;
            return;
        }
    }
    if (w.inst == (w.curInst | INST_STALE)) w.inst = w.curInst;   // the hit of an earlier visit of this instance stands
    if (!IsInstanceEntry(next)) WalkSetRay(bvh.base, bvh.cell, w, oW, dW);
    w.tMax = mark ? -tW : tW;
    w.curInst = -1;
    w.node = next;
}

__device__ inline bool WalkAmbiguous(const RayWalk &w) { return (FloatToBits(w.tMax) >> 31) != 0; }
__device__ inline float WalkT(const RayWalk &w) { return __builtin_fabsf(w.tMax); }
constexpr float TIE_BAND = 1 + 0x1p-20f;
__device__ inline float WalkBound(const FastBVH &bvh, float t) { return fma(t, bvh.tieRel, bvh.absBand); }
// a candidate hit at t: clearly nearer -> new best (an older mark is dropped: those candidates lie beyond);
// within the band of the best -> keep the nearer one, mark the ray
// PAIRS (the kernels of scenes with quadrics / patches / curves): the band of a comparison is the wide one when the candidate or the best
// hit so far is such a shape — or when the ray is already marked: a mark may stand for a general shape seen earlier whose t lies within
// the wide band of the candidate, and it must not be dropped by a triangle that is nearer by the narrow band only
template <bool PAIRS = false>
__device__ inline float WalkTestBound(const FastBVH &bvh, const RayWalk &w, bool candGeneral) {
    const float cur = __builtin_fabsf(w.tMax);
    if constexpr (PAIRS)
        if (!(candGeneral || w.prim >= bvh.firstGeneral || WalkAmbiguous(w))) return fma(cur, bvh.tieRelTri, bvh.absBandTri);
    return WalkBound(bvh, cur);
}
template <bool PAIRS = false>
__device__ inline bool WalkAccept(const FastBVH &bvh, RayWalk &w, float t, bool candGeneral = false) {
    const float cur = __builtin_fabsf(w.tMax);
    float bt = WalkBound(bvh, t);
    if constexpr (PAIRS)
        if (!(candGeneral || w.prim >= bvh.firstGeneral || WalkAmbiguous(w))) bt = fma(t, bvh.tieRelTri, bvh.absBandTri);
    if (bt < cur) { w.tMax = t; return true; }
    const bool nearer = t < cur;
    w.tMax = -(nearer ? t : cur);
    return nearer;
}

__device__ inline float CvtLo(uint32_t v) { return (float)(v & 0xffffu); }
__device__ inline float CvtHi(uint32_t v) { return (float)(v >> 16); }

// one child's slab test: entry t (lowest admissible), exit t
__device__ inline void ChildSlab(const RayWalk &w, uint32_t qx, uint32_t qy, uint32_t qz, float *tN, float *tF) {
    const uint32_t x = __builtin_amdgcn_perm(qx, qx, w.selx), y = __builtin_amdgcn_perm(qy, qy, w.sely), z = __builtin_amdgcn_perm(qz, qz, w.selz);
    const f2 X = __builtin_elementwise_fma(f2{CvtLo(x), CvtHi(x)}, f2{w.a.x, w.af.x}, f2{w.bn.x, w.bf.x});
    const f2 Y = __builtin_elementwise_fma(f2{CvtLo(y), CvtHi(y)}, f2{w.a.y, w.af.y}, f2{w.bn.y, w.bf.y});
    const f2 Z = __builtin_elementwise_fma(f2{CvtLo(z), CvtHi(z)}, f2{w.a.z, w.af.z}, f2{w.bn.z, w.bf.z});
    *tN = __builtin_fmaxf(__builtin_fmaxf(X.x, Y.x), Z.x);
    *tF = __builtin_fminf(__builtin_fminf(X.y, Y.y), Z.y);
}
__device__ inline void CSwap(float &ka, int &ra, float &kb, int &rb) {
    const bool s = kb < ka;
    const float k = s ? kb : ka, K = s ? ka : kb;
    const int r = s ? rb : ra, R = s ? ra : rb;
    ka = k; kb = K; ra = r; rb = R;
}
// Interior visit: branch-free test of the four children, nearest entry first.  n = the node's four 16-byte words.  Precondition: w.node >= 0.
// RELAX: prune against the near-tie band (closest hit); any-hit walks prune against the exact tMax (their result
// does not depend on the visiting order)
// (Measured and dropped, round 6: any-hit walks visiting the hit children in slot order without the sorting network; reserving room for
// the step's pushes with one ring-full test, 28.5 against 27.4 ms closest-hit.)
template <bool RELAX = true, typename Stack>
__device__ inline void InteriorStep(const FastBVH &bvh, RayWalk &w, Stack &st, const U4 *n) {
    const float tPrune = RELAX ? WalkBound(bvh, __builtin_fabsf(w.tMax)) : w.tMax;
    float k0, k1, k2, k3, e;
    ChildSlab(w, n[0].x, n[0].y, n[0].z, &k0, &e);
    const bool h0 = __builtin_fmaxf(k0, 0.f) <= __builtin_fminf(e, tPrune);
    ChildSlab(w, n[0].w, n[1].x, n[1].y, &k1, &e);
    const bool h1 = __builtin_fmaxf(k1, 0.f) <= __builtin_fminf(e, tPrune);
    ChildSlab(w, n[1].z, n[1].w, n[2].x, &k2, &e);
    const bool h2 = __builtin_fmaxf(k2, 0.f) <= __builtin_fminf(e, tPrune);
    ChildSlab(w, n[2].y, n[2].z, n[2].w, &k3, &e);
    const bool h3 = __builtin_fmaxf(k3, 0.f) <= __builtin_fminf(e, tPrune);
    k0 = h0 ? k0 : WF_INFINITY; k1 = h1 ? k1 : WF_INFINITY; k2 = h2 ? k2 : WF_INFINITY; k3 = h3 ? k3 : WF_INFINITY;
    int r0 = (int)n[3].x, r1 = (int)n[3].y, r2 = (int)n[3].z, r3 = (int)n[3].w;
    // nearest entry first: 5-comparator sorting network; missed children (key = inf) sink to the end
    CSwap(k0, r0, k1, r1); CSwap(k2, r2, k3, r3); CSwap(k0, r0, k2, r2); CSwap(k1, r1, k3, r3); CSwap(k1, r1, k2, r2);
    const int nh = (int)h0 + (int)h1 + (int)h2 + (int)h3;
    if (nh == 0) { w.node = st.empty() ? NODE_NONE : st.pop(); return; }
    if (nh > 3) st.push(r3);
    if (nh > 2) st.push(r2);
    if (nh > 1) st.push(r1);
    w.node = r0;
}
// Leaf: <= 16 triangle tests.  ANY: stop at the first hit.  Precondition: w.node < 0 && w.node != NODE_NONE.
// The general-primitive variants (ALPHA): leaf entries marked c.z == 2 are triangles whose mesh carries an alpha
// texture (ex.accept(prim, b0, b1, b2) decides), entries marked c.z == 3 are spheres (ex.sphere(prim, tMax, &hit);
// the hit's pObj travels in b0..b2).  Scenes without either use the plain variants, which never see the marks.
// RayWalk::route bit: the walk met a leaf entry only the general-primitive kernels can test (a quadric / patch / curve: c.z == 3) and
// stopped — the ray is walked again by those kernels (round 6, wf_backend.hip "TWO-CLASS TRAVERSAL").  Extra::deferGeneral selects it.
constexpr uint32_t WALK_DEFER = 0x40000000u;
struct NoExtra {
    static constexpr bool pairBands = false;
    static constexpr bool deferGeneral = false;
    __device__ bool accept(int, float, float, float) const { return true; }
    __device__ bool sphere(int, float, QuadricHit *) const { return false; }
};
template <bool ANY, bool ALPHA = false, bool INST = false, typename Stack, typename Extra = NoExtra>
__device__ inline void LeafStep(const FastBVH &bvh, RayWalk &w, Stack &st, const Extra &ex = Extra()) {
    unsigned ref = ~(unsigned)w.node;
    int first = (int)(ref >> 4), count = (int)(ref & 15u) + 1;
    bool done = false;
    for (int i = 0; i < count; ++i) {
        const LeafTri *lt = bvh.tris + first + i;
        const F4 ta = lt->a, tb = lt->b, tc = lt->c;
        TriHit h;
        if constexpr (INST)
            if (tc.z == 4.f) {  // an object instance: visited through the stack (the main loop enters it when it is popped)
                st.push((int)~(((unsigned)INST_FIRST + FloatToBits(tc.y)) << 4));
                continue;
            }
        if constexpr (Extra::deferGeneral)
            if (tc.z == 3.f) { w.route |= WALK_DEFER; done = true; break; }
        // closest hit: test against the relaxed bound so that near-ties are seen (WalkAccept sorts them out)
        constexpr bool PAIRS = Extra::pairBands;
        if constexpr (ALPHA)
            if (tc.z == 3.f) {
                const float tTest = ANY ? w.tMax : WalkBound(bvh, __builtin_fabsf(w.tMax));
                QuadricHit qh;
                // (closest hit: against the RELAXED bound, like the triangles below — a quadric whose t lies inside the near-tie band of
                //  the current best must reach WalkAccept to mark the ray; tested against the exact bound, the second of two coincident
                //  quadrics was silently dropped and the visiting order decided: fuzz finding s200010 on the GPU, round 4)
                if (ex.sphere((int)FloatToBits(tc.y), tTest, &qh)) {
                    if (ANY) { w.prim = (int)FloatToBits(tc.y); w.tMax = qh.tHit; done = true; break; }
                    if (WalkAccept<PAIRS>(bvh, w, qh.tHit, true)) {
                        w.prim = (int)FloatToBits(tc.y);
                        w.inst = w.curInst;
                        w.route = FloatToBits(tc.w);
                        w.b0 = qh.pObj.x; w.b1 = qh.pObj.y; w.b2 = qh.pObj.z;
                    }
                }
                continue;
            }
        const float tTest = ANY ? w.tMax : WalkTestBound<PAIRS>(bvh, w, false);
        if ((ALPHA ? tc.z != 1.f : tc.z == 0.f) &&
            IntersectTriangleSheared(w.o, w.sh, tTest, V3{ta.x, ta.y, ta.z}, V3{ta.w, tb.x, tb.y}, V3{tb.z, tb.w, tc.x}, &h, false)) {
            if constexpr (ALPHA)
                if (tc.z == 2.f && !ex.accept((int)FloatToBits(tc.y), h.b0, h.b1, h.b2)) continue;
            if (ANY) { w.prim = (int)FloatToBits(tc.y); w.tMax = h.t; done = true; break; }
            if (WalkAccept<PAIRS>(bvh, w, h.t, false)) {
                w.prim = (int)FloatToBits(tc.y);
                w.inst = w.curInst;
                w.route = FloatToBits(tc.w);
                w.b0 = h.b0; w.b1 = h.b1; w.b2 = h.b2;
            }
        }
    }
    w.node = (done || st.empty()) ? NODE_NONE : st.pop();
}

}  // namespace wf
