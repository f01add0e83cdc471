// wf_fastbvh.h — the records of the production traversal layout (QNode / LeafTri / FastDef / SubEntry behind a FastBVH header) and the
// constants that size the traversal stacks.  Plain data, no device code: the walk kernels (hip/wf_traverse.h, hip/wf_backend.hip) read
// these records and the host-only tree builder and scene planner (hip/wf_fastbvh_build.cpp, hip/wf_plan.cpp) write and size them, so the
// layout is pinned here, once, for both sides.  How the walk uses the layout: the head of hip/wf_traverse.h.
#pragma once
#include "wf_kernels.h"

namespace wf {

// four children per node (64-byte nodes, half the dependent fetches per ray: measured -10 % closest-hit and shadow time on both the
// 30 k-triangle and the 10 M-triangle instanced scene against the two-child layout of round 1)
struct alignas(16) QNode {
    // q[3c + a]: child c, axis a: min plane (low half) | max plane << 16 on the 16-bit grid of the tree (plane = base + q * cell,
    // with build-time outward margins); an empty slot has min > max on every axis (never hit)
    uint32_t q[12];
    int32_t child[4];  // >= 0: interior QNode index; < 0: leaf ~((first << 4) | (count - 1))
};
constexpr int QNODE_U4 = 4;
struct alignas(16) LeafTri {
    F4 a;  // p0.xyz, p1.x
    F4 b;  // p1.yz, p2.xy
    F4 c;  // p2.z, triangle id (int bits), 1.0 if the triangle is degenerate (zero-length normal) else 0, routing code (int bits)
};
struct alignas(16) U4 { uint32_t x, y, z, w; };

constexpr int NODE_NONE = (int)0x80000000;
#ifndef WF_TBLOCK
#define WF_TBLOCK 256
#endif
#ifndef WF_TSTACK
#define WF_TSTACK 16   // a power of two: the LDS part of the stack is a ring (LdsStackT)
#endif
constexpr int TBLOCK = WF_TBLOCK;        // threads per workgroup of the traversal kernels
constexpr int TSTACK = WF_TSTACK;        // LDS stack entries per lane (x 4 B x TBLOCK)
// ... and of the reference-order walks (wf_backend.hip: workgroups of 256 lanes); PlanScene sizes the spill rows behind both
constexpr int STACK_LDS = 24;   // LDS stack entries per lane: 24 x 4 B x 256 lanes = 24 KiB per workgroup
constexpr int STACK_MAX = 64;   // nodesToVisit[64], cpu/aggregates.cpp:538

struct FastBVH {
    const QNode *nodes;
    const LeafTri *tris;
    int nNodes;
    float base[3], cell[3];  // grid: plane(q) = base + q * cell (real arithmetic; the builder keeps a margin, see BuildFastBVH)
    float absBand;           // 2^-20 x the scene extent: absolute part of the near-tie band
    // relative part of the band (1 + 2^-20).  Scenes with quadrics / patches / curves use 2^-10 for both parts (round 4): those shapes
    // accept a hit when the UPPER BOUND of its interval-arithmetic t is <= tMax (shapes.h:147-233: Sphere::BasicIntersect and
    // friends), so two candidates closer than the interval's width — 10^-5 t and more, far outside the triangles' 2^-20 — are
    // decided by the visiting order: of two coincident cylinders the reference keeps the FIRST, this walk kept whichever its own
    // order met first and never marked the ray (fuzz finding s200010 on the GPU: 7 % of the pixels)
    float tieRel;
    // ... but only a pair of candidates that INVOLVES such a shape needs the wide band (round 4, second step): two triangles are ordered
    // by their exact t on both sides, 2^-20 decides.  With the wide band applied to every pair the 10 M-triangle scene plus ONE sphere
    // marked so many rays that the re-trace launches took 162 ms of a 358 ms frame.  tieRelTri / absBandTri: the triangles' own band;
    // firstGeneral: the first primitive id that is not a triangle (INT_MAX without such shapes; then both bands are the same).
    float tieRelTri, absBandTri;
    int firstGeneral;
    const struct FastDef *defs;       // per instance definition (scenes with object instances)
    const struct SubEntry *subs;      // the instance entries of the top-level tree (round 6: partial re-braiding, see SubEntry)
    const wf_instance *instances;
    const SceneView *sv;              // device-resident copy of the scene view, for the out-of-line general-primitive callbacks
};
struct FastDef {
    int root;                // QNode index of the definition's root
    float base[3], cell[3];  // its quantisation grid
    int pad;
};
// An ENTRY of the top-level tree into an object instance (round 6).  Until round 5 an instance was one leaf entry of the top-level tree,
// bounded by one box, and its walk started at the definition's root: on the spec scene a ray entered eight instances and six of the
// visits ended without a primitive test — the box of a cluster of objects is mostly empty, and every visit pays the reference's
// interval-arithmetic ray transform twice (in and out).  PARTIAL RE-BRAIDING (Benthin, Woop, Wald, Afra: "Improved two-level BVHs using
// partial re-braiding", HPG 2017): the top-level tree is built over the instances OPENED a few levels into their definitions' trees —
// an entry is (instance, node of the definition's production tree), bounded by the box of that subtree's transformed vertices — so
// the top-level tree separates the objects of a cluster, and a ray changes spaces only for subtrees whose own box it meets.  The walk
// inside is the same; only its starting node differs.  Which triangles can be reached is a superset of the reference's hits as
// before (the exact triangle test decides, near ties are re-walked in the reference's order).
struct SubEntry {
    int inst;   // wf_instance index
    int node;   // where the walk starts in the definition's production tree: QNode index (>= 0) or a leaf reference (< 0)
};
constexpr int INST_FIRST = 1 << 26;          // leaf references with first >= INST_FIRST: instance entry (first - INST_FIRST) of FastBVH::subs
constexpr int NODE_EXIT = (int)0x80000001;   // stack marker: leave the instance (the world tMax is the entry below it)
constexpr int INST_STALE = 1 << 30;          // RayWalk::inst flag while its instance is being re-visited (EnterInstance)

// the two units that share these records (device walks, host builder) agree on their sizes
static_assert(sizeof(QNode) == 64, "QNode");
static_assert(sizeof(LeafTri) == 48, "LeafTri");
static_assert(sizeof(FastDef) == 32, "FastDef");
static_assert(sizeof(SubEntry) == 8, "SubEntry");

// A leaf reference (QNode::child < 0, SubEntry::node < 0): the run of `count` (1..16) LeafTri records from `first`, or — first >= INST_FIRST —
// the instance entry first - INST_FIRST
inline int LeafRef(int first, int count) { return (int)~(((unsigned)first << 4) | (unsigned)(count - 1)); }
inline void LeafRun(int ref, int *first, int *count) {
    const unsigned r = ~(unsigned)ref;
    *first = (int)(r >> 4);
    *count = (int)(r & 15u) + 1;
}

}  // namespace wf
