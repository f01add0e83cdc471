// wf_fastbvh_build.cpp — the builder of the production traversal layout (BuildFastBVH: the records of common/wf_fastbvh.h from the
// description's reference-layout trees) and its host-only self-check (wf_debug_fastbvh_check).  Plain C++: no HIP header, no device.
#include <array>
#include <climits>
#include <cstdio>
#include <atomic>
#include <thread>
#include <utility>
#include "wf_plan.h"

using namespace wf;
using namespace wf::planning;

// ---- the top-level tree of a two-level scene, rebuilt over RE-BRAIDED instances (round 6; SubEntry in wf_fastbvh.h) ----
// One primitive of the builder: a top-level triangle / quadric (its LeafTri record of the scene's leaf order) or an instance entry.
namespace {
struct TopPrim {
    float b[6];
    int kind;   // 0: the LeafTri record `idx` of the reference's leaf order; 1: instance entry `idx` (FastBVH::subs)
    int idx;
};
// Binned SAH (16 bins on the axis of the largest centroid extent, the reference's cost model: cpu/aggregates.cpp:270-370 — this tree is
// the production walk's own, nothing is pinned to it), written as reference-layout nodes (depth first: left child = i + 1, right child =
// offset) so that the four-wide collapse and the quantisation below take it like a reference tree.  A leaf holds at most four LeafTri
// records; an instance entry is always a leaf of its own, referenced by the node itself (offset = INST_FIRST + entry: the walk pops
// the entry without a LeafTri fetch).  `order` receives the primitives in leaf order.
struct TopTreeBuilder {
    std::vector<TopPrim> &P;
    std::vector<wf_bvh_node> &out;
    int leafBase;   // LeafTri index of P[0] in the new leaf order
    static double Area(const float b[6]) {
        const double dx = (double)b[3] - b[0], dy = (double)b[4] - b[1], dz = (double)b[5] - b[2];
        return dx * dy + dy * dz + dz * dx;
    }
    int Build(int lo, int hi) {
        const int me = (int)out.size();
        out.emplace_back();
        float bb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY}, cb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
        bool anyEntry = false;
        for (int i = lo; i < hi; ++i) {
            const TopPrim &p = P[i];
            anyEntry = anyEntry || p.kind == 1;
            for (int a = 0; a < 3; ++a) {
                bb[a] = std::min(bb[a], p.b[a]); bb[3 + a] = std::max(bb[3 + a], p.b[3 + a]);
                const float c = 0.5f * p.b[a] + 0.5f * p.b[3 + a];
                cb[a] = std::min(cb[a], c); cb[3 + a] = std::max(cb[3 + a], c);
            }
        }
        const int count = hi - lo;
        auto makeLeaf = [&]() {
            wf_bvh_node &nd = out[me];
            for (int a = 0; a < 3; ++a) { nd.bmin[a] = bb[a]; nd.bmax[a] = bb[3 + a]; }
            nd.axis = 0; nd.pad = 0;
            nd.nprims = (uint16_t)count;
            nd.offset = (count == 1 && P[lo].kind == 1) ? INST_FIRST + P[lo].idx : leafBase + lo;
            return me;
        };
        if (count == 1) return makeLeaf();
        int axis = 0;
        for (int a = 1; a < 3; ++a) if (cb[3 + a] - cb[a] > cb[3 + axis] - cb[axis]) axis = a;
        int mid = (lo + hi) / 2;
        const float cmin = cb[axis], cext = cb[3 + axis] - cb[axis];
        bool split = false;
        if (cext > 0) {
            constexpr int NB = 16;
            int cnt[NB] = {};
            float bbox[NB][6];
            for (int k = 0; k < NB; ++k) for (int a = 0; a < 3; ++a) { bbox[k][a] = INFINITY; bbox[k][3 + a] = -INFINITY; }
            auto binOf = [&](const TopPrim &p) {
                const float c = 0.5f * p.b[axis] + 0.5f * p.b[3 + axis];
                int k = (int)(NB * ((c - cmin) / cext));
                return k < 0 ? 0 : (k >= NB ? NB - 1 : k);
            };
            for (int i = lo; i < hi; ++i) {
                const int k = binOf(P[i]);
                ++cnt[k];
                for (int a = 0; a < 3; ++a) { bbox[k][a] = std::min(bbox[k][a], P[i].b[a]); bbox[k][3 + a] = std::max(bbox[k][3 + a], P[i].b[3 + a]); }
            }
            double costR[NB] = {};
            {
                float r[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
                int c = 0;
                for (int k = NB - 1; k >= 1; --k) {
                    if (cnt[k]) for (int a = 0; a < 3; ++a) { r[a] = std::min(r[a], bbox[k][a]); r[3 + a] = std::max(r[3 + a], bbox[k][3 + a]); }
                    c += cnt[k];
                    costR[k] = c ? c * Area(r) : 0;
                }
            }
            float l[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
            int c = 0, best = -1;
            double bestCost = 0;
            for (int k = 0; k + 1 < NB; ++k) {
                if (cnt[k]) for (int a = 0; a < 3; ++a) { l[a] = std::min(l[a], bbox[k][a]); l[3 + a] = std::max(l[3 + a], bbox[k][3 + a]); }
                c += cnt[k];
                if (c == 0 || c == count) continue;
                const double cost = c * Area(l) + costR[k + 1];
                if (best < 0 || cost < bestCost) { best = k; bestCost = cost; }
            }
            if (best >= 0) {
                const double area = Area(bb);
                const double minCost = 0.5 + (area > 0 ? bestCost / area : 0);
                if (count <= 4 && !anyEntry && !(minCost < count)) return makeLeaf();
                TopPrim *m = std::partition(P.data() + lo, P.data() + hi, [&](const TopPrim &p) { return binOf(p) <= best; });
                mid = (int)(m - P.data());
                split = mid > lo && mid < hi;
            }
        }
        if (!split) {
            // coincident centroids: up to four records share a leaf, more (or any instance entry) are dealt half and half
            if (count <= 4 && !anyEntry) return makeLeaf();
            mid = (lo + hi) / 2;
        }
        Build(lo, mid);
        const int right = Build(mid, hi);
        wf_bvh_node &nd = out[me];
        for (int a = 0; a < 3; ++a) { nd.bmin[a] = bb[a]; nd.bmax[a] = bb[3 + a]; }
        nd.axis = (uint8_t)axis; nd.pad = 0;
        nd.nprims = 0;
        nd.offset = right;
        return me;
    }
};
// [lo, hi] widened by 2^-18 of the magnitudes involved plus 2^-19 of the scene's, rounded outward to floats; false: not finite
bool PaddedBox(const double lo[3], const double hi[3], double mag, double sceneMag, float b[6]) {
    bool finite = true;
    for (int a = 0; a < 3; ++a) {
        const double pad = 0x1p-18 * (mag + (hi[a] - lo[a])) + 0x1p-19 * sceneMag + 1e-30;
        b[a] = (float)(lo[a] - pad); b[3 + a] = (float)(hi[a] + pad);
        if (!((double)b[a] <= lo[a] - 0.5 * pad)) b[a] = NextFloatDown(b[a]);
        if (!((double)b[3 + a] >= hi[a] + 0.5 * pad)) b[3 + a] = NextFloatUp(b[3 + a]);
        finite = finite && std::isfinite(b[a]) && std::isfinite(b[3 + a]);
    }
    return finite;
}
}  // namespace

// Reference LinearBVHNode arrays (depth-first: left child = i + 1, right child = offset) -> QNode (breadth-first
// numbering per tree, quantised child boxes on the tree's own grid) + LeafTri (vertices in leaf order).  The top-level
// tree comes first; every instance definition's tree follows with its own grid (FastDef).  How the walk reads them: wf_traverse.h.
bool wf::planning::BuildFastBVH(const wf_scene_desc *d, const Switches &sw, FastTrees *trees, FastDepths *depths) {
    std::vector<QNode> *nodes = &trees->nodes;
    std::vector<LeafTri> *tris = &trees->tris;
    std::vector<FastDef> *defs = &trees->defs;
    std::vector<SubEntry> *subs = &trees->subs;
    FastBVH *out = &trees->header;
    const wf_bvh_node *L = d->bvh_nodes;   // (rebound to the extended array once the re-braided top-level tree has been appended)
    int n = d->n_bvh_nodes;
    const int nRef = n;                    // nodes of the reference's trees
    const int nGeom = d->n_triangles + d->n_quadrics;
    const int nPrims = (int)BvhPrimCount(d);    // entries of bvh_prims: every triangle / quadric once, every instance once (no nested placements here: below)
    if (n == 0 || (size_t)nPrims >= (size_t)INST_FIRST || d->n_instances >= INST_FIRST) return false;
    for (int i = 0; i < n; ++i)
        if (L[i].nprims > 16) return false;
    // nested placements (animated shapes inside instance definitions, wf_abi.h wf_instance) have no entry form in the production tree: such
    // scenes keep the reference-order walks, which take the third level from BVHIntersectClosestDef / BVHIntersectAnyDef<ANIM>
    if (NestedPlacements(d) > 0) return false;
    tris->resize((size_t)nPrims);
    for (int k = 0; k < nPrims; ++k) {
        int t = d->bvh_prims[k];
        if (t >= nGeom) {
            // an object instance: c.z == 4, entered by the INST kernel variants
            LeafTri lt;
            lt.a = F4{0, 0, 0, 0};
            lt.b = F4{0, 0, 0, 0};
            lt.c = F4{0, BitsToFloat((uint32_t)(t - nGeom)), 4.f, BitsToFloat(0u)};
            (*tris)[k] = lt;
            continue;
        }
        if (t >= d->n_triangles) {
            // a sphere: c.z == 3, tested by the general-primitive kernel variants from wf_quadric (object space)
            const wf_mesh &mesh = d->meshes[d->tri_mesh[t]];
            uint32_t route = mesh.material >= 0 ? (uint32_t)d->materials[mesh.material].type | (mesh.first_light >= 0 ? 16u : 0u) : 32u;
            LeafTri lt;
            lt.a = F4{0, 0, 0, 0};
            lt.b = F4{0, 0, 0, 0};
            lt.c = F4{0, BitsToFloat((uint32_t)t), 3.f, BitsToFloat(route)};
            (*tris)[k] = lt;
            continue;
        }
        const int32_t *v = d->tri_indices + 3 * (size_t)t;
        const float *p0 = d->P + 3 * (size_t)v[0], *p1 = d->P + 3 * (size_t)v[1], *p2 = d->P + 3 * (size_t)v[2];
        LeafTri lt;
        lt.a = F4{p0[0], p0[1], p0[2], p1[0]};
        lt.b = F4{p1[1], p1[2], p2[0], p2[1]};
        // IntersectTriangle's first test (shapes.cpp:172-173), hoisted to build time
        V3 q0{p0[0], p0[1], p0[2]}, q1{p1[0], p1[1], p1[2]}, q2{p2[0], p2[1], p2[2]};
        bool degenerate = LengthSquared(Cross(q2 - q0, q1 - q0)) == 0;
        // routing code of EnqueueWorkAfterIntersection (intersect.h:48-156), so that the traversal kernel needs no
        // per-hit mesh / material gathers: material type | emissive << 4 | interface << 5
        const wf_mesh &mesh = d->meshes[d->tri_mesh[t]];
        uint32_t route = 0;
        if (mesh.material >= 0) route = (uint32_t)d->materials[mesh.material].type | (mesh.first_light >= 0 ? 16u : 0u);
        else route = 32u;
        // c.z: 0 = test, 1 = degenerate (never hit), 2 = test, then the mesh's alpha texture decides (ALPHA kernel variants)
        lt.c = F4{p2[2], BitsToFloat((uint32_t)t), degenerate ? 1.f : mesh.alpha_tex >= 0 ? 2.f : 0.f, BitsToFloat(route)};
        (*tris)[k] = lt;
    }
    nodes->clear();
    bool gridOk = true;
    std::vector<int> bfsIndex(n, -1);
    // Subtree collapse: the production tree need not mirror the reference's leaves — a reference subtree holding at most
    // `collapse` primitives (contiguous in bvh_prims: leaf order is depth-first) becomes ONE leaf here.  The walk then tests
    // a superset of the triangles the reference tests, which changes no result (the exact triangle test decides, near-ties
    // are re-traced in reference order) and removes the bottom levels of dependent node fetches: instance definitions are
    // built with one primitive per leaf (maxPrimsInNode = 1, scene.cpp:1539).
    const int collapse = sw.leafCollapse;
    std::vector<int> subFirst(n), subCount(n);
    auto fillSubRanges = [&](int from, int to) {   // nodes [from, to): a complete set of depth-first trees
        for (int i = to - 1; i >= from; --i) {
            if (L[i].nprims > 0) { subFirst[i] = L[i].offset; subCount[i] = L[i].nprims; }
            else { subFirst[i] = subFirst[i + 1]; subCount[i] = subCount[i + 1] + subCount[L[i].offset]; }
        }
    };
    fillSubRanges(0, n);
    auto leafLike = [&](int i) { return L[i].nprims > 0 || subCount[i] <= collapse; };
    auto leafRef = [&](int i) { return LeafRef(subFirst[i], subCount[i]); };
    // TIGHT INSTANCE BOXES (round 5).  The reference bounds an instance by the box of the eight transformed corners of its definition's
    // box (TransformedPrimitive::Bounds) — for a rotated definition up to three times the surface area of the box of the transformed
    // GEOMETRY — and the spec scene's rays entered eight instances each, three of four visits without a single primitive test.  The
    // production walk only has to visit a superset of what can be hit, so its top-level tree carries, for an instance of an all-triangle
    // definition, the box of the definition's transformed vertices (widened by 2^-18 of the magnitudes involved: the transform's rounding
    // and the instance-space ray's), clipped to the reference's box, and interior boxes re-united bottom-up.  Topology, leaves and the
    // reference-layout nodes (counting kernels, near-tie re-walk, CPU checker) are untouched: same hits, fewer entries.  WF_TIGHT_INSTANCES=0: off.
    // WF_BRAID = most entries one instance is opened into (round 6, SubEntry in wf_fastbvh.h; 0: one entry per instance in the reference's
    // own top-level tree, as in round 5)
    const int braidMax = sw.braidMax;
    const bool braid = braidMax > 0 && d->n_instances > 0 && d->n_top_bvh_nodes > 0 && L[0].nprims == 0;
    std::vector<wf_bvh_node> tightTop;
    if (!braid && d->n_instances > 0 && d->n_top_bvh_nodes > 0 && sw.tightInstances) {
        const int nTop = d->n_top_bvh_nodes;
        std::vector<std::vector<int32_t>> defVerts((size_t)d->n_instance_defs);
        std::vector<char> defGeneral((size_t)d->n_instance_defs, 0);
        for (int k = 0; k < d->n_instance_defs; ++k) {
            const wf_instance_def &def = d->instance_defs[k];
            std::vector<int32_t> &v = defVerts[k];
            for (int j = def.first_prim; j < def.first_prim + def.n_prims; ++j) {
                const int t = d->bvh_prims[j];
                if (t >= d->n_triangles) { defGeneral[k] = 1; break; }
                const int32_t *ix = d->tri_indices + 3 * (size_t)t;
                v.push_back(ix[0]); v.push_back(ix[1]); v.push_back(ix[2]);
            }
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
            if (v.empty()) defGeneral[k] = 1;
        }
        std::vector<std::array<float, 6>> ib((size_t)d->n_instances);
        std::vector<char> ibOk((size_t)d->n_instances, 0);
        // (the pad also carries 2^-19 of the SCENE's magnitude, like the re-braided entries' boxes below: the instance-space ray the
        //  reference decides hits with carries the rounding of the render-space origin and of the distance travelled — ADVICE r5)
        double sceneMagT = 0;
        for (int a = 0; a < 3; ++a) sceneMagT = std::max(sceneMagT, std::max(std::fabs((double)L[0].bmin[a]), std::fabs((double)L[0].bmax[a])) + ((double)L[0].bmax[a] - L[0].bmin[a]));
        for (int i = 0; i < d->n_instances; ++i) {
            const wf_instance &in = d->instances[i];
            if (defGeneral[in.def] || in.anim_plus1 != 0) continue;   // (an AnimatedPrimitive keeps the reference's motion bounds)
            const float(*m)[4] = in.render_from_instance.m;
            if (m[3][0] != 0 || m[3][1] != 0 || m[3][2] != 0 || m[3][3] != 1) continue;
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, mag = 0;
            for (int32_t vi : defVerts[in.def]) {
                const float *pp = d->P + 3 * (size_t)vi;
                for (int a = 0; a < 3; ++a) {
                    const double c = (double)m[a][0] * pp[0] + (double)m[a][1] * pp[1] + (double)m[a][2] * pp[2] + (double)m[a][3];
                    lo[a] = std::min(lo[a], c); hi[a] = std::max(hi[a], c);
                    mag = std::max(mag, std::fabs((double)m[a][0] * pp[0]) + std::fabs((double)m[a][1] * pp[1]) + std::fabs((double)m[a][2] * pp[2]) + std::fabs((double)m[a][3]));
                }
            }
            ibOk[i] = PaddedBox(lo, hi, mag, sceneMagT, ib[i].data());
        }
        tightTop.assign(L, L + nTop);
        for (int i = nTop - 1; i >= 0; --i) {
            wf_bvh_node &t = tightTop[i];
            float b[6];
            bool have = false, keep = false;
            if (L[i].nprims > 0) {
                for (int j = L[i].offset; j < L[i].offset + L[i].nprims && !keep; ++j) {
                    const int pr = d->bvh_prims[j];
                    if (pr < nGeom || !ibOk[pr - nGeom]) { keep = true; break; }   // a triangle / quadric or an instance left alone: the reference's box stands
                    const std::array<float, 6> &q = ib[pr - nGeom];
                    if (!have) { for (int a = 0; a < 6; ++a) b[a] = q[a]; have = true; }
                    else for (int a = 0; a < 3; ++a) { b[a] = std::min(b[a], q[a]); b[3 + a] = std::max(b[3 + a], q[3 + a]); }
                }
            } else {
                const wf_bvh_node &c0 = tightTop[i + 1], &c1 = tightTop[L[i].offset];
                for (int a = 0; a < 3; ++a) { b[a] = std::min(c0.bmin[a], c1.bmin[a]); b[3 + a] = std::max(c0.bmax[a], c1.bmax[a]); }
                have = true;
            }
            if (keep || !have) continue;
            for (int a = 0; a < 3; ++a) {   // clipped to the reference's box (the geometry lies in both)
                t.bmin[a] = std::max(L[i].bmin[a], b[a]);
                t.bmax[a] = std::min(L[i].bmax[a], b[3 + a]);
                if (!(t.bmin[a] <= t.bmax[a])) { t.bmin[a] = L[i].bmin[a]; t.bmax[a] = L[i].bmax[a]; }
            }
        }
    }
    // the boxes the production tree is packed from: the tightened ones for the top-level tree, the reference's everywhere else
    auto BoxOf = [&](int i) -> const wf_bvh_node & { return (!tightTop.empty() && i < (int)tightTop.size()) ? tightTop[i] : L[i]; };
    // one tree: linear nodes [root, ...) reachable from root; grid written to base / cell; returns the root's QNode index
    int lastTreeDepth = 0;   // levels of the four-wide tree buildTree made last (a single leaf-like root: 1)
    std::vector<std::array<int, 4>> qKids;   // per QNode: the reference-layout nodes its four children stand for (-1: empty slot)
    auto buildTree = [&](int root, float baseOut[3], float cellOut[3]) -> int {
        lastTreeDepth = 1;
        // Quantisation grid over the root bounds.  A plane is the REAL number base + q * cell (the device never forms
        // it as a float: WalkSetRay folds base and cell into per-ray fma constants).  Every stored plane lies at least
        // `margin` outside the float box it bounds; margin = 2^-20 of the largest coordinate magnitude, which covers the
        // rounding of (base - o) and of the box's own float planes in the reference's slab test.
        double margin[3];
        for (int a = 0; a < 3; ++a) {
            double lo = L[root].bmin[a], hi = L[root].bmax[a];
            double ext = hi - lo;
            margin[a] = 0x1p-20 * (std::max(std::fabs(lo), std::fabs(hi)) + ext) + 1e-37;
            float base = (float)(lo - 2 * margin[a]);
            while ((double)base > lo - 2 * margin[a]) base = NextFloatDown(base);
            float cell = (float)((hi + 2 * margin[a] - (double)base) / 65535.0);
            if (!(cell > 0)) cell = 1e-30f;
            cell = NextFloatUp(NextFloatUp(cell));
            baseOut[a] = base;
            cellOut[a] = cell;
        }
        auto plane = [&](int q, int a) { return (double)baseOut[a] + (double)q * (double)cellOut[a]; };
        auto qlo = [&](float v, int a) {
            double target = (double)v - margin[a];
            int q = (int)std::floor((target - baseOut[a]) / cellOut[a]);
            q = std::min(std::max(q, 0), 65535);
            while (q > 0 && plane(q, a) > target) --q;
            if (plane(q, a) > target) gridOk = false;
            return (uint32_t)q;
        };
        auto qhi = [&](float v, int a) {
            double target = (double)v + margin[a];
            int q = (int)std::ceil((target - baseOut[a]) / cellOut[a]);
            q = std::min(std::max(q, 0), 65535);
            while (q < 65535 && plane(q, a) < target) ++q;
            if (plane(q, a) < target) gridOk = false;
            return (uint32_t)q;
        };
        const int qBase = (int)nodes->size();
        auto emptyBox = [&](uint32_t q[12], int slot) { for (int a = 0; a < 3; ++a) q[slot * 3 + a] = 0x0000ffffu; };
        auto area = [&](int i) {
            const wf_bvh_node &bx = BoxOf(i);
            double dx = (double)bx.bmax[0] - bx.bmin[0], dy = (double)bx.bmax[1] - bx.bmin[1], dz = (double)bx.bmax[2] - bx.bmin[2];
            return dx * dy + dy * dz + dz * dx;
        };
        auto packBox = [&](const wf_bvh_node &b, uint32_t q[12], int slot) {
            for (int a = 0; a < 3; ++a) q[slot * 3 + a] = qlo(b.bmin[a], a) | (qhi(b.bmax[a], a) << 16);
        };
        if (leafLike(root)) {
            QNode qn{};
            packBox(BoxOf(root), qn.q, 0);
            qn.child[0] = leafRef(root);
            for (int c = 1; c < 4; ++c) { emptyBox(qn.q, c); qn.child[c] = NODE_NONE; }
            nodes->push_back(qn);
            qKids.push_back({root, -1, -1, -1});
            return qBase;
        }
        // four-way collapse of the binary tree: a node's children are its two binary children, the largest interior ones
        // replaced by their own children until there are four (or only leaves are left); breadth-first numbering
        std::vector<int> order;
        order.push_back(root);
        bfsIndex[root] = qBase;
        std::vector<std::array<int, 4>> kidsOf;
        std::vector<int> level{1};
        for (size_t h = 0; h < order.size(); ++h) {
            int i = order[h];
            lastTreeDepth = std::max(lastTreeDepth, level[h] + 1);   // + 1: the leaves hanging off this node
            std::array<int, 4> kids = {i + 1, (int)L[i].offset, -1, -1};
            int nk = 2;
            while (nk < 4) {
                int best = -1;
                for (int k = 0; k < nk; ++k)
                    if (!leafLike(kids[k]) && (best < 0 || area(kids[k]) > area(kids[best]))) best = k;
                if (best < 0) break;
                int c = kids[best];
                kids[best] = c + 1;
                kids[nk++] = L[c].offset;
            }
            for (int k = 0; k < nk; ++k)
                if (!leafLike(kids[k])) { bfsIndex[kids[k]] = qBase + (int)order.size(); order.push_back(kids[k]); level.push_back(level[h] + 1); }
            kidsOf.push_back(kids);
        }
        nodes->resize((size_t)qBase + order.size());
        qKids.insert(qKids.end(), kidsOf.begin(), kidsOf.end());
        for (size_t h = 0; h < order.size(); ++h) {
            QNode qn{};
            for (int c = 0; c < 4; ++c) {
                int k = kidsOf[h][c];
                if (k < 0) { emptyBox(qn.q, c); qn.child[c] = NODE_NONE; continue; }
                packBox(BoxOf(k), qn.q, c);
                qn.child[c] = !leafLike(k) ? bfsIndex[k] : leafRef(k);
            }
            (*nodes)[(size_t)qBase + h] = qn;
        }
        return qBase;
    };
    // the definitions' trees first (the entries of the re-braided top-level tree name their nodes), then the top-level tree; afterwards
    // the top-level tree is moved to the FRONT of the array: the walk starts at node 0
    for (int i = 0; i < nRef; ++i)
        if (leafLike(i)) {
            int ni = 0;
            for (int k = 0; k < subCount[i]; ++k) ni += d->bvh_prims[subFirst[i] + k] >= nGeom;
            depths->maxLeafInstances = std::max(depths->maxLeafInstances, ni);
        }
    defs->clear();
    for (int k = 0; k < d->n_instance_defs; ++k) {
        FastDef fd{};
        fd.root = d->instance_defs[k].bvh_root >= 0 ? buildTree(d->instance_defs[k].bvh_root, fd.base, fd.cell) : -1;
        if (d->instance_defs[k].bvh_root >= 0) depths->def = std::max(depths->def, lastTreeDepth);
        defs->push_back(fd);
    }
    const int nDefQ = (int)nodes->size();
    subs->clear();
    std::vector<wf_bvh_node> Lx;
    int topRoot = 0;
    if (braid) {
        // ---- partial re-braiding: the entries of every instance
        const int nTop = d->n_top_bvh_nodes;
        std::vector<char> defGeneral((size_t)d->n_instance_defs, 0);
        for (int k = 0; k < d->n_instance_defs; ++k) {
            const wf_instance_def &def = d->instance_defs[k];
            if (def.bvh_root < 0 || def.n_prims <= 0) { defGeneral[k] = 1; continue; }
            for (int j = def.first_prim; j < def.first_prim + def.n_prims; ++j)
                if (d->bvh_prims[j] >= d->n_triangles) { defGeneral[k] = 1; break; }
        }
        double sceneMag = 0;
        for (int a = 0; a < 3; ++a) sceneMag = std::max(sceneMag, std::max(std::fabs((double)L[0].bmin[a]), std::fabs((double)L[0].bmax[a])) + ((double)L[0].bmax[a] - L[0].bmin[a]));
        struct Entry { int bnode; float b[6]; };
        std::vector<std::vector<Entry>> entriesOf((size_t)d->n_instances);
        // the box of a definition's subtree under an instance's transformation: its triangles' transformed vertices (double arithmetic),
        // widened by 2^-18 of the magnitudes involved plus 2^-19 of the SCENE's (the instance-space ray the reference decides hits with
        // carries the rounding of the render-space ray's origin and of the distance travelled — ADVICE r5: not of the instance's own
        // coordinates only)
        auto subtreeBox = [&](const wf_instance &in, int bnode, float b[6]) {
            const float(*m)[4] = in.render_from_instance.m;
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, mag = 0;
            for (int j = subFirst[bnode]; j < subFirst[bnode] + subCount[bnode]; ++j) {
                const LeafTri &lt = (*tris)[j];
                const float v[3][3] = {{lt.a.x, lt.a.y, lt.a.z}, {lt.a.w, lt.b.x, lt.b.y}, {lt.b.z, lt.b.w, lt.c.x}};
                for (int q = 0; q < 3; ++q)
                    for (int a = 0; a < 3; ++a) {
                        const double t0 = (double)m[a][0] * v[q][0], t1 = (double)m[a][1] * v[q][1], t2 = (double)m[a][2] * v[q][2];
                        const double c = t0 + t1 + t2 + (double)m[a][3];
                        lo[a] = std::min(lo[a], c); hi[a] = std::max(hi[a], c);
                        mag = std::max(mag, std::fabs(t0) + std::fabs(t1) + std::fabs(t2) + std::fabs((double)m[a][3]));
                    }
            }
            return PaddedBox(lo, hi, mag, sceneMag, b);
        };
        auto refOf = [&](int bnode) { return leafLike(bnode) ? leafRef(bnode) : bfsIndex[bnode]; };
        const double minFrac = sw.braidMinFrac;
        auto openInstance = [&](int i) {
            const wf_instance &in = d->instances[i];
            std::vector<Entry> &es = entriesOf[i];
            if (in.def < 0 || in.def >= d->n_instance_defs || defGeneral[in.def]) return;
            if (in.anim_plus1 != 0) return;   // an AnimatedPrimitive: one entry under the reference's motion bounds (its leaf's box)
            const float(*m)[4] = in.render_from_instance.m;
            if (m[3][0] != 0 || m[3][1] != 0 || m[3][2] != 0 || m[3][3] != 1) return;
            Entry root;
            root.bnode = d->instance_defs[in.def].bvh_root;
            if (!subtreeBox(in, root.bnode, root.b)) return;
            const double rootArea = TopTreeBuilder::Area(root.b);
            es.push_back(root);
            while ((int)es.size() < braidMax) {
                int best = -1;
                double bestArea = minFrac * rootArea;
                for (int k = 0; k < (int)es.size(); ++k) {
                    if (leafLike(es[k].bnode)) continue;
                    const double ar = TopTreeBuilder::Area(es[k].b);
                    if (ar > bestArea) { best = k; bestArea = ar; }
                }
                if (best < 0) break;
                const std::array<int, 4> &kids = qKids[(size_t)bfsIndex[es[best].bnode]];
                int nk = 0;
                for (int c = 0; c < 4; ++c) nk += kids[c] >= 0;
                if ((int)es.size() - 1 + nk > braidMax) break;
                Entry ch[4];
                bool ok = true;
                int w = 0;
                for (int c = 0; c < 4 && ok; ++c)
                    if (kids[c] >= 0) { ch[w].bnode = kids[c]; ok = subtreeBox(in, kids[c], ch[w].b); ++w; }
                if (!ok) break;
                es[best] = ch[0];
                for (int c = 1; c < w; ++c) es.push_back(ch[c]);
            }
        };
        {
            unsigned nThreads = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
            if ((unsigned)d->n_instances < 4 * nThreads) nThreads = 1;
            std::atomic<int> next{0};
            auto worker = [&]() { for (int i; (i = next.fetch_add(1)) < d->n_instances;) openInstance(i); };
            std::vector<std::thread> pool;
            for (unsigned t = 1; t < nThreads; ++t) pool.emplace_back(worker);
            worker();
            for (std::thread &t : pool) t.join();
        }
        // ---- the primitives of the new top-level tree, in the reference's leaf order (deterministic)
        std::vector<TopPrim> P;
        P.reserve((size_t)subCount[0] + (size_t)d->n_instances * 4);
        for (int i = 0; i < nTop; ++i) {
            if (L[i].nprims == 0) continue;
            for (int j = L[i].offset; j < L[i].offset + L[i].nprims; ++j) {
                const int t = d->bvh_prims[j];
                TopPrim p;
                if (t < d->n_triangles) {
                    const LeafTri &lt = (*tris)[j];
                    const float v[3][3] = {{lt.a.x, lt.a.y, lt.a.z}, {lt.a.w, lt.b.x, lt.b.y}, {lt.b.z, lt.b.w, lt.c.x}};
                    for (int a = 0; a < 3; ++a) { p.b[a] = std::min(v[0][a], std::min(v[1][a], v[2][a])); p.b[3 + a] = std::max(v[0][a], std::max(v[1][a], v[2][a])); }
                    p.kind = 0; p.idx = j;
                    P.push_back(p);
                } else if (t < nGeom) {   // a quadric / patch / curve: the reference's leaf box bounds it
                    for (int a = 0; a < 3; ++a) { p.b[a] = L[i].bmin[a]; p.b[3 + a] = L[i].bmax[a]; }
                    p.kind = 0; p.idx = j;
                    P.push_back(p);
                } else {
                    const int ii = t - nGeom;
                    const wf_instance &in = d->instances[ii];
                    if (entriesOf[ii].empty()) {   // left alone (general primitives inside, a projective matrix): one entry at the definition's root, the reference's leaf box
                        for (int a = 0; a < 3; ++a) { p.b[a] = L[i].bmin[a]; p.b[3 + a] = L[i].bmax[a]; }
                        p.kind = 1; p.idx = (int)subs->size();
                        const int root = (in.def >= 0 && in.def < d->n_instance_defs) ? d->instance_defs[in.def].bvh_root : -1;
                        subs->push_back(SubEntry{ii, root >= 0 ? refOf(root) : NODE_NONE});
                        P.push_back(p);
                    } else
                        for (const Entry &e : entriesOf[ii]) {
                            for (int a = 0; a < 6; ++a) p.b[a] = e.b[a];
                            p.kind = 1; p.idx = (int)subs->size();
                            subs->push_back(SubEntry{ii, refOf(e.bnode)});
                            P.push_back(p);
                        }
                }
            }
        }
        if (P.empty() || subs->size() >= (size_t)INST_FIRST) return false;
        // ---- the tree, as reference-layout nodes behind the reference's own
        const int leafBase = (int)tris->size();
        Lx.assign(L, L + n);
        TopTreeBuilder tb{P, Lx, leafBase};
        // (node indices of the builder are positions in Lx: it appends)
        topRoot = tb.Build(0, (int)P.size());
        tris->resize((size_t)leafBase + P.size());
        for (size_t k = 0; k < P.size(); ++k) {
            if (P[k].kind == 0) (*tris)[(size_t)leafBase + k] = (*tris)[(size_t)P[k].idx];
            else (*tris)[(size_t)leafBase + k].c = F4{0, BitsToFloat((uint32_t)P[k].idx), 4.f, BitsToFloat(0u)};   // (never read: an entry is a leaf of its own)
        }
        if (tris->size() >= (size_t)INST_FIRST) return false;
        L = Lx.data();
        n = (int)Lx.size();
        subFirst.resize(n); subCount.resize(n); bfsIndex.resize(n, -1);
        fillSubRanges(nRef, n);
        if (sw.braidVerbose) fprintf(stderr, "[wf] re-braided top-level tree: %d instances -> %zu entries, %zu primitives, %d nodes\n", d->n_instances, subs->size(), P.size(), n - nRef);
    } else {
        // one entry per instance, at its definition's root
        for (int i = 0; i < d->n_instances; ++i) {
            const int def = d->instances[i].def;
            const int root = (def >= 0 && def < d->n_instance_defs) ? d->instance_defs[def].bvh_root : -1;
            subs->push_back(SubEntry{i, root < 0 ? NODE_NONE : (leafLike(root) ? leafRef(root) : bfsIndex[root])});
        }
    }
    buildTree(topRoot, out->base, out->cell);
    depths->top = lastTreeDepth;
    {
        // the top-level tree to the front
        const int nAll = (int)nodes->size(), nTopQ = nAll - nDefQ;
        auto remap = [&](int r) { return r < 0 ? r : (r >= nDefQ ? r - nDefQ : r + nTopQ); };
        std::vector<QNode> moved((size_t)nAll);
        for (int i = 0; i < nAll; ++i) {
            QNode qn = (*nodes)[(size_t)i];
            for (int c = 0; c < 4; ++c) qn.child[c] = remap(qn.child[c]);
            moved[(size_t)remap(i)] = qn;
        }
        nodes->swap(moved);
        for (FastDef &fd : *defs) fd.root = fd.root < 0 ? 0 : remap(fd.root);
        for (SubEntry &se : *subs) se.node = remap(se.node);
    }
    {
        double ext = 0;
        for (int a = 0; a < 3; ++a) ext = std::max(ext, std::max(std::fabs((double)L[0].bmin[a]), std::fabs((double)L[0].bmax[a])) + ((double)L[0].bmax[a] - L[0].bmin[a]));
        const double band = d->n_quadrics > 0 ? 0x1p-10 : 0x1p-20;   // (FastBVH::tieRel: quadric hits are accepted by interval bounds)
        out->absBand = (float)(band * ext);
        out->tieRel = (float)(1 + band);
        out->absBandTri = (float)(0x1p-20 * ext);   // the band of a triangle / triangle pair (wf_traverse.h, WalkAccept<PAIRS>)
        out->tieRelTri = (float)(1 + 0x1p-20);
        out->firstGeneral = d->n_quadrics > 0 ? d->n_triangles : INT_MAX;
    }
    if (!gridOk) return false;
    out->nNodes = (int)nodes->size();
    return true;
}

// ---- host-only self-check of the production layout (wf_debug_fastbvh_check; CPU suite) ----------------------------------------------
// Walks the QNode / LeafTri / SubEntry arrays on the HOST with random rays, in double arithmetic and without pruning by distance, and
// checks that every triangle a ray really hits (brute force over the top-level triangles and every (instance, triangle) pair, in the
// instance's space) is among the triangles the walk tests — the one property the production tree owes (wf_traverse.h: "a superset of
// visited nodes, the exact triangle test decides").  No device is needed: BuildFastBVH is host code.
namespace {
struct CheckWalk {
    const std::vector<QNode> &nodes;
    const std::vector<LeafTri> &tris;
    const std::vector<FastDef> &defs;
    const std::vector<SubEntry> &subs;
    const wf_scene_desc *d;
    const FastBVH &top;
    std::vector<std::pair<int, int>> tested;   // (triangle id, instance or -1)
    long long nodesVisited = 0, entries = 0;
    static bool Slab(const float base[3], const float cell[3], const uint32_t q[3], const double o[3], const double dir[3]) {
        double t0 = 0, t1 = 1e300;
        for (int a = 0; a < 3; ++a) {
            const double lo = (double)base[a] + (double)(q[a] & 0xffffu) * (double)cell[a], hi = (double)base[a] + (double)(q[a] >> 16) * (double)cell[a];
            if (lo > hi) return false;   // an empty slot
            if (dir[a] == 0) { if (o[a] < lo || o[a] > hi) return false; continue; }
            double tn = (lo - o[a]) / dir[a], tf = (hi - o[a]) / dir[a];
            if (tn > tf) std::swap(tn, tf);
            t0 = std::max(t0, tn); t1 = std::min(t1, tf);
        }
        return t0 <= t1;
    }
    void Leaf(int ref, int inst, const double o[3], const double dir[3]) {
        int first, count;
        LeafRun(ref, &first, &count);
        if (first >= INST_FIRST) { Enter(first - INST_FIRST, o, dir); return; }
        for (int i = 0; i < count; ++i) {
            const LeafTri &lt = tris[(size_t)first + i];
            if (lt.c.z == 4.f) { if (inst < 0) Enter((int)FloatToBits(lt.c.y), o, dir); continue; }
            tested.push_back({(int)FloatToBits(lt.c.y), inst});
        }
    }
    void Tree(int ref, const float base[3], const float cell[3], int inst, const double o[3], const double dir[3]) {
        std::vector<int> st{ref};
        while (!st.empty()) {
            const int r = st.back();
            st.pop_back();
            if (r == NODE_NONE) continue;
            if (r < 0) { Leaf(r, inst, o, dir); continue; }
            ++nodesVisited;
            const QNode &qn = nodes[(size_t)r];
            for (int c = 0; c < 4; ++c)
                if (qn.child[c] != NODE_NONE && Slab(base, cell, qn.q + 3 * c, o, dir)) st.push_back(qn.child[c]);
        }
    }
    void Enter(int entry, const double oW[3], const double dW[3]) {
        ++entries;
        const SubEntry se = subs[(size_t)entry];
        if (se.node == NODE_NONE) return;
        const wf_instance &in = d->instances[se.inst];
        const float(*mi)[4] = in.render_from_instance.mInv;
        double o[3], dir[3];
        for (int a = 0; a < 3; ++a) {
            o[a] = (double)mi[a][0] * oW[0] + (double)mi[a][1] * oW[1] + (double)mi[a][2] * oW[2] + (double)mi[a][3];
            dir[a] = (double)mi[a][0] * dW[0] + (double)mi[a][1] * dW[1] + (double)mi[a][2] * dW[2];
        }
        const FastDef &fd = defs[(size_t)in.def];
        Tree(se.node, fd.base, fd.cell, se.inst, o, dir);
    }
};
// does the ray hit the triangle well inside (barycentrics > eps, in front of the origin)?  Moeller-Trumbore in double arithmetic
bool HitsClearly(const double o[3], const double dir[3], const float *p0, const float *p1, const float *p2) {
    double e1[3], e2[3], pv[3], tv[3], qv[3];
    for (int a = 0; a < 3; ++a) { e1[a] = (double)p1[a] - p0[a]; e2[a] = (double)p2[a] - p0[a]; tv[a] = o[a] - p0[a]; }
    pv[0] = dir[1] * e2[2] - dir[2] * e2[1]; pv[1] = dir[2] * e2[0] - dir[0] * e2[2]; pv[2] = dir[0] * e2[1] - dir[1] * e2[0];
    const double det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
    const double scale = std::sqrt((e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]) * (e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]) * (dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]));
    if (!(std::fabs(det) > 1e-9 * scale)) return false;
    const double u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) / det;
    qv[0] = tv[1] * e1[2] - tv[2] * e1[1]; qv[1] = tv[2] * e1[0] - tv[0] * e1[2]; qv[2] = tv[0] * e1[1] - tv[1] * e1[0];
    const double v = (dir[0] * qv[0] + dir[1] * qv[1] + dir[2] * qv[2]) / det;
    const double t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) / det;
    return u > 1e-4 && v > 1e-4 && u + v < 1 - 1e-4 && t > 1e-6;
}
}  // namespace

extern "C" int wf_debug_fastbvh_check(const wf_scene_desc *d, int n_rays, uint64_t seed, int64_t out[8]) {
    if (!d || !out || n_rays < 0) return fail(-1, "wf_debug_fastbvh_check: bad arguments");
    FastTrees trees;
    FastDepths fdep;
    for (int k = 0; k < 8; ++k) out[k] = 0;
    if (!BuildFastBVH(d, Switches::FromEnv(), &trees, &fdep)) return fail(-1, "wf_debug_fastbvh_check: the scene has no production layout");
    out[0] = (int64_t)trees.nodes.size(); out[1] = (int64_t)trees.tris.size(); out[2] = (int64_t)trees.subs.size(); out[3] = fdep.top;
    // structure: every child reference names a node / a leaf run / an entry inside the arrays
    for (size_t i = 0; i < trees.nodes.size(); ++i)
        for (int c = 0; c < 4; ++c) {
            const int r = trees.nodes[i].child[c];
            if (r == NODE_NONE) continue;
            if (r >= 0) { if ((size_t)r >= trees.nodes.size()) return fail(-1, "wf_debug_fastbvh_check: node %zu child %d out of range", i, c); continue; }
            int first, count;
            LeafRun(r, &first, &count);
            if (first >= INST_FIRST ? (size_t)(first - INST_FIRST) >= trees.subs.size() : (size_t)first + count > trees.tris.size()) return fail(-1, "wf_debug_fastbvh_check: node %zu child %d: leaf run out of range", i, c);
        }
    for (const SubEntry &se : trees.subs)
        if (se.inst < 0 || se.inst >= d->n_instances || (se.node >= 0 && (size_t)se.node >= trees.nodes.size())) return fail(-1, "wf_debug_fastbvh_check: entry out of range");
    // coverage with random rays through the scene's box
    uint64_t rng = seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
    auto rnd = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (double)(rng >> 11) * (1.0 / 9007199254740992.0); };
    const wf_bvh_node &root = d->bvh_nodes[0];
    CheckWalk cw{trees.nodes, trees.tris, trees.defs, trees.subs, d, trees.header, {}};
    const int nGeom = d->n_triangles + d->n_quadrics;
    for (int r = 0; r < n_rays; ++r) {
        double o[3], dir[3], tgt[3];
        for (int a = 0; a < 3; ++a) {
            const double lo = root.bmin[a], hi = root.bmax[a], ext = hi - lo;
            o[a] = lo - 0.1 * ext + 1.2 * ext * rnd();
            tgt[a] = lo + ext * rnd();
            dir[a] = tgt[a] - o[a];
        }
        cw.tested.clear();
        cw.Tree(0, trees.header.base, trees.header.cell, -1, o, dir);
        std::sort(cw.tested.begin(), cw.tested.end());
        out[6] += (int64_t)cw.tested.size();
        auto check = [&](int tri, int inst, const double oo[3], const double dd[3]) {
            const int32_t *v = d->tri_indices + 3 * (size_t)tri;
            if (!HitsClearly(oo, dd, d->P + 3 * (size_t)v[0], d->P + 3 * (size_t)v[1], d->P + 3 * (size_t)v[2])) return;
            ++out[4];
            if (!std::binary_search(cw.tested.begin(), cw.tested.end(), std::make_pair(tri, inst))) ++out[5];
        };
        // the top-level primitives and, per instance, its definition's
        int nTopPrims = 0;
        for (int i = 0; i < (d->n_top_bvh_nodes > 0 ? d->n_top_bvh_nodes : d->n_bvh_nodes); ++i) nTopPrims += d->bvh_nodes[i].nprims;
        for (int j = 0; j < nTopPrims; ++j) {
            const int t = d->bvh_prims[j];
            if (t < d->n_triangles) { check(t, -1, o, dir); continue; }
            if (t < nGeom) continue;
            const int ii = t - nGeom;
            const wf_instance &in = d->instances[ii];
            if (in.def < 0 || in.def >= d->n_instance_defs) continue;
            const float(*mi)[4] = in.render_from_instance.mInv;
            double oI[3], dI[3];
            for (int a = 0; a < 3; ++a) {
                oI[a] = (double)mi[a][0] * o[0] + (double)mi[a][1] * o[1] + (double)mi[a][2] * o[2] + (double)mi[a][3];
                dI[a] = (double)mi[a][0] * dir[0] + (double)mi[a][1] * dir[1] + (double)mi[a][2] * dir[2];
            }
            const wf_instance_def &def = d->instance_defs[in.def];
            for (int k = def.first_prim; k < def.first_prim + def.n_prims; ++k)
                if (d->bvh_prims[k] < d->n_triangles) check(d->bvh_prims[k], ii, oI, dI);
        }
    }
    out[7] = cw.entries;
    out[3] = cw.nodesVisited;
    return 0;
}
