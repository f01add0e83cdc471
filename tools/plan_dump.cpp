// tools/plan_dump.cpp — the library's host-only planning units (pbrt-v4_amd/csrc/hip/wf_plan.cpp, wf_fastbvh_build.cpp) run stand-alone:
// no device, no libwfhip / libwfhost, nothing loaded into another process.  For every scene file on the command line: ParseFiles,
// BuildSceneTables, PlanScene under the environment's switches and the builder's self-check, then ONE line with every field of the plan,
// the sizes and a 64-bit FNV-1a of the four arrays of the production traversal layout, a hash of the header's scalar fields and the
// eight outputs of the self-check.  Two builds of the planning code agree on a scene exactly when their lines are equal; built with
// sanitizers (make -C pbrt-v4_amd SAN="-fsanitize=..." ...plan_dump, tools/sanitize_checker.sh) it is how that code is run under them.
//
// With --tables the line also carries what BuildSceneTables made: `name=count:fnv64` for every vector SceneTables::Save writes, the
// scalars it writes, materialTypePresent and a hash of the descriptor with its pointers cleared — two builds of scene_build.cpp agree on
// a scene exactly when these are equal (tools/plan_dump_all.sh tables, profiles/scene_build_tables_parent_vs_change.txt).
//
//   plan_dump [--datadir <dir>] [--rays <n>] [--tables] scene.pbrt ...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "check_common.h"
#include "../pbrt-v4_amd/csrc/hip/wf_plan.h"

using namespace wf;
using namespace wf::planning;

static uint64_t Fnv(const void *p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
template <typename T>
static uint64_t FnvOf(const std::vector<T> &v) { return Fnv(v.data(), v.size() * sizeof(T)); }

// every array and scalar of SceneTables::Save, in its order
static void DumpTables(const SceneTables &T) {
#define VEC(v) (T.v.empty() ? printf(" " #v "=0") : printf(" " #v "=%zu:%016llx", T.v.size(), (unsigned long long)FnvOf(T.v)))
    VEC(P); VEC(N); VEC(UV); VEC(triIndices); VEC(triMesh); VEC(bvhPrims); VEC(infiniteLights);
    VEC(meshes); VEC(quadrics); VEC(instances); VEC(instanceDefs); VEC(animated); VEC(sobolMatrices); VEC(vdcSobol); VEC(vdcSobolInv); VEC(haltonPrimes); VEC(haltonPermOffsets);
    VEC(haltonPerms); VEC(bvhNodes); VEC(pool.spectra); VEC(pool.data); VEC(textures); VEC(materials);
    VEC(lights); VEC(lightBvh); VEC(lightTransforms); VEC(filterData); VEC(powerAlias); VEC(imageLights);
    VEC(noisePerm); VEC(texImages); VEC(tableData); VEC(media); VEC(mediumData);
    printf(" imageFile=%zu:%016llx", T.imageFile.size(), (unsigned long long)Fnv(T.imageFile.data(), T.imageFile.size()));
    VEC(sRGBFromFilmRGB); VEC(S);
#undef VEC
    printf(" scalars=%d,%d,%d,%d,%d,%d,%d,%d matTypePresent=", T.nTopBvhNodes, T.nTopPrims, T.saveFP16 ? 1 : 0, T.spp, T.scanlinesPerPass, T.maxQueueSize, T.nPasses,
           T.desc.rgb2spec_coeffs ? 1 : 0);
    for (bool b : T.materialTypePresent) putchar('0' + b);
    // the descriptor without its addresses: Finalize() of a SceneTables with no arrays sets every pointer it owns to null (and the counts,
    // which the sizes above already give, to 0); the one pointer that is not into the tables is cleared by hand (the 0/1 flag above)
    SceneTables E;
    E.desc = T.desc;
    E.Finalize();
    E.desc.rgb2spec_coeffs = nullptr;
    printf(" desc=%016llx", (unsigned long long)Fnv(&E.desc, sizeof E.desc));
}

static void DumpScene(const std::string &path, int nRays, bool tables) {
    RenderOptions opt = check::QuietOptions();
    SceneTables T;
    check::LoadTables(path, &opt, &T);
    const size_t slash = path.rfind('/');
    printf("%s:", (slash == std::string::npos ? path : path.substr(slash + 1)).c_str());
    if (tables) DumpTables(T);
    ScenePlan p;
    FastTrees trees;
    if (PlanScene(&T.desc, Switches::FromEnv(), &p, &trees)) { printf(" rejected: %s\n", wf_last_error()); return; }
    printf(" nBvhPrims=%lld nInstances=%d nestedAnimated=%d haveAlpha=%d texNeedsFootprint=%d haveMix=%d haveSubsurface=%d haveQuadricAlpha=%d haveCurves=%d haveAnimated=%d",
           (long long)p.nBvhPrims, p.nInstances, p.nestedAnimated, p.haveAlpha, p.texNeedsFootprint, p.haveMix, p.haveSubsurface, p.haveQuadricAlpha, p.haveCurves, p.haveAnimated);
    printf(" matTypeMask=%#x matPresent=", p.matTypeMask);
    for (bool b : p.matPresent) putchar('0' + b);
    printf(" mediumLean=%d portalLights=%d leanShade=%d leanType=", p.mediumLean, p.portalLights, p.leanShade);
    for (bool b : p.leanType) putchar('0' + b);
    printf(" rareLights=%d genMode=%d deferGeneral=%d genTri=%d fastBuilt=%d fastOk=%d animFast=%d cursorChunk=%d cursorChunkShadow=%d spillRows=%d trRoute=%d",
           p.rareLights, p.genMode, p.deferGeneral, p.genTri, p.fastBuilt, p.fastOk, p.animFast, p.cursorChunk, p.cursorChunkShadow, p.spillRows, p.trRoute);
    printf(" cameraAnim=%d routeVariant=%d trFastAlpha=%d shadeVariant=", p.cameraAnim, p.routeVariant, p.trFastAlpha);
    for (int v : p.shadeVariant) putchar('0' + v);
    if (!p.fastBuilt) { printf(" trees: no production layout\n"); return; }
    const FastBVH &h = trees.header;
    uint64_t hh = Fnv(&h.nNodes, sizeof h.nNodes);   // the header's fields one by one: no padding, no pointers
    hh = Fnv(h.base, sizeof h.base, hh);
    hh = Fnv(h.cell, sizeof h.cell, hh);
    hh = Fnv(&h.absBand, sizeof h.absBand, hh);
    hh = Fnv(&h.tieRel, sizeof h.tieRel, hh);
    hh = Fnv(&h.tieRelTri, sizeof h.tieRelTri, hh);
    hh = Fnv(&h.absBandTri, sizeof h.absBandTri, hh);
    hh = Fnv(&h.firstGeneral, sizeof h.firstGeneral, hh);
    printf(" nodes=%zu:%016llx tris=%zu:%016llx defs=%zu:%016llx subs=%zu:%016llx header=%016llx", trees.nodes.size(), (unsigned long long)FnvOf(trees.nodes),
           trees.tris.size(), (unsigned long long)FnvOf(trees.tris), trees.defs.size(), (unsigned long long)FnvOf(trees.defs), trees.subs.size(),
           (unsigned long long)FnvOf(trees.subs), (unsigned long long)hh);
    int64_t out[8];
    if (wf_debug_fastbvh_check(&T.desc, nRays, 1, out)) { printf(" check: %s\n", wf_last_error()); return; }
    printf(" check=");
    for (int k = 0; k < 8; ++k) printf("%s%lld", k ? "," : "", (long long)out[k]);
    printf("\n");
}

int main(int argc, char **argv) {
    std::string dataDir;
    int nRays = 64;
    bool tables = false;
    std::vector<std::string> scenes;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--datadir" && i + 1 < argc) dataDir = argv[++i];
        else if (a == "--rays" && i + 1 < argc) nRays = atoi(argv[++i]);
        else if (a == "--tables") tables = true;
        else scenes.push_back(a);
    }
    if (scenes.empty()) { fprintf(stderr, "usage: plan_dump [--datadir <dir>] [--rays <n>] [--tables] scene.pbrt ...\n"); return 1; }
    return check::Guarded("", [&] {
        check::InitData(dataDir, argv[0], "/../data");   // (the binary's usual location: pbrt-v4_amd/_build/plan_dump)
        for (const std::string &s : scenes) { DumpScene(s, nRays, tables); fflush(stdout); }
        return 0;
    });
}
