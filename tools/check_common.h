// tools/check_common.h — what the stand-alone host programs over scene files share (tools/plan_dump.cpp, light_sample_check.cpp,
// bsdf_check.cpp, oracle/wf_cpu/wf_cpu.cpp): the data directory's default, a scene file loaded into its tables and the host SceneView
// over them (csrc/common/wf_scene_view.h HostSceneView), the catch around it all, and the two --eval / --self helpers of the checkers.
// Each program keeps its own command line, messages and exit codes.  Host only; the program links the host objects (Makefile).
#pragma once
#include <cstdint>
#include <cstdio>
#include <exception>
#include <string>
#include <vector>
#include "../pbrt-v4_amd/csrc/common/wf_kernels.h"
#include "../pbrt-v4_amd/csrc/common/wf_scene_view.h"
#include "../pbrt-v4_amd/csrc/host/scene.h"
#include "../pbrt-v4_amd/csrc/host/spectra.h"

namespace wf { namespace check {

// SpectralData::Init on --datadir's value, or, without one, on `rel` (the way to <repo>/pbrt-v4_amd/data) beside the running binary
inline void InitData(std::string dataDir, const char *argv0, const char *rel) {
    if (dataDir.empty()) {
        const std::string self = argv0;
        const size_t p = self.rfind('/');
        dataDir = (p == std::string::npos ? std::string(".") : self.substr(0, p)) + rel;
    }
    SpectralData::Init(dataDir, dataDir + "/cache");
}
inline RenderOptions QuietOptions(int spp = 0) {
    RenderOptions opt;
    opt.quiet = true;
    if (spp > 0) opt.pixelSamples = spp;
    return opt;
}
inline void LoadTables(const std::string &path, RenderOptions *opt, SceneTables *T) {
    ParsedScene parsed;
    ParseFiles({path}, opt, &parsed);
    BuildSceneTables(parsed, *opt, T);
}
// A scene file's tables with the full host view over them: self attached, and the fatal word RaiseFatal (wf_scene.h) writes to
struct HostScene {
    SceneTables T;
    uint32_t sobol[WF_SOBOL_WORDS];
    int32_t fatalWord = 0;
    SceneView sv;
    HostScene(const std::string &path, RenderOptions *opt) {
        LoadTables(path, opt, &T);
        FillSobol2D(sobol);
        sv = HostSceneView(T.desc, sobol);
        sv.self = &sv;
        sv.fatal = &fatalWord;
    }
    HostScene(const HostScene &) = delete;
};
// main's body under the catch of the parser's and the builder's errors: "<what>: <message>" (or the message alone), exit code 1
template <typename F>
int Guarded(const std::string &what, F body) {
    try {
        return body();
    } catch (const std::exception &e) {
        fprintf(stderr, "%s%s%s\n", what.c_str(), what.empty() ? "" : ": ", e.what());
        return 1;
    }
}

template <typename T> bool ReadVec(FILE *f, std::vector<T> &v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}
// four wavelengths a quarter of the visible range apart, rotated into it: the first from u in [0, 1)
inline F4 RotatedWavelengths(float u) {
    F4 l;
    l.x = 360.f + u * 470.f;
    float *p = &l.x;
    for (int i = 1; i < 4; ++i) { p[i] = p[i - 1] + 117.5f; if (p[i] > 830.f) p[i] = 360.f + (p[i] - 830.f); }
    return l;
}

}}  // namespace check
