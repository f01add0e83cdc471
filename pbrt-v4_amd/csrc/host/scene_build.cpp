// scene_build.cpp — flattens a ParsedScene into the index-addressed tables of wf_scene_desc.
// Restates the object construction the reference spreads over BasicScene::Create* (scene.cpp:835-1591)
// and the per-class ::Create functions, for the feature subset the wavefront kernels implement:
//   film.cpp:66-172,213-253,484-497,573-585   FilmBaseParameters / PixelSensor / RGBFilm
//   filters.cpp:26-147                         filters + FilterSampler
//   cameras.cpp:27-57,269-281,486-528          CameraTransform / Perspective / Orthographic
//   samplers.cpp:146-170                       ZSobol
//   materials.cpp:51-659                       material parameter defaults
//   lights.cpp:120-166,684-941,1345-1380       light parameter handling, scale normalisation, Bounds()
//   util/mesh.cpp:25-75, shapes.cpp:283-307,368-438  triangle meshes (vertices transformed to render space)
#include "scene.h"
#include <unistd.h>
#include <zlib.h>
#include "../common/wf_camera.h"
#include "hanimated.h"
#include "../common/wf_shapes.h"
#include "../common/wf_bssrdf.h"
#include "../common/wf_lights.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <functional>
#include <array>
#include <sstream>
#include <set>
#include <thread>
#include <mutex>
#include <atomic>

namespace wf {

[[noreturn]] static void Die(const std::string &loc, const std::string &msg) {
    throw SceneError("Error: " + loc + ": " + msg);
}

// Image::Read with the default encoding (8-bit PNG: sRGB) for the light sources: the pixels as Image::GetChannel returns
// them, grey replicated to three channels; *nc is the file's channel count (1 Y, 3 R G B, 4 R G B A)
static void ReadLightImage(const std::string &filename, const std::string &loc, std::vector<float> *rgb, int *w, int *h, int *nc, HostImage *raw = nullptr) {
    HostImage localImg;
    HostImage &img = raw ? *raw : localImg;
    try { ReadImage(filename, ColorEnc(), &img); } catch (const SceneError &e) { Die(loc, std::string(e.what()).substr(7)); }
    *w = img.w; *h = img.h; *nc = img.nc;
    rgb->resize((size_t)img.w * img.h * 3);
    for (size_t i = 0; i < (size_t)img.w * img.h; ++i)
        for (int c = 0; c < 3; ++c) (*rgb)[3 * i + c] = img.Get(i * img.nc + (img.nc >= 3 ? c : 0));
}

void SceneTables::Finalize() {
    desc.abi_version = WF_ABI_VERSION;
    desc.n_vertices = (int)P.size() / 3;
    desc.n_triangles = (int)triIndices.size() / 3;
    desc.n_meshes = (int)meshes.size();
    desc.n_bvh_nodes = (int)bvhNodes.size();
    desc.P = P.data(); desc.N = N.data(); desc.UV = UV.data();
    desc.n_tangents = (int64_t)S.size() / 3; desc.S = S.empty() ? nullptr : S.data();
    desc.tri_indices = triIndices.data(); desc.tri_mesh = triMesh.data();
    desc.meshes = meshes.data(); desc.bvh_nodes = bvhNodes.data(); desc.bvh_prims = bvhPrims.data();
    desc.n_quadrics = (int)quadrics.size(); desc.quadrics = quadrics.data();
    desc.n_instances = (int)instances.size(); desc.instances = instances.data();
    desc.n_instance_defs = (int)instanceDefs.size(); desc.instance_defs = instanceDefs.data();
    desc.n_animated = (int)animated.size(); desc.animated = animated.empty() ? nullptr : animated.data();
    desc.n_top_bvh_nodes = nTopBvhNodes; desc.n_top_prims = nTopPrims;
    desc.sobol_matrices = sobolMatrices.empty() ? nullptr : sobolMatrices.data();
    desc.vdc_sobol = vdcSobol.empty() ? nullptr : vdcSobol.data();
    desc.vdc_sobol_inv = vdcSobolInv.empty() ? nullptr : vdcSobolInv.data();
    desc.halton_primes = haltonPrimes.empty() ? nullptr : haltonPrimes.data();
    desc.halton_perm_offsets = haltonPermOffsets.empty() ? nullptr : haltonPermOffsets.data();
    desc.halton_perms = haltonPerms.empty() ? nullptr : haltonPerms.data();
    desc.n_halton_perms = (int64_t)haltonPerms.size();
    desc.n_spectra = (int)pool.spectra.size(); desc.n_spectrum_floats = (int)pool.data.size();
    desc.spectra = pool.spectra.data(); desc.spectrum_data = pool.data.data();
    desc.n_textures = (int)textures.size(); desc.textures = textures.data();
    desc.n_materials = (int)materials.size(); desc.materials = materials.data();
    desc.n_lights = (int)lights.size(); desc.lights = lights.data();
    desc.n_infinite_lights = (int)infiniteLights.size(); desc.infinite_lights = infiniteLights.data();
    desc.n_light_bvh_nodes = (int)lightBvh.size(); desc.light_bvh_nodes = lightBvh.data();
    desc.n_light_transforms = (int)lightTransforms.size(); desc.light_transforms = lightTransforms.data();
    desc.power_alias = powerAlias.data();
    desc.n_filter_floats = (int)filterData.size(); desc.filter_data = filterData.data();
    desc.n_image_lights = (int)imageLights.size(); desc.image_lights = imageLights.data();
    desc.n_tex_images = (int)texImages.size(); desc.tex_images = texImages.data();
    desc.n_table_floats = (int)tableData.size(); desc.table_data = tableData.data();
    desc.noise_perm = noisePerm.empty() ? nullptr : noisePerm.data();
    desc.n_media = (int)media.size(); desc.media = media.data();
    desc.n_medium_floats = (int)mediumData.size(); desc.medium_data = mediumData.data();
}

// ---- on-disk cache of the built tables -------------------------------------------------------------------------------
namespace {
constexpr uint64_t kTablesMagic = 0x3230424154465755ull;  // "UWFTAB02"
template <typename V> void putVec(FILE *f, const V &v) {
    uint64_t n = v.size();
    fwrite(&n, 8, 1, f);
    if (n) fwrite(v.data(), sizeof(v[0]), n, f);
}
template <typename V> bool getVec(FILE *f, V &v) {
    uint64_t n = 0;
    if (fread(&n, 8, 1, f) != 1 || n > (1ull << 36)) return false;
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(v[0]), n, f) == n;
}
}  // namespace
bool SceneTables::Save(const std::string &path) const {
    const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return false;
    uint64_t hdr[4] = {kTablesMagic, (uint64_t)WF_ABI_VERSION, sizeof(wf_scene_desc), sizeof(SceneTables)};
    fwrite(hdr, 8, 4, f);
    fwrite(&desc, sizeof(desc), 1, f);
    putVec(f, P); putVec(f, N); putVec(f, UV); putVec(f, triIndices); putVec(f, triMesh); putVec(f, bvhPrims); putVec(f, infiniteLights);
    putVec(f, meshes); putVec(f, quadrics); putVec(f, instances); putVec(f, instanceDefs); putVec(f, animated); putVec(f, sobolMatrices); putVec(f, vdcSobol); putVec(f, vdcSobolInv); putVec(f, haltonPrimes); putVec(f, haltonPermOffsets);
    putVec(f, haltonPerms); putVec(f, bvhNodes); putVec(f, pool.spectra); putVec(f, pool.data); putVec(f, textures); putVec(f, materials);
    putVec(f, lights); putVec(f, lightBvh); putVec(f, lightTransforms); putVec(f, filterData); putVec(f, powerAlias); putVec(f, imageLights);
    putVec(f, noisePerm); putVec(f, texImages); putVec(f, tableData); putVec(f, media); putVec(f, mediumData); putVec(f, imageFile); putVec(f, sRGBFromFilmRGB); putVec(f, S);
    int32_t sc[8] = {nTopBvhNodes, nTopPrims, saveFP16 ? 1 : 0, spp, scanlinesPerPass, maxQueueSize, nPasses, desc.rgb2spec_coeffs ? 1 : 0};
    fwrite(sc, 4, 8, f);
    fwrite(materialTypePresent, sizeof(materialTypePresent), 1, f);
    uint64_t end = kTablesMagic;
    fwrite(&end, 8, 1, f);
    bool ok = fflush(f) == 0;
    fclose(f);
    if (!ok || rename(tmp.c_str(), path.c_str()) != 0) { remove(tmp.c_str()); return false; }  // atomic: readers never see a partial file
    return true;
}
bool SceneTables::Load(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    uint64_t hdr[4];
    bool ok = fread(hdr, 8, 4, f) == 4 && hdr[0] == kTablesMagic && hdr[1] == (uint64_t)WF_ABI_VERSION && hdr[2] == sizeof(wf_scene_desc) && hdr[3] == sizeof(SceneTables);
    ok = ok && fread(&desc, sizeof(desc), 1, f) == 1;
    ok = ok && getVec(f, P) && getVec(f, N) && getVec(f, UV) && getVec(f, triIndices) && getVec(f, triMesh) && getVec(f, bvhPrims) && getVec(f, infiniteLights) &&
         getVec(f, meshes) && getVec(f, quadrics) && getVec(f, instances) && getVec(f, instanceDefs) && getVec(f, animated) && getVec(f, sobolMatrices) && getVec(f, vdcSobol) && getVec(f, vdcSobolInv) && getVec(f, haltonPrimes) && getVec(f, haltonPermOffsets) &&
         getVec(f, haltonPerms) && getVec(f, bvhNodes) && getVec(f, pool.spectra) && getVec(f, pool.data) && getVec(f, textures) && getVec(f, materials) &&
         getVec(f, lights) && getVec(f, lightBvh) && getVec(f, lightTransforms) && getVec(f, filterData) && getVec(f, powerAlias) && getVec(f, imageLights) &&
         getVec(f, noisePerm) && getVec(f, texImages) && getVec(f, tableData) && getVec(f, media) && getVec(f, mediumData) && getVec(f, imageFile) && getVec(f, sRGBFromFilmRGB) && getVec(f, S);
    int32_t sc[8];
    ok = ok && fread(sc, 4, 8, f) == 8 && fread(materialTypePresent, sizeof(materialTypePresent), 1, f) == 1;
    uint64_t end = 0;
    ok = ok && fread(&end, 8, 1, f) == 1 && end == kTablesMagic;
    fclose(f);
    if (!ok) return false;
    nTopBvhNodes = sc[0]; nTopPrims = sc[1]; saveFP16 = sc[2] != 0; spp = sc[3]; scanlinesPerPass = sc[4]; maxQueueSize = sc[5]; nPasses = sc[6];
    Finalize();
    // the one pointer that does not point into this object: the sRGB RGB -> spectrum coefficient table (process-wide)
    desc.rgb2spec_coeffs = sc[7] ? SpectralData::Get().sRGB()->table->coeffs.data() : nullptr;
    return true;
}

namespace {

// ---- textures & materials ---------------------------------------------------------------------------
// GetMediumScatteringProperties (media.cpp:79-150) over data/medium_presets.txt (tools/extract_medium_presets.py): RGBUnboundedSpectrum in sRGB
static bool MediumPreset(const std::string &name, SpectrumP *sigma_a, SpectrumP *sigma_s) {
    std::ifstream f(SpectralData::Get().DataDir() + "/medium_presets.txt");
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        size_t b1 = line.find(" | "), b2 = line.find(" | ", b1 == std::string::npos ? 0 : b1 + 3);
        if (b1 == std::string::npos || b2 == std::string::npos || line.substr(0, b1) != name) continue;
        double s[3], a[3];
        if (sscanf(line.c_str() + b1 + 3, "%lf %lf %lf", &s[0], &s[1], &s[2]) != 3 || sscanf(line.c_str() + b2 + 3, "%lf %lf %lf", &a[0], &a[1], &a[2]) != 3) continue;
        const float sf[3] = {(float)s[0], (float)s[1], (float)s[2]}, af[3] = {(float)a[0], (float)a[1], (float)a[2]};  // RGB(double, double, double)
        *sigma_a = SpectralData::Get().sRGB()->Unbounded(af);
        *sigma_s = SpectralData::Get().sRGB()->Unbounded(sf);
        return true;
    }
    return false;
}

// the Perlin permutation of util/noise.cpp (data/noise_perm.txt, written by tools/extract_noise_perm.py)
static void LoadNoisePerm(SceneTables *T) {
    if (!T->noisePerm.empty()) return;
    std::ifstream f(SpectralData::Get().DataDir() + "/noise_perm.txt");
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ls(line);
        int v;
        while (ls >> v) T->noisePerm.push_back(v);
    }
    if (T->noisePerm.size() != 512) Die("", "data/noise_perm.txt: expected the 512-entry Perlin permutation (tools/extract_noise_perm.py)");
}

struct TexBuilder {
    SceneTables *T;
    std::map<std::string, int> floatTextures, spectrumTexturesAlbedo, spectrumTexturesUnbounded, spectrumTexturesIllum;
    const ParsedScene *scene;
    bool disableImageTextures = false;

    std::vector<int> texDepth;  // nesting depth of every texture node: the device walks the graph with a stack of WF_TEX_STACK frames
    int AddTex(const wf_texture &t) {
        int d = 1;
        if (t.type != WF_TEX_SPECTRUM_BILERP)  // (its tex0..2 hold spectrum ids, not child textures)
            for (int c : {t.tex0, t.tex1, t.tex2})
                if (c >= 0) d = std::max(d, 1 + texDepth[c]);
        if (d > WF_TEX_STACK) Die("", "texture graph nested deeper than " + std::to_string(WF_TEX_STACK) + " levels");
        texDepth.push_back(d);
        T->textures.push_back(t);
        return (int)T->textures.size() - 1;
    }
    int FloatConst(float v) {
        wf_texture t{};
        t.type = WF_TEX_FLOAT_CONSTANT; t.f0 = v; t.spectrum = t.tex0 = t.tex1 = t.tex2 = -1;
        return AddTex(t);
    }
    int SpectrumConst(const SpectrumH &s) {
        wf_texture t{};
        t.type = WF_TEX_SPECTRUM_CONSTANT; t.spectrum = T->pool.Add(s); t.tex0 = t.tex1 = t.tex2 = -1;
        return AddTex(t);
    }
    std::map<std::string, int> &SpecMap(SpectrumType st) {
        return st == SpectrumType::Albedo ? spectrumTexturesAlbedo : (st == SpectrumType::Unbounded ? spectrumTexturesUnbounded : spectrumTexturesIllum);
    }
    // TextureParameterDictionary::GetFloatTextureOrNull (paramdict.cpp:700-745)
    int GetFloatTextureOrNull(const ParamSet &ps, const std::string &name) {
        for (const Param &p : ps.params) {
            if (p.name != name) continue;
            if (p.type == "texture") {
                p.lookedUp = true;
                auto it = floatTextures.find(p.strings.at(0));
                if (it == floatTextures.end()) Die(p.loc, "Couldn't find float texture named \"" + p.strings[0] + "\" for parameter \"" + name + "\"");
                return it->second;
            } else if (p.type == "float") {
                p.lookedUp = true;
                return FloatConst(p.floats.at(0));
            }
        }
        return -1;
    }
    int GetFloatTexture(const ParamSet &ps, const std::string &name, float def) {
        int t = GetFloatTextureOrNull(ps, name);
        return t >= 0 ? t : FloatConst(def);
    }
    // TextureParameterDictionary::GetSpectrumTextureOrNull (paramdict.cpp:747-820)
    int GetSpectrumTextureOrNull(const ParamSet &ps, const std::string &name, SpectrumType st) {
        for (const Param &p : ps.params) {
            if (p.name != name) continue;
            if (p.type == "texture") {
                p.lookedUp = true;
                auto &m = SpecMap(st);
                auto it = m.find(p.strings.at(0));
                if (it == m.end()) Die(p.loc, "Couldn't find spectrum texture named \"" + p.strings[0] + "\" for parameter \"" + name + "\"");
                return it->second;
            } else if (p.type == "rgb" || p.type == "spectrum" || p.type == "blackbody") {
                SpectrumP s = ps.GetOneSpectrum(name, nullptr, st);
                if (s) return SpectrumConst(*s);
            }
        }
        return -1;
    }
    int GetSpectrumTexture(const ParamSet &ps, const std::string &name, const SpectrumH &def, SpectrumType st) {
        int t = GetSpectrumTextureOrNull(ps, name, st);
        return t >= 0 ? t : SpectrumConst(def);
    }

    // TextureMapping2D::Create (textures.cpp:49-73) for the 2D checkerboard: UVMapping(su, sv, du, dv)
    // TextureMapping2D::Create (textures.cpp:49-73)
    void SetMapping2D(const TextureEntity &te, wf_texture *t) {
        const ParamSet &ps = te.params;
        std::string type = ps.GetOneString("mapping", "uv");
        t->xform = -1;
        if (type == "uv") {
            t->mapping = WF_TEXMAP_UV;
            t->map[0] = ps.GetOneFloat("uscale", 1.f);
            t->map[1] = ps.GetOneFloat("vscale", 1.f);
            t->map[2] = ps.GetOneFloat("udelta", 0.f);
            t->map[3] = ps.GetOneFloat("vdelta", 0.f);
            return;
        }
        if (type == "spherical") t->mapping = WF_TEXMAP_SPHERICAL;
        else if (type == "cylindrical") t->mapping = WF_TEXMAP_CYLINDRICAL;
        else if (type == "planar") {
            t->mapping = WF_TEXMAP_PLANAR;
            V3 v1 = ps.GetOneVector3f("v1", V3{1, 0, 0}), v2 = ps.GetOneVector3f("v2", V3{0, 1, 0});
            t->map[2] = ps.GetOneFloat("udelta", 0.f);
            t->map[3] = ps.GetOneFloat("vdelta", 0.f);
            t->map[4] = v1.x; t->map[5] = v1.y; t->map[6] = v1.z;
            t->map[7] = v2.x; t->map[8] = v2.y; t->map[9] = v2.z;
        } else Die(te.loc, "2D texture mapping \"" + type + "\" unknown");
        t->xform = (int)T->lightTransforms.size();
        T->lightTransforms.push_back(te.renderFromTexture.abi());
    }
    // TextureMapping3D::Create (textures.cpp:75-79): PointTransformMapping(Inverse(renderFromTexture))
    void SetMapping3D(const TextureEntity &te, wf_texture *t) {
        t->mapping = WF_TEXMAP_POINT3D;
        t->xform = (int)T->lightTransforms.size();
        T->lightTransforms.push_back(te.renderFromTexture.abi());
    }
    void NeedNoise() { LoadNoisePerm(T); }
    void NeedSRGBTable() {
        if (T->desc.rgb2spec_coeffs) return;
        const ColorSpace *cs = SpectralData::Get().sRGB();
        T->desc.rgb2spec_coeffs = cs->table->coeffs.data();
        for (int i = 0; i < 64; ++i) T->desc.rgb2spec_znodes[i] = cs->table->zNodes[i];
    }
    void CheckerMapping(const TextureEntity &te, wf_texture *t) {
        int dim = te.params.GetOneInt("dimension", 2);
        if (dim != 2 && dim != 3) Die(te.loc, std::to_string(dim) + " dimensional checkerboard texture not supported");
        if (dim == 2) SetMapping2D(te, t);
        else SetMapping3D(te, t);
    }
    // ImageTextureBase ctor + MIPMap::CreateFromFile + Image::GeneratePyramid (textures.h:528-550, util/mipmap.cpp:163-206, 351-383,
    // util/image.cpp:313-383).  The levels are uploaded as floats holding exactly what Image::GetChannel returns for the
    // level's own storage format: an 8-bit image's levels are re-encoded to bytes (and a 16-bit one's to halves) after the
    // float down-sampling, as CopyRectIn does, and decoded again here.
    std::map<std::string, int> imageCache;
    int ewaLutOffset = -1;
    std::map<std::string, int> namedMaterialIds;  // in definition order: a "mix" material names earlier ones
    std::map<std::string, int> measuredCache;     // .bsdf file -> header offset in tableData
    std::map<std::string, int> texelLutCache;     // colour encoding -> its 256-entry ToLinear table in tableData (8-bit image maps)
    // Image::ResampleWeights / FloatResizeUp (util/image.cpp:386-497): separable windowed-sinc up-sampling to the next
    // power of two; the result per pixel does not depend on the reference's tiling
    static void FloatResizeUp(const HostImage &img, int wm, int nw, int nh, std::vector<float> *out) {
        struct RW { int first; float w[4]; };
        auto weights = [](int oldRes, int newRes) {
            std::vector<RW> wt(newRes);
            const float filterRadius = 2, tau = 2;
            auto sinc = [](float x) { x = Pi * x; return 1 - x * x == 1 ? 1.f : std::sin(x) / x; };   // SinXOverX (util/math.h)
            for (int i = 0; i < newRes; ++i) {
                float center = (i + .5f) * oldRes / newRes;
                wt[i].first = (int)std::floor((center - filterRadius) + 0.5f);
                for (int j = 0; j < 4; ++j) {
                    float pos = wt[i].first + j + .5f, x = pos - center;
                    wt[i].w[j] = std::abs(x) > filterRadius ? 0.f : sinc(x) * sinc(x / tau);
                }
                float invSumWts = 1 / (wt[i].w[0] + wt[i].w[1] + wt[i].w[2] + wt[i].w[3]);
                for (int j = 0; j < 4; ++j) wt[i].w[j] *= invSumWts;
            }
            return wt;
        };
        const std::vector<RW> xw = weights(img.w, nw), yw = weights(img.h, nh);
        const int nc = img.nc;
        // CopyRectOut's lookups: RemapPixelCoords with the texture's wrap mode, 0 outside for "black"
        auto fetch = [&](int x, int y, int c) -> float {
            if (wm == WF_WRAP_OCTAHEDRAL) {
                if (x < 0) { x = -x; y = img.h - 1 - y; } else if (x >= img.w) { x = 2 * img.w - 1 - x; y = img.h - 1 - y; }
                if (y < 0) { x = img.w - 1 - x; y = -y; } else if (y >= img.h) { x = img.w - 1 - x; y = 2 * img.h - 1 - y; }
                if (img.w == 1) x = 0;
                if (img.h == 1) y = 0;
            } else {
                auto mod = [](int a, int b) { int r = a - (a / b) * b; return r < 0 ? r + b : r; };
                if (x < 0 || x >= img.w) { if (wm == WF_WRAP_REPEAT) x = mod(x, img.w); else if (wm == WF_WRAP_CLAMP) x = std::min(std::max(x, 0), img.w - 1); else return 0.f; }
                if (y < 0 || y >= img.h) { if (wm == WF_WRAP_REPEAT) y = mod(y, img.h); else if (wm == WF_WRAP_CLAMP) y = std::min(std::max(y, 0), img.h - 1); else return 0.f; }
            }
            return img.Get(((size_t)y * img.w + x) * nc + c);
        };
        out->assign((size_t)nw * nh * nc, 0.f);
        std::vector<float> xrow((size_t)4 * nc);
        for (int y = 0; y < nh; ++y)
            for (int x = 0; x < nw; ++x) {
                const RW &rx = xw[x], &ry = yw[y];
                for (int j = 0; j < 4; ++j)
                    for (int c = 0; c < nc; ++c)
                        xrow[(size_t)j * nc + c] = rx.w[0] * fetch(rx.first, ry.first + j, c) + rx.w[1] * fetch(rx.first + 1, ry.first + j, c) +
                                                   rx.w[2] * fetch(rx.first + 2, ry.first + j, c) + rx.w[3] * fetch(rx.first + 3, ry.first + j, c);
                for (int c = 0; c < nc; ++c)
                    (*out)[((size_t)y * nw + x) * nc + c] = std::max(0.f, (ry.w[0] * xrow[c] + ry.w[1] * xrow[nc + c] + ry.w[2] * xrow[2 * nc + c] + ry.w[3] * xrow[3 * nc + c]));
            }
    }
    int LoadTexImage(const TextureEntity &te, wf_texture *t) {
        const ParamSet &ps = te.params;
        SetMapping2D(te, t);
        const float maxAniso = ps.GetOneFloat("maxanisotropy", 8.f);
        std::string filter = ps.GetOneString("filter", "bilinear"), wrap = ps.GetOneString("wrap", "repeat");
        // ParseFilter (util/mipmap.cpp:27-41)
        int ff = filter == "point" ? WF_MIP_POINT : filter == "bilinear" ? WF_MIP_BILINEAR : filter == "trilinear" ? WF_MIP_TRILINEAR :
                 (filter == "ewa" || filter == "EWA") ? WF_MIP_EWA : -1;
        if (ff < 0) Die(te.loc, filter + ": filter function unknown");
        int wm = wrap == "clamp" ? WF_WRAP_CLAMP : wrap == "repeat" ? WF_WRAP_REPEAT : wrap == "black" ? WF_WRAP_BLACK : wrap == "octahedralsphere" ? WF_WRAP_OCTAHEDRAL : -1;
        if (wm < 0) Die(te.loc, wrap + ": wrap mode unknown");
        t->f0 = ps.GetOneFloat("scale", 1.f);
        t->f1 = ps.GetOneBool("invert", false) ? 1.f : 0.f;
        std::string filename = ps.GetOneString("filename", "");
        if (filename.empty()) Die(te.loc, "imagemap texture without a filename");
        if (filename[0] != '/') filename = scene->baseDir + "/" + filename;
        // textures.cpp:436-438: 8-bit files default to sRGB, everything else to linear
        const bool isPng = filename.size() > 4 && (filename.substr(filename.size() - 4) == ".png" || filename.substr(filename.size() - 4) == ".PNG");
        const ColorEnc enc = ColorEnc::Parse(ps.GetOneString("encoding", isPng ? "sRGB" : "linear"));
        std::string key = filename + "|" + filter + "|" + wrap + "|" + enc.Key() + "|" + (ff == WF_MIP_EWA ? std::to_string(maxAniso) : "");
        auto it = imageCache.find(key);
        if (it != imageCache.end()) return it->second;
        HostImage img;
        try { ReadImage(filename, enc, &img); } catch (const SceneError &e) { Die(te.loc, std::string(e.what()).substr(7)); }
        // MIPMap::CreateFromFile: R G B, plus A unless it is 1 everywhere
        if (img.nc == 4) {
            bool allOne = true;
            for (size_t i = 0; i < (size_t)img.w * img.h && allOne; ++i) allOne = img.Get(i * 4 + 3) == 1;
            if (allOne) img.SelectChannels(0, 3);
        }
        const int nc = img.nc;
        int w = img.w, h = img.h;
        std::vector<float> level;
        if ((w & (w - 1)) || (h & (h - 1))) {
            auto roundUpPow2 = [](int v) { int r = 1; while (r < v) r *= 2; return r; };
            const int nw = roundUpPow2(w), nh = roundUpPow2(h);
            FloatResizeUp(img, wm, nw, nh, &level);
            w = nw; h = nh;
        } else {
            level.resize((size_t)w * h * nc);
            for (size_t i = 0; i < level.size(); ++i) level[i] = img.Get(i);   // ConvertToFormat(Float)
        }
        wf_tex_image im{};
        im.res[0] = w; im.res[1] = h; im.n_channels = nc; im.wrap = wm; im.filter = ff;
        im.max_anisotropy = maxAniso;
        im.format = img.format == HostImage::U256 ? WF_TEXEL_U8 : img.format == HostImage::Half ? WF_TEXEL_HALF : WF_TEXEL_FLOAT;
        if (getenv("WF_TEXELS_FLOAT")) { /* A/B and debugging: every image map as decoded floats, 4 bytes per texel */ im.format = WF_TEXEL_FLOAT; }
        if (im.format == WF_TEXEL_U8) {
            auto it = texelLutCache.find(img.enc.Key());
            if (it == texelLutCache.end()) {
                it = texelLutCache.emplace(img.enc.Key(), (int)T->tableData.size()).first;
                for (int code = 0; code < 256; ++code) T->tableData.push_back(img.enc.ToLinear((uint8_t)code));
            }
            im.lut_offset = it->second;
        }
        if (ff == WF_MIP_EWA) {
            // MIPFilterLUT (util/mipmap.cpp:45-191): the table's literals are exp(-2 r2) - exp(-2) in float, r2 = i / 127
            if (ewaLutOffset < 0) {
                ewaLutOffset = (int)T->tableData.size();
                for (int i = 0; i < 128; ++i) {
                    float alpha = 2, r2 = float(i) / float(127);
                    T->tableData.push_back(std::exp(-alpha * r2) - std::exp(-alpha));
                }
            }
            im.ewa_lut_offset = ewaLutOffset;
        }
        int lw = w, lh = h;
        im.n_levels = 1 + (31 - __builtin_clz((unsigned)std::max(w, h)));
        if (im.n_levels > 20) Die(te.loc, "texture too large");
        for (int l = 0; l < im.n_levels; ++l) {
            im.level_offset[l] = (int)T->tableData.size();
            if (im.format == WF_TEXEL_FLOAT) { for (float v : level) T->tableData.push_back(img.Quantize(v)); }   // (Float images: Quantize is the identity)
            else {
                // CopyRectIn into the level's format (util/image.cpp:370-372): the codes are stored, GetChannel's decode happens at the lookup
                const size_t bytesPer = img.format == HostImage::U256 ? 1 : 2, nBytes = level.size() * bytesPer;
                const size_t at = T->tableData.size();
                T->tableData.resize(at + (nBytes + 3) / 4, 0.f);
                uint8_t *dst = reinterpret_cast<uint8_t *>(&T->tableData[at]);
                if (bytesPer == 1) for (size_t i = 0; i < level.size(); ++i) dst[i] = (uint8_t)img.QuantizeCode(level[i]);
                else for (size_t i = 0; i < level.size(); ++i) { const uint16_t hb = (uint16_t)img.QuantizeCode(level[i]); memcpy(dst + 2 * i, &hb, 2); }
            }
            if (l == im.n_levels - 1) break;
            int nw = std::max(1, lw / 2), nh = std::max(1, lh / 2);
            std::vector<float> next((size_t)nw * nh * nc);
            int d1 = nc, d2 = nc * lw, d3 = nc * (lw + 1);
            if (lw == 1) { d1 = 0; d3 -= nc; }
            if (lh == 1) { d2 = 0; d3 -= nc * lw; }
            for (int y = 0; y < nh; ++y) {
                size_t src = (size_t)(2 * y) * lw * nc, dst = (size_t)y * nw * nc;
                for (int x = 0; x < nw; ++x, src += nc)
                    for (int c = 0; c < nc; ++c, ++src, ++dst)
                        next[dst] = (level[src] + level[src + d1] + level[src + d2] + level[src + d3]) / 4;
            }
            level.swap(next);
            lw = nw; lh = nh;
        }
        if (disableImageTextures) {
            // MIPMap ctor with Options->disableImageTextures (util/mipmap.cpp:199-203): the pyramid is its last (coarsest) level alone
            im.level_offset[0] = im.level_offset[im.n_levels - 1];
            im.n_levels = 1;
            im.res[0] = lw; im.res[1] = lh;
        }
        int id = (int)T->texImages.size();
        T->texImages.push_back(im);
        imageCache[key] = id;
        return id;
    }
    // BasicScene::startLoadingNormalMaps (scene.cpp:885-910): Image::Read with the linear encoding, the R G B channels,
    // read bilinearly at level 0 with repeat wrap by NormalMap()
    int LoadNormalMap(std::string filename, const std::string &loc) {
        if (filename.empty()) return -1;
        if (filename[0] != '/') filename = scene->baseDir + "/" + filename;
        std::string key = filename + "|normalmap";
        auto it = imageCache.find(key);
        if (it != imageCache.end()) return it->second;
        HostImage img;
        try { ReadImage(filename, ColorEnc::Linear(), &img); } catch (const SceneError &e) { Die(loc, std::string(e.what()).substr(7)); }
        if (img.nc < 3) Die(loc, filename + ": normal map image must contain R, G, and B channels");
        img.SelectChannels(0, 3);
        wf_tex_image im{};
        im.res[0] = img.w; im.res[1] = img.h; im.n_channels = 3; im.wrap = WF_WRAP_REPEAT; im.filter = WF_MIP_BILINEAR; im.n_levels = 1;
        im.level_offset[0] = (int)T->tableData.size();
        for (size_t i = 0; i < (size_t)img.w * img.h * 3; ++i) T->tableData.push_back(img.Get(i));
        int id = (int)T->texImages.size();
        T->texImages.push_back(im);
        imageCache[key] = id;
        return id;
    }
    void CreateNamedTextures() {
        for (const TextureEntity &te : scene->textures) {
            const ParamSet &ps = te.params;
            if (te.texType == "float") {
                wf_texture t{};
                t.spectrum = t.tex0 = t.tex1 = t.tex2 = -1;
                if (te.name == "constant") { t.type = WF_TEX_FLOAT_CONSTANT; t.f0 = ps.GetOneFloat("value", 1.f); }
                else if (te.name == "scale") {
                    t.type = WF_TEX_FLOAT_SCALE;
                    t.tex0 = GetFloatTexture(ps, "tex", 1.f);
                    t.tex1 = GetFloatTexture(ps, "scale", 1.f);
                    // FloatScaledTexture::Create (textures.cpp:892-925) folds a CONSTANT factor away: a factor of 1 returns the other
                    // texture itself, a constant times an image texture returns a copy of the image texture with its own scale multiplied
                    // (MultiplyScale) — in either argument order.  Not an optimisation only: the result is an image texture, which the
                    // wavefront path's BasicTextureEvaluator evaluates, and the factor is applied before `invert` (fuzz finding s600258).
                    int a = t.tex0, b = t.tex1, folded = -1;
                    for (int i = 0; i < 2 && folded < 0; ++i) {
                        if (T->textures[b].type == WF_TEX_FLOAT_CONSTANT) {
                            const float cs = T->textures[b].f0;
                            if (cs == 1) folded = a;
                            else if (T->textures[a].type == WF_TEX_FLOAT_IMAGE) { wf_texture c = T->textures[a]; c.f0 *= cs; folded = AddTex(c); }
                        }
                        std::swap(a, b);
                    }
                    if (folded >= 0) {
                        if (floatTextures.count(te.texName)) Die(te.loc, "Redefining texture \"" + te.texName + "\".");
                        floatTextures[te.texName] = folded;
                        ps.ReportUnused("Texture");
                        continue;
                    }
                } else if (te.name == "mix") {
                    t.type = WF_TEX_FLOAT_MIX;
                    t.tex0 = GetFloatTexture(ps, "tex1", 0.f);
                    t.tex1 = GetFloatTexture(ps, "tex2", 1.f);
                    t.tex2 = GetFloatTexture(ps, "amount", 0.5f);
                } else if (te.name == "imagemap") {
                    // FloatImageTexture::Create (textures.cpp:335-370)
                    t.type = WF_TEX_FLOAT_IMAGE;
                    t.i0 = LoadTexImage(te, &t);
                } else if (te.name == "checkerboard") {
                    // FloatCheckerboardTexture::Create (textures.cpp:219-241)
                    CheckerMapping(te, &t);
                    t.type = WF_TEX_FLOAT_CHECKERBOARD;
                    t.tex0 = GetFloatTexture(ps, "tex1", 1.f);
                    t.tex1 = GetFloatTexture(ps, "tex2", 0.f);
                } else if (te.name == "bilerp") {
                    // FloatBilerpTexture::Create (textures.cpp:141-151)
                    SetMapping2D(te, &t);
                    t.type = WF_TEX_FLOAT_BILERP;
                    t.f0 = ps.GetOneFloat("v00", 0.f); t.f1 = ps.GetOneFloat("v01", 1.f);
                    t.map[10] = ps.GetOneFloat("v10", 0.f); t.map[11] = ps.GetOneFloat("v11", 1.f);
                } else if (te.name == "directionmix") {
                    // FloatDirectionMixTexture::Create (textures.cpp:563-571); stored as a mix with weight |n . dir|
                    t.type = WF_TEX_FLOAT_DIRECTIONMIX;
                    V3 dir = Normalize(te.renderFromTexture.Vector(ps.GetOneVector3f("dir", V3{0, 1, 0})));
                    t.map[4] = dir.x; t.map[5] = dir.y; t.map[6] = dir.z;
                    t.tex1 = GetFloatTexture(ps, "tex1", 0.f);
                    t.tex0 = GetFloatTexture(ps, "tex2", 1.f);
                } else if (te.name == "fbm" || te.name == "wrinkled") {
                    // FBmTexture::Create / WrinkledTexture::Create (textures.cpp:343-351, 980-988)
                    NeedNoise();
                    SetMapping3D(te, &t);
                    t.type = te.name == "fbm" ? WF_TEX_FLOAT_FBM : WF_TEX_FLOAT_WRINKLED;
                    t.i0 = ps.GetOneInt("octaves", 8);
                    t.f0 = ps.GetOneFloat("roughness", .5f);
                } else if (te.name == "windy") {
                    NeedNoise();
                    SetMapping3D(te, &t);
                    t.type = WF_TEX_FLOAT_WINDY;
                } else if (te.name == "dots") {
                    // FloatDotsTexture::Create (textures.cpp:305-315) hands ("inside", "outside") to a constructor declared
                    // (mapping, outsideDot, insideDot) (textures.h:429-431): inside a dot the reference evaluates the "outside" parameter
                    NeedNoise();
                    SetMapping2D(te, &t);
                    t.type = WF_TEX_FLOAT_DOTS;
                    t.tex0 = GetFloatTexture(ps, "inside", 1.f);
                    t.tex1 = GetFloatTexture(ps, "outside", 0.f);
                } else Die(te.loc, te.name + ": float texture type not supported by this build");
                if (floatTextures.count(te.texName)) Die(te.loc, "Redefining texture \"" + te.texName + "\".");
                floatTextures[te.texName] = AddTex(t);
                ps.ReportUnused("Texture");   // FloatTexture::Create, textures.cpp:1490
            } else {
                // the reference instantiates each spectrum texture three times, once per SpectrumType
                for (SpectrumType st : {SpectrumType::Albedo, SpectrumType::Unbounded, SpectrumType::Illuminant}) {
                    wf_texture t{};
                    t.spectrum = t.tex0 = t.tex1 = t.tex2 = -1;
                    if (te.name == "constant") {
                        SpectrumP one = MakeConstant(1.f);
                        SpectrumP s = ps.GetOneSpectrum("value", one, st);
                        t.type = WF_TEX_SPECTRUM_CONSTANT; t.spectrum = T->pool.Add(*s);
                    } else if (te.name == "scale") {
                        t.type = WF_TEX_SPECTRUM_SCALE;
                        t.tex0 = GetSpectrumTexture(ps, "tex", *MakeConstant(1.f), st);
                        t.tex1 = GetFloatTexture(ps, "scale", 1.f);
                        // SpectrumScaledTexture::Create (textures.cpp:927-957): a constant factor of 1 returns `tex` itself, a constant times
                        // an image texture returns a copy of the image texture with the factor in its own scale — applied to the RGB texel
                        // BEFORE `invert`, the clamp and the RGB -> spectrum conversion, and evaluated by the BasicTextureEvaluator
                        // (fuzz finding s600258: a diffuse transmittance 9.6 % off)
                        if (T->textures[t.tex1].type == WF_TEX_FLOAT_CONSTANT) {
                            const float cs = T->textures[t.tex1].f0;
                            int folded = -1;
                            if (cs == 1) folded = t.tex0;
                            else if (T->textures[t.tex0].type == WF_TEX_SPECTRUM_IMAGE) { wf_texture c = T->textures[t.tex0]; c.f0 *= cs; folded = AddTex(c); }
                            if (folded >= 0) {
                                auto &fm = SpecMap(st);
                                if (st == SpectrumType::Albedo && fm.count(te.texName)) Die(te.loc, "Redefining texture \"" + te.texName + "\".");
                                fm[te.texName] = folded;
                                ps.ReportUnused("Texture");
                                continue;
                            }
                        }
                    } else if (te.name == "mix") {
                        t.type = WF_TEX_SPECTRUM_MIX;
                        t.tex0 = GetSpectrumTexture(ps, "tex1", *MakeConstant(0.f), st);
                        t.tex1 = GetSpectrumTexture(ps, "tex2", *MakeConstant(1.f), st);
                        t.tex2 = GetFloatTexture(ps, "amount", 0.5f);
                    } else if (te.name == "imagemap") {
                        // SpectrumImageTexture::Create (textures.cpp:372-407); the PFM carries no colour space -> sRGB
                        t.type = WF_TEX_SPECTRUM_IMAGE;
                        t.i0 = LoadTexImage(te, &t);
                        t.spectrum = st == SpectrumType::Albedo ? 0 : (st == SpectrumType::Unbounded ? 1 : 2);
                        const ColorSpace *ics = SpectralData::Get().sRGB();
                        T->desc.rgb2spec_coeffs = ics->table->coeffs.data();
                        for (int i = 0; i < 64; ++i) T->desc.rgb2spec_znodes[i] = ics->table->zNodes[i];
                        T->desc.cs_illuminant_offset = T->pool.AddDense(*ics->illuminant);
                    } else if (te.name == "checkerboard") {
                        // SpectrumCheckerboardTexture::Create (textures.cpp:250-278)
                        CheckerMapping(te, &t);
                        t.type = WF_TEX_SPECTRUM_CHECKERBOARD;
                        t.tex0 = GetSpectrumTexture(ps, "tex1", *MakeConstant(1.f), st);
                        t.tex1 = GetSpectrumTexture(ps, "tex2", *MakeConstant(0.f), st);
                    } else if (te.name == "bilerp") {
                        // SpectrumBilerpTexture::Create (textures.cpp:159-174)
                        SetMapping2D(te, &t);
                        t.type = WF_TEX_SPECTRUM_BILERP;
                        SpectrumP zero = MakeConstant(0.f), one = MakeConstant(1.f);
                        t.spectrum = T->pool.Add(*ps.GetOneSpectrum("v00", zero, st));
                        t.tex1 = T->pool.Add(*ps.GetOneSpectrum("v01", one, st));
                        t.tex0 = T->pool.Add(*ps.GetOneSpectrum("v10", zero, st));
                        t.tex2 = T->pool.Add(*ps.GetOneSpectrum("v11", one, st));
                    } else if (te.name == "directionmix") {
                        // SpectrumDirectionMixTexture::Create (textures.cpp:573-583)
                        t.type = WF_TEX_SPECTRUM_DIRECTIONMIX;
                        V3 dir = Normalize(te.renderFromTexture.Vector(ps.GetOneVector3f("dir", V3{0, 1, 0})));
                        t.map[4] = dir.x; t.map[5] = dir.y; t.map[6] = dir.z;
                        t.tex1 = GetSpectrumTexture(ps, "tex1", *MakeConstant(0.f), st);
                        t.tex0 = GetSpectrumTexture(ps, "tex2", *MakeConstant(1.f), st);
                    } else if (te.name == "marble") {
                        // MarbleTexture::Create (textures.cpp:511-520); the same texture for every SpectrumType
                        NeedNoise();
                        NeedSRGBTable();
                        SetMapping3D(te, &t);
                        t.type = WF_TEX_SPECTRUM_MARBLE;
                        t.i0 = ps.GetOneInt("octaves", 8);
                        t.f0 = ps.GetOneFloat("roughness", .5f);
                        t.f1 = ps.GetOneFloat("scale", 1.f);
                        t.map[10] = ps.GetOneFloat("variation", .2f);
                    } else if (te.name == "dots") {
                        // SpectrumDotsTexture::Create (textures.cpp:322-334): same argument swap as the float variant
                        NeedNoise();
                        SetMapping2D(te, &t);
                        t.type = WF_TEX_SPECTRUM_DOTS;
                        t.tex0 = GetSpectrumTexture(ps, "inside", *MakeConstant(1.f), st);
                        t.tex1 = GetSpectrumTexture(ps, "outside", *MakeConstant(0.f), st);
                    } else Die(te.loc, te.name + ": spectrum texture type not supported by this build");
                    auto &m = SpecMap(st);
                    if (st == SpectrumType::Albedo && m.count(te.texName)) Die(te.loc, "Redefining texture \"" + te.texName + "\".");
                    m[te.texName] = AddTex(t);
                    ps.ReportUnused("Texture");   // SpectrumTexture::Create, textures.cpp:1545
                }
            }
        }
    }

    SpectrumP GetEta(const ParamSet &ps, const std::string &name) {
        std::vector<float> fa = ps.GetFloatArray(name);
        if (!fa.empty()) return MakeConstant(fa[0]);
        SpectrumP eta = ps.GetOneSpectrum(name, nullptr, SpectrumType::Unbounded);
        if (!eta) eta = MakeConstant(1.5f);
        return eta;
    }

    int CreateMaterial(const Entity &e) {
        const ParamSet &ps = e.params;
        wf_material m{};
        for (int &t : m.tex) t = -1;
        m.eta_spectrum = -1;
        const std::string &name = e.name;
        // "normalmap" is looked up for every material (scene.cpp:1142,1159), "displacement" by the Create() of the types that have one
        // (materials.cpp: every type but hair, mix and interface) — which decides whether a stray one is an unused parameter
        m.displacement = -1;
        if (name != "hair" && name != "mix" && name != "interface" && name != "none" && !name.empty()) m.displacement = GetFloatTextureOrNull(ps, "displacement");
        m.normalmap = LoadNormalMap(ps.GetOneString("normalmap", ""), e.loc);
        auto roughness = [&](const char *u, const char *v, const char *r, int us, int vs) {
            int ur = GetFloatTextureOrNull(ps, u), vr = GetFloatTextureOrNull(ps, v);
            if (ur < 0) ur = GetFloatTexture(ps, r, 0.f);
            if (vr < 0) vr = GetFloatTexture(ps, r, 0.f);
            m.tex[us] = ur; m.tex[vs] = vr;
        };
        auto conductorParams = [&](const char *etaName, const char *kName, int etaSlot, int kSlot) {
            int eta = GetSpectrumTextureOrNull(ps, etaName, SpectrumType::Unbounded);
            int k = GetSpectrumTextureOrNull(ps, kName, SpectrumType::Unbounded);
            int refl = GetSpectrumTextureOrNull(ps, "reflectance", SpectrumType::Albedo);
            if (refl >= 0 && (eta >= 0 || k >= 0)) Die(e.loc, "both \"reflectance\" and \"eta\" and \"k\" can't be provided.");
            if (refl < 0) {
                if (eta < 0) eta = SpectrumConst(*SpectralData::Get().Named("metal-Cu-eta"));
                if (k < 0) k = SpectrumConst(*SpectralData::Get().Named("metal-Cu-k"));
            } else m.flags |= WF_MATFLAG_CONDUCTOR_REFLECTANCE;
            m.tex[etaSlot] = eta; m.tex[kSlot] = k; m.tex[WF_MT_REFLECTANCE] = refl;
        };
        if (name == "diffuse") {
            m.type = WF_MAT_DIFFUSE;
            m.tex[WF_MT_REFLECTANCE] = GetSpectrumTexture(ps, "reflectance", *MakeConstant(0.5f), SpectrumType::Albedo);
        } else if (name == "conductor") {
            m.type = WF_MAT_CONDUCTOR;
            conductorParams("eta", "k", WF_MT_ETA, WF_MT_K);
            roughness("uroughness", "vroughness", "roughness", WF_MT_UROUGH, WF_MT_VROUGH);
            if (ps.GetOneBool("remaproughness", true)) m.flags |= WF_MATFLAG_REMAP_ROUGHNESS;
        } else if (name == "dielectric") {
            m.type = WF_MAT_DIELECTRIC;
            m.eta_spectrum = T->pool.Add(*GetEta(ps, "eta"));
            roughness("uroughness", "vroughness", "roughness", WF_MT_UROUGH, WF_MT_VROUGH);
            if (ps.GetOneBool("remaproughness", true)) m.flags |= WF_MATFLAG_REMAP_ROUGHNESS;
        } else if (name == "thindielectric") {
            m.type = WF_MAT_THIN_DIELECTRIC;
            m.eta_spectrum = T->pool.Add(*GetEta(ps, "eta"));
        } else if (name == "diffusetransmission") {
            m.type = WF_MAT_DIFFUSE_TRANSMISSION;
            m.tex[WF_MT_REFLECTANCE] = GetSpectrumTexture(ps, "reflectance", *MakeConstant(0.25f), SpectrumType::Albedo);
            m.tex[WF_MT_TRANSMITTANCE] = GetSpectrumTexture(ps, "transmittance", *MakeConstant(0.25f), SpectrumType::Albedo);
            m.scale = ps.GetOneFloat("scale", 1.f);
        } else if (name == "coateddiffuse") {
            m.type = WF_MAT_COATED_DIFFUSE;
            m.tex[WF_MT_REFLECTANCE] = GetSpectrumTexture(ps, "reflectance", *MakeConstant(0.5f), SpectrumType::Albedo);
            roughness("uroughness", "vroughness", "roughness", WF_MT_UROUGH, WF_MT_VROUGH);
            m.tex[WF_MT_THICKNESS] = GetFloatTexture(ps, "thickness", .01f);
            m.eta_spectrum = T->pool.Add(*GetEta(ps, "eta"));
            m.maxdepth = ps.GetOneInt("maxdepth", 10);
            m.nsamples = ps.GetOneInt("nsamples", 1);
            m.tex[WF_MT_G] = GetFloatTexture(ps, "g", 0.f);
            m.tex[WF_MT_ALBEDO] = GetSpectrumTexture(ps, "albedo", *MakeConstant(0.f), SpectrumType::Albedo);
            if (ps.GetOneBool("remaproughness", true)) m.flags |= WF_MATFLAG_REMAP_ROUGHNESS;
        } else if (name == "coatedconductor") {
            m.type = WF_MAT_COATED_CONDUCTOR;
            roughness("interface.uroughness", "interface.vroughness", "interface.roughness", WF_MT_UROUGH, WF_MT_VROUGH);
            m.tex[WF_MT_THICKNESS] = GetFloatTexture(ps, "thickness", .01f);
            m.eta_spectrum = T->pool.Add(*GetEta(ps, "interface.eta"));
            roughness("conductor.uroughness", "conductor.vroughness", "conductor.roughness", WF_MT_COND_UROUGH, WF_MT_COND_VROUGH);
            conductorParams("conductor.eta", "conductor.k", WF_MT_COND_ETA, WF_MT_COND_K);
            m.maxdepth = ps.GetOneInt("maxdepth", 10);
            m.nsamples = ps.GetOneInt("nsamples", 1);
            m.tex[WF_MT_G] = GetFloatTexture(ps, "g", 0.f);
            m.tex[WF_MT_ALBEDO] = GetSpectrumTexture(ps, "albedo", *MakeConstant(0.f), SpectrumType::Albedo);
            if (ps.GetOneBool("remaproughness", true)) m.flags |= WF_MATFLAG_REMAP_ROUGHNESS;
        } else if (name == "subsurface") {
            // SubsurfaceMaterial::Create (materials.cpp:498-567)
            m.type = WF_MAT_SUBSURFACE;
            float g = ps.GetOneFloat("g", 0.f);
            int sigma_a = -1, sigma_s = -1;
            if (std::string pname = ps.GetOneString("name", ""); !pname.empty()) {
                // 1. by name: the measured coefficients are reduced scattering coefficients, so g is forced to 0
                SpectrumP pa, psc;
                if (!MediumPreset(pname, &pa, &psc)) Die(e.loc, pname + ": named medium not found.");
                g = 0;
                sigma_a = SpectrumConst(*pa);
                sigma_s = SpectrumConst(*psc);
            } else {
                sigma_a = GetSpectrumTextureOrNull(ps, "sigma_a", SpectrumType::Unbounded);
                sigma_s = GetSpectrumTextureOrNull(ps, "sigma_s", SpectrumType::Unbounded);
            }
            if (sigma_a >= 0 && sigma_s < 0) Die(e.loc, "Provided \"sigma_a\" parameter without \"sigma_s\".");
            if (sigma_s >= 0 && sigma_a < 0) Die(e.loc, "Provided \"sigma_s\" parameter without \"sigma_a\".");
            if (sigma_a < 0) {
                int refl = GetSpectrumTextureOrNull(ps, "reflectance", SpectrumType::Albedo);
                if (refl >= 0) {
                    m.tex[WF_MT_REFLECTANCE] = refl;
                    m.tex[WF_MT_MFP] = GetSpectrumTexture(ps, "mfp", *MakeConstant(1.f), SpectrumType::Unbounded);
                } else {
                    // RGBUnboundedSpectrum(*RGBColorSpace::sRGB, ...) whatever the scene's colour space is
                    const float a[3] = {.0011f, .0024f, .014f}, sc[3] = {2.55f, 3.21f, 3.77f};
                    sigma_a = SpectrumConst(*SpectralData::Get().sRGB()->Unbounded(a));
                    sigma_s = SpectrumConst(*SpectralData::Get().sRGB()->Unbounded(sc));
                }
            }
            if (sigma_a >= 0) { m.tex[WF_MT_SIGMA_A] = sigma_a; m.tex[WF_MT_SIGMA_S] = sigma_s; m.flags |= WF_MATFLAG_SSS_COEFFICIENTS; }
            m.scale = ps.GetOneFloat("scale", 1.f);
            m.sss_eta = ps.GetOneFloat("eta", 1.33f);
            roughness("uroughness", "vroughness", "roughness", WF_MT_UROUGH, WF_MT_VROUGH);
            if (ps.GetOneBool("remaproughness", true)) m.flags |= WF_MATFLAG_REMAP_ROUGHNESS;
            // the material's BSSRDFTable (materials.h:719-720)
            std::vector<float> table(wf::BSSRDF_TABLE_FLOATS);
            wf::ComputeBeamDiffusionBSSRDF(g, m.sss_eta, table.data());
            m.sss_table = (int)T->tableData.size();
            T->tableData.insert(T->tableData.end(), table.begin(), table.end());
        } else if (name == "hair") {
            // HairMaterial::Create (materials.cpp:135-184)
            m.type = WF_MAT_HAIR;
            int sigma_a = GetSpectrumTextureOrNull(ps, "sigma_a", SpectrumType::Unbounded);
            int refl = GetSpectrumTextureOrNull(ps, "reflectance", SpectrumType::Albedo);
            if (refl < 0) refl = GetSpectrumTextureOrNull(ps, "color", SpectrumType::Albedo);
            int eu = GetFloatTextureOrNull(ps, "eumelanin"), ph = GetFloatTextureOrNull(ps, "pheomelanin");
            if (sigma_a >= 0) { refl = eu = ph = -1; }
            else if (refl >= 0) { eu = ph = -1; }
            else if (eu < 0 && ph < 0) {
                // default: brown-ish hair, RGBUnboundedSpectrum(SigmaAFromConcentration(1.3, 0)) in sRGB
                const float rgb[3] = {1.3f * 0.419f + 0.f * 0.187f, 1.3f * 0.697f + 0.f * 0.4f, 1.3f * 1.37f + 0.f * 1.05f};
                sigma_a = SpectrumConst(*SpectralData::Get().sRGB()->Unbounded(rgb));
            }
            m.tex[WF_MT_SIGMA_A] = sigma_a; m.tex[WF_MT_REFLECTANCE] = refl;
            m.tex[WF_MT_HAIR_EUMELANIN] = eu; m.tex[WF_MT_HAIR_PHEOMELANIN] = ph;
            if (eu >= 0 || ph >= 0) NeedSRGBTable();
            m.tex[WF_MT_HAIR_ETA] = GetFloatTexture(ps, "eta", 1.55f);
            m.tex[WF_MT_HAIR_BETA_M] = GetFloatTexture(ps, "beta_m", 0.3f);
            m.tex[WF_MT_HAIR_BETA_N] = GetFloatTexture(ps, "beta_n", 0.3f);
            m.tex[WF_MT_HAIR_ALPHA] = GetFloatTexture(ps, "alpha", 2.f);
            m.displacement = -1; m.normalmap = -1;   // GetDisplacement() / GetNormalMap() return null
        } else if (name == "measured") {
            // MeasuredMaterial::Create (materials.cpp:610-621); the data of one file is shared by its materials (MeasuredBxDF::BRDFDataFromFile, bxdfs.cpp:974-980)
            m.type = WF_MAT_MEASURED;
            std::string filename = ps.GetOneString("filename", "");
            if (filename.empty()) Die(e.loc, "Filename must be provided for MeasuredMaterial");
            if (filename[0] != '/') filename = scene->baseDir + "/" + filename;
            auto it = measuredCache.find(filename);
            if (it == measuredCache.end()) {
                int at = -1;
                try { at = ReadMeasuredBRDF(filename, &T->tableData); } catch (const SceneError &err) { Die(e.loc, std::string(err.what()).substr(7)); }
                it = measuredCache.emplace(filename, at).first;
            }
            m.measured_table = it->second;
        } else if (name == "interface" || name == "none" || name.empty()) {
            m.type = WF_MAT_INTERFACE;
        } else if (name == "mix") {
            // Material::Create "mix" (materials.cpp:664-681) + MixMaterial::Create (:105-125)
            m.type = WF_MAT_MIX;
            std::vector<std::string> names = ps.GetStringArray("materials");
            if (names.size() != 2) Die(e.loc, "Must provide two values for \"string materials\" for mix material.");
            for (int i = 0; i < 2; ++i) {
                auto it = namedMaterialIds.find(names[i]);
                if (it == namedMaterialIds.end()) Die(e.loc, names[i] + ": named material not found.");
                if (T->materials[it->second].type == WF_MAT_INTERFACE)
                    Die(e.loc, names[i] + ": an \"interface\" material cannot be used as an element of the \"mix\" material.");
                m.mix[i] = it->second;
            }
            m.tex[WF_MT_AMOUNT] = GetFloatTexture(ps, "amount", 0.5f);
            ps.ReportUnused("Material");
            // updateMaterialNeeds (wavefront/integrator.cpp:55-61) runs over every created material: the wavefront path refuses a mix whose
            // amount the BasicTextureEvaluator cannot evaluate (textures.h:1162-1177: a constant or an image map)
            if (const int ty = T->textures[m.tex[WF_MT_AMOUNT]].type; ty != WF_TEX_FLOAT_CONSTANT && ty != WF_TEX_FLOAT_IMAGE)
                Die(e.loc, "\"mix\" material has a texture that can't be evaluated with the BasicTextureEvaluator, which is all that is currently supported "
                           "int the wavefront renderer--sorry!");
            T->materials.push_back(m);
            return (int)T->materials.size() - 1;
        } else Die(e.loc, name + ": material type unknown.");
        if (m.type != WF_MAT_INTERFACE) ps.ReportUnused("Material");   // Material::Create, materials.cpp:688 ("interface" returns before it)
        T->materialTypePresent[m.type] = true;
        T->materials.push_back(m);
        return (int)T->materials.size() - 1;
    }
};

// ---- filter ---------------------------------------------------------------------------------------
struct FilterH {
    int type;
    float rx, ry, sigma = 0.5f, expX = 0, expY = 0, b = 1.f / 3.f, c = 1.f / 3.f, tau = 3.f;
    static float Sinc(float x) {  // util/math.h:227-231, SinXOverX :340-344
        float px = Pi * x;
        if (1 - px * px == 1) return 1;
        return std::sin(px) / px;
    }
    static float WindowedSinc(float x, float radius, float tau) {
        if (std::abs(x) > radius) return 0;
        return Sinc(x) * Sinc(x / tau);
    }
    float Mitchell1D(float x) const {
        x = std::abs(x);
        if (x <= 1) return ((12 - 9 * b - 6 * c) * x * x * x + (-18 + 12 * b + 6 * c) * x * x + (6 - 2 * b)) * (1.f / 6.f);
        else if (x <= 2) return ((-b - 6 * c) * x * x * x + (6 * b + 30 * c) * x * x + (-12 * b - 48 * c) * x + (8 * b + 24 * c)) * (1.f / 6.f);
        else return 0;
    }
    float Evaluate(float px, float py) const {
        switch (type) {
        case WF_FILTER_BOX: return (std::abs(px) <= rx && std::abs(py) <= ry) ? 1 : 0;
        case WF_FILTER_GAUSSIAN: return std::max<float>(0, Gaussian(px, 0, sigma) - expX) * std::max<float>(0, Gaussian(py, 0, sigma) - expY);
        case WF_FILTER_MITCHELL: return Mitchell1D(2 * px / rx) * Mitchell1D(2 * py / ry);
        case WF_FILTER_SINC: return WindowedSinc(px, rx, tau) * WindowedSinc(py, ry, tau);
        case WF_FILTER_TRIANGLE: return std::max<float>(0, rx - std::abs(px)) * std::max<float>(0, ry - std::abs(py));
        }
        return 0;
    }
};

// PiecewiseConstant1D construction (util/sampling.h:620-645)
void BuildPC1D(const float *f, int n, float mn, float mx, std::vector<float> *func, std::vector<float> *cdf, float *funcInt) {
    func->assign(f, f + n);
    cdf->assign(n + 1, 0.f);
    for (float &v : *func) v = std::abs(v);
    (*cdf)[0] = 0;
    for (int i = 1; i < n + 1; ++i) (*cdf)[i] = (*cdf)[i - 1] + (*func)[i - 1] * (mx - mn) / n;
    *funcInt = (*cdf)[n];
    if (*funcInt == 0) for (int i = 1; i < n + 1; ++i) (*cdf)[i] = float(i) / float(n);
    else for (int i = 1; i < n + 1; ++i) (*cdf)[i] /= *funcInt;
}

void BuildFilter(const ParsedScene &scene, SceneTables *T) {
    const Entity &e = scene.filter;
    const ParamSet &ps = e.params;
    FilterH f{};
    wf_filter &wfF = T->desc.filter;
    if (e.name == "box") { f.type = WF_FILTER_BOX; f.rx = ps.GetOneFloat("xradius", 0.5f); f.ry = ps.GetOneFloat("yradius", 0.5f); }
    else if (e.name == "gaussian") {
        f.type = WF_FILTER_GAUSSIAN; f.rx = ps.GetOneFloat("xradius", 1.5f); f.ry = ps.GetOneFloat("yradius", 1.5f);
        f.sigma = ps.GetOneFloat("sigma", 0.5f);
        f.expX = Gaussian(f.rx, 0, f.sigma); f.expY = Gaussian(f.ry, 0, f.sigma);
    } else if (e.name == "mitchell") {
        f.type = WF_FILTER_MITCHELL; f.rx = ps.GetOneFloat("xradius", 2.f); f.ry = ps.GetOneFloat("yradius", 2.f);
        f.b = ps.GetOneFloat("B", 1.f / 3.f); f.c = ps.GetOneFloat("C", 1.f / 3.f);
    } else if (e.name == "sinc") {
        f.type = WF_FILTER_SINC; f.rx = ps.GetOneFloat("xradius", 4.f); f.ry = ps.GetOneFloat("yradius", 4.f);
        f.tau = ps.GetOneFloat("tau", 3.f);
    } else if (e.name == "triangle") { f.type = WF_FILTER_TRIANGLE; f.rx = ps.GetOneFloat("xradius", 2.f); f.ry = ps.GetOneFloat("yradius", 2.f); }
    else Die(e.loc, e.name + ": filter type unknown.");
    ps.ReportUnused("PixelFilter");
    wfF.type = f.type; wfF.radius[0] = f.rx; wfF.radius[1] = f.ry;
    wfF.domain_min[0] = -f.rx; wfF.domain_min[1] = -f.ry; wfF.domain_max[0] = f.rx; wfF.domain_max[1] = f.ry;
    wfF.nx = wfF.ny = 0;
    if (f.type == WF_FILTER_BOX || f.type == WF_FILTER_TRIANGLE) return;  // analytic Sample()
    // FilterSampler (filters.cpp:133-147)
    int nx = int(32 * f.rx), ny = int(32 * f.ry);
    wfF.nx = nx; wfF.ny = ny;
    std::vector<float> tab((size_t)nx * ny);
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            float tx = (x + 0.5f) / nx, ty = (y + 0.5f) / ny;
            // Bounds2f::Lerp: (Lerp(t.x, pMin.x, pMax.x), Lerp(t.y, pMin.y, pMax.y))
            float px = Lerp(tx, -f.rx, f.rx), py = Lerp(ty, -f.ry, f.ry);
            tab[(size_t)y * nx + x] = f.Evaluate(px, py);
        }
    std::vector<float> &D = T->filterData;
    wfF.f_offset = (int)D.size();
    D.insert(D.end(), tab.begin(), tab.end());
    // PiecewiseConstant2D (util/sampling.h:706-722)
    std::vector<float> condFunc, condCdf, condInt(ny);
    for (int v = 0; v < ny; ++v) {
        std::vector<float> fn, cdf;
        float fi;
        BuildPC1D(&tab[(size_t)v * nx], nx, -f.rx, f.rx, &fn, &cdf, &fi);
        condFunc.insert(condFunc.end(), fn.begin(), fn.end());
        condCdf.insert(condCdf.end(), cdf.begin(), cdf.end());
        condInt[v] = fi;
    }
    std::vector<float> mFunc, mCdf;
    float mInt;
    BuildPC1D(condInt.data(), ny, -f.ry, f.ry, &mFunc, &mCdf, &mInt);
    wfF.cond_func_offset = (int)D.size(); D.insert(D.end(), condFunc.begin(), condFunc.end());
    wfF.cond_cdf_offset = (int)D.size(); D.insert(D.end(), condCdf.begin(), condCdf.end());
    wfF.cond_int_offset = (int)D.size(); D.insert(D.end(), condInt.begin(), condInt.end());
    wfF.marg_func_offset = (int)D.size(); D.insert(D.end(), mFunc.begin(), mFunc.end());
    wfF.marg_cdf_offset = (int)D.size(); D.insert(D.end(), mCdf.begin(), mCdf.end());
    wfF.marg_int = mInt;
}

// PiecewiseConstant2D over [0,1]^2 (util/sampling.h:706-722) of a w x h function, appended to a float table
static wf_pc2d AppendPC2D(std::vector<float> *Dp, const std::vector<float> &f, int w, int h) {
    wf_pc2d t{};
    t.nx = w; t.ny = h;
    std::vector<float> condFunc, condCdf, condInt(h), mFunc, mCdf;
    for (int v = 0; v < h; ++v) {
        std::vector<float> fn, cdf;
        float fi;
        BuildPC1D(&f[(size_t)v * w], w, 0.f, 1.f, &fn, &cdf, &fi);
        condFunc.insert(condFunc.end(), fn.begin(), fn.end());
        condCdf.insert(condCdf.end(), cdf.begin(), cdf.end());
        condInt[v] = fi;
    }
    BuildPC1D(condInt.data(), h, 0.f, 1.f, &mFunc, &mCdf, &t.marg_int);
    std::vector<float> &D = *Dp;
    t.cond_func_offset = (int)D.size(); D.insert(D.end(), condFunc.begin(), condFunc.end());
    t.cond_cdf_offset = (int)D.size(); D.insert(D.end(), condCdf.begin(), condCdf.end());
    t.cond_int_offset = (int)D.size(); D.insert(D.end(), condInt.begin(), condInt.end());
    t.marg_func_offset = (int)D.size(); D.insert(D.end(), mFunc.begin(), mFunc.end());
    t.marg_cdf_offset = (int)D.size(); D.insert(D.end(), mCdf.begin(), mCdf.end());
    return t;
}

// ---- film / sampler / camera -------------------------------------------------------------------------
void BuildFilm(const ParsedScene &scene, const RenderOptions &opt, SceneTables *T) {
    const ParamSet &ps = scene.film.params;
    if (scene.film.name != "rgb" && scene.film.name != "spectral" && scene.film.name != "gbuffer")
        Die(scene.film.loc, scene.film.name + ": film type not supported by this build (rgb, gbuffer, spectral)");
    wf_film &F = T->desc.film;
    F.type = scene.film.name == "spectral" ? WF_FILM_SPECTRAL : scene.film.name == "gbuffer" ? WF_FILM_GBUFFER : WF_FILM_RGB;
    F.apply_inverse = 0;
    if (F.type == WF_FILM_GBUFFER) {
        // GBufferFilm::Create (film.cpp:806-846); the transform itself is set once the camera is known (BuildSceneTables)
        const std::string cs = ps.GetOneString("coordinatesystem", "camera");
        if (cs != "camera" && cs != "world") Die(scene.film.loc, cs + ": unknown coordinate system for GBufferFilm. (Expecting \"camera\" or \"world\".)");
        F.apply_inverse = cs == "camera" ? 1 : 0;
    }
    F.n_buckets = 0;
    F.lambda_min = 360.f; F.lambda_max = 830.f;
    if (F.type == WF_FILM_SPECTRAL) {
        // SpectralFilm::Create (film.cpp:1037-1069)
        F.n_buckets = ps.GetOneInt("nbuckets", 16);
        F.lambda_min = ps.GetOneFloat("lambdamin", 360.f);
        F.lambda_max = ps.GetOneFloat("lambdamax", 830.f);
        if (F.lambda_min < 360.f || F.lambda_max > 830.f) Die(scene.film.loc, "Unfortunately pbrt must be recompiled to render wavelengths beyond the [360,830] range");
        if (F.n_buckets < 1) Die(scene.film.loc, "spectral film: \"nbuckets\" must be positive");
    }
    float exposureTime = scene.camera.params.GetOneFloat("shutterclose", 1.f) - scene.camera.params.GetOneFloat("shutteropen", 0.f);
    F.max_component_value = ps.GetOneFloat("maxcomponentvalue", WF_INFINITY);
    T->saveFP16 = ps.GetOneBool("savefp16", true);
    // PixelSensor::Create (film.cpp:213-253)
    float ISO = ps.GetOneFloat("iso", 100.f);
    float whiteBalanceTemp = ps.GetOneFloat("whitebalance", 0);
    std::string sensorName = ps.GetOneString("sensor", "cie1931");
    // "Pass through 0 for cie1931 if it's unspecified so that it doesn't do any white balancing. For actual sensors, 6500 is the default"
    if (sensorName != "cie1931" && whiteBalanceTemp == 0) whiteBalanceTemp = 6500;
    F.imaging_ratio = exposureTime * ISO / 100;
    const SpectralData &sd = SpectralData::Get();
    const ColorSpace *cs = scene.filmColorSpace;
    Mat3 XYZFromSensorRGB = Mat3::Identity();
    SpectrumP rBar = sd.X, gBar = sd.Y, bBar = sd.Z;
    if (sensorName != "cie1931") {
        // PixelSensor ctor for a measured sensor (film.h:45-78): the response curves densely sampled, XYZFromSensorRGB = the linear
        // least-squares fit that takes the sensor's RGB of the 24 ColorChecker swatches under the white-balance illuminant to
        // their XYZ under the output colour space's illuminant
        SpectrumP r = sd.Named(sensorName + "_r"), g = sd.Named(sensorName + "_g"), b = sd.Named(sensorName + "_b");
        if (!r || !g || !b) Die(scene.film.loc, sensorName + ": unknown sensor type");
        rBar = MakeDense(*r); gBar = MakeDense(*g); bBar = MakeDense(*b);
        SpectrumP sensorIllum = DaylightD(whiteBalanceTemp);
        constexpr int nSwatch = 24;
        // PixelSensor::ProjectReflectance (film.h:119-131): float accumulation over the integer wavelengths 360..830
        auto Project = [](const SpectrumH &refl, const SpectrumH &illum, const SpectrumH &b1, const SpectrumH &b2, const SpectrumH &b3, float out[3]) {
            float res[3] = {0, 0, 0}, g_integral = 0;
            for (float lambda = 360; lambda <= 830; ++lambda) {
                g_integral += b2(lambda) * illum(lambda);
                res[0] += b1(lambda) * refl(lambda) * illum(lambda);
                res[1] += b2(lambda) * refl(lambda) * illum(lambda);
                res[2] += b3(lambda) * refl(lambda) * illum(lambda);
            }
            for (int c = 0; c < 3; ++c) out[c] = res[c] / g_integral;
        };
        float rgbCamera[nSwatch][3], xyzOutput[nSwatch][3];
        const float sensorWhiteG = InnerProduct(*sensorIllum, *gBar);
        const float sensorWhiteY = InnerProduct(*sensorIllum, *sd.Y);
        for (int i = 0; i < nSwatch; ++i) {
            SpectrumP sw = MakeFromInterleaved(sd.raw.at("swatch_" + std::to_string(i)), false);
            Project(*sw, *sensorIllum, *rBar, *gBar, *bBar, rgbCamera[i]);
            float xyz[3];
            Project(*sw, *cs->illuminant, *sd.X, *sd.Y, *sd.Z, xyz);
            const float k = sensorWhiteY / sensorWhiteG;
            for (int c = 0; c < 3; ++c) xyzOutput[i][c] = k * xyz[c];
        }
        // LinearLeastSquares (util/math.h:701-718)
        Mat3 AtA{}, AtB{};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                for (int r2 = 0; r2 < nSwatch; ++r2) {
                    AtA.m[i][j] += rgbCamera[r2][i] * rgbCamera[r2][j];
                    AtB.m[i][j] += rgbCamera[r2][i] * xyzOutput[r2][j];
                }
        Mat3 AtAi;
        if (!Inverse(AtA, &AtAi)) Die(scene.film.loc, "Sensor XYZ from RGB matrix could not be solved.");
        const Mat3 prod = AtAi * AtB;
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) XYZFromSensorRGB.m[i][j] = prod.m[j][i];
    } else if (whiteBalanceTemp != 0) {
        // PixelSensor ctor for the XYZ matching functions (film.h:78-90): XYZFromSensorRGB = WhiteBalance(xy of the D illuminant of
        // that temperature, the output colour space's white), the Bradford transform of util/color.h:541-560
        SpectrumP dIllum = DaylightD(whiteBalanceTemp);
        float xyz[3];
        SpectrumToXYZ(*dIllum, xyz);
        const float srcWhite[2] = {xyz[0] / (xyz[0] + xyz[1] + xyz[2]), xyz[1] / (xyz[0] + xyz[1] + xyz[2])};
        const float dstWhite[2] = {cs->w[0], cs->w[1]};
        auto FromxyY = [](const float xy[2], float out[3]) {
            const float Y = 1;
            if (xy[1] == 0) { out[0] = out[1] = out[2] = 0; return; }
            out[0] = xy[0] * Y / xy[1]; out[1] = Y; out[2] = (1 - xy[0] - xy[1]) * Y / xy[1];
        };
        Mat3 LMSFromXYZ, XYZFromLMS;
        const double a[9] = {0.8951, 0.2664, -0.1614, -0.7502, 1.7135, 0.0367, 0.0389, -0.0685, 1.0296};
        const double b[9] = {0.986993, -0.147054, 0.159963, 0.432305, 0.51836, 0.0492912, -0.00852866, 0.0400428, 0.968487};
        for (int i = 0; i < 9; ++i) { LMSFromXYZ.m[i / 3][i % 3] = (float)a[i]; XYZFromLMS.m[i / 3][i % 3] = (float)b[i]; }
        float srcXYZ[3], dstXYZ[3], srcLMS[3], dstLMS[3];
        FromxyY(srcWhite, srcXYZ);
        FromxyY(dstWhite, dstXYZ);
        Mul3(LMSFromXYZ, srcXYZ, srcLMS);
        Mul3(LMSFromXYZ, dstXYZ, dstLMS);
        Mat3 LMScorrect{};
        for (int i = 0; i < 3; ++i) LMScorrect.m[i][i] = dstLMS[i] / srcLMS[i];
        XYZFromSensorRGB = XYZFromLMS * LMScorrect * LMSFromXYZ;
    }
    F.rbar_offset = T->pool.AddDense(*rBar);
    F.gbar_offset = T->pool.AddDense(*gBar);
    F.bbar_offset = T->pool.AddDense(*bBar);
    Mat3 out = cs->RGBFromXYZ * XYZFromSensorRGB;  // film.cpp:496
    std::memcpy(F.XYZFromSensorRGB, XYZFromSensorRGB.m, sizeof(F.XYZFromSensorRGB));
    std::memcpy(F.outputRGBFromSensorRGB, out.m, sizeof(F.outputRGBFromSensorRGB));
    std::memcpy(F.RGBFromXYZ, cs->RGBFromXYZ.m, sizeof(F.RGBFromXYZ));
    T->sRGBFromFilmRGB.clear();
    if (cs != sd.sRGB()) {   // ConvertRGBColorSpace(film colour space, sRGB) = to.RGBFromXYZ * from.XYZFromRGB (util/colorspace.cpp:37-41), for Image::Write
        const Mat3 conv = sd.sRGB()->RGBFromXYZ * cs->XYZFromRGB;
        T->sRGBFromFilmRGB.assign(&conv.m[0][0], &conv.m[0][0] + 9);
    }
    F.illuminant_offset = F.type == WF_FILM_GBUFFER ? T->pool.AddDense(*MakeDense(*cs->illuminant)) : -1;
    // FilmBaseParameters (film.cpp:66-172)
    T->imageFile = ps.GetOneString("filename", "");
    if (!opt.imageFile.empty()) T->imageFile = opt.imageFile;
    else if (T->imageFile.empty()) T->imageFile = "pbrt.pfm";
    if (F.type != WF_FILM_RGB && (T->imageFile.size() < 4 || T->imageFile.substr(T->imageFile.size() - 4) != ".exr"))
        Die(scene.film.loc, T->imageFile + (F.type == WF_FILM_SPECTRAL ? ": EXR is the only output format supported by the SpectralFilm." : ": EXR is the only format supported by the GBufferFilm."));
    F.full_res[0] = ps.GetOneInt("xresolution", 1280);
    F.full_res[1] = ps.GetOneInt("yresolution", 720);
    if (opt.quickRender) { F.full_res[0] = std::max(1, F.full_res[0] / 4); F.full_res[1] = std::max(1, F.full_res[1] / 4); }   // film.cpp:92-95
    int pb[4] = {0, 0, F.full_res[0], F.full_res[1]};  // xmin, ymin, xmax, ymax
    auto intersect = [&](int x0, int y0, int x1, int y1) {
        pb[0] = std::max(pb[0], x0); pb[1] = std::max(pb[1], y0); pb[2] = std::min(pb[2], x1); pb[3] = std::min(pb[3], y1);
    };
    std::vector<int> pbv = ps.GetIntArray("pixelbounds");
    if (opt.hasPixelBounds) intersect(opt.pixelBounds[0], opt.pixelBounds[2], opt.pixelBounds[1], opt.pixelBounds[3]);
    else if (pbv.size() == 4) intersect(pbv[0], pbv[2], pbv[1], pbv[3]);
    std::vector<float> cr = ps.GetFloatArray("cropwindow");
    const float *crop = nullptr;
    float cropv[4];
    if (opt.hasCropWindow) crop = opt.cropWindow;
    else if (cr.size() == 4) { std::memcpy(cropv, cr.data(), 16); crop = cropv; }
    if (crop) {
        float c0 = Clamp(crop[0], 0.f, 1.f), c1 = Clamp(crop[1], 0.f, 1.f), c2 = Clamp(crop[2], 0.f, 1.f), c3 = Clamp(crop[3], 0.f, 1.f);
        pb[0] = (int)std::ceil(F.full_res[0] * c0); pb[1] = (int)std::ceil(F.full_res[1] * c2);
        pb[2] = (int)std::ceil(F.full_res[0] * c1); pb[3] = (int)std::ceil(F.full_res[1] * c3);
    }
    if (pb[0] >= pb[2] || pb[1] >= pb[3]) Die(scene.film.loc, "Degenerate pixel bounds provided to film");
    F.pixel_min[0] = pb[0]; F.pixel_min[1] = pb[1]; F.pixel_max[0] = pb[2]; F.pixel_max[1] = pb[3];
    ps.GetOneFloat("diagonal", 35.f);
    ps.ReportUnused("Film");
}

void BuildSampler(const ParsedScene &scene, const RenderOptions &opt, SceneTables *T) {
    const ParamSet &ps = scene.sampler.params;
    wf_sampler &S = T->desc.sampler;
    int nsamp = ps.GetOneInt("pixelsamples", 16);
    if (opt.pixelSamples > 0) nsamp = opt.pixelSamples;
    S.seed = ps.GetOneInt("seed", opt.seed);
    if (scene.sampler.name == "zsobol") {
        S.type = WF_SAMPLER_ZSOBOL;
        std::string s = ps.GetOneString("randomization", "fastowen");
        if (s == "none") S.randomize = WF_RAND_NONE;
        else if (s == "permutedigits") S.randomize = WF_RAND_PERMUTE_DIGITS;
        else if (s == "fastowen") S.randomize = WF_RAND_FAST_OWEN;
        else if (s == "owen") S.randomize = WF_RAND_OWEN;
        else Die(scene.sampler.loc, s + ": unknown randomization strategy given to ZSobolSampler");
        if (nsamp & (nsamp - 1)) fprintf(stderr, "Warning: Sobol samplers with non power-of-two sample counts (%d) are suboptimal.\n", nsamp);
        // samplers.h:228-240
        auto Log2Int = [](uint32_t v) { return 31 - __builtin_clz(v); };
        auto RoundUpPow2 = [](int32_t v) { v--; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; return v + 1; };
        S.log2spp = Log2Int((uint32_t)nsamp);
        int res = RoundUpPow2(std::max(T->desc.film.full_res[0], T->desc.film.full_res[1]));
        int log4spp = (S.log2spp + 1) / 2;
        S.nBase4Digits = Log2Int((uint32_t)res) + log4spp;
        S.spp = 1 << S.log2spp;
    } else if (scene.sampler.name == "independent") {
        // samplers.cpp IndependentSampler::Create: default 4 samples
        S.type = WF_SAMPLER_INDEPENDENT;
        S.spp = ps.GetOneInt("pixelsamples", 4);
        if (opt.pixelSamples > 0) S.spp = opt.pixelSamples;
    } else if (scene.sampler.name == "stratified") {
        // StratifiedSampler::Create
        S.type = WF_SAMPLER_STRATIFIED;
        S.jitter = ps.GetOneBool("jitter", true);
        int xs = ps.GetOneInt("xsamples", 4), ys = ps.GetOneInt("ysamples", 4);
        if (opt.pixelSamples > 0) {
            int n = opt.pixelSamples;
            int div = (int)std::sqrt((double)n);
            while (n % div) --div;
            xs = n / div;
            ys = n / xs;
        }
        S.x_samples = xs; S.y_samples = ys;
        S.spp = xs * ys;
    } else if (scene.sampler.name == "paddedsobol") {
        // PaddedSobolSampler::Create
        S.type = WF_SAMPLER_PADDED_SOBOL;
        std::string s = ps.GetOneString("randomization", "fastowen");
        if (s == "none") S.randomize = WF_RAND_NONE;
        else if (s == "permutedigits") S.randomize = WF_RAND_PERMUTE_DIGITS;
        else if (s == "fastowen") S.randomize = WF_RAND_FAST_OWEN;
        else if (s == "owen") S.randomize = WF_RAND_OWEN;
        else Die(scene.sampler.loc, s + ": unknown randomization strategy given to PaddedSobolSampler");
        if (nsamp & (nsamp - 1)) fprintf(stderr, "Warning: Sobol samplers with non power-of-two sample counts (%d) are suboptimal.\n", nsamp);
        S.spp = nsamp;
    } else if (scene.sampler.name == "sobol") {
        // SobolSampler::Create + ctor (samplers.cpp:258-283, samplers.h:482-490)
        S.type = WF_SAMPLER_SOBOL;
        std::string s = ps.GetOneString("randomization", "fastowen");
        if (s == "none") S.randomize = WF_RAND_NONE;
        else if (s == "permutedigits") S.randomize = WF_RAND_PERMUTE_DIGITS;
        else if (s == "fastowen") S.randomize = WF_RAND_FAST_OWEN;
        else if (s == "owen") S.randomize = WF_RAND_OWEN;
        else Die(scene.sampler.loc, s + ": unknown randomization strategy given to SobolSampler");
        if (nsamp & (nsamp - 1)) fprintf(stderr, "Warning: Non power-of-two sample count %d will perform suboptimally with the SobolSampler.\n", nsamp);
        S.spp = nsamp;
        {
            // film.FullResolution() (scene.cpp:771): the film built just before this, --quick's quartering included
            const int rx = T->desc.film.full_res[0], ry = T->desc.film.full_res[1];
            int sc = 1;
            while (sc < std::max(rx, ry)) sc *= 2;  // RoundUpPow2
            S.sobol_scale = sc;
        }
        std::ifstream f(SpectralData::Get().DataDir() + "/sobol_matrices.bin", std::ios::binary);
        uint32_t hdr[5] = {};
        f.read((char *)hdr, sizeof(hdr));
        if (!f || memcmp(hdr, "SOBM", 4) != 0 || hdr[1] != 1024 || hdr[2] != 52 || hdr[3] != 25 || hdr[4] != 26)
            Die(scene.sampler.loc, "data/sobol_matrices.bin is missing or malformed (tools/extract_sobol_matrices.py)");
        T->sobolMatrices.resize(1024 * 52); T->vdcSobol.resize(25 * 52); T->vdcSobolInv.resize(26 * 52);
        f.read((char *)T->sobolMatrices.data(), T->sobolMatrices.size() * 4);
        f.read((char *)T->vdcSobol.data(), T->vdcSobol.size() * 8);
        f.read((char *)T->vdcSobolInv.data(), T->vdcSobolInv.size() * 8);
        if (!f) Die(scene.sampler.loc, "data/sobol_matrices.bin is truncated");
    } else if (scene.sampler.name == "halton") {
        // HaltonSampler::Create + ctor (samplers.cpp:32-52,67-92)
        S.type = WF_SAMPLER_HALTON;
        std::string s = ps.GetOneString("randomization", "permutedigits");
        if (s == "none") S.randomize = WF_RAND_NONE;
        else if (s == "permutedigits") S.randomize = WF_RAND_PERMUTE_DIGITS;
        else if (s == "fastowen") Die(scene.sampler.loc, "\"fastowen\" randomization not supported by Halton sampler.");
        else if (s == "owen") S.randomize = WF_RAND_OWEN;
        else Die(scene.sampler.loc, s + ": unknown randomization strategy given to HaltonSampler");
        S.spp = nsamp;
        for (int i = 0; i < 2; ++i) {
            int base = (i == 0) ? 2 : 3, scale = 1, exp = 0;
            while (scale < std::min(T->desc.film.full_res[i], 128)) { scale *= base; ++exp; }
            S.halton_base_scales[i] = scale;
            S.halton_base_exponents[i] = exp;
        }
        // multiplicativeInverse via the extended GCD (samplers.h:100-116)
        struct G { static void gcd(uint64_t a, uint64_t b, int64_t *x, int64_t *y) {
            if (b == 0) { *x = 1; *y = 0; return; }
            int64_t d = a / b, xp, yp;
            gcd(b, a % b, &xp, &yp);
            *x = yp; *y = xp - (d * yp);
        } };
        auto multInv = [](int64_t a, int64_t n) { int64_t x, y; G::gcd(a, n, &x, &y); int64_t r = x - (x / n) * n; return (int)(r < 0 ? r + n : r); };
        S.halton_mult_inverse[0] = multInv(S.halton_base_scales[1], S.halton_base_scales[0]);
        S.halton_mult_inverse[1] = multInv(S.halton_base_scales[0], S.halton_base_scales[1]);
        // Primes[1000] (util/primes.cpp) by sieve; DigitPermutation per prime (util/lowdiscrepancy.h:30-48)
        std::vector<char> composite(7920, 0);
        for (int i = 2; i < 7920 && (int)T->haltonPrimes.size() < 1000; ++i) {
            if (composite[i]) continue;
            T->haltonPrimes.push_back(i);
            for (int j = 2 * i; j < 7920; j += i) composite[j] = 1;
        }
        T->haltonPermOffsets.assign(1000, 0);
        if (S.randomize == WF_RAND_PERMUTE_DIGITS)
            for (int d = 0; d < 1000; ++d) {
                const int base = T->haltonPrimes[d];
                int nDigits = 0;
                float invBase = (float)1 / (float)base, invBaseM = 1;
                while (1 - (base - 1) * invBaseM < 1) { ++nDigits; invBaseM *= invBase; }
                T->haltonPermOffsets[d] = (int32_t)T->haltonPerms.size();
                for (int digitIndex = 0; digitIndex < nDigits; ++digitIndex) {
                    uint32_t w[3] = {(uint32_t)base, (uint32_t)digitIndex, (uint32_t)S.seed};
                    uint64_t dseed = HashWords(w, 3);
                    for (int digitValue = 0; digitValue < base; ++digitValue)
                        T->haltonPerms.push_back((uint16_t)PermutationElement((uint32_t)digitValue, (uint32_t)base, (uint32_t)dseed));
                }
            }
    } else Die(scene.sampler.loc, scene.sampler.name + ": sampler type not supported by this build (zsobol, sobol, independent, stratified, paddedsobol, halton)");
    T->spp = S.spp;
    ps.ReportUnused("Sampler");
}

// Medium::Create (media.cpp:667-689): HomogeneousMedium::Create (:201-234) and GridMedium::Create (:283-360) with the
// constructors' precomputation (spectra densely sampled and pre-scaled, 16^3 majorant grid, media.cpp:238-272)
static void BuildMedia(const ParsedScene &scene, SceneTables *T, std::map<std::string, int> *ids) {
    for (const auto &nm : scene.media) {
        const Entity &e = nm.second;
        const ParamSet &ps = e.params;
        if (ids->count(nm.first)) Die(e.loc, nm.first + ": named medium redefined.");
        wf_medium M{};
        M.temperature_offset = -1;
        auto dense = [&](const SpectrumH &s, float scale) {
            SpectrumP d = MakeDense(s);
            d->Scale(scale);
            return T->pool.AddDense(*d);
        };
        M.g = ps.GetOneFloat("g", 0.f);
        float sigmaScale = ps.GetOneFloat("scale", 1.f);
        const bool rgbGrid = e.name == "rgbgrid";  // its sigma_a / sigma_s / Le are per-cell RGB arrays
        SpectrumP sig_a, sig_s;
        if (e.name == "homogeneous")   // HomogeneousMedium::Create (media.cpp:169-186): the only medium with presets
            if (std::string preset = ps.GetOneString("preset", ""); !preset.empty() && !MediumPreset(preset, &sig_a, &sig_s))
                fprintf(stderr, "Warning: %s: Material preset \"%s\" not found.\n", e.loc.c_str(), preset.c_str());
        if (!sig_a) sig_a = rgbGrid ? nullptr : ps.GetOneSpectrum("sigma_a", nullptr, SpectrumType::Unbounded);
        if (!sig_a) sig_a = MakeConstant(1.f);
        if (!sig_s) sig_s = rgbGrid ? nullptr : ps.GetOneSpectrum("sigma_s", nullptr, SpectrumType::Unbounded);
        if (!sig_s) sig_s = MakeConstant(1.f);
        M.sigma_a_offset = dense(*sig_a, sigmaScale);
        M.sigma_s_offset = dense(*sig_s, sigmaScale);
        SpectrumP Le = rgbGrid ? nullptr : ps.GetOneSpectrum("Le", nullptr, SpectrumType::Illuminant);
        if (e.name == "homogeneous") {
            M.type = WF_MEDIUM_HOMOGENEOUS;
            float LeScale = ps.GetOneFloat("Lescale", 1.f);
            if (!Le || Le->MaxValue() == 0) Le = MakeConstant(0.f);
            else LeScale /= SpectrumToPhotometric(*Le);
            SpectrumP d = MakeDense(*Le);
            d->Scale(LeScale);
            M.is_emissive = d->MaxValue() > 0;
            M.le_offset = T->pool.AddDense(*d);
        } else if (e.name == "uniformgrid") {
            M.type = WF_MEDIUM_GRID;
            std::vector<float> density = ps.GetFloatArray("density");
            if (density.empty()) Die(e.loc, "No \"density\" value provided for grid medium.");
            std::vector<float> temperature = ps.GetFloatArray("temperature");
            if (!temperature.empty() && temperature.size() != density.size()) Die(e.loc, "Different number of samples provided for \"density\" and \"temperature\".");
            if (Le && !temperature.empty()) Die(e.loc, "Both \"Le\" and \"temperature\" values were provided.");
            M.nx = ps.GetOneInt("nx", 1); M.ny = ps.GetOneInt("ny", 1); M.nz = ps.GetOneInt("nz", 1);
            if ((long long)density.size() != (long long)M.nx * M.ny * M.nz)
                Die(e.loc, "Grid medium has " + std::to_string(density.size()) + " density values; expected nx*ny*nz = " + std::to_string((long long)M.nx * M.ny * M.nz));
            float LeNorm = 1;
            if (!Le || Le->MaxValue() == 0) Le = MakeConstant(0.f);
            else LeNorm = 1 / SpectrumToPhotometric(*Le);
            SpectrumP d = MakeDense(*Le);
            M.is_emissive = !temperature.empty() ? 1 : d->MaxValue() > 0;  // media.cpp:238
            M.le_offset = T->pool.AddDense(*d);
            M.temperature_offset = -1;
            if (!temperature.empty()) {
                M.temperature_offset = (int)T->mediumData.size();
                T->mediumData.insert(T->mediumData.end(), temperature.begin(), temperature.end());
            }
            M.temperature_shift = ps.GetOneFloat("temperatureoffset", ps.GetOneFloat("temperaturecutoff", 0.f));
            M.temperature_scale = ps.GetOneFloat("temperaturescale", 1.f);
            std::vector<float> LeScale = ps.GetFloatArray("Lescale");
            M.le_scale_offset = (int)T->mediumData.size();
            if (LeScale.empty()) {
                M.le_nx = M.le_ny = M.le_nz = 1;
                T->mediumData.push_back(LeNorm);
            } else {
                if (LeScale.size() != density.size()) Die(e.loc, "\"Lescale\" must have nx*ny*nz values");
                M.le_nx = M.nx; M.le_ny = M.ny; M.le_nz = M.nz;
                for (float v : LeScale) T->mediumData.push_back(v * LeNorm);
            }
            V3 p0 = ps.GetOnePoint3f("p0", V3{0, 0, 0}), p1 = ps.GetOnePoint3f("p1", V3{1, 1, 1});
            // Bounds3f(p0, p1): componentwise min / max
            for (int c = 0; c < 3; ++c) { M.bounds[c] = std::min(p0[c], p1[c]); M.bounds[3 + c] = std::max(p0[c], p1[c]); }
            M.render_from_medium = scene.mediaTransforms.at(nm.first).abi();
            M.density_offset = (int)T->mediumData.size();
            T->mediumData.insert(T->mediumData.end(), density.begin(), density.end());
            // majorant grid: SampledGrid::MaxValue over each voxel's bounds (util/containers.h:828-845)
            M.maj_res[0] = M.maj_res[1] = M.maj_res[2] = 16;
            M.maj_offset = (int)T->mediumData.size();
            const int nx = M.nx, ny = M.ny, nz = M.nz;
            auto lookup = [&](int x, int y, int z) -> float {
                if (!(x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz)) return 0.f;
                return density[((size_t)z * ny + y) * nx + x];
            };
            for (int z = 0; z < 16; ++z)
                for (int y = 0; y < 16; ++y)
                    for (int x = 0; x < 16; ++x) {
                        // MajorantGrid::VoxelBounds (media.h:124-128)
                        float b0[3] = {float(x) / 16, float(y) / 16, float(z) / 16};
                        float b1[3] = {float(x + 1) / 16, float(y + 1) / 16, float(z + 1) / 16};
                        float ps0[3] = {b0[0] * nx - .5f, b0[1] * ny - .5f, b0[2] * nz - .5f};
                        float ps1[3] = {b1[0] * nx - .5f, b1[1] * ny - .5f, b1[2] * nz - .5f};
                        int lo[3], hi[3];
                        const int n3[3] = {nx, ny, nz};
                        for (int c = 0; c < 3; ++c) {
                            lo[c] = std::max((int)std::floor(ps0[c]), 0);
                            hi[c] = std::min((int)std::floor(ps1[c]) + 1, n3[c] - 1);
                        }
                        float mx = lookup(lo[0], lo[1], lo[2]);
                        for (int zz = lo[2]; zz <= hi[2]; ++zz)
                            for (int yy = lo[1]; yy <= hi[1]; ++yy)
                                for (int xx = lo[0]; xx <= hi[0]; ++xx) mx = std::max(mx, lookup(xx, yy, zz));
                        T->mediumData.push_back(mx);
                    }
        } else if (e.name == "rgbgrid") {
            // RGBGridMedium::Create + ctor (media.cpp:380-456, 339-378)
            M.type = WF_MEDIUM_RGB_GRID;
            std::vector<V3> a = ps.GetTuple3Array("sigma_a", "rgb"), s = ps.GetTuple3Array("sigma_s", "rgb"), le = ps.GetTuple3Array("Le", "rgb");
            if (a.empty() && s.empty()) Die(e.loc, "RGB grid requires \"sigma_a\" and/or \"sigma_s\" parameter values.");
            size_t nDensity = !a.empty() ? a.size() : s.size();
            if (!a.empty() && !s.empty() && a.size() != s.size()) Die(e.loc, "Different number of samples provided for \"sigma_a\" and \"sigma_s\".");
            if (!le.empty() && a.empty()) Die(e.loc, "RGB grid requires \"sigma_a\" if \"Le\" value provided.");
            if (!le.empty() && nDensity != le.size()) Die(e.loc, "Wrong number of values for the \"Le\" parameter.");
            M.nx = ps.GetOneInt("nx", 1); M.ny = ps.GetOneInt("ny", 1); M.nz = ps.GetOneInt("nz", 1);
            if ((long long)nDensity != (long long)M.nx * M.ny * M.nz) Die(e.loc, "RGB grid medium has " + std::to_string(nDensity) + " density values; expected nx*ny*nz");
            const ColorSpace *cs = ps.colorSpace;
            // the cells as {c0, c1, c2, scale}; RGBSigmoidPolynomial::MaxValue (util/color.h:348-355) for the majorants
            auto polyMax = [](float c0, float c1, float c2) {
                float result = std::max(SigmoidPoly(360.f, c0, c1, c2), SigmoidPoly(830.f, c0, c1, c2));
                float lambda = -c1 / (2 * c0);
                if (lambda >= 360 && lambda <= 830) result = std::max(result, SigmoidPoly(lambda, c0, c1, c2));
                return result;
            };
            std::vector<float> maxA, maxS;
            auto pushGrid = [&](const std::vector<V3> &rgbs, bool illuminant, std::vector<float> *maxv) {
                int off = (int)T->mediumData.size();
                for (const V3 &c : rgbs) {
                    float rgb[3] = {c.x, c.y, c.z};
                    SpectrumP sp = illuminant ? cs->Illuminant(rgb) : cs->Unbounded(rgb);
                    T->mediumData.push_back(sp->c0); T->mediumData.push_back(sp->c1); T->mediumData.push_back(sp->c2); T->mediumData.push_back(sp->scale);
                    if (maxv) maxv->push_back(sp->scale * polyMax(sp->c0, sp->c1, sp->c2));
                }
                return off;
            };
            M.rgb_a_offset = a.empty() ? -1 : pushGrid(a, false, &maxA);
            M.rgb_s_offset = s.empty() ? -1 : pushGrid(s, false, &maxS);
            M.rgb_le_offset = le.empty() ? -1 : pushGrid(le, true, nullptr);
            V3 p0 = ps.GetOnePoint3f("p0", V3{0, 0, 0}), p1 = ps.GetOnePoint3f("p1", V3{1, 1, 1});
            for (int c = 0; c < 3; ++c) { M.bounds[c] = std::min(p0[c], p1[c]); M.bounds[3 + c] = std::max(p0[c], p1[c]); }
            M.le_scale = ps.GetOneFloat("Lescale", 1.f);
            M.g = ps.GetOneFloat("g", 0.f);
            M.sigma_scale = ps.GetOneFloat("scale", 1.f);
            M.is_emissive = !le.empty() && M.le_scale > 0;
            M.le_offset = T->pool.AddDense(*cs->illuminant);
            M.sigma_a_offset = M.sigma_s_offset = M.le_offset;  // unused by this medium type
            M.render_from_medium = scene.mediaTransforms.at(nm.first).abi();
            M.maj_res[0] = M.maj_res[1] = M.maj_res[2] = 16;
            M.maj_offset = (int)T->mediumData.size();
            const int nx = M.nx, ny = M.ny, nz = M.nz;
            auto gridMax = [&](const std::vector<float> &v, const int lo[3], const int hi[3]) {
                auto lookup = [&](int x, int y, int z) -> float {
                    if (!(x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz)) return 0.f;
                    return v[((size_t)z * ny + y) * nx + x];
                };
                float mx = lookup(lo[0], lo[1], lo[2]);
                for (int zz = lo[2]; zz <= hi[2]; ++zz)
                    for (int yy = lo[1]; yy <= hi[1]; ++yy)
                        for (int xx = lo[0]; xx <= hi[0]; ++xx) mx = std::max(mx, lookup(xx, yy, zz));
                return mx;
            };
            for (int z = 0; z < 16; ++z)
                for (int y = 0; y < 16; ++y)
                    for (int x = 0; x < 16; ++x) {
                        float b0[3] = {float(x) / 16, float(y) / 16, float(z) / 16};
                        float b1[3] = {float(x + 1) / 16, float(y + 1) / 16, float(z + 1) / 16};
                        int lo[3], hi[3];
                        const int n3[3] = {nx, ny, nz};
                        for (int c = 0; c < 3; ++c) {
                            lo[c] = std::max((int)std::floor(b0[c] * n3[c] - .5f), 0);
                            hi[c] = std::min((int)std::floor(b1[c] * n3[c] - .5f) + 1, n3[c] - 1);
                        }
                        float maxSigma_t = (a.empty() ? 1 : gridMax(maxA, lo, hi)) + (s.empty() ? 1 : gridMax(maxS, lo, hi));
                        T->mediumData.push_back(M.sigma_scale * maxSigma_t);
                    }
        } else if (e.name == "cloud") {
            // CloudMedium::Create (media.cpp:462-484): no "scale", no emission
            M.type = WF_MEDIUM_CLOUD;
            M.sigma_a_offset = dense(*sig_a, 1.f);
            M.sigma_s_offset = dense(*sig_s, 1.f);
            M.le_offset = M.sigma_a_offset;
            M.cloud_density = ps.GetOneFloat("density", 1.f);
            M.cloud_wispiness = ps.GetOneFloat("wispiness", 1.f);
            M.cloud_frequency = ps.GetOneFloat("frequency", 5.f);
            V3 p0 = ps.GetOnePoint3f("p0", V3{0, 0, 0}), p1 = ps.GetOnePoint3f("p1", V3{1, 1, 1});
            // Bounds3f(p0, p1): componentwise min / max
            for (int c = 0; c < 3; ++c) { M.bounds[c] = std::min(p0[c], p1[c]); M.bounds[3 + c] = std::max(p0[c], p1[c]); }
            M.render_from_medium = scene.mediaTransforms.at(nm.first).abi();
            LoadNoisePerm(T);
        } else if (e.name == "nanovdb") {
            // NanoVDBMedium::Create + ctor (media.cpp:512-660).  Parity unpinned: nanovdb_io.cpp.
            M.type = WF_MEDIUM_NANOVDB;
            std::string fn = ps.GetOneString("filename", "");
            if (fn.empty()) Die(e.loc, "Must supply \"filename\" to \"nanovdb\" medium.");
            if (fn[0] != '/') fn = scene.baseDir + "/" + fn;
            VdbGrid dg, tg;
            ReadNanoVDBGrid(fn, ps.GetOneString("gridname", "density"), &dg);
            if (!dg.found) Die(e.loc, fn + ": didn't find \"density\" grid.");
            ReadNanoVDBGrid(fn, ps.GetOneString("temperaturename", "temperature"), &tg);
            M.le_scale = ps.GetOneFloat("Lescale", 1.f);
            M.temperature_shift = ps.GetOneFloat("temperatureoffset", ps.GetOneFloat("temperaturecutoff", 0.f));
            M.temperature_scale = ps.GetOneFloat("temperaturescale", 1.f);
            M.le_offset = T->pool.AddDense(*MakeDense(*MakeConstant(0.f)));
            M.is_emissive = tg.found && M.le_scale > 0;   // IsEmissive(), media.h:612
            M.render_from_medium = scene.mediaTransforms.at(nm.first).abi();
            auto put = [&](const VdbGrid &g, int32_t vmin[3], int32_t vdim[3], float inv[9], float vec[3], float *bg) {
                for (int a = 0; a < 3; ++a) { vmin[a] = g.min[a]; vdim[a] = g.dim[a]; vec[a] = g.vec[a]; }
                for (int a = 0; a < 9; ++a) inv[a] = g.invMat[a];
                *bg = g.background;
                if ((long long)T->mediumData.size() + (long long)g.values.size() > (1ll << 31) - 1) Die(e.loc, fn + ": the dense grids exceed this build's 2^31-float medium pool");
                int off = (int)T->mediumData.size();
                T->mediumData.insert(T->mediumData.end(), g.values.begin(), g.values.end());
                if (g.values.empty()) T->mediumData.push_back(g.background);
                return off;
            };
            M.density_offset = put(dg, M.vdb_min, M.vdb_dim, M.vdb_inv_mat, M.vdb_vec, &M.vdb_background);
            M.temperature_offset = tg.found ? put(tg, M.vdbt_min, M.vdbt_dim, M.vdbt_inv_mat, M.vdbt_vec, &M.vdbt_background) : -1;
            // bounds = the density grid's world bounding box, joined with the temperature grid's (media.cpp:540-556), as floats
            for (int c = 0; c < 3; ++c) { M.bounds[c] = (float)dg.worldBBox[c]; M.bounds[3 + c] = (float)dg.worldBBox[3 + c]; }
            if (tg.found)
                for (int c = 0; c < 3; ++c) { M.bounds[c] = std::min(M.bounds[c], (float)tg.worldBBox[c]); M.bounds[3 + c] = std::max(M.bounds[3 + c], (float)tg.worldBBox[3 + c]); }
            // the 64^3 majorant grid (media.cpp:571-623): per cell the maximum voxel value over the cell's index-space extent +- 1
            M.maj_res[0] = M.maj_res[1] = M.maj_res[2] = 64;
            M.maj_offset = (int)T->mediumData.size();
            T->mediumData.resize(T->mediumData.size() + 64 * 64 * 64);
            float *maj = &T->mediumData[M.maj_offset];
            auto lerpB = [&](int c, float t) { return (1 - t) * M.bounds[c] + t * M.bounds[3 + c]; };   // Bounds3::Lerp -> Lerp(t, pMin, pMax)
            auto toIndex = [&](const float w[3], float out[3]) {
                const float x = w[0] - dg.vec[0], y = w[1] - dg.vec[1], z = w[2] - dg.vec[2];
                for (int r = 0; r < 3; ++r) out[r] = std::fmaf(x, dg.invMat[3 * r], std::fmaf(y, dg.invMat[3 * r + 1], z * dg.invMat[3 * r + 2]));
            };
            auto value = [&](int x, int y, int z) -> float {
                x -= dg.min[0]; y -= dg.min[1]; z -= dg.min[2];
                if (!(x >= 0 && x < dg.dim[0] && y >= 0 && y < dg.dim[1] && z >= 0 && z < dg.dim[2])) return dg.background;
                return dg.values[((size_t)z * dg.dim[1] + y) * dg.dim[0] + x];
            };
            for (int z = 0; z < 64; ++z)
                for (int y = 0; y < 64; ++y)
                    for (int x = 0; x < 64; ++x) {
                        const float w0[3] = {lerpB(0, float(x) / 64), lerpB(1, float(y) / 64), lerpB(2, float(z) / 64)};
                        const float w1[3] = {lerpB(0, float(x + 1) / 64), lerpB(1, float(y + 1) / 64), lerpB(2, float(z + 1) / 64)};
                        float i0[3], i1[3];
                        toIndex(w0, i0);
                        toIndex(w1, i1);
                        const float delta = 1.f;
                        int lo[3], hi[3];
                        for (int a = 0; a < 3; ++a) {
                            lo[a] = std::max(int(i0[a] - delta), dg.min[a]);
                            hi[a] = std::min(int(i1[a] + delta), dg.min[a] + dg.dim[a] - 1);
                        }
                        float mx = 0;
                        for (int zz = lo[2]; zz <= hi[2]; ++zz)
                            for (int yy = lo[1]; yy <= hi[1]; ++yy)
                                for (int xx = lo[0]; xx <= hi[0]; ++xx) mx = std::max(mx, value(xx, yy, zz));
                        maj[(z * 64 + y) * 64 + x] = mx;
                    }
        } else Die(e.loc, e.name + ": medium type is not supported by this build (homogeneous, uniformgrid, rgbgrid, cloud, nanovdb)");
        ps.ReportUnused("MakeNamedMedium");   // Medium::Create, media.cpp:687
        (*ids)[nm.first] = (int)T->media.size();
        T->media.push_back(M);
    }
}

// PowerLightSampler ctor (lightsamplers.cpp:64-86): Light::Phi at SampleVisible(0.5) / pdf, averaged, then the
// AliasTable construction of util/sampling.cpp:34-86 (same work-list order, so the same bins)
static void BuildPowerAlias(SceneTables *T) {
    const size_t n = T->lights.size();
    T->powerAlias.assign(3 * n, 0.f);
    if (n == 0) return;
    Wavelengths lambda = SampleVisible(0.5f);
    std::vector<float> lightPower;
    for (const wf_light &l : T->lights) {
        S4 Ls = S4c(0.f);
        for (int i = 0; i < 4; ++i) {
            int o = (int)std::lround(lambda.lambda[i]) - WF_LAMBDA_MIN;
            Ls[i] = (o < 0 || o >= WF_NDENSE) ? 0.f : T->pool.data[l.spectrum_offset + o];
        }
        S4 phi = S4c(0.f);
        switch (l.type) {
        case WF_LIGHT_POINT: phi = 4 * Pi * l.scale * Ls; break;                              // lights.cpp:164-166
        case WF_LIGHT_SPOT:                                                                   // lights.cpp:1365-1368
            phi = l.scale * Ls * 2 * Pi * ((1 - l.cosFalloffStart) + (l.cosFalloffStart - l.cosFalloffEnd) / 2);
            break;
        case WF_LIGHT_DISTANT: phi = l.scale * Ls * Pi * Sqr(l.sceneRadius); break;           // lights.cpp:216-218
        case WF_LIGHT_PROJECTION: {                                                           // lights.cpp:362-382
            const wf_tex_image &im = T->texImages[l.image];
            const ColorSpace *ics = SpectralData::Get().sRGB();
            Mat4 lm, lmi;
            std::memcpy(lm.m, T->lightTransforms[l.xform2].mInv, sizeof(lm.m));
            std::memcpy(lmi.m, T->lightTransforms[l.xform2].m, sizeof(lmi.m));
            Transform lightFromScreen(lm, lmi);
            S4 sum = S4c(0.f);
            const int w = im.res[0], h = im.res[1];
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    float tx = (x + 0.5f) / w, ty = (y + 0.5f) / h;
                    V2 p2{(1 - tx) * l.screen_bounds[0] + tx * l.screen_bounds[2], (1 - ty) * l.screen_bounds[1] + ty * l.screen_bounds[3]};
                    V3 wv = Normalize(lightFromScreen.Point(V3{p2.x, p2.y, 0}));
                    float dwdA = wv.z * wv.z * wv.z;
                    const float *px = &T->tableData[im.level_offset[0] + 3 * ((size_t)y * w + x)];
                    float rgb[3] = {std::max(0.f, px[0]), std::max(0.f, px[1]), std::max(0.f, px[2])};
                    SpectrumP sp = ics->Illuminant(rgb);
                    S4 s;
                    for (int i = 0; i < 4; ++i) s[i] = sp->scale * SigmoidPoly(lambda.lambda[i], sp->c0, sp->c1, sp->c2);
                    sum = sum + (s * Ls) * dwdA;  // Ls = the colour space's illuminant at lambda
                }
            phi = l.scale * l.area * sum / (float)(w * h);
            break;
        }
        case WF_LIGHT_GONIOMETRIC: {                                                          // lights.cpp:554-561
            const wf_tex_image &im = T->texImages[l.image];
            float sumY = 0;
            for (size_t i = 0; i < (size_t)im.res[0] * im.res[1]; ++i) sumY += T->tableData[im.level_offset[0] + i];
            phi = l.scale * Ls * 4 * Pi * sumY / (float)(im.res[0] * im.res[1]);
            break;
        }
        case WF_LIGHT_DIFFUSE_AREA:                                                           // lights.cpp:769-786
            if (l.image >= 0) {
                const wf_tex_image &im = T->texImages[l.image];
                const ColorSpace *ics = SpectralData::Get().sRGB();
                S4 Lsum = S4c(0.f);
                for (size_t i = 0; i < (size_t)im.res[0] * im.res[1]; ++i) {
                    const float *px = &T->tableData[im.level_offset[0] + 3 * i];
                    float rgb[3] = {std::max(0.f, px[0]), std::max(0.f, px[1]), std::max(0.f, px[2])};
                    SpectrumP sp = ics->Illuminant(rgb);
                    S4 s;
                    for (int k = 0; k < 4; ++k) s[k] = sp->scale * SigmoidPoly(lambda.lambda[k], sp->c0, sp->c1, sp->c2);
                    Lsum = Lsum + s * Ls;  // Ls = the colour space's illuminant at lambda
                }
                Lsum = Lsum * (l.scale / (im.res[0] * im.res[1]));
                phi = Pi * ((l.flags & WF_LIGHTFLAG_TWOSIDED) ? 2 : 1) * l.area * Lsum;
                break;
            }
            phi = Pi * ((l.flags & WF_LIGHTFLAG_TWOSIDED) ? 2 : 1) * l.area * (Ls * l.scale);
            break;
        case WF_LIGHT_UNIFORM_INFINITE: phi = 4 * Pi * Pi * Sqr(l.sceneRadius) * l.scale * Ls; break;  // lights.cpp:974-976
        case WF_LIGHT_PORTAL_INFINITE: {                                                      // lights.cpp:1183-1206
            const wf_image_light &im = T->imageLights[l.image];
            const ColorSpace *ics = SpectralData::Get().sRGB();
            S4 sumL = S4c(0.f);
            for (int y = 0; y < im.res; ++y)
                for (int x = 0; x < im.res; ++x) {
                    const float *px = &T->tableData[im.pixel_offset + 3 * ((size_t)y * im.res + x)];
                    float rgb[3] = {std::max(0.f, px[0]), std::max(0.f, px[1]), std::max(0.f, px[2])};
                    V2 st{(x + 0.5f) / im.res, (y + 0.5f) / im.res};
                    float duv_dw;
                    (void)PortalRenderFromImage(im, st, &duv_dw);
                    SpectrumP sp = ics->Illuminant(rgb);
                    S4 s;
                    for (int i = 0; i < 4; ++i) s[i] = sp->scale * SigmoidPoly(lambda.lambda[i], sp->c0, sp->c1, sp->c2);
                    sumL = sumL + (s * Ls) / duv_dw;
                }
            V3 c0{im.portal[0][0], im.portal[0][1], im.portal[0][2]}, c1{im.portal[1][0], im.portal[1][1], im.portal[1][2]}, c3{im.portal[3][0], im.portal[3][1], im.portal[3][2]};
            float area = Length(c1 - c0) * Length(c3 - c0);
            phi = l.scale * area * sumL / (float)(im.res * im.res);
            break;
        }
        case WF_LIGHT_IMAGE_INFINITE: {                                                       // lights.cpp:1054-1072
            const wf_image_light &im = T->imageLights[l.image];
            const ColorSpace *ics = SpectralData::Get().sRGB();
            S4 sumL = S4c(0.f);
            for (int v = 0; v < im.res; ++v)
                for (int u = 0; u < im.res; ++u) {
                    const float *px = &T->tableData[im.pixel_offset + 3 * ((size_t)v * im.res + u)];
                    float rgb[3] = {std::max(0.f, px[0]), std::max(0.f, px[1]), std::max(0.f, px[2])};
                    SpectrumP sp = ics->Illuminant(rgb);
                    S4 s;
                    for (int i = 0; i < 4; ++i) s[i] = sp->scale * SigmoidPoly(lambda.lambda[i], sp->c0, sp->c1, sp->c2);
                    sumL = sumL + s * Ls;  // Ls = the colour space's illuminant at lambda
                }
            phi = 4 * Pi * Pi * Sqr(l.sceneRadius) * l.scale * sumL / (float)(im.res * im.res);
            break;
        }
        default: break;
        }
        lightPower.push_back(SafeDiv(phi, lambda.PDF()).Average());
    }
    float total = 0.f;
    for (float v : lightPower) total += v;  // std::accumulate(..., 0.f)
    if (total == 0.f) std::fill(lightPower.begin(), lightPower.end(), 1.f);
    // AliasTable::AliasTable: the sum is accumulated in double (std::accumulate(..., 0.)) and stored as Float
    double dsum = 0.;
    for (float v : lightPower) dsum += v;
    const float sum = (float)dsum;
    struct Bin { float q = 0, p = 0; int alias = 0; };
    std::vector<Bin> bins(n);
    for (size_t i = 0; i < n; ++i) bins[i].p = lightPower[i] / sum;
    struct Outcome { float pHat; size_t index; };
    std::vector<Outcome> under, over;
    for (size_t i = 0; i < n; ++i) {
        float pHat = bins[i].p * n;
        if (pHat < 1) under.push_back(Outcome{pHat, i});
        else over.push_back(Outcome{pHat, i});
    }
    while (!under.empty() && !over.empty()) {
        Outcome un = under.back(), ov = over.back();
        under.pop_back();
        over.pop_back();
        bins[un.index].q = un.pHat;
        bins[un.index].alias = (int)ov.index;
        float pExcess = un.pHat + ov.pHat - 1;
        if (pExcess < 1) under.push_back(Outcome{pExcess, ov.index});
        else over.push_back(Outcome{pExcess, ov.index});
    }
    while (!over.empty()) { Outcome ov = over.back(); over.pop_back(); bins[ov.index].q = 1; bins[ov.index].alias = -1; }
    while (!under.empty()) { Outcome un = under.back(); under.pop_back(); bins[un.index].q = 1; bins[un.index].alias = -1; }
    for (size_t i = 0; i < n; ++i) {
        T->powerAlias[3 * i] = bins[i].q;
        T->powerAlias[3 * i + 1] = bins[i].p;
        T->powerAlias[3 * i + 2] = BitsToFloat((uint32_t)bins[i].alias);
    }
}

void BuildCamera(const ParsedScene &scene, const Transform &renderFromWorld, SceneTables *T) {
    const ParamSet &ps = scene.camera.params;
    wf_camera &C = T->desc.camera;
    const wf_film &F = T->desc.film;
    C.shutterOpen = ps.GetOneFloat("shutteropen", 0.f);
    C.shutterClose = ps.GetOneFloat("shutterclose", 1.f);
    if (C.shutterClose < C.shutterOpen) std::swap(C.shutterClose, C.shutterOpen);
    C.medium = -1;
    Transform renderFromCamera = renderFromWorld * scene.worldFromCamera;  // cameras.cpp:52-56
    C.renderFromCamera = renderFromCamera.abi();
    // ... as the AnimatedTransform it is: rfc[1] = renderFromWorld * worldFromCamera.endTransform over the camera's TransformTimes
    C.anim = MakeAnimatedTransform(renderFromCamera, scene.transformStartTime, renderFromWorld * scene.worldFromCameraEnd, scene.transformEndTime);
    float lensradius = ps.GetOneFloat("lensradius", 0.f);
    float focaldistance = ps.GetOneFloat("focaldistance", 1e6f);
    float frame = ps.GetOneFloat("frameaspectratio", float(F.full_res[0]) / float(F.full_res[1]));
    float sMinX, sMaxX, sMinY, sMaxY;
    if (frame > 1.f) { sMinX = -frame; sMaxX = frame; sMinY = -1.f; sMaxY = 1.f; }
    else { sMinX = -1.f; sMaxX = 1.f; sMinY = -1.f / frame; sMaxY = 1.f / frame; }
    std::vector<float> sw = ps.GetFloatArray("screenwindow");
    if (sw.size() == 4) { sMinX = sw[0]; sMaxX = sw[1]; sMinY = sw[2]; sMaxY = sw[3]; }
    if (scene.camera.name == "realistic") {
        // RealisticCamera::Create + ctor (cameras.cpp:1294-1446, 695-747): the lens prescription, the film's physical extent, the lens
        // moved to focus (thick-lens approximation from two traced rays), 64 exit-pupil bounds from 2^20 traced rays each
        C.type = WF_CAMERA_REALISTIC;
        std::string lensFile = ps.GetOneString("lensfile", "");
        float apertureDiameter = ps.GetOneFloat("aperturediameter", 1.0f);
        const float focusDistance = ps.GetOneFloat("focusdistance", 10.0f);
        if (lensFile.empty()) Die(scene.camera.loc, "No lens description file supplied!");
        if (lensFile[0] != '/') lensFile = scene.baseDir + "/" + lensFile;
        std::vector<float> lensParameters;
        {
            // ReadFloatFile (util/file.cpp:224-290): numbers separated by anything, '#' comments to the end of the line
            std::ifstream f(lensFile);
            if (!f) Die(scene.camera.loc, "Error reading lens specification file \"" + lensFile + "\".");
            std::string line;
            while (std::getline(f, line)) {
                size_t h = line.find('#');
                if (h != std::string::npos) line.resize(h);
                const char *c = line.c_str();
                while (*c) {
                    if (isdigit((unsigned char)*c) || *c == '.' || *c == '-' || *c == '+') {
                        char *end = nullptr;
                        lensParameters.push_back(strtof(c, &end));
                        if (end == c) Die(scene.camera.loc, lensFile + ": unable to parse float value");
                        c = end;
                    } else ++c;
                }
            }
        }
        if (lensParameters.empty()) Die(scene.camera.loc, "Error reading lens specification file \"" + lensFile + "\".");
        if (lensParameters.size() % 4 != 0) Die(scene.camera.loc, lensFile + ": excess values in lens specification file; must be multiple-of-four values, read " + std::to_string(lensParameters.size()) + ".");
        const std::string apertureName = ps.GetOneString("aperture", "");
        C.aperture_image = -1;
        if (!apertureName.empty()) {
            const int builtinRes = 256;
            int aw = builtinRes, ah = builtinRes;
            std::vector<float> img((size_t)aw * ah, 0.f);
            auto rasterize = [&](const std::vector<V2> &vert) {
                for (int y = 0; y < ah; ++y)
                    for (int x = 0; x < aw; ++x) {
                        V2 pt{-1 + 2 * (x + 0.5f) / aw, -1 + 2 * (y + 0.5f) / ah};
                        int windingNumber = 0;
                        for (size_t i = 0; i < vert.size(); ++i) {
                            size_t i1 = (i + 1) % vert.size();
                            float e = (pt.x - vert[i].x) * (vert[i1].y - vert[i].y) - (pt.y - vert[i].y) * (vert[i1].x - vert[i].x);
                            if (vert[i].y <= pt.y) { if (vert[i1].y > pt.y && e > 0) ++windingNumber; }
                            else if (vert[i1].y <= pt.y && e < 0) --windingNumber;
                        }
                        img[(size_t)y * aw + x] = windingNumber == 0 ? 0.f : 1.f;
                    }
            };
            if (apertureName == "gaussian") {
                for (int y = 0; y < ah; ++y)
                    for (int x = 0; x < aw; ++x) {
                        V2 uv{-1 + 2 * (x + 0.5f) / aw, -1 + 2 * (y + 0.5f) / ah};
                        float r2 = Sqr(uv.x) + Sqr(uv.y), sigma2 = 1;
                        img[(size_t)y * aw + x] = std::max(0.f, std::exp(-r2 / sigma2) - std::exp(-1 / sigma2));
                    }
            } else if (apertureName == "square") {
                for (int y = (int)(.25 * builtinRes); y < (int)(.75 * builtinRes); ++y)
                    for (int x = (int)(.25 * builtinRes); x < (int)(.75 * builtinRes); ++x) img[(size_t)y * aw + x] = 4.f;
            } else if (apertureName == "pentagon") {
                float c1 = (std::sqrt(5.f) - 1) / 4, c2 = (std::sqrt(5.f) + 1) / 4;
                float s1 = std::sqrt(10.f + 2.f * std::sqrt(5.f)) / 4, s2 = std::sqrt(10.f - 2.f * std::sqrt(5.f)) / 4;
                std::vector<V2> vert = {V2{0, 1}, V2{s1, c1}, V2{s2, -c2}, V2{-s2, -c2}, V2{-s1, c1}};
                for (V2 &v : vert) { v.x *= .8f; v.y *= .8f; }
                rasterize(vert);
            } else if (apertureName == "star") {
                std::vector<V2> vert(10);
                for (int i = 0; i < 10; ++i) {
                    float r = (i & 1) ? 1.f : (std::cos(Radians(72.f)) / std::cos(Radians(36.f)));
                    vert[i] = V2{r * std::cos(Pi * i / 5.f), r * std::sin(Pi * i / 5.f)};
                }
                std::reverse(vert.begin(), vert.end());
                rasterize(vert);
            } else {
                std::string fn = apertureName[0] == '/' ? apertureName : scene.baseDir + "/" + apertureName;
                HostImage hi;
                try { ReadImage(fn, ColorEnc(), &hi); } catch (const SceneError &e) { Die(scene.camera.loc, std::string(e.what()).substr(7)); }
                if (hi.nc == 2) Die(scene.camera.loc, fn + ": didn't find R, G, B channels to average for aperture image.");
                aw = hi.w; ah = hi.h;
                img.resize((size_t)aw * ah);
                for (size_t i = 0; i < img.size(); ++i) {
                    if (hi.nc == 1) img[i] = hi.Get(i);
                    else img[i] = (hi.Get(i * hi.nc) + hi.Get(i * hi.nc + 1) + hi.Get(i * hi.nc + 2)) / 3;   // ImageChannelValues::Average
                }
            }
            // FlipY, then normalised so that the brightness matches a circular aperture (cameras.cpp:1419-1435)
            for (int y = 0; y < ah / 2; ++y)
                for (int x = 0; x < aw; ++x) std::swap(img[(size_t)y * aw + x], img[(size_t)(ah - 1 - y) * aw + x]);
            float sum = 0;
            for (int y = 0; y < ah; ++y) for (int x = 0; x < aw; ++x) sum += img[(size_t)y * aw + x];
            float avg = sum / (aw * ah);
            float scale = (Pi / 4) / avg;
            for (float &v : img) v = v * scale;
            wf_tex_image im{};
            im.res[0] = aw; im.res[1] = ah; im.n_levels = 1; im.n_channels = 1; im.wrap = WF_WRAP_BLACK; im.filter = WF_MIP_BILINEAR;
            im.level_offset[0] = (int)T->tableData.size();
            T->tableData.insert(T->tableData.end(), img.begin(), img.end());
            C.aperture_image = (int)T->texImages.size();
            T->texImages.push_back(im);
        }
        // film extent
        const float diagonal = scene.film.params.GetOneFloat("diagonal", 35.f) * .001f;
        C.film_diagonal = diagonal;
        {
            float aspect = (float)F.full_res[1] / (float)F.full_res[0];
            float x = std::sqrt(Sqr(diagonal) / (1 + Sqr(aspect)));
            float y = aspect * x;
            C.physical_extent[0] = -x / 2; C.physical_extent[1] = -y / 2; C.physical_extent[2] = x / 2; C.physical_extent[3] = y / 2;
        }
        // element interfaces
        const int nEl = (int)lensParameters.size() / 4;
        C.n_lens_elements = nEl;
        C.lens_offset = (int)T->tableData.size();
        for (int i = 0; i < nEl; ++i) {
            float curvatureRadius = lensParameters[4 * i] / 1000, thickness = lensParameters[4 * i + 1] / 1000;
            float eta = lensParameters[4 * i + 2], apDiameter = lensParameters[4 * i + 3] / 1000;
            if (curvatureRadius == 0) {
                apertureDiameter /= 1000;
                if (apertureDiameter > apDiameter) fprintf(stderr, "Warning: Aperture diameter %f is greater than maximum possible %f. Clamping it.\n", apertureDiameter, apDiameter);
                else apDiameter = apertureDiameter;
            }
            T->tableData.push_back(curvatureRadius); T->tableData.push_back(thickness); T->tableData.push_back(eta); T->tableData.push_back(apDiameter / 2);
        }
        C.n_exit_pupil_bounds = 0;
        C.exit_pupil_offset = 0;
        SceneView tmp{};
        auto view = [&]() -> const SceneView & { tmp.camera = C; tmp.film = F; tmp.tableData = T->tableData.data(); tmp.texImages = T->texImages.data(); return tmp; };
        auto thicknessAt = [&](int i) -> float & { return T->tableData[C.lens_offset + 4 * i + 1]; };
        // FocusThickLens / ComputeThickLensApproximation / ComputeCardinalPoints (cameras.cpp:815-859)
        {
            float pz[2], fz[2];
            float x = .001f * diagonal;
            float frontZ = 0;
            for (int i = 0; i < nEl; ++i) frontZ += thicknessAt(i);
            const float rearZ = thicknessAt(nEl - 1);
            auto cardinal = [](V3 inO, V3 outO, V3 outD, float *pzv, float *fzv) {
                float tf = -outO.x / outD.x;
                *fzv = -(outO + outD * tf).z;
                float tp = (inO.x - outO.x) / outD.x;
                *pzv = -(outO + outD * tp).z;
            };
            V3 sO{x, 0, frontZ + 1}, sD{0, 0, -1}, fO, fD;
            if (!TraceLensesFromScene(view(), C, sO, sD, &fO, &fD))
                Die(scene.camera.loc, "Unable to trace ray from scene to film for thick lens approximation. Is aperture stop extremely small?");
            cardinal(sO, fO, fD, &pz[0], &fz[0]);
            V3 rO{x, 0, rearZ - 1}, rD{0, 0, 1}, oO, oD;
            if (TraceLensesFromFilm(view(), C, rO, rD, &oO, &oD) == 0)
                Die(scene.camera.loc, "Unable to trace ray from film to scene for thick lens approximation. Is aperture stop extremely small?");
            cardinal(rO, oO, oD, &pz[1], &fz[1]);
            float f = fz[0] - pz[0];
            float z = -focusDistance;
            float c = (pz[1] - z - pz[0]) * (pz[1] - z - 4 * f - pz[0]);
            if (c <= 0) Die(scene.camera.loc, "Coefficient must be positive. It looks focusDistance is too short for a given lenses configuration");
            float delta = (pz[1] - z + pz[0] - std::sqrt(c)) / 2;
            thicknessAt(nEl - 1) = thicknessAt(nEl - 1) + delta;
        }
        // exit pupil bounds (cameras.cpp:861-895), one task per film-radius interval
        {
            const int nBounds = 64;
            std::vector<float> bounds((size_t)4 * nBounds);
            const SceneView &sv0 = view();
            const float rearRadius = T->tableData[C.lens_offset + 4 * (nEl - 1) + 3], rearZ = thicknessAt(nEl - 1);
            auto boundOne = [&](int i) {
                float filmX0 = (float)i / nBounds * diagonal / 2, filmX1 = (float)(i + 1) / nBounds * diagonal / 2;
                const float INF = std::numeric_limits<float>::max();
                float b[4] = {INF, INF, -INF, -INF};   // Bounds2f(): max / lowest
                const int nSamples = 1024 * 1024;
                const float pr[4] = {-1.5f * rearRadius, -1.5f * rearRadius, 1.5f * rearRadius, 1.5f * rearRadius};
                for (int k = 0; k < nSamples; ++k) {
                    V3 pFilm{Lerp((k + 0.5f) / nSamples, filmX0, filmX1), 0, 0};
                    float u0 = RadicalInverseBase(2, (uint64_t)k), u1 = RadicalInverseBase(3, (uint64_t)k);
                    V3 pRear{Lerp(u0, pr[0], pr[2]), Lerp(u1, pr[1], pr[3]), rearZ};
                    const bool inside = pRear.x >= b[0] && pRear.x <= b[2] && pRear.y >= b[1] && pRear.y <= b[3];
                    if (!inside && TraceLensesFromFilm(sv0, C, pFilm, pRear - pFilm, nullptr, nullptr)) {
                        b[0] = std::min(b[0], pRear.x); b[1] = std::min(b[1], pRear.y); b[2] = std::max(b[2], pRear.x); b[3] = std::max(b[3], pRear.y);
                    }
                }
                if (!(b[0] >= b[2] || b[1] >= b[3])) {   // !IsDegenerate: expand for the sample spacing
                    float ddx = pr[2] - pr[0], ddy = pr[3] - pr[1];
                    float e = 2 * std::sqrt(ddx * ddx + ddy * ddy) / std::sqrt((float)nSamples);
                    b[0] -= e; b[1] -= e; b[2] += e; b[3] += e;
                }
                for (int c = 0; c < 4; ++c) bounds[4 * i + c] = b[c];
            };
            unsigned nt = std::max(1u, std::min(64u, std::thread::hardware_concurrency()));
            std::vector<std::thread> threads;
            std::atomic<int> next{0};
            for (unsigned t = 0; t < nt; ++t)
                threads.emplace_back([&] { for (int i = next++; i < nBounds; i = next++) boundOne(i); });
            for (auto &th : threads) th.join();
            C.n_exit_pupil_bounds = nBounds;
            C.exit_pupil_offset = (int)T->tableData.size();
            T->tableData.insert(T->tableData.end(), bounds.begin(), bounds.end());
        }
        // CameraBase::FindMinimumDifferentials (cameras.cpp:153-203) over the generic CameraBase::GenerateRayDifferential (:116-152)
        {
            const float INF = std::numeric_limits<float>::infinity();
            V3 minPosX{INF, INF, INF}, minPosY = minPosX, minDirX = minPosX, minDirY = minPosX;
            const SceneView &sv0 = view();
            const int n = 512;
            for (int i = 0; i < n; ++i) {
                V2 pFilm{float(i) / (n - 1) * F.full_res[0], float(i) / (n - 1) * F.full_res[1]};
                CameraRayR cr = GenerateCameraRay(sv0, pFilm, 0.5f, V2{0.5f, 0.5f}, false);
                if (!cr.valid) continue;
                V3 rxo = cr.o, rxd = cr.d, ryo = cr.o, ryd = cr.d;   // RayDifferential(ray): differentials unset = the ray's own Point3f() / Vector3f()
                rxo = ryo = V3{0, 0, 0}; rxd = ryd = V3{0, 0, 0};
                for (float eps : {.05f, -.05f}) {
                    CameraRayR rx = GenerateCameraRay(sv0, V2{pFilm.x + eps, pFilm.y}, 0.5f, V2{0.5f, 0.5f}, false);
                    if (rx.valid) { rxo = cr.o + (rx.o - cr.o) / eps; rxd = cr.d + (rx.d - cr.d) / eps; break; }
                }
                for (float eps : {.05f, -.05f}) {
                    CameraRayR ry = GenerateCameraRay(sv0, V2{pFilm.x, pFilm.y + eps}, 0.5f, V2{0.5f, 0.5f}, false);
                    if (ry.valid) { ryo = cr.o + (ry.o - cr.o) / eps; ryd = cr.d + (ry.d - cr.d) / eps; break; }
                }
                wf_transform rfcT;   // CameraFromRender(v, ray.time): the camera's transformation at the ray's time (a moving camera)
                CameraRenderFromCameraAt(C, cr.time, &rfcT);
                V3 dox = XfVector(rfcT.mInv, rxo - cr.o);
                if (Length(dox) < Length(minPosX)) minPosX = dox;
                V3 doy = XfVector(rfcT.mInv, ryo - cr.o);
                if (Length(doy) < Length(minPosY)) minPosY = doy;
                V3 rd = Normalize(cr.d);
                rxd = Normalize(rxd); ryd = Normalize(ryd);
                Frame f = Frame::FromZ(rd);
                V3 df = f.ToLocal(rd);
                V3 dxf = Normalize(f.ToLocal(rxd)), dyf = Normalize(f.ToLocal(ryd));
                if (Length(dxf - df) < Length(minDirX)) minDirX = dxf - df;
                if (Length(dyf - df) < Length(minDirY)) minDirY = dyf - df;
            }
            for (int k = 0; k < 3; ++k) {
                C.minPosDifferentialX[k] = minPosX[k]; C.minPosDifferentialY[k] = minPosY[k];
                C.minDirDifferentialX[k] = minDirX[k]; C.minDirDifferentialY[k] = minDirY[k];
            }
        }
        C.lensRadius = 0; C.focalDistance = 0;
        ps.ReportUnused("Camera");
        return;
    }
    Transform screenFromCamera;
    if (scene.camera.name == "perspective") {
        C.type = WF_CAMERA_PERSPECTIVE;
        float fov = ps.GetOneFloat("fov", 90.f);
        screenFromCamera = Perspective(fov, 1e-2f, 1000.f);
    } else if (scene.camera.name == "orthographic") {
        C.type = WF_CAMERA_ORTHOGRAPHIC;
        screenFromCamera = Orthographic(0, 1);
    } else if (scene.camera.name == "spherical") {
        // SphericalCamera::Create (cameras.cpp:632-690): lens and screen window parameters are read and ignored
        C.type = WF_CAMERA_SPHERICAL;
        std::string m = ps.GetOneString("mapping", "equalarea");
        if (m == "equalarea") C.spherical_mapping = 0;
        else if (m == "equirectangular") C.spherical_mapping = 1;
        else Die(scene.camera.loc, m + ": unknown mapping for spherical camera. (Must be \"equalarea\" or \"equirectangular\".)");
        screenFromCamera = Orthographic(0, 1);  // unused by the spherical camera
        lensradius = 0;
    } else Die(scene.camera.loc, scene.camera.name + ": camera type not supported by this build (perspective, orthographic, spherical, realistic)");
    // ProjectiveCamera (cameras.h:243-263)
    Transform NDCFromScreen = Scale(1 / (sMaxX - sMinX), 1 / (sMaxY - sMinY), 1) * Translate(V3{-sMinX, -sMaxY, 0});
    Transform rasterFromNDC = Scale((float)F.full_res[0], -(float)F.full_res[1], 1);
    Transform rasterFromScreen = rasterFromNDC * NDCFromScreen;
    Transform screenFromRaster = Inverse(rasterFromScreen);
    Transform cameraFromRaster = Inverse(screenFromCamera) * screenFromRaster;
    C.cameraFromRaster = cameraFromRaster.abi();
    C.lensRadius = lensradius;
    C.focalDistance = focaldistance;
    V3 dx, dy;
    if (C.type == WF_CAMERA_PERSPECTIVE) {
        dx = cameraFromRaster.Point(V3{1, 0, 0}) - cameraFromRaster.Point(V3{0, 0, 0});
        dy = cameraFromRaster.Point(V3{0, 1, 0}) - cameraFromRaster.Point(V3{0, 0, 0});
    } else {
        dx = cameraFromRaster.Vector(V3{1, 0, 0});
        dy = cameraFromRaster.Vector(V3{0, 1, 0});
        for (int i = 0; i < 3; ++i) { C.minPosDifferentialX[i] = dx[i]; C.minPosDifferentialY[i] = dy[i]; }
    }
    for (int i = 0; i < 3; ++i) { C.dxCamera[i] = dx[i]; C.dyCamera[i] = dy[i]; }
    if (C.type == WF_CAMERA_SPHERICAL) {
        // CameraBase::FindMinimumDifferentials (cameras.cpp:153-203) over the generic CameraBase::GenerateRayDifferential
        // (cameras.cpp:116-152: finite differences of GenerateRay at +-0.05 pixel)
        const float INF = std::numeric_limits<float>::infinity();
        V3 minPosX{INF, INF, INF}, minPosY = minPosX, minDirX = minPosX, minDirY = minPosX;
        SceneView tmp{};
        tmp.camera = C;
        tmp.film = F;
        const int n = 512;
        for (int i = 0; i < n; ++i) {
            V2 pFilm{float(i) / (n - 1) * F.full_res[0], float(i) / (n - 1) * F.full_res[1]};
            CameraRayR cr = GenerateCameraRay(tmp, pFilm, 0.5f, V2{0.5f, 0.5f});
            const float eps = .05f;  // GenerateRay never fails for this camera, so the first eps is taken
            CameraRayR rx = GenerateCameraRay(tmp, V2{pFilm.x + eps, pFilm.y}, 0.5f, V2{0.5f, 0.5f});
            CameraRayR ry = GenerateCameraRay(tmp, V2{pFilm.x, pFilm.y + eps}, 0.5f, V2{0.5f, 0.5f});
            V3 rxo = cr.o + (rx.o - cr.o) / eps, rxd = cr.d + (rx.d - cr.d) / eps;
            V3 ryo = cr.o + (ry.o - cr.o) / eps, ryd = cr.d + (ry.d - cr.d) / eps;
            wf_transform rfcT;
            CameraRenderFromCameraAt(C, cr.time, &rfcT);
            V3 dox = XfVector(rfcT.mInv, rxo - cr.o);
            if (Length(dox) < Length(minPosX)) minPosX = dox;
            V3 doy = XfVector(rfcT.mInv, ryo - cr.o);
            if (Length(doy) < Length(minPosY)) minPosY = doy;
            V3 rd = Normalize(cr.d);
            rxd = Normalize(rxd); ryd = Normalize(ryd);
            Frame f = Frame::FromZ(rd);
            V3 df = f.ToLocal(rd);
            V3 dxf = Normalize(f.ToLocal(rxd)), dyf = Normalize(f.ToLocal(ryd));
            if (Length(dxf - df) < Length(minDirX)) minDirX = dxf - df;
            if (Length(dyf - df) < Length(minDirY)) minDirY = dyf - df;
        }
        for (int k = 0; k < 3; ++k) {
            C.minPosDifferentialX[k] = minPosX[k]; C.minPosDifferentialY[k] = minPosY[k];
            C.minDirDifferentialX[k] = minDirX[k]; C.minDirDifferentialY[k] = minDirY[k];
        }
    }
    if (C.type == WF_CAMERA_PERSPECTIVE) {
        // CameraBase::FindMinimumDifferentials (cameras.cpp:153-203) over PerspectiveCamera::GenerateRayDifferential
        // (cameras.cpp:429-478) with pLens = (0.5, 0.5), time = 0.5
        const float INF = std::numeric_limits<float>::infinity();
        V3 minPosX{INF, INF, INF}, minPosY = minPosX, minDirX = minPosX, minDirY = minPosX;
        const int n = 512;
        for (int i = 0; i < n; ++i) {
            float fx = float(i) / (n - 1) * F.full_res[0], fy = float(i) / (n - 1) * F.full_res[1];
            V3 pCamera = XfPoint(C.cameraFromRaster.m, V3{fx, fy, 0});
            V3 o{0, 0, 0}, d = Normalize(pCamera);
            V3 rxo, ryo, rxd, ryd;
            if (lensradius > 0) {
                V2 pLens{0, 0};  // lensRadius * SampleUniformDiskConcentric((0.5, 0.5)) = (0, 0)
                float ft = focaldistance / d.z;
                V3 pFocus = o + d * ft;
                o = V3{pLens.x, pLens.y, 0};
                d = Normalize(pFocus - o);
                V3 ddx = Normalize(pCamera + dx);
                ft = focaldistance / ddx.z;
                pFocus = V3{0, 0, 0} + (ft * ddx);
                rxo = V3{pLens.x, pLens.y, 0};
                rxd = Normalize(pFocus - rxo);
                V3 ddy = Normalize(pCamera + dy);
                ft = focaldistance / ddy.z;
                pFocus = V3{0, 0, 0} + (ft * ddy);
                ryo = V3{pLens.x, pLens.y, 0};
                ryd = Normalize(pFocus - ryo);
            } else {
                rxo = ryo = o;
                rxd = Normalize(pCamera + dx);
                ryd = Normalize(pCamera + dy);
            }
            // RenderFromCamera(RayDifferential), util/transform.h:350-360
            // (AnimatedTransform::operator()(RayDifferential), util/transform.cpp: the transformation at the ray's time
            // Lerp(sample.time = 0.5, shutterOpen, shutterClose) when the camera moves)
            wf_transform rfcT;
            CameraRenderFromCameraAt(C, Lerp(0.5f, C.shutterOpen, C.shutterClose), &rfcT);
            V3 ro = o, rd = d;
            XfRay(rfcT.m, &ro, &rd);
            rxo = XfPoint(rfcT.m, rxo); ryo = XfPoint(rfcT.m, ryo);
            rxd = XfVector(rfcT.m, rxd); ryd = XfVector(rfcT.m, ryd);
            V3 dox = XfVector(rfcT.mInv, rxo - ro);
            if (Length(dox) < Length(minPosX)) minPosX = dox;
            V3 doy = XfVector(rfcT.mInv, ryo - ro);
            if (Length(doy) < Length(minPosY)) minPosY = doy;
            rd = Normalize(rd); rxd = Normalize(rxd); ryd = Normalize(ryd);
            Frame f = Frame::FromZ(rd);
            V3 df = f.ToLocal(rd);
            V3 dxf = Normalize(f.ToLocal(rxd)), dyf = Normalize(f.ToLocal(ryd));
            if (Length(dxf - df) < Length(minDirX)) minDirX = dxf - df;
            if (Length(dyf - df) < Length(minDirY)) minDirY = dyf - df;
        }
        for (int k = 0; k < 3; ++k) {
            C.minPosDifferentialX[k] = minPosX[k]; C.minPosDifferentialY[k] = minPosY[k];
            C.minDirDifferentialX[k] = minDirX[k]; C.minDirDifferentialY[k] = minDirY[k];
        }
    }
    ps.ReportUnused("Camera");
}

// ---- shapes -----------------------------------------------------------------------------------------
struct MeshSource {
    std::vector<int> indices;
    std::vector<int> quads;  // bilinear patches: p00 p10 p01 p11 per patch (a PLY quad face f0 f1 f2 f3 is stored f0 f1 f3 f2, util/mesh.cpp:302-305)
    std::vector<V3> P, N;
    std::vector<V3> S;   // "S" shading tangents (trianglemesh only)
    std::string emissionFilename;   // bilinearmesh "emissionfilename" (resolved when the patches are built)
    std::vector<V2> uv;
};

bool ReadPLY(const std::string &fn, MeshSource *out, std::string *err);
// PLY files read ahead by a pool of threads (PrefetchPLY below: a San-Miguel-class scene has thousands of them); an entry is handed
// out once (moved), a file that failed to read stays absent and is read — and reported — again by the shape that names it
struct PlyPrefetch { std::map<std::string, MeshSource> meshes; std::map<std::string, int> uses; };
static thread_local PlyPrefetch *g_plyPrefetch = nullptr;

// TriQuadMesh::ComputeNormals (util/mesh.cpp:444-467): area-unweighted sum of the unit face normals
static void ComputeMeshNormals(MeshSource *m) {
    m->N.assign(m->P.size(), V3{0, 0, 0});
    for (size_t i = 0; i + 2 < m->indices.size(); i += 3) {
        const int v[3] = {m->indices[i], m->indices[i + 1], m->indices[i + 2]};
        const V3 v10 = m->P[v[1]] - m->P[v[0]], v21 = m->P[v[2]] - m->P[v[1]];
        V3 vn = Cross(v10, v21);
        if (LengthSquared(vn) > 0) {
            vn = vn / Length(vn);
            for (int k = 0; k < 3; ++k) m->N[v[k]] = m->N[v[k]] + vn;
        }
    }
    for (V3 &n : m->N) if (LengthSquared(n) > 0) n = n / Length(n);
}
// TriQuadMesh::Displace + Refine (util/mesh.h:91-181) as the "plymesh" shape calls it (shapes.cpp:1417-1455): every triangle
// is split at the midpoint of its longest edge until all three edges are shorter than maxDist in render space (a split edge is
// split once: the midpoint vertex is shared through the edge map), the vertices are moved along their normals by the
// displacement texture's value, the normals are recomputed.  Host-only load-time work, like the reference's.
static void DisplaceMesh(MeshSource *m, const Transform &rfo, float maxDist, const std::function<float(V3, V2)> &displacement, const std::string &loc) {
    if (m->uv.empty()) Die(loc, "Vertex uvs are currently required by Displace(). Sorry.");
    // TriQuadMesh::ConvertToOnlyTriangles (util/mesh.cpp:425-442); the quads are stored f0 f1 f3 f2 here as there
    for (size_t i = 0; i + 3 < m->quads.size(); i += 4) {
        const int *q = &m->quads[i];
        const int t[6] = {q[0], q[1], q[3], q[0], q[3], q[2]};
        m->indices.insert(m->indices.end(), t, t + 6);
    }
    m->quads.clear();
    if (m->N.empty()) ComputeMeshNormals(m);
    std::vector<int> oldTriIndices;
    oldTriIndices.swap(m->indices);
    std::map<std::pair<int, int>, int> edgeSplit;
    auto dist = [&](V3 a, V3 b) { return Distance(rfo.Point(a), rfo.Point(b)); };
    // explicit stack in the recursion's order (first child, then second)
    std::vector<std::array<int, 3>> stack;
    for (size_t i = 0; i + 2 < oldTriIndices.size(); i += 3) {
        stack.push_back({oldTriIndices[i], oldTriIndices[i + 1], oldTriIndices[i + 2]});
        while (!stack.empty()) {
            const std::array<int, 3> t = stack.back();
            stack.pop_back();
            const int v0 = t[0], v1 = t[1], v2 = t[2];
            const V3 p0 = m->P[v0], p1 = m->P[v1], p2 = m->P[v2];
            const float d01 = dist(p0, p1), d12 = dist(p1, p2), d20 = dist(p2, p0);
            if (d01 < maxDist && d12 < maxDist && d20 < maxDist) {
                m->indices.push_back(v0); m->indices.push_back(v1); m->indices.push_back(v2);
                continue;
            }
            if (m->P.size() > (size_t)1 << 28) Die(loc, "plymesh displacement: more than 2^28 vertices (\"edgelength\" too small, or a non-finite edge length)");
            std::array<int, 3> v;   // the first two vertices have the longest edge
            if (d01 > d12) { if (d01 > d20) v = {v0, v1, v2}; else v = {v2, v0, v1}; }
            else { if (d12 > d20) v = {v1, v2, v0}; else v = {v2, v0, v1}; }
            std::pair<int, int> edge(v[0], v[1]);
            if (v[0] > v[1]) std::swap(edge.first, edge.second);
            int vmid;
            auto it = edgeSplit.find(edge);
            if (it != edgeSplit.end()) vmid = it->second;
            else {
                vmid = (int)m->P.size();
                edgeSplit.emplace(edge, vmid);
                m->P.push_back((m->P[v[0]] + m->P[v[1]]) / 2.f);
                V3 nn = m->N[v[0]] + m->N[v[1]];
                if (LengthSquared(nn) > 0) nn = nn / Length(nn);
                m->N.push_back(nn);
                m->uv.push_back(V2{(m->uv[v[0]].x + m->uv[v[1]].x) / 2.f, (m->uv[v[0]].y + m->uv[v[1]].y) / 2.f});
            }
            stack.push_back({vmid, v[1], v[2]});
            stack.push_back({v[0], vmid, v[2]});
        }
    }
    for (size_t i = 0; i < m->P.size(); ++i) {
        const float d = displacement(m->P[i], m->uv[i]);
        m->P[i] = m->P[i] + V3{d * m->N[i].x, d * m->N[i].y, d * m->N[i].z};
    }
    ComputeMeshNormals(m);
}

bool LoadShapeGeometry(const ShapeEntity &sh, const std::string &baseDir, MeshSource *m) {
    const ParamSet &ps = sh.params;
    if (sh.name == "trianglemesh") {
        m->indices = ps.GetIntArray("indices");
        m->P = ps.GetPoint3fArray("P");
        m->uv = ps.GetPoint2fArray("uv");
        m->N = ps.GetTuple3Array("N", "normal");
        if (m->N.empty()) m->N = ps.GetTuple3Array("N", "normal3");
        if (m->indices.empty()) {
            if (m->P.size() == 3) m->indices = {0, 1, 2};
            else { fprintf(stderr, "Error: %s: Vertex indices \"indices\" must be provided with triangle mesh.\n", sh.loc.c_str()); return false; }
        } else while (m->indices.size() % 3) m->indices.pop_back();
        if (m->P.empty()) { fprintf(stderr, "Error: %s: Vertex positions \"P\" must be provided with triangle mesh.\n", sh.loc.c_str()); return false; }
        if (!m->uv.empty() && m->uv.size() != m->P.size()) m->uv.clear();
        if (!m->N.empty() && m->N.size() != m->P.size()) m->N.clear();
        for (int vi : m->indices) if (vi < 0 || vi >= (int)m->P.size()) { fprintf(stderr, "Error: %s: trianglemesh has out of-bounds vertex index %d\n", sh.loc.c_str(), vi); return false; }
        m->S = ps.GetTuple3Array("S", "vector3");   // shading tangents (shapes.cpp:404-409)
        if (m->S.empty()) m->S = ps.GetTuple3Array("S", "vector");
        if (!m->S.empty() && m->S.size() != m->P.size()) {
            fprintf(stderr, "Error: %s: Number of \"S\"s for triangle mesh must match \"P\"s. Discarding \"S\"s.\n", sh.loc.c_str());
            m->S.clear();
        }
        // "faceIndices" (shapes.cpp:426-433): read by the reference and handed to the textures as TextureEvalContext::faceIndex, whose only
        // consumer is the Ptex texture (not in this build, nor in the oracle's); looked up so that ReportUnused agrees with the reference
        {
            const std::vector<int> faceIndices = ps.GetIntArray("faceIndices");
            if (!faceIndices.empty() && faceIndices.size() != m->indices.size() / 3)
                fprintf(stderr, "Error: %s: Number of face indices %d does not match number of triangles %d. Discarding face indices.\n", sh.loc.c_str(),
                        (int)faceIndices.size(), (int)(m->indices.size() / 3));
        }
        return true;
    } else if (sh.name == "loopsubdiv") {
        // shapes.cpp:1473-1490
        const int nLevels = ps.GetOneInt("levels", 3);
        std::vector<int> vertexIndices = ps.GetIntArray("indices");
        if (vertexIndices.empty()) Die(sh.loc, "Vertex indices \"indices\" not provided for LoopSubdiv shape.");
        std::vector<V3> P = ps.GetPoint3fArray("P");
        if (P.empty()) Die(sh.loc, "Vertex positions \"P\" not provided for LoopSubdiv shape.");
        for (int vi : vertexIndices) if (vi < 0 || vi >= (int)P.size()) Die(sh.loc, "loopsubdiv has out of-bounds vertex index " + std::to_string(vi));
        ps.GetOneString("scheme", "loop");
        LoopSubdivide(nLevels, vertexIndices, P, &m->indices, &m->P, &m->N);
        return true;
    } else if (sh.name == "plymesh") {
        std::string fn = ps.GetOneString("filename", "");
        if (!fn.empty() && fn[0] != '/') fn = baseDir + "/" + fn;
        std::string err;
        bool have = false;
        if (g_plyPrefetch) {
            auto it = g_plyPrefetch->meshes.find(fn);
            if (it != g_plyPrefetch->meshes.end()) {
                if (--g_plyPrefetch->uses[fn] <= 0) { *m = std::move(it->second); g_plyPrefetch->meshes.erase(it); }   // last user: no copy
                else *m = it->second;
                have = true;
            }
        }
        if (!have && !ReadPLY(fn, m, &err)) Die(sh.loc, fn + ": " + err);
        return true;   // a "displacement" texture is applied by the caller (DisplaceMesh: it needs the scene's textures)
    }
    if (sh.name == "bilinearmesh") {
        // BilinearPatch::CreateMesh (shapes.cpp:910-1010)
        m->quads = ps.GetIntArray("indices");
        m->P = ps.GetPoint3fArray("P");
        m->uv = ps.GetPoint2fArray("uv");
        m->N = ps.GetTuple3Array("N", "normal");
        if (m->N.empty()) m->N = ps.GetTuple3Array("N", "normal3");
        if (m->quads.empty()) {
            if (m->P.size() == 4) m->quads = {0, 1, 2, 3};
            else { fprintf(stderr, "Error: %s: Vertex indices \"indices\" must be provided with bilinear patch mesh shape.\n", sh.loc.c_str()); return false; }
        } else while (m->quads.size() % 4) m->quads.pop_back();
        if (m->P.empty()) { fprintf(stderr, "Error: %s: Vertex positions \"P\" must be provided with bilinear patch mesh shape.\n", sh.loc.c_str()); return false; }
        if (!m->uv.empty() && m->uv.size() != m->P.size()) m->uv.clear();
        if (!m->N.empty() && m->N.size() != m->P.size()) m->N.clear();
        for (int vi : m->quads) if (vi < 0 || vi >= (int)m->P.size()) { fprintf(stderr, "Error: %s: Bilinear patch mesh has out of-bounds vertex index %d\n", sh.loc.c_str(), vi); return false; }
        (void)ps.GetIntArray("faceIndices");   // shapes.cpp:965-973: read (Ptex's face index; no consumer in this build), so not "unused"
        // "emissionfilename" (shapes.cpp:978-994): the patches are sampled by area with the image's distribution
        m->emissionFilename = ps.GetOneString("emissionfilename", "");
        if (!m->emissionFilename.empty() && m->emissionFilename[0] != '/') m->emissionFilename = baseDir + "/" + m->emissionFilename;
        if (!m->emissionFilename.empty() && !m->uv.empty()) {
            fprintf(stderr, "Error: %s: \"emissionfilename\" is currently ignored for bilinear patches if \"uv\" coordinates have been provided--sorry!\n", sh.loc.c_str());
            m->emissionFilename.clear();
        }
        return true;
    }
    Die(sh.loc, sh.name + ": shape type not supported by this build (trianglemesh, plymesh, loopsubdiv, bilinearmesh, curve, sphere, disk, cylinder)");
}

// Minimal PLY reader (ascii + binary_little_endian; vertex x,y,z[,nx,ny,nz][,u,v|s,t], face vertex_indices
// with triangle faces — TriQuadMesh::ReadPLY, util/mesh.cpp:158-420; quad faces are bilinear patches in the reference: refused)
bool ReadPLY(const std::string &fn, MeshSource *out, std::string *err) {
    // the whole file in memory; "*.gz" through zlib, as the reference's rply does (ext/rply/rply.cpp:382-393)
    std::string content;
    {
        const size_t L = fn.size();
        const bool gz = L > 3 && fn[L - 3] == '.' && tolower((unsigned char)fn[L - 2]) == 'g' && tolower((unsigned char)fn[L - 1]) == 'z';
        if (gz) {
            gzFile g = gzopen(fn.c_str(), "rb");
            if (!g) { *err = "unable to open PLY file"; return false; }
            char buf[1 << 16];
            int n;
            while ((n = gzread(g, buf, sizeof(buf))) > 0) content.append(buf, (size_t)n);
            gzclose(g);
            if (n < 0) { *err = "error reading gzipped PLY file"; return false; }
        } else {
            std::ifstream f(fn, std::ios::binary);
            if (!f) { *err = "unable to open PLY file"; return false; }
            f.seekg(0, std::ios::end);
            content.resize((size_t)f.tellg());
            f.seekg(0);
            f.read(&content[0], (std::streamsize)content.size());
        }
    }
    // only the header goes through a stream (the body of a large mesh is hundreds of megabytes)
    size_t headerEnd = content.find("end_header");
    if (headerEnd != std::string::npos) headerEnd = content.find('\n', headerEnd);
    if (headerEnd == std::string::npos) { *err = "not a PLY file"; return false; }
    ++headerEnd;
    std::istringstream in(content.substr(0, headerEnd));
    std::string line;
    std::getline(in, line);
    if (line.substr(0, 3) != "ply") { *err = "not a PLY file"; return false; }
    enum { ASCII, BLE, BBE } fmt = ASCII;
    struct Prop { std::string name, type, countType; bool list = false; };
    struct Elem { std::string name; long count = 0; std::vector<Prop> props; };
    std::vector<Elem> elems;
    while (std::getline(in, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        std::istringstream ls(line);
        std::string kw;
        ls >> kw;
        if (kw == "format") {
            std::string f; ls >> f;
            if (f == "ascii") fmt = ASCII; else if (f == "binary_little_endian") fmt = BLE; else if (f == "binary_big_endian") fmt = BBE;
            else { *err = "unknown PLY format \"" + f + "\""; return false; }
        }
        else if (kw == "element") {
            Elem e; ls >> e.name >> e.count;
            if (!ls || e.count < 0 || e.count > (1l << 31)) { *err = "malformed PLY element count"; return false; }
            elems.push_back(e);
        }
        else if (kw == "property") {
            Prop p; std::string t; ls >> t;
            if (t == "list") { p.list = true; ls >> p.countType >> p.type >> p.name; }
            else { p.type = t; ls >> p.name; }
            if (elems.empty()) { *err = "property before element"; return false; }
            elems.back().props.push_back(p);
        } else if (kw == "end_header") break;
    }
    // the body in one read; property types and roles resolved once per element (a 10 M-triangle scene reads ~60 M numbers)
    const char *cur = content.data() + headerEnd, *const bodyEnd = content.data() + content.size();
    enum Ty { I8, U8, I16, U16, I32, U32, F32, F64 };
    auto typeOf = [](const std::string &t) {
        if (t == "char" || t == "int8") return I8;
        if (t == "uchar" || t == "uint8") return U8;
        if (t == "short" || t == "int16") return I16;
        if (t == "ushort" || t == "uint16") return U16;
        if (t == "int" || t == "int32") return I32;
        if (t == "uint" || t == "uint32") return U32;
        if (t == "float" || t == "float32") return F32;
        return F64;
    };
    bool truncated = false;
    auto readNum = [&](Ty t) -> double {
        if (fmt == ASCII) {
            while (cur < bodyEnd && isspace((unsigned char)*cur)) ++cur;
            if (cur >= bodyEnd) { truncated = true; return 0; }
            char *e = nullptr;
            double v = strtod(cur, &e);
            if (e == cur) { truncated = true; return 0; }
            cur = e;
            return v;
        }
        static const int size[8] = {1, 1, 2, 2, 4, 4, 4, 8};
        if (cur + size[t] > bodyEnd) { truncated = true; return 0; }
        const char *b = cur;
        cur += size[t];
        char swapped[8];
        if (fmt == BBE && size[t] > 1) {   // binary_big_endian: reverse the bytes of every value
            for (int k = 0; k < size[t]; ++k) swapped[k] = b[size[t] - 1 - k];
            b = swapped;
        }
        switch (t) {
        case I8: return *(const int8_t *)b;
        case U8: return *(const uint8_t *)b;
        case I16: { int16_t v; memcpy(&v, b, 2); return v; }
        case U16: { uint16_t v; memcpy(&v, b, 2); return v; }
        case I32: { int32_t v; memcpy(&v, b, 4); return v; }
        case U32: { uint32_t v; memcpy(&v, b, 4); return v; }
        case F32: { float v; memcpy(&v, b, 4); return v; }
        default: { double v; memcpy(&v, b, 8); return v; }
        }
    };
    for (const Elem &e : elems) {
        struct P2 { Ty type, countType; bool list; int role; };  // role: 0..2 position, 3..5 normal, 6 / 7 uv, 8 vertex indices, -1 skipped
        std::vector<P2> props;
        for (const Prop &p : e.props) {
            P2 q{typeOf(p.type), typeOf(p.countType), p.list, -1};
            if (e.name == "vertex") {
                if (p.name == "x") q.role = 0; else if (p.name == "y") q.role = 1; else if (p.name == "z") q.role = 2;
                else if (p.name == "nx") q.role = 3; else if (p.name == "ny") q.role = 4; else if (p.name == "nz") q.role = 5;
                else if (p.name == "u" || p.name == "s" || p.name == "texture_u" || p.name == "texture_s") q.role = 6;
                else if (p.name == "v" || p.name == "t" || p.name == "texture_v" || p.name == "texture_t") q.role = 7;
            } else if (e.name == "face" && (p.name == "vertex_indices" || p.name == "vertex_index")) q.role = 8;
            props.push_back(q);
        }
        if (e.name == "vertex") {
            bool hasN = false, hasUV = false;
            // normals need nx, ny and nz, texture coordinates u and v: a partial set is ignored, never written through an empty vector
            bool r[8] = {};
            for (const P2 &p : props) if (p.role >= 0 && p.role < 8) r[p.role] = true;
            hasN = r[3] && r[4] && r[5];
            hasUV = r[6] && r[7];
            out->P.resize(e.count);
            if (hasN) out->N.resize(e.count);
            if (hasUV) out->uv.resize(e.count);
            for (long i = 0; i < e.count && !truncated; ++i)
                for (const P2 &p : props) {
                    if (p.list) { int n = (int)readNum(p.countType); for (int k = 0; k < n; ++k) readNum(p.type); continue; }
                    float v = (float)readNum(p.type);
                    switch (p.role) {
                    case 0: out->P[i].x = v; break; case 1: out->P[i].y = v; break; case 2: out->P[i].z = v; break;
                    case 3: if (hasN) out->N[i].x = v; break; case 4: if (hasN) out->N[i].y = v; break; case 5: if (hasN) out->N[i].z = v; break;
                    case 6: if (hasUV) out->uv[i].x = v; break; case 7: if (hasUV) out->uv[i].y = v; break;
                    default: break;
                    }
                }
        } else if (e.name == "face") {
            out->indices.reserve(out->indices.size() + 3 * (size_t)e.count);
            for (long i = 0; i < e.count && !truncated; ++i)
                for (const P2 &p : props) {
                    if (!p.list) { readNum(p.type); continue; }
                    int n = (int)readNum(p.countType);
                    if (p.role != 8) { for (int k = 0; k < n; ++k) readNum(p.type); continue; }
                    if (n == 3) { for (int k = 0; k < 3; ++k) out->indices.push_back((int)readNum(p.type)); }
                    else if (n == 4) {
                        // quad faces become BilinearPatch shapes (shapes.cpp:1465-1472); face order 0, 1, 3, 2 (util/mesh.cpp:302-305)
                        int q[4];
                        for (int k = 0; k < 4; ++k) q[k] = (int)readNum(p.type);
                        out->quads.push_back(q[0]); out->quads.push_back(q[1]); out->quads.push_back(q[3]); out->quads.push_back(q[2]);
                    } else { *err = "only triangle and quad faces are supported (as in the reference, util/mesh.cpp:290-310)"; return false; }
                }
        } else {
            for (long i = 0; i < e.count && !truncated; ++i)
                for (const P2 &p : props) {
                    if (p.list) { int n = (int)readNum(p.countType); for (int k = 0; k < n; ++k) readNum(p.type); }
                    else readNum(p.type);
                }
        }
    }
    if (truncated) { *err = "unexpected end of PLY data"; return false; }
    for (int vi : out->indices) if (vi < 0 || vi >= (int)out->P.size()) { *err = "vertex index out of bounds"; return false; }
    for (int vi : out->quads) if (vi < 0 || vi >= (int)out->P.size()) { *err = "vertex index out of bounds"; return false; }
    return true;
}

// ---- the scene's tables, stage by stage ---------------------------------------------------------------
struct PendingAreaLight { int mesh; int lightEntity; Transform renderFromObject; };
struct PendingSphere { wf_quadric s; B3 bounds; float area = 0; /* curves: Curve::Area */ };
// a definition's nested placement (an animated shape created inside it) — the record every use of the definition repeats
struct NestedPlacement { const InstanceUse *use = nullptr; wf_instance record{}; };
// the primitive lists in the reference's creation order (scene.cpp:1386-1470): (primitive id, bounds).  Quadric ids
// are patched once the triangle count is known (they follow ALL triangles): stored as -1 - quadric index meanwhile.
typedef std::vector<std::pair<int, B3>> PrimList;
struct AccelParams { int splitCode; /* 0 sah, 1 hlbvh, 2 middle, 3 equal */ int maxPrims; };
// what the DiffuseAreaLights of one shape share (DiffuseAreaLight::Create, lights.cpp:873-941)
struct AreaLightParams { bool twoSided, alphaZero; int alphaTex, spectrumOffset, image; float scale, power, imageLumAvg, LemitMax; };
// an RGB image registered as a light's emission: its pixels and its wf_tex_image
struct LightImage { std::vector<float> rgb; int w = 0, h = 0, id = -1; };

// fn(i) for every i < n, on a pool of threads that take the items in turn (WF_BUILD_THREADS: how many); fn must not throw
template <typename F> void ParallelFor(size_t n, F fn) {
    std::atomic<size_t> next{0};
    unsigned nt = std::max(1u, std::min((unsigned)n, std::thread::hardware_concurrency()));
    if (const char *e = getenv("WF_BUILD_THREADS")) nt = std::max(1, atoi(e));
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt && n > 0; ++t)
        pool.emplace_back([&] { for (size_t i = next++; i < n; i = next++) fn(i); });
    for (auto &th : pool) th.join();
}

bool IsAffine(const Transform &t) { return t.m.m[3][0] == 0 && t.m.m[3][1] == 0 && t.m.m[3][2] == 0 && t.m.m[3][3] == 1; }

// BilinearPatch::NormalBounds (shapes.cpp:1080-1126): the cone's axis (normalised once) and the cosine of its spread
void PatchNormalBounds(const BlpData &d, bool flip, V3 *w, float *cosTheta) {
    const V3 p00 = d.p00, p10 = d.p10, p01 = d.p01, p11 = d.p11;
    auto eq = [](V3 a, V3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; };
    if (eq(p00, p10) || eq(p10, p11) || eq(p11, p01) || eq(p01, p00)) {
        V3 dpdu = LerpV(0.5f, p10, p11) - LerpV(0.5f, p00, p01);
        V3 dpdv = LerpV(0.5f, p01, p11) - LerpV(0.5f, p00, p10);
        V3 n = Normalize(Cross(dpdu, dpdv));
        if (d.hasN) {
            N3 ns = (d.n00 + d.n10 + d.n01 + d.n11) / 4;
            n = toV(FaceForward(toN(n), ns));
        } else if (flip) n = -n;
        *w = Normalize(n);
        *cosTheta = 1;
    } else {
        V3 n00 = Normalize(Cross(p10 - p00, p01 - p00));
        if (d.hasN) n00 = toV(FaceForward(toN(n00), d.n00));
        else if (flip) n00 = -n00;
        V3 n10 = Normalize(Cross(p11 - p10, p00 - p10));
        V3 n01 = Normalize(Cross(p00 - p01, p11 - p01));
        V3 n11 = Normalize(Cross(p01 - p11, p10 - p11));
        if (d.hasN) {
            n10 = toV(FaceForward(toN(n10), d.n10));
            n01 = toV(FaceForward(toN(n01), d.n01));
            n11 = toV(FaceForward(toN(n11), d.n11));
        } else if (flip) { n10 = -n10; n01 = -n01; n11 = -n11; }
        V3 n = Normalize(n00 + n10 + n01 + n11);
        float ct = std::min(std::min(Dot(n, n00), Dot(n, n01)), std::min(Dot(n, n10), Dot(n, n11)));
        *w = Normalize(n);   // DirectionCone(w, cosTheta) normalises
        *cosTheta = ct < -1 ? -1 : (ct > 1 ? 1 : ct);
    }
}

// a vertex, radius or transformation that is not finite (NaN / infinite bounds) would index outside the builders' buckets:
// refused here, before any builder sees it (the reference's builder has the same undefined bucket index, cpu/aggregates.cpp:268-275)
void RequireFinite(const PrimList &prims, const std::string &what) {
    // ... and neither may the extent of the whole set overflow: the SAH costs are surface areas, the bucket index divides by the
    // centroid extent — with infinite values no split is ever chosen and the recursion (the reference's too) never ends
    B3 all;
    for (const auto &p : prims) all = Union(all, p.second);
    if (!prims.empty()) {
        const V3 d = all.Diagonal();
        // (count x surface area: the largest SAH cost the builders can form)
        if (!std::isfinite(d.x) || !std::isfinite(d.y) || !std::isfinite(d.z) || !std::isfinite((float)prims.size() * all.SurfaceArea()))
            Die("", what + ": the extent of the primitives overflows single precision (coordinates of the order of 1e19 or more)");
    }
    for (const auto &p : prims) {
        const B3 &b = p.second;
        const float v[6] = {b.pMin.x, b.pMin.y, b.pMin.z, b.pMax.x, b.pMax.y, b.pMax.z};
        for (float f : v)
            if (!std::isfinite(f)) Die("", what + ": a primitive has bounds that are not finite (a NaN or infinite vertex position, radius or transformation)");
    }
}

// Everything BuildSceneTables' stages share.  The stages run in the order of the reference's BasicScene::Create* (scene.cpp); each appends
// to the tables — ids are positions, so neither the order of the stages nor the order of appends inside one may change.
struct SceneBuild {
    const ParsedScene &scene;
    RenderOptions opt;
    SceneTables *T;
    TexBuilder tb;
    std::map<std::string, int> mediumIds;
    std::vector<int> materialIds;
    std::string lightSamplerName;
    // shapes
    PlyPrefetch prefetch;
    std::vector<PendingAreaLight> pendingArea;
    bool anyMediumInterface = false;
    std::vector<PendingSphere> spheres;             // every quadric, patch and curve segment, in creation order
    std::map<int, int> sphereOfMesh;                // mesh id -> its sphere / disk / cylinder
    std::map<int, std::vector<int>> patchesOfMesh;  // mesh id -> its bilinear patches (indices into spheres)
    std::map<int, std::vector<int>> curvesOfMesh;   // mesh id -> its Curve primitives (indices into spheres)
    PrimList topPrims;
    // instance definitions: only those that are used, each with a BVH of its own
    std::map<std::string, int> defIndex;
    std::vector<PrimList> defPrims;
    std::vector<std::vector<NestedPlacement>> defNested;
    std::vector<B3> defBounds;
    std::vector<InstanceUse> allUses;
    // lights
    std::vector<std::pair<int, LightBoundsH>> bvhLights;
    B3 allLightBounds;
    // WF_LOAD_TIMING=1: where the load time goes (stderr)
    const bool timing = getenv("WF_LOAD_TIMING") != nullptr;
    std::chrono::steady_clock::time_point tPhase = std::chrono::steady_clock::now();

    SceneBuild(const ParsedScene &scene, const RenderOptions &opt, SceneTables *T) : scene(scene), opt(opt), T(T) {}
    ~SceneBuild() { g_plyPrefetch = nullptr; }
    void Tick(const char *what) {
        if (!timing) return;
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[load] %-44s %7.3f s\n", what, std::chrono::duration<double>(now - tPhase).count());
        tPhase = now;
    }
    int MediumId(const std::string &name, const std::string &loc) const {
        if (name.empty()) return -1;
        auto it = mediumIds.find(name);
        if (it == mediumIds.end()) Die(loc, name + ": medium is not defined.");
        return it->second;
    }
    void AddLightBounds(int lightId, const LightBoundsH &lb) {
        if (lb.phi > 0) { bvhLights.emplace_back(lightId, lb); allLightBounds = Union(allLightBounds, lb.bounds); }
    }
    // a light without Bounds() (distant, infinite): sampled with the infinite lights
    void AddInfinite(wf_light l) {
        l.infinite_index = (int)T->infiniteLights.size();
        T->infiniteLights.push_back((int)T->lights.size());
        T->lights.push_back(l);
    }
    // a light at the point p, with its LightBounds
    void AddLightAt(const wf_light &l, V3 p, V3 w, float phi, float cosTheta_o, float cosTheta_e) {
        const int lightId = (int)T->lights.size();
        T->lights.push_back(l);
        LightBoundsH lb;
        lb.bounds.pMin = lb.bounds.pMax = p;
        lb.w = w; lb.phi = phi; lb.cosTheta_o = cosTheta_o; lb.cosTheta_e = cosTheta_e; lb.twoSided = false;
        AddLightBounds(lightId, lb);
    }

    // the part of a shape that is not geometry: material, alpha, media, area light (scene.cpp:1395-1440)
    void CommitMesh(wf_mesh &mesh, int meshId, const ShapeEntity &sh, const Transform &rfo, bool instanced) {
        if (!sh.materialName.empty()) {
            auto it = tb.namedMaterialIds.find(sh.materialName);
            if (it == tb.namedMaterialIds.end()) Die(sh.loc, sh.materialName + ": no named material defined.");
            mesh.material = it->second;
        } else mesh.material = materialIds.at(sh.materialIndex);
        if (T->materials[mesh.material].type == WF_MAT_INTERFACE) mesh.material = -1;
        mesh.first_light = -1;
        mesh.alpha_tex = -1;
        // getAlphaTexture (scene.cpp:1270-1286): a named float texture, or a constant when "float alpha" < 1
        if (!sh.params.GetTexture("alpha").empty()) mesh.alpha_tex = tb.GetFloatTextureOrNull(sh.params, "alpha");
        else if (float alpha = sh.params.GetOneFloat("alpha", 1.f); alpha < 1.f) mesh.alpha_tex = tb.FloatConst(alpha);
        if (mesh.alpha_tex >= 0 && sh.name == "curve") {
            // alpha on curves (round 5): the interaction of such a hit is rebuilt by replaying GeometricPrimitive::Intersect's alpha
            // recursion, which only the material stage does (wf_shapes.h HitInteraction<GENERAL, CURVE_ALPHA>)
            const int mt = mesh.material < 0 ? (int)WF_MAT_INTERFACE : T->materials[mesh.material].type;
            if (mt == WF_MAT_INTERFACE || mt == WF_MAT_MIX || mt == WF_MAT_SUBSURFACE || sh.lightIndex >= 0)
                Die(sh.loc, "an alpha texture on a curve with an interface / mix / subsurface material or an area light is not supported by this build");
        }
        mesh.medium_inside = MediumId(sh.insideMedium, sh.loc);
        mesh.medium_outside = MediumId(sh.outsideMedium, sh.loc);
        if (!sh.insideMedium.empty() || !sh.outsideMedium.empty()) anyMediumInterface = true;
        T->meshes.push_back(mesh);
        if (sh.lightIndex >= 0 && !instanced) {
            if (mesh.material < 0) fprintf(stderr, "Warning: %s: Ignoring area light specification for shape with \"interface\" material.\n", sh.loc.c_str());
            else pendingArea.push_back({meshId, sh.lightIndex, rfo});
        }
        sh.params.ReportUnused("Shape");
    }

    // the wf_mesh of a shape that is not a triangle mesh (quadric, curve): first_tri is set to its first primitive's id once the triangle count is known
    wf_mesh MeshWithoutTriangles(const ShapeEntity &sh) const {
        wf_mesh mesh{};
        mesh.first_tri = -1;
        mesh.ntris = 0;
        mesh.first_vertex = (int)T->P.size() / 3;
        mesh.nverts = 0;
        mesh.flags = 0;
        if (sh.reverseOrientation ^ sh.renderFromObject.SwapsHandedness()) mesh.flags |= WF_MESH_FLIP_NORMAL;
        if (sh.reverseOrientation) mesh.flags |= WF_MESH_REVERSE_ORIENTATION;
        return mesh;
    }

    void AddShape(const ShapeEntity &sh, PrimList *prims, bool inDefinition) {
        if (sh.name == "sphere" || sh.name == "disk" || sh.name == "cylinder") AddQuadric(sh, prims);
        else if (sh.name == "curve") AddCurve(sh, prims, inDefinition);
        else AddMesh(sh, prims, inDefinition);
    }

    void AddQuadric(const ShapeEntity &sh, PrimList *prims) {
        // Sphere / Disk / Cylinder::Create + ctors (shapes.cpp:71-81,106-115,132-142; shapes.h:117-129,387-398,737-748);
        // kept in object space like the reference's
        const Transform &rfo = sh.renderFromObject;
        const ParamSet &ps = sh.params;
        float radius = ps.GetOneFloat("radius", 1.f);
        auto clampf = [](float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); };
        PendingSphere p{};
        p.s.radius = radius;
        if (sh.name == "sphere") {
            p.s.type = WF_QUADRIC_SPHERE;
            float zmin = ps.GetOneFloat("zmin", -radius), zmax = ps.GetOneFloat("zmax", radius);
            p.s.z_min = clampf(std::min(zmin, zmax), -radius, radius);
            p.s.z_max = clampf(std::max(zmin, zmax), -radius, radius);
            p.s.theta_z_min = std::acos(clampf(std::min(zmin, zmax) / radius, -1, 1));
            p.s.theta_z_max = std::acos(clampf(std::max(zmin, zmax) / radius, -1, 1));
        } else if (sh.name == "disk") {
            p.s.type = WF_QUADRIC_DISK;
            p.s.z_min = p.s.z_max = ps.GetOneFloat("height", 0.f);
            p.s.inner_radius = ps.GetOneFloat("innerradius", 0.f);
        } else {
            p.s.type = WF_QUADRIC_CYLINDER;
            float zmin = ps.GetOneFloat("zmin", -1.f), zmax = ps.GetOneFloat("zmax", 1.f);
            p.s.z_min = std::min(zmin, zmax);
            p.s.z_max = std::max(zmin, zmax);
        }
        float phimax = ps.GetOneFloat("phimax", 360.f);
        p.s.phi_max = Radians(clampf(phimax, 0, 360));
        p.s.render_from_object = rfo.abi();
        if (!IsAffine(rfo)) Die(sh.loc, "sphere: only affine transformations are supported");
        // Sphere::Bounds (shapes.cpp:33-36) through Transform::operator()(Bounds3f) (util/transform.cpp:134-139)
        V3 lo{-radius, -radius, p.s.z_min}, hi{radius, radius, p.s.z_max};
        for (int c = 0; c < 8; ++c) p.bounds = Union(p.bounds, rfo.Point(V3{(c & 1) ? hi.x : lo.x, (c & 2) ? hi.y : lo.y, (c & 4) ? hi.z : lo.z}));
        prims->emplace_back(-1 - (int)spheres.size(), p.bounds);
        wf_mesh mesh = MeshWithoutTriangles(sh);
        int meshId = (int)T->meshes.size();
        p.s.mesh = meshId;
        sphereOfMesh[meshId] = (int)spheres.size();
        spheres.push_back(p);
        // (not inDefinition, unlike curves and meshes: a quadric's area light inside an object definition is created)
        CommitMesh(mesh, meshId, sh, rfo, false);
    }

    void AddCurve(const ShapeEntity &sh, PrimList *prims, bool inDefinition) {
        // Curve::Create + CreateCurve + CurveCommon (shapes.cpp:761-900, 494-517, 458-481): every Bezier / b-spline segment becomes
        // 2^splitdepth Curve primitives over sub-ranges of u, all sharing the shape's wf_mesh
        const Transform &rfo = sh.renderFromObject;
        const ParamSet &ps = sh.params;
        float width = ps.GetOneFloat("width", 1.f);
        float width0 = ps.GetOneFloat("width0", width), width1 = ps.GetOneFloat("width1", width);
        int degree = ps.GetOneInt("degree", 3);
        if (degree != 2 && degree != 3) Die(sh.loc, "Invalid degree " + std::to_string(degree) + ": only degree 2 and 3 curves are supported.");
        std::string basis = ps.GetOneString("basis", "bezier");
        if (basis != "bezier" && basis != "bspline") Die(sh.loc, "Invalid basis \"" + basis + "\": only \"bezier\" and \"bspline\" are supported.");
        std::vector<V3> cp = ps.GetTuple3Array("P", "point3");
        int nSegments;
        if (basis == "bezier") {
            if ((((int)cp.size() - 1 - degree) % degree) != 0 || (int)cp.size() < degree + 1)
                Die(sh.loc, "Invalid number of control points " + std::to_string(cp.size()) + " for the degree " + std::to_string(degree) + " Bezier basis.");
            nSegments = ((int)cp.size() - 1) / degree;
        } else {
            if ((int)cp.size() < degree + 1) Die(sh.loc, "Invalid number of control points " + std::to_string(cp.size()) + " for the degree " + std::to_string(degree) + " b-spline basis.");
            nSegments = (int)cp.size() - degree;
        }
        std::string curveType = ps.GetOneString("type", "flat");
        int type = curveType == "flat" ? 0 : curveType == "cylinder" ? 1 : curveType == "ribbon" ? 2 : -1;
        if (type < 0) { fprintf(stderr, "Error: %s: Unknown curve type \"%s\".  Using \"cylinder\".\n", sh.loc.c_str(), curveType.c_str()); type = 1; }
        std::vector<V3> nrm = ps.GetTuple3Array("N", "normal");
        if (!nrm.empty()) {
            if (type != 2) { fprintf(stderr, "Warning: Curve normals are only used with \"ribbon\" type curves.\n"); nrm.clear(); }
            else if ((int)nrm.size() != nSegments + 1) Die(sh.loc, "Invalid number of normals " + std::to_string(nrm.size()) + ": must provide " + std::to_string(nSegments + 1) + " normals for ribbon curves with " + std::to_string(nSegments) + " segments.");
        } else if (type == 2) Die(sh.loc, "Must provide normals \"N\" at curve endpoints with ribbon curves.");
        const int sd = ps.GetOneInt("splitdepth", 3);
        if (!IsAffine(rfo)) Die(sh.loc, "curve: only affine transformations are supported");
        wf_mesh mesh = MeshWithoutTriangles(sh);
        const int meshId = (int)T->meshes.size();
        auto lerp3 = [](float t, V3 a, V3 b) { return (1 - t) * a + t * b; };
        int cpOffset = 0;
        for (int seg = 0; seg < nSegments; ++seg) {
            V3 b[4];
            const V3 *c = &cp[cpOffset];
            if (basis == "bezier") {
                if (degree == 2) { b[0] = c[0]; b[1] = lerp3(2.f / 3.f, c[0], c[1]); b[2] = lerp3(1.f / 3.f, c[1], c[2]); b[3] = c[2]; }   // ElevateQuadraticBezierToCubic
                else for (int i = 0; i < 4; ++i) b[i] = c[i];
                cpOffset += degree;
            } else {
                if (degree == 2) {
                    // QuadraticBSplineToBezier, then elevated (util/splines.h:76-91)
                    V3 q0 = lerp3(0.5f, c[0], c[1]), q1 = c[1], q2 = lerp3(0.5f, c[1], c[2]);
                    b[0] = q0; b[1] = lerp3(2.f / 3.f, q0, q1); b[2] = lerp3(1.f / 3.f, q1, q2); b[3] = q2;
                } else {
                    // CubicBSplineToBezier (util/splines.h:93-110)
                    V3 p122 = lerp3(2.f / 3.f, c[0], c[1]), p223 = lerp3(1.f / 3.f, c[1], c[2]), p233 = lerp3(2.f / 3.f, c[1], c[2]), p334 = lerp3(1.f / 3.f, c[2], c[3]);
                    b[0] = lerp3(0.5f, p122, p223); b[1] = p223; b[2] = p233; b[3] = lerp3(0.5f, p233, p334);
                }
                ++cpOffset;
            }
            const float w0 = Lerp(float(seg) / float(nSegments), width0, width1), w1 = Lerp(float(seg + 1) / float(nSegments), width0, width1);
            PendingSphere proto{};
            proto.s.type = WF_QUADRIC_CURVE;
            proto.s.mesh = meshId;
            proto.s.radius = w0;
            proto.s.theta_z_min = w1;
            proto.s.inner_radius = (float)type;
            for (int i = 0; i < 4; ++i) { proto.s.ext[3 * i] = b[i].x; proto.s.ext[3 * i + 1] = b[i].y; proto.s.ext[3 * i + 2] = b[i].z; }
            if (!nrm.empty()) {
                // CurveCommon ctor: normalised end normals, the angle between them and 1 / sin of it
                V3 n0 = Normalize(nrm[seg]), n1 = Normalize(nrm[seg + 1]);
                auto safeASin = [](float x) { return std::asin(x < -1 ? -1.f : (x > 1 ? 1.f : x)); };
                float normalAngle = Dot(n0, n1) < 0 ? Pi - 2 * safeASin(Length(n0 + n1) / 2) : 2 * safeASin(Length(n1 - n0) / 2);
                proto.s.theta_z_max = normalAngle;
                proto.s.phi_max = 1 / std::sin(normalAngle);
                proto.s.ext[12] = n0.x; proto.s.ext[13] = n0.y; proto.s.ext[14] = n0.z;
                proto.s.ext[15] = n1.x; proto.s.ext[16] = n1.y; proto.s.ext[17] = n1.z;
            }
            proto.s.render_from_object = rfo.abi();
            const int nSplit = 1 << sd;
            for (int i = 0; i < nSplit; ++i) {
                PendingSphere p = proto;
                const float uMin = i / (float)nSplit, uMax = (i + 1) / (float)nSplit;
                p.s.z_min = uMin; p.s.z_max = uMax;
                // Curve::Bounds (shapes.cpp:519-528): the control points of the u-range, expanded by half the larger width, transformed
                V3 cs[4];
                if (uMin == 0 && uMax == 1) for (int k = 0; k < 4; ++k) cs[k] = b[k];
                else CubicBezierControlPoints(b, uMin, uMax, cs);
                B3 ob;
                ob = Union(Union(Union(Union(ob, cs[0]), cs[1]), cs[2]), cs[3]);
                const float e = std::max(Lerp(uMin, w0, w1), Lerp(uMax, w0, w1)) * 0.5f;
                ob.pMin = ob.pMin - V3{e, e, e}; ob.pMax = ob.pMax + V3{e, e, e};
                for (int cnr = 0; cnr < 8; ++cnr)
                    p.bounds = Union(p.bounds, rfo.Point(V3{(cnr & 1) ? ob.pMax.x : ob.pMin.x, (cnr & 2) ? ob.pMax.y : ob.pMin.y, (cnr & 4) ? ob.pMax.z : ob.pMin.z}));
                {
                    // Curve::Area (shapes.cpp:530-540): the control polygon's length of the u-range times the average width
                    V3 ca[4];
                    CubicBezierControlPoints(b, uMin, uMax, ca);
                    const float width0u = Lerp(uMin, w0, w1), width1u = Lerp(uMax, w0, w1);
                    const float avgWidth = (width0u + width1u) * 0.5f;
                    float approxLength = 0.f;
                    for (int k = 0; k < 3; ++k) approxLength += Length(ca[k] - ca[k + 1]);
                    p.area = approxLength * avgWidth;
                }
                prims->emplace_back(-1 - (int)spheres.size(), p.bounds);
                curvesOfMesh[meshId].push_back((int)spheres.size());
                spheres.push_back(p);
            }
        }
        CommitMesh(mesh, meshId, sh, rfo, inDefinition);
    }

    void AddMesh(const ShapeEntity &sh, PrimList *prims, bool inDefinition) {
        MeshSource src;
        if (!LoadShapeGeometry(sh, scene.baseDir, &src)) return;
        const Transform &rfo = sh.renderFromObject;
        if (sh.name == "plymesh" && !sh.params.GetTexture("displacement").empty()) {
            // shapes.cpp:1417-1455: UniversalTextureEvaluator on a TextureEvalContext that holds only p (object space) and uv
            const std::string texName = sh.params.GetTexture("displacement");
            auto it = tb.floatTextures.find(texName);
            if (it == tb.floatTextures.end()) Die(sh.loc, texName + ": no such texture defined.");
            const int texId = it->second;
            float edgeLength = sh.params.GetOneFloat("edgelength", 1.f);
            edgeLength *= opt.displacementEdgeScale;   // Options->displacementEdgeScale (--displacement-edge-scale)
            SceneView tv{};
            tv.textures = T->textures.data(); tv.texImages = T->texImages.data(); tv.tableData = T->tableData.data();
            tv.lightXforms = T->lightTransforms.data(); tv.noisePerm = T->noisePerm.empty() ? nullptr : T->noisePerm.data();
            tv.spectra = T->pool.spectra.data(); tv.spectrumData = T->pool.data.data();
            tv.self = &tv;
            DisplaceMesh(&src, rfo, edgeLength, [&](V3 p, V2 uv) { TexCtx tc; tc.p = p; tc.uv = uv; return EvalFloatTexture(tv, texId, tc); }, sh.loc);
            src.S.clear();   // the displaced mesh is created without tangents (shapes.cpp:1458-1461)
        }
        wf_mesh mesh{};
        mesh.first_tri = (int)T->triIndices.size() / 3;
        mesh.ntris = (int)src.indices.size() / 3;
        mesh.first_vertex = (int)T->P.size() / 3;
        mesh.nverts = (int)src.P.size();
        bool swaps = rfo.SwapsHandedness();
        mesh.flags = 0;
        if (!src.N.empty()) mesh.flags |= WF_MESH_HAS_N;
        if (!src.uv.empty()) mesh.flags |= WF_MESH_HAS_UV;
        if (sh.reverseOrientation ^ swaps) mesh.flags |= WF_MESH_FLIP_NORMAL;
        if (!src.S.empty() && src.S.size() == src.P.size()) {   // TriangleMesh ctor, util/mesh.cpp:58-63: renderFromObject(Vector3f)
            mesh.flags |= WF_MESH_HAS_S;
            mesh.first_s = (int)(T->S.size() / 3);
            for (const V3 &s : src.S) { const V3 r = rfo.Vector(s); T->S.push_back(r.x); T->S.push_back(r.y); T->S.push_back(r.z); }
        }
        for (size_t i = 0; i < src.P.size(); ++i) {
            V3 p = rfo.Point(src.P[i]);
            if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z))
                Die(sh.loc, sh.name + ": vertex " + std::to_string(i) + " is not finite in render space (a NaN or infinite position or transformation)");
            T->P.push_back(p.x); T->P.push_back(p.y); T->P.push_back(p.z);
            N3 n{0, 0, 0};
            if (!src.N.empty()) {
                n = rfo.Normal(toN(src.N[i]));
                if (sh.reverseOrientation) n = -n;
            }
            T->N.push_back(n.x); T->N.push_back(n.y); T->N.push_back(n.z);
            V2 uv{0, 0};
            if (!src.uv.empty()) uv = src.uv[i];
            T->UV.push_back(uv.x); T->UV.push_back(uv.y);
        }
        int meshId = (int)T->meshes.size();
        for (int vi : src.indices) T->triIndices.push_back(mesh.first_vertex + vi);
        for (int i = 0; i < mesh.ntris; ++i) {
            T->triMesh.push_back(meshId);
            prims->emplace_back(mesh.first_tri + i, TriangleBounds(T->P, T->triIndices, mesh.first_tri + i));
        }
        if (!src.quads.empty()) AddPatches(sh, src, rfo, mesh, prims, inDefinition);
        else CommitMesh(mesh, meshId, sh, rfo, inDefinition);
    }

    // The quad faces of a mesh: BilinearPatchMesh + BilinearPatch::CreatePatches (util/mesh.cpp:183-230, shapes.cpp:1040-1060): after the shape's triangles,
    // in render space, sharing the shape's wf_mesh (material, media, orientation)
    // a PLY file with both triangle and quad faces: the patches get a wf_mesh entry of their own (same vertices, material, alpha,
    // media), so that a hit finds its emitter as first_light + (primitive id - first_tri) in either part; the reference creates
    // the triangles' lights first, then the patches' (shapes.cpp:1458-1471, scene.cpp:1290-1340)
    void AddPatches(const ShapeEntity &sh, const MeshSource &src, const Transform &rfo, wf_mesh &mesh, PrimList *prims, bool inDefinition) {
        const int meshId = (int)T->meshes.size();
        int patchMeshId = meshId;
        wf_mesh patchMesh = mesh;
        if (mesh.ntris > 0) {
            CommitMesh(mesh, meshId, sh, rfo, inDefinition);
            patchMeshId = (int)T->meshes.size();
            patchMesh.ntris = 0;
        }
        patchMesh.first_tri = -1;  // set to the first patch's primitive id once the triangle count is known
        const size_t v0 = (size_t)mesh.first_vertex;
        auto P3 = [&](int vi) { return V3{T->P[3 * (v0 + vi)], T->P[3 * (v0 + vi) + 1], T->P[3 * (v0 + vi) + 2]}; };
        auto N3f = [&](int vi) { return V3{T->N[3 * (v0 + vi)], T->N[3 * (v0 + vi) + 1], T->N[3 * (v0 + vi) + 2]}; };
        auto UV2 = [&](int vi) { return V2{T->UV[2 * (v0 + vi)], T->UV[2 * (v0 + vi) + 1]}; };
        // BilinearPatchMesh::imageDistribution (shapes.cpp:985-993): Image::Read, FlipY, GetSamplingDistribution (the average of
        // ALL the image's channels per pixel, util/image.cpp:440-470), PiecewiseConstant2D over [0,1]^2; one table per mesh, its
        // descriptor in every patch record (ext[0..7], flag bit 3)
        wf_pc2d emissionDist{};
        bool haveEmissionDist = false;
        if (!src.emissionFilename.empty()) {
            HostImage img;
            try { ReadImage(src.emissionFilename, ColorEnc(), &img); } catch (const SceneError &e) { Die(sh.loc, std::string(e.what()).substr(7)); }
            std::vector<float> d((size_t)img.w * img.h);
            for (int y = 0; y < img.h; ++y)
                for (int x = 0; x < img.w; ++x) {
                    float sum = 0;
                    const size_t src0 = ((size_t)(img.h - 1 - y) * img.w + x) * img.nc;   // FlipY
                    for (int c = 0; c < img.nc; ++c) sum += img.Get(src0 + c);
                    d[(size_t)y * img.w + x] = sum / img.nc;
                }
            emissionDist = AppendPC2D(&T->tableData, d, img.w, img.h);
            haveEmissionDist = true;
        }
        for (size_t q = 0; q + 3 < src.quads.size(); q += 4) {
            PendingSphere p{};
            p.s.type = WF_QUADRIC_BILINEAR;
            p.s.mesh = patchMeshId;
            p.s.pad[0] = (float)((src.N.empty() ? 0 : 1) | (src.uv.empty() ? 0 : 2) | (haveEmissionDist ? 8 : 0));
            if (haveEmissionDist) memcpy(p.s.ext, &emissionDist, sizeof(emissionDist));
            float *a = &p.s.render_from_object.m[0][0], *b = &p.s.render_from_object.mInv[0][0];
            const int *vi = &src.quads[q];
            for (int k = 0; k < 4; ++k) {
                V3 pk = P3(vi[k]), nk = N3f(vi[k]);
                a[3 * k] = pk.x; a[3 * k + 1] = pk.y; a[3 * k + 2] = pk.z;
                b[3 * k] = nk.x; b[3 * k + 1] = nk.y; b[3 * k + 2] = nk.z;
            }
            V2 u00 = UV2(vi[0]), u10 = UV2(vi[1]), u01 = UV2(vi[2]), u11 = UV2(vi[3]);
            a[12] = u00.x; a[13] = u00.y; a[14] = u10.x; a[15] = u10.y;
            b[12] = u01.x; b[13] = u01.y; b[14] = u11.x; b[15] = u11.y;
            // BilinearPatch::Bounds (shapes.cpp:1070-1078)
            V3 p00 = P3(vi[0]), p10 = P3(vi[1]), p01 = P3(vi[2]), p11 = P3(vi[3]);
            p.bounds = Union(Union(Union(B3(), p00), p01), Union(Union(B3(), p10), p11));
            // BilinearPatch ctor (shapes.cpp:1036-1067): IsRectangle() and the area, kept in the record (flag bit 2, radius field)
            const BlpData bd = LoadBlp(p.s);
            const bool rect = BlpIsRectangle(bd);
            if (rect) p.s.pad[0] = (float)((int)p.s.pad[0] | 4);
            p.s.radius = BlpArea(bd, rect);
            prims->emplace_back(-1 - (int)spheres.size(), p.bounds);
            patchesOfMesh[patchMeshId].push_back((int)spheres.size());
            spheres.push_back(p);
        }
        CommitMesh(patchMesh, patchMeshId, sh, rfo, inDefinition);
    }

    // reads every PLY file the scene uses with a pool of threads first (the shape stages then find them in memory)
    void PrefetchPly() {
        std::vector<std::string> files;
        auto want = [&](const ShapeEntity &sh) {
            if (sh.name != "plymesh") return;
            std::string fn = sh.params.GetOneString("filename", "");
            if (fn.empty()) return;
            if (fn[0] != '/') fn = scene.baseDir + "/" + fn;
            if (prefetch.uses[fn]++ == 0) files.push_back(fn);
        };
        for (const ShapeEntity &sh : scene.shapes) want(sh);
        std::set<std::string> seenDefs;
        std::vector<InstanceUse> allUsesPrefetch(scene.animatedShapes);
        allUsesPrefetch.insert(allUsesPrefetch.end(), scene.instances.begin(), scene.instances.end());
        for (const InstanceUse &u : allUsesPrefetch) {
            auto it = scene.instanceDefinitions.find(u.name);
            if (it == scene.instanceDefinitions.end() || !seenDefs.insert(u.name).second) continue;
            for (const ShapeEntity &sh : it->second.shapes) want(sh);
            for (const InstanceUse &nu : it->second.animatedShapes) {
                auto nit = scene.instanceDefinitions.find(nu.name);
                if (nit != scene.instanceDefinitions.end()) for (const ShapeEntity &sh : nit->second.shapes) want(sh);
            }
        }
        if (files.size() < 8) return;
        std::vector<MeshSource> loaded(files.size());
        std::vector<char> ok(files.size(), 0);
        ParallelFor(files.size(), [&](size_t i) {
            std::string err;
            try { ok[i] = ReadPLY(files[i], &loaded[i], &err) ? 1 : 0; } catch (...) { ok[i] = 0; }
        });
        for (size_t i = 0; i < files.size(); ++i)
            if (ok[i]) prefetch.meshes.emplace(files[i], std::move(loaded[i]));
        g_plyPrefetch = &prefetch;   // (until this SceneBuild goes)
    }

    // instance definitions (scene.cpp:1522-1557): the shapes stay in the definition's own render space, each definition
    // gets its own BVH; only definitions that are used are built
    void CreateDefinitions() {
        // the animated shapes' hidden definitions first, then the object instances: the order of the reference's top-level primitives
        // (shapes, animated shapes, instances: scene.cpp:1441-1577)
        allUses = scene.animatedShapes;
        allUses.insert(allUses.end(), scene.instances.begin(), scene.instances.end());
        for (const InstanceUse &u : allUses) {
            auto it = scene.instanceDefinitions.find(u.name);
            if (it == scene.instanceDefinitions.end()) Die("", u.name + ": object instance not defined");
            if (defIndex.count(u.name)) continue;
            const int di = (int)defPrims.size();
            defIndex[u.name] = di;
            defPrims.emplace_back();
            defNested.emplace_back();
            for (const ShapeEntity &sh : it->second.shapes) {
                if (sh.lightIndex >= 0) fprintf(stderr, "Warning: %s: Area lights not supported with object instancing\n", sh.loc.c_str());
                AddShape(sh, &defPrims.back(), true);
            }
            // the definition's animated shape entities (scene.cpp:1535-1539), after its static shapes: each a hidden definition of its own, placed
            // inside this one once the bounds are known (below, with the instances)
            for (const InstanceUse &nu : it->second.animatedShapes) {
                const int hi = (int)defPrims.size();
                defIndex[nu.name] = hi;
                defPrims.emplace_back();
                defNested.emplace_back();
                for (const ShapeEntity &sh : scene.instanceDefinitions.at(nu.name).shapes) AddShape(sh, &defPrims[hi], true);
                NestedPlacement np;
                np.use = &nu;
                np.record.def = hi;
                defNested[di].push_back(np);
            }
        }
    }

    void AddPlaceholderIfEmpty() {
        if (!T->triIndices.empty() || !spheres.empty()) return;
        // A scene without geometry renders (the reference's aggregate is then empty: every ray escapes, scene.cpp:1590-1600,
        // wavefront/aggregate.cpp:24-32).  The tables keep one primitive that no ray can hit — a triangle whose three vertices are the
        // render-space origin: IntersectTriangle's first test rejects a zero-area triangle (shapes.cpp:172-173), and the scene bounds it
        // gives Light::Preprocess (centre 0, radius 0) are those of the reference's empty Bounds3f.
        if (scene.materials.empty()) Die("", "scene has no geometry");
        ShapeEntity ph;
        ph.name = "trianglemesh";
        ph.loc = "(placeholder of a scene without geometry)";
        Param idx; idx.type = "integer"; idx.name = "indices"; idx.ints = {0, 1, 2};
        Param pos; pos.type = "point3"; pos.name = "P"; pos.floats.assign(9, 0.f);
        ph.params.params = {idx, pos};
        ph.materialIndex = 0;
        AddShape(ph, &topPrims, false);
        if (T->triIndices.empty()) Die("", "scene has no geometry");
    }

    // quadrics, patches and curve segments: their primitive ids follow the triangles'
    void AssignQuadricIds() {
        const int nTris = (int)T->triIndices.size() / 3;
        for (size_t i = 0; i < spheres.size(); ++i) {
            wf_mesh &qm = T->meshes[spheres[i].s.mesh];
            if (spheres[i].s.type != WF_QUADRIC_BILINEAR && spheres[i].s.type != WF_QUADRIC_CURVE) qm.first_tri = nTris + (int)i;
            else if (qm.ntris == 0 && qm.first_tri < 0) qm.first_tri = nTris + (int)i;  // a patch or curve mesh: its first primitive
            T->triMesh.push_back(spheres[i].s.mesh);
            T->quadrics.push_back(spheres[i].s);
        }
        for (auto &pr : topPrims) if (pr.first < 0) pr.first = nTris + (-1 - pr.first);
        for (PrimList &dl : defPrims)
            for (auto &pr : dl) if (pr.first < 0) pr.first = nTris + (-1 - pr.first);
    }

    // ---- lights: area lights first (scene.cpp:1290-1340), then the others ----
    // An RGB image as a light's emission (DiffuseAreaLight::Create with "filename", lights.cpp:884-910; ProjectionLight::Create, :448-518):
    // read, checked, appended as a one-level image; .pfm carries no colour space, so it is sRGB's RGB -> spectrum table the device needs
    LightImage AddLightImage(const std::string &filename, const std::string &loc, const std::string &channelsError, int filter) {
        LightImage img;
        int fileNc = 0;
        ReadLightImage(filename, loc, &img.rgb, &img.w, &img.h, &fileNc);
        if (fileNc < 3) Die(loc, channelsError);
        for (float v : img.rgb) if (!std::isfinite(v)) Die(loc, filename + ": image has infinite or not-a-number pixel values and so is not suitable as a light.");
        wf_tex_image im{};
        im.res[0] = img.w; im.res[1] = img.h; im.n_levels = 1; im.n_channels = 3; im.wrap = WF_WRAP_CLAMP; im.filter = filter;
        im.level_offset[0] = (int)T->tableData.size();
        T->tableData.insert(T->tableData.end(), img.rgb.begin(), img.rgb.end());
        img.id = (int)T->texImages.size();
        T->texImages.push_back(im);
        UseSRGBTable();
        return img;
    }

    // the device-side RGB -> spectrum table of a light image's colour space (the caller sets desc.cs_illuminant_offset)
    void UseSRGBTable() {
        const ColorSpace *ics = SpectralData::Get().sRGB();
        T->desc.rgb2spec_coeffs = ics->table->coeffs.data();
        for (int i = 0; i < 64; ++i) T->desc.rgb2spec_znodes[i] = ics->table->zNodes[i];
    }

    // One DiffuseAreaLight (lights.cpp:873-941) and its Bounds() (lights.cpp:788-806) for the primitive `prim` of a shape: its area, its box and
    // its shape's NormalBounds() (the cone's axis w as the LightBounds constructor leaves it, and cosTheta_o)
    void AddAreaLight(const AreaLightParams &a, int prim, float area, const B3 &box, V3 w, float cosTheta_o) {
        float sc = a.scale;
        if (a.power > 0) {
            float k_e = a.image >= 0 ? a.imageLumAvg : 1.f;
            k_e *= (a.twoSided ? 2 : 1) * area * Pi;
            sc *= a.power / k_e;
        }
        wf_light l{};
        l.type = WF_LIGHT_DIFFUSE_AREA;
        l.flags = (a.twoSided ? WF_LIGHTFLAG_TWOSIDED : 0) | (a.alphaZero ? WF_LIGHTFLAG_DELTA_POSITION : 0);
        l.alpha_tex_plus1 = a.alphaZero ? 0 : a.alphaTex + 1;
        l.spectrum_offset = a.spectrumOffset;
        l.scale = sc;
        l.tri = prim;
        l.area = area;
        l.bit_trail = -1; l.infinite_index = -1; l.xform = -1; l.image = a.image;
        int lightId = (int)T->lights.size();
        T->lights.push_back(l);
        LightBoundsH lb;
        lb.bounds = box;
        lb.w = w;
        lb.phi = a.LemitMax * (sc * area * Pi);
        lb.cosTheta_o = cosTheta_o;
        lb.cosTheta_e = std::cos(Pi / 2);
        lb.twoSided = a.twoSided;
        AddLightBounds(lightId, lb);
    }

    void AddAreaLights() {
        for (const PendingAreaLight &pa : pendingArea) {
            const Entity &al = scene.areaLights[pa.lightEntity];
            if (al.name != "diffuse") Die(al.loc, al.name + ": area light type unknown.");
            const ParamSet &ps = al.params;
            const ColorSpace *cs = ps.colorSpace;
            // DiffuseAreaLight::Create (lights.cpp:873-941)
            SpectrumP L = ps.GetOneSpectrum("L", nullptr, SpectrumType::Illuminant);
            float scale = ps.GetOneFloat("scale", 1);
            bool twoSided = ps.GetOneBool("twosided", false);
            // DiffuseAreaLight::Create with "filename" (lights.cpp:884-910): an RGB image in the (u, v) square; .pfm -> sRGB
            int lightImage = -1;
            float imageLumAvg = 1, imageChannelAvg = 0;
            std::string filename = ps.GetOneString("filename", "");
            if (!filename.empty()) {
                if (L) Die(al.loc, "Both \"L\" and \"filename\" specified for DiffuseAreaLight.");
                if (filename[0] != '/') filename = scene.baseDir + "/" + filename;
                const LightImage img = AddLightImage(filename, al.loc, filename + ": Image provided to \"diffuse\" area light must have R, G, and B channels.", WF_MIP_BILINEAR);
                const std::vector<float> &rgb = img.rgb;
                const int w = img.w, h = img.h;
                const ColorSpace *ics = SpectralData::Get().sRGB();
                lightImage = img.id;
                float k_e = 0, sum = 0;
                for (size_t i = 0; i < (size_t)w * h; ++i)
                    for (int c = 0; c < 3; ++c) { k_e += rgb[3 * i + c] * ics->XYZFromRGB.m[1][c]; sum += rgb[3 * i + c]; }
                imageLumAvg = k_e / (w * h);           // lights.cpp:917-925
                imageChannelAvg = sum / (3 * w * h);   // DiffuseAreaLight::Bounds, lights.cpp:792-799
                L = ics->illuminant;
            }
            if (!L) L = cs->illuminant;
            scale /= SpectrumToPhotometric(*L);
            float phi_v = ps.GetOneFloat("power", -1.0f);
            wf_mesh &mesh = T->meshes[pa.mesh];
            mesh.first_light = (int)T->lights.size();
            // a constant-zero alpha makes the emitter a DeltaPosition light without an alpha texture (lights.cpp:690-709)
            const bool alphaZero = mesh.alpha_tex >= 0 && T->textures[mesh.alpha_tex].type == WF_TEX_FLOAT_CONSTANT && T->textures[mesh.alpha_tex].f0 == 0;
            int specOff = T->pool.AddDense(*L);
            float LemitMax = lightImage >= 0 ? imageChannelAvg : MakeDense(*L)->MaxValue();  // Bounds(): image average or Lemit max
            if (lightImage >= 0) T->desc.cs_illuminant_offset = specOff;
            const AreaLightParams a{twoSided, alphaZero, mesh.alpha_tex, specOff, lightImage, scale, phi_v, imageLumAvg, LemitMax};
            const V3 up = Normalize(V3{0, 0, 1});   // DirectionCone::EntireSphere(): this axis, cosTheta -1
            const int nTris = (int)T->triIndices.size() / 3;
            if (auto sit = sphereOfMesh.find(pa.mesh); sit != sphereOfMesh.end()) {
                // Sphere / Disk / Cylinder::Area (shapes.h:292,407,559); Sphere / Cylinder::NormalBounds = DirectionCone::EntireSphere()
                const PendingSphere &sp = spheres[sit->second];
                V3 w = up;
                float cosTheta_o = -1.f;
                if (sp.s.type == WF_QUADRIC_DISK) {
                    // Disk::NormalBounds (shapes.cpp:89-94): DirectionCone(Vector3f(n)) normalizes, the LightBounds ctor again
                    N3 n = pa.renderFromObject.Normal(N3{0, 0, 1});
                    if (T->meshes[sp.s.mesh].flags & WF_MESH_REVERSE_ORIENTATION) n = -n;
                    w = Normalize(Normalize(toV(n)));
                    cosTheta_o = 1.f;
                }
                AddAreaLight(a, mesh.first_tri, QuadricArea(sp.s), sp.bounds, w, cosTheta_o);
            }
            for (int t = 0; t < mesh.ntris; ++t) {
                // Triangle::Area (shapes.h:852-858), Triangle::NormalBounds (shapes.cpp:292-307)
                const int tri = mesh.first_tri + t;
                const int32_t *v = &T->triIndices[3 * (size_t)tri];
                auto P = [&](int i) { return V3{T->P[3 * (size_t)i], T->P[3 * (size_t)i + 1], T->P[3 * (size_t)i + 2]}; };
                const V3 p0 = P(v[0]), p1 = P(v[1]), p2 = P(v[2]);
                N3 n = Normalize(toN(Cross(p1 - p0, p2 - p0)));
                if (mesh.flags & WF_MESH_HAS_N) {
                    auto NN = [&](int i) { return N3{T->N[3 * (size_t)i], T->N[3 * (size_t)i + 1], T->N[3 * (size_t)i + 2]}; };
                    N3 ns = NN(v[0]) + NN(v[1]) + NN(v[2]);
                    n = FaceForward(n, ns);
                } else if (mesh.flags & WF_MESH_FLIP_NORMAL) n = n * -1.f;
                B3 b;
                b.pMin = {fmin(p0.x, p1.x), fmin(p0.y, p1.y), fmin(p0.z, p1.z)};
                b.pMax = {fmax(p0.x, p1.x), fmax(p0.y, p1.y), fmax(p0.z, p1.z)};
                // DirectionCone(Vector3f(n)) normalizes (cosTheta 1); the LightBounds ctor normalizes again
                AddAreaLight(a, tri, 0.5f * Length(Cross(p1 - p0, p2 - p0)), Union(b, p2), Normalize(Normalize(toV(n))), 1.f);
            }
            if (auto pit = patchesOfMesh.find(pa.mesh); pit != patchesOfMesh.end()) {
                // one DiffuseAreaLight per bilinear patch (scene.cpp:1290-1340), in patch order; hits find theirs as
                // first_light + (primitive id - first_tri)
                for (int si : pit->second) {
                    const PendingSphere &sp = spheres[si];
                    V3 w;
                    float cosTheta;
                    PatchNormalBounds(LoadBlp(sp.s), (mesh.flags & WF_MESH_FLIP_NORMAL) != 0, &w, &cosTheta);
                    AddAreaLight(a, nTris + si, sp.s.radius, sp.bounds, Normalize(w), cosTheta);   // (the LightBounds ctor normalises again)
                }
            }
            if (auto cit = curvesOfMesh.find(pa.mesh); cit != curvesOfMesh.end()) {
                // An emissive curve: the reference creates one DiffuseAreaLight per Curve primitive like for any shape (scene.cpp:1290-1340) —
                // area from Curve::Area, bounds from Curve::Bounds, NormalBounds = the entire sphere (shapes.h:1251) —, lets camera and specular
                // rays see its emission, and aborts the moment a sample is drawn from it or its PDF is asked for (Curve::Sample / Curve::PDF:
                // LOG_FATAL "not implemented", shapes.cpp:736-760).  Same here: SphereSample / SpherePDF raise the context's fatal flag.
                for (int si : cit->second) AddAreaLight(a, nTris + si, spheres[si].area, spheres[si].bounds, up, -1.f);
            }
            ps.ReportUnused("AreaLightSource");
        }
    }

    void AddLights() {
        for (const LightEntity &le : scene.lights) {
            wf_light l{};
            l.bit_trail = -1; l.infinite_index = -1; l.xform = -1; l.image = -1; l.tri = -1;
            if (le.name == "point") AddPointLight(le, l);
            else if (le.name == "spot") AddSpotLight(le, l);
            else if (le.name == "projection") AddProjectionLight(le, l);
            else if (le.name == "goniometric") AddGoniometricLight(le, l);
            else if (le.name == "distant") AddDistantLight(le, l);
            else if (le.name == "infinite") AddInfiniteLight(le, l);
            else Die(le.loc, le.name + ": light type not supported by this build (point, spot, projection, goniometric, distant, infinite)");
            le.params.ReportUnused("LightSource");
        }
        if (T->lights.empty()) Die("", "No light sources specified");
    }

    void AddPointLight(const LightEntity &le, wf_light l) {
        const ParamSet &ps = le.params;
        const ColorSpace *cs = ps.colorSpace;
        SpectrumP I = ps.GetOneSpectrum("I", cs->illuminant, SpectrumType::Illuminant);
        float sc = ps.GetOneFloat("scale", 1);
        sc /= SpectrumToPhotometric(*I);
        float phi_v = ps.GetOneFloat("power", -1);
        if (phi_v > 0) { float k_e = 4 * Pi; sc *= phi_v / k_e; }
        V3 from = ps.GetOnePoint3f("from", V3{0, 0, 0});
        Transform tf = Translate(from);
        Transform rfl = le.renderFromLight * tf;
        V3 p = rfl.Point(V3{0, 0, 0});
        l.type = WF_LIGHT_POINT; l.scale = sc; l.spectrum_offset = T->pool.AddDense(*I);
        l.pos[0] = p.x; l.pos[1] = p.y; l.pos[2] = p.z;
        AddLightAt(l, p, Normalize(V3{0, 0, 1}), 4 * Pi * sc * MakeDense(*I)->MaxValue(), std::cos(Pi), std::cos(Pi / 2));
    }

    void AddSpotLight(const LightEntity &le, wf_light l) {
        const ParamSet &ps = le.params;
        const ColorSpace *cs = ps.colorSpace;
        SpectrumP I = ps.GetOneSpectrum("I", cs->illuminant, SpectrumType::Illuminant);
        float sc = ps.GetOneFloat("scale", 1);
        float coneangle = ps.GetOneFloat("coneangle", 30.f);
        float conedelta = ps.GetOneFloat("conedeltaangle", 5.f);
        V3 from = ps.GetOnePoint3f("from", V3{0, 0, 0});
        V3 to = ps.GetOnePoint3f("to", V3{0, 0, 1});
        Frame fr = Frame::FromZ(Normalize(to - from));
        Transform dirToZ(M4(fr.x.x, fr.x.y, fr.x.z, 0, fr.y.x, fr.y.y, fr.y.z, 0, fr.z.x, fr.z.y, fr.z.z, 0, 0, 0, 0, 1));
        Transform t = Translate(from) * Inverse(dirToZ);
        Transform rfl = le.renderFromLight * t;
        sc /= SpectrumToPhotometric(*I);
        float phi_v = ps.GetOneFloat("power", -1);
        if (phi_v > 0) {
            float cosFalloffEnd = std::cos(Radians(coneangle));
            float cosFalloffStart = std::cos(Radians(coneangle - conedelta));
            float k_e = 2 * Pi * ((1 - cosFalloffStart) + (cosFalloffStart - cosFalloffEnd) / 2);
            sc *= phi_v / k_e;
        }
        l.type = WF_LIGHT_SPOT; l.scale = sc; l.spectrum_offset = T->pool.AddDense(*I);
        l.cosFalloffEnd = std::cos(Radians(coneangle));
        l.cosFalloffStart = std::cos(Radians(coneangle - conedelta));
        V3 p = rfl.Point(V3{0, 0, 0});
        l.pos[0] = p.x; l.pos[1] = p.y; l.pos[2] = p.z;
        l.xform = (int)T->lightTransforms.size();
        T->lightTransforms.push_back(rfl.abi());
        float cosTheta_e = std::cos(std::acos(l.cosFalloffEnd) - std::acos(l.cosFalloffStart));
        if (cosTheta_e == 1 && l.cosFalloffEnd != l.cosFalloffStart) cosTheta_e = 0.999f;
        AddLightAt(l, p, Normalize(Normalize(rfl.Vector(V3{0, 0, 1}))), sc * MakeDense(*I)->MaxValue() * 4 * Pi, l.cosFalloffStart, cosTheta_e);
    }

    // ProjectionLight::Create + ctor + Bounds (lights.cpp:448-518, 287-321, 384-399); .pfm only in this build
    void AddProjectionLight(const LightEntity &le, wf_light l) {
        const ParamSet &ps = le.params;
        float sc = ps.GetOneFloat("scale", 1);
        float power = ps.GetOneFloat("power", -1);
        float fov = ps.GetOneFloat("fov", 90.f);
        std::string filename = ps.GetOneString("filename", "");
        if (filename.empty()) Die(le.loc, "Must provide \"filename\" to \"projection\" light source");
        if (filename[0] != '/') filename = scene.baseDir + "/" + filename;
        const LightImage img = AddLightImage(filename, le.loc, "Image provided to \"projection\" light must have R, G, and B channels.", WF_MIP_POINT);
        const std::vector<float> &rgb = img.rgb;
        const int w = img.w, h = img.h;
        const ColorSpace *ics = SpectralData::Get().sRGB();
        l.image = img.id;
        sc /= SpectrumToPhotometric(*ics->illuminant);
        const float hither = 1e-3f;
        float aspect = float(w) / float(h);
        float sb[4];
        if (aspect > 1) { sb[0] = -aspect; sb[1] = -1; sb[2] = aspect; sb[3] = 1; }
        else { sb[0] = -1; sb[1] = -1 / aspect; sb[2] = 1; sb[3] = 1 / aspect; }
        Transform screenFromLight = Perspective(fov, hither, 1e30f);
        Transform lightFromScreen = Inverse(screenFromLight);
        float opposite = std::tan(Radians(fov) / 2);
        float A = 4 * Sqr(opposite) * (aspect > 1 ? aspect : (1 / aspect));
        auto screenLerp = [&](float tx, float ty) { return V2{(1 - tx) * sb[0] + tx * sb[2], (1 - ty) * sb[1] + ty * sb[3]}; };
        if (power > 0) {
            float sum = 0;
            float lum[3];
            for (int c = 0; c < 3; ++c) lum[c] = ics->XYZFromRGB.m[1][c];  // RGBColorSpace::LuminanceVector
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    V2 p2 = screenLerp((x + .5f) / w, (y + .5f) / h);
                    V3 wv = Normalize(lightFromScreen.Point(V3{p2.x, p2.y, 0}));
                    float dwdA = wv.z * wv.z * wv.z;
                    for (int c = 0; c < 3; ++c) sum += rgb[3 * ((size_t)y * w + x) + c] * lum[c] * dwdA;
                }
            sc *= power / (A * sum / (w * h));
        }
        Transform rfl = le.renderFromLight * Scale(1, -1, 1);
        l.type = WF_LIGHT_PROJECTION; l.scale = sc; l.spectrum_offset = T->pool.AddDense(*ics->illuminant);
        l.area = A;
        for (int k = 0; k < 4; ++k) l.screen_bounds[k] = sb[k];
        T->desc.cs_illuminant_offset = l.spectrum_offset;
        V3 p = rfl.Point(V3{0, 0, 0});
        l.pos[0] = p.x; l.pos[1] = p.y; l.pos[2] = p.z;
        l.xform = (int)T->lightTransforms.size();
        T->lightTransforms.push_back(rfl.abi());
        l.xform2 = (int)T->lightTransforms.size();
        T->lightTransforms.push_back(screenFromLight.abi());
        float sumMax = 0;
        for (size_t i = 0; i < (size_t)w * h; ++i) sumMax += std::max(std::max(rgb[3 * i], rgb[3 * i + 1]), rgb[3 * i + 2]);
        V3 wCorner = Normalize(lightFromScreen.Point(V3{sb[2], sb[3], 0}));
        AddLightAt(l, p, Normalize(Normalize(rfl.Vector(V3{0, 0, 1}))), sc * sumMax / (w * h), std::cos(0.f), wCorner.z);
    }

    // GoniometricLight::Create + ctor + Bounds (lights.cpp:603-682, 521-536, 563-575); .pfm only in this build
    void AddGoniometricLight(const LightEntity &le, wf_light l) {
        const ParamSet &ps = le.params;
        const ColorSpace *cs = ps.colorSpace;
        SpectrumP I = ps.GetOneSpectrum("I", cs->illuminant, SpectrumType::Illuminant);
        float sc = ps.GetOneFloat("scale", 1);
        std::string filename = ps.GetOneString("filename", "");
        if (filename.empty()) Die(le.loc, "goniometric light without a \"filename\" is not supported by this build");
        if (filename[0] != '/') filename = scene.baseDir + "/" + filename;
        std::vector<float> rgb;
        int w = 0, h = 0;
        int fileNc = 0;
        HostImage rawImg;
        ReadLightImage(filename, le.loc, &rgb, &w, &h, &fileNc, &rawImg);
        if (w != h) Die(le.loc, filename + ": image resolution is non-square. It's unlikely this is an equal-area environment map.");
        const bool grey = fileNc == 1;
        wf_tex_image im{};
        im.res[0] = w; im.res[1] = h; im.n_levels = 1; im.n_channels = 1; im.wrap = WF_WRAP_CLAMP; im.filter = WF_MIP_POINT;
        im.level_offset[0] = (int)T->tableData.size();
        float sumY = 0;
        for (size_t i = 0; i < (size_t)w * h; ++i) {
            // R G B files: a "Y" image of the file's own pixel format holds the channel average (lights.cpp:648-657), so an 8-bit or
            // half file's average is re-quantised by SetChannel
            float v = grey ? rgb[3 * i] : rawImg.Quantize((0.f + rgb[3 * i] + rgb[3 * i + 1] + rgb[3 * i + 2]) / 3);
            if (!std::isfinite(v)) Die(le.loc, filename + ": image has infinite or not-a-number pixel values and so is not suitable as a light.");
            T->tableData.push_back(v);
            sumY += v;
        }
        l.image = (int)T->texImages.size();
        T->texImages.push_back(im);
        sc /= SpectrumToPhotometric(*I);
        float phi_v = ps.GetOneFloat("power", -1);
        if (phi_v > 0) {
            float k_e = 4 * Pi * sumY / (w * h);
            sc *= phi_v / k_e;
        }
        Transform swapYZ(M4(1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 1));
        Transform rfl = le.renderFromLight * swapYZ;
        l.type = WF_LIGHT_GONIOMETRIC; l.scale = sc; l.spectrum_offset = T->pool.AddDense(*I);
        l.area = sumY / (w * h);  // mean texel, for Phi (lights.cpp:554-561)
        V3 p = rfl.Point(V3{0, 0, 0});
        l.pos[0] = p.x; l.pos[1] = p.y; l.pos[2] = p.z;
        l.xform = (int)T->lightTransforms.size();
        T->lightTransforms.push_back(rfl.abi());
        AddLightAt(l, p, Normalize(V3{0, 0, 1}), sc * MakeDense(*I)->MaxValue() * 4 * Pi * sumY / (w * h), std::cos(Pi), std::cos(Pi / 2));
    }

    void AddDistantLight(const LightEntity &le, wf_light l) {
        const ParamSet &ps = le.params;
        const ColorSpace *cs = ps.colorSpace;
        SpectrumP L = ps.GetOneSpectrum("L", cs->illuminant, SpectrumType::Illuminant);
        float sc = ps.GetOneFloat("scale", 1);
        V3 from = ps.GetOnePoint3f("from", V3{0, 0, 0});
        V3 to = ps.GetOnePoint3f("to", V3{0, 0, 1});
        V3 w = Normalize(from - to);
        V3 v1, v2;
        CoordinateSystem(w, &v1, &v2);
        Transform t(M4(v1.x, v2.x, w.x, 0, v1.y, v2.y, w.y, 0, v1.z, v2.z, w.z, 0, 0, 0, 0, 1));
        Transform rfl = le.renderFromLight * t;
        sc /= SpectrumToPhotometric(*L);
        float E_v = ps.GetOneFloat("illuminance", -1);
        if (E_v > 0) sc *= E_v;
        l.type = WF_LIGHT_DISTANT; l.scale = sc; l.spectrum_offset = T->pool.AddDense(*L);
        V3 wi = Normalize(rfl.Vector(V3{0, 0, 1}));  // DistantLight::SampleLi (lights.h:262)
        l.pos[0] = wi.x; l.pos[1] = wi.y; l.pos[2] = wi.z;
        AddInfinite(l);
    }

    void AddInfiniteLight(const LightEntity &le, wf_light l) {
        const ParamSet &ps = le.params;
        std::vector<V3> portal = ps.GetPoint3fArray("portal");
        std::string filename = ps.GetOneString("filename", "");
        SpectrumP L = ps.GetOneSpectrum("L", nullptr, SpectrumType::Illuminant);
        float scale = ps.GetOneFloat("scale", 1);
        float E_v = ps.GetOneFloat("illuminance", -1);
        if (!filename.empty() || (L && !portal.empty())) {
            // ImageInfiniteLight (lights.cpp:1567-1672, ctor :1001-1040)
            if (L && !filename.empty()) Die(le.loc, "Can't specify both emission \"L\" and \"filename\" with ImageInfiniteLight");
            LightImage img;
            int fileNc = 0;
            if (filename.empty()) {
                // "L" with a portal (lights.cpp:1569-1590): a 1 x 1 image holding L converted to sRGB
                float xyz[3], c[3];
                SpectrumToXYZ(*L, xyz);
                Mul3(SpectralData::Get().sRGB()->RGBFromXYZ, xyz, c);   // RGBColorSpace::ToRGB
                img.rgb = {c[0], c[1], c[2]};
                img.w = img.h = 1; fileNc = 3;
            } else {
                if (filename[0] != '/') filename = scene.baseDir + "/" + filename;
                ReadLightImage(filename, le.loc, &img.rgb, &img.w, &img.h, &fileNc);
            }
            if (fileNc < 3) Die(le.loc, filename + ": image used for ImageInfiniteLight doesn't have R, G, B channels.");
            for (float v : img.rgb) {
                if (std::isinf(v)) Die(le.loc, filename + ": image has infinite pixel values and so is not suitable as a light.");
                if (std::isnan(v)) Die(le.loc, filename + ": image has not-a-number pixel values and so is not suitable as a light.");
            }
            if (img.w != img.h) Die(le.loc, filename + ": image resolution is non-square. It's unlikely this is an equal area environment map.");
            const std::vector<float> &rgb = img.rgb;
            const int w = img.w, h = img.h;
            const ColorSpace *ics = SpectralData::Get().sRGB();  // PFM carries no colour space: ImageMetadata::GetColorSpace() -> sRGB
            scale /= SpectrumToPhotometric(*ics->illuminant);
            if (E_v > 0) {
                // upper-hemisphere illuminance of the map (lights.cpp:1620-1648)
                float illuminance = 0;
                float lum[3];
                for (int c = 0; c < 3; ++c) lum[c] = ics->XYZFromRGB.m[1][c];  // RGBColorSpace::LuminanceVector
                for (int y = 0; y < h; ++y) {
                    float v = (float(y) + 0.5f) / float(h);
                    for (int x = 0; x < w; ++x) {
                        float u = (x + 0.5f) / w;
                        V3 wv = EqualAreaSquareToSphere(V2{u, v});
                        if (wv.z <= 0) continue;
                        const float *px = &rgb[3 * ((size_t)y * w + x)];
                        for (int c = 0; c < 3; ++c) illuminance += px[c] * lum[c] * wv.z;  // ... * CosTheta(w)
                    }
                }
                illuminance *= 2 * Pi / (w * h);
                scale *= E_v / illuminance;
            }
            if (!portal.empty()) AddPortalLight(le, l, img, scale, portal);
            else AddImageInfiniteLight(le, l, img, scale);
            return;
        }
        const ColorSpace *cs = ps.colorSpace;
        if (!L) L = cs->illuminant;
        scale /= SpectrumToPhotometric(*L);
        if (E_v > 0) { float k_e = Pi; scale *= E_v / k_e; }
        l.type = WF_LIGHT_UNIFORM_INFINITE; l.scale = scale; l.spectrum_offset = T->pool.AddDense(*L);
        AddInfinite(l);
    }

    // the rest of ImageInfiniteLight (ctor, lights.cpp:1001-1040): the image, its sampling distribution and the compensated one
    void AddImageInfiniteLight(const LightEntity &le, wf_light l, const LightImage &img, float scale) {
        const std::vector<float> &rgb = img.rgb;
        const int w = img.w, h = img.h;
        const ColorSpace *ics = SpectralData::Get().sRGB();
        wf_image_light im{};
        im.res = w;
        im.pixel_offset = (int)T->tableData.size();
        T->tableData.insert(T->tableData.end(), rgb.begin(), rgb.end());
        // Image::GetSamplingDistribution (util/image.h:449-470): channel average per pixel
        std::vector<float> d((size_t)w * h);
        for (size_t i = 0; i < d.size(); ++i) {
            float sum = 0;
            for (int c = 0; c < 3; ++c) sum += rgb[3 * i + c];
            d[i] = sum / 3;
        }
        im.distribution = AppendPC2D(&T->tableData, d, w, h);
        // compensated distribution (lights.cpp:1031-1039)
        double acc = 0.;
        for (float v : d) acc += v;
        float average = (float)(acc / d.size());
        bool allZero = true;
        for (float &v : d) { v = std::max(v - average, 0.f); if (v != 0) allZero = false; }
        if (allZero) std::fill(d.begin(), d.end(), 1.f);
        im.compensated = AppendPC2D(&T->tableData, d, w, h);
        l.type = WF_LIGHT_IMAGE_INFINITE; l.scale = scale; l.spectrum_offset = T->pool.AddDense(*ics->illuminant);
        l.image = (int)T->imageLights.size();
        T->imageLights.push_back(im);
        l.xform = (int)T->lightTransforms.size();
        T->lightTransforms.push_back(le.renderFromLight.abi());
        AddInfinite(l);
        UseSRGBTable();
        T->desc.cs_illuminant_offset = l.spectrum_offset;
    }

    // PortalImageInfiniteLight ctor (lights.cpp:1109-1181): the portal in render space, its frame, the environment map
    // resampled into the portal's (alpha, beta) parametrisation, the sampling function and its summed-area table
    void AddPortalLight(const LightEntity &le, wf_light l, const LightImage &img, float scale, const std::vector<V3> &portal) {
        const std::vector<float> &rgb = img.rgb;
        const int w = img.w, h = img.h;
        const ColorSpace *ics = SpectralData::Get().sRGB();
        if (portal.size() != 4) Die(le.loc, "Expected 4 vertices for infinite light portal but given " + std::to_string(portal.size()));
        wf_image_light im{};
        im.is_portal = 1;
        im.res = w;
        V3 P[4];
        for (int i = 0; i < 4; ++i) {
            // cameraTransform.RenderFromWorld(p) = worldFromRender.ApplyInverse(p) (cameras.h:42): the portal is given in world space.
            // (ApplyInverse sums in pairs: with a rotation in worldFromRender — rendercoordsys camera — the left-to-right sum of
            //  operator() lands a last bit away: fuzz finding s1800141, round 5)
            P[i] = Inverse(scene.renderFromWorld).ApplyInversePoint(portal[i]);
            im.portal[i][0] = P[i].x; im.portal[i][1] = P[i].y; im.portal[i][2] = P[i].z;
        }
        V3 p01 = Normalize(P[1] - P[0]), p12 = Normalize(P[2] - P[1]), p32 = Normalize(P[2] - P[3]), p03 = Normalize(P[3] - P[0]);
        if (std::abs(Dot(p01, p32) - 1) > .001 || std::abs(Dot(p12, p03) - 1) > .001 || std::abs(Dot(p01, p12)) > .001 ||
            std::abs(Dot(p12, p32)) > .001 || std::abs(Dot(p32, p03)) > .001 || std::abs(Dot(p03, p01)) > .001)
            fprintf(stderr, "Error: %s: Infinite light portal isn't a planar quadrilateral\n", le.loc.c_str());
        V3 fz = Cross(p03, p01);   // Frame::FromXY(p03, p01)
        for (int k = 0; k < 3; ++k) { im.portal_frame[0][k] = p03[k]; im.portal_frame[1][k] = p01[k]; im.portal_frame[2][k] = fz[k]; }
        wf_tex_image src{};
        src.res[0] = w; src.res[1] = h; src.n_levels = 1; src.n_channels = 3; src.wrap = WF_WRAP_OCTAHEDRAL; src.filter = WF_MIP_BILINEAR;
        std::vector<float> rect((size_t)3 * w * h), dfun((size_t)w * h);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                V2 uv{(x + 0.5f) / w, (y + 0.5f) / h};
                float duv_dw;
                V3 wr = PortalRenderFromImage(im, uv, &duv_dw);
                V3 wl = Normalize(XfVector3(le.renderFromLight.mInv.m, wr));   // renderFromLight.ApplyInverse(w)
                V2 uvEqui = EqualAreaSphereToSquare(wl);
                float sum = 0;
                for (int c = 0; c < 3; ++c) {
                    float v = ImageBilerpChannel(rgb.data(), src, 0, uvEqui, c);
                    rect[3 * ((size_t)y * w + x) + c] = v;
                    sum += v;
                }
                dfun[(size_t)y * w + x] = (sum / 3) * duv_dw;   // GetSamplingDistribution: channel average x Jacobian at the pixel centre
            }
        // SummedAreaTable (util/sampling.h:834-848), double sums of the float function
        std::vector<double> sat((size_t)w * h);
        auto S = [&](int x, int y) -> double & { return sat[(size_t)y * w + x]; };
        auto F = [&](int x, int y) { return dfun[(size_t)y * w + x]; };
        S(0, 0) = F(0, 0);
        for (int x = 1; x < w; ++x) S(x, 0) = F(x, 0) + S(x - 1, 0);
        for (int y = 1; y < h; ++y) S(0, y) = F(0, y) + S(0, y - 1);
        for (int y = 1; y < h; ++y)
            for (int x = 1; x < w; ++x) S(x, y) = (F(x, y) + S(x - 1, y) + S(x, y - 1) - S(x - 1, y - 1));
        im.pixel_offset = (int)T->tableData.size();
        T->tableData.insert(T->tableData.end(), rect.begin(), rect.end());
        im.func_offset = (int)T->tableData.size();
        T->tableData.insert(T->tableData.end(), dfun.begin(), dfun.end());
        if (T->tableData.size() & 1) T->tableData.push_back(0.f);   // doubles: 8-byte aligned
        im.sat_offset = (int)T->tableData.size();
        T->tableData.resize(T->tableData.size() + 2 * sat.size());
        std::memcpy(&T->tableData[im.sat_offset], sat.data(), sat.size() * sizeof(double));
        l.type = WF_LIGHT_PORTAL_INFINITE; l.scale = scale; l.spectrum_offset = T->pool.AddDense(*ics->illuminant);
        l.image = (int)T->imageLights.size();
        T->imageLights.push_back(im);
        l.xform = -1;
        AddInfinite(l);
        UseSRGBTable();
        T->desc.cs_illuminant_offset = l.spectrum_offset;
    }

    // ---- acceleration structure (scene.cpp:1575-1591, cpu/aggregates.cpp:725-744) ----
    // CreateAccelerator (cpu/aggregates.cpp:1163-1178): "bvh" | "kdtree", anything else is an error.  A kd-tree finds the same closest hit and
    // the same occlusion as the BVH (exact ties between coplanar primitives aside): it is replaced by the BVH, as the reference's own GPU path
    // replaces every accelerator by its own
    AccelParams ParseAccelerator() const {
        if (scene.accelerator.name == "kdtree") {
            fprintf(stderr, "Warning: accelerator \"kdtree\" is replaced by the BVH\n");
            // KdTreeAggregate::Create's parameters (cpu/aggregates.cpp:1151-1160) count as looked up
            for (const char *k : {"intersectcost", "traversalcost", "maxprims", "maxdepth"}) scene.accelerator.params.GetOneInt(k, 0);
            scene.accelerator.params.GetOneFloat("emptybonus", 0.5f);
        }
        else if (scene.accelerator.name != "bvh") Die(scene.accelerator.loc, scene.accelerator.name + ": accelerator type unknown.");
        std::string split = scene.accelerator.params.GetOneString("splitmethod", "sah");
        if (getenv("WF_BVH_SPLIT")) split = getenv("WF_BVH_SPLIT");   // load-time experiments: build the top-level tree with the other method
        if (split != "sah" && split != "hlbvh" && split != "middle" && split != "equal") {
            fprintf(stderr, "Warning: BVH split method \"%s\" unknown.  Using \"sah\".\n", split.c_str());   // cpu/aggregates.cpp:737-740
            split = "sah";
        }
        AccelParams a;
        a.splitCode = split == "hlbvh" ? 1 : split == "middle" ? 2 : split == "equal" ? 3 : 0;
        a.maxPrims = scene.accelerator.params.GetOneInt("maxnodeprims", 4);
        scene.accelerator.params.ReportUnused("Accelerator");   // CreateAccelerator, cpu/aggregates.cpp:1176
        return a;
    }

    // checks every primitive list and bounds every definition (= the union of its primitives' bounds, what the root of BVHAggregate(prims) holds)
    void BoundDefinitions() {
        RequireFinite(topPrims, "scene");
        for (const PrimList &prims : defPrims) RequireFinite(prims, "object instance definition");
        defBounds.resize(defPrims.size());
        ParallelFor(defPrims.size(), [this](size_t d) {
            B3 b;   // (in creation order, as the builder's root does: the first of two signed zeros stays)
            for (const auto &p : defPrims[d]) b = Union(b, p.second);
            defBounds[d] = b;
        });
    }

    // AnimatedPrimitive around the aggregate with the bounds `db` (a top-level animated shape, an animated use of a definition, an animated
    // shape inside a definition): records its AnimatedTransform, returns its Bounds()
    B3 AnimatedPlacement(const InstanceUse &u, const B3 &db, wf_instance *in) {
        const float b[6] = {db.pMin.x, db.pMin.y, db.pMin.z, db.pMax.x, db.pMax.y, db.pMax.z};
        B3 wb;
        // AnimatedPrimitive (cpu/primitive.cpp:132-153): Bounds() = renderFromPrimitive.MotionBounds(primitive.Bounds())
        // (util/transform.cpp:1083-1096).  Without rotation that is the union of the start and end boxes — restated exactly.  WITH
        // rotation the reference bounds every corner's path through the zeros of the motion derivative (its c1..c5 terms: 530
        // lines of generated coefficient code, not restated): here the path of every corner is sampled at 1025 times and the box
        // widened by the largest step between neighbouring samples, which contains the path.  A top-level box only decides which
        // nodes a ray visits, not what it hits; the tree built over this box can differ from the reference's, which matters for
        // the ORDER of candidates at exactly coincident geometry only (stated in DESIGN.md 2).
        if (!IsAffine(u.renderFromInstanceEnd)) Die(u.loc, "only affine animated transformations are supported");
        // (every material: the consumers of a hit interpolate the transformation at the ray's time — the walks, the transmittance trace,
        // the interface skip and MixMaterial resolve of the routing, the material stage: wf_shapes.h InstanceAt<ANIM>; the subsurface
        // probes at time 0, as the reference's)
        const wf_animated_transform A = MakeAnimatedTransform(u.renderFromInstance, u.startTime, u.renderFromInstanceEnd, u.endTime);
        in->anim_plus1 = (int)T->animated.size() + 1;
        T->animated.push_back(A);
        {
            // Transform::Decompose leaves a mirror in R ("XXX TODO FIXME deal with flip", util/transform.cpp:223): the quaternion of an
            // improper R is not a unit one, and the reference's in-between matrices and motion bounds are off.  The matrices are
            // restated (so the motion is the reference's); the bounds are this build's samples of it — say so.
            const auto &m = u.renderFromInstance.m.m;
            const float det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                              m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
            if (det < 0 && A.actually_animated)
                fprintf(stderr, "Warning: %s: animated transformation with a mirror: the reference's decomposition does not handle the flip; images may differ from it where its motion bounds cut the primitive\n", u.loc.c_str());
        }
        auto corner = [&](int c) { return V3{b[(c & 1) ? 3 : 0], b[(c & 2) ? 4 : 1], b[(c & 4) ? 5 : 2]}; };
        if (!A.has_rotation) {
            for (int c = 0; c < 8; ++c) wb = Union(wb, u.renderFromInstance.Point(corner(c)));
            B3 we;
            for (int c = 0; c < 8; ++c) we = Union(we, u.renderFromInstanceEnd.Point(corner(c)));
            wb = Union(wb, we);
        } else {
            constexpr int NS = 1024;
            float pad = 0;
            for (int c = 0; c < 8; ++c) {
                V3 prev{0, 0, 0};
                for (int k = 0; k <= NS; ++k) {
                    const float time = u.startTime + (u.endTime - u.startTime) * ((float)k / NS);
                    const V3 q = AnimatedAt(A, k == 0 ? u.startTime : k == NS ? u.endTime : time).Point(corner(c));
                    wb = Union(wb, q);
                    if (k > 0) pad = std::max(pad, Length(q - prev));
                    prev = q;
                }
            }
            wb.pMin = wb.pMin - V3{pad, pad, pad};
            wb.pMax = wb.pMax + V3{pad, pad, pad};
        }
        return wb;
    }

    // the animated shapes inside definitions (scene.cpp:1535-1551): AnimatedPrimitive(the entity's aggregate, renderFromShape) joins the
    // definition's primitives after its static shapes, under MotionBounds of the entity's box; the definition's tree and root box are built over that
    void PlaceNested() {
        const int nTrisAll = (int)T->triIndices.size() / 3, nQuads = (int)T->quadrics.size();
        for (size_t d = 0; d < defPrims.size(); ++d) {
            if (defNested[d].empty()) continue;
            std::vector<NestedPlacement> kept;
            for (NestedPlacement &np : defNested[d]) {
                if (defPrims[np.record.def].empty()) continue;   // (an entity whose shapes made no primitive)
                // (its hidden definition's name is no message for a user: the Shape's location instead)
                if (!IsAffine(np.use->renderFromInstance)) Die(np.use->loc, "only affine transformations are supported for an animated shape inside an object instance definition");
                np.record.render_from_instance = np.use->renderFromInstance.abi();
                const B3 nb = AnimatedPlacement(*np.use, defBounds[np.record.def], &np.record);
                for (int c = 0; c < 3; ++c)
                    if (!std::isfinite(nb.pMin[c]) || !std::isfinite(nb.pMax[c])) Die(np.use->loc, "the bounds of an animated shape are not finite (its transformation?)");
                defPrims[d].emplace_back(nTrisAll + nQuads + (int)kept.size(), nb);
                kept.push_back(np);
            }
            defNested[d] = kept;
            RequireFinite(defPrims[d], "object instance definition");
            B3 b;
            for (const auto &p : defPrims[d]) b = Union(b, p.second);
            defBounds[d] = b;
        }
    }

    // the instances (scene.cpp:1560-1577): TransformedPrimitive(definition, renderFromInstance), after the shapes
    void PlaceInstances() {
        const int nTrisAll = (int)T->triIndices.size() / 3, nQuads = (int)T->quadrics.size();
        for (const InstanceUse &u : allUses) {
            const int d = defIndex.at(u.name);
            if (defPrims[d].empty()) continue;  // empty instance
            wf_instance in{};
            in.render_from_instance = u.renderFromInstance.abi();
            if (!IsAffine(u.renderFromInstance)) Die("", u.name + ": only affine instance transformations are supported");
            in.def = d;
            // TransformedPrimitive::Bounds = (*renderFromPrimitive)(primitive.Bounds()): the 8 corners (util/transform.cpp:134-139)
            const B3 &db = defBounds[d];
            const float b[6] = {db.pMin.x, db.pMin.y, db.pMin.z, db.pMax.x, db.pMax.y, db.pMax.z};
            B3 wb;
            if (u.animated) wb = AnimatedPlacement(u, db, &in);
            else for (int c = 0; c < 8; ++c) wb = Union(wb, u.renderFromInstance.Point(V3{b[(c & 1) ? 3 : 0], b[(c & 2) ? 4 : 1], b[(c & 4) ? 5 : 2]}));
            for (int c = 0; c < 3; ++c)
                if (!std::isfinite(wb.pMin[c]) || !std::isfinite(wb.pMax[c])) Die("", u.name + ": the bounds of an object instance are not finite (its transformation?)");
            topPrims.emplace_back(nTrisAll + nQuads + (int)T->instances.size(), wb);
            const int outer = (int)T->instances.size();
            if (!defNested[d].empty()) in.nested_first = outer + 1;
            T->instances.push_back(in);
            // one record per nested placement of this use (include/wf_abi.h wf_instance): a hit names the pair (use, moving entity) by its index
            for (const NestedPlacement &np : defNested[d]) {
                wf_instance rec = np.record;
                rec.outer_plus1 = outer + 1;
                T->instances.push_back(rec);
            }
        }
    }

    // The top-level tree needs only the BOUNDS of the instance definitions (= the union of their primitives' bounds, what the root of
    // BVHAggregate(prims) holds), so it is built CONCURRENTLY with the definitions' trees: on the device when it is large and a GPU is visible
    // (csrc/hip/wf_bvh_build.hip — the host cores stay with the definitions), else by the host builder's own helper threads.
    // Definitions: BVHAggregate(prims) with the constructor's default maxPrimsInNode = 1 (scene.cpp:1539-1543, cpu/aggregates.h:34).
    void BuildTrees(const AccelParams &accel) {
        std::vector<wf_bvh_node> defNodes;
        std::vector<int32_t> defOrdered;
        T->instanceDefs.resize(defPrims.size());
        std::string topError;
        std::thread topBuild([&] {
            try { BuildBVH(topPrims, accel.maxPrims, &T->bvhNodes, &T->bvhPrims, accel.splitCode); }
            catch (const std::exception &e) { topError = e.what(); }
        });
        // (an exception between here and the join — a bad_alloc of the definitions' arrays — must not destroy a joinable thread, which
        // is std::terminate instead of a SceneError: ADVICE r3)
        struct JoinGuard { std::thread &t; ~JoinGuard() { if (t.joinable()) t.join(); } } topBuildGuard{topBuild};
        // the definitions' trees are independent: built concurrently into local arrays (a pool of threads takes them in turn), then
        // appended in definition order — the arrays are the sequential loop's
        std::vector<std::vector<wf_bvh_node>> ln(defPrims.size());
        std::vector<std::vector<int32_t>> lo(defPrims.size());
        std::vector<int> lroot(defPrims.size(), -1);
        std::string firstError;
        std::mutex errMutex;
        ParallelFor(defPrims.size(), [&](size_t d) {
            try { lroot[d] = BuildBVH(defPrims[d], 1, &ln[d], &lo[d], 0, /* forceHost: the device is busy with the top level */ true); }
            catch (const std::exception &e) { std::lock_guard<std::mutex> g(errMutex); if (firstError.empty()) firstError = e.what(); }
        });
        if (!firstError.empty()) { topBuild.join(); throw SceneError(firstError); }
        for (size_t d = 0; d < defPrims.size(); ++d) {
            wf_instance_def &def = T->instanceDefs[d];
            def = wf_instance_def{};
            def.first_prim = (int)defOrdered.size();
            def.n_prims = (int)defPrims[d].size();
            const int nodeBase = (int)defNodes.size(), primBase = (int)defOrdered.size();
            def.bvh_root = lroot[d] < 0 ? -1 : nodeBase + lroot[d];
            for (wf_bvh_node &n : ln[d]) n.offset += n.nprims > 0 ? primBase : nodeBase;
            defNodes.insert(defNodes.end(), ln[d].begin(), ln[d].end());
            defOrdered.insert(defOrdered.end(), lo[d].begin(), lo[d].end());
            def.n_nodes = (int)defNodes.size() - (def.bvh_root < 0 ? (int)defNodes.size() : def.bvh_root);
            if (def.bvh_root >= 0)
                for (int c = 0; c < 3; ++c) { def.bounds[c] = defNodes[def.bvh_root].bmin[c]; def.bounds[3 + c] = defNodes[def.bvh_root].bmax[c]; }
        }
        Tick("instance-definition BVHs (SAH)");
        topBuild.join();
        if (!topError.empty()) throw SceneError(topError);
        Tick(accel.splitCode == 1 ? "top-level BVH (HLBVH), the part not hidden behind the definitions" : "top-level BVH (SAH), the part not hidden behind the definitions");
        MergeDefinitionTrees(defNodes, defOrdered);
    }

    // the definitions' trees go behind the top-level tree in the same arrays
    void MergeDefinitionTrees(std::vector<wf_bvh_node> &defNodes, const std::vector<int32_t> &defOrdered) {
        T->nTopBvhNodes = (int)T->bvhNodes.size();
        T->nTopPrims = (int)T->bvhPrims.size();
        const int nodeShift = T->nTopBvhNodes, primShift = T->nTopPrims;
        for (wf_bvh_node &n : defNodes) n.offset += n.nprims > 0 ? primShift : nodeShift;
        for (wf_instance_def &def : T->instanceDefs) { if (def.bvh_root >= 0) def.bvh_root += nodeShift; def.first_prim += primShift; }
        T->bvhNodes.insert(T->bvhNodes.end(), defNodes.begin(), defNodes.end());
        T->bvhPrims.insert(T->bvhPrims.end(), defOrdered.begin(), defOrdered.end());
    }

    // Light::Preprocess(sceneBounds) (integrator.cpp:172-173; lights.h:243-246,546-549)
    void PreprocessLights() {
        B3 sceneBounds;
        for (int c = 0; c < 3; ++c) { sceneBounds.pMin[c] = T->bvhNodes[0].bmin[c]; sceneBounds.pMax[c] = T->bvhNodes[0].bmax[c]; }
        for (int c = 0; c < 3; ++c) { T->desc.scene_bounds[c] = sceneBounds.pMin[c]; T->desc.scene_bounds[3 + c] = sceneBounds.pMax[c]; }
        V3 center = (sceneBounds.pMin + sceneBounds.pMax) / 2;
        float radius = Inside(center, sceneBounds) ? Distance(center, sceneBounds.pMax) : 0;
        for (wf_light &l : T->lights)
            if (l.type == WF_LIGHT_DISTANT || l.type == WF_LIGHT_UNIFORM_INFINITE || l.type == WF_LIGHT_IMAGE_INFINITE || l.type == WF_LIGHT_PORTAL_INFINITE) {
                l.sceneCenter[0] = center.x; l.sceneCenter[1] = center.y; l.sceneCenter[2] = center.z;
                l.sceneRadius = radius;
            }
    }

    // ---- light sampler (integrator.cpp:181-187, lightsamplers.cpp:28-62) ----
    void BuildLightSampler() {
        if (T->lights.size() == 1) lightSamplerName = "uniform";
        if (lightSamplerName == "uniform") T->desc.light_sampler = WF_LS_UNIFORM;
        else if (lightSamplerName == "power") {
            T->desc.light_sampler = WF_LS_POWER;
            BuildPowerAlias(T);
        } else {
            if (lightSamplerName != "bvh") fprintf(stderr, "Warning: Light sample distribution type \"%s\" unknown. Using \"bvh\".\n", lightSamplerName.c_str());
            T->desc.light_sampler = WF_LS_BVH;
            // lights without Bounds() (distant, infinite) are the BVH sampler's "infiniteLights" — already listed
            BuildLightBVH(bvhLights, allLightBounds, &T->lightBvh, &T->lights);
        }
        for (int c = 0; c < 3; ++c) { T->desc.all_light_bounds[c] = allLightBounds.pMin[c]; T->desc.all_light_bounds[3 + c] = allLightBounds.pMax[c]; }
    }

    // "haveMedia" (integrator.cpp:91-111,51): a shape names a medium, or an "interface" material is present
    void SetHaveMedia() {
        T->desc.have_media = anyMediumInterface ? 1 : 0;
        for (const wf_mesh &m : T->meshes) if (m.material < 0) T->desc.have_media = 1;
        // ... "present": updateMaterialNeeds runs over every material the scene CREATES, named or not, used by a shape or not
        // (wavefront/integrator.cpp:47-66,139-146) — a defined but unused "interface" material already sends the shadow rays through
        // TraceTransmittance (differential fuzzing, round 3: 1-ulp differences on 8 % of the values of such a scene)
        for (const wf_material &m : T->materials) if (m.type == WF_MAT_INTERFACE) T->desc.have_media = 1;
    }

    // wavefront pass geometry (integrator.cpp:227-236)
    void SetPassGeometry() {
        const wf_film &F = T->desc.film;
        int resx = F.pixel_max[0] - F.pixel_min[0], resy = F.pixel_max[1] - F.pixel_min[1];
        int maxSamples = 1024 * 1024;
        T->scanlinesPerPass = std::max(1, maxSamples / resx);
        T->nPasses = (resy + T->scanlinesPerPass - 1) / T->scanlinesPerPass;
        T->scanlinesPerPass = (resy + T->nPasses - 1) / T->nPasses;
        T->maxQueueSize = resx * T->scanlinesPerPass;
    }
};

}  // namespace

// ---- main entry ---------------------------------------------------------------------------------------
void BuildSceneTables(const ParsedScene &scene, const RenderOptions &optIn, SceneTables *T) {
    SceneBuild b(scene, optIn, T);
    RenderOptions &opt = b.opt;
    // the samplers' Create functions: `if (Options->quickRender) nsamp = 1` after the --spp override (samplers.cpp:74,113,152,214,264,314 —
    // every sampler but the independent one, which keeps its sample count)
    if (opt.quickRender && scene.sampler.name != "independent") opt.pixelSamples = 1;
    // rendering space: camera-world (cameras.cpp:35-41)
    // (for a moving camera: its position at the middle of the TransformTimes interval — computed where the Camera directive is parsed)
    Transform renderFromWorld = scene.renderFromWorld;
    Transform worldFromRender = Inverse(renderFromWorld);

    BuildFilter(scene, T);
    BuildFilm(scene, opt, T);
    BuildSampler(scene, opt, T);
    BuildCamera(scene, renderFromWorld, T);
    if (T->desc.film.type == WF_FILM_GBUFFER) {
        // outputFromRender: cameraTransform.RenderFromCamera() applied inversely ("camera"), or WorldFromRender ("world") — film.cpp:828-839
        T->desc.film.gbuffer_from_render = T->desc.film.apply_inverse ? T->desc.camera.renderFromCamera : worldFromRender.abi();
        if (T->desc.film.apply_inverse && T->desc.camera.anim.actually_animated)
            Die(scene.film.loc, "gbuffer film: \"coordinatesystem\" \"camera\" with a moving camera is not supported by this build (use \"world\")");
    }

    T->desc.options.seed = opt.seed;
    T->desc.options.disable_pixel_jitter = opt.disablePixelJitter;
    T->desc.options.disable_wavelength_jitter = opt.disableWavelengthJitter;
    T->desc.options.disable_texture_filtering = opt.disableTextureFiltering;

    // integrator (wavefront/integrator.cpp:183-198)
    const ParamSet &ip = scene.integrator.params;
    if (scene.integrator.name != "path" && scene.integrator.name != "volpath")
        fprintf(stderr, "Warning: Ignoring specified integrator \"%s\": the wavefront integrator always uses a \"volpath\" integrator.\n", scene.integrator.name.c_str());
    T->desc.regularize = ip.GetOneBool("regularize", false);
    T->desc.max_depth = ip.GetOneInt("maxdepth", 5);
    b.lightSamplerName = ip.GetOneString("lightsampler", "bvh");

    // media (scene.cpp CreateMedia -> Medium::Create, media.cpp:667-689)
    BuildMedia(scene, T, &b.mediumIds);
    T->desc.camera.medium = b.MediumId(scene.cameraMedium, scene.camera.loc);

    // textures and materials (scene.cpp:1110-1171)
    TexBuilder &tb = b.tb;
    tb.T = T;
    tb.scene = &scene;
    tb.disableImageTextures = opt.disableImageTextures;
    tb.CreateNamedTextures();
    for (const auto &nm : scene.namedMaterials) tb.namedMaterialIds[nm.first] = tb.CreateMaterial(nm.second);
    for (const Entity &m : scene.materials) b.materialIds.push_back(tb.CreateMaterial(m));

    // shapes -> meshes; instances are flattened (each use re-instantiates the definition's triangles
    // with renderFromInstance applied) — see DESIGN.md "Instancing".
    b.PrefetchPly();
    for (const ShapeEntity &sh : scene.shapes) b.AddShape(sh, &b.topPrims, false);
    b.CreateDefinitions();
    b.AddPlaceholderIfEmpty();
    b.AssignQuadricIds();

    b.AddAreaLights();
    b.AddLights();
    b.Tick("textures, materials, shapes (PLY), lights");

    const AccelParams accel = b.ParseAccelerator();
    b.BoundDefinitions();
    b.PlaceNested();
    b.PlaceInstances();
    b.BuildTrees(accel);

    b.PreprocessLights();
    b.BuildLightSampler();
    b.SetHaveMedia();
    b.SetPassGeometry();
    // (no ReportUnused: only Integrator::Create — the CPU integrators — reports the integrator's unused parameters, cpu/integrators.cpp:3691;
    //  the wavefront integrator reads what it knows and ignores the rest)
    T->Finalize();
    b.Tick("light sampler, finalisation");
}

}  // namespace wf
