// tools/film_add_check.cpp — the per-item bodies of wf_film_add_samples_device (pbrt-v4_amd/csrc/hip/wf_film_add.h) compiled for the
// host and run against the render's own film update, KUpdateFilm (csrc/common/wf_kernels.h).  Stand-alone: no device, neither library.
//
// For each film type (RGB, spectral, GBuffer) it fabricates a SceneView — a dense sensor table, a wf_film with a crop window — and a
// WorkState of one sample per pixel, runs KUpdateFilm into one film and filmadd::AddItem into another (both start from the same
// non-zero accumulators, and the items are added twice, as two calls), and requires the rgb / weight accumulators and the spectral
// accumulators to be equal byte for byte.  The items cover the pixel bounds (every pixel of the window and one step outside each
// edge) and, on chosen pixels:
//   component maxima one ulp below, at and one ulp above max_component_value     PDFs with one, three and four zeros
//   wavelengths at lambda_min, at lambda_max and on every bucket boundary         two wavelengths of one item in one bucket
//   negative and zero filter weights                                              +infinity and NaN radiance
// Then the one-sample-per-pixel contract: a call whose items name pixels twice rejects exactly the second ones and adds what the call
// without them adds; the next call (the next epoch) adds to the same pixels again.  And the epochs' wrap, with the entry point's own
// bookkeeping (filmadd::NextEpoch): after the call of epoch INT32_MAX the stamps are cleared and the call of epoch 1 adds every item,
// which it would not over the stamps an earlier call of epoch 1 left.
// Exits non-zero at the first difference.  Built with -fsanitize=address,undefined it is how that code is run under the sanitizers.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "../pbrt-v4_amd/csrc/hip/wf_film_add.h"

using namespace wf;

namespace {

constexpr int W = 23, H = 11, X0 = 3, Y0 = 2, NB = 16;
constexpr float MCV = 3.5f, INF = std::numeric_limits<float>::infinity();
constexpr int PROBE = 400 - WF_LAMBDA_MIN;   // the table entry of 400 nm: rbar 4, gbar 2, bbar 1 (with imaging_ratio 1/2: r = Lw[0] / 2 exactly)

struct Items {
    std::vector<I2> pixel;
    std::vector<F4> L, camW, lambda, pdf, zero;
    std::vector<float> fw;
    size_t size() const { return pixel.size(); }
};

float BucketEdge(int k) { return 360.f + (float)k * (470.f / NB); }

Items MakeItems(std::mt19937 &rng) {
    std::uniform_real_distribution<float> uni(0.f, 1.f);
    Items it;
    for (int y = Y0 - 1; y <= Y0 + H; ++y)
        for (int x = X0 - 1; x <= X0 + W; ++x) {
            it.pixel.push_back(I2{x, y});
            const float u = uni(rng);
            F4 lam;
            float *l = &lam.x;
            l[0] = 360.f + u * 470.f;
            for (int i = 1; i < 4; ++i) { l[i] = l[i - 1] + 117.5f; if (l[i] > 830.f) l[i] = 360.f + (l[i] - 830.f); }
            it.lambda.push_back(lam);
            const float p = 1.f / 470.f;
            it.pdf.push_back(F4{p, p, p, p});
            const float s = std::pow(10.f, -3.f + 5.f * uni(rng));   // up to 100: many samples' sensor maxima exceed MCV
            it.L.push_back(F4{s * uni(rng), s * uni(rng), s * uni(rng), s * uni(rng)});
            it.camW.push_back(F4{0.5f + uni(rng), 0.5f + uni(rng), 0.5f + uni(rng), 0.5f + uni(rng)});
            it.fw.push_back(-0.2f + 1.4f * uni(rng));
        }
    it.zero.assign(it.size(), F4{0, 0, 0, 0});
    auto at = [&](int x, int y) { return (size_t)(y - (Y0 - 1)) * (W + 2) + (x - (X0 - 1)); };
    // row Y0 + 1: the clamp threshold.  Lw = (x, 0, 0, 0) at 400 nm with PDF (1, 0, 0, 0): r = x / 2, the largest component
    const float around[3] = {std::nextafter(MCV, 0.f), MCV, std::nextafter(MCV, INF)};
    for (int k = 0; k < 3; ++k) {
        const size_t i = at(X0 + 1 + k, Y0 + 1);
        it.L[i] = F4{2 * around[k], 7.f, 9.f, 11.f}; it.camW[i] = F4{1, 1, 1, 1};
        it.lambda[i] = F4{400.f, 517.5f, 635.f, 752.5f}; it.pdf[i] = F4{1, 0, 0, 0};   // (three zeros)
        it.fw[i] = 0.75f;
    }
    it.pdf[at(X0 + 5, Y0 + 1)].z = 0;                                   // one zero
    it.pdf[at(X0 + 6, Y0 + 1)] = F4{0, 0, 0, 0};                        // four zeros
    it.pdf[at(X0 + 7, Y0 + 1)] = F4{0.25f / 470.f, 0, 0, 0};            // a terminated secondary
    // row Y0 + 2 .. : lambda_min, lambda_max and every bucket boundary, in each of the four slots
    for (int k = 0; k <= NB; ++k) {
        const size_t i = at(X0 + k, Y0 + 2), j = at(X0 + k, Y0 + 3);
        it.lambda[i].x = BucketEdge(k);
        it.lambda[j].w = BucketEdge(k);
        it.lambda[j].y = std::nextafter(BucketEdge(k), 0.f);
    }
    it.lambda[at(X0 + 18, Y0 + 2)] = F4{360.f, 830.f, 360.f, 830.f};
    it.lambda[at(X0 + 19, Y0 + 2)] = F4{500.f, 501.f, 502.f, 700.f};    // three wavelengths in one bucket
    it.lambda[at(X0 + 20, Y0 + 2)] = F4{359.4f, 830.6f, 300.f, 900.f};  // outside the table: sensor 0, the bucket clamp
    // row Y0 + 4: weights and non-finite radiance
    it.fw[at(X0 + 0, Y0 + 4)] = 0.f;
    it.fw[at(X0 + 1, Y0 + 4)] = -0.f;
    it.fw[at(X0 + 2, Y0 + 4)] = -0.625f;
    it.L[at(X0 + 3, Y0 + 4)].y = INF;
    it.L[at(X0 + 4, Y0 + 4)].x = std::numeric_limits<float>::quiet_NaN();
    it.L[at(X0 + 5, Y0 + 4)] = F4{INF, INF, INF, INF};
    it.L[at(X0 + 6, Y0 + 4)].w = -INF;
    it.L[at(X0 + 7, Y0 + 4)] = F4{0, 0, 0, 0};
    it.L[at(X0 + 8, Y0 + 4)] = F4{-1.f, 2.f, -3.f, 4.f};
    // corners of the window with large radiance (the clamp on an edge pixel)
    for (size_t i : {at(X0, Y0), at(X0 + W - 1, Y0), at(X0, Y0 + H - 1), at(X0 + W - 1, Y0 + H - 1)}) it.L[i] = F4{900.f, 800.f, 700.f, 600.f};
    return it;
}

struct Film {
    std::vector<double> rgbw, spectral;
    std::vector<wf_gbuffer_pixel> gb;
};

bool Same(const char *what, int type, const std::vector<double> &a, const std::vector<double> &b, int per) {
    if (a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0)) return true;
    for (size_t i = 0; i < a.size() && i < b.size(); ++i)
        if (memcmp(&a[i], &b[i], sizeof(double)) != 0) {
            fprintf(stderr, "film type %d, %s: pixel %zu value %zu: KUpdateFilm %a, AddItem %a\n", type, what, i / per, i % per, a[i], b[i]);
            break;
        }
    return false;
}

template <bool SPECTRAL>
int AddAll(const SceneView &sv, Film &f, std::vector<int32_t> &stamps, int32_t epoch, const Items &it, const std::vector<F4> &Lw, const std::vector<size_t> &order) {
    int rejected = 0;
    for (size_t i : order)
        rejected += filmadd::AddItem<SPECTRAL>(sv, f.rgbw.data(), SPECTRAL ? f.spectral.data() : nullptr, stamps.data(), epoch, it.pixel[i], Lw[i], it.lambda[i],
                                               it.pdf[i], it.fw[i]);
    return rejected;
}

int CheckType(int type) {
    std::mt19937 rng(11 + type);
    std::uniform_real_distribution<float> uni(0.f, 1.f);
    // the sensor: three dense spectra of positive values; the probe entry is exact
    std::vector<float> table(3 * WF_NDENSE);
    for (float &v : table) v = 0.05f + 1.9f * uni(rng);
    table[PROBE] = 4.f; table[WF_NDENSE + PROBE] = 2.f; table[2 * WF_NDENSE + PROBE] = 1.f;
    SceneView sv{};
    sv.spectrumData = table.data();
    wf_film &F = sv.film;
    F.full_res[0] = 40; F.full_res[1] = 20;
    F.pixel_min[0] = X0; F.pixel_min[1] = Y0; F.pixel_max[0] = X0 + W; F.pixel_max[1] = Y0 + H;
    F.imaging_ratio = 0.5f;
    F.max_component_value = MCV;
    F.rbar_offset = 0; F.gbar_offset = WF_NDENSE; F.bbar_offset = 2 * WF_NDENSE;
    F.type = type;
    F.n_buckets = NB; F.lambda_min = 360.f; F.lambda_max = 830.f;

    const Items it = MakeItems(rng);
    const size_t n = it.size(), pixels = (size_t)W * H;
    std::vector<F4> L = it.L, camW = it.camW, lam = it.lambda, pdf = it.pdf, zero = it.zero;
    std::vector<I2> pix = it.pixel;
    std::vector<float> fw = it.fw;
    // Lw as the caller of the device call computes it: one fp32 multiply per channel
    std::vector<F4> Lw(n);
    for (size_t i = 0; i < n; ++i) Lw[i] = F4{L[i].x * camW[i].x, L[i].y * camW[i].y, L[i].z * camW[i].z, L[i].w * camW[i].w};

    // what the items were built to cover, checked on the unclamped sensor values
    {
        SceneView open = sv;
        open.film.max_component_value = INF;
        int below = 0, at = 0, above = 0, over = 0;
        for (size_t i = 0; i < n; ++i) {
            Wavelengths w;
            memcpy(w.lambda, &lam[i], 16); memcpy(w.pdf, &pdf[i], 16);
            float v[4];
            FilmSensorRGBW(open, toS4(Lw[i]), w, 1.f, v);
            const float m = std::fmax(std::fmax(v[0], v[1]), v[2]);
            below += m == std::nextafter(MCV, 0.f); at += m == MCV; above += m == std::nextafter(MCV, INF); over += m > MCV;
        }
        if (below != 1 || at != 1 || above != 1 || over < 20) {
            fprintf(stderr, "the fabricated items miss the clamp threshold: %d below, %d at, %d above, %d over\n", below, at, above, over);
            return 1;
        }
    }

    Film want, got;
    want.rgbw.resize(4 * pixels);
    for (double &v : want.rgbw) v = (double)uni(rng) * 3.;
    if (type == WF_FILM_SPECTRAL) { want.spectral.resize(2 * NB * pixels); for (double &v : want.spectral) v = (double)uni(rng); }
    if (type == WF_FILM_GBUFFER) want.gb.assign(pixels, wf_gbuffer_pixel{});
    got = want;
    const Film start = want;

    WorkState ws{};
    ws.maxQueueSize = ws.pixelsPerPass = (int)n; ws.samplesPerPass = 1; ws.slotStride = 1;
    ws.stripCount = 1; ws.stripHeight = 1; ws.localRows = H;
    ws.filterWeight = fw.data(); ws.pPixel = pix.data(); ws.lambda = lam.data(); ws.lambdaPdf = pdf.data(); ws.L = L.data(); ws.cameraRayWeight = camW.data();
    ws.film = want.rgbw.data();
    ws.filmSpectral = type == WF_FILM_SPECTRAL ? want.spectral.data() : nullptr;
    ws.filmGBuffer = type == WF_FILM_GBUFFER ? want.gb.data() : nullptr;
    ws.vsP = zero.data();   // a GBuffer film's samples without a visible surface (vp.w == 0): the RGB part only

    std::vector<int32_t> stamps(pixels, 0);
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = i;
    int32_t epoch = 0;
    for (int call = 0; call < 2; ++call) {
        for (size_t p = 0; p < n; ++p) KUpdateFilm(sv, ws, (int)p, 1);
        const int rej = type == WF_FILM_SPECTRAL ? AddAll<true>(sv, got, stamps, ++epoch, it, Lw, order) : AddAll<false>(sv, got, stamps, ++epoch, it, Lw, order);
        if (rej != 0) { fprintf(stderr, "film type %d, call %d: %d items rejected, every item names a pixel of its own\n", type, call, rej); return 1; }
        if (!Same("rgb / weight", type, want.rgbw, got.rgbw, 4) || !Same("spectral", type, want.spectral, got.spectral, 2 * NB)) return 1;
    }
    if (want.rgbw == start.rgbw) { fprintf(stderr, "film type %d: nothing was added\n", type); return 1; }
    if (type == WF_FILM_GBUFFER && memcmp(want.gb.data(), start.gb.data(), pixels * sizeof(wf_gbuffer_pixel)) != 0) {
        fprintf(stderr, "gbuffer: KUpdateFilm touched the visible-surface sums of samples without a surface\n");
        return 1;
    }

    // duplicates: seven in-window items a second time (identical values), spread through the call
    std::vector<size_t> dup = order;
    int made = 0;
    for (size_t i = 0; i < n && made < 7; i += 31) {
        size_t idx;
        if (!filmadd::FilmIndex(F, it.pixel[i], &idx)) continue;
        dup.insert(dup.begin() + (made % 2 ? dup.size() / 2 : dup.size()), i);
        ++made;
    }
    Film a = got, b = got;
    std::vector<int32_t> sa = stamps, sb = stamps;
    const int32_t e = ++epoch;
    const int ra = type == WF_FILM_SPECTRAL ? AddAll<true>(sv, a, sa, e, it, Lw, order) : AddAll<false>(sv, a, sa, e, it, Lw, order);
    const int rb = type == WF_FILM_SPECTRAL ? AddAll<true>(sv, b, sb, e, it, Lw, dup) : AddAll<false>(sv, b, sb, e, it, Lw, dup);
    if (made != 7 || ra != 0 || rb != 7) { fprintf(stderr, "film type %d: %d duplicates made, %d / %d rejected without / with them\n", type, made, ra, rb); return 1; }
    if (!Same("rgb / weight with duplicates", type, a.rgbw, b.rgbw, 4) || !Same("spectral with duplicates", type, a.spectral, b.spectral, 2 * NB)) return 1;
    const int32_t next = ++epoch;
    const int rc = type == WF_FILM_SPECTRAL ? AddAll<true>(sv, b, sb, next, it, Lw, order) : AddAll<false>(sv, b, sb, next, it, Lw, order);
    if (rc != 0) { fprintf(stderr, "film type %d: the call after the duplicates rejected %d items\n", type, rc); return 1; }

    // the epochs wrap: every pixel carries the stamp of a call of epoch 1, the first half of the items the stamp of the call of epoch
    // INT32_MAX as well.  The next call is epoch 1 again, over cleared stamps (NextEpoch says so), and must add every item; over the
    // stamps as they stand it would reject the items of the second half, whose pixels still say 1
    {
        bool clear;
        if (filmadd::NextEpoch(0, &clear) != 1 || clear || filmadd::NextEpoch(1, &clear) != 2 || clear ||
            filmadd::NextEpoch(INT32_MAX - 1, &clear) != INT32_MAX || clear) {
            fprintf(stderr, "NextEpoch: the epochs do not run 1, 2 .. INT32_MAX without a clear\n");
            return 1;
        }
        const std::vector<size_t> half(order.begin(), order.begin() + n / 2);
        size_t stale = 0, idx;   // in-window items of the second half
        for (size_t i = n / 2; i < n; ++i) stale += filmadd::FilmIndex(F, it.pixel[i], &idx);
        Film w = got, ref = got;
        std::vector<int32_t> sw(pixels, 0), sr(pixels, 0);
        int r = type == WF_FILM_SPECTRAL ? AddAll<true>(sv, w, sw, 1, it, Lw, order) : AddAll<false>(sv, w, sw, 1, it, Lw, order);
        r += type == WF_FILM_SPECTRAL ? AddAll<true>(sv, w, sw, INT32_MAX, it, Lw, half) : AddAll<false>(sv, w, sw, INT32_MAX, it, Lw, half);
        r += type == WF_FILM_SPECTRAL ? AddAll<true>(sv, ref, sr, 1, it, Lw, order) : AddAll<false>(sv, ref, sr, 1, it, Lw, order);
        r += type == WF_FILM_SPECTRAL ? AddAll<true>(sv, ref, sr, 2, it, Lw, half) : AddAll<false>(sv, ref, sr, 2, it, Lw, half);
        const int32_t wrapped = filmadd::NextEpoch(INT32_MAX, &clear);
        if (r != 0 || wrapped != 1 || !clear) { fprintf(stderr, "film type %d: before the wrap %d rejected; NextEpoch(INT32_MAX) = %d, clear %d\n", type, r, wrapped, (int)clear); return 1; }
        Film kept = w;
        std::vector<int32_t> sk = sw;
        const int rk = type == WF_FILM_SPECTRAL ? AddAll<true>(sv, kept, sk, wrapped, it, Lw, order) : AddAll<false>(sv, kept, sk, wrapped, it, Lw, order);
        if (stale == 0 || rk != (int)stale) { fprintf(stderr, "film type %d: epoch 1 over uncleared stamps rejected %d items, %zu stale pixels\n", type, rk, stale); return 1; }
        std::fill(sw.begin(), sw.end(), 0);
        const int rw = type == WF_FILM_SPECTRAL ? AddAll<true>(sv, w, sw, wrapped, it, Lw, dup) : AddAll<false>(sv, w, sw, wrapped, it, Lw, dup);
        const int rr = type == WF_FILM_SPECTRAL ? AddAll<true>(sv, ref, sr, 3, it, Lw, order) : AddAll<false>(sv, ref, sr, 3, it, Lw, order);
        if (rw != 7 || rr != 0) { fprintf(stderr, "film type %d: the call after the wrap rejected %d items (7 duplicates), the one without a wrap %d\n", type, rw, rr); return 1; }
        if (!Same("rgb / weight across the epoch wrap", type, ref.rgbw, w.rgbw, 4) || !Same("spectral across the epoch wrap", type, ref.spectral, w.spectral, 2 * NB)) return 1;
    }

    printf("film type %d: %zu items (%zu pixels in the window), 2 calls: no difference; 7 duplicates rejected; the epoch wrap adds every item\n", type, n, pixels);
    return 0;
}

}  // namespace

int main() {
    for (int type : {(int)WF_FILM_RGB, (int)WF_FILM_SPECTRAL, (int)WF_FILM_GBUFFER})
        if (CheckType(type)) return 1;
    return 0;
}
