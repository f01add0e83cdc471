// tools/film_develop_check.cpp — the per-pixel bodies of the device film develop (pbrt-v4_amd/csrc/hip/wf_film_develop.h) compiled for
// the host and run against the host loops of csrc/host/image_io.cpp they restate.  Stand-alone: no device, neither library.
//
//   film_develop_check round [threads]   the header's RoundToHalf against image_io.cpp's over all 2^32 float bit patterns
//   film_develop_check arrays            DevelopRGB / DevelopBucket / DevelopGBuffer against FilmToRGB / SpectralFilmImage /
//                                        GBufferFilmImage over fabricated accumulators: every half value, every tie between two halves
//                                        and one ulp either side of it, the subnormal halves, the overflow threshold, zero and negative
//                                        weights, NaN and infinite sums, zero-length normals, variance counts 0 / 1 / 2 — with savefp16
//                                        on and off, every value compared by its bits, the NaN counts against the construction
//
// Exits non-zero at the first difference.  Built with -fsanitize=address,undefined (make -C pbrt-v4_amd OUT=<dir> SAN="..." with CXX the
// compiler of every unit) the `arrays` run is how that code is run under the sanitizers.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <thread>
#include <vector>
#include "../pbrt-v4_amd/csrc/host/scene.h"
#include "../pbrt-v4_amd/csrc/hip/wf_film_develop.h"

using namespace wf;

static uint32_t BitsOf(float f) { uint32_t x; memcpy(&x, &f, 4); return x; }
static float FloatOf(uint32_t x) { float f; memcpy(&f, &x, 4); return f; }

static int CheckRound(int threads) {
    std::atomic<bool> bad{false};
    std::vector<std::thread> pool;
    const uint64_t total = 1ull << 32, chunk = total / threads + 1;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            const uint64_t a = t * chunk, b = std::min(total, a + chunk);
            for (uint64_t u = a; u < b; ++u) {
                const float f = FloatOf((uint32_t)u);
                const uint32_t want = BitsOf(RoundToHalf(f)), got = BitsOf(develop::RoundToHalf(f));
                if (want != got) {
                    if (!bad.exchange(true)) fprintf(stderr, "RoundToHalf(0x%08x): image_io.cpp 0x%08x, wf_film_develop.h 0x%08x\n", (uint32_t)u, want, got);
                    return;
                }
                if ((u & 0xffffff) == 0 && bad.load()) return;
            }
        });
    for (std::thread &th : pool) th.join();
    if (bad) return 1;
    printf("RoundToHalf: 4294967296 bit patterns, no difference\n");
    return 0;
}

static wf_film TestFilm(int nBuckets) {
    wf_film F{};
    const float m[3][3] = {{1.3459433f, -0.2556075f, -0.0511118f}, {-0.5445989f, 1.5081673f, 0.0205351f}, {0.0125f, -0.0118501f, 1.2118128f}};
    memcpy(F.outputRGBFromSensorRGB, m, sizeof(m));
    F.n_buckets = nBuckets;
    F.lambda_min = 360; F.lambda_max = 830;
    return F;
}

static bool SameBits(const char *what, const std::vector<float> &want, const std::vector<float> &got, int nc) {
    for (size_t i = 0; i < want.size(); ++i)
        if (BitsOf(want[i]) != BitsOf(got[i])) {
            fprintf(stderr, "%s: pixel %zu channel %zu: host loop 0x%08x, header 0x%08x\n", what, i / nc, i % nc, BitsOf(want[i]), BitsOf(got[i]));
            return false;
        }
    return true;
}

// the values the spectral buckets carry past RoundToHalf: every finite half, the midpoint above it and one float either side of that
static std::vector<float> HalfProbeValues() {
    std::vector<float> v;
    for (uint32_t h = 0; h < 0x7c00u; ++h) {
        const int e = (int)(h >> 10), m = (int)(h & 0x3ffu);
        const float x = e == 0 ? std::ldexp((float)m, -24) : std::ldexp((float)(1024 + m), e - 25);
        const float quantum = std::ldexp(1.f, (e == 0 ? 1 : e) - 25), mid = x + 0.5f * quantum;   // (65520 above the last half)
        for (float p : {x, std::nextafter(mid, 0.f), mid, std::nextafter(mid, std::numeric_limits<float>::infinity())}) { v.push_back(p); v.push_back(-p); }
    }
    for (float p : {65504.f, 65519.996f, 65520.f, 65536.f, 1e9f, 3.4e38f, std::numeric_limits<float>::infinity(), 1e-30f, 1e-42f}) { v.push_back(p); v.push_back(-p); }
    return v;
}

static int CheckArrays() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> uni(0., 1.);
    auto logUniform = [&] { return std::pow(10., -9. + 15. * uni(rng)); };
    for (int save = 0; save < 2; ++save) {
        // ---- RGB
        const int w = 64, h = 64;
        const size_t n = (size_t)w * h;
        std::vector<double> film(4 * n);
        for (size_t i = 0; i < n; ++i) { for (int c = 0; c < 3; ++c) film[4 * i + c] = logUniform(); film[4 * i + 3] = 0.25 + 8 * uni(rng); }
        size_t nanPixels = 0;
        auto set = [&](size_t i, double r, double g, double b, double wt) { film[4 * i] = r; film[4 * i + 1] = g; film[4 * i + 2] = b; film[4 * i + 3] = wt; };
        set(0, 1.5, 2.5, 3.5, 0.);
        set(1, nan, 1., 1., 2.); ++nanPixels;
        set(2, 1., 1., nan, 0.); ++nanPixels;
        set(3, inf, 0., 0., 1.);
        set(4, 0., -inf, 0., 1.);
        set(5, -1., -2., -3., 4.);
        set(6, 65510., 65510., 65510., 1.);
        set(7, 1e6, 1e6, 1e6, 1.);
        set(8, 3e-5, 2e-6, 5e-8, 1.);
        set(9, 1. + std::ldexp(1., -30), 1. / 3., 1e-46, 1.);
        set(10, 1e300, 1., 1., 1e-300);
        const wf_film F = TestFilm(8);
        const develop::RGBMatrix M = develop::OutputMatrix(F);
        std::vector<float> want(3 * n), got(3 * n);
        FilmToRGB(F, film.data(), w, h, want.data(), save != 0);
        size_t count = 0;
        for (size_t i = 0; i < n; ++i) count += develop::DevelopRGB(M, &film[4 * i], save != 0, save != 0, &got[3 * i]);
        if (!SameBits("rgb", want, got, 3)) return 1;
        if (count != 3 * nanPixels) { fprintf(stderr, "rgb: %zu NaN values counted, %zu constructed\n", count, 3 * nanPixels); return 1; }

        // ---- spectral: weights 1, sums the probe values, over as many films as they take
        const std::vector<float> probes = HalfProbeValues();
        const int nb = F.n_buckets, nc = 3 + nb;
        std::vector<std::string> names;
        size_t next = 0, rounds = 0;
        while (next < probes.size()) {
            std::vector<double> sp(2 * nb * n);
            size_t expectNaN = 0;
            for (size_t i = 0; i < n; ++i)
                for (int b = 0; b < nb; ++b) {
                    const size_t slot = i * nb + b;
                    double sum = 1., wt = 1.;
                    if (slot == 5) wt = 0.;
                    else if (slot == 6) wt = -1.;
                    else if (slot == 7) { sum = nan; ++expectNaN; }
                    else if (slot == 9) { sum = inf; wt = inf; ++expectNaN; }
                    else sum = next < probes.size() ? (double)probes[next++] : logUniform();
                    sp[2 * nb * i + b] = sum;
                    sp[2 * nb * i + nb + b] = wt;
                }
            std::vector<float> ref, dev(nc * n);
            SpectralFilmImage(F, film.data(), sp.data(), w, h, save != 0, &names, &ref);
            count = 0;
            for (size_t i = 0; i < n; ++i) {
                count += develop::DevelopRGB(M, &film[4 * i], save != 0, save != 0, &dev[nc * i]);
                for (int b = 0; b < nb; ++b) count += develop::DevelopBucket(sp[2 * nb * i + b], sp[2 * nb * i + nb + b], save != 0, &dev[nc * i + 3 + b]);
            }
            if (!SameBits("spectral", ref, dev, nc)) return 1;
            if (count != 3 * nanPixels + expectNaN) { fprintf(stderr, "spectral: %zu NaN values counted, %zu constructed\n", count, 3 * nanPixels + expectNaN); return 1; }
            ++rounds;
        }

        // ---- GBuffer
        std::vector<wf_gbuffer_pixel> gb(n);
        auto sym = [&] { return (float)((uni(rng) - 0.5) * 20.); };
        for (size_t i = 0; i < n; ++i) {
            wf_gbuffer_pixel &g = gb[i];
            memset(&g, 0, sizeof(g));
            g.gbuffer_weight_sum = 0.5 + 4 * uni(rng);
            for (int c = 0; c < 3; ++c) {
                g.rgb_albedo_sum[c] = uni(rng) * 4;
                g.var_n[c] = 4; g.var_mean[c] = (float)logUniform(); g.var_s[c] = (float)logUniform();
                g.p_sum[c] = sym(); g.n_sum[c] = sym(); g.ns_sum[c] = sym();
            }
            g.dzdx_sum = sym(); g.dzdy_sum = sym(); g.uv_sum[0] = (float)uni(rng); g.uv_sum[1] = (float)uni(rng);
        }
        gb[20].gbuffer_weight_sum = 0;
        for (int c = 0; c < 3; ++c) { gb[21].n_sum[c] = 0; gb[22].ns_sum[c] = 0; gb[23].var_n[c] = c; gb[24].var_mean[c] = 0; }
        gb[25].dzdx_sum = -3.25f; gb[25].dzdy_sum = -0.f;
        gb[26].p_sum[1] = std::numeric_limits<float>::quiet_NaN();
        gb[27].var_s[0] = 1e30f; gb[27].var_mean[0] = 1e-20f;   // an unclamped channel above the half range
        gb[28].n_sum[0] = 1e-30f; gb[28].n_sum[1] = gb[28].n_sum[2] = 0;   // squared length underflows to 0
        std::vector<float> ref, dev(develop::GBUFFER_CHANNELS * n);
        GBufferFilmImage(F, film.data(), gb.data(), w, h, save != 0, &names, &ref);
        count = 0;
        for (size_t i = 0; i < n; ++i) count += develop::DevelopGBuffer(M, &film[4 * i], gb[i], save != 0, &dev[develop::GBUFFER_CHANNELS * i]);
        if (!SameBits("gbuffer", ref, dev, develop::GBUFFER_CHANNELS)) return 1;
        // pixels 1 and 2: R G B, and the albedo of pixel 2 (0 / weight 0 stays 0: not NaN); pixel 26: P.Y
        if (count != 3 * nanPixels + 1) { fprintf(stderr, "gbuffer: %zu NaN values counted, %zu constructed\n", count, 3 * nanPixels + 1); return 1; }
        printf("savefp16 %d: rgb %zu pixels, spectral %zu films of %zu bucket slots (%zu probe values), gbuffer %zu pixels: no difference\n", save, n, rounds,
               n * nb, probes.size(), n);
    }
    return 0;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "round") {
        int threads = argc > 2 ? atoi(argv[2]) : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
        return CheckRound(std::max(1, threads));
    }
    if (mode == "arrays") return CheckArrays();
    fprintf(stderr, "usage: film_develop_check round [threads] | arrays\n");
    return 2;
}
