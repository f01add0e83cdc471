// wf_results.hip — libwfhip.so: what a caller reads back (include/wf_abi.h), host code only: the film's download / upload / device-pointer /
// develop / gather calls, the statistics, the profile and counter calls, the debug words and the queues.  No kernel lives here (the
// film develop's are behind the launchers of wf_film_develop.hip), so an edit here leaves every device code object as it was.
// (A .hip unit like wf_boundary.hip; its device pass has nothing to emit.)
#include "wf_ctx.h"

extern "C" {

int wf_film_download(wf_ctx *ctx, double *dst) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    HIPCHK(hipMemcpyAsync(dst, ctx->ws.film, (size_t)ctx->W * ctx->H * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int wf_film_spectral_download(wf_ctx *ctx, double *dst) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    if (!ctx->ws.filmSpectral) return fail(-1, "wf_film_spectral_download: the scene's film is not a spectral film");
    HIPCHK(hipMemcpyAsync(dst, ctx->ws.filmSpectral, (size_t)ctx->W * ctx->H * 2 * ctx->svHost.film.n_buckets * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int wf_film_gbuffer_download(wf_ctx *ctx, wf_gbuffer_pixel *dst) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    if (!ctx->ws.filmGBuffer) return fail(-1, "wf_film_gbuffer_download: the scene's film is not a gbuffer film");
    HIPCHK(hipMemcpyAsync(dst, ctx->ws.filmGBuffer, (size_t)ctx->W * ctx->H * sizeof(wf_gbuffer_pixel), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int wf_film_upload(wf_ctx *ctx, const double *src) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    HIPCHK(hipMemcpyAsync(ctx->ws.film, src, (size_t)ctx->W * ctx->H * 4 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int wf_film_device_ptr(wf_ctx *ctx, void **dptr, uint64_t *nbytes) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    *dptr = ctx->ws.film;
    *nbytes = (uint64_t)ctx->W * ctx->H * 4 * sizeof(double);
    return 0;
}
// device-to-device copies of the film accumulators, for the multi-GPU film reduce: the caller owns a
// device buffer of wf_film_device_ptr's size (e.g. a torch tensor handed to RCCL)
int wf_film_copy_to_device(wf_ctx *ctx, void *dst_device) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    HIPCHK(hipMemcpyAsync(dst_device, ctx->ws.film, (size_t)ctx->W * ctx->H * 4 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int wf_film_copy_from_device(wf_ctx *ctx, const void *src_device) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    HIPCHK(hipMemcpyAsync(ctx->ws.film, src_device, (size_t)ctx->W * ctx->H * 4 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
// The mirrors of the two downloads above: checkpoint / restore of a spectral or GBuffer film
int wf_film_spectral_upload(wf_ctx *ctx, const double *src) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    if (!ctx->ws.filmSpectral) return fail(-1, "wf_film_spectral_upload: the scene's film is not a spectral film");
    if (!src) return fail(-1, "wf_film_spectral_upload: null argument");
    HIPCHK(hipMemcpyAsync(ctx->ws.filmSpectral, src, (size_t)ctx->W * ctx->H * 2 * ctx->svHost.film.n_buckets * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int wf_film_gbuffer_upload(wf_ctx *ctx, const wf_gbuffer_pixel *src) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    if (!ctx->ws.filmGBuffer) return fail(-1, "wf_film_gbuffer_upload: the scene's film is not a gbuffer film");
    if (!src) return fail(-1, "wf_film_gbuffer_upload: null argument");
    HIPCHK(hipMemcpyAsync(ctx->ws.filmGBuffer, src, (size_t)ctx->W * ctx->H * sizeof(wf_gbuffer_pixel), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// The film's GetImage step on the device (kernels and launchers: wf_film_develop.hip)
static int FilmChannelCount(const wf_ctx *ctx) {
    return ctx->ws.filmSpectral ? 3 + ctx->svHost.film.n_buckets : ctx->ws.filmGBuffer ? develop::GBUFFER_CHANNELS : 3;
}
int wf_film_channel_count(wf_ctx *ctx, int *n) {
    if (!ctx || !n) return fail(-1, "wf_film_channel_count: null argument");
    if (!ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    *n = FilmChannelCount(ctx);
    return 0;
}
static int FilmDevelop(wf_ctx *ctx, const char *what, bool rgbOnly, float *dst, uint64_t dstFloats, int saveFP16, uint64_t *nanValues) {
    if (!ctx || !dst) return fail(-1, "%s: null argument", what);
    if (!ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    const size_t pixels = (size_t)ctx->W * ctx->H;
    const int nc = rgbOnly ? 3 : FilmChannelCount(ctx);
    if (dstFloats != (uint64_t)pixels * nc)
        return fail(-1, "%s: dst_floats is %llu, the image holds %d x %d x %d = %llu floats", what, (unsigned long long)dstFloats, ctx->H, ctx->W, nc,
                    (unsigned long long)((uint64_t)pixels * nc));
    if (nanValues) {
        if (!ctx->developNaN) { if (int e = devAlloc(ctx, &ctx->developNaN, (size_t)1)) return e; }
        HIPCHK(hipMemsetAsync(ctx->developNaN, 0, sizeof(unsigned long long), ctx->stream));
    }
    unsigned long long *counter = nanValues ? ctx->developNaN : nullptr;
    const wf_film &F = ctx->svHost.film;
    int e;
    if (!rgbOnly && ctx->ws.filmSpectral) e = develop::LaunchDevelopSpectral(ctx->stream, ctx->ws.film, ctx->ws.filmSpectral, pixels, F, saveFP16 != 0, dst, counter);
    else if (!rgbOnly && ctx->ws.filmGBuffer) e = develop::LaunchDevelopGBuffer(ctx->stream, ctx->ws.film, ctx->ws.filmGBuffer, pixels, F, saveFP16 != 0, dst, counter);
    else e = develop::LaunchDevelopRGB(ctx->stream, ctx->ws.film, pixels, F, saveFP16 != 0, dst, counter);
    if (e) return fail(e, "%s: the launch failed: %s", what, hipGetErrorString((hipError_t)e));
    if (nanValues) {
        unsigned long long count = 0;
        HIPCHK(hipMemcpyAsync(&count, ctx->developNaN, sizeof(count), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        *nanValues = count;
    }
    return 0;
}
int wf_film_develop_device(wf_ctx *ctx, float *dst_device, uint64_t dst_floats, int save_fp16, uint64_t *nan_values) {
    return FilmDevelop(ctx, "wf_film_develop_device", false, dst_device, dst_floats, save_fp16, nan_values);
}
int wf_film_develop_rgb_device(wf_ctx *ctx, float *dst_device, uint64_t dst_floats, int save_fp16, uint64_t *nan_values) {
    return FilmDevelop(ctx, "wf_film_develop_rgb_device", true, dst_device, dst_floats, save_fp16, nan_values);
}
// The gather of a strip-partitioned render (wf_set_strips) without a host round trip or a collective: the scanline strips `src` owns
// are copied from its film into `dst`'s film — peer to peer over xGMI when the contexts sit on different devices, device to device on
// one.  A strip is `height` whole scanlines = one contiguous range of the [H][W][4] double film; a rank of N moves 1/N of the film
// (the reduce(SUM) of full films it replaces moved N x the film, mostly zeros: VERDICT r3).  Both contexts must hold the same scene and
// be idle (wf_sync'ed); the copies run on dst's stream and are synchronised before returning.
int wf_film_gather_strips(wf_ctx *dst, wf_ctx *src) {
    if (!dst || !src || !dst->sceneLoaded || !src->sceneLoaded) return fail(-1, "wf_film_gather_strips: no scene uploaded");
    if (dst->W != src->W || dst->H != src->H) return fail(-1, "wf_film_gather_strips: the films differ in size");
    if (dst == src) return 0;
    useDevice(dst);
    const int count = src->ws.stripCount > 1 ? src->ws.stripCount : 1, rank = count > 1 ? src->ws.stripRank : 0, height = count > 1 ? src->ws.stripHeight : src->H;
    const size_t rowBytes = (size_t)src->W * 4 * sizeof(double);
    if (dst->device != src->device) {
        int can = 0;
        (void)hipDeviceCanAccessPeer(&can, dst->device, src->device);
        if (can) { hipError_t e = hipDeviceEnablePeerAccess(src->device, 0); if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError(); else (void)hipGetLastError(); }
    }
    for (int y0 = 0; y0 < src->H; y0 += height) {
        if ((y0 / height) % count != rank) continue;
        const int rows = y0 + height <= src->H ? height : src->H - y0;
        char *d = reinterpret_cast<char *>(dst->ws.film) + (size_t)y0 * rowBytes;
        const char *sp = reinterpret_cast<const char *>(src->ws.film) + (size_t)y0 * rowBytes;
        if (dst->device == src->device) HIPCHK(hipMemcpyAsync(d, sp, rows * rowBytes, hipMemcpyDeviceToDevice, dst->stream));
        else HIPCHK(hipMemcpyPeerAsync(d, dst->device, sp, src->device, rows * rowBytes, dst->stream));
    }
    HIPCHK(hipStreamSynchronize(dst->stream));
    return 0;
}
// the ray counters of another context added to this one's (the statistics of a multi-device render, summed on the gathering context)
int wf_stats_add(wf_ctx *dst, wf_ctx *src) {
    if (!dst || !src || !dst->sceneLoaded || !src->sceneLoaded) return fail(-1, "wf_stats_add: no scene uploaded");
    unsigned long long a[STAT_COUNT], b[STAT_COUNT];   // the ray counts and the item counters behind them
    useDevice(src);
    HIPCHK(hipMemcpy(b, src->ws.stats, sizeof(b), hipMemcpyDeviceToHost));
    useDevice(dst);
    HIPCHK(hipMemcpy(a, dst->ws.stats, sizeof(a), hipMemcpyDeviceToHost));
    for (int i = 0; i < STAT_COUNT; ++i) a[i] += b[i];
    HIPCHK(hipMemcpy(dst->ws.stats, a, sizeof(a), hipMemcpyHostToDevice));
    useDevice(src);
    HIPCHK(hipMemset(src->ws.stats, 0, sizeof(b)));   // (moved, not copied: a second call adds only what src counted since)
    useDevice(dst);
    return 0;
}
// items the material stage evaluated since the last wf_film_clear, per material type (out[0 .. WF_MAT_NTYPES)), and the items of the
// medium-sample stage (out[WF_MAT_NTYPES]): the counts the queues held when they were reset, plus what they hold now
int wf_material_items_download(wf_ctx *ctx, uint64_t out[16]) {
    if (int e = checkReady(ctx)) return e;
    unsigned long long h[STAT_NITEMS];
    std::vector<int32_t> cnt((size_t)CNT_COUNT * CNT_STRIDE);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(h, ctx->ws.stats + STAT_ITEMS, sizeof(h), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cnt.data(), ctx->ws.counters, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < STAT_NITEMS; ++i) out[i] = i <= WF_MAT_NTYPES ? h[i] + (uint64_t)cnt[(size_t)(CNT_MAT0 + i) * CNT_STRIDE] : 0;
    return 0;
}
int wf_stats_download(wf_ctx *ctx, wf_render_stats *out) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    unsigned long long h[STAT_ITEMS];
    HIPCHK(hipMemcpyAsync(h, ctx->ws.stats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    out->camera_rays = h[STAT_CAMERA];
    for (int i = 0; i < STAT_DEPTHS; ++i) { out->indirect_rays[i] = h[STAT_INDIRECT + i]; out->shadow_rays[i] = h[STAT_SHADOW + i]; }
    return 0;
}

int wf_profile_enable(wf_ctx *ctx, int enabled) {
    if (!ctx) return fail(-1, "null context");
    ctx->profile = enabled;
    return 0;
}
// total milliseconds and launch count of the named kernel since the last report (drains nothing)
int wf_kernel_time_ms(wf_ctx *ctx, const char *name, double *total_ms, int *launches) {
    if (!ctx || !name) return fail(-1, "null argument");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    double sum = 0;
    int n = 0;
    for (auto &e : ctx->events)
        if (e.name == name) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, e.a, e.b));
            sum += ms;
            ++n;
        }
    if (total_ms) *total_ms = sum;
    if (launches) *launches = n;
    return 0;
}
int wf_profile_report(wf_ctx *ctx, wf_kernel_profile_entry *entries, int max_entries, int *n_out) {
    if (!ctx) return fail(-1, "null context");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::map<std::string, wf_kernel_profile_entry> agg;
    std::vector<std::string> order;
    for (auto &e : ctx->events) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e.a, e.b));
        auto it = agg.find(e.name);
        if (it == agg.end()) {
            wf_kernel_profile_entry pe{};
            snprintf(pe.name, sizeof(pe.name), "%s", e.name.c_str());
            pe.launches = 1; pe.total_ms = pe.min_ms = pe.max_ms = ms;
            agg[e.name] = pe;
            order.push_back(e.name);
        } else {
            it->second.launches++;
            it->second.total_ms += ms;
            if (ms < it->second.min_ms) it->second.min_ms = ms;
            if (ms > it->second.max_ms) it->second.max_ms = ms;
        }
        ctx->eventPool.push_back(e.a);
        ctx->eventPool.push_back(e.b);
    }
    ctx->events.clear();
    int n = 0;
    for (auto &name : order) {
        if (n >= max_entries) break;
        entries[n++] = agg[name];
    }
    if (n_out) *n_out = n;
    return 0;
}

int wf_counters_enable(wf_ctx *ctx, int enabled) {
    if (!ctx) return fail(-1, "null context");
    ctx->countTraversal = enabled != 0;
    return 0;
}
int wf_counters_download(wf_ctx *ctx, wf_traversal_counters *out) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    unsigned long long h[8];
    HIPCHK(hipMemcpyAsync(h, ctx->ws.trav, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    out->closest_rays = h[0]; out->closest_nodes = h[1]; out->closest_tris = h[2]; out->closest_hits = h[3];
    out->shadow_rays = h[4]; out->shadow_nodes = h[5]; out->shadow_tris = h[6]; out->shadow_unoccluded = h[7];
    return 0;
}
int wf_debug_counters(wf_ctx *ctx, uint64_t out[4], int reset) {
    if (!ctx || !ctx->sceneLoaded || !out) return fail(-1, "wf_debug_counters: no scene uploaded");
    int h[4] = {0, 0, 0, 0};
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(h, ctx->dbgWords, sizeof(h), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out[i] = (uint64_t)(unsigned)h[i];
    if (reset) HIPCHK(hipMemset(ctx->dbgWords, 0, sizeof(h)));
    return 0;
}
int wf_queue_size(wf_ctx *ctx, const char *queue, int *size) {
    if (int e = checkReady(ctx)) return e;
    static const std::map<std::string, int> idx = {{"ray0", CNT_RAY0}, {"ray1", CNT_RAY1}, {"escaped", CNT_ESCAPED}, {"hitlight", CNT_HITLIGHT},
                                                   {"shadow", CNT_SHADOW}, {"retrace", CNT_RETRACE}, {"mat_diffuse", CNT_MAT0 + WF_MAT_DIFFUSE},
                                                   {"mat_conductor", CNT_MAT0 + WF_MAT_CONDUCTOR}, {"mat_dielectric", CNT_MAT0 + WF_MAT_DIELECTRIC},
                                                   {"mat_thindielectric", CNT_MAT0 + WF_MAT_THIN_DIELECTRIC},
                                                   {"mat_diffusetransmission", CNT_MAT0 + WF_MAT_DIFFUSE_TRANSMISSION},
                                                   {"mat_coateddiffuse", CNT_MAT0 + WF_MAT_COATED_DIFFUSE},
                                                   {"mat_coatedconductor", CNT_MAT0 + WF_MAT_COATED_CONDUCTOR}};
    auto it = idx.find(queue ? queue : "");
    if (it == idx.end()) return fail(-1, "unknown queue \"%s\"", queue ? queue : "(null)");
    HIPCHK(hipMemcpyAsync(size, ctx->ws.counters + it->second * CNT_STRIDE, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int wf_queue_download(wf_ctx *ctx, const char *queue, const char *member, void *dst, uint64_t nbytes) {
    if (int e = checkReady(ctx)) return e;
    const WorkState &ws = ctx->ws;
    std::string q = queue ? queue : "", m = member ? member : "";
    const void *src = nullptr;
    auto rayMember = [&](const RayQueueV &r) -> const void * {
        if (m == "o") return r.o; if (m == "d") return r.d; if (m == "beta") return r.beta; if (m == "r_u") return r.r_u;
        if (m == "r_l") return r.r_l; if (m == "ctx0") return r.ctx0; if (m == "ctx1") return r.ctx1; if (m == "ctx2") return r.ctx2;
        if (m == "meta") return r.meta;
        return nullptr;
    };
    if (q == "ray0") src = rayMember(ws.rq[0]);
    else if (q == "ray1") src = rayMember(ws.rq[1]);
    else if (q == "pixel") {
        if (m == "L") src = ws.L; else if (m == "lambda") src = ws.lambda; else if (m == "lambda_pdf") src = ws.lambdaPdf;
        else if (m == "pPixel") src = ws.pPixel; else if (m == "filterWeight") src = ws.filterWeight;
        else if (m == "cameraRayWeight") src = ws.cameraRayWeight; else if (m == "samples0") src = ws.samples0; else if (m == "samples1") src = ws.samples1;
    } else if (q == "hit") src = ws.hit;
    else if (q == "shadow") {
        if (m == "o") src = ws.sq.o; else if (m == "d") src = ws.sq.d; else if (m == "Ld") src = ws.sq.Ld;
        else if (m == "r_u") src = ws.sq.r_u; else if (m == "r_l") src = ws.sq.r_l;
    }
    if (!src) return fail(-1, "unknown queue member \"%s\".\"%s\"", q.c_str(), m.c_str());
    HIPCHK(hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
