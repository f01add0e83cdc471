// wf_boundary.hip — libwfhip.so: the boundary calls of include/wf_abi.h, host code only.  A caller's rays, hit records, segments and film
// samples, in device buffers (wf_*_device) or host arrays (wf_trace_*_host), through the walks and stages of the uploaded scene, and the
// plain device-memory calls.  No kernel lives here: the walks are wf_backend.hip's, launched through the pointers PickWalkKernels /
// PickStageKernels left in the context (ctx->walk, ctx->stage), and the boundary's own kernels are behind the launchers of
// wf_boundary_intr.hip, wf_film_add.hip, wf_boundary_light.hip, wf_boundary_bsdf.hip and wf_boundary_medium.hip — so an edit to a call's argument checks leaves every device code object as it was.
// (A .hip unit for the LAUNCH* macros of wf_ctx.h; its device pass has nothing to emit.)
#include "wf_ctx.h"
#include "wf_boundary_bsdf.h"
#include "wf_boundary_medium.h"
#include "wf_media.h"

extern "C" {

int wf_trace_closest_device(wf_ctx *ctx, int n, const float *rays7, wf_hit_record *out) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    if (ctx->svHost.haveAnimated) return fail(-1, "%s: the scene has animated primitives — a ray needs its time (wf_trace_closest_device_t / wf_trace_any_device_t)", __func__);
    useDevice(ctx);
    if (n <= 0) return 0;
    if (!ctx->plan.fastOk) { LAUNCH("trace closest (device rays)", ctx->stage.traceClosestRef, gridFor(n), ctx->svHost, n, rays7, 7, out, ctx->stackSpill, 0); return 0; }
    LAUNCHT("trace closest fast (device rays)", ctx->walk.traceClosest, ctx->walk.grid, ctx->svHost, ctx->fast, n, rays7, out, ctx->spillArea());
    // (the variants that do not resolve their near ties inside the walk mark them: re-traced in reference order)
    if (!RetraceInline(ctx->plan.genMode)) LAUNCH("trace closest (near-tie re-trace)", ctx->stage.traceClosestRef, gridFor(n), ctx->svHost, n, rays7, 7, out, ctx->stackSpill, TRACE_ONLY_MARKED);
    return 0;
}
int wf_trace_any_device(wf_ctx *ctx, int n, const float *rays7, int32_t *occluded) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    if (ctx->svHost.haveAnimated) return fail(-1, "%s: the scene has animated primitives — a ray needs its time (wf_trace_closest_device_t / wf_trace_any_device_t)", __func__);
    useDevice(ctx);
    if (n <= 0) return 0;
    if (!ctx->plan.fastOk) { LAUNCH("trace any (device rays)", ctx->stage.traceAnyRef, gridFor(n), ctx->svHost, n, rays7, 7, occluded, (int32_t *)nullptr, (int32_t *)nullptr, ctx->stackSpill); return 0; }
    LAUNCHT("trace any fast (device rays)", ctx->walk.traceAny, ctx->walk.grid, ctx->svHost, ctx->fast, n, rays7, occluded, ctx->spillArea());
    return 0;
}
// The transmittance launch of the HOST-ARRAY boundary calls (wf_trace_shadow_tr_host / _host_t) over their scratch WorkState `ws` of n
// items: one loop per lane, whatever the scene's plan routes the render through — the independent witness the device-buffer call is
// compared with, hence a rule of its own and not LaunchTransmittance's.  timed: the items carry times (ws.pathTime), read by the reference-order
// walk's ANIM variant on any scene; otherwise the per-lane production walk where there is one (one-level fastOk scenes; never its MLEAN variant), else the reference-order walk.
static int LaunchHostTr(wf_ctx *ctx, const WorkState &ws, int n, bool timed) {
    if (timed) LAUNCH("shadow Tr (host rays, timed)", ctx->stage.shadowTr[1], gridFor(n), ctx->svHost, ws, ctx->stackSpill);
    else if (ctx->plan.fastOk && ctx->svHost.nInstances == 0) LAUNCHT("shadow Tr (host rays)", ctx->stage.shadowTrFastWitness, ctx->walk.grid, ctx->svHost, ws, ctx->fast, ctx->spillArea());
    else LAUNCH("shadow Tr (host rays)", ctx->stage.shadowTr[0], gridFor(n), ctx->svHost, ws, ctx->stackSpill);
    return 0;
}
// The two calls above with the rays' TIMES (rays8), on any scene: the walk is chosen by what the scene is.
//   static                  the walks of the untimed calls, reading eight floats per ray (the time is ignored)
//   plan.animFast           the production walks' ANIM variants (walk.traceClosest8 / traceAny8)
//   any other animated one  the reference-order walks of wf_trace_*_host_t, on the caller's buffers
// The records carry no visit counts on any of them.
static int TraceDeviceTimed(wf_ctx *ctx, const char *fn, int n, const float *rays8, wf_hit_record *hits, int32_t *occluded) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "%s: no scene uploaded", fn);
    if (n <= 0) return 0;
    if (!rays8) return fail(-1, "%s: null rays8", fn);
    if (!hits && !occluded) return fail(-1, "%s: null output buffer", fn);
    if (!Aligned16(rays8)) return fail(-1, "%s: rays8 is not aligned to 16 bytes (a ray is read as two 16-byte loads)", fn);
    useDevice(ctx);
    const float *times = rays8 + 7;
    if (ctx->svHost.haveAnimated && !ctx->plan.animFast) {
        if (hits) LAUNCH("trace closest (device rays, timed)", ctx->stage.traceClosestTimed, gridFor(n), ctx->svHost, n, rays8, 8, times, 8, hits, ctx->stackSpill, 0);
        else LAUNCH("trace any (device rays, timed)", ctx->stage.traceAnyTimed, gridFor(n), ctx->svHost, n, rays8, 8, times, 8, occluded, ctx->stackSpill);
    } else if (ctx->svHost.haveAnimated) {
        if (hits) LAUNCHT("trace closest fast (device rays, timed)", ctx->walk.traceClosest8, ctx->walk.grid, ctx->svHost, ctx->fast, n, rays8, hits, ctx->spillArea());
        else LAUNCHT("trace any fast (device rays, timed)", ctx->walk.traceAny8, ctx->walk.grid, ctx->svHost, ctx->fast, n, rays8, occluded, ctx->spillArea());
    } else if (!ctx->plan.fastOk) {
        if (hits) LAUNCH("trace closest (device rays, static)", ctx->stage.traceClosestRef, gridFor(n), ctx->svHost, n, rays8, 8, hits, ctx->stackSpill, TRACE_NO_COUNTS);
        else LAUNCH("trace any (device rays, static)", ctx->stage.traceAnyRef, gridFor(n), ctx->svHost, n, rays8, 8, occluded, (int32_t *)nullptr, (int32_t *)nullptr, ctx->stackSpill);
    } else if (hits) {
        LAUNCHT("trace closest fast (device rays, static)", ctx->walk.traceClosest8, ctx->walk.grid, ctx->svHost, ctx->fast, n, rays8, hits, ctx->spillArea());
        if (!RetraceInline(ctx->plan.genMode)) LAUNCH("trace closest (near-tie re-trace)", ctx->stage.traceClosestRef, gridFor(n), ctx->svHost, n, rays8, 8, hits, ctx->stackSpill, TRACE_ONLY_MARKED);
    } else LAUNCHT("trace any fast (device rays, static)", ctx->walk.traceAny8, ctx->walk.grid, ctx->svHost, ctx->fast, n, rays8, occluded, ctx->spillArea());
    return 0;
}
int wf_trace_closest_device_t(wf_ctx *ctx, int n, const float *rays8, wf_hit_record *out) {
    if (ctx && n > 0 && !out) return fail(-1, "wf_trace_closest_device_t: null out");
    return TraceDeviceTimed(ctx, "wf_trace_closest_device_t", n, rays8, out, nullptr);
}
int wf_trace_any_device_t(wf_ctx *ctx, int n, const float *rays8, int32_t *occluded) {
    if (ctx && n > 0 && !occluded) return fail(-1, "wf_trace_any_device_t: null occluded");
    return TraceDeviceTimed(ctx, "wf_trace_any_device_t", n, rays8, nullptr, occluded);
}
// The hit records of wf_trace_closest_device_t as SurfaceInteractions, and the scene's camera rays as rays8 (kernels and launchers:
// wf_boundary_intr.hip).  Everything is checked before anything is launched.
int wf_hit_interaction_device(wf_ctx *ctx, int n, const float *rays8, const wf_hit_record *hits, float *out_f, int32_t *out_i) {
    const char *fn = "wf_hit_interaction_device";
    if (!ctx) return fail(-1, "%s: null context", fn);
    if (!ctx->sceneLoaded) return fail(-1, "%s: no scene uploaded", fn);
    if (n <= 0) return 0;
    if (n > (1 << 30)) return fail(-1, "%s: n = %d is more than 2^30 items", fn, n);
    if (!rays8 || !hits || !out_f || !out_i) return fail(-1, "%s: null %s", fn, !rays8 ? "rays8" : !hits ? "hits" : !out_f ? "out_f" : "out_i");
    if (!Aligned16(rays8) || !Aligned16(hits) || !Aligned16(out_f) || !Aligned16(out_i))
        return fail(-1, "%s: %s is not aligned to 16 bytes (rays, records and planes are read and written 16 bytes at a time)", fn,
                    !Aligned16(rays8) ? "rays8" : !Aligned16(hits) ? "hits" : !Aligned16(out_f) ? "out_f" : "out_i");
    useDevice(ctx);
    Prof prof_(ctx, "Hit interaction (device records)");
    const int e = boundary::LaunchHitInteraction(ctx->stream, ctx->plan.intrVariant, ctx->svDev, n, rays8, hits, out_f, out_i);
    if (e) return fail(e, "%s: the launch failed: %s", fn, e < 0 ? "the library holds no kernel for the scene's intr_variant" : hipGetErrorString((hipError_t)e));
    return 0;
}
// wf_camera_rays_device, and with the three weight arrays wf_camera_samples_device (all of them or none): one set of checks, one pass state
static int CameraRaysDevice(wf_ctx *ctx, const char *fn, bool weights, int y0, int sample_index, int n_max, float *rays8, int32_t *pixel_xy, float *lambda4,
                            float *lambda_pdf4, float *camera_weight4, float *filter_weight, int32_t *n_out_device) {
    if (!ctx) return fail(-1, "%s: null context", fn);
    if (!ctx->sceneLoaded) return fail(-1, "%s: no scene uploaded", fn);
    if (!ctx->queuesAllocated) return fail(-1, "%s: queues not allocated (wf_queues_alloc)", fn);
    if (!rays8 || !pixel_xy || !lambda4 || !n_out_device)
        return fail(-1, "%s: null %s", fn, !rays8 ? "rays8" : !pixel_xy ? "pixel_xy" : !lambda4 ? "lambda4" : "n_out_device");
    if (weights && (!lambda_pdf4 || !camera_weight4 || !filter_weight))
        return fail(-1, "%s: null %s", fn, !lambda_pdf4 ? "lambda_pdf4" : !camera_weight4 ? "camera_weight4" : "filter_weight");
    if (!Aligned16(rays8) || !Aligned16(lambda4) || ((uintptr_t)pixel_xy & 7u) || ((uintptr_t)n_out_device & 3u))
        return fail(-1, "%s: misaligned buffer (rays8 and lambda4: 16 bytes, pixel_xy: 8, n_out_device: 4)", fn);
    if (weights && (!Aligned16(lambda_pdf4) || !Aligned16(camera_weight4) || ((uintptr_t)filter_weight & 3u)))
        return fail(-1, "%s: misaligned buffer (lambda_pdf4 and camera_weight4: 16 bytes, filter_weight: 4)", fn);
    if (n_max < ctx->ws.pixelsPerPass) return fail(-1, "%s: n_max = %d, a band holds up to %d rays", fn, n_max, ctx->ws.pixelsPerPass);
    if (sample_index < 0) return fail(-1, "%s: sample_index %d", fn, sample_index);
    // one sample index per call, whatever the last render's passes carried: the pass state is the call's own for its launches and is
    // put back afterwards (the kernels have taken their copy of it as an argument by then)
    const int step = ctx->passStep, samples = ctx->passSamples, slotStride = ctx->ws.slotStride, passY0 = ctx->passY0;
    ctx->passStep = 1; ctx->passSamples = 1; ctx->ws.slotStride = ctx->pixelMajor ? 1 : 0;
    int e = GenCameraRays(ctx, y0, sample_index, false);
    if (!e) {
        Prof prof_(ctx, weights ? "Pack camera samples (device buffers)" : "Pack camera rays (device buffers)");
        e = weights ? boundary::LaunchPackCameraSamples(ctx->stream, ctx->ws, n_max, rays8, pixel_xy, lambda4, lambda_pdf4, camera_weight4, filter_weight, n_out_device)
                    : boundary::LaunchPackCameraRays(ctx->stream, ctx->ws, n_max, rays8, pixel_xy, lambda4, n_out_device);
        if (e) e = fail(e, "%s: the launch failed: %s", fn, hipGetErrorString((hipError_t)e));
    }
    ctx->passStep = step; ctx->passSamples = samples; ctx->ws.slotStride = slotStride; ctx->passY0 = passY0;
    return e;
}
int wf_camera_rays_device(wf_ctx *ctx, int y0, int sample_index, int n_max, float *rays8, int32_t *pixel_xy, float *lambda4, int32_t *n_out_device) {
    return CameraRaysDevice(ctx, "wf_camera_rays_device", false, y0, sample_index, n_max, rays8, pixel_xy, lambda4, nullptr, nullptr, nullptr, n_out_device);
}
int wf_camera_samples_device(wf_ctx *ctx, int y0, int sample_index, int n_max, float *rays8, int32_t *pixel_xy, float *lambda4, float *lambda_pdf4,
                             float *camera_weight4, float *filter_weight, int32_t *n_out_device) {
    return CameraRaysDevice(ctx, "wf_camera_samples_device", true, y0, sample_index, n_max, rays8, pixel_xy, lambda4, lambda_pdf4, camera_weight4, filter_weight,
                            n_out_device);
}
// Film::AddSample on a caller's device items (kernel and launcher: wf_film_add.hip).  Everything is checked before anything is launched.
// The stamps (one int32 per film pixel: the epoch of the last call that added to it) are allocated and zeroed by the scene's first call;
// epochs run from 1, and when they are used up the stamps are zeroed again, in stream order.
int wf_film_add_samples_device(wf_ctx *ctx, int n, const int32_t *n_device, const int32_t *pixel_xy, const float *L4, const float *lambda4,
                               const float *lambda_pdf4, const float *filter_weight, uint32_t *rejected_device) {
    const char *fn = "wf_film_add_samples_device";
    if (!ctx) return fail(-1, "%s: null context", fn);
    if (!ctx->sceneLoaded) return fail(-1, "%s: no scene uploaded", fn);
    if (n <= 0) return 0;
    if (!pixel_xy || !L4 || !lambda4 || !lambda_pdf4 || !filter_weight)
        return fail(-1, "%s: null %s", fn, !pixel_xy ? "pixel_xy" : !L4 ? "L4" : !lambda4 ? "lambda4" : !lambda_pdf4 ? "lambda_pdf4" : "filter_weight");
    if (!Aligned16(L4) || !Aligned16(lambda4) || !Aligned16(lambda_pdf4))
        return fail(-1, "%s: %s is not aligned to 16 bytes (an item's four floats are one 16-byte load)", fn, !Aligned16(L4) ? "L4" : !Aligned16(lambda4) ? "lambda4" : "lambda_pdf4");
    if ((uintptr_t)pixel_xy & 7u) return fail(-1, "%s: pixel_xy is not aligned to 8 bytes", fn);
    if (((uintptr_t)filter_weight & 3u) || ((uintptr_t)n_device & 3u) || ((uintptr_t)rejected_device & 3u))
        return fail(-1, "%s: %s is not aligned to 4 bytes", fn, ((uintptr_t)filter_weight & 3u) ? "filter_weight" : ((uintptr_t)n_device & 3u) ? "n_device" : "rejected_device");
    useDevice(ctx);
    const size_t pixels = (size_t)ctx->W * ctx->H;
    if (!ctx->filmStamps) {
        if (int e = devAlloc(ctx, &ctx->filmStamps, pixels)) return e;   // (zeroed on the context's stream)
        ctx->filmEpoch = 0;
    }
    bool clear;
    const int32_t epoch = filmadd::NextEpoch(ctx->filmEpoch, &clear);
    if (clear) HIPCHK(hipMemsetAsync(ctx->filmStamps, 0, pixels * sizeof(int32_t), ctx->stream));
    ctx->filmEpoch = epoch;
    filmadd::Args a{};
    a.film = ctx->ws.film; a.spectral = ctx->ws.filmSpectral; a.stamps = ctx->filmStamps; a.epoch = ctx->filmEpoch;
    a.n = n; a.nDevice = n_device; a.pixelXY = pixel_xy; a.L4 = L4; a.lambda4 = lambda4; a.lambdaPdf4 = lambda_pdf4; a.filterWeight = filter_weight;
    a.rejected = rejected_device;
    Prof prof_(ctx, "Add film samples (device items)");
    const int e = filmadd::LaunchFilmAdd(ctx->stream, ctx->svDev, a);
    if (e) return fail(e, "%s: the launch failed: %s", fn, hipGetErrorString((hipError_t)e));
    return 0;
}
// The scene's lights on a caller's device items (kernels and launchers: wf_boundary_light.hip).  Everything is checked before anything is
// launched; the calls read the uploaded scene and the caller's buffers, nothing of the render's state.
static const char *FirstNull(std::initializer_list<std::pair<const char *, const void *>> ps) {
    for (const auto &p : ps) if (!p.second) return p.first;
    return nullptr;
}
static const char *FirstMisaligned(std::initializer_list<std::pair<const char *, const void *>> ps, uintptr_t mask) {
    for (const auto &p : ps) if ((uintptr_t)p.second & mask) return p.first;
    return nullptr;
}
int wf_light_sample_device(wf_ctx *ctx, int n, const int32_t *n_device, const float *planes_f, const int32_t *planes_i, const float *lambda4, const float *u4,
                           const int32_t *side, float *shadow_rays8, float *L4, float *wi_pdf4, int32_t *light4) {
    const char *fn = "wf_light_sample_device";
    if (!ctx) return fail(-1, "%s: null context", fn);
    if (!ctx->sceneLoaded) return fail(-1, "%s: no scene uploaded", fn);
    if (n < 0) return fail(-1, "%s: n = %d", fn, n);
    if (n == 0) return 0;
    if (n > (1 << 30)) return fail(-1, "%s: n = %d is more than 2^30 items", fn, n);
    if (const char *w = FirstNull({{"planes_f", planes_f}, {"planes_i", planes_i}, {"lambda4", lambda4}, {"u4", u4}, {"shadow_rays8", shadow_rays8}, {"L4", L4},
                                   {"wi_pdf4", wi_pdf4}, {"light4", light4}}))
        return fail(-1, "%s: null %s", fn, w);
    if (const char *w = FirstMisaligned({{"planes_f", planes_f}, {"planes_i", planes_i}, {"lambda4", lambda4}, {"u4", u4}, {"shadow_rays8", shadow_rays8}, {"L4", L4},
                                         {"wi_pdf4", wi_pdf4}, {"light4", light4}}, 15u))
        return fail(-1, "%s: %s is not aligned to 16 bytes (planes and rows are read and written 16 bytes at a time)", fn, w);
    if (const char *w = FirstMisaligned({{"side", side}, {"n_device", n_device}}, 3u)) return fail(-1, "%s: %s is not aligned to 4 bytes", fn, w);
    useDevice(ctx);
    blight::SampleArgs a;
    a.n = n; a.nDevice = n_device; a.planesF = planes_f; a.planesI = planes_i; a.lambda4 = lambda4; a.u4 = u4; a.side = side;
    a.rays8 = shadow_rays8; a.L4 = L4; a.wiPdf4 = wi_pdf4; a.light4 = light4;
    Prof prof_(ctx, "Sample lights (device items)");
    const int e = blight::LaunchLightSample(ctx->stream, ctx->plan.rareLights, ctx->svDev, a);
    if (e) return fail(e, "%s: the launch failed: %s", fn, hipGetErrorString((hipError_t)e));
    return 0;
}
int wf_light_emitted_device(wf_ctx *ctx, int n, const int32_t *n_device, const float *rays8, const float *planes_f, const int32_t *planes_i, const float *lambda4,
                            int infinite_index, const float *prev_planes_f, float *Le4, float *pmf_pdf4) {
    const char *fn = "wf_light_emitted_device";
    if (!ctx) return fail(-1, "%s: null context", fn);
    if (!ctx->sceneLoaded) return fail(-1, "%s: no scene uploaded", fn);
    if (n < 0) return fail(-1, "%s: n = %d", fn, n);
    // (a scene without infinite lights accepts index 0: its misses are black)
    if (infinite_index < 0 || infinite_index >= std::max(1, ctx->plan.nInfiniteLights))
        return fail(-1, "%s: infinite_index %d, the scene has %d infinite lights", fn, infinite_index, ctx->plan.nInfiniteLights);
    if (n == 0) return 0;
    if (n > (1 << 30)) return fail(-1, "%s: n = %d is more than 2^30 items", fn, n);
    if (const char *w = FirstNull({{"rays8", rays8}, {"planes_f", planes_f}, {"planes_i", planes_i}, {"lambda4", lambda4}, {"Le4", Le4}, {"pmf_pdf4", pmf_pdf4}}))
        return fail(-1, "%s: null %s", fn, w);
    if (const char *w = FirstMisaligned({{"rays8", rays8}, {"planes_f", planes_f}, {"planes_i", planes_i}, {"lambda4", lambda4}, {"prev_planes_f", prev_planes_f},
                                         {"Le4", Le4}, {"pmf_pdf4", pmf_pdf4}}, 15u))
        return fail(-1, "%s: %s is not aligned to 16 bytes (rays, planes and rows are read and written 16 bytes at a time)", fn, w);
    if ((uintptr_t)n_device & 3u) return fail(-1, "%s: n_device is not aligned to 4 bytes", fn);
    useDevice(ctx);
    blight::EmittedArgs a;
    a.n = n; a.infiniteIndex = infinite_index; a.nDevice = n_device; a.rays8 = rays8; a.planesF = planes_f; a.planesI = planes_i; a.lambda4 = lambda4;
    a.prevF = prev_planes_f; a.Le4 = Le4; a.pmfPdf4 = pmf_pdf4;
    Prof prof_(ctx, "Emitted radiance (device items)");
    const int e = blight::LaunchLightEmitted(ctx->stream, ctx->plan.emittedVariant, ctx->svDev, a);
    if (e) return fail(e, "%s: the launch failed: %s", fn, e < 0 ? "the library holds no kernel for the scene's light_emitted_variant" : hipGetErrorString((hipError_t)e));
    return 0;
}
// The scene's BSDFs on a caller's device items (kernels and launchers: wf_boundary_bsdf.hip, one code object per material type).
// Everything is checked before anything is launched; the calls read the uploaded scene and the caller's buffers, nothing of the
// render's state.  A call is the type-independent launch (type 0) and then one launch per material type the scene's plan says is present.
using BsdfMakeFn = int (*)(void *, const SceneView *, const bbsdf::MakeArgs *);
using BsdfEvalFn = int (*)(void *, const SceneView *, const bbsdf::EvalArgs *);
static const BsdfMakeFn kBsdfMake[WF_MAT_NTYPES] = {wf_launch_bsdf_make_0, wf_launch_bsdf_make_1, wf_launch_bsdf_make_2, wf_launch_bsdf_make_3,
                                                    wf_launch_bsdf_make_4, wf_launch_bsdf_make_5, wf_launch_bsdf_make_6, wf_launch_bsdf_make_7,
                                                    wf_launch_bsdf_make_8, wf_launch_bsdf_make_9, wf_launch_bsdf_make_10};
static const BsdfEvalFn kBsdfEval[WF_MAT_NTYPES] = {wf_launch_bsdf_eval_0, wf_launch_bsdf_eval_1, wf_launch_bsdf_eval_2, wf_launch_bsdf_eval_3,
                                                    wf_launch_bsdf_eval_4, wf_launch_bsdf_eval_5, wf_launch_bsdf_eval_6, wf_launch_bsdf_eval_7,
                                                    wf_launch_bsdf_eval_8, wf_launch_bsdf_eval_9, wf_launch_bsdf_eval_10};
int wf_bsdf_make_device(wf_ctx *ctx, int n, const int32_t *n_device, const float *rays8, const float *planes_f, const int32_t *planes_i, const float *lambda4,
                        const int32_t *regularize, float *bsdf_rec, int32_t *bsdf4) {
    const char *fn = "wf_bsdf_make_device";
    if (!ctx) return fail(-1, "%s: null context", fn);
    if (!ctx->sceneLoaded) return fail(-1, "%s: no scene uploaded", fn);
    if (n < 0) return fail(-1, "%s: n = %d", fn, n);
    if (n == 0) return 0;
    if (n > (1 << 30)) return fail(-1, "%s: n = %d is more than 2^30 items", fn, n);
    if (const char *w = FirstNull({{"rays8", rays8}, {"planes_f", planes_f}, {"planes_i", planes_i}, {"lambda4", lambda4}, {"bsdf_rec", bsdf_rec}, {"bsdf4", bsdf4}}))
        return fail(-1, "%s: null %s", fn, w);
    if (const char *w = FirstMisaligned({{"rays8", rays8}, {"planes_f", planes_f}, {"planes_i", planes_i}, {"lambda4", lambda4}, {"bsdf_rec", bsdf_rec}, {"bsdf4", bsdf4}}, 15u))
        return fail(-1, "%s: %s is not aligned to 16 bytes (rays, planes, records and rows are read and written 16 bytes at a time)", fn, w);
    if (const char *w = FirstMisaligned({{"regularize", regularize}, {"n_device", n_device}}, 3u)) return fail(-1, "%s: %s is not aligned to 4 bytes", fn, w);
    useDevice(ctx);
    if ((size_t)n > ctx->bsdfRouteCap) {
        // (the outgrown array is not freed here: launches of earlier calls may still read it; it goes with the context)
        const size_t cap = std::max((size_t)n, 2 * ctx->bsdfRouteCap);
        int32_t *route = nullptr;
        if (int e = devAlloc(ctx, &route, cap)) return e;
        ctx->bsdfRoute = route; ctx->bsdfRouteCap = cap;
    }
    bbsdf::MakeArgs a;
    a.n = n; a.nMaterials = ctx->plan.nMaterials; a.cameraAnim = ctx->plan.cameraAnim; a.nDevice = n_device; a.rays8 = rays8; a.planesF = planes_f;
    a.lambda4 = lambda4; a.planesI = planes_i; a.regularize = regularize; a.route = ctx->bsdfRoute; a.rec = bsdf_rec; a.bsdf4 = bsdf4;
    Prof prof_(ctx, "Make BSDFs (device items)");
    for (int t = 0; t < WF_MAT_NTYPES; ++t) {
        if (t != 0 && !ctx->plan.matPresent[t]) continue;
        if (const int e = kBsdfMake[t](ctx->stream, ctx->svDev, &a)) return fail(e, "%s: the launch for material type %d failed: %s", fn, t, hipGetErrorString((hipError_t)e));
    }
    return 0;
}
int wf_bsdf_eval_device(wf_ctx *ctx, int n, const int32_t *n_device, const float *bsdf_rec, const float *planes_f, const int32_t *planes_i, const float *wi4,
                        const float *u4, float *f4, float *pdf4, float *next_rays8, float *sample_f4, float *sample_pdf4, int32_t *sample_i4) {
    const char *fn = "wf_bsdf_eval_device";
    if (!ctx) return fail(-1, "%s: null context", fn);
    if (!ctx->sceneLoaded) return fail(-1, "%s: no scene uploaded", fn);
    if (n < 0) return fail(-1, "%s: n = %d", fn, n);
    if (!wi4 && !u4) return fail(-1, "%s: neither wi4 nor u4 is given", fn);
    if (n == 0) return 0;
    if (n > (1 << 30)) return fail(-1, "%s: n = %d is more than 2^30 items", fn, n);
    if (const char *w = FirstNull({{"bsdf_rec", bsdf_rec}, {"planes_f", planes_f}, {"planes_i", planes_i}})) return fail(-1, "%s: null %s", fn, w);
    if (wi4) if (const char *w = FirstNull({{"f4", f4}, {"pdf4", pdf4}})) return fail(-1, "%s: wi4 is given and %s is null", fn, w);
    if (u4)
        if (const char *w = FirstNull({{"next_rays8", next_rays8}, {"sample_f4", sample_f4}, {"sample_pdf4", sample_pdf4}, {"sample_i4", sample_i4}}))
            return fail(-1, "%s: u4 is given and %s is null", fn, w);
    // (the outputs of an absent half are not written: they are not looked at either)
    if (!wi4) f4 = pdf4 = nullptr;
    if (!u4) { next_rays8 = sample_f4 = sample_pdf4 = nullptr; sample_i4 = nullptr; }
    if (const char *w = FirstMisaligned({{"bsdf_rec", bsdf_rec}, {"planes_f", planes_f}, {"planes_i", planes_i}, {"wi4", wi4}, {"u4", u4}, {"f4", f4}, {"pdf4", pdf4},
                                         {"next_rays8", next_rays8}, {"sample_f4", sample_f4}, {"sample_pdf4", sample_pdf4}, {"sample_i4", sample_i4}}, 15u))
        return fail(-1, "%s: %s is not aligned to 16 bytes (records, planes and rows are read and written 16 bytes at a time)", fn, w);
    if ((uintptr_t)n_device & 3u) return fail(-1, "%s: n_device is not aligned to 4 bytes", fn);
    useDevice(ctx);
    bbsdf::EvalArgs a;
    a.n = n; a.nMaterials = ctx->plan.nMaterials; a.nDevice = n_device; a.rec = bsdf_rec; a.planesF = planes_f; a.planesI = planes_i; a.wi4 = wi4; a.u4 = u4;
    a.f4 = f4; a.pdf4 = pdf4; a.nextRays8 = next_rays8; a.sampleF4 = sample_f4; a.samplePdf4 = sample_pdf4; a.sampleI4 = sample_i4;
    Prof prof_(ctx, "Evaluate BSDFs (device items)");
    for (int t = 0; t < WF_MAT_NTYPES; ++t) {
        if (t != 0 && !ctx->plan.matPresent[t]) continue;
        if (const int e = kBsdfEval[t](ctx->stream, ctx->svDev, &a)) return fail(e, "%s: the launch for material type %d failed: %s", fn, t, hipGetErrorString((hipError_t)e));
    }
    return 0;
}
// The scene's media and phase functions on a caller's device items (include/wf_media.h; kernels and launchers: wf_boundary_medium.hip).
// Everything is checked before anything is launched; the calls read the uploaded scene and the caller's buffers, nothing of the
// render's state.
int wf_medium_sample_device(wf_ctx *ctx, int n, const int32_t *n_device, const float *rays8, const int32_t *medium, const float *lambda4, const float *beta4,
                            const float *r_u4, const float *r_l4, const int32_t *flags, int32_t *event4, float *p_g4, float *out_beta4, float *out_r_u4,
                            float *out_r_l4, float *L4) {
    const char *fn = "wf_medium_sample_device";
    if (!ctx) return fail(-1, "%s: null context", fn);
    if (!ctx->sceneLoaded) return fail(-1, "%s: no scene uploaded", fn);
    if (!ctx->svHost.haveMedia) return fail(-1, "%s: the scene has no media", fn);
    if (n < 0) return fail(-1, "%s: n = %d", fn, n);
    if (n == 0) return 0;
    if (n > (1 << 30)) return fail(-1, "%s: n = %d is more than 2^30 items", fn, n);
    if (const char *w = FirstNull({{"rays8", rays8}, {"medium", medium}, {"lambda4", lambda4}, {"beta4", beta4}, {"r_u4", r_u4}, {"r_l4", r_l4}, {"event4", event4},
                                   {"p_g4", p_g4}, {"out_beta4", out_beta4}, {"out_r_u4", out_r_u4}, {"out_r_l4", out_r_l4}, {"L4", L4}}))
        return fail(-1, "%s: null %s", fn, w);
    if (const char *w = FirstMisaligned({{"rays8", rays8}, {"lambda4", lambda4}, {"beta4", beta4}, {"r_u4", r_u4}, {"r_l4", r_l4}, {"event4", event4}, {"p_g4", p_g4},
                                         {"out_beta4", out_beta4}, {"out_r_u4", out_r_u4}, {"out_r_l4", out_r_l4}, {"L4", L4}}, 15u))
        return fail(-1, "%s: %s is not aligned to 16 bytes (rays and rows are read and written 16 bytes at a time)", fn, w);
    if (const char *w = FirstMisaligned({{"medium", medium}, {"flags", flags}, {"n_device", n_device}}, 3u)) return fail(-1, "%s: %s is not aligned to 4 bytes", fn, w);
    useDevice(ctx);
    bmedium::TrackArgs a;
    a.n = n; a.nMedia = ctx->plan.nMedia; a.nDevice = n_device; a.rays8 = rays8; a.medium = medium; a.lambda4 = lambda4; a.beta4 = beta4; a.ru4 = r_u4; a.rl4 = r_l4;
    a.flags = flags; a.event4 = event4; a.pG4 = p_g4; a.outBeta4 = out_beta4; a.outRu4 = out_r_u4; a.outRl4 = out_r_l4; a.L4 = L4;
    Prof prof_(ctx, "Sample media (device items)");
    const int e = bmedium::LaunchMediumTrack(ctx->stream, ctx->plan.mediumLean, ctx->svDev, a);
    if (e) return fail(e, "%s: the launch failed: %s", fn, hipGetErrorString((hipError_t)e));
    return 0;
}
int wf_phase_device(wf_ctx *ctx, int n, const int32_t *n_device, const float *rays8, const float *p_g4, const float *wi4, const float *u4, float *p_pdf4,
                    float *sample4, float *next_rays8) {
    const char *fn = "wf_phase_device";
    if (!ctx) return fail(-1, "%s: null context", fn);
    if (!ctx->sceneLoaded) return fail(-1, "%s: no scene uploaded", fn);
    if (!ctx->svHost.haveMedia) return fail(-1, "%s: the scene has no media", fn);
    if (n < 0) return fail(-1, "%s: n = %d", fn, n);
    if (!wi4 && !u4) return fail(-1, "%s: neither wi4 nor u4 is given", fn);
    if (n == 0) return 0;
    if (n > (1 << 30)) return fail(-1, "%s: n = %d is more than 2^30 items", fn, n);
    if (const char *w = FirstNull({{"rays8", rays8}, {"p_g4", p_g4}})) return fail(-1, "%s: null %s", fn, w);
    if (wi4 && !p_pdf4) return fail(-1, "%s: wi4 is given and p_pdf4 is null", fn);
    if (u4) if (const char *w = FirstNull({{"sample4", sample4}, {"next_rays8", next_rays8}})) return fail(-1, "%s: u4 is given and %s is null", fn, w);
    // (the outputs of an absent half are not written: they are not looked at either)
    if (!wi4) p_pdf4 = nullptr;
    if (!u4) sample4 = next_rays8 = nullptr;
    if (const char *w = FirstMisaligned({{"rays8", rays8}, {"p_g4", p_g4}, {"wi4", wi4}, {"u4", u4}, {"p_pdf4", p_pdf4}, {"sample4", sample4}, {"next_rays8", next_rays8}}, 15u))
        return fail(-1, "%s: %s is not aligned to 16 bytes (rays and rows are read and written 16 bytes at a time)", fn, w);
    if ((uintptr_t)n_device & 3u) return fail(-1, "%s: n_device is not aligned to 4 bytes", fn);
    useDevice(ctx);
    bmedium::PhaseArgs a;
    a.n = n; a.nDevice = n_device; a.rays8 = rays8; a.pG4 = p_g4; a.wi4 = wi4; a.u4 = u4; a.pPdf4 = p_pdf4; a.sample4 = sample4; a.nextRays8 = next_rays8;
    Prof prof_(ctx, "Phase functions (device items)");
    const int e = bmedium::LaunchPhase(ctx->stream, a);
    if (e) return fail(e, "%s: the launch failed: %s", fn, hipGetErrorString((hipError_t)e));
    return 0;
}
// room for n items in ctx->trScratch, the wavefront's arrays among them if the scene's plan routes through it.  Growth waits for the
// launches that still read the old arrays; a call that fits allocates and waits for nothing.
static int GrowTrScratch(wf_ctx *ctx, size_t n) {
    wf_ctx::TrScratch &t = ctx->trScratch;
    if (!t.counters) {
        HIPCHK(hipMalloc((void **)&t.counters, (size_t)CNT_COUNT * CNT_STRIDE * sizeof(int32_t)));
        HIPCHK(hipMemsetAsync(t.counters, 0, (size_t)CNT_COUNT * CNT_STRIDE * sizeof(int32_t), ctx->stream));
    }
    const bool wavefront = ctx->plan.trRoute == 2;
    if (n <= t.capacity && (!wavefront || t.trO)) return 0;
    const size_t cap = n > t.capacity ? std::max(n, 2 * t.capacity) : t.capacity;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (const wf_ctx::TrScratch::Slot &sl : t.slots()) {
        if (*sl.p) HIPCHK(hipFree(*sl.p));
        *sl.p = nullptr;
    }
    t.capacity = 0;
    for (const wf_ctx::TrScratch::Slot &sl : t.slots())
        if (!sl.wavefront || wavefront) HIPCHK(hipMalloc(sl.p, cap * sl.elem));
    t.capacity = cap;
    return 0;
}
// IntersectShadowTr on the caller's device items: TraceShadowTrHost's scratch WorkState, with the caller's arrays in place of the
// uploaded copies and the rest packed on the device into the context's scratch
int wf_trace_shadow_tr_device(wf_ctx *ctx, int n, const float *rays8, const int32_t *medium, const float *lambda, const float *Ld, const float *r_u,
                              const float *r_l, float *out_L) {
    const char *fn = "wf_trace_shadow_tr_device";
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "%s: no scene uploaded", fn);
    if (!ctx->svHost.haveMedia) return fail(-1, "%s: the scene has no media", fn);
    if (n <= 0) return 0;
    if (!rays8 || !medium || !lambda || !Ld || !r_u || !r_l) return fail(-1, "%s: null input array", fn);
    if (!out_L) return fail(-1, "%s: null out_L", fn);
    if (!Aligned16(rays8)) return fail(-1, "%s: rays8 is not aligned to 16 bytes (a ray is read as two 16-byte loads)", fn);
    if (!Aligned16(lambda) || !Aligned16(Ld) || !Aligned16(r_u) || !Aligned16(r_l) || !Aligned16(out_L))
        return fail(-1, "%s: lambda / Ld / r_u / r_l / out_L are read and written four floats at a time: not aligned to 16 bytes", fn);
    useDevice(ctx);
    if (int e = GrowTrScratch(ctx, (size_t)n)) return e;
    const wf_ctx::TrScratch &t = ctx->trScratch;
    const bool timed = ctx->svHost.haveAnimated;   // (a static scene's items need no times)
    WorkState ws = ctx->ws;   // counters / stats of the context, every per-item array replaced below (the kernels only read the caller's inputs)
    ws.sq.o = t.o; ws.sq.d = t.d; ws.lambdaPdf = t.lambdaPdf;
    ws.sq.Ld = (F4 *)Ld; ws.sq.r_u = (F4 *)r_u; ws.sq.r_l = (F4 *)r_l; ws.sq.medium = (int32_t *)medium;
    ws.lambda = (F4 *)lambda;
    ws.L = (F4 *)out_L;
    ws.counters = t.counters;
    if (timed) ws.pathTime = t.pathTime;
    // (the wavefront's state, queues and hit records: null on the other routes, whose kernels touch none of them)
    ws.trO = t.trO; ws.trD = t.trD; ws.trT = t.trT; ws.trRu = t.trRu; ws.trRl = t.trRl; ws.trRng = t.trRng;
    ws.trQ[0] = t.trQ[0]; ws.trQ[1] = t.trQ[1]; ws.hit = t.hit; ws.hitInst = t.hitInst;
    LAUNCH("shadow Tr (device rays): pack items", ctx->stage.packShadowItems, gridFor(n), n, rays8, t.o, t.d, t.lambdaPdf, timed ? t.pathTime : (float *)nullptr, (F4 *)out_L, t.counters);
    // the scene's planned route, as the render's own stage runs it (route 1 is for static scenes: only route 0's name tells timed items)
    LaunchTransmittance(ctx, ws, n, ctx->plan.trRoute, timed, {"shadow Tr (device rays): reset", "shadow Tr (device rays): begin", "shadow Tr (device rays): trace", "shadow Tr (device rays): segment",
                                                                "shadow Tr (device rays): rest", timed ? "shadow Tr (device rays, timed)" : "shadow Tr (device rays)"});
    return 0;
}
// IntersectOneRandom on the caller's device segments {p0, p1, time}: the kernel of the host-array calls, at the segments' times on a
// scene with animated primitives
int wf_trace_one_random_device(wf_ctx *ctx, int n, const float *segs7, const int32_t *material, wf_hit_record *out, float *reservoir_pdf) {
    const char *fn = "wf_trace_one_random_device";
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "%s: no scene uploaded", fn);
    if (n <= 0) return 0;
    if (!segs7 || !material) return fail(-1, "%s: null input array", fn);
    if (!out || !reservoir_pdf) return fail(-1, "%s: null output buffer", fn);
    useDevice(ctx);
    if (ctx->svHost.haveAnimated) LAUNCH("intersect one random (device segments, timed)", ctx->stage.traceOneRandom[1], gridFor(n), ctx->svHost, n, segs7, 7, material, segs7 + 6, 7, out, reservoir_pdf, ctx->stackSpill);
    else LAUNCH("intersect one random (device segments)", ctx->stage.traceOneRandom[0], gridFor(n), ctx->svHost, n, segs7, 7, material, (const float *)nullptr, 0, out, reservoir_pdf, ctx->stackSpill);
    return 0;
}
int wf_device_alloc(wf_ctx *ctx, uint64_t nbytes, void **dptr) {
    if (!ctx || !dptr) return fail(-1, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMalloc(dptr, nbytes ? nbytes : 1));
    return 0;
}
int wf_device_free(wf_ctx *ctx, void *dptr) {
    if (!ctx) return fail(-1, "null context");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipFree(dptr));
    return 0;
}
int wf_device_upload(wf_ctx *ctx, void *dst_device, const void *src_host, uint64_t nbytes) {
    if (!ctx) return fail(-1, "null context");
    HIPCHK(hipMemcpyAsync(dst_device, src_host, nbytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int wf_device_download(wf_ctx *ctx, void *dst_host, const void *src_device, uint64_t nbytes) {
    if (!ctx) return fail(-1, "null context");
    HIPCHK(hipMemcpyAsync(dst_host, src_device, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int wf_trace_closest_host(wf_ctx *ctx, int n, const float *o, const float *d, const float *tmax, wf_hit_record *out, int count_visits) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    if (ctx->svHost.haveAnimated) return fail(-1, "%s: the scene has animated primitives — a ray needs its time (wf_trace_closest_host_t / wf_trace_any_host_t)", __func__);
    useDevice(ctx);
    if (n <= 0) return 0;
    const std::vector<float> rays = PackRays7(o, d, tmax, n);
    DeviceScratch tmp(ctx->stream);
    float *dr = nullptr;
    wf_hit_record *dh = nullptr;
    int e;
    if ((e = tmp.upload(&dr, rays.data(), rays.size())) || (e = tmp.alloc(&dh, (size_t)n))) return e;
    if (count_visits || !ctx->plan.fastOk) {
        LAUNCH("trace closest (host rays)", ctx->stage.traceClosestRef, gridFor(n), ctx->svHost, n, dr, 7, dh, ctx->stackSpill, 0);
    } else if ((e = wf_trace_closest_device(ctx, n, dr, dh))) return e;
    HIPCHK(hipMemcpyAsync(out, dh, (size_t)n * sizeof(wf_hit_record), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
// IntersectShadowTr on caller-supplied shadow rays: a scratch WorkState over temporary device arrays (one "pixel" per ray) run through
// the same transmittance kernels as the render.  time != nullptr (wf_trace_shadow_tr_host_t): the rays' times are the pixels' path
// times (ws.pathTime) of the reference-order walk's ANIM variant, the render's kernel for scenes with animated primitives.
static int TraceShadowTrHost(wf_ctx *ctx, const char *fn, int n, const float *o, const float *d, const float *tmax, const int32_t *medium, const float *lambda,
                             const float *Ld, const float *r_u, const float *r_l, const float *time, float *out_L) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    if (!ctx->svHost.haveMedia) return fail(-1, "%s: the scene has no media", fn);
    if (ctx->svHost.haveAnimated && !time) return fail(-1, "%s: the scene has animated primitives and this entry point carries no ray times (wf_trace_shadow_tr_host_t)", fn);
    if (n <= 0) return 0;
    std::vector<F4> ho(n), hd(n), hl(n), hp(n, F4{1, 1, 1, 1});
    for (int i = 0; i < n; ++i) {
        ho[i] = F4{o[3 * i], o[3 * i + 1], o[3 * i + 2], tmax[i]};
        hd[i] = F4{d[3 * i], d[3 * i + 1], d[3 * i + 2], BitsToFloat((uint32_t)i)};   // pixelIndex = i
        hl[i] = F4{lambda[4 * i], lambda[4 * i + 1], lambda[4 * i + 2], lambda[4 * i + 3]};
    }
    WorkState ws = ctx->ws;   // counters / stats of the context, every per-item array replaced below
    DeviceScratch tmp(ctx->stream);
    const size_t N = (size_t)n;
    int e;
    int32_t *cnt = nullptr;
    if ((e = tmp.upload(&ws.sq.o, ho.data(), N)) || (e = tmp.upload(&ws.sq.d, hd.data(), N)) || (e = tmp.upload(&ws.sq.Ld, (const void *)Ld, N)) ||
        (e = tmp.upload(&ws.sq.r_u, (const void *)r_u, N)) || (e = tmp.upload(&ws.sq.r_l, (const void *)r_l, N)) || (e = tmp.upload(&ws.sq.medium, medium, N)) ||
        (e = tmp.upload(&ws.lambda, hl.data(), N)) || (e = tmp.upload(&ws.lambdaPdf, hp.data(), N)) || (e = tmp.zeroed(&ws.L, N)) ||
        (e = tmp.zeroed(&cnt, (size_t)CNT_COUNT * CNT_STRIDE)))
        return e;
    HIPCHK(hipMemcpyAsync(cnt + CNT_SHADOW * CNT_STRIDE, &n, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ws.counters = cnt;
    if (time && (e = tmp.upload(&ws.pathTime, time, N))) return e;
    if ((e = LaunchHostTr(ctx, ws, n, time != nullptr))) return e;
    HIPCHK(hipMemcpyAsync(out_L, ws.L, n * sizeof(F4), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int wf_trace_shadow_tr_host(wf_ctx *ctx, int n, const float *o, const float *d, const float *tmax, const int32_t *medium, const float *lambda,
                            const float *Ld, const float *r_u, const float *r_l, float *out_L) {
    return TraceShadowTrHost(ctx, "wf_trace_shadow_tr_host", n, o, d, tmax, medium, lambda, Ld, r_u, r_l, nullptr, out_L);
}
int wf_trace_shadow_tr_host_t(wf_ctx *ctx, int n, const float *o, const float *d, const float *tmax, const int32_t *medium, const float *lambda,
                              const float *Ld, const float *r_u, const float *r_l, const float *time, float *out_L) {
    if (!time) return fail(-1, "wf_trace_shadow_tr_host_t: no ray times");
    return TraceShadowTrHost(ctx, "wf_trace_shadow_tr_host_t", n, o, d, tmax, medium, lambda, Ld, r_u, r_l, time, out_L);
}
// time != nullptr (wf_trace_one_random_host_t): every segment walked at its own time (the render's probes walk at time 0,
// wavefront/subsurface.cpp:70)
static int TraceOneRandomHost(wf_ctx *ctx, int n, const float *p0, const float *p1, const int32_t *material, const float *time, wf_hit_record *out, float *reservoir_pdf) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    // (without times an animated scene is refused instead of answered for the start-time geometry)
    if (ctx->svHost.haveAnimated && !time) return fail(-1, "wf_trace_one_random_host: the scene has animated primitives and this entry point carries no segment times (wf_trace_one_random_host_t)");
    if (n <= 0) return 0;
    std::vector<float> segs((size_t)n * 6);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) { segs[(size_t)i * 6 + k] = p0[3 * i + k]; segs[(size_t)i * 6 + 3 + k] = p1[3 * i + k]; }
    DeviceScratch tmp(ctx->stream);
    float *ds = nullptr, *dp = nullptr, *dt = nullptr;
    int32_t *dm = nullptr;
    wf_hit_record *dh = nullptr;
    int e;
    if ((e = tmp.upload(&ds, segs.data(), segs.size())) || (e = tmp.upload(&dm, material, (size_t)n)) || (e = tmp.alloc(&dh, (size_t)n)) || (e = tmp.alloc(&dp, (size_t)n))) return e;
    if (time) {
        if ((e = tmp.upload(&dt, time, (size_t)n))) return e;
        LAUNCH("intersect one random (host segments, timed)", ctx->stage.traceOneRandom[1], gridFor(n), ctx->svHost, n, ds, 6, dm, (const float *)dt, 1, dh, dp, ctx->stackSpill);
    } else LAUNCH("intersect one random (host segments)", ctx->stage.traceOneRandom[0], gridFor(n), ctx->svHost, n, ds, 6, dm, (const float *)nullptr, 0, dh, dp, ctx->stackSpill);
    HIPCHK(hipMemcpyAsync(out, dh, (size_t)n * sizeof(wf_hit_record), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(reservoir_pdf, dp, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int wf_trace_one_random_host(wf_ctx *ctx, int n, const float *p0, const float *p1, const int32_t *material, wf_hit_record *out, float *reservoir_pdf) {
    return TraceOneRandomHost(ctx, n, p0, p1, material, nullptr, out, reservoir_pdf);
}
int wf_trace_one_random_host_t(wf_ctx *ctx, int n, const float *p0, const float *p1, const int32_t *material, const float *time, wf_hit_record *out, float *reservoir_pdf) {
    if (!time) return fail(-1, "wf_trace_one_random_host_t: no segment times");
    return TraceOneRandomHost(ctx, n, p0, p1, material, time, out, reservoir_pdf);
}
int wf_trace_any_host(wf_ctx *ctx, int n, const float *o, const float *d, const float *tmax, int32_t *occluded, int32_t *nodes_visited, int32_t *tris_tested) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    if (ctx->svHost.haveAnimated) return fail(-1, "%s: the scene has animated primitives — a ray needs its time (wf_trace_closest_host_t / wf_trace_any_host_t)", __func__);
    useDevice(ctx);
    if (n <= 0) return 0;
    const std::vector<float> rays = PackRays7(o, d, tmax, n);
    DeviceScratch tmp(ctx->stream);
    float *dr = nullptr;
    int32_t *dres = nullptr;
    int e;
    if ((e = tmp.upload(&dr, rays.data(), rays.size())) || (e = tmp.alloc(&dres, (size_t)3 * n))) return e;
    if (nodes_visited || tris_tested || !ctx->plan.fastOk) {
        LAUNCH("trace any (host rays)", ctx->stage.traceAnyRef, gridFor(n), ctx->svHost, n, dr, 7, dres, dres + n, dres + 2 * (size_t)n, ctx->stackSpill);
    } else if ((e = wf_trace_any_device(ctx, n, dr, dres))) return e;
    HIPCHK(hipMemcpyAsync(occluded, dres, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (nodes_visited) HIPCHK(hipMemcpyAsync(nodes_visited, dres + n, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (tris_tested) HIPCHK(hipMemcpyAsync(tris_tested, dres + 2 * (size_t)n, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
// IntersectClosest / IntersectShadow on caller-supplied rays WITH their times (the untimed entry points would walk an animated
// scene at its start time): the reference-order walks, interpolating every AnimatedPrimitive's transformation at the ray's time
static int TraceTimed(wf_ctx *ctx, int n, const float *o, const float *d, const float *tmax, const float *time, wf_hit_record *hits, int32_t *occluded) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    if (!o || !d || !tmax || !time) return fail(-1, "wf_trace_*_host_t: null ray arrays");
    useDevice(ctx);
    if (n <= 0) return 0;
    std::vector<float> rays = PackRays7(o, d, tmax, n);
    rays.insert(rays.end(), time, time + n);   // the n times behind the n rays
    DeviceScratch tmp(ctx->stream);
    float *dr = nullptr;
    char *dres = nullptr;
    const size_t resBytes = hits ? (size_t)n * sizeof(wf_hit_record) : (size_t)n * sizeof(int32_t);
    int e;
    if ((e = tmp.upload(&dr, rays.data(), rays.size())) || (e = tmp.alloc(&dres, resBytes))) return e;
    if (hits) LAUNCH("trace closest (host rays with times)", ctx->stage.traceClosestTimed, gridFor(n), ctx->svHost, n, dr, 7, dr + (size_t)n * 7, 1, (wf_hit_record *)dres, ctx->stackSpill, 1);
    else LAUNCH("trace any (host rays with times)", ctx->stage.traceAnyTimed, gridFor(n), ctx->svHost, n, dr, 7, dr + (size_t)n * 7, 1, (int32_t *)dres, ctx->stackSpill);
    HIPCHK(hipMemcpyAsync(hits ? (void *)hits : (void *)occluded, dres, resBytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int wf_trace_closest_host_t(wf_ctx *ctx, int n, const float *o, const float *d, const float *tmax, const float *time, wf_hit_record *out) {
    if (!out) return fail(-1, "wf_trace_closest_host_t: null out");
    return TraceTimed(ctx, n, o, d, tmax, time, out, nullptr);
}
int wf_trace_any_host_t(wf_ctx *ctx, int n, const float *o, const float *d, const float *tmax, const float *time, int32_t *occluded) {
    if (!occluded) return fail(-1, "wf_trace_any_host_t: null occluded");
    return TraceTimed(ctx, n, o, d, tmax, time, nullptr, occluded);
}

}  // extern "C"
