/*
 * wf_media.h — the scene's participating media and phase functions on a caller's DEVICE items (libwfhip.so): the medium half of a
 * volumetric path vertex, computed by the render's own functions.  An addition to wf_abi.h under the same conventions (plain C, 0 or an
 * error code and wf_last_error(), one in-order stream per context); WF_ABI_VERSION is unchanged — nothing of wf_abi.h moved.
 *
 * With wf_trace_closest_device_t, wf_hit_interaction_device, the light and BSDF calls, wf_trace_shadow_tr_device and the film calls of
 * wf_abi.h, a caller writes a VOLUMETRIC path tracer against the render's own scene; every value equals the render's bit for bit.  The
 * loop of one depth, for rays in flight with their media:
 *     hits   = wf_trace_closest_device_t(rays)                         tMax of a row = its hit's t, +infinity for a miss
 *     events = wf_medium_sample_device(rays with that tMax, medium)    kind 1: on to the hit or the escape, as without media
 *                                                                      kind 3: a scatter at p_g4 — wf_light_sample_device on the
 *                                                                      planes of a medium point, wf_phase_device for the light's
 *                                                                      direction and for the next ray, wf_trace_shadow_tr_device
 * Both calls are launched on the context's stream (wf_stream) and NOT synchronised; every argument is checked by name before anything
 * is launched (a null pointer is named; 4-float arrays and rays are aligned to 16 bytes, int arrays and n_device to 4; all device
 * pointers of the context's device; n < 0 is an error, n = 0 touches nothing); n_device is NULL or a device word: min(n, *n_device)
 * rows are processed, each written exactly once as whole 16-byte stores, and the rows after them are not written.  They need an
 * uploaded scene, no queues, and touch none of the render's queues, pixel state or statistics.  A scene without media answers both
 * with an error that says so.
 *
 * wf_medium_sample_device: the lambda of SampleMediumInteraction (wavefront/media.cpp:29-164) up to the routing, without the path
 * state — delta tracking along the ray: absorb, scatter or null-collide, with the medium's emission.
 *   reads    rays8[i] = {o, d (NOT normalised: as the ray carries it), tMax in units of d, time}: the layout of wf_trace_closest_device_t;
 *            tMax = the t of the closest-hit record, +infinity for a miss
 *            medium[i] = the medium the ray is in;  lambda4[i] = the four wavelengths
 *            beta4, r_u4, r_l4 = the path's state on entry
 *            flags[i] (flags may be NULL: all 1): bit 0 = collect the medium's emission — the render's `depth < maxDepth`, which belongs
 *            to the caller's path
 *   writes   event4[i] = {kind, tentative collisions taken, 0, 0} (int32)
 *              kind 0  no row: medium[i] >= "media" (wf_ctx_query), an origin that is not finite, a direction whose squared length is
 *                      not a finite positive number (zero, NaN, infinite, under- or overflowing), a NaN or negative tMax.  Every output
 *                      is zeros; the tables are not indexed by the id and the tracking loop is not entered.
 *              kind 1  the ray reached tMax with beta and r_u not black: beta, r_u and r_l are rescaled by T_maj / T_maj[0].  The caller
 *                      goes on to its hit or its escape.  A row with medium[i] < 0 (a ray in no medium) is kind 1 with its spectra
 *                      copied bit for bit and 0 collisions.
 *              kind 2  the path ended: absorbed, a scatter or a null collision that left beta or r_u black, or black on arrival.  The
 *                      spectra are what the render holds when it drops the item.  (Also a row that took 2^20 tentative collisions: the
 *                      walk of a row is bounded; the rows of tools/medium_check --self take 15 at the most, profiles/medium_device.txt shows 19.)
 *              kind 3  a real scatter with usable throughput: p_g4[i] = {p, the phase function's g}; beta and r_u as media.cpp:104-106
 *                      updates them; out_r_l4 is the row's r_l on entry (the scatter item carries none: the next ray's is r_u / pdf)
 *            p_g4[i] (zeros unless kind 3);  out_beta4, out_r_u4, out_r_l4: each may be the same pointer as its input (a row is read
 *            before it is written);  L4[i] = the emission collected along the ray, from 0: the render adds it to the pixel's L; zeros
 *            where the flag is clear
 *   The RNG of a row is seeded as the render seeds it, Hash(o, tMax), Hash(d): the same ray gives the render's own event.  The kernel is
 *   the scene's variant, "medium_sample_variant" (wf_ctx_query): 1 the lean one, as "medium_lean".
 *
 * wf_phase_device: the phase-function half of SampleMediumScattering (wavefront/media.cpp:270-348) — Henyey-Greenstein, the only phase
 * function of this path.
 *   reads    rays8[i] of the ray that scattered: wo = -d, NOT normalised, as the render carries it; the time
 *            p_g4[i] of wf_medium_sample_device;  wi4[i] = {wi, unused} (may be NULL);  u4[i] = {u[0], u[1], unused, unused} (may be
 *            NULL).  At least one of wi4 and u4 is given; the outputs of an absent half may be NULL and are not written.
 *   writes   wi4:  p_pdf4[i] = {phase.p(wo, wi), phase.PDF(wo, wi), 0, 0}
 *            u4:   sample4[i] = {p, pdf, 0, 0} of phase.Sample_p(wo, u);  next_rays8[i] = {p, wi, +infinity, the row's time}: a ray of
 *                  wf_trace_closest_device_t.  A sample with pdf 0 is zeros in both.
 *   Russian roulette, the next ray's medium (the one the ray was in) and depth + 1 are the caller's.  The light sample of the vertex is
 *   wf_light_sample_device on fabricated planes: pi lower = pi upper = p, n = ns = 0, the time in plane 2.w, valid = 1, medium inside =
 *   outside = the ray's medium (wfpt.Scene.medium_light_planes).
 * NOT here: the BSSRDF (wf_abi.h).
 */
#ifndef WF_MEDIA_H
#define WF_MEDIA_H

#include "wf_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

int wf_medium_sample_device(wf_ctx *ctx, int n, const int32_t *n_device /* may be NULL */, const float *rays8 /* [n][8] */,
                            const int32_t *medium /* [n] */, const float *lambda4 /* [n][4] */, const float *beta4 /* [n][4] */,
                            const float *r_u4 /* [n][4] */, const float *r_l4 /* [n][4] */, const int32_t *flags /* [n], may be NULL */,
                            int32_t *event4 /* [n][4] */, float *p_g4 /* [n][4] */, float *out_beta4 /* [n][4] */, float *out_r_u4 /* [n][4] */,
                            float *out_r_l4 /* [n][4] */, float *L4 /* [n][4] */);
int wf_phase_device(wf_ctx *ctx, int n, const int32_t *n_device /* may be NULL */, const float *rays8 /* [n][8] */, const float *p_g4 /* [n][4] */,
                    const float *wi4 /* [n][4], may be NULL */, const float *u4 /* [n][4], may be NULL */, float *p_pdf4 /* [n][4] */,
                    float *sample4 /* [n][4] */, float *next_rays8 /* [n][8] */);

#ifdef __cplusplus
}
#endif
#endif /* WF_MEDIA_H */
