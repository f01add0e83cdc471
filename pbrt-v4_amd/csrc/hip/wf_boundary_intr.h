// wf_boundary_intr.h — the launchers of wf_boundary_intr.hip: the two kernels behind wf_hit_interaction_device and
// wf_camera_rays_device (include/wf_abi.h).  The kernels live in a unit of their own so that no kernel of wf_backend.hip shares a
// device code object with them; wf_boundary.hip holds the entry points (argument checks, the context's stream, the profile bracket).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../../include/wf_abi.h"

namespace wf {
struct SceneView;
struct WorkState;
// (hidden: shared by the library's units, not exported from it)
namespace boundary __attribute__((visibility("hidden"))) {

// k_hit_interaction<variant> (planning::IntrVariant, wf_plan.h) over n (ray, hit record) pairs into the planes out_f [WF_INTR_FPLANES][n][4] / out_i [WF_INTR_IPLANES][n][4].
// svDev: the scene view's device-resident copy.  Returns a hipError_t (0: launched); -1: no such variant.
int LaunchHitInteraction(hipStream_t stream, int variant, const SceneView *svDev, int n, const float *rays8, const wf_hit_record *hits, float *outF,
                         int32_t *outI);
// k_pack_camera_rays: ray queue 0 of `ws` (at most nMax items) to the caller's arrays, the queue's size to *nOut
int LaunchPackCameraRays(hipStream_t stream, const WorkState &ws, int nMax, float *rays8, int32_t *pixelXY, float *lambda4, int32_t *nOut);
// k_pack_camera_samples (wf_camera_samples_device): the same, with the wavelengths' PDF, the camera-ray weight and the filter weight of each item's pixel sample
int LaunchPackCameraSamples(hipStream_t stream, const WorkState &ws, int nMax, float *rays8, int32_t *pixelXY, float *lambda4, float *lambdaPdf4,
                            float *cameraWeight4, float *filterWeight, int32_t *nOut);

}}  // namespace wf::boundary
