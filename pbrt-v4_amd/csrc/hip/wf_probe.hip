// wf_probe.hip — libwfhip.so: test infrastructure.  The three kernels that exist only for the tests — the sampler probe, the libm probe
// and the known-answer harness of wf_kat.h — with their entry points (include/wf_abi.h), in a code object of their own: the render's
// carries none of them.  Compiled with wf_backend.hip's flags and prelude (wf_ctx.h), so the probes exercise the device functions as
// the render's unit compiles them.
#include "wf_ctx.h"

__global__ void __launch_bounds__(BLOCK) k_sampler_probe(const SceneView sv, int n, const int32_t *px, const int32_t *py, const int32_t *si, int startDim, int ndims, float *out) {
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        PixelSampler s(sv);
        s.StartPixelSample(px[i], py[i], si[i], startDim);
        SamplerProbeRecord(s, ndims, out + (size_t)i * (ndims > 0 ? ndims : ndims == -3 ? 30 : 2));
    }
}

extern "C" {

int wf_sampler_probe(wf_ctx *ctx, int n, const int32_t *px, const int32_t *py, const int32_t *sample_index, int start_dim, int ndims, float *out) {
    if (!ctx || !ctx->sceneLoaded) return fail(-1, "no scene uploaded");
    useDevice(ctx);
    if (n <= 0) return 0;
    if (ndims == 0 || ndims < -4 || ndims == -1) return fail(-1, "wf_sampler_probe: ndims %d", ndims);
    const int mode = ndims;
    ndims = mode > 0 ? mode : mode == -3 ? 30 : 2;   // floats per record (SamplerProbeRecord, wf_camera.h)
    DeviceScratch tmp(ctx->stream);
    int32_t *din = nullptr;
    float *dout = nullptr;
    int e;
    if ((e = tmp.alloc(&din, (size_t)3 * n)) || (e = tmp.alloc(&dout, (size_t)n * ndims))) return e;
    HIPCHK(hipMemcpyAsync(din, px, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(din + n, py, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(din + 2 * (size_t)n, sample_index, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    LAUNCH("sampler probe", k_sampler_probe, gridFor(n), ctx->svHost, n, din, din + n, din + 2 * (size_t)n, start_dim, mode, dout);
    HIPCHK(hipMemcpyAsync(out, dout, (size_t)n * ndims * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

__global__ void k_libm_probe(int fn, int n, const float *in, float *out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float r;
    if (fn == 9) r = wf::atan2(in[2 * i], in[2 * i + 1]);
    else {
        float x = in[i];
        switch (fn) {
        case 0: r = wf::sin(x); break;
        case 1: r = wf::cos(x); break;
        case 2: r = wf::exp(x); break;
        case 3: r = wf::log(x); break;
        case 4: r = wf::atan(x); break;
        case 5: r = wf::asin(x); break;
        case 6: r = wf::acos(x); break;
        case 7: r = wf::cosh(x); break;
        case 10: r = wf::sinh(x); break;
        case 11: r = wf::tan(x); break;
        default: r = wf::atanh(x); break;
        }
    }
    out[i] = r;
    }
}
int wf_libm_probe(wf_ctx *ctx, int fn, int n, const float *in, float *out) {
    if (!ctx) return fail(-1, "null context");
    if (fn < 0 || fn > 11) return fail(-1, "wf_libm_probe: unknown function %d", fn);
    if (n <= 0) return 0;
    size_t nin = (size_t)n * (fn == 9 ? 2 : 1);
    DeviceScratch tmp(ctx->stream);
    float *din = nullptr, *dout = nullptr;
    int e;
    if ((e = tmp.upload(&din, in, nin)) || (e = tmp.alloc(&dout, (size_t)n))) return e;
    LAUNCH("libm probe", k_libm_probe, gridFor(n), fn, n, din, dout);
    HIPCHK(hipMemcpyAsync(out, dout, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

__global__ void k_kat_probe(int n, const uint64_t *in, uint64_t *out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) wf::KatRun(in + 16 * (size_t)i, out + 8 * (size_t)i);
}
int wf_kat_probe(wf_ctx *ctx, int n, const uint64_t *in, uint64_t *out) {
    if (!ctx) return fail(-1, "null context");
    if (n <= 0) return 0;
    DeviceScratch tmp(ctx->stream);
    uint64_t *din = nullptr, *dout = nullptr;
    int e;
    if ((e = tmp.upload(&din, in, (size_t)n * 16)) || (e = tmp.alloc(&dout, (size_t)n * 8))) return e;
    LAUNCH("known-answer probe", k_kat_probe, gridFor(n), n, din, dout);
    HIPCHK(hipMemcpyAsync(out, dout, (size_t)n * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
