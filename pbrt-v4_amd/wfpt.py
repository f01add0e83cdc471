"""wfpt — ctypes binding of the MI355X wavefront path tracer's two shared libraries:

  _build/libwfhost.so  (include/wf_host.h)  scene parser, flat-table builder, render loop
  _build/libwfhip.so   (include/wf_abi.h)   HIP/CDNA4 kernels behind the C ABI

Python is plumbing only (tests, bench.py, torch.distributed for the multi-GPU film reduce).  There is no
CPU fallback: if the libraries are missing, or no gfx950 device is visible when a renderer is created,
the calls raise.

The package directory is called ``pbrt-v4_amd`` (not an importable identifier); load this module with
``importlib`` — see ``load()`` in tests/conftest.py, bench.py and __graft_entry__.py.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.environ.get("WF_BUILD_DIR") or os.path.join(HERE, "_build")  # WF_BUILD_DIR: timing / validation of variant builds (pbrt-v4_amd/_exp*)
DATA = os.path.join(HERE, "data")


class WfError(RuntimeError):
    pass


class Info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "width", "height", "spp", "max_queue_size", "n_passes", "scanlines_per_pass",
        "n_triangles", "n_bvh_nodes", "n_lights", "max_depth", "save_fp16", "y0")]


class RenderStats(C.Structure):
    _fields_ = [("camera_rays", C.c_uint64), ("indirect_rays", C.c_uint64 * 64), ("shadow_rays", C.c_uint64 * 64)]


class HitRecord(C.Structure):
    _fields_ = [("prim", C.c_int32), ("t", C.c_float), ("b0", C.c_float), ("b1", C.c_float), ("b2", C.c_float),
                ("nodes_visited", C.c_int32), ("tris_tested", C.c_int32), ("instance", C.c_int32)]


# wf_hit_record as a numpy structured dtype (eight 32-bit words)
HIT_DTYPE = np.dtype([("prim", "<i4"), ("t", "<f4"), ("b0", "<f4"), ("b1", "<f4"), ("b2", "<f4"),
                      ("nodes_visited", "<i4"), ("tris_tested", "<i4"), ("instance", "<i4")])


def hit_records(words):
    """The int32 [n, 8] tensor of record words that the device-buffer calls return (Scene.trace_device, Scene.trace_one_random_device),
    downloaded and viewed as wf_hit_record fields: a numpy structured array of n records (HIT_DTYPE)."""
    a = np.ascontiguousarray(words.detach().cpu().numpy(), dtype=np.int32).reshape(-1, 8)
    return a.view(HIT_DTYPE).reshape(-1).copy()


class TraversalCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "closest_rays", "closest_nodes", "closest_tris", "closest_hits",
        "shadow_rays", "shadow_nodes", "shadow_tris", "shadow_unoccluded")]


class ProfileEntry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_int32), ("total_ms", C.c_float), ("min_ms", C.c_float), ("max_ms", C.c_float)]


# every symbol include/wf_abi.h and include/wf_host.h declare (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "wf_last_error", "wf_abi_version", "wf_ctx_create", "wf_ctx_destroy", "wf_sync", "wf_stream", "wf_scene_upload",
    "wf_medium_sample", "wf_intersect_shadow_tr", "wf_subsurface_probe", "wf_intersect_one_random", "wf_subsurface_scatter", "wf_trace_one_random_host", "wf_morton_sort", "wf_build_bvh_sah", "wf_aggregate_bounds", "wf_queues_alloc", "wf_set_pass_samples", "wf_set_strips", "wf_film_clear", "wf_reset_ray_queue", "wf_reset_stage_queues",
    "wf_gen_camera_rays", "wf_gen_ray_samples", "wf_intersect_closest", "wf_handle_escaped", "wf_handle_emissive",
    "wf_eval_material", "wf_intersect_shadow", "wf_update_film", "wf_render_pass", "wf_film_download",
    "wf_film_device_ptr", "wf_film_upload", "wf_film_spectral_download", "wf_film_gbuffer_download", "wf_film_copy_to_device", "wf_film_copy_from_device", "wf_film_gather_strips", "wf_stats_add", "wf_material_items_download", "wf_stats_download",
    "wf_profile_report", "wf_profile_enable",
    "wf_trace_closest_host", "wf_trace_any_host", "wf_sampler_probe", "wf_libm_probe", "wf_kat_probe", "wf_queue_size", "wf_queue_download",
    "wf_counters_enable", "wf_counters_download", "wf_kernel_time_ms", "wf_debug_counters", "wf_debug_fastbvh_check", "wf_scene_check_instances", "wf_scene_plan_query", "wf_trace_closest_host_t", "wf_trace_any_host_t", "wf_ctx_query",
    "wf_trace_closest_device", "wf_trace_any_device", "wf_device_alloc", "wf_device_free", "wf_device_upload", "wf_device_download", "wf_trace_shadow_tr_host",
    "wf_trace_shadow_tr_host_t", "wf_trace_one_random_host_t",
    "wf_trace_closest_device_t", "wf_trace_any_device_t", "wf_trace_shadow_tr_device", "wf_trace_one_random_device",
    "wf_film_spectral_upload", "wf_film_gbuffer_upload", "wf_film_channel_count", "wf_film_develop_device", "wf_film_develop_rgb_device",
    "wf_hit_interaction_device", "wf_camera_rays_device",
    "wf_camera_samples_device", "wf_film_add_samples_device", "wf_light_sample_device", "wf_light_emitted_device",
    "wf_bsdf_make_device", "wf_bsdf_eval_device",
]
# every symbol include/wf_media.h declares (checked by tests/test_medium_host.py): an addition beside wf_abi.h, same library
MEDIA_SYMBOLS = ["wf_medium_sample_device", "wf_phase_device"]
# the event kinds of wf_medium_sample_device (event4 word 0)
MEDIUM_NONE, MEDIUM_ARRIVED, MEDIUM_ENDED, MEDIUM_SCATTER = 0, 1, 2, 3
# the planes of a wf_bsdf_make_device record (include/wf_abi.h: WF_BSDF_PLANES), and the bit of bsdf4 word 0 beside the BxDFFlags
BSDF_PLANES = 10
BSDF_TERMINATED = 1 << 8
# the planes of wf_hit_interaction_device (include/wf_abi.h): WF_INTR_FPLANES float planes, WF_INTR_IPLANES int planes, 4 words per item each
INTR_FPLANES = 11
INTR_IPLANES = 2
HOST_SYMBOLS = [
    "wfh_init", "wfh_last_error", "wfh_scene_load", "wfh_scene_load_string", "wfh_scene_free", "wfh_scene_desc", "wfh_scene_info",
    "wfh_renderer_create", "wfh_renderer_create_strips", "wfh_renderer_set_strips", "wfh_renderer_samples_per_pass", "wfh_renderer_ctx", "wfh_render", "wfh_clear_film", "wfh_download_film", "wfh_stats",
    "wfh_film_to_rgb", "wfh_write_image", "wfh_read_image", "wfh_read_nanovdb", "wfh_build_bvh_host", "wfh_film_channels", "wfh_write_film_image",
    "wfh_film_image_device",
]

_hip = None
_host = None


def libs():
    """Load (once) and return (libwfhost, libwfhip).  Raises if the in-tree build is missing."""
    global _hip, _host
    if _host is not None:
        return _host, _hip
    hip_path = os.path.join(BUILD, "libwfhip.so")
    host_path = os.path.join(BUILD, "libwfhost.so")
    for p in (hip_path, host_path):
        if not os.path.exists(p):
            raise WfError("%s is missing: run __graft_entry__.build() (make -C pbrt-v4_amd)" % p)
    _hip = C.CDLL(hip_path, mode=C.RTLD_GLOBAL)
    _host = C.CDLL(host_path, mode=C.RTLD_GLOBAL)
    _hip.wf_last_error.restype = C.c_char_p
    _hip.wf_stream.restype = C.c_void_p
    _hip.wf_stream.argtypes = [C.c_void_p]
    _host.wfh_last_error.restype = C.c_char_p
    _host.wfh_scene_load.restype = C.c_void_p
    _host.wfh_scene_load.argtypes = [C.c_char_p, C.c_int, C.c_int]
    _host.wfh_scene_load_string.restype = C.c_void_p
    _host.wfh_scene_load_string.argtypes = [C.c_char_p, C.c_int, C.c_int]
    _host.wfh_scene_free.argtypes = [C.c_void_p]
    _host.wfh_scene_desc.restype = C.c_void_p
    _host.wfh_scene_desc.argtypes = [C.c_void_p]
    _host.wfh_scene_info.argtypes = [C.c_void_p, C.POINTER(Info)]
    _host.wfh_renderer_create.argtypes = [C.c_void_p, C.c_int, C.c_int]
    _host.wfh_renderer_create_strips.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    _host.wfh_renderer_samples_per_pass.argtypes = [C.c_void_p]
    _host.wfh_renderer_set_strips.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    _host.wfh_renderer_ctx.restype = C.c_void_p
    _host.wfh_renderer_ctx.argtypes = [C.c_void_p]
    _host.wfh_render.restype = C.c_double
    _host.wfh_render.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    _host.wfh_clear_film.argtypes = [C.c_void_p]
    _host.wfh_download_film.argtypes = [C.c_void_p, C.c_void_p]
    _host.wfh_stats.argtypes = [C.c_void_p, C.POINTER(RenderStats)]
    _host.wfh_film_to_rgb.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    _host.wfh_write_image.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    _host.wfh_read_image.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
    for name in ("wf_sync", "wf_film_clear", "wf_ctx_destroy"):
        getattr(_hip, name).argtypes = [C.c_void_p]
    _hip.wf_profile_enable.argtypes = [C.c_void_p, C.c_int]
    _hip.wf_counters_enable.argtypes = [C.c_void_p, C.c_int]
    _hip.wf_counters_download.argtypes = [C.c_void_p, C.POINTER(TraversalCounters)]
    _hip.wf_profile_report.argtypes = [C.c_void_p, C.POINTER(ProfileEntry), C.c_int, C.POINTER(C.c_int)]
    _hip.wf_film_device_ptr.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    _hip.wf_film_copy_to_device.argtypes = [C.c_void_p, C.c_void_p]
    _hip.wf_film_copy_from_device.argtypes = [C.c_void_p, C.c_void_p]
    _hip.wf_trace_closest_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    _hip.wf_trace_any_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _hip.wf_sampler_probe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    _hip.wf_libm_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    _hip.wf_kat_probe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    _hip.wf_material_items_download.argtypes = [C.c_void_p, C.c_void_p]
    _hip.wf_kernel_time_ms.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    _hip.wf_aggregate_bounds.argtypes = [C.c_void_p, C.c_void_p]
    _hip.wf_render_pass.argtypes = [C.c_void_p, C.c_int, C.c_int]
    _hip.wf_film_channel_count.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    for f in (_hip.wf_film_develop_device, _hip.wf_film_develop_rgb_device):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    for name in ("wf_film_upload", "wf_film_spectral_upload", "wf_film_gbuffer_upload", "wf_film_spectral_download", "wf_film_gbuffer_download"):
        getattr(_hip, name).argtypes = [C.c_void_p, C.c_void_p]
    _host.wfh_film_image_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    if _host.wfh_init(DATA.encode()) != 0:
        raise WfError("wfh_init failed (data dir %s)" % DATA)
    return _host, _hip


def _check(rc, what):
    if rc != 0:
        _, hip = libs()
        raise WfError("%s failed: %s" % (what, hip.wf_last_error().decode(errors="replace")))


class Scene:
    """A parsed .pbrt scene flattened into the ABI's tables (BasicScene + CreateAggregate equivalent)."""

    def __init__(self, path=None, text=None, spp=0, seed=0):
        host, _ = libs()
        if path is not None:
            self.h = host.wfh_scene_load(os.fsencode(path), spp, seed)
        else:
            self.h = host.wfh_scene_load_string(text.encode(), spp, seed)
        if not self.h:
            host.wfh_last_error.restype = C.c_char_p
            raise WfError("scene load failed: " + (host.wfh_last_error() or b"").decode(errors="replace"))
        self.info = Info()
        host.wfh_scene_info(self.h, C.byref(self.info))
        self._renderer = False

    @property
    def width(self):
        return self.info.width

    @property
    def height(self):
        return self.info.height

    @property
    def spp(self):
        return self.info.spp

    def create_renderer(self, device=0, samples_per_pass=0, strips=None):
        """WavefrontPathIntegrator ctor: upload tables to HIP device `device`, allocate queues.
        samples_per_pass: sample indices one pass carries (0 = automatic); the film is bit-identical for any value.
        strips = (rank, count[, height]): this renderer is one rank of a multi-GPU image partition from the start — its queues are
        sized for its own rows (wfh_renderer_create_strips)."""
        host, _ = libs()
        if strips is not None and strips[1] > 1:
            rc = host.wfh_renderer_create_strips(self.h, device, samples_per_pass, strips[0], strips[1], strips[2] if len(strips) > 2 else 16)
        else:
            rc = host.wfh_renderer_create(self.h, device, samples_per_pass)
        if rc != 0:
            raise WfError("renderer creation failed: " + (host.wfh_last_error() or b"").decode(errors="replace"))
        self._renderer = True
        self.device = device
        self.nan_values = 0   # NaN channel values the last image_tensor() / film_channels_tensor() stored as 0
        self.samples_per_pass = host.wfh_renderer_samples_per_pass(self.h)
        self.ctx = host.wfh_renderer_ctx(self.h)
        return self

    def set_strips(self, rank, count, height=16):
        """multi-GPU image partition (wf_set_strips): this renderer owns the scanline strips rank, rank + count, ..."""
        host, _ = libs()
        if host.wfh_renderer_set_strips(self.h, rank, count, height) != 0:
            raise WfError("set_strips failed")

    def render(self, sample_begin=0, sample_end=None, sample_step=1, fused=True):
        """Render(): returns wall seconds."""
        host, _ = libs()
        if not self._renderer:
            raise WfError("create_renderer() first")
        if sample_end is None:
            sample_end = self.info.spp
        s = host.wfh_render(self.h, sample_begin, sample_end, sample_step, 1 if fused else 0)
        if s < 0:
            raise WfError("render failed")
        return s

    def clear_film(self):
        host, _ = libs()
        host.wfh_clear_film(self.h)

    def film(self):
        """[H, W, 4] float64: rgbSum[3], weightSum per pixel (film.h:302-307)."""
        host, _ = libs()
        a = np.empty((self.info.height, self.info.width, 4), dtype=np.float64)
        if host.wfh_download_film(self.h, a.ctypes.data) != 0:
            raise WfError("film download failed")
        return a

    def film_to_rgb(self, film):
        host, _ = libs()
        film = np.ascontiguousarray(film, dtype=np.float64)
        rgb = np.empty((self.info.height, self.info.width, 3), dtype=np.float32)
        host.wfh_film_to_rgb(self.h, film.ctypes.data, rgb.ctypes.data)
        return rgb

    def image(self):
        return self.film_to_rgb(self.film())

    def film_channels(self):
        """SpectralFilm / GBufferFilm::GetImage of a scene with `Film "spectral"` or `Film "gbuffer"`: (channel names, float32 array [H][W][n])"""
        host, _ = libs()
        host.wfh_film_channels.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_char_p, C.c_void_p]
        nc = C.c_int32(0)
        if host.wfh_film_channels(self.h, C.byref(nc), None, None) != 0:
            raise WfError(host.wfh_last_error().decode(errors="replace"))
        names = C.create_string_buffer(32 * nc.value)
        px = np.empty((self.info.height, self.info.width, nc.value), np.float32)
        if host.wfh_film_channels(self.h, C.byref(nc), names, px.ctypes.data) != 0:
            raise WfError(host.wfh_last_error().decode(errors="replace"))
        return [names.raw[32 * i:32 * (i + 1)].split(b"\0")[0].decode() for i in range(nc.value)], px

    def write_film_image(self, path):
        host, _ = libs()
        host.wfh_write_film_image.argtypes = [C.c_void_p, C.c_char_p]
        if host.wfh_write_film_image(self.h, os.fsencode(path)) != 0:
            raise WfError("could not write %s: %s" % (path, host.wfh_last_error().decode(errors="replace")))

    def stats(self):
        host, _ = libs()
        st = RenderStats()
        host.wfh_stats(self.h, C.byref(st))
        return {"camera_rays": int(st.camera_rays), "indirect_rays": [int(v) for v in st.indirect_rays],
                "shadow_rays": [int(v) for v in st.shadow_rays]}

    def total_rays(self):
        st = self.stats()
        return st["camera_rays"] + sum(st["indirect_rays"][1:]) + sum(st["shadow_rays"])

    # ---- direct C-ABI access used by the parity tests and bench.py ----
    def trace_closest(self, o, d, tmax, reference_order=True):
        """reference_order=True: the reference-order walk (fills nodes_visited / tris_tested);
        False: the production traversal kernel (wf_traverse.h)"""
        _, hip = libs()
        o = np.ascontiguousarray(o, dtype=np.float32)
        d = np.ascontiguousarray(d, dtype=np.float32)
        tmax = np.ascontiguousarray(tmax, dtype=np.float32)
        n = o.shape[0]
        out = (HitRecord * n)()
        _check(hip.wf_trace_closest_host(self.ctx, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, out, 1 if reference_order else 0), "wf_trace_closest_host")
        return np.frombuffer(out, dtype=np.dtype([("prim", "<i4"), ("t", "<f4"), ("b0", "<f4"), ("b1", "<f4"), ("b2", "<f4"),
                                                  ("nodes_visited", "<i4"), ("tris_tested", "<i4"), ("instance", "<i4")])).copy()

    def trace_timed(self, o, d, tmax, time, any_hit=False):
        """wf_trace_closest_host_t / wf_trace_any_host_t: the reference-order walks at the rays' own times (AnimatedPrimitive)"""
        _, hip = libs()
        o = np.ascontiguousarray(o, dtype=np.float32)
        d = np.ascontiguousarray(d, dtype=np.float32)
        tmax = np.ascontiguousarray(tmax, dtype=np.float32)
        time = np.ascontiguousarray(time, dtype=np.float32)
        n = o.shape[0]
        for f in (hip.wf_trace_closest_host_t, hip.wf_trace_any_host_t):
            f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if any_hit:
            occ = np.empty(n, dtype=np.int32)
            _check(hip.wf_trace_any_host_t(self.ctx, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, time.ctypes.data, occ.ctypes.data), "wf_trace_any_host_t")
            return occ
        out = (HitRecord * n)()
        _check(hip.wf_trace_closest_host_t(self.ctx, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, time.ctypes.data, C.addressof(out)), "wf_trace_closest_host_t")
        return np.frombuffer(out, dtype=np.dtype([("prim", "<i4"), ("t", "<f4"), ("b0", "<f4"), ("b1", "<f4"), ("b2", "<f4"),
                                                  ("nodes_visited", "<i4"), ("tris_tested", "<i4"), ("instance", "<i4")])).copy()

    def trace_shadow_tr(self, o, d, tmax, medium, lambda_, Ld, r_u, r_l, time=None):
        """wf_trace_shadow_tr_host (time=None) / wf_trace_shadow_tr_host_t: IntersectShadowTr on the given shadow rays of a scene with media —
        per ray the medium id, four wavelengths and the item's Ld / r_u / r_l; returns the [n, 4] radiance each ray adds to its pixel"""
        _, hip = libs()
        o, d, tmax = (np.ascontiguousarray(a, dtype=np.float32) for a in (o, d, tmax))
        medium = np.ascontiguousarray(medium, dtype=np.int32)
        lambda_, Ld, r_u, r_l = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4) for a in (lambda_, Ld, r_u, r_l))
        n = o.shape[0]
        out = np.zeros((n, 4), dtype=np.float32)
        args = [self.ctx, n] + [a.ctypes.data for a in (o, d, tmax, medium, lambda_, Ld, r_u, r_l)]
        if time is None:
            hip.wf_trace_shadow_tr_host.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 9
            _check(hip.wf_trace_shadow_tr_host(*args, out.ctypes.data), "wf_trace_shadow_tr_host")
        else:
            time = np.ascontiguousarray(time, dtype=np.float32)
            hip.wf_trace_shadow_tr_host_t.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 10
            _check(hip.wf_trace_shadow_tr_host_t(*args, time.ctypes.data, out.ctypes.data), "wf_trace_shadow_tr_host_t")
        return out

    def trace_one_random(self, p0, p1, material, time=None):
        """wf_trace_one_random_host (time=None) / wf_trace_one_random_host_t: IntersectOneRandom on probe segments p0 -> p1 —
        (hit records, reservoir pdfs) of one surface of material[i] along each segment"""
        _, hip = libs()
        p0, p1 = (np.ascontiguousarray(a, dtype=np.float32) for a in (p0, p1))
        material = np.ascontiguousarray(material, dtype=np.int32)
        n = p0.shape[0]
        out = (HitRecord * n)()
        pdf = np.zeros(n, dtype=np.float32)
        if time is None:
            hip.wf_trace_one_random_host.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
            _check(hip.wf_trace_one_random_host(self.ctx, n, p0.ctypes.data, p1.ctypes.data, material.ctypes.data, C.addressof(out), pdf.ctypes.data),
                   "wf_trace_one_random_host")
        else:
            time = np.ascontiguousarray(time, dtype=np.float32)
            hip.wf_trace_one_random_host_t.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
            _check(hip.wf_trace_one_random_host_t(self.ctx, n, p0.ctypes.data, p1.ctypes.data, material.ctypes.data, time.ctypes.data, C.addressof(out),
                                                  pdf.ctypes.data), "wf_trace_one_random_host_t")
        return np.frombuffer(out, dtype=np.dtype([("prim", "<i4"), ("t", "<f4"), ("b0", "<f4"), ("b1", "<f4"), ("b2", "<f4"),
                                                  ("nodes_visited", "<i4"), ("tris_tested", "<i4"), ("instance", "<i4")])).copy(), pdf

    # ---- the device-buffer boundary (what a GPU-resident integrator binds): torch tensors in, torch tensors out, no host round trip ----
    def _device_call(self, what, fn, argtypes, tensors, *args):
        """Launch one device-buffer entry point on the context's stream (wf_stream), ordered after torch's current stream, and order
        torch's current stream after it: tensors that torch ops produced just before the call, and ops that consume the results just
        after it, need no synchronisation by the caller."""
        import torch
        _, hip = libs()
        dev = tensors[0].device
        for t in tensors:
            if not (t.is_cuda and t.device == dev and t.is_contiguous()):
                raise WfError("%s: the arguments are contiguous tensors on the context's device" % what)
        fn.argtypes = argtypes
        cur = torch.cuda.current_stream(dev)
        ext = torch.cuda.ExternalStream(hip.wf_stream(self.ctx), device=dev)
        ext.wait_stream(cur)
        rc = fn(self.ctx, *args)
        cur.wait_stream(ext)
        _check(rc, what)

    @staticmethod
    def _as(t, dtype, cols, what):
        import torch
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or (cols and (t.dim() != 2 or t.shape[1] != cols)) or (not cols and t.dim() != 1):
            raise WfError("%s: expected a %s tensor of shape [n%s]" % (what, dtype, ", %d" % cols if cols else ""))
        return t

    def trace_device(self, rays8, any_hit=False, out=None):
        """wf_trace_closest_device_t / wf_trace_any_device_t: rays8 = float32 [n, 8] rows {o, d, tMax, time} on the device.  Returns the
        hit records as an int32 [n, 8] tensor of their words (hit_records() views a downloaded copy by field), or — any_hit — the
        int32 [n] occlusion flags.  Any scene: a static one ignores the times.  out: a tensor to write into instead of a new one."""
        import torch
        _, hip = libs()
        self._as(rays8, torch.float32, 8, "trace_device rays8")
        n = rays8.shape[0]
        if out is None:
            out = torch.empty((n,) if any_hit else (n, 8), dtype=torch.int32, device=rays8.device)
        else:
            self._as(out, torch.int32, 0 if any_hit else 8, "trace_device out")
            if out.shape[0] < n:
                raise WfError("trace_device: out holds fewer than n results")
        f = hip.wf_trace_any_device_t if any_hit else hip.wf_trace_closest_device_t
        self._device_call(f.__name__, f, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p], [rays8, out], n, rays8.data_ptr(), out.data_ptr())
        return out

    def trace_shadow_tr_device(self, rays8, medium, lambda_, Ld, r_u, r_l):
        """wf_trace_shadow_tr_device: IntersectShadowTr on device items of a scene with media — rays8 float32 [n, 8], medium int32 [n],
        lambda_ / Ld / r_u / r_l float32 [n, 4].  Returns the float32 [n, 4] radiance each ray adds to its pixel."""
        import torch
        _, hip = libs()
        self._as(rays8, torch.float32, 8, "trace_shadow_tr_device rays8")
        self._as(medium, torch.int32, 0, "trace_shadow_tr_device medium")
        for t in (lambda_, Ld, r_u, r_l):
            self._as(t, torch.float32, 4, "trace_shadow_tr_device lambda_ / Ld / r_u / r_l")
        n = rays8.shape[0]
        if any(t.shape[0] != n for t in (medium, lambda_, Ld, r_u, r_l)):
            raise WfError("trace_shadow_tr_device: the arrays hold different numbers of items")
        out = torch.empty((n, 4), dtype=torch.float32, device=rays8.device)
        ts = [rays8, medium, lambda_, Ld, r_u, r_l, out]
        self._device_call("wf_trace_shadow_tr_device", hip.wf_trace_shadow_tr_device, [C.c_void_p, C.c_int] + [C.c_void_p] * 7, ts, n, *[t.data_ptr() for t in ts])
        return out

    def trace_one_random_device(self, segs7, material):
        """wf_trace_one_random_device: IntersectOneRandom on device probe segments — segs7 float32 [n, 7] rows {p0, p1, time}, material
        int32 [n].  Returns (hit records as an int32 [n, 8] tensor, reservoir pdfs as a float32 [n] tensor)."""
        import torch
        _, hip = libs()
        self._as(segs7, torch.float32, 7, "trace_one_random_device segs7")
        self._as(material, torch.int32, 0, "trace_one_random_device material")
        n = segs7.shape[0]
        if material.shape[0] != n:
            raise WfError("trace_one_random_device: the arrays hold different numbers of items")
        out = torch.empty((n, 8), dtype=torch.int32, device=segs7.device)
        pdf = torch.empty((n,), dtype=torch.float32, device=segs7.device)
        ts = [segs7, material, out, pdf]
        self._device_call("wf_trace_one_random_device", hip.wf_trace_one_random_device, [C.c_void_p, C.c_int] + [C.c_void_p] * 4, ts, n, *[t.data_ptr() for t in ts])
        return out, pdf

    def interactions_device(self, rays8, hits, out=None):
        """wf_hit_interaction_device: the SurfaceInteractions of the hit records `hits` (the int32 [n, 8] tensor of trace_device) that the
        rays `rays8` (float32 [n, 8]) found.  Returns a dict of tensor VIEWS into the call's two plane tensors — float32 [n, 3]: pi_lo,
        pi_hi, n, ns, wo, dpdu, dpdv, dpdus, dpdvs, dndus, dndvs; float32 [n, 2]: uv; float32 [n]: time, t; int32 [n]: material (-1: an
        interface surface), area_light (-1: none), medium_inside, medium_outside, mesh, valid (1 hit, 0 miss, -1 a record outside the
        scene's ranges), mesh_flags (WF_MESH_*) — and the plane tensors themselves as "planes_f" [11, n, 4] / "planes_i" [2, n, 4].
        out = (float32 tensor, int32 tensor), contiguous, of at least 11 * n * 4 and 2 * n * 4 elements: written into instead of new
        ones (the planes are the leading elements)."""
        import torch
        _, hip = libs()
        self._as(rays8, torch.float32, 8, "interactions_device rays8")
        self._as(hits, torch.int32, 8, "interactions_device hits")
        n = rays8.shape[0]
        if hits.shape[0] != n:
            raise WfError("interactions_device: rays8 and hits hold different numbers of items")
        nf, ni = INTR_FPLANES * n * 4, INTR_IPLANES * n * 4
        if out is None:
            of = torch.empty((nf,), dtype=torch.float32, device=rays8.device)
            oi = torch.empty((ni,), dtype=torch.int32, device=rays8.device)
        else:
            of, oi = out
            if not (isinstance(of, torch.Tensor) and isinstance(oi, torch.Tensor) and of.dtype == torch.float32 and oi.dtype == torch.int32
                    and of.is_contiguous() and oi.is_contiguous() and of.numel() >= nf and oi.numel() >= ni):
                raise WfError("interactions_device: out is (float32 tensor of >= %d elements, int32 tensor of >= %d elements), contiguous" % (nf, ni))
            of, oi = of.view(-1), oi.view(-1)
        self._device_call("wf_hit_interaction_device", hip.wf_hit_interaction_device, [C.c_void_p, C.c_int] + [C.c_void_p] * 4, [rays8, hits, of, oi],
                          n, rays8.data_ptr(), hits.data_ptr(), of.data_ptr(), oi.data_ptr())
        F = of[:nf].view(INTR_FPLANES, n, 4)
        I = oi[:ni].view(INTR_IPLANES, n, 4)
        r = {"planes_f": F, "planes_i": I}
        for k, name in enumerate(("pi_lo", "pi_hi", "n", "ns", "wo", "dpdu", "dpdv", "dpdus", "dpdvs", "dndus", "dndvs")):
            r[name] = F[k, :, :3]
        r["uv"] = torch.as_strided(F, (n, 2), (4, 4 * n), F.storage_offset() + 3)   # the w words of planes 0 and 1
        r["time"], r["t"] = F[2, :, 3], F[3, :, 3]
        for k, name in enumerate(("material", "area_light", "medium_inside", "medium_outside")):
            r[name] = I[0, :, k]
        r["mesh"], r["valid"], r["mesh_flags"] = I[1, :, 0], I[1, :, 1], I[1, :, 2]
        return r

    def camera_rays_device(self, sample_index, y0=None):
        """wf_camera_rays_device: the scene's own camera rays of sample index `sample_index` as device tensors (rays8 float32 [n, 8] rows
        {o, d, tMax = inf, time}, pixel_xy int32 [n, 2], lambda4 float32 [n, 4]), trimmed to the number of rays generated (a realistic
        camera's lens blocks some).  y0: the first scanline of ONE band of the renderer's passes; None: every band of the image, in
        order.  Reads the ray count back, so it synchronises; overwrites the renderer's per-pass state (for an idle renderer)."""
        import torch
        _, hip = libs()
        if not self._renderer:
            raise WfError("camera_rays_device: create_renderer() first")
        dev = torch.device("cuda", self.device)
        cap = self.query("pixels_per_pass")
        rows = max(1, cap // self.info.width)
        bands = [y0] if y0 is not None else list(range(self.info.y0, self.info.y0 + self.info.height, rows))
        parts = []
        for y in bands:
            rays = torch.empty((cap, 8), dtype=torch.float32, device=dev)
            pix = torch.empty((cap, 2), dtype=torch.int32, device=dev)
            lam = torch.empty((cap, 4), dtype=torch.float32, device=dev)
            count = torch.zeros((1,), dtype=torch.int32, device=dev)
            ts = [rays, pix, lam, count]
            self._device_call("wf_camera_rays_device", hip.wf_camera_rays_device, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4, ts,
                              y, sample_index, cap, *[t.data_ptr() for t in ts])
            parts.append((rays, pix, lam, count))
        out = []
        for rays, pix, lam, count in parts:
            k = int(count.item())
            out.append((rays[:k], pix[:k], lam[:k]))
        if len(out) == 1:
            return out[0]
        return tuple(torch.cat([o[j] for o in out]) for j in range(3))

    def camera_samples_device(self, sample_index, y0=None):
        """wf_camera_samples_device: camera_rays_device plus the three weights the film needs — returns (rays8, pixel_xy, lambda4,
        lambda_pdf4 float32 [n, 4], camera_weight4 float32 [n, 4], filter_weight float32 [n]), in ray-queue order, trimmed to the number
        of rays generated.  y0 / bands, the synchronisation and the overwritten per-pass state: as camera_rays_device."""
        import torch
        _, hip = libs()
        if not self._renderer:
            raise WfError("camera_samples_device: create_renderer() first")
        dev = torch.device("cuda", self.device)
        cap = self.query("pixels_per_pass")
        rows = max(1, cap // self.info.width)
        bands = [y0] if y0 is not None else list(range(self.info.y0, self.info.y0 + self.info.height, rows))
        parts = []
        for y in bands:
            ts = [torch.empty((cap, 8), dtype=torch.float32, device=dev), torch.empty((cap, 2), dtype=torch.int32, device=dev)]
            ts += [torch.empty((cap, 4), dtype=torch.float32, device=dev) for _ in range(3)]
            ts += [torch.empty((cap,), dtype=torch.float32, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)]
            self._device_call("wf_camera_samples_device", hip.wf_camera_samples_device, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7, ts,
                              y, sample_index, cap, *[t.data_ptr() for t in ts])
            parts.append(ts)
        out = []
        for ts in parts:
            k = int(ts[-1].item())
            out.append(tuple(t[:k] for t in ts[:-1]))
        if len(out) == 1:
            return out[0]
        return tuple(torch.cat([o[j] for o in out]) for j in range(6))

    def film_add_device(self, pixel_xy, L4, lambda4, lambda_pdf4, filter_weight, n_device=None, rejected=None):
        """wf_film_add_samples_device: Film::AddSample for n device items — pixel_xy int32 [n, 2], L4 float32 [n, 4] = the radiance times
        the camera-ray weight, lambda4 / lambda_pdf4 float32 [n, 4], filter_weight float32 [n] (what camera_samples_device returns).
        One sample per pixel per call: a second item of one pixel is not added, and counted into `rejected` (an int32 or uint32 tensor
        of one element that the caller zeroes; None: not counted).  n_device: an int32 tensor of one element; only the first
        min(n, n_device) items are added, without a host synchronisation.  Not synchronised: ordered with torch's current stream on
        both sides, like every device-buffer call; image_tensor() / film() see the samples."""
        import torch
        _, hip = libs()
        self._as(pixel_xy, torch.int32, 2, "film_add_device pixel_xy")
        for t in (L4, lambda4, lambda_pdf4):
            self._as(t, torch.float32, 4, "film_add_device L4 / lambda4 / lambda_pdf4")
        self._as(filter_weight, torch.float32, 0, "film_add_device filter_weight")
        n = pixel_xy.shape[0]
        ts = [pixel_xy, L4, lambda4, lambda_pdf4, filter_weight]
        if any(t.shape[0] != n for t in ts):
            raise WfError("film_add_device: the arrays hold different numbers of items")
        if n == 0:
            return
        for t, what in ((n_device, "n_device"), (rejected, "rejected")):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.numel() != 1 or t.element_size() != 4 or t.is_floating_point():
                raise WfError("film_add_device: %s is a 32-bit integer tensor of one element" % what)
            ts.append(t)
        self._device_call("wf_film_add_samples_device", hip.wf_film_add_samples_device, [C.c_void_p, C.c_int] + [C.c_void_p] * 7, ts, n,
                          n_device.data_ptr() if n_device is not None else None, pixel_xy.data_ptr(), L4.data_ptr(), lambda4.data_ptr(), lambda_pdf4.data_ptr(),
                          filter_weight.data_ptr(), rejected.data_ptr() if rejected is not None else None)

    def first_hit(self, sample_index):
        """The closed loop of the device-buffer boundary: the camera rays of `sample_index`, their closest hits and the hits'
        interactions, all as device tensors.  Returns the dict of interactions_device plus "rays8", "pixel_xy", "lambda4" and "hits"."""
        rays, pix, lam = self.camera_rays_device(sample_index)
        hits = self.trace_device(rays)
        r = self.interactions_device(rays, hits)
        r.update(rays8=rays, pixel_xy=pix, lambda4=lam, hits=hits)
        return r

    @staticmethod
    def _planes(it, what):
        """(planes_f, planes_i, n) of an interactions_device dict, or of a (planes_f [11, n, 4], planes_i [2, n, 4]) pair a caller made"""
        import torch
        F, I = (it["planes_f"], it["planes_i"]) if isinstance(it, dict) else it
        if not (isinstance(F, torch.Tensor) and isinstance(I, torch.Tensor) and F.dtype == torch.float32 and I.dtype == torch.int32 and F.dim() == 3
                and I.dim() == 3 and F.shape[0] == INTR_FPLANES and I.shape[0] == INTR_IPLANES and F.shape[2] == 4 and I.shape[2] == 4
                and F.shape[1] == I.shape[1]):
            raise WfError("%s: it is the dict of interactions_device, or (planes_f float32 [%d, n, 4], planes_i int32 [%d, n, 4])" % (what, INTR_FPLANES, INTR_IPLANES))
        return F, I, F.shape[1]

    @staticmethod
    def _count_arg(n_device, what):
        import torch
        if n_device is not None and not (isinstance(n_device, torch.Tensor) and n_device.numel() == 1 and n_device.dtype == torch.int32):
            raise WfError("%s: n_device is an int32 tensor of one element" % what)
        return n_device

    def sample_lights_device(self, it, lambda4, u4, side=None, n_device=None, out=None):
        """wf_light_sample_device: the light half of next-event estimation for n device items, by the render's own light sampler and
        lights.  it: the dict of interactions_device / first_hit (or its two plane tensors); lambda4 float32 [n, 4]; u4 float32 [n, 4]
        rows {uc, u[0], u[1], unused}; side int32 [n] (None: all 0): 0 the light sees the position interval, +1 the point offset along
        wo (a BSDF that only reflects), -1 the point offset against wo (one that reflects and transmits).  Returns a dict of views:
        "shadow_rays8" float32 [n, 8] (ready for trace_device(any_hit=True) / trace_shadow_tr_device; d is not normalised), "L" float32
        [n, 4], "wi" float32 [n, 3], "pdf" float32 [n] (of the direction), "pmf" float32 [n] (of the light), "light" int32 [n] (-1:
        none), "flags" int32 [n] (bit 0: a delta light), "medium" int32 [n], and the tensors themselves as "L4", "wi_pdf4", "light4".
        A row the render would not take to its BSDF has L = 0, pdf = 0 and a zero ray.  n_device: an int32 tensor of one element;
        only the first min(n, n_device) rows are written.  out: the dict of an earlier call with the same n, written into again."""
        import torch
        _, hip = libs()
        F, I, n = self._planes(it, "sample_lights_device")
        self._as(lambda4, torch.float32, 4, "sample_lights_device lambda4")
        self._as(u4, torch.float32, 4, "sample_lights_device u4")
        if side is not None:
            self._as(side, torch.int32, 0, "sample_lights_device side")
        if any(t.shape[0] != n for t in (lambda4, u4) + ((side,) if side is not None else ())):
            raise WfError("sample_lights_device: the arrays hold different numbers of items")
        self._count_arg(n_device, "sample_lights_device")
        dev = F.device
        if out is None:
            rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
            L4 = torch.empty((n, 4), dtype=torch.float32, device=dev)
            wp = torch.empty((n, 4), dtype=torch.float32, device=dev)
            li = torch.empty((n, 4), dtype=torch.int32, device=dev)
        else:
            rays, L4, wp, li = out["shadow_rays8"], out["L4"], out["wi_pdf4"], out["light4"]
            if rays.shape != (n, 8) or L4.shape != (n, 4) or wp.shape != (n, 4) or li.shape != (n, 4):
                raise WfError("sample_lights_device: out is the dict of a call with the same number of items")
        r = {"shadow_rays8": rays, "L4": L4, "wi_pdf4": wp, "light4": li, "L": L4, "wi": wp[:, :3], "pdf": wp[:, 3], "light": li[:, 0],
             "pmf": li[:, 1].view(torch.float32), "flags": li[:, 2], "medium": li[:, 3]}
        if n == 0:
            return r
        ts = [F, I, lambda4, u4, rays, L4, wp, li] + [t for t in (side, n_device) if t is not None]
        self._device_call("wf_light_sample_device", hip.wf_light_sample_device, [C.c_void_p, C.c_int] + [C.c_void_p] * 10, ts, n,
                          n_device.data_ptr() if n_device is not None else None, F.data_ptr(), I.data_ptr(), lambda4.data_ptr(), u4.data_ptr(),
                          side.data_ptr() if side is not None else None, rays.data_ptr(), L4.data_ptr(), wp.data_ptr(), li.data_ptr())
        return r

    def emitted_device(self, rays8, it, lambda4, infinite_index=0, prev=None, out=None, n_device=None):
        """wf_light_emitted_device: the emission at the end of n device rays — rays8 float32 [n, 8], `it` the interactions of their hits
        (as sample_lights_device takes them), lambda4 float32 [n, 4].  A hit row on an emitter gets the emitter's radiance towards the
        ray's origin (for infinite_index 0 only), a miss row the radiance of the scene's infinite light number infinite_index
        (query("infinite_lights") of them: sum the calls).  prev: the interactions of the vertices the rays LEFT (a dict of
        interactions_device, or a float32 [>= 4, n, 4] tensor of planes 0 - 3): with it the rows also get the light sampler's
        probability of the light and the PDF of the ray's direction, both as seen from that vertex — the two factors of the MIS
        weight.  Returns a dict of views: "Le" float32 [n, 4], "pmf" float32 [n], "pdf" float32 [n], and "Le4", "pmf_pdf4"."""
        import torch
        _, hip = libs()
        self._as(rays8, torch.float32, 8, "emitted_device rays8")
        F, I, n = self._planes(it, "emitted_device")
        self._as(lambda4, torch.float32, 4, "emitted_device lambda4")
        if rays8.shape[0] != n or lambda4.shape[0] != n:
            raise WfError("emitted_device: the arrays hold different numbers of items")
        P = None
        if prev is not None:
            P = prev["planes_f"] if isinstance(prev, dict) else prev
            if not (isinstance(P, torch.Tensor) and P.dtype == torch.float32 and P.dim() == 3 and P.shape[0] >= 4 and P.shape[1] == n and P.shape[2] == 4):
                raise WfError("emitted_device: prev is a dict of interactions_device or a float32 [>= 4, n, 4] tensor of planes")
        self._count_arg(n_device, "emitted_device")
        if out is None:
            Le = torch.empty((n, 4), dtype=torch.float32, device=F.device)
            pp = torch.empty((n, 4), dtype=torch.float32, device=F.device)
        else:
            Le, pp = out["Le4"], out["pmf_pdf4"]
            if Le.shape != (n, 4) or pp.shape != (n, 4):
                raise WfError("emitted_device: out is the dict of a call with the same number of items")
        r = {"Le4": Le, "pmf_pdf4": pp, "Le": Le, "pmf": pp[:, 0], "pdf": pp[:, 1]}
        ts = [rays8, F, I, lambda4, Le, pp] + [t for t in (P, n_device) if t is not None]
        # (n = 0 still goes through: the index is checked)
        self._device_call("wf_light_emitted_device", hip.wf_light_emitted_device, [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 3, ts, n,
                          n_device.data_ptr() if n_device is not None else None, rays8.data_ptr(), F.data_ptr(), I.data_ptr(), lambda4.data_ptr(), int(infinite_index),
                          P.data_ptr() if P is not None else None, Le.data_ptr(), pp.data_ptr())
        return r

    def bsdf_device(self, rays8, it, lambda4, regularize=None, n_device=None):
        """wf_bsdf_make_device: the scene's BSDF at n device vertices — the MixMaterial choice, the textures, the normal or bump map and
        the material's BxDF, by the render's own functions.  rays8 float32 [n, 8]: the rays that found the hits (the mix choice hashes
        their direction); it: the dict of interactions_device / first_hit (or its two plane tensors); lambda4 float32 [n, 4];
        regularize int32 [n] (None: nowhere): non-zero where the caller's path has had a non-specular bounce and the scene regularises.
        Returns a dict: "rec" float32 [10, n, 4], opaque, for bsdf_eval_device; "bsdf4" int32 [n, 4] and its views "flags" (the
        BxDFFlags: 1 reflection, 2 transmission, 4 diffuse, 8 glossy, 16 specular), "side" (what sample_lights_device takes; 0 also
        where the BSDF is specular only and takes no light sample), "material" (after the mix resolve), "type" (0: the row has no
        BSDF — a miss, an interface surface — and is all zeros), "terminated" (bool: the material's dispersion terminated the
        secondary wavelengths — the caller zeroes lambda_pdf4[:, 1:] and divides lambda_pdf4[:, 0] by 4 unless they are zero already)."""
        import torch
        _, hip = libs()
        self._as(rays8, torch.float32, 8, "bsdf_device rays8")
        F, I, n = self._planes(it, "bsdf_device")
        self._as(lambda4, torch.float32, 4, "bsdf_device lambda4")
        if regularize is not None:
            self._as(regularize, torch.int32, 0, "bsdf_device regularize")
        if any(t.shape[0] != n for t in (rays8, lambda4) + ((regularize,) if regularize is not None else ())):
            raise WfError("bsdf_device: the arrays hold different numbers of items")
        self._count_arg(n_device, "bsdf_device")
        rec = torch.empty((BSDF_PLANES, n, 4), dtype=torch.float32, device=F.device)
        b4 = torch.empty((n, 4), dtype=torch.int32, device=F.device)
        r = {"rec": rec, "bsdf4": b4, "side": b4[:, 1], "material": b4[:, 2], "type": b4[:, 3]}
        if n > 0:
            ts = [rays8, F, I, lambda4, rec, b4] + [t for t in (regularize, n_device) if t is not None]
            self._device_call("wf_bsdf_make_device", hip.wf_bsdf_make_device, [C.c_void_p, C.c_int] + [C.c_void_p] * 8, ts, n,
                              n_device.data_ptr() if n_device is not None else None, rays8.data_ptr(), F.data_ptr(), I.data_ptr(), lambda4.data_ptr(),
                              regularize.data_ptr() if regularize is not None else None, rec.data_ptr(), b4.data_ptr())
        r["flags"] = b4[:, 0] & 0xff
        r["terminated"] = (b4[:, 0] & BSDF_TERMINATED) != 0
        r["ns"] = rec[1, :, :3]   # the final shading normal (after the normal / bump map): what light_planes() hands the lights
        return r

    def light_planes(self, it, bsdf):
        """The float planes of `it` with the BSDF's final shading normal in plane 3, where the row has a BSDF: the LightSampleContext
        the render samples its lights from (and keeps with the indirect ray for the MIS weights) carries the shading normal AFTER the
        normal or bump map, which only bsdf_device knows.  Pass (light_planes(it, bsdf), it["planes_i"]) to sample_lights_device and
        as `prev` to emitted_device; on a scene without normal and bump maps the planes are equal to it["planes_f"]."""
        import torch
        F, _, n = self._planes(it, "light_planes")
        out = F.clone()
        live = (bsdf["type"] != 0)[:, None]
        out[3, :, :3] = torch.where(live, bsdf["rec"][1, :, :3], F[3, :, :3])
        return out

    def bsdf_eval_device(self, bsdf, it, wi=None, u4=None, n_device=None):
        """wf_bsdf_eval_device: the BSDFs of bsdf_device (its dict, or the "rec" tensor) evaluated for given directions and / or
        sampled.  it: the interactions the BSDFs were made from.  wi float32 [n, 4] rows {wi, unused}: "f" float32 [n, 4] = bsdf.f(wo,
        wi), "pdf" float32 [n] = bsdf.PDF(wo, wi), "cos" float32 [n] = |wi . ns|.  u4 float32 [n, 4] rows {uc, u[0], u[1], unused}:
        bsdf.Sample_f — "sample_f" float32 [n, 4], "sample_pdf" float32 [n], "pdf_mis" float32 [n] (what the render divides r_u by:
        the BSDF's PDF where the sample's own is only proportional), "sample_cos" float32 [n], "eta" float32 [n], "sample_valid" /
        "sample_flags" / "next_medium" / "proportional" int32 [n], "next_rays8" float32 [n, 8] (ready for trace_device).  With these
        beta = sample_f * sample_cos / sample_pdf, r_l = r_u / pdf_mis and etaScale * eta ** 2 are the render's values.  An invalid
        sample and a row without a BSDF are zeros.  The tensors themselves: "f4", "pdf4", "sample_f4", "sample_pdf4", "sample_i4"."""
        import torch
        _, hip = libs()
        rec = bsdf["rec"] if isinstance(bsdf, dict) else bsdf
        F, I, n = self._planes(it, "bsdf_eval_device")
        if not (isinstance(rec, torch.Tensor) and rec.dtype == torch.float32 and rec.shape == (BSDF_PLANES, n, 4)):
            raise WfError("bsdf_eval_device: bsdf is the dict of bsdf_device or its float32 [%d, n, 4] record tensor, of the interactions' n" % BSDF_PLANES)
        if wi is None and u4 is None:
            raise WfError("bsdf_eval_device: give wi, u4 or both")
        for t, what in ((wi, "wi"), (u4, "u4")):
            if t is not None:
                self._as(t, torch.float32, 4, "bsdf_eval_device " + what)
                if t.shape[0] != n:
                    raise WfError("bsdf_eval_device: the arrays hold different numbers of items")
        self._count_arg(n_device, "bsdf_eval_device")
        dev = F.device
        r = {}
        ts = [rec, F, I]
        f4 = pdf4 = nxt = sf = sp = si = None
        if wi is not None:
            f4 = torch.empty((n, 4), dtype=torch.float32, device=dev)
            pdf4 = torch.empty((n, 4), dtype=torch.float32, device=dev)
            r.update(f4=f4, pdf4=pdf4, f=f4, pdf=pdf4[:, 0], cos=pdf4[:, 1])
            ts += [wi, f4, pdf4]
        if u4 is not None:
            nxt = torch.empty((n, 8), dtype=torch.float32, device=dev)
            sf = torch.empty((n, 4), dtype=torch.float32, device=dev)
            sp = torch.empty((n, 4), dtype=torch.float32, device=dev)
            si = torch.empty((n, 4), dtype=torch.int32, device=dev)
            r.update(next_rays8=nxt, sample_f4=sf, sample_pdf4=sp, sample_i4=si, sample_f=sf, sample_pdf=sp[:, 0], pdf_mis=sp[:, 1], sample_cos=sp[:, 2],
                     eta=sp[:, 3], sample_valid=si[:, 0], sample_flags=si[:, 1], next_medium=si[:, 2], proportional=si[:, 3])
            ts += [u4, nxt, sf, sp, si]
        if n == 0:
            return r
        if n_device is not None:
            ts.append(n_device)
        p = lambda t: t.data_ptr() if t is not None else None
        self._device_call("wf_bsdf_eval_device", hip.wf_bsdf_eval_device, [C.c_void_p, C.c_int] + [C.c_void_p] * 12, ts, n, p(n_device), rec.data_ptr(), F.data_ptr(),
                          I.data_ptr(), p(wi), p(u4), p(f4), p(pdf4), p(nxt), p(sf), p(sp), p(si))
        return r

    def medium_sample_device(self, rays8, medium, lambda4, beta, r_u, r_l, flags=None, n_device=None, out=None):
        """wf_medium_sample_device (include/wf_media.h): delta tracking along n device rays through the scene's media, by the render's
        own functions — absorb, scatter or null-collide, with the media's emission.  rays8 float32 [n, 8] rows {o, d, tMax, time} with
        tMax the closest hit's t (trace_device) or +inf; medium int32 [n] (-1: in no medium); lambda4, beta, r_u, r_l float32 [n, 4]
        (the path's state on entry); flags int32 [n] (None: all 1): bit 0 = collect the emission (the render's depth < maxDepth).
        Returns a dict: "event4" int32 [n, 4] and its views "kind" (MEDIUM_NONE 0: no row, all zeros; MEDIUM_ARRIVED 1: the ray reached
        tMax, go on to the hit or the escape; MEDIUM_ENDED 2: the path ended; MEDIUM_SCATTER 3: a real scatter at "p") and "steps" (the
        tentative collisions taken); "p_g4" float32 [n, 4] with views "p" [n, 3] and "g" [n]; "beta", "r_u", "r_l" float32 [n, 4]; "L"
        float32 [n, 4], the emission collected along the ray (add it to the pixel's L).  out: a dict with "beta", "r_u", "r_l" (and
        optionally the others) to write into — they may be the input tensors themselves: a row is read before it is written."""
        import torch
        _, hip = libs()
        what = "medium_sample_device"
        self._as(rays8, torch.float32, 8, what + " rays8")
        self._as(medium, torch.int32, 0, what + " medium")
        for t in (lambda4, beta, r_u, r_l):
            self._as(t, torch.float32, 4, what + " lambda4 / beta / r_u / r_l")
        if flags is not None:
            self._as(flags, torch.int32, 0, what + " flags")
        n = rays8.shape[0]
        if any(t.shape[0] != n for t in (medium, lambda4, beta, r_u, r_l) + ((flags,) if flags is not None else ())):
            raise WfError(what + ": the arrays hold different numbers of items")
        self._count_arg(n_device, what)
        dev = rays8.device
        out = dict(out) if out is not None else {}
        for k, dt in (("event4", torch.int32), ("p_g4", torch.float32), ("beta", torch.float32), ("r_u", torch.float32), ("r_l", torch.float32), ("L", torch.float32)):
            if k not in out:
                out[k] = torch.empty((n, 4), dtype=dt, device=dev)
            self._as(out[k], dt, 4, what + " out[%r]" % k)
            if out[k].shape[0] != n:
                raise WfError(what + ": out is the dict of a call with the same number of items")
        ev, pg = out["event4"], out["p_g4"]
        r = {"event4": ev, "p_g4": pg, "beta": out["beta"], "r_u": out["r_u"], "r_l": out["r_l"], "L": out["L"], "kind": ev[:, 0], "steps": ev[:, 1],
             "p": pg[:, :3], "g": pg[:, 3]}
        ts = [rays8, medium, lambda4, beta, r_u, r_l, ev, pg, r["beta"], r["r_u"], r["r_l"], r["L"]] + [t for t in (flags, n_device) if t is not None]
        p = lambda t: t.data_ptr() if t is not None else None
        # (n = 0 still goes through: a scene without media is refused)
        self._device_call("wf_medium_sample_device", hip.wf_medium_sample_device, [C.c_void_p, C.c_int] + [C.c_void_p] * 14, ts, n, p(n_device), rays8.data_ptr(),
                          medium.data_ptr(), lambda4.data_ptr(), beta.data_ptr(), r_u.data_ptr(), r_l.data_ptr(), p(flags), ev.data_ptr(), pg.data_ptr(),
                          r["beta"].data_ptr(), r["r_u"].data_ptr(), r["r_l"].data_ptr(), r["L"].data_ptr())
        return r

    def phase_device(self, rays8, p_g4, wi=None, u4=None, n_device=None):
        """wf_phase_device (include/wf_media.h): the Henyey-Greenstein phase function at the scatter points of medium_sample_device.
        rays8 float32 [n, 8]: the rays that scattered (wo = -d, and the time); p_g4 float32 [n, 4]: rows {p, g}.  wi float32 [n, 4]
        rows {wi, unused}: "p" float32 [n] = phase.p(wo, wi), "pdf" float32 [n] = phase.PDF(wo, wi).  u4 float32 [n, 4] rows {u[0],
        u[1], unused, unused}: phase.Sample_p — "sample_p", "sample_pdf" float32 [n], "next_rays8" float32 [n, 8] rows {p, wi, +inf, the
        row's time} (ready for trace_device; the next ray's medium is the one the ray was in).  A sample with pdf 0 is zeros.  The
        tensors themselves: "p_pdf4", "sample4".  Russian roulette and depth + 1 are the caller's."""
        import torch
        _, hip = libs()
        self._as(rays8, torch.float32, 8, "phase_device rays8")
        self._as(p_g4, torch.float32, 4, "phase_device p_g4")
        n = rays8.shape[0]
        if p_g4.shape[0] != n:
            raise WfError("phase_device: the arrays hold different numbers of items")
        if wi is None and u4 is None:
            raise WfError("phase_device: give wi, u4 or both")
        for t, what in ((wi, "wi"), (u4, "u4")):
            if t is not None:
                self._as(t, torch.float32, 4, "phase_device " + what)
                if t.shape[0] != n:
                    raise WfError("phase_device: the arrays hold different numbers of items")
        self._count_arg(n_device, "phase_device")
        dev = rays8.device
        r = {}
        ts = [rays8, p_g4]
        pp = sm = nxt = None
        if wi is not None:
            pp = torch.empty((n, 4), dtype=torch.float32, device=dev)
            r.update(p_pdf4=pp, p=pp[:, 0], pdf=pp[:, 1])
            ts += [wi, pp]
        if u4 is not None:
            sm = torch.empty((n, 4), dtype=torch.float32, device=dev)
            nxt = torch.empty((n, 8), dtype=torch.float32, device=dev)
            r.update(sample4=sm, next_rays8=nxt, sample_p=sm[:, 0], sample_pdf=sm[:, 1])
            ts += [u4, sm, nxt]
        if n_device is not None:
            ts.append(n_device)
        p = lambda t: t.data_ptr() if t is not None else None
        # (n = 0 still goes through: a scene without media is refused)
        self._device_call("wf_phase_device", hip.wf_phase_device, [C.c_void_p, C.c_int] + [C.c_void_p] * 8, ts, n, p(n_device), rays8.data_ptr(), p_g4.data_ptr(),
                          p(wi), p(u4), p(pp), p(sm), p(nxt))
        return r

    def medium_light_planes(self, p_g4, rays8, medium):
        """The (planes_f float32 [11, n, 4], planes_i int32 [2, n, 4]) of n medium vertices for sample_lights_device: the reference's
        LightSampleContext of a point in a medium — pi lower = pi upper = p, n = ns = 0 — with the ray's time in plane 2.w, valid = 1
        and medium inside = outside = the ray's medium (the shadow ray's medium either way).  p_g4: the scatter points of
        medium_sample_device; rays8: the rays that scattered; medium int32 [n]."""
        import torch
        self._as(p_g4, torch.float32, 4, "medium_light_planes p_g4")
        self._as(rays8, torch.float32, 8, "medium_light_planes rays8")
        self._as(medium, torch.int32, 0, "medium_light_planes medium")
        n = p_g4.shape[0]
        if rays8.shape[0] != n or medium.shape[0] != n:
            raise WfError("medium_light_planes: the arrays hold different numbers of items")
        F = torch.zeros((INTR_FPLANES, n, 4), dtype=torch.float32, device=p_g4.device)
        I = torch.zeros((INTR_IPLANES, n, 4), dtype=torch.int32, device=p_g4.device)
        F[0, :, :3] = p_g4[:, :3]
        F[1, :, :3] = p_g4[:, :3]
        F[2, :, 3] = rays8[:, 7]
        I[0, :, 0] = -1
        I[0, :, 1] = -1
        I[0, :, 2] = medium
        I[0, :, 3] = medium
        I[1, :, 0] = -1
        I[1, :, 1] = 1
        return F, I

    def bounds(self):
        """WavefrontAggregate::Bounds() in rendering space: (pMin[3], pMax[3])"""
        _, hip = libs()
        b = (C.c_float * 6)()
        _check(hip.wf_aggregate_bounds(self.ctx, b), "wf_aggregate_bounds")
        return np.array(b[:3], dtype=np.float32), np.array(b[3:], dtype=np.float32)

    def trace_any(self, o, d, tmax, reference_order=True):
        _, hip = libs()
        o = np.ascontiguousarray(o, dtype=np.float32)
        d = np.ascontiguousarray(d, dtype=np.float32)
        tmax = np.ascontiguousarray(tmax, dtype=np.float32)
        n = o.shape[0]
        occ = np.empty(n, dtype=np.int32)
        nodes = np.empty(n, dtype=np.int32)
        tris = np.empty(n, dtype=np.int32)
        _check(hip.wf_trace_any_host(self.ctx, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, occ.ctypes.data,
                                     nodes.ctypes.data if reference_order else None, tris.ctypes.data if reference_order else None),
               "wf_trace_any_host")
        return occ, nodes, tris

    def sampler_probe(self, px, py, sample_index, start_dim, ndims):
        _, hip = libs()
        px = np.ascontiguousarray(px, dtype=np.int32)
        py = np.ascontiguousarray(py, dtype=np.int32)
        si = np.ascontiguousarray(sample_index, dtype=np.int32)
        out = np.empty((px.shape[0], ndims if ndims > 0 else 30 if ndims == -3 else 2), dtype=np.float32)   # record sizes: include/wf_abi.h
        _check(hip.wf_sampler_probe(self.ctx, px.shape[0], px.ctypes.data, py.ctypes.data, si.ctypes.data, start_dim, ndims, out.ctypes.data),
               "wf_sampler_probe")
        return out

    LIBM_FNS = ("sin", "cos", "exp", "log", "atan", "asin", "acos", "cosh", "atanh", "atan2", "sinh", "tan")

    def libm_probe(self, fn, x):
        """Device evaluation of the kernels' elementary function `fn` over float32 array x ((n, 2) (y, x) pairs for atan2)."""
        _, hip = libs()
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.shape[0]
        out = np.empty(n, dtype=np.float32)
        _check(hip.wf_libm_probe(self.ctx, self.LIBM_FNS.index(fn), n, x.ctypes.data, out.ctypes.data), "wf_libm_probe")
        return out

    def material_items(self):
        """items the material stage evaluated since the last clear_film(): {material type: count}, plus "medium_sample" """
        _, hip = libs()
        out = (C.c_uint64 * 16)()
        _check(hip.wf_material_items_download(self.ctx, out), "wf_material_items_download")
        d = {i: int(out[i]) for i in range(11)}
        d["medium_sample"] = int(out[11])
        return d

    def kat_probe(self, records):
        """Device evaluation of the known-answer probe (csrc/common/wf_kat.h): (n, 16) uint64 records in, (n, 8) uint64 out."""
        _, hip = libs()
        records = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, 16)
        out = np.empty((records.shape[0], 8), dtype=np.uint64)
        _check(hip.wf_kat_probe(self.ctx, records.shape[0], records.ctypes.data, out.ctypes.data), "wf_kat_probe")
        return out

    def query(self, key):
        """wf_ctx_query: which kernel variants the uploaded scene runs ("fast_ok", "gen_mode", "defer_general", "anim_fast", "lean_type_2", ...)"""
        _, hip = libs()
        v = C.c_int64(0)
        hip.wf_ctx_query.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
        _check(hip.wf_ctx_query(self.ctx, key.encode(), C.byref(v)), "wf_ctx_query")
        return int(v.value)

    def fastbvh_check(self, n_rays=32, seed=1):
        """host-only self-check of the production traversal layout (wf_debug_fastbvh_check): needs no device.  Returns a dict."""
        host, hip = libs()
        out = (C.c_int64 * 8)()
        hip.wf_debug_fastbvh_check.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_int64)]
        rc = hip.wf_debug_fastbvh_check(host.wfh_scene_desc(self.h), n_rays, seed, out)
        if rc != 0:
            hip.wf_last_error.restype = C.c_char_p
            raise WfError("wf_debug_fastbvh_check: " + hip.wf_last_error().decode())
        keys = ["qnodes", "leaf_records", "entries", "nodes_visited", "true_hits", "missed", "tested", "entries_taken"]
        return dict(zip(keys, [int(v) for v in out]))

    def check_instances(self):
        """host-only range check of the instance tables (wf_scene_check_instances): needs no device.  Returns a dict."""
        host, hip = libs()
        out = (C.c_int64 * 4)()
        hip.wf_scene_check_instances.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        if hip.wf_scene_check_instances(host.wfh_scene_desc(self.h), out) != 0:
            hip.wf_last_error.restype = C.c_char_p
            raise WfError("wf_scene_check_instances: " + hip.wf_last_error().decode())
        return dict(zip(["bvh_prims", "top_level_instances", "nested_records", "nested_entries"], [int(v) for v in out]))

    def plan(self, key):
        """host-only form of query() (wf_scene_plan_query): which kernel variants an upload of this scene would choose under the current
        environment switches.  Needs no device and no renderer."""
        host, hip = libs()
        v = C.c_int64(0)
        hip.wf_scene_plan_query.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
        if hip.wf_scene_plan_query(host.wfh_scene_desc(self.h), key.encode(), C.byref(v)) != 0:
            raise WfError("wf_scene_plan_query: " + hip.wf_last_error().decode())
        return int(v.value)

    def enable_profile(self, on=True):
        _, hip = libs()
        _check(hip.wf_profile_enable(self.ctx, int(on)), "wf_profile_enable")   # 0 off, 1 every launch, 2 the Intersect* launches only

    def profile_report(self):
        _, hip = libs()
        ent = (ProfileEntry * 64)()
        n = C.c_int(0)
        _check(hip.wf_profile_report(self.ctx, ent, 64, C.byref(n)), "wf_profile_report")
        return [{"name": ent[i].name.decode(), "launches": ent[i].launches, "total_ms": ent[i].total_ms,
                 "min_ms": ent[i].min_ms, "max_ms": ent[i].max_ms} for i in range(n.value)]

    def enable_counters(self, on=True):
        _, hip = libs()
        _check(hip.wf_counters_enable(self.ctx, 1 if on else 0), "wf_counters_enable")

    def counters(self):
        _, hip = libs()
        c = TraversalCounters()
        _check(hip.wf_counters_download(self.ctx, C.byref(c)), "wf_counters_download")
        return {n: int(getattr(c, n)) for n, _ in TraversalCounters._fields_}

    def debug_counters(self, reset=True):
        """rare-path counters of the production traversal (wf_debug_counters): spilled stack entries, overflow flag,
        inline near-tie re-traces, cursor path taken"""
        _, hip = libs()
        out = (C.c_uint64 * 4)()
        hip.wf_debug_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        _check(hip.wf_debug_counters(self.ctx, out, 1 if reset else 0), "wf_debug_counters")
        return {"spilled_entries": int(out[0]), "overflow": int(out[1]), "inline_retraces": int(out[2]), "cursor": int(out[3])}

    # ---- the film developed on the device (wf_film_develop_device): the image as a torch tensor, no host round trip ----
    def _develop(self, what, rgb_only, channels, out):
        import torch
        host, hip = libs()
        dev = torch.device("cuda", self.device)
        shape = (self.info.height, self.info.width, channels)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
            raise WfError("%s: out is a contiguous float32 tensor of shape %s on %s" % (what, list(shape), dev))
        # the kernel runs on the context's stream (wf_stream), behind the render and behind whatever torch's stream still does with `out`
        torch.cuda.ExternalStream(hip.wf_stream(self.ctx), device=dev).wait_stream(torch.cuda.current_stream(dev))
        nan = C.c_uint64(0)
        if host.wfh_film_image_device(self.h, out.data_ptr(), out.numel(), 1 if rgb_only else 0, C.byref(nan)) != 0:
            raise WfError("%s failed: %s" % (what, host.wfh_last_error().decode(errors="replace")))
        _check(hip.wf_sync(self.ctx), "wf_sync")   # torch's stream is not the context's: the image is complete when the call returns
        self.nan_values = int(nan.value)
        return out

    def image_tensor(self, out=None):
        """image() developed on the device: a float32 [H, W, 3] torch tensor on the renderer's device, bit-identical with image().
        out: a tensor to write into instead of a new one.  Sets self.nan_values (NaN values stored as 0)."""
        if not self._renderer:
            raise WfError("image_tensor: create_renderer() first")
        return self._develop("image_tensor", True, 3, out)

    def film_channels_tensor(self, out=None):
        """film_channels() developed on the device: (channel names, float32 [H, W, C] torch tensor on the renderer's device), bit-identical
        with film_channels(); (["R", "G", "B"], image_tensor()) for an RGB film.  Sets self.nan_values."""
        if not self._renderer:
            raise WfError("film_channels_tensor: create_renderer() first")
        host, hip = libs()
        nc = C.c_int(0)
        _check(hip.wf_film_channel_count(self.ctx, C.byref(nc)), "wf_film_channel_count")
        if nc.value == 3:   # an RGB film (wfh_film_channels names the channels of the other two)
            return ["R", "G", "B"], self._develop("film_channels_tensor", False, 3, out)
        host.wfh_film_channels.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_char_p, C.c_void_p]
        names = C.create_string_buffer(32 * nc.value)
        n32 = C.c_int32(0)
        if host.wfh_film_channels(self.h, C.byref(n32), names, None) != 0 or n32.value != nc.value:
            raise WfError("film_channels_tensor: " + host.wfh_last_error().decode(errors="replace"))
        return ([names.raw[32 * i:32 * (i + 1)].split(b"\0")[0].decode() for i in range(nc.value)],
                self._develop("film_channels_tensor", False, nc.value, out))

    def film_to_tensor(self, tensor):
        """device-to-device copy of the film accumulators into a torch CUDA float64 tensor (for the RCCL reduce)"""
        _, hip = libs()
        _check(hip.wf_film_copy_to_device(self.ctx, C.c_void_p(tensor.data_ptr())), "wf_film_copy_to_device")

    def film_from_tensor(self, tensor):
        _, hip = libs()
        _check(hip.wf_film_copy_from_device(self.ctx, C.c_void_p(tensor.data_ptr())), "wf_film_copy_from_device")

    def close(self):
        host, _ = libs()
        if self.h:
            host.wfh_scene_free(self.h)
            self.h = None


def write_pfm(path, rgb):
    host, _ = libs()
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    if host.wfh_write_image(os.fsencode(path), rgb.ctypes.data, rgb.shape[1], rgb.shape[0]) != 0:
        raise WfError("could not write %s" % path)


def read_image(path, encoding=None):
    """Image::Read through the host library (.pfm, .png, .exr): (float32 array [h][w][nc], storage format 0 8-bit / 1 half / 2 float)."""
    host, _ = libs()
    w, h, nc, fmt = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    enc = None if encoding is None else encoding.encode()
    if host.wfh_read_image(os.fsencode(path), enc, C.byref(w), C.byref(h), C.byref(nc), C.byref(fmt), None) != 0:
        raise WfError(host.wfh_last_error().decode())
    px = np.empty((h.value, w.value, nc.value), np.float32)
    if host.wfh_read_image(os.fsencode(path), enc, None, None, None, None, px.ctypes.data) != 0:
        raise WfError(host.wfh_last_error().decode())
    return px, fmt.value


def read_nanovdb(path, grid_name):
    """The float grid `grid_name` of a NanoVDB file through the host library's own reader (parity unpinned): None if the file has no
    such grid, else dict(min, dim, inv_mat, vec, background, values[z][y][x])."""
    host, _ = libs()
    mn, dm = (C.c_int32 * 3)(), (C.c_int32 * 3)()
    inv, vec, bg = (C.c_float * 9)(), (C.c_float * 3)(), C.c_float()
    host.wfh_read_nanovdb.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = host.wfh_read_nanovdb(os.fsencode(path), grid_name.encode(), mn, dm, inv, vec, C.byref(bg), None)
    if rc == 1:
        return None
    if rc != 0:
        raise WfError(host.wfh_last_error().decode(errors="replace"))
    vals = np.empty((dm[2], dm[1], dm[0]), np.float32)
    if host.wfh_read_nanovdb(os.fsencode(path), grid_name.encode(), mn, dm, inv, vec, C.byref(bg), vals.ctypes.data) != 0:
        raise WfError(host.wfh_last_error().decode(errors="replace"))
    return {"min": list(mn), "dim": list(dm), "inv_mat": list(inv), "vec": list(vec), "background": bg.value, "values": vals}


def read_pfm(path):
    with open(path, "rb") as f:
        magic = f.readline().strip()
        if magic not in (b"PF", b"Pf"):
            raise WfError("%s: not a PFM file" % path)
        w, h = map(int, f.readline().split())
        scale = float(f.readline())
        nc = 3 if magic == b"PF" else 1
        data = np.frombuffer(f.read(), dtype="<f4" if scale < 0 else ">f4").reshape(h, w, nc)
    return data[::-1].astype(np.float32)
