"""What the GPU tests of the device-buffer boundary share (test_device_trace_gpu, test_interaction_device_gpu, test_film_add_gpu,
test_film_develop_gpu, test_light_device_gpu, test_bsdf_device_gpu, test_transmittance_wavefront_anim_gpu): the fixture that brings the
library's HIP runtime up before torch's, scenes opened as one band, seeded device inputs, bit-for-bit comparisons, the description's
light and material tables, the render's stages driven one by one through the C ABI, and the round trip through a host checker's --eval.
A plain module: a test module imports what it uses by name (the fixture too: it then is module-scoped and autouse there)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

DIFFUSE, CONDUCTOR, DIELECTRIC, THIN_DIELECTRIC, DIFFUSE_TRANSMISSION, COATED_DIFFUSE, COATED_CONDUCTOR = range(1, 8)
# the LightSampleContext's side by the material's BSDF (surfscatter.cpp:256-261): reflective only +1, reflective and transmissive -1
SIDE_OF = {DIFFUSE: 1, CONDUCTOR: 1, COATED_DIFFUSE: 1, COATED_CONDUCTOR: 1, DIELECTRIC: -1, THIN_DIELECTRIC: -1, DIFFUSE_TRANSMISSION: -1}
MATERIAL_WORDS, LIGHT_WORDS = 25, 25   # sizeof(wf_material) / 4, sizeof(wf_light) / 4; word 0 = type, word 4 of a light = tri


@pytest.fixture(scope="module", autouse=True)
def renderer_before_torch(wfpt):
    """The library's HIP runtime comes up (a first renderer) before this module imports torch, which brings a runtime of its own: the
    order every test of the device-buffer calls has (scene first, tensors second), also when this file runs alone."""
    s = wfpt.Scene(path=os.path.join(GOLDEN, "cornell64.pbrt"), spp=4)
    s.create_renderer(0)
    s.close()


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _f32_bits(a):
    """the words of the values as float32 (a float32 array: its own words)"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_rows_equal(got, want, keys, what):
    """got[k] (a tensor or an array) and want[k] hold the same words, for every k of keys: [n][cols] arrays, or [plane][n][4] ones, whose
    row i is column i of every plane"""
    for k in keys:
        g, w = got[k] if isinstance(got[k], np.ndarray) else _np(got[k]), want[k]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        planes = g.ndim == 3
        differ = _bits(g) != _bits(w)
        bad = np.nonzero(differ.any(axis=(0, 2)) if planes else differ.reshape(g.shape[0], -1).any(axis=1))[0]
        first = (g[:, bad[0]], w[:, bad[0]]) if bad.size and planes else (g[bad[0]], w[bad[0]]) if bad.size else None
        assert bad.size == 0, "%s: %s differs in %d of %d rows, first row %d: %r" % (what, k, bad.size, g.shape[-2] if planes else g.shape[0], bad[0], first)


def open_scene(wfpt, name, spp=4, text=None):
    s = wfpt.Scene(path=os.path.join(GOLDEN, name + ".pbrt"), spp=spp) if text is None else wfpt.Scene(text=text, spp=spp)
    s.create_renderer(0, samples_per_pass=1)
    assert s.query("pixels_per_pass") == s.width * s.height   # the image is one band
    return s


def seeded(n, cols, seed, dev):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, cols), generator=g, dtype=torch.float32).to(dev)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rays8(o, d, tmax, time):
    return np.concatenate([o, d, tmax[:, None], time[:, None]], axis=1).astype(np.float32)


def _shadow_rays(lo, hi, n, seed, n_media):
    rng = np.random.RandomState(seed)
    o = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    to = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = (to - o).astype(np.float32)
    tmax = np.full(n, 0.9999, dtype=np.float32)
    medium = rng.randint(-1, n_media, size=n).astype(np.int32)
    lam = np.sort(rng.uniform(380, 780, size=(n, 4)), axis=1).astype(np.float32)
    Ld = rng.uniform(0.1, 2, size=(n, 4)).astype(np.float32)
    ones = np.ones((n, 4), dtype=np.float32)
    return o, d, tmax, medium, lam, Ld, ones, ones.copy()


def _tr_device(s, rays, time):
    o, d, tmax, medium, lam, Ld, r_u, r_l = rays
    return s.trace_shadow_tr_device(_dev(_rays8(o, d, tmax, time)), _dev(medium), _dev(lam), _dev(Ld), _dev(r_u), _dev(r_l)).cpu().numpy()


def _launch_names(s):
    return {e["name"] for e in s.profile_report() if e["launches"] > 0}


def eval_on_host(program, options, scene_path, parts, tmp):
    """A host checker's --eval: the parts written one behind the other as in.bin, the program run on the scene, out.bin's bytes"""
    a, b = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(a, "wb") as f:
        for x in parts:
            f.write(np.ascontiguousarray(x).tobytes())
    subprocess.run([program] + list(options) + ["--eval", scene_path, a, b], check=True, capture_output=True)
    return open(b, "rb").read()


class DescLights(C.Structure):   # the leading members of wf_scene_desc, up to the light table
    _fields_ = [("abi_version", C.c_int32), ("n_vertices", C.c_int32), ("n_triangles", C.c_int32), ("n_meshes", C.c_int32), ("n_bvh_nodes", C.c_int32),
                ("P", C.c_void_p), ("N", C.c_void_p), ("UV", C.c_void_p), ("tri_indices", C.c_void_p), ("tri_mesh", C.c_void_p), ("meshes", C.c_void_p),
                ("bvh_nodes", C.c_void_p), ("bvh_prims", C.c_void_p), ("scene_bounds", C.c_float * 6),
                ("n_spectra", C.c_int32), ("n_spectrum_floats", C.c_int32), ("n_textures", C.c_int32), ("n_materials", C.c_int32),
                ("spectra", C.c_void_p), ("spectrum_data", C.c_void_p), ("textures", C.c_void_p), ("materials", C.c_void_p),
                ("n_lights", C.c_int32), ("n_infinite_lights", C.c_int32), ("n_light_bvh_nodes", C.c_int32), ("n_light_transforms", C.c_int32),
                ("lights", C.c_void_p), ("infinite_lights", C.c_void_p)]


def tables(wfpt, s):
    """(type of every light, tri of every light, type of every material, n_triangles, flags of every light) from the description the
    host library built"""
    host, _ = wfpt.libs()
    h = DescLights.from_address(host.wfh_scene_desc(s.h))
    lights = np.ctypeslib.as_array((C.c_int32 * (LIGHT_WORDS * max(h.n_lights, 1))).from_address(h.lights)).reshape(-1, LIGHT_WORDS)[:h.n_lights].copy() \
        if h.n_lights else np.zeros((0, LIGHT_WORDS), np.int32)
    mats = np.ctypeslib.as_array((C.c_int32 * (MATERIAL_WORDS * h.n_materials)).from_address(h.materials)).reshape(-1, MATERIAL_WORDS)[:, 0].copy()
    assert h.n_lights == s.query("lights") and h.n_infinite_lights == s.query("infinite_lights")
    return lights[:, 0], lights[:, 4], mats, h.n_triangles, lights[:, 1]


# ---- the render's stages through the C ABI ----------------------------------------------------------------------------------------------
def download(wfpt, s, queue, member, n, dtype, cols):
    _, hip = wfpt.libs()
    hip.wf_queue_download.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_uint64]
    a = np.empty((n, cols), dtype)
    if n:
        wfpt._check(hip.wf_queue_download(s.ctx, queue.encode(), member.encode(), a.ctypes.data, a.nbytes), "wf_queue_download")
    return a


def queue_size(wfpt, s, queue):
    _, hip = wfpt.libs()
    hip.wf_queue_size.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
    v = C.c_int(0)
    wfpt._check(hip.wf_queue_size(s.ctx, queue.encode(), C.byref(v)), "wf_queue_size")
    return v.value


def stage(wfpt, s, name, *args):
    _, hip = wfpt.libs()
    f = getattr(hip, name)
    f.argtypes = [C.c_void_p] + [C.c_int] * len(args)
    wfpt._check(f(s.ctx, *args), name)


def begin_pass(wfpt, s):
    """the unfused order of the render's pass (csrc/host/integrator.cpp), sample index 0, up to depth 0's closest hits"""
    stage(wfpt, s, "wf_set_pass_samples", 1, 1)
    stage(wfpt, s, "wf_reset_ray_queue", 0)
    stage(wfpt, s, "wf_gen_camera_rays", s.info.y0, 0)
    stage(wfpt, s, "wf_reset_stage_queues", 0)
    stage(wfpt, s, "wf_gen_ray_samples", 0, 0)
    stage(wfpt, s, "wf_intersect_closest", 0)


def emission(wfpt, s, depth):
    stage(wfpt, s, "wf_handle_escaped", depth)
    stage(wfpt, s, "wf_handle_emissive", depth)
    stage(wfpt, s, "wf_sync")


def shade(wfpt, s, depth, mats):
    for t in sorted(set(int(m) for m in mats) - {0, 11}):
        stage(wfpt, s, "wf_eval_material", t, depth)
    stage(wfpt, s, "wf_sync")


def average(x):
    """S4::Average (wf_math.h): s = v0; s += v1; s += v2; s += v3; s / 4"""
    s = x[:, 0]
    s = s + x[:, 1]
    s = s + x[:, 2]
    s = s + x[:, 3]
    return (s / 4)[:, None]


class Camera:
    """the camera samples of sample index 0, their first hits, and the row of every pixel index"""

    def __init__(self, wfpt, s):
        import torch
        self.rays, self.pix, self.lam, self.pdf, self.cam_w, self.fw = s.camera_samples_device(0)
        self.hits = s.trace_device(self.rays)
        self.it = s.interactions_device(self.rays, self.hits)
        torch.cuda.synchronize()
        xy = _np(self.pix)
        self.pixel_index = (xy[:, 1].astype(np.int64) - s.info.y0) * s.width + xy[:, 0]
        assert len(np.unique(self.pixel_index)) == len(xy) == s.width * s.height
        self.row_of = np.full(s.width * s.height, -1, np.int64)
        self.row_of[self.pixel_index] = np.arange(len(xy))
