"""wf_light_sample_device and wf_light_emitted_device on the MI355X: the scene's lights on a caller's device items.

Everything is bit for bit.  The expected values come from three independent places: the host program light_sample_check --eval (the
render's own light functions composed directly, on the host), the render's own stages driven through the C ABI (depth-0 emission, the
shadow queue of next-event estimation, the depth-1 MIS weights), and the calls themselves on other shapes of the same input."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from boundary_helpers import (SIDE_OF, Camera, DescLights, _bits, _np, assert_rows_equal, average, begin_pass, download, emission, eval_on_host, open_scene,
                              queue_size, renderer_before_torch, same, seeded, shade, stage, tables)  # noqa: F401 (the fixture)
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

CHECK = os.path.join(ROOT, "pbrt-v4_amd", "_build", "light_sample_check")
FIXTURES = ["cornell64", "materials_lights", "materials_lights_power", "envmap", "lights_extra", "portal_light", "portal_uniform", "quadrics",
            "bilinear_lights", "arealight_image", "arealight_alpha"]
POINT, DISTANT, SPOT, AREA, UNIFORM_INF, IMAGE_INF, GONIO, PROJECTION, PORTAL = range(9)
# the light types each fixture is here for: one of every set must be among the lights the sample call chose
TYPES = {"cornell64": [{AREA}], "materials_lights": [{POINT}, {DISTANT}, {SPOT}, {AREA}, {UNIFORM_INF, IMAGE_INF}],
         "materials_lights_power": [{POINT}, {DISTANT}, {SPOT}, {AREA}, {UNIFORM_INF, IMAGE_INF}], "envmap": [{IMAGE_INF}],
         "lights_extra": [{POINT}, {GONIO}, {PROJECTION}], "portal_light": [{PORTAL}, {POINT}], "portal_uniform": [{PORTAL}, {POINT}],
         "quadrics": [{AREA}, {POINT}, {UNIFORM_INF, IMAGE_INF}], "bilinear_lights": [{AREA}], "arealight_image": [{AREA}, {UNIFORM_INF, IMAGE_INF}],
         "arealight_alpha": [{AREA}]}
NON_TRIANGLE_EMITTERS = ("quadrics", "bilinear_lights")
SPECULAR_BOUNCE = 1

TWO_SKIES = """
LookAt 0 1 -6   0 1 0   0 1 0
Camera "perspective" "float fov" [ 45 ]
Sampler "zsobol" "integer pixelsamples" [ 4 ]
Integrator "volpath" "integer maxdepth" [ 5 ]
Film "rgb" "string filename" [ "two_skies.pfm" ] "integer xresolution" [ 48 ] "integer yresolution" [ 40 ] "bool savefp16" [ false ]
WorldBegin
LightSource "infinite" "rgb L" [ 0.4 0.5 0.9 ]
LightSource "infinite" "rgb L" [ 0.3 0.1 0.05 ] "float scale" [ 2 ]
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ 9 7 3 ] "bool twosided" [ true ]
  Material "diffuse" "rgb reflectance" [ 0.5 0.5 0.5 ]
  Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -0.5 1.5 1  0.5 1.5 1  0.5 2.5 1  -0.5 2.5 1 ]
AttributeEnd
Material "diffuse" "rgb reflectance" [ 0.6 0.6 0.6 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -3 0 -1  3 0 -1  3 0 4  -3 0 4 ]
"""


def eval_host(name_or_path, call, planes_f, planes_i, lam, u4=None, side=None, rays=None, prev=None, index=0, tmp=None):
    """light_sample_check --eval on downloaded inputs -> the expected outputs (numpy)"""
    n = planes_f.shape[1]
    path = name_or_path if os.path.sep in name_or_path else os.path.join(GOLDEN, name_or_path + ".pbrt")
    head = np.array([0x4c534331, call, n, index, int(side is not None), int(prev is not None), 0, 0], np.int32)
    parts = [head, planes_f.astype(np.float32), planes_i.astype(np.int32), lam.astype(np.float32)]
    parts += [u4.astype(np.float32)] + ([side.astype(np.int32)] if side is not None else []) if call == 0 else \
        [rays.astype(np.float32)] + ([prev[:4].astype(np.float32)] if prev is not None else [])
    raw = eval_on_host(CHECK, [], path, parts, tmp)
    if call == 0:
        assert len(raw) == n * 80
        return {"shadow_rays8": np.frombuffer(raw, np.float32, n * 8).reshape(n, 8), "L4": np.frombuffer(raw, np.float32, n * 4, n * 32).reshape(n, 4),
                "wi_pdf4": np.frombuffer(raw, np.float32, n * 4, n * 48).reshape(n, 4), "light4": np.frombuffer(raw, np.int32, n * 4, n * 64).reshape(n, 4)}
    assert len(raw) == n * 32
    return {"Le4": np.frombuffer(raw, np.float32, n * 4).reshape(n, 4), "pmf_pdf4": np.frombuffer(raw, np.float32, n * 4, n * 16).reshape(n, 4)}


SAMPLE_KEYS = ("shadow_rays8", "L4", "wi_pdf4", "light4")
EMITTED_KEYS = ("Le4", "pmf_pdf4")


# ---- 1: against the host oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_both_calls_equal_the_host_composition(wfpt, name, tmp_path):
    import torch
    dev = torch.device("cuda", 0)
    s = open_scene(wfpt, name)
    light_type, light_tri, _, n_tris, light_flags = tables(wfpt, s)
    fh = s.first_hit(0)
    n = fh["rays8"].shape[0]
    u4 = seeded(n, 4, 1234, dev)
    side = (torch.arange(n, dtype=torch.int32, device=dev) % 3 - 1).contiguous()
    out = s.sample_lights_device(fh, fh["lambda4"], u4, side)
    torch.cuda.synchronize()
    pf, pi, lam = _np(fh["planes_f"]), _np(fh["planes_i"]), _np(fh["lambda4"])
    want = eval_host(name, 0, pf, pi, lam, u4=_np(u4), side=_np(side), tmp=str(tmp_path))
    assert_rows_equal(out, want, SAMPLE_KEYS, name + " sample")
    # the views name the same words
    assert same(_np(out["pdf"]), want["wi_pdf4"][:, 3]) and same(_np(out["light"]), want["light4"][:, 0])
    assert same(_bits(_np(out["pmf"])), _bits(want["light4"][:, 1]))
    # the light types this fixture is here for were chosen
    ids = _np(out["light"])
    valid = _np(fh["valid"])
    assert (ids[valid != 1] == -1).all() and (valid == 1).any()
    chosen = set(light_type[ids[ids >= 0]].tolist())
    for group in TYPES[name]:
        assert chosen & group, (name, "no light of types", group, "among", chosen)
    if name in NON_TRIANGLE_EMITTERS:
        assert (light_tri[ids[ids >= 0]] >= n_tris).any()
    usable = _np(out["pdf"]) != 0
    assert usable.any() and (~usable).any() if (valid != 1).any() else usable.any()
    assert not _np(out["shadow_rays8"])[~usable].any() and not _np(out["L"])[~usable].any()
    delta = np.isin(light_type, (POINT, DISTANT, SPOT, GONIO, PROJECTION)) | ((light_flags & 2) != 0)   # IsDeltaLight
    assert (_np(out["flags"])[ids >= 0] == delta[ids[ids >= 0]]).all()

    # emitted: the usable shadow directions, traced to their ends
    rows = torch.nonzero(out["pdf"] != 0).flatten()
    rays = out["shadow_rays8"][rows].clone()
    rays[:, 6] = float("inf")
    hits = s.trace_device(rays)
    it = s.interactions_device(rays, hits)
    prev = fh["planes_f"][:, rows].contiguous()
    lam2 = fh["lambda4"][rows].contiguous()
    torch.cuda.synchronize()
    v2 = _np(it["valid"])
    n_inf = s.query("infinite_lights")
    assert (v2 == 1).any()
    if n_inf > 0:
        assert (v2 == 0).any(), "no ray of %s escapes" % name
    emitting = with_pdf = 0
    for k in range(max(1, n_inf)):
        for with_prev in (False, True):
            got = s.emitted_device(rays, it, lam2, infinite_index=k, prev=prev if with_prev else None)
            torch.cuda.synchronize()
            exp = eval_host(name, 1, _np(it["planes_f"]), _np(it["planes_i"]), _np(lam2), rays=_np(rays), prev=_np(prev) if with_prev else None, index=k,
                            tmp=str(tmp_path))
            assert_rows_equal(got, exp, EMITTED_KEYS, "%s emitted, index %d, prev %d" % (name, k, with_prev))
            emitting += int(_np(got["Le"]).any(axis=1).sum())
            with_pdf += int((_np(got["pdf"]) != 0).sum())
            if not with_prev:
                assert not _np(got["pmf_pdf4"]).any()
    if chosen & {AREA, UNIFORM_INF, IMAGE_INF}:
        assert emitting > 0
    if chosen & {AREA, IMAGE_INF}:
        assert with_pdf > 0
    s.close()


# ---- 2: depth-0 emission ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell64", "envmap", "quadrics", "arealight_image", "portal_light", "two_skies"])
def test_emitted_sums_to_the_renders_depth0_emission(wfpt, name):
    import torch
    s = open_scene(wfpt, name, text=TWO_SKIES if name == "two_skies" else None)
    n_pix = s.width * s.height
    n_inf = s.query("infinite_lights")
    if name == "two_skies":
        assert n_inf == 2 and s.query("lights") == 4
    cam = Camera(wfpt, s)
    assert (_np(cam.cam_w) == 1).all()
    total = torch.zeros((n_pix, 4), dtype=torch.float32, device=cam.rays.device)
    hit_emission = 0
    for k in range(max(1, n_inf)):
        e = s.emitted_device(cam.rays, cam.it, cam.lam, infinite_index=k)
        if k > 0:
            assert not _np(e["Le"])[_np(cam.it["valid"]) == 1].any()     # the hit rows' emission is in the k = 0 term alone
        else:
            hit_emission = int(_np(e["Le"])[_np(cam.it["valid"]) == 1].any(axis=1).sum())
        total = total + e["Le"]
    begin_pass(wfpt, s)
    assert (download(wfpt, s, "ray0", "beta", n_pix, np.float32, 4) == 1).all() and (download(wfpt, s, "ray0", "r_u", n_pix, np.float32, 4) == 1).all()
    emission(wfpt, s, 0)
    L = download(wfpt, s, "pixel", "L", n_pix, np.float32, 4)
    got = _np(total)
    assert L.any()
    assert same(_bits(L[cam.pixel_index]), _bits(got)), int((_bits(L[cam.pixel_index]) != _bits(got)).any(axis=1).sum())
    if name in ("cornell64", "quadrics", "arealight_image", "two_skies"):
        assert hit_emission > 0, "no emitter in view"
    if n_inf:
        assert got[_np(cam.it["valid"]) == 0].any()
    s.close()


# ---- 3: the shadow queue of next-event estimation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell64", "materials_lights", "materials_lights_power", "lights_extra", "portal_uniform", "quadrics"])
def test_sample_rows_equal_the_renders_shadow_queue(wfpt, name):
    import torch
    dev = torch.device("cuda", 0)
    s = open_scene(wfpt, name)
    assert s.plan("tr_route") == -1   # no media: the pass below has no medium stage
    _, _, mat_type, _, _ = tables(wfpt, s)
    n_pix = s.width * s.height
    cam = Camera(wfpt, s)
    begin_pass(wfpt, s)
    assert (download(wfpt, s, "ray0", "r_u", n_pix, np.float32, 4) == 1).all()
    emission(wfpt, s, 0)
    shade(wfpt, s, 0, mat_type)
    m = queue_size(wfpt, s, "shadow")
    assert m > 0
    so, sd, sr_l = (download(wfpt, s, "shadow", k, m, np.float32, 4) for k in ("o", "d", "r_l"))
    samples0 = download(wfpt, s, "pixel", "samples0", n_pix, np.float32, 4)
    item_pixel = sd[:, 3].copy().view(np.int32).astype(np.int64)
    assert len(np.unique(item_pixel)) == m and (item_pixel >= 0).all() and (item_pixel < n_pix).all()
    rows = cam.row_of[item_pixel]
    assert (rows >= 0).all()
    # every pixel's row: its interaction, its samples, its material's side
    mat = _np(cam.it["material"])
    types = np.where(mat >= 0, mat_type[np.maximum(mat, 0)], 0)
    assert set(types[rows].tolist()) <= set(SIDE_OF), set(types[rows].tolist())
    side = np.array([SIDE_OF.get(int(t), 0) for t in types], np.int32)
    u4 = torch.from_numpy(samples0[cam.pixel_index]).to(dev)
    out = s.sample_lights_device(cam.it, cam.lam, u4, torch.from_numpy(side).to(dev))
    prod = out["pmf"] * out["pdf"]                                        # one fp32 multiply
    torch.cuda.synchronize()
    rays, prod = _np(out["shadow_rays8"])[rows], _np(prod)[rows]
    assert same(_bits(rays[:, :3]), _bits(so[:, :3])), int((_bits(rays[:, :3]) != _bits(so[:, :3])).any(axis=1).sum())
    assert same(_bits(rays[:, 3:6]), _bits(sd[:, :3])), int((_bits(rays[:, 3:6]) != _bits(sd[:, :3])).any(axis=1).sum())
    assert same(_bits(rays[:, 6]), _bits(so[:, 3]))
    assert same(_bits(np.repeat(prod[:, None], 4, axis=1)), _bits(sr_l)), int((_bits(np.repeat(prod[:, None], 4, axis=1)) != _bits(sr_l)).any(axis=1).sum())
    assert len(set(side[rows].tolist())) >= (2 if name.startswith("materials_lights") else 1)
    s.close()


# ---- 4: the depth-1 MIS weights -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, kind", [("cornell64", "emitter"), ("envmap", "escape")])
def test_emitted_pmf_and_pdf_give_the_renders_depth1_mis_weights(wfpt, name, kind):
    import torch
    dev = torch.device("cuda", 0)
    s = open_scene(wfpt, name)
    _, _, mat_type, _, _ = tables(wfpt, s)
    n_pix = s.width * s.height
    n_inf = s.query("infinite_lights")
    begin_pass(wfpt, s)
    emission(wfpt, s, 0)
    shade(wfpt, s, 0, mat_type)
    stage(wfpt, s, "wf_intersect_shadow", 0)
    stage(wfpt, s, "wf_reset_stage_queues", 1)
    stage(wfpt, s, "wf_gen_ray_samples", 1, 0)
    stage(wfpt, s, "wf_intersect_closest", 1)
    stage(wfpt, s, "wf_sync")
    m = queue_size(wfpt, s, "ray1")
    assert m > 0
    q = {k: download(wfpt, s, "ray1", k, m, np.float32, 4) for k in ("o", "d", "beta", "r_u", "r_l", "ctx0", "ctx1", "ctx2")}
    meta = download(wfpt, s, "ray1", "meta", m, np.int32, 4)
    lam_pix = download(wfpt, s, "pixel", "lambda", n_pix, np.float32, 4)
    L_before = download(wfpt, s, "pixel", "L", n_pix, np.float32, 4)
    emission(wfpt, s, 1)
    L_after = download(wfpt, s, "pixel", "L", n_pix, np.float32, 4)
    pixel = meta[:, 0].astype(np.int64)
    assert (meta[:, 1] == 1).all() and len(np.unique(pixel)) == m
    # the rays, their hits, and the vertex they left (LoadCtx's unpacking)
    rays8 = np.concatenate([q["o"][:, :3], q["d"][:, :3], np.full((m, 1), np.inf, np.float32), q["o"][:, 3:4]], axis=1).astype(np.float32)
    prev = np.zeros((4, m, 4), np.float32)
    prev[0, :, :3] = q["ctx0"][:, :3]
    prev[1, :, 0], prev[1, :, 1:3] = q["ctx0"][:, 3], q["ctx1"][:, :2]
    prev[2, :, :2], prev[2, :, 2] = q["ctx1"][:, 2:], q["ctx2"][:, 0]
    prev[3, :, :3] = q["ctx2"][:, 1:]
    rays_t = torch.from_numpy(rays8).to(dev)
    it = s.interactions_device(rays_t, s.trace_device(rays_t))
    lam = torch.from_numpy(lam_pix[pixel]).to(dev)
    prev_t = torch.from_numpy(prev).to(dev)
    # the expressions in torch fp32 on the host (IEEE division), operation for operation
    beta, r_u, r_l0 = (torch.from_numpy(q[k]) for k in ("beta", "r_u", "r_l"))
    specular = torch.from_numpy((meta[:, 2] & SPECULAR_BOUNCE) != 0)[:, None]
    valid = it["valid"].cpu()
    L = torch.zeros((m, 4), dtype=torch.float32)
    if kind == "escape":
        # KHandleEscaped: L += beta * Le / (r_u + (r_l * pmf) * pdf).Average() per infinite light with Le != 0, then L += pixel L if L != 0
        assert n_inf >= 1
        for k in range(n_inf):
            e = s.emitted_device(rays_t, it, lam, infinite_index=k, prev=prev_t)
            Le, pmf, pdf = e["Le"].cpu(), e["pmf"].cpu(), e["pdf"].cpu()
            r_l = (r_l0 * pmf[:, None]) * pdf[:, None]
            term = torch.where(specular, beta * Le / average(r_u), beta * Le / average(r_u + r_l))
            lit = ((valid == 0) & (Le != 0).any(dim=1))[:, None]
            L = torch.where(lit, L + term, L)
        rows = _np((valid == 0) & (L != 0).any(dim=1))
        assert (_np(valid) == 0).any()
    else:
        # KHandleEmissive: L = beta * Le / (r_u + r_l * (pmf * pdf)).Average() where Le != 0, then L += pixel L
        e = s.emitted_device(rays_t, it, lam, infinite_index=0, prev=prev_t)
        Le, pmf, pdf = e["Le"].cpu(), e["pmf"].cpu(), e["pdf"].cpu()
        r_l = r_l0 * (pmf * pdf)[:, None]
        L = torch.where(specular, beta * Le / average(r_u), beta * Le / average(r_u + r_l))
        rows = _np((valid == 1) & (it["area_light"].cpu() >= 0) & (Le != 0).any(dim=1))
        assert (_np(pdf)[rows] > 0).all() and (_np(pmf)[rows] > 0).all()
    assert rows.sum() > 20, "too few %s rows at depth 1: %d" % (kind, rows.sum())
    want = L_before.copy()
    want[pixel[rows]] = _np(L + torch.from_numpy(L_before[pixel]))[rows]
    diff = (_bits(L_after) != _bits(want)).any(axis=1)
    if kind == "escape":
        # the emitter stage ran too: only the pixels of escaped rays are this test's
        sel = np.zeros(n_pix, bool)
        sel[pixel[_np(valid) == 0]] = True
        diff &= sel
    else:
        sel = np.zeros(n_pix, bool)
        sel[pixel[_np(valid) == 1]] = True
        diff &= sel
    assert not diff.any(), "%d pixels differ" % diff.sum()
    assert (_bits(L_after) != _bits(L_before)).any(axis=1)[pixel[rows]].any()
    s.close()


# ---- 5: shapes -----------------------------------------------------------------------------------------------------------------------------
class Shapes:
    """one input with misses and invalid rows between the hits (envmap), the full call's outputs, and the host's"""

    def __init__(self, wfpt, tmp):
        import torch
        dev = torch.device("cuda", 0)
        self.s = s = open_scene(wfpt, "envmap")
        fh = s.first_hit(0)
        self.n = n = fh["rays8"].shape[0]
        assert n % 37 != 0
        order = (torch.arange(n, device=dev) * 37) % n                          # every prefix holds pixels from all over the image: sky and objects
        self.pf, self.pi = fh["planes_f"][:, order].contiguous(), fh["planes_i"][:, order].contiguous()
        self.pi[1, 3::7, 1] = -1                                                # records outside the scene's ranges
        self.lam, self.rays = fh["lambda4"][order].contiguous(), fh["rays8"][order].contiguous()
        self.u4 = seeded(n, 4, 99, dev)
        self.side = (torch.arange(n, dtype=torch.int32, device=dev) % 3 - 1).contiguous()
        self.full = s.sample_lights_device((self.pf, self.pi), self.lam, self.u4, self.side)
        self.full_e = s.emitted_device(self.rays, (self.pf, self.pi), self.lam, prev=self.pf)
        torch.cuda.synchronize()
        valid = _np(self.pi[1, :, 1])
        assert (valid == 1).any() and (valid == 0).any() and (valid == -1).any()
        assert (valid[:513] == 1).any() and (valid[:513] == 0).any()
        want = eval_host("envmap", 0, _np(self.pf), _np(self.pi), _np(self.lam), u4=_np(self.u4), side=_np(self.side), tmp=tmp)
        assert_rows_equal(self.full, want, SAMPLE_KEYS, "envmap with invalid rows, sample")
        want = eval_host("envmap", 1, _np(self.pf), _np(self.pi), _np(self.lam), rays=_np(self.rays), prev=_np(self.pf), tmp=tmp)
        assert_rows_equal(self.full_e, want, EMITTED_KEYS, "envmap with invalid rows, emitted")

    def prefix(self, k):
        return ((self.pf[:, :k].contiguous(), self.pi[:, :k].contiguous()), self.lam[:k].contiguous(), self.u4[:k].contiguous(), self.side[:k].contiguous(),
                self.rays[:k].contiguous())


@pytest.fixture(scope="module")
def shapes(wfpt, tmp_path_factory):
    sh = Shapes(wfpt, str(tmp_path_factory.mktemp("shapes")))
    yield sh
    sh.s.close()


@pytest.mark.parametrize("k", [1, 63, 64, 65, 255, 256, 257, 513])
def test_prefixes_give_the_rows_of_the_full_call(shapes, k):
    import torch
    it, lam, u4, side, rays = shapes.prefix(k)
    a = shapes.s.sample_lights_device(it, lam, u4, side)
    b = shapes.s.emitted_device(rays, it, lam, prev=it[0])
    torch.cuda.synchronize()
    assert_rows_equal(a, {x: _np(shapes.full[x])[:k] for x in SAMPLE_KEYS}, SAMPLE_KEYS, "prefix %d" % k)
    assert_rows_equal(b, {x: _np(shapes.full_e[x])[:k] for x in EMITTED_KEYS}, EMITTED_KEYS, "prefix %d" % k)


def test_the_device_count_and_the_rows_after_n_are_respected(wfpt, shapes):
    import torch
    dev = torch.device("cuda", 0)
    sh, s = shapes, shapes.s
    a = s.sample_lights_device((sh.pf, sh.pi), sh.lam, sh.u4, sh.side)
    b = s.emitted_device(sh.rays, (sh.pf, sh.pi), sh.lam, prev=sh.pf)
    for count in (300, 0, -4, 10 ** 6):
        for d, keys in ((a, SAMPLE_KEYS), (b, EMITTED_KEYS)):
            for x in keys:
                d[x].view(torch.int32).fill_(0x7fc12345)
        nd = torch.tensor([count], dtype=torch.int32, device=dev)
        s.sample_lights_device((sh.pf, sh.pi), sh.lam, sh.u4, sh.side, n_device=nd, out=a)
        s.emitted_device(sh.rays, (sh.pf, sh.pi), sh.lam, prev=sh.pf, out=b, n_device=nd)
        torch.cuda.synchronize()
        k = min(max(count, 0), sh.n)
        for d, full, keys in ((a, sh.full, SAMPLE_KEYS), (b, sh.full_e, EMITTED_KEYS)):
            for x in keys:
                g = _np(d[x].view(torch.int32))
                assert same(g[:k], _np(full[x].view(torch.int32))[:k]), (count, x)
                assert (g[k:] == 0x7fc12345).all(), (count, x)
    # buffers longer than n: the rows after row n stay as they were (the raw calls, n = 257 of the 321 rows allocated)
    _, hip = wfpt.libs()
    n, room = 257, 321
    it, lam, u4, side, rays = sh.prefix(n)
    outs = [torch.full((room, c), 0x7fc12345, dtype=torch.int32, device=dev) for c in (8, 4, 4, 4, 4, 4)]
    torch.cuda.synchronize()
    f = hip.wf_light_sample_device
    f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 10
    assert f(s.ctx, n, None, it[0].data_ptr(), it[1].data_ptr(), lam.data_ptr(), u4.data_ptr(), side.data_ptr(), *[t.data_ptr() for t in outs[:4]]) == 0, hip.wf_last_error()
    g = hip.wf_light_emitted_device
    g.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 3
    assert g(s.ctx, n, None, rays.data_ptr(), it[0].data_ptr(), it[1].data_ptr(), lam.data_ptr(), 0, it[0].data_ptr(), outs[4].data_ptr(), outs[5].data_ptr()) == 0, hip.wf_last_error()
    stage(wfpt, s, "wf_sync")
    for t, full in zip(outs, [sh.full[x] for x in SAMPLE_KEYS] + [sh.full_e[x] for x in EMITTED_KEYS]):
        assert same(_np(t)[:n], _np(full.view(torch.int32))[:n]) and (_np(t)[n:] == 0x7fc12345).all()


def test_rows_that_want_nothing_and_a_scene_without_lights(wfpt, shapes):
    import torch
    sh = shapes
    pi = sh.pi.clone()
    pi[1, :, 1] = 0
    a = sh.s.sample_lights_device((sh.pf, pi), sh.lam, sh.u4, sh.side)
    torch.cuda.synchronize()
    assert not _np(a["shadow_rays8"]).any() and not _np(a["L4"]).any() and not _np(a["wi_pdf4"]).any()
    assert (_np(a["light4"]) == np.array([-1, 0, 0, -1], np.int32)).all()
    # a scene without lights.  The scene loader refuses one ("No light sources specified", as the reference's integrator does), so the
    # description of cornell64 is uploaded through the C ABI with its light table emptied: no light, no infinite light, no light BVH
    host, hip = wfpt.libs()
    scene = wfpt.Scene(path=os.path.join(GOLDEN, "cornell64.pbrt"), spp=4)
    h = DescLights.from_address(host.wfh_scene_desc(scene.h))
    saved = (h.n_lights, h.n_infinite_lights, h.n_light_bvh_nodes)
    assert saved[0] > 0
    hip.wf_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    hip.wf_scene_upload.argtypes = [C.c_void_p, C.c_void_p]
    hip.wf_ctx_query.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
    hip.wf_sync.argtypes = [C.c_void_p]
    ctx = C.c_void_p()
    assert hip.wf_ctx_create(0, C.byref(ctx)) == 0 and ctx.value, hip.wf_last_error()
    try:
        h.n_lights = h.n_infinite_lights = h.n_light_bvh_nodes = 0
        assert hip.wf_scene_upload(ctx, host.wfh_scene_desc(scene.h)) == 0, hip.wf_last_error()
        for key in (b"lights", b"infinite_lights", b"light_sample_rare"):
            v = C.c_int64(-1)
            assert hip.wf_ctx_query(ctx, key, C.byref(v)) == 0 and v.value == 0, key
        n = 257
        it, lam, u4, side, rays = sh.prefix(n)                 # hits and misses; some hits name an area light the empty table does not hold
        it[1][0, ::5, 1] = 1
        dev = lam.device
        outs = [torch.full((n, c), 0x7fc12345, dtype=torch.int32, device=dev) for c in (8, 4, 4, 4, 4, 4)]
        torch.cuda.synchronize()
        f = hip.wf_light_sample_device
        f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 10
        g = hip.wf_light_emitted_device
        g.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 3
        assert f(ctx, n, None, it[0].data_ptr(), it[1].data_ptr(), lam.data_ptr(), u4.data_ptr(), side.data_ptr(), *[t.data_ptr() for t in outs[:4]]) == 0, hip.wf_last_error()
        emitted = (rays.data_ptr(), it[0].data_ptr(), it[1].data_ptr(), lam.data_ptr())
        assert g(ctx, n, None, *emitted, 0, it[0].data_ptr(), outs[4].data_ptr(), outs[5].data_ptr()) == 0, hip.wf_last_error()
        assert g(ctx, n, None, *emitted, 1, it[0].data_ptr(), outs[4].data_ptr(), outs[5].data_ptr()) != 0 and b"infinite_index 1" in hip.wf_last_error()
        assert hip.wf_sync(ctx) == 0, hip.wf_last_error()
        valid = _np(it[1][1, :, 1])
        assert (valid == 1).any() and (valid == 0).any()
        assert (_np(outs[3]) == np.array([-1, 0, 0, -1], np.int32)).all()          # light id -1 everywhere
        for t in outs[:3] + outs[4:]:
            assert not _np(t).any()                                                # zero rays, L = 0, Le = 0
    finally:
        h.n_lights, h.n_infinite_lights, h.n_light_bvh_nodes = saved
        hip.wf_ctx_destroy.argtypes = [C.c_void_p]
        hip.wf_ctx_destroy(ctx)
        scene.close()


# ---- 6: variants ---------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from conftest import load_pkg, GOLDEN
wfpt = load_pkg(); wfpt.libs()
s = wfpt.Scene(path=os.path.join(GOLDEN, "cornell64.pbrt"), spp=4)
s.create_renderer(0, samples_per_pass=1)
import torch
assert s.query("light_sample_rare") == 1 and s.query("light_emitted_variant") == 7
fh = s.first_hit(0)
n = fh["rays8"].shape[0]
g = torch.Generator().manual_seed(77)
u4 = torch.rand((n, 4), generator=g, dtype=torch.float32).to(fh["rays8"].device)
side = (torch.arange(n, dtype=torch.int32, device=u4.device) % 3 - 1).contiguous()
a = s.sample_lights_device(fh, fh["lambda4"], u4, side)
rays = a["shadow_rays8"].clone(); rays[:, 6] = float("inf")
it = s.interactions_device(rays, s.trace_device(rays))
e = s.emitted_device(rays, it, fh["lambda4"], prev=fh)
torch.cuda.synchronize()
np.savez(sys.argv[2], **{k: a[k].cpu().numpy() for k in ("shadow_rays8", "L4", "wi_pdf4", "light4")}, **{k: e[k].cpu().numpy() for k in ("Le4", "pmf_pdf4")})
s.close()
"""


def test_the_scene_picks_the_variants_and_the_general_ones_agree(wfpt, tmp_path):
    import torch
    for name, rare, emitted in (("portal_light", 1, 5), ("quadrics", 1, 4), ("cornell64", 0, 0)):
        s = open_scene(wfpt, name)
        assert s.query("light_sample_rare") == s.query("rare_lights") == rare and s.query("light_emitted_variant") == emitted, name
        if name != "cornell64":
            s.close()
    fh = s.first_hit(0)
    n = fh["rays8"].shape[0]
    u4 = seeded(n, 4, 77, fh["rays8"].device)
    side = (torch.arange(n, dtype=torch.int32, device=u4.device) % 3 - 1).contiguous()
    a = s.sample_lights_device(fh, fh["lambda4"], u4, side)
    rays = a["shadow_rays8"].clone()
    rays[:, 6] = float("inf")
    it = s.interactions_device(rays, s.trace_device(rays))
    e = s.emitted_device(rays, it, fh["lambda4"], prev=fh)
    torch.cuda.synchronize()
    out = str(tmp_path / "general.npz")
    env = dict(os.environ, WF_RARE_LIGHTS="1")
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, out], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    z = np.load(out)
    assert_rows_equal(a, z, SAMPLE_KEYS, "lean against general, sample")
    assert_rows_equal(e, z, EMITTED_KEYS, "lean against general, emitted")
    assert _np(e["Le4"]).any() and _np(e["pmf_pdf4"]).any()
    s.close()


# ---- 7: neighbourliness -----------------------------------------------------------------------------------------------------------------------
def test_the_calls_queue_behind_torchs_stream_without_a_host_sync(shapes):
    """inputs written by a torch op on a side stream immediately before the calls, results consumed by a torch op immediately after them"""
    import torch
    sh = shapes
    stream = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        big = torch.ones((4096, 4096), dtype=torch.float32, device="cuda:0")
        for _ in range(8):                                    # work the producer has to wait behind
            big = big @ big * (1.0 / 4096)
        u4 = sh.u4 * big[0, 0]                                # = the samples, once the products are done
        lam = sh.lam * big[1, 1]
        a = sh.s.sample_lights_device((sh.pf, sh.pi), lam, u4, sh.side)
        e = sh.s.emitted_device(sh.rays, (sh.pf, sh.pi), lam, prev=sh.pf)
        total = a["L4"].sum(dtype=torch.float64) + e["Le4"].sum(dtype=torch.float64)
        kept = {k: a[k].clone() for k in SAMPLE_KEYS}
        kept.update({k: e[k].clone() for k in EMITTED_KEYS})
    stream.synchronize()
    assert_rows_equal(kept, {k: _np(sh.full[k]) for k in SAMPLE_KEYS}, SAMPLE_KEYS, "behind a side stream")
    assert_rows_equal(kept, {k: _np(sh.full_e[k]) for k in EMITTED_KEYS}, EMITTED_KEYS, "behind a side stream")
    want = _np(sh.full["L4"]).astype(np.float64).sum() + _np(sh.full_e["Le4"]).astype(np.float64).sum()
    assert want > 0 and abs(float(total) - want) <= 1e-6 * abs(want)


def test_a_render_is_the_same_after_a_hundred_calls(wfpt):
    import torch
    s = open_scene(wfpt, "cornell64")
    s.clear_film()
    s.render()
    film, stats = s.film(), s.stats()
    fh = s.first_hit(0)
    n = fh["rays8"].shape[0]
    u4 = seeded(n, 4, 3, fh["rays8"].device)
    for k in range(50):
        a = s.sample_lights_device(fh, fh["lambda4"], u4)
        s.emitted_device(a["shadow_rays8"], fh, fh["lambda4"], prev=fh)
    torch.cuda.synchronize()
    assert s.stats() == stats                                  # nothing counted
    s.clear_film()
    s.render()
    assert s.film().tobytes() == film.tobytes() and s.stats() == stats
    s.close()


def test_arguments_are_refused_before_any_launch(wfpt, shapes):
    import torch
    dev = torch.device("cuda", 0)
    _, hip = wfpt.libs()
    sh, s = shapes, shapes.s
    n = 64
    it, lam, u4, side, rays = sh.prefix(n)
    outs = [torch.full((n * c + 8,), 0x7fc12345, dtype=torch.int32, device=dev) for c in (8, 4, 4, 4, 4, 4)]
    count = torch.tensor([n, 0], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    f = hip.wf_light_sample_device
    f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 10
    names = ["n_device", "planes_f", "planes_i", "lambda4", "u4", "side", "shadow_rays8", "L4", "wi_pdf4", "light4"]
    good = [count.data_ptr(), it[0].data_ptr(), it[1].data_ptr(), lam.data_ptr(), u4.data_ptr(), side.data_ptr()] + [t.data_ptr() for t in outs[:4]]

    def refused(fn, label, *args):
        assert fn(*args) != 0, label
        err = hip.wf_last_error()
        assert fn.__name__.encode() in err and label.encode() in err, (label, err)

    for k, name in enumerate(names):
        if name not in ("n_device", "side"):
            bad = list(good); bad[k] = None
            refused(f, name, s.ctx, n, *bad)
        for off in ((1, 2) if name in ("n_device", "side") else (4, 8)):
            bad = list(good); bad[k] = good[k] + off
            refused(f, name, s.ctx, n, *bad)
    refused(f, "n = -1", s.ctx, -1, *good)
    assert f(None, n, *good) != 0 and b"wf_light_sample_device: null context" in hip.wf_last_error()
    assert f(s.ctx, 0, *[None] * 10) == 0
    g = hip.wf_light_emitted_device
    g.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 3
    names = ["n_device", "rays8", "planes_f", "planes_i", "lambda4", "prev_planes_f", "Le4", "pmf_pdf4"]
    good_e = [count.data_ptr(), rays.data_ptr(), it[0].data_ptr(), it[1].data_ptr(), lam.data_ptr(), it[0].data_ptr(), outs[4].data_ptr(), outs[5].data_ptr()]
    call = lambda a, index=0, m=n, ctx=s.ctx: (ctx, m, a[0], a[1], a[2], a[3], a[4], index, a[5], a[6], a[7])
    for k, name in enumerate(names):
        if name not in ("n_device", "prev_planes_f"):
            bad = list(good_e); bad[k] = None
            refused(g, name, *call(bad))
        for off in ((1, 2) if name == "n_device" else (4, 8)):
            bad = list(good_e); bad[k] = good_e[k] + off
            refused(g, name, *call(bad))
    refused(g, "n = -1", *call(good_e, m=-1))
    for index in (-1, 1, 7):                                   # envmap has one infinite light
        refused(g, "infinite_index %d" % index, *call(good_e, index=index))
    refused(g, "infinite_index 1", *call(good_e, index=1, m=0))  # ... checked for an empty call too
    assert g(*call(good_e, ctx=None)) != 0 and b"wf_light_emitted_device: null context" in hip.wf_last_error()
    stage(wfpt, s, "wf_sync")
    torch.cuda.synchronize()
    for t in outs:
        assert (_np(t) == 0x7fc12345).all()
    # ... and the same arguments as they should be are accepted
    assert f(s.ctx, n, *good) == 0 and g(*call(good_e)) == 0, hip.wf_last_error()
    stage(wfpt, s, "wf_sync")
    assert same(_np(outs[1])[:n * 4].reshape(n, 4), _np(sh.full["L4"].view(torch.int32))[:n])
