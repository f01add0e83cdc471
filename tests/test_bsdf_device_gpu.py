"""wf_bsdf_make_device and wf_bsdf_eval_device on the MI355X: the scene's BSDFs on a caller's device items.

Everything is bit for bit.  The expected values come from three independent places: the host program bsdf_check --eval (the render's
own material functions composed directly, on the host, every BxDF kept as the render's struct), the render's own stages driven through
the C ABI (the indirect rays and the shadow queue of depth 0, the pixel radiance after the shadow stage), and the calls themselves on
other shapes of the same input."""
import ctypes as C
import os

import numpy as np
import pytest

from boundary_helpers import (SIDE_OF, Camera, _bits, _np, assert_rows_equal, average, begin_pass, download, emission, eval_on_host, open_scene, queue_size,
                              renderer_before_torch, same, seeded, shade, stage, tables)  # noqa: F401 (the fixture)
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

CHECK = os.path.join(ROOT, "pbrt-v4_amd", "_build", "bsdf_check")
FIXTURES = ["matrix_lean", "matrix_lean_tex", "mix_materials", "materials_lights", "textures_bump", "alpha_normalmap", "displacement", "hair",
            "measured", "subsurface", "textures_noise", "parser_torture"]
RENDER_FIXTURES = ["cornell64", "materials_lights", "matrix_lean_tex", "mix_materials", "alpha_normalmap", "displacement", "hair", "measured"]
REFLECTION, TRANSMISSION, DIFFUSE_BIT, GLOSSY, SPECULAR = 1, 2, 4, 8, 16
SUBSURFACE, MIX = 8, 11
SPECULAR_BOUNCE, ANY_NONSPECULAR = 1, 2   # RAYFLAG_* of wf_kernels.h
MAKE_KEYS = ("rec", "bsdf4")
WI_KEYS = ("f4", "pdf4")
U_KEYS = ("next_rays8", "sample_f4", "sample_pdf4", "sample_i4")


def eval_host(name, rays, planes_f, planes_i, lam, reg=None, wi=None, u4=None, tmp=None, spp=4):
    """bsdf_check --eval on downloaded inputs -> the expected outputs (numpy); spp: what open_scene opened the scene with"""
    n = planes_f.shape[1]
    head = np.array([0x42534431, n, int(reg is not None), int(wi is not None), int(u4 is not None), 0, 0, 0], np.int32)
    parts = [head, rays.astype(np.float32), planes_f.astype(np.float32), planes_i.astype(np.int32), lam.astype(np.float32)]
    parts += [x for x in (None if reg is None else reg.astype(np.int32), wi, u4) if x is not None]
    raw = eval_on_host(CHECK, ["--spp", str(spp)], os.path.join(GOLDEN, name + ".pbrt"), parts, tmp)
    off = [0]

    def take(dtype, shape):
        count = int(np.prod(shape))
        v = np.frombuffer(raw, dtype, count, off[0]).reshape(shape)
        off[0] += 4 * count
        return v
    out = {"rec": take(np.float32, (10, n, 4)), "bsdf4": take(np.int32, (n, 4))}
    if wi is not None:
        out.update(f4=take(np.float32, (n, 4)), pdf4=take(np.float32, (n, 4)))
    if u4 is not None:
        out.update(next_rays8=take(np.float32, (n, 8)), sample_f4=take(np.float32, (n, 4)), sample_pdf4=take(np.float32, (n, 4)), sample_i4=take(np.int32, (n, 4)))
    assert off[0] == len(raw)
    return out


def make_and_eval(s, fh, dev, seed=99):
    """bsdf_device on the first hits, the lights sampled with its side, bsdf_eval_device for the light directions and for seeded u4"""
    import torch
    n = fh["rays8"].shape[0]
    reg = (torch.arange(n, dtype=torch.int32, device=dev) % 2).contiguous()
    b = s.bsdf_device(fh["rays8"], fh, fh["lambda4"], regularize=reg)
    ls = s.sample_lights_device(fh, fh["lambda4"], seeded(n, 4, seed, dev), b["side"].contiguous())
    u4 = seeded(n, 4, seed + 1, dev)
    e = s.bsdf_eval_device(b, fh, wi=ls["wi_pdf4"], u4=u4)
    torch.cuda.synchronize()
    return reg, b, ls, u4, e


# ---- 1: against the host oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_both_calls_equal_the_host_composition(wfpt, name, tmp_path):
    import torch
    dev = torch.device("cuda", 0)
    s = open_scene(wfpt, name)
    _, _, mat_type, _, _ = tables(wfpt, s)
    fh = s.first_hit(0)
    reg, b, ls, u4, e = make_and_eval(s, fh, dev)
    want = eval_host(name, _np(fh["rays8"]), _np(fh["planes_f"]), _np(fh["planes_i"]), _np(fh["lambda4"]), reg=_np(reg), wi=_np(ls["wi_pdf4"]), u4=_np(u4),
                     tmp=str(tmp_path))
    assert_rows_equal(b, want, MAKE_KEYS, name + " make")
    assert_rows_equal(e, want, WI_KEYS + U_KEYS, name + " eval")
    b4 = want["bsdf4"]
    # the views name the same words
    assert same(_np(b["flags"]), b4[:, 0] & 0xff) and same(_np(b["side"]), b4[:, 1]) and same(_np(b["material"]), b4[:, 2]) and same(_np(b["type"]), b4[:, 3])
    assert same(_np(b["terminated"]), (b4[:, 0] & 256) != 0)
    assert same(_np(e["pdf_mis"]), want["sample_pdf4"][:, 1]) and same(_np(e["sample_valid"]), want["sample_i4"][:, 0]) and same(_np(e["cos"]), want["pdf4"][:, 1])
    # rows without a BSDF are zeros; the others carry the scene's material types, the mix resolved
    valid, mat = _np(fh["valid"]), _np(fh["material"])
    none = (valid != 1) | (mat < 0)
    assert (b4[none] == 0).all() and not want["rec"][:, none].any() and (b4[~none, 3] >= 1).all() and (~none).any()
    assert (mat_type[b4[~none, 2]] == b4[~none, 3]).all() and MIX not in set(b4[:, 3].tolist())
    plain = ~none & (mat_type[np.maximum(mat, 0)] != MIX)
    assert (b4[plain, 2] == mat[plain]).all()
    if name == "mix_materials":
        assert (~none & ~plain).any()
    # the side word is the table the light tests answer it from, on the types that table covers
    covered = np.isin(b4[:, 3], list(SIDE_OF)) & ((b4[:, 0] & (DIFFUSE_BIT | GLOSSY)) != 0)
    assert same(b4[covered, 1], np.array([SIDE_OF[int(t)] for t in b4[covered, 3]], np.int32))
    assert (e["sample_valid"] == 1).any() and _np(e["f4"]).any()
    if name == "parser_torture":
        assert _np(b["terminated"]).any()
    s.close()


# ---- the render's depth 0, unfused ------------------------------------------------------------------------------------------------------
def name_has_no_bump(b, it):
    """no row's final shading normal differs from its interaction's (a scene without normal and bump maps)"""
    live = _np(b["type"]) != 0
    return same(_np(b["ns"])[live], _np(it["ns"])[live])



class Depth0:
    """the render's unfused depth-0 stages through the C ABI, and the caller's side of the same vertices through the device calls"""

    def __init__(self, wfpt, s, shadow_stage=False):
        import torch
        self.dev = dev = torch.device("cuda", 0)
        _, _, self.mat_type, _, _ = tables(wfpt, s)
        self.n_pix = n_pix = s.width * s.height
        self.cam = cam = Camera(wfpt, s)
        self.emitted = torch.zeros((n_pix, 4), dtype=torch.float32, device=dev)
        for k in range(max(1, s.query("infinite_lights"))):
            self.emitted = self.emitted + s.emitted_device(cam.rays, cam.it, cam.lam, infinite_index=k)["Le"]
        begin_pass(wfpt, s)
        assert (download(wfpt, s, "ray0", "beta", n_pix, np.float32, 4) == 1).all() and (download(wfpt, s, "ray0", "r_u", n_pix, np.float32, 4) == 1).all()
        emission(wfpt, s, 0)
        shade(wfpt, s, 0, self.mat_type)
        self.s0 = download(wfpt, s, "pixel", "samples0", n_pix, np.float32, 4)[cam.pixel_index]
        self.s1 = download(wfpt, s, "pixel", "samples1", n_pix, np.float32, 4)[cam.pixel_index]
        m = queue_size(wfpt, s, "ray1")
        self.ray = {k: download(wfpt, s, "ray1", k, m, np.float32, 4) for k in ("o", "d", "beta", "r_u", "r_l")}
        self.ray["meta"] = download(wfpt, s, "ray1", "meta", m, np.int32, 4)
        k = queue_size(wfpt, s, "shadow")
        self.shadow = {key: download(wfpt, s, "shadow", key, k, np.float32, 4) for key in ("o", "d", "Ld", "r_u", "r_l")}
        if shadow_stage:
            stage(wfpt, s, "wf_intersect_shadow", 0)
            stage(wfpt, s, "wf_sync")
            self.L = download(wfpt, s, "pixel", "L", n_pix, np.float32, 4)[cam.pixel_index]
        # the caller's side: the BSDF of every first hit (nothing regularised at depth 0), the lights with its side, the BSDF for both
        self.b = s.bsdf_device(cam.rays, cam.it, cam.lam)
        # (the render's LightSampleContext carries the FINAL shading normal — after the normal or bump map — so the lights get the planes
        #  with the BSDF's ns in plane 3)
        self.light_it = (s.light_planes(cam.it, self.b), cam.it["planes_i"])
        assert not same(_np(self.light_it[0]), _np(cam.it["planes_f"])) or name_has_no_bump(self.b, cam.it)
        self.ls = s.sample_lights_device(self.light_it, cam.lam, torch.from_numpy(self.s0).to(dev), self.b["side"].contiguous())
        u4 = np.stack([self.s0[:, 3], self.s1[:, 0], self.s1[:, 1], np.zeros(len(self.s0), np.float32)], axis=1)
        self.e = s.bsdf_eval_device(self.b, cam.it, wi=self.ls["wi_pdf4"], u4=torch.from_numpy(np.ascontiguousarray(u4)).to(dev))
        torch.cuda.synchronize()

    def rows_of(self, pixel):
        assert len(np.unique(pixel)) == len(pixel) and (pixel >= 0).all() and (pixel < self.n_pix).all()
        rows = self.cam.row_of[pixel]
        assert (rows >= 0).all()
        return rows

    def nee(self):
        """(usable rows, Ld, r_u, r_l) of next-event estimation as MatNeeFinish computes them, in torch fp32 on the host"""
        import torch
        f, cosine, pdf = self.e["f"].cpu(), self.e["cos"].cpu(), self.e["pdf"].cpu()
        L, lpdf, pmf, delta = self.ls["L"].cpu(), self.ls["pdf"].cpu(), self.ls["pmf"].cpu(), (self.ls["flags"].cpu() & 1) != 0
        Ld = (f * cosine[:, None]) * L                                        # beta = it.beta (1) * f * AbsDot(wi, ns);  Ld = beta * ls.L
        r_u = torch.where(delta, torch.zeros_like(pdf), pdf)[:, None].expand(-1, 4)   # it.r_u (1) * bsdfPDF
        r_l = (lpdf * pmf)[:, None].expand(-1, 4)                             # it.r_u (1) * (ls.pdf * lightPMF)
        nonspecular = (self.b["flags"].cpu() & (DIFFUSE_BIT | GLOSSY)) != 0
        usable = nonspecular & (lpdf != 0) & (f != 0).any(dim=1)
        return _np(usable), _np(Ld), _np(r_u.contiguous()), _np(r_l.contiguous())


# ---- 2: against the render's indirect rays ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RENDER_FIXTURES)
def test_samples_equal_the_renders_indirect_rays(wfpt, name):
    import torch
    s = open_scene(wfpt, name)
    assert s.plan("tr_route") == -1   # no media: the next ray's medium is -1 on both sides
    d0 = Depth0(wfpt, s)
    e, q = d0.e, d0.ray
    f, pdf, pdf_mis, cosine, eta = (e[k].cpu() for k in ("sample_f", "sample_pdf", "pdf_mis", "sample_cos", "eta"))
    flags, valid = _np(e["sample_flags"]), _np(e["sample_valid"])
    beta = f * cosine[:, None] / pdf[:, None]                                 # wbeta (1) * bs.f * AbsDot(wi, ns) / bs.pdf
    r_l = torch.ones_like(f) / pdf_mis[:, None]                               # r_u (1) / (the proportional PDF's stand-in, or bs.pdf)
    eta_scale = torch.where(torch.from_numpy((flags & TRANSMISSION) != 0), 1 * (eta * eta), torch.ones_like(eta))
    beta, r_l, eta_scale = _np(beta), _np(r_l), _np(eta_scale)
    specular = (flags & SPECULAR) != 0
    ray_flags = np.where(specular, SPECULAR_BOUNCE, ANY_NONSPECULAR).astype(np.int32)
    # the pushed rays are the valid samples with a throughput; a subsurface row that transmits goes to the BSSRDF stage instead
    bssrdf = (_np(d0.b["type"]) == SUBSURFACE) & ((flags & TRANSMISSION) != 0) & (valid == 1)
    pushed = (valid == 1) & (beta != 0).any(axis=1) & ~bssrdf
    rows = d0.rows_of(q["meta"][:, 0].astype(np.int64))
    assert same(np.sort(rows), np.nonzero(pushed)[0]), (len(rows), int(pushed.sum()), int(bssrdf.sum()))
    assert len(rows) > 0
    nxt = _np(e["next_rays8"])[rows]
    for got, want, what in ((nxt[:, :3], q["o"][:, :3], "o"), (nxt[:, 7], q["o"][:, 3], "time"), (nxt[:, 3:6], q["d"][:, :3], "d"), (eta_scale[rows], q["d"][:, 3], "etaScale"),
                            (beta[rows], q["beta"], "beta"), (np.ones((len(rows), 4), np.float32), q["r_u"], "r_u"), (r_l[rows], q["r_l"], "r_l")):
        bad = (_bits(got) != _bits(want)).reshape(len(rows), -1).any(axis=1)
        assert not bad.any(), "%s: %s differs in %d of %d rays, first %r / %r" % (name, what, bad.sum(), len(rows), got[bad][0], want[bad][0])
    meta = np.stack([d0.cam.pixel_index[rows].astype(np.int32), np.ones(len(rows), np.int32), ray_flags[rows], _np(e["next_medium"])[rows]], axis=1)
    assert same(meta, q["meta"])
    if name == "matrix_lean_tex":
        assert bssrdf.any() and (_np(e["proportional"])[rows] == 1).any() and specular[rows].any() and ((flags & TRANSMISSION) != 0)[rows].any()
    s.close()


# ---- 3: against the render's shadow queue --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RENDER_FIXTURES)
def test_evaluations_equal_the_renders_shadow_queue(wfpt, name):
    s = open_scene(wfpt, name)
    d0 = Depth0(wfpt, s)
    sh = d0.shadow
    assert len(sh["d"]) > 0, "no next-event estimation in " + name
    rows = d0.rows_of(sh["d"][:, 3].copy().view(np.int32).astype(np.int64))
    usable, Ld, r_u, r_l = d0.nee()
    assert same(np.sort(rows), np.nonzero(usable)[0]), (len(rows), int(usable.sum()))
    for got, want, what in ((Ld[rows], sh["Ld"], "Ld"), (r_u[rows], sh["r_u"], "r_u"), (r_l[rows], sh["r_l"], "r_l"),
                            (_np(d0.ls["shadow_rays8"])[rows, :3], sh["o"][:, :3], "o"), (_np(d0.ls["shadow_rays8"])[rows, 3:6], sh["d"][:, :3], "d")):
        bad = (_bits(got) != _bits(want)).reshape(len(rows), -1).any(axis=1)
        assert not bad.any(), "%s: %s differs in %d of %d shadow items, first %r / %r" % (name, what, bad.sum(), len(rows), got[bad][0], want[bad][0])
    s.close()


# ---- 4: direct lighting, end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell64", "materials_lights"])
def test_direct_lighting_equals_the_renders_pixels_after_the_shadow_stage(wfpt, name):
    import torch
    s = open_scene(wfpt, name)
    d0 = Depth0(wfpt, s, shadow_stage=True)
    usable, Ld, r_u, r_l = d0.nee()
    occluded = _np(s.trace_device(d0.ls["shadow_rays8"], any_hit=True))
    lit = usable & (occluded == 0)
    assert lit.any() and (usable & (occluded != 0)).any()
    # KRecordShadowRay: Ld / (r_u + r_l).Average(), then pixel L + that; the pixel's L is the depth-0 emission (zero plus the terms, in order)
    Ld, r_u, r_l = (torch.from_numpy(x) for x in (Ld, r_u, r_l))
    term = Ld / average(r_u + r_l)
    emitted = d0.emitted.cpu()
    L = torch.where(torch.from_numpy(lit)[:, None], emitted + term, emitted)
    bad = (_bits(_np(L)) != _bits(d0.L)).any(axis=1)
    assert not bad.any(), "%s: %d of %d pixels differ, first %r / %r" % (name, bad.sum(), len(bad), _np(L)[bad][0], d0.L[bad][0])
    s.close()


# ---- 5: shapes -------------------------------------------------------------------------------------------------------------------------------
def test_prefixes_counts_misses_corrupt_headers_and_argument_errors(wfpt):
    import torch
    dev = torch.device("cuda", 0)
    _, hip = wfpt.libs()
    s = open_scene(wfpt, "matrix_lean_tex")
    fh = s.first_hit(0)
    n = fh["rays8"].shape[0]
    reg, b, ls, u4, e = make_and_eval(s, fh, dev)
    full = {k: _np(v) for k, v in list(b.items()) + list(e.items()) if k in MAKE_KEYS + WI_KEYS + U_KEYS}
    wi = ls["wi_pdf4"]

    def calls(k, n_device=None, it=None):
        it = it or (fh["planes_f"][:, :k].contiguous(), fh["planes_i"][:, :k].contiguous())
        bk = s.bsdf_device(fh["rays8"][:k].contiguous(), it, fh["lambda4"][:k].contiguous(), regularize=reg[:k].contiguous(), n_device=n_device)
        ek = s.bsdf_eval_device(bk, it, wi=wi[:k].contiguous(), u4=u4[:k].contiguous(), n_device=n_device)
        torch.cuda.synchronize()
        return bk, ek
    # prefixes: the plane stride changes with n, the rows do not
    for k in (1, 63, 64, 65, 255, 256, 257, 513):
        bk, ek = calls(k)
        assert same(_np(bk["rec"]), full["rec"][:, :k]) and same(_np(bk["bsdf4"]), full["bsdf4"][:k]), k
        for key in WI_KEYS + U_KEYS:
            assert same(_np(ek[key]), full[key][:k]), (k, key)
    # n_device below, at and above n: the rows past the count keep what they held (torch.empty: filled here with a sentinel first)
    k = 300
    it = (fh["planes_f"][:, :k].contiguous(), fh["planes_i"][:, :k].contiguous())
    _, hipl = wfpt.libs()
    for count in (137, k, k + 1000):
        m = min(count, k)
        nd = torch.tensor([count], dtype=torch.int32, device=dev)
        rec = torch.full((10, k, 4), -7.5, dtype=torch.float32, device=dev)
        b4 = torch.full((k, 4), -77, dtype=torch.int32, device=dev)
        outs = [torch.full((k, c), -7.5, dtype=torch.float32, device=dev) for c in (4, 4, 8, 4, 4)] + [torch.full((k, 4), -77, dtype=torch.int32, device=dev)]
        ts = [fh["rays8"][:k].contiguous(), it[0], it[1], fh["lambda4"][:k].contiguous(), reg[:k].contiguous(), rec, b4, nd]
        s._device_call("wf_bsdf_make_device", hipl.wf_bsdf_make_device, [C.c_void_p, C.c_int] + [C.c_void_p] * 8, ts, k, nd.data_ptr(), ts[0].data_ptr(), it[0].data_ptr(),
                       it[1].data_ptr(), ts[3].data_ptr(), ts[4].data_ptr(), rec.data_ptr(), b4.data_ptr())
        wk, uk = wi[:k].contiguous(), u4[:k].contiguous()
        s._device_call("wf_bsdf_eval_device", hipl.wf_bsdf_eval_device, [C.c_void_p, C.c_int] + [C.c_void_p] * 12, [rec, it[0], it[1], wk, uk, nd] + outs, k, nd.data_ptr(),
                       rec.data_ptr(), it[0].data_ptr(), it[1].data_ptr(), wk.data_ptr(), uk.data_ptr(), *[o.data_ptr() for o in outs])
        torch.cuda.synchronize()
        assert same(_np(rec)[:, :m], full["rec"][:, :m]) and same(_np(b4)[:m], full["bsdf4"][:m]), count
        assert (_np(rec)[:, m:] == -7.5).all() and (_np(b4)[m:] == -77).all(), count
        for o, key in zip(outs, WI_KEYS + U_KEYS):
            assert same(_np(o)[:m], full[key][:m]), (count, key)
            assert (_np(o)[m:] == (-77 if key == "sample_i4" else -7.5)).all(), (count, key)
    # a buffer of misses: zeros everywhere
    zf, zi = torch.zeros((11, 200, 4), dtype=torch.float32, device=dev), torch.zeros((2, 200, 4), dtype=torch.int32, device=dev)
    zi[0] = -1
    bz = s.bsdf_device(fh["rays8"][:200].contiguous(), (zf, zi), fh["lambda4"][:200].contiguous())
    ez = s.bsdf_eval_device(bz, (zf, zi), wi=wi[:200].contiguous(), u4=u4[:200].contiguous())
    torch.cuda.synchronize()
    assert not _np(bz["rec"]).any() and not _np(bz["bsdf4"]).any() and all(not _np(ez[key]).any() for key in WI_KEYS + U_KEYS)
    # a record whose header names no BSDF of this scene (a type or a material out of range, or the two at odds) is a row of zeros: the
    # header is checked against the scene before anything is indexed by it (RecordType, wf_boundary_bsdf.h), and the other rows stand
    rec = b["rec"].clone()
    live = np.nonzero(full["bsdf4"][:, 3] != 0)[0]
    assert len(live) > 8
    words = rec.view(torch.int32)
    bad_rows = live[:6]
    for row, (word, value) in zip(bad_rows, ((0, 99), (0, -5), (0, 0x7fffffff), (2, 1 << 20), (2, -3), (0, 0))):
        words[0, int(row), word] = value
    other = [int(t) for t in range(1, 11) if t != int(full["bsdf4"][live[6], 3])][0]
    words[0, int(live[6]), 0] = other                                          # a valid type that is not the material's
    bad_rows = np.append(bad_rows, live[6])
    ec = s.bsdf_eval_device(rec, fh, wi=wi, u4=u4)
    torch.cuda.synchronize()
    keep = np.ones(n, bool)
    keep[bad_rows] = False
    for key in WI_KEYS + U_KEYS:
        got = _np(ec[key])
        assert not got[bad_rows].any(), key
        assert same(got[keep], full[key][keep]), key
    _, again = calls(257)                                                      # ... and the process is as healthy as before
    assert same(_np(again["sample_f4"]), full["sample_f4"][:257])
    # argument errors are refused, by name, before anything is launched: the outputs keep their sentinel
    mk, ev = hip.wf_bsdf_make_device, hip.wf_bsdf_eval_device
    mk.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
    ev.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 12
    rec2 = torch.full((10, n, 4), -7.5, dtype=torch.float32, device=dev)
    b42 = torch.full((n, 4), -77, dtype=torch.int32, device=dev)
    good = [None, fh["rays8"].data_ptr(), fh["planes_f"].data_ptr(), fh["planes_i"].data_ptr(), fh["lambda4"].data_ptr(), None, rec2.data_ptr(), b42.data_ptr()]
    names = ["n_device", "rays8", "planes_f", "planes_i", "lambda4", "regularize", "bsdf_rec", "bsdf4"]
    torch.cuda.synchronize()
    for i, nm in enumerate(names):
        if good[i] is not None:
            a = list(good)
            a[i] = None
            assert mk(s.ctx, n, *a) != 0 and ("null " + nm).encode() in hip.wf_last_error(), nm
            a[i] = good[i] + 4
            assert mk(s.ctx, n, *a) != 0 and (nm + " is not aligned to 16").encode() in hip.wf_last_error(), nm
    for i in (0, 5):
        a = list(good)
        a[i] = reg.data_ptr() + 2
        assert mk(s.ctx, n, *a) != 0 and (names[i] + " is not aligned to 4").encode() in hip.wf_last_error()
    assert mk(s.ctx, -1, *good) != 0 and b"n = -1" in hip.wf_last_error()
    assert mk(s.ctx, 0, *good) == 0
    outs = [torch.full((n, c), -7.5, dtype=torch.float32, device=dev) for c in (4, 4, 8, 4, 4)] + [torch.full((n, 4), -77, dtype=torch.int32, device=dev)]
    egood = [None, b["rec"].data_ptr(), fh["planes_f"].data_ptr(), fh["planes_i"].data_ptr(), wi.data_ptr(), u4.data_ptr()] + [o.data_ptr() for o in outs]
    enames = ["n_device", "bsdf_rec", "planes_f", "planes_i", "wi4", "u4", "f4", "pdf4", "next_rays8", "sample_f4", "sample_pdf4", "sample_i4"]
    torch.cuda.synchronize()
    for i, nm in enumerate(enames):
        if i in (0, 4, 5):
            continue
        a = list(egood)
        a[i] = None
        assert ev(s.ctx, n, *a) != 0 and (nm + " is null" if i >= 6 else "null " + nm).encode() in hip.wf_last_error(), nm
        a[i] = egood[i] + 4
        assert ev(s.ctx, n, *a) != 0 and (nm + " is not aligned to 16").encode() in hip.wf_last_error(), nm
    a = list(egood)
    a[4] = a[5] = None
    assert ev(s.ctx, n, *a) != 0 and b"neither wi4 nor u4" in hip.wf_last_error()
    assert ev(s.ctx, -2, *egood) != 0 and b"n = -2" in hip.wf_last_error()
    stage(wfpt, s, "wf_sync")
    torch.cuda.synchronize()
    assert (_np(rec2) == -7.5).all() and (_np(b42) == -77).all() and all((_np(o) == (-77 if o.dtype == torch.int32 else -7.5)).all() for o in outs)
    # one half alone: the other half's outputs may be null and the given half's rows are the full call's
    only_wi = s.bsdf_eval_device(b, fh, wi=wi)
    only_u = s.bsdf_eval_device(b, fh, u4=u4)
    torch.cuda.synchronize()
    assert set(only_wi) & set(U_KEYS) == set() and all(same(_np(only_wi[k]), full[k]) for k in WI_KEYS) and all(same(_np(only_u[k]), full[k]) for k in U_KEYS)
    s.close()


# ---- 6: cleanliness --------------------------------------------------------------------------------------------------------------------------
def test_the_calls_leave_the_render_alone_and_queue_behind_torchs_stream(wfpt):
    import torch
    dev = torch.device("cuda", 0)
    s = open_scene(wfpt, "materials_lights")
    s.render()
    before = s.film().copy()
    stats = s.stats()
    fh = s.first_hit(0)
    n = fh["rays8"].shape[0]
    reg, b, ls, u4, e = make_and_eval(s, fh, dev)
    want = {k: _np(v).copy() for k, v in list(b.items()) + list(e.items()) if k in MAKE_KEYS + WI_KEYS + U_KEYS}
    # inputs that torch is still computing when the calls are issued, results consumed by torch ops right after: no host sync in between
    a = torch.rand((2048, 2048), device=dev)
    for _ in range(50):
        for _ in range(4):
            a = (a @ a).clamp_(0, 1)
        lam = fh["lambda4"] * (a[0, 0] * 0 + 1)                                # behind the matrix products on torch's stream; x * 1 is x
        wi = ls["wi_pdf4"] * (a[1, 1] * 0 + 1)
        bq = s.bsdf_device(fh["rays8"], fh, lam, regularize=reg)
        eq = s.bsdf_eval_device(bq, fh, wi=wi, u4=u4)
        got = {k: v.clone() for k, v in list(bq.items()) + list(eq.items()) if k in want}   # (torch ops, ordered after the calls)
    torch.cuda.synchronize()
    for k in want:
        assert same(_np(got[k]), want[k]), k
    assert same(s.film(), before)                                             # a hundred calls later the film is what the render left
    assert s.stats() == stats
    s.close()
