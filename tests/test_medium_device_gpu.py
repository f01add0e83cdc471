"""wf_medium_sample_device and wf_phase_device (include/wf_media.h) on the MI355X: the scene's media and phase functions on a caller's
device items.

Everything is bit for bit.  The expected values come from three independent places: the host program medium_check --eval (the per-row
bodies on the host — which tests/test_medium_host.py pins to the render's own stages on a one-slot WorkState; every row of this file
completes there, with its step count, before a GPU sees it), the render's own stages driven through the C ABI on the two scenes whose
camera sits in a medium (the ray slots, the pixels, the scattered rays, the shadow queue, the pixels after the transmittance stage), and
the calls themselves on other shapes of the same input."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from boundary_helpers import (_bits, _np, assert_rows_equal, begin_pass, download, open_scene, queue_size, renderer_before_torch, same, seeded,
                              stage)  # noqa: F401 (the fixture)
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

CHECK = os.path.join(ROOT, "pbrt-v4_amd", "_build", "medium_check")
FIXTURES = ["media_box", "media_preset", "media_instances", "nan_ray_grid_medium", "cloud_medium", "tempgrid_medium", "rgbgrid_medium", "animated_tr_routes",
            "camera_in_fog"]
CAMERA_IN_MEDIUM = ["camera_in_fog", "nan_ray_grid_medium"]
TRACK_KEYS = ("event4", "p_g4", "beta", "r_u", "r_l", "L")
WI_KEYS = ("p_pdf4",)
U_KEYS = ("sample4", "next_rays8")
MAGIC = 0x4d444331
N_ROWS = 2048


def eval_host(name, parts, head, tmp):
    """medium_check --eval -> (out.bin's bytes, the program's JSON line: rows and the tentative collisions they took on the host)"""
    a, b = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(a, "wb") as f:
        f.write(np.array(head, np.int32).tobytes())
        for x in parts:
            f.write(np.ascontiguousarray(x).tobytes())
    p = subprocess.run([CHECK, "--eval", os.path.join(GOLDEN, name + ".pbrt"), a, b], check=True, capture_output=True, text=True)
    return open(b, "rb").read(), (json.loads(p.stdout.strip().splitlines()[-1]) if p.stdout.strip() else {})


def host_track(name, rows, tmp):
    rays, medium, lam, beta, r_u, r_l, flags = rows
    n = len(medium)
    raw, info = eval_host(name, [rays, medium, lam, beta, r_u, r_l] + ([flags] if flags is not None else []), [MAGIC, 0, n, int(flags is not None), 0, 0, 0, 0], tmp)
    assert len(raw) == n * 16 * 6 and info["rows"] == n
    print(name, "host:", info)                                                  # every row completed on the host, in this many steps
    out = {"event4": np.frombuffer(raw, np.int32, 4 * n, 0).reshape(n, 4)}
    for k, key in enumerate(TRACK_KEYS[1:], 1):
        out[key] = np.frombuffer(raw, np.float32, 4 * n, 16 * n * k).reshape(n, 4)
    return out


def host_phase(name, rays, pg, wi, u4, tmp):
    n = len(pg)
    raw, _ = eval_host(name, [rays, pg] + [x for x in (wi, u4) if x is not None], [MAGIC, 1, n, 0, int(wi is not None), int(u4 is not None), 0, 0], tmp)
    out, off = {}, 0
    if wi is not None:
        out["p_pdf4"] = np.frombuffer(raw, np.float32, 4 * n, off).reshape(n, 4)
        off += 16 * n
    if u4 is not None:
        out["sample4"] = np.frombuffer(raw, np.float32, 4 * n, off).reshape(n, 4)
        out["next_rays8"] = np.frombuffer(raw, np.float32, 8 * n, off + 16 * n).reshape(n, 8)
        off += 48 * n
    assert off == len(raw)
    return out


def hit_tmax(hits):
    """the t of the closest-hit records (int32 [n, 8] words: prim, t, ...), +inf for a miss"""
    import torch
    t = hits[:, 1].contiguous().view(torch.float32)
    return torch.where(hits[:, 0] >= 0, t, torch.full_like(t, float("inf")))


def seeded_rows(s, n, seed, dev):
    """(rays8, medium, lambda4, beta, r_u, r_l, flags) as numpy: origins inside the scene's bounds, seeded directions of seeded lengths,
    media from -1 to one past the table's end + 1, tMax from trace_device or +inf, non-unit spectra, alternating flags, and a handful
    of rows that must not be walked (proven to be kind 0 on the host first)"""
    import torch
    rng = np.random.RandomState(seed)
    lo, hi = s.bounds()
    o = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d *= (rng.uniform(0.5, 1.5, size=(n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    time = rng.uniform(0, 1, size=n).astype(np.float32)
    rays = np.concatenate([o, d, np.full((n, 1), np.inf, np.float32), time[:, None]], axis=1).astype(np.float32)
    hits = s.trace_device(torch.from_numpy(rays).to(dev))
    tmax = _np(hit_tmax(hits))
    tmax[::4] = np.inf                                                          # every fourth ray runs on to infinity whatever lies in its way
    rays[:, 6] = tmax
    media = s.query("media")
    medium = rng.randint(-1, media + 2, size=n).astype(np.int32)
    nan = np.float32(np.nan)
    for row, (col, value) in zip(range(5, n, max(1, n // 9)), ((0, nan), (1, np.inf), (3, nan), (4, -np.inf), (6, nan), (6, -1.0), (3, None), (3, 1e-30), (3, 1e30))):
        if value is None:
            rays[row, 3:6] = 0
        elif value in (1e-30, 1e30):
            rays[row, 3:6] = (value, 0 if value < 1 else value, 0)
        else:
            rays[row, col] = value
        medium[row] = 0
    lam = np.sort(rng.uniform(380, 780, size=(n, 4)), axis=1).astype(np.float32)
    beta, r_u, r_l = (rng.uniform(0.25, 1.75, size=(n, 4)).astype(np.float32) for _ in range(3))
    flags = (np.arange(n) & 1).astype(np.int32)
    return rays, medium, lam, beta, r_u, r_l, flags


def phase_rays(rays):
    """the rays for the phase call: the handful of rows that must not be walked (a NaN, an infinite, a zero, a denormal-length or an
    overflowing ray) replaced by row 0's ray — the phase function of a NaN direction is a NaN, whose payload is nobody's contract"""
    out = rays.copy()
    n = len(out)
    out[5::max(1, n // 9)][:9] = out[0]
    assert np.isfinite(out[:, :6]).all()
    return out


def to_dev(rows, dev):
    import torch
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in rows]


# ---- 1: against the host oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_both_calls_equal_the_host_bodies(wfpt, name, tmp_path):
    import torch
    dev = torch.device("cuda", 0)
    s = open_scene(wfpt, name)
    assert s.query("medium_sample_variant") == s.query("medium_lean") and s.query("media") > 0
    rows = seeded_rows(s, N_ROWS, 5, dev)
    want = host_track(name, rows, str(tmp_path))                                # the host first: every row ends there
    kind = want["event4"][:, 0]
    assert (kind[5::max(1, N_ROWS // 9)][:9] == 0).all()                        # the rows that must not be walked are kind 0 on the host
    t = to_dev(rows, dev)
    got = s.medium_sample_device(*t[:6], flags=t[6])
    torch.cuda.synchronize()
    assert_rows_equal(got, want, TRACK_KEYS, name + " medium sample")
    assert same(_np(got["kind"]), kind) and same(_np(got["steps"]), want["event4"][:, 1]) and same(_np(got["p"]), want["p_g4"][:, :3])
    assert set(kind.tolist()) >= {0, 1, 3} and (want["event4"][:, 1] > 0).any()
    assert not want["L"][rows[6] == 0].any()                                    # no emission where the flag is clear
    zero = kind == 0
    assert all(not want[k][zero].any() for k in TRACK_KEYS)
    out_of_medium = (rows[1] < 0) & ~zero
    assert out_of_medium.any() and (kind[out_of_medium] == 1).all() and same(want["beta"][out_of_medium], rows[3][out_of_medium])
    # the phase call on every row (the rows without a scatter carry a zero p_g4: straight-line code, whatever the row holds)
    rng = np.random.RandomState(17)
    wi = rng.normal(size=(N_ROWS, 4)).astype(np.float32)
    wi[:, :3] /= np.linalg.norm(wi[:, :3], axis=1, keepdims=True)
    u4 = rng.uniform(0, 1, size=(N_ROWS, 4)).astype(np.float32)
    pr = phase_rays(rows[0])
    pw = host_phase(name, pr, want["p_g4"], wi, u4, str(tmp_path))
    pg = s.phase_device(torch.from_numpy(pr).to(dev), got["p_g4"], wi=torch.from_numpy(wi).to(dev), u4=torch.from_numpy(u4).to(dev))
    torch.cuda.synchronize()
    assert_rows_equal(pg, pw, WI_KEYS + U_KEYS, name + " phase")
    scatter = kind == 3
    assert (pw["sample4"][scatter, 1] > 0).all() and same(pw["next_rays8"][scatter, :3], want["p_g4"][scatter, :3]) and same(pw["next_rays8"][scatter, 7], rows[0][scatter, 7])
    s.close()


# ---- 2: against the render's unfused depth 0, the camera inside a medium ----------------------------------------------------------------
class CameraRows:
    """the camera samples of sample index 0 and their first hits, as boundary_helpers.Camera has them; the row of every pixel index comes
    from the render's own pixel table once a pass has begun (pixel_rows), so that a film with a crop window is served too"""

    def __init__(self, s):
        import torch
        self.rays, self.pix, self.lam, self.pdf, self.cam_w, self.fw = s.camera_samples_device(0)
        self.hits = s.trace_device(self.rays)
        torch.cuda.synchronize()

    def pixel_rows(self, wfpt, s):
        n_pix = s.width * s.height
        key = lambda xy: xy[:, 1].astype(np.int64) * (1 << 20) + xy[:, 0]
        mine, theirs = key(_np(self.pix)), key(download(wfpt, s, "pixel", "pPixel", n_pix, np.int32, 2))
        assert len(np.unique(mine)) == len(mine) == n_pix and same(np.sort(mine), np.sort(theirs))
        order = np.argsort(mine)
        self.row_of = order[np.searchsorted(mine[order], theirs)]              # pixel index -> row of the caller's arrays
        self.pixel_index = np.empty(n_pix, np.int64)
        self.pixel_index[self.row_of] = np.arange(n_pix)                        # row -> pixel index


class MediumDepth0:
    """the render's depth 0 up to its medium stage through the C ABI, and the caller's side of the same camera rays"""

    def __init__(self, wfpt, s, shadow_stage=False):
        import torch
        self.dev = dev = torch.device("cuda", 0)
        self.n_pix = n_pix = s.width * s.height
        self.cam = cam = CameraRows(s)
        self.medium_id = s.query("camera_medium")
        assert self.medium_id >= 0
        begin_pass(wfpt, s)
        cam.pixel_rows(wfpt, s)
        meta0 = download(wfpt, s, "ray0", "meta", n_pix, np.int32, 4)
        self.slot_row = cam.row_of[meta0[:, 0].astype(np.int64)]                # ray slot -> row of the caller's arrays
        assert same(np.sort(self.slot_row), np.arange(n_pix)) and (meta0[:, 3] == self.medium_id).all() and (meta0[:, 1] == 0).all()
        self.entry = {k: download(wfpt, s, "ray0", k, n_pix, np.float32, 4) for k in ("o", "d", "beta", "r_u", "r_l")}
        assert (self.entry["beta"] == 1).all() and (self.entry["r_u"] == 1).all() and (self.entry["r_l"] == 1).all()
        assert same(self.entry["o"][:, :3], _np(cam.rays)[self.slot_row, :3]) and same(self.entry["d"][:, :3], _np(cam.rays)[self.slot_row, 3:6])
        stage(wfpt, s, "wf_medium_sample", 0)
        stage(wfpt, s, "wf_sync")
        self.slot = {k: download(wfpt, s, "ray0", k, n_pix, np.float32, 4) for k in ("beta", "r_u", "r_l")}
        self.L_medium = download(wfpt, s, "pixel", "L", n_pix, np.float32, 4)[cam.pixel_index]
        self.s0 = download(wfpt, s, "pixel", "samples0", n_pix, np.float32, 4)[cam.pixel_index]
        self.s1 = download(wfpt, s, "pixel", "samples1", n_pix, np.float32, 4)[cam.pixel_index]
        m = queue_size(wfpt, s, "ray1")
        self.ray = {k: download(wfpt, s, "ray1", k, m, np.float32, 4) for k in ("o", "d", "beta", "r_u", "r_l")}
        self.ray["meta"] = download(wfpt, s, "ray1", "meta", m, np.int32, 4)
        k = queue_size(wfpt, s, "shadow")
        self.shadow = {key: download(wfpt, s, "shadow", key, k, np.float32, 4) for key in ("o", "d", "Ld", "r_u", "r_l")}
        if shadow_stage:
            stage(wfpt, s, "wf_intersect_shadow_tr", 0)
            stage(wfpt, s, "wf_sync")
            self.L = download(wfpt, s, "pixel", "L", n_pix, np.float32, 4)[cam.pixel_index]
        # the caller's side: trace_device -> medium_sample_device with the camera's medium and unit spectra
        self.rays = cam.rays.clone()
        self.rays[:, 6] = hit_tmax(cam.hits)
        self.medium = torch.full((n_pix,), self.medium_id, dtype=torch.int32, device=dev)
        one = torch.ones((n_pix, 4), dtype=torch.float32, device=dev)
        self.ev = s.medium_sample_device(self.rays, self.medium, cam.lam, one, one.clone(), one.clone())
        self.kind = _np(self.ev["kind"])
        self.scatter = self.kind == 3
        # the scattered rows: the vertex's light sample on the planes of a medium point, the phase function for its direction and sampled
        self.planes = s.medium_light_planes(self.ev["p_g4"], self.rays, self.medium)
        self.ls = s.sample_lights_device(self.planes, cam.lam, torch.from_numpy(self.s0).to(dev))
        u4 = np.stack([self.s1[:, 0], self.s1[:, 1], np.zeros(n_pix, np.float32), np.zeros(n_pix, np.float32)], axis=1)
        self.ph = s.phase_device(self.rays, self.ev["p_g4"], wi=self.ls["wi_pdf4"], u4=torch.from_numpy(np.ascontiguousarray(u4)).to(dev))
        torch.cuda.synchronize()

    def nee(self):
        """(usable rows, Ld, r_u, r_l) of the scatter's next-event estimation as KSampleMediumScattering computes them, in torch fp32"""
        import torch
        beta, r_u = self.ev["beta"].cpu(), self.ev["r_u"].cpu()
        p, pdf = self.ph["p"].cpu(), self.ph["pdf"].cpu()
        L, lpdf, pmf, delta = self.ls["L"].cpu(), self.ls["pdf"].cpu(), self.ls["pmf"].cpu(), (self.ls["flags"].cpu() & 1) != 0
        Ld = (beta * p[:, None]) * L                                           # beta = wbeta * phase.p;  Ld = beta * ls.L
        ru = r_u * torch.where(delta, torch.zeros_like(pdf), pdf)[:, None]     # wr_u * phasePDF
        rl = r_u * (lpdf * pmf)[:, None]                                       # wr_u * (ls.pdf * lightPMF)
        usable = torch.from_numpy(self.scatter) & (lpdf > 0) & (L != 0).any(dim=1)
        return _np(usable), _np(Ld), _np(ru.contiguous()), _np(rl.contiguous())


def rows_differ(got, want):
    return (_bits(got) != _bits(want)).reshape(len(got), -1).any(axis=1)


@pytest.mark.parametrize("name", CAMERA_IN_MEDIUM)
def test_events_equal_the_renders_medium_stage(wfpt, name):
    s = open_scene(wfpt, name)
    d0 = MediumDepth0(wfpt, s)
    kind = d0.kind
    assert (kind != 0).all() and (kind == 1).any() and (kind == 3).any(), np.bincount(kind, minlength=4)
    written = np.isin(kind, (1, 3))[d0.slot_row]                               # the stage writes the slots of arriving and scattering rays back
    for key in ("beta", "r_u", "r_l"):
        got = _np(d0.ev[key])[d0.slot_row]
        bad = rows_differ(got[written], d0.slot[key][written])
        assert not bad.any(), "%s: %s differs in %d of %d ray slots, first %r / %r" % (name, key, bad.sum(), written.sum(), got[written][bad][0], d0.slot[key][written][bad][0])
    bad = rows_differ(_np(d0.ev["L"]), d0.L_medium)
    assert not bad.any(), "%s: L differs in %d pixels, first %r / %r" % (name, bad.sum(), _np(d0.ev["L"])[bad][0], d0.L_medium[bad][0])
    if name == "camera_in_fog":
        assert d0.L_medium.any()                                               # the fog emits
    s.close()


@pytest.mark.parametrize("name", CAMERA_IN_MEDIUM)
def test_phase_samples_equal_the_renders_scattered_rays(wfpt, name):
    import torch
    s = open_scene(wfpt, name)
    d0 = MediumDepth0(wfpt, s)
    q = d0.ray
    scattered = q["meta"][:, 1] == 1                                           # (depth 0 items of this queue: rays that went on through an interface)
    q = {k: v[scattered] for k, v in q.items()}
    pdf = d0.ph["sample_pdf"].cpu()
    pushed = d0.scatter & (_np(pdf) != 0)
    rows = d0.cam.row_of[q["meta"][:, 0].astype(np.int64)]
    assert same(np.sort(rows), np.nonzero(pushed)[0]) and len(rows) > 0, (len(rows), int(pushed.sum()))
    wbeta, wr_u = d0.ev["beta"].cpu(), d0.ev["r_u"].cpu()
    beta = _np(wbeta * pdf[:, None] / pdf[:, None])                            # wbeta * phaseSample.p / phaseSample.pdf, p == pdf
    r_l = _np(wr_u / pdf[:, None])
    nxt = _np(d0.ph["next_rays8"])[rows]
    assert np.isinf(nxt[:, 6]).all()
    for got, want, what in ((nxt[:, :3], q["o"][:, :3], "o"), (nxt[:, 7], q["o"][:, 3], "time"), (nxt[:, 3:6], q["d"][:, :3], "d"), (beta[rows], q["beta"], "beta"),
                            (_np(wr_u)[rows], q["r_u"], "r_u"), (r_l[rows], q["r_l"], "r_l")):
        bad = rows_differ(got, want)
        assert not bad.any(), "%s: %s differs in %d of %d rays, first %r / %r" % (name, what, bad.sum(), len(rows), got[bad][0], want[bad][0])
    meta = np.stack([d0.cam.pixel_index[rows].astype(np.int32), np.ones(len(rows), np.int32), np.full(len(rows), 2, np.int32), np.full(len(rows), d0.medium_id, np.int32)], axis=1)
    assert same(meta, q["meta"])                                               # pixel, depth + 1, any-non-specular, the medium the ray was in
    assert (q["d"][:, 3] == 1).all()                                           # etaScale
    s.close()


@pytest.mark.parametrize("name", CAMERA_IN_MEDIUM)
def test_light_and_phase_equal_the_renders_shadow_queue(wfpt, name):
    s = open_scene(wfpt, name)
    d0 = MediumDepth0(wfpt, s)
    sh = d0.shadow
    assert len(sh["d"]) > 0, "no next-event estimation in " + name
    rows = d0.cam.row_of[sh["d"][:, 3].copy().view(np.int32).astype(np.int64)]
    usable, Ld, r_u, r_l = d0.nee()
    assert same(np.sort(rows), np.nonzero(usable)[0]), (len(rows), int(usable.sum()))
    sr = _np(d0.ls["shadow_rays8"])
    for got, want, what in ((sr[rows, :3], sh["o"][:, :3], "o"), (sr[rows, 6], sh["o"][:, 3], "tMax"), (sr[rows, 3:6], sh["d"][:, :3], "d"), (Ld[rows], sh["Ld"], "Ld"),
                            (r_u[rows], sh["r_u"], "r_u"), (r_l[rows], sh["r_l"], "r_l")):
        bad = rows_differ(got, want)
        assert not bad.any(), "%s: %s differs in %d of %d shadow items, first %r / %r" % (name, what, bad.sum(), len(rows), got[bad][0], want[bad][0])
    assert (_np(d0.ls["medium"])[rows] == d0.medium_id).all()
    if name == "camera_in_fog":                                                # the area light, the point light and the infinite light are all sampled
        assert len(set(_np(d0.ls["light"])[rows].tolist())) >= 3
    s.close()


@pytest.mark.parametrize("name", CAMERA_IN_MEDIUM)
def test_medium_lighting_equals_the_renders_pixels_after_the_transmittance_stage(wfpt, name):
    import torch
    s = open_scene(wfpt, name)
    d0 = MediumDepth0(wfpt, s, shadow_stage=True)
    usable, Ld, r_u, r_l = d0.nee()
    assert usable.any()
    idx = torch.from_numpy(np.nonzero(usable)[0]).to(d0.dev)                   # the rows with a shadow item, as the caller's own compaction
    take = lambda x: (x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(d0.dev))[idx].contiguous()
    out = s.trace_shadow_tr_device(take(d0.ls["shadow_rays8"]), take(d0.ls["medium"]), take(d0.cam.lam), take(Ld), take(r_u), take(r_l))
    torch.cuda.synchronize()
    # the pixel's L after the stages run here: the medium's emission, then what the shadow ray adds (a pixel has one of each at most)
    L = _np(d0.ev["L"]).copy()
    L[usable] = L[usable] + _np(out)
    bad = rows_differ(L, d0.L)
    assert not bad.any(), "%s: %d of %d pixels differ, first %r / %r" % (name, bad.sum(), len(bad), L[bad][0], d0.L[bad][0])
    assert _np(out).any()
    s.close()


# ---- 3: shapes ---------------------------------------------------------------------------------------------------------------------------
def test_prefixes_counts_in_place_halves_unwalked_rows_and_argument_errors(wfpt, tmp_path):
    import torch
    dev = torch.device("cuda", 0)
    _, hip = wfpt.libs()
    name = "media_box"
    s = open_scene(wfpt, name)
    rows = seeded_rows(s, 600, 23, dev)
    want = host_track(name, rows, str(tmp_path))                                # the host first
    t = to_dev(rows, dev)
    full_t = s.medium_sample_device(*t[:6], flags=t[6])
    rng = np.random.RandomState(3)
    wi = torch.from_numpy(rng.normal(size=(600, 4)).astype(np.float32)).to(dev)
    u4 = torch.from_numpy(rng.uniform(0, 1, size=(600, 4)).astype(np.float32)).to(dev)
    pr = torch.from_numpy(phase_rays(rows[0])).to(dev)
    full_p = s.phase_device(pr, full_t["p_g4"], wi=wi, u4=u4)
    torch.cuda.synchronize()
    full = {k: _np(v).copy() for k, v in list(full_t.items()) + list(full_p.items()) if k in TRACK_KEYS + WI_KEYS + U_KEYS}
    assert_rows_equal(full, want, TRACK_KEYS, "media_box, 600 rows")
    pg = full_t["p_g4"]
    # prefixes
    for k in (1, 63, 64, 65, 255, 256, 257, 513):
        tk = s.medium_sample_device(*[x[:k].contiguous() for x in t[:6]], flags=t[6][:k].contiguous())
        pk = s.phase_device(pr[:k].contiguous(), pg[:k].contiguous(), wi=wi[:k].contiguous(), u4=u4[:k].contiguous())
        torch.cuda.synchronize()
        for key in TRACK_KEYS:
            assert same(_np(tk[key]), full[key][:k]), (k, key)
        for key in WI_KEYS + U_KEYS:
            assert same(_np(pk[key]), full[key][:k]), (k, key)
    # n_device below, at and above n: the rows past the count keep their sentinel
    k = 300
    tk = [x[:k].contiguous() for x in t]
    for count in (137, k, k + 1000):
        m = min(count, k)
        nd = torch.tensor([count], dtype=torch.int32, device=dev)
        out = {"event4": torch.full((k, 4), -77, dtype=torch.int32, device=dev)}
        out.update({key: torch.full((k, 4), -7.5, dtype=torch.float32, device=dev) for key in TRACK_KEYS[1:]})
        got = s.medium_sample_device(*tk[:6], flags=tk[6], n_device=nd, out=out)
        pouts = [torch.full((k, c), -7.5, dtype=torch.float32, device=dev) for c in (4, 4, 8)]
        wk, uk, pgk = wi[:k].contiguous(), u4[:k].contiguous(), pg[:k].contiguous()
        prk = pr[:k].contiguous()
        s._device_call("wf_phase_device", hip.wf_phase_device, [C.c_void_p, C.c_int] + [C.c_void_p] * 8, [prk, pgk, wk, uk, nd] + pouts, k, nd.data_ptr(), prk.data_ptr(),
                       pgk.data_ptr(), wk.data_ptr(), uk.data_ptr(), *[o.data_ptr() for o in pouts])
        torch.cuda.synchronize()
        for key in TRACK_KEYS:
            assert got[key] is out[key] and same(_np(out[key])[:m], full[key][:m]), (count, key)
            assert (_np(out[key])[m:] == (-77 if key == "event4" else -7.5)).all(), (count, key)
        for o, key in zip(pouts, WI_KEYS + U_KEYS):
            assert same(_np(o)[:m], full[key][:m]) and (_np(o)[m:] == -7.5).all(), (count, key)
    # in place: the spectra written over their inputs equal the separate outputs
    b2, u2, l2 = t[3].clone(), t[4].clone(), t[5].clone()
    inplace = s.medium_sample_device(t[0], t[1], t[2], b2, u2, l2, flags=t[6], out={"beta": b2, "r_u": u2, "r_l": l2})
    torch.cuda.synchronize()
    assert inplace["beta"] is b2 and all(same(_np(inplace[key]), full[key]) for key in TRACK_KEYS)
    # flags = None reads as all 1
    all_on = s.medium_sample_device(*t[:6])
    ones = s.medium_sample_device(*t[:6], flags=torch.ones_like(t[6]))
    torch.cuda.synchronize()
    assert all(same(_np(all_on[key]), _np(ones[key])) for key in TRACK_KEYS) and _np(all_on["L"]).any()
    # one half of the phase call alone equals the full call
    only_wi = s.phase_device(pr, pg, wi=wi)
    only_u = s.phase_device(pr, pg, u4=u4)
    torch.cuda.synchronize()
    assert set(only_wi) & set(U_KEYS) == set() and set(only_u) & set(WI_KEYS) == set()
    assert all(same(_np(only_wi[key]), full[key]) for key in WI_KEYS) and all(same(_np(only_u[key]), full[key]) for key in U_KEYS)
    # the rows proven on the host to be kind 0 give zeros, and the rows beside them stand (they equal the host's: above)
    zero = want["event4"][:, 0] == 0
    assert zero.sum() >= 9 and all(not full[key][zero].any() for key in TRACK_KEYS) and (full["event4"][~zero, 0] > 0).all()
    # argument errors are refused, by name, before anything is launched: the outputs keep their sentinel
    n = 600
    ms, ph = hip.wf_medium_sample_device, hip.wf_phase_device
    ms.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 14
    ph.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
    ev = torch.full((n, 4), -77, dtype=torch.int32, device=dev)
    outs = [torch.full((n, 4), -7.5, dtype=torch.float32, device=dev) for _ in range(5)]
    good = [None] + [x.data_ptr() for x in t[:6]] + [t[6].data_ptr(), ev.data_ptr()] + [o.data_ptr() for o in outs]
    names = ["n_device", "rays8", "medium", "lambda4", "beta4", "r_u4", "r_l4", "flags", "event4", "p_g4", "out_beta4", "out_r_u4", "out_r_l4", "L4"]
    torch.cuda.synchronize()
    for i, nm in enumerate(names):
        if nm not in ("n_device", "flags"):
            a = list(good)
            a[i] = None
            assert ms(s.ctx, n, *a) != 0 and ("null " + nm).encode() in hip.wf_last_error(), nm
        a = list(good)
        if nm in ("n_device", "medium", "flags"):
            a[i] = t[1].data_ptr() + 2
            assert ms(s.ctx, n, *a) != 0 and (nm + " is not aligned to 4").encode() in hip.wf_last_error(), nm
        else:
            a[i] = good[i] + 4
            assert ms(s.ctx, n, *a) != 0 and (nm + " is not aligned to 16").encode() in hip.wf_last_error(), nm
    assert ms(s.ctx, -1, *good) != 0 and b"n = -1" in hip.wf_last_error()
    assert ms(s.ctx, 0, *good) == 0
    pouts = [torch.full((n, c), -7.5, dtype=torch.float32, device=dev) for c in (4, 4, 8)]
    pgood = [None, t[0].data_ptr(), pg.data_ptr(), wi.data_ptr(), u4.data_ptr()] + [o.data_ptr() for o in pouts]
    pnames = ["n_device", "rays8", "p_g4", "wi4", "u4", "p_pdf4", "sample4", "next_rays8"]
    torch.cuda.synchronize()
    for i, nm in enumerate(pnames):
        if i in (0, 3, 4):
            continue
        a = list(pgood)
        a[i] = None
        assert ph(s.ctx, n, *a) != 0 and (nm + " is null" if i >= 5 else "null " + nm).encode() in hip.wf_last_error(), nm
        a[i] = pgood[i] + 4
        assert ph(s.ctx, n, *a) != 0 and (nm + " is not aligned to 16").encode() in hip.wf_last_error(), nm
    for i in (3, 4):
        a = list(pgood)
        a[i] = pgood[i] + 4
        assert ph(s.ctx, n, *a) != 0 and (pnames[i] + " is not aligned to 16").encode() in hip.wf_last_error()
    a = list(pgood)
    a[0] = t[1].data_ptr() + 2
    assert ph(s.ctx, n, *a) != 0 and b"n_device is not aligned to 4" in hip.wf_last_error()
    a = list(pgood)
    a[3] = a[4] = None
    assert ph(s.ctx, n, *a) != 0 and b"neither wi4 nor u4" in hip.wf_last_error()
    assert ph(s.ctx, -2, *pgood) != 0 and b"n = -2" in hip.wf_last_error()
    assert ph(s.ctx, 0, *pgood) == 0
    stage(wfpt, s, "wf_sync")
    torch.cuda.synchronize()
    assert (_np(ev) == -77).all() and all((_np(o) == -7.5).all() for o in outs + pouts)
    s.close()
    # a scene without media is refused by both calls
    s = open_scene(wfpt, "cornell64")
    assert s.query("media") == 0 and s.query("camera_medium") == -1
    with pytest.raises(wfpt.WfError, match="the scene has no media"):
        s.medium_sample_device(*[x[:8].contiguous() for x in t[:6]])
    with pytest.raises(wfpt.WfError, match="the scene has no media"):
        s.phase_device(t[0][:8].contiguous(), pg[:8].contiguous(), wi=wi[:8].contiguous())
    s.close()


# ---- 4: cleanliness ----------------------------------------------------------------------------------------------------------------------
def test_the_calls_leave_the_render_alone_and_queue_behind_torchs_stream(wfpt):
    import torch
    dev = torch.device("cuda", 0)
    s = open_scene(wfpt, "camera_in_fog")
    s.render()
    before = s.film().copy()
    stats = s.stats()
    rows = seeded_rows(s, 1024, 41, dev)
    t = to_dev(rows, dev)
    pr = torch.from_numpy(phase_rays(rows[0])).to(dev)
    u4 = seeded(1024, 4, 7, dev)
    ev = s.medium_sample_device(*t[:6], flags=t[6])
    ph = s.phase_device(pr, ev["p_g4"], wi=u4, u4=u4)
    torch.cuda.synchronize()
    want = {k: _np(v).copy() for k, v in list(ev.items()) + list(ph.items()) if k in TRACK_KEYS + WI_KEYS + U_KEYS}
    # inputs that torch is still computing when the calls are issued, results consumed by torch ops right after: no host sync in between
    a = torch.rand((2048, 2048), device=dev)
    for _ in range(50):
        for _ in range(4):
            a = (a @ a).clamp_(0, 1)
        lam = t[2] * (a[0, 0] * 0 + 1)                                         # behind the matrix products on torch's stream; x * 1 is x
        beta = t[3] * (a[1, 1] * 0 + 1)
        eq = s.medium_sample_device(t[0], t[1], lam, beta, t[4], t[5], flags=t[6])
        pq = s.phase_device(pr, eq["p_g4"], wi=u4, u4=u4)
        got = {k: v.clone() for k, v in list(eq.items()) + list(pq.items()) if k in want}   # (torch ops, ordered after the calls)
    torch.cuda.synchronize()
    for k in want:
        assert same(_np(got[k]), want[k]), k
    assert same(s.film(), before)                                              # a hundred calls later the film is what the render left
    assert s.stats() == stats
    s.close()
