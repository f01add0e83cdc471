"""The film developed on the device (wf_film_develop_device, Scene.image_tensor / film_channels_tensor) against the host loops of
csrc/host/image_io.cpp (Scene.image / film_to_rgb / film_channels): equality of the uint32 views of every value, never allclose.
Every film is 64 x 64 = 16 blocks of 256 lanes.

The golden scene files all say `"bool savefp16" [ false ]`; the savefp16-true case of each is the same text with that value replaced."""
import ctypes as C
import os

import numpy as np
import pytest

from boundary_helpers import _f32_bits as bits
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GB_DTYPE = np.dtype([("gbuffer_weight_sum", "<f8"), ("rgb_albedo_sum", "<f8", 3), ("var_n", "<i8", 3), ("var_mean", "<f4", 3), ("var_s", "<f4", 3),
                     ("p_sum", "<f4", 3), ("dzdx_sum", "<f4"), ("dzdy_sum", "<f4"), ("n_sum", "<f4", 3), ("ns_sum", "<f4", 3), ("uv_sum", "<f4", 2),
                     ("pad", "<f4")])   # wf_gbuffer_pixel, include/wf_abi.h
assert GB_DTYPE.itemsize == 136

_scenes = {}


def scene(wfpt, name, fp16):
    """the golden scene `name` with savefp16 = fp16, with a renderer, rendered at 4 spp (one per module; the fabricated tests overwrite
    its accumulators, so a test that wants the render calls rendered())"""
    key = (name, fp16)
    if key not in _scenes:
        path = os.path.join(GOLDEN, name + ".pbrt")
        if fp16:
            text = open(path).read()
            assert '"bool savefp16" [ false ]' in text
            s = wfpt.Scene(text=text.replace('"bool savefp16" [ false ]', '"bool savefp16" [ true ]'), spp=4)
        else:
            s = wfpt.Scene(path=path, spp=4)
        assert bool(s.info.save_fp16) == fp16 and (s.height, s.width) == (64, 64)
        s.create_renderer(0)
        _scenes[key] = s
    return _scenes[key]


def rendered(wfpt, name, fp16):
    s = scene(wfpt, name, fp16)
    s.clear_film()
    s.render()
    return s


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for s in _scenes.values():
        s.close()
    _scenes.clear()


def same_bits(got, want):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d values differ, first at %s: 0x%08x, host 0x%08x" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def host_of(t):
    return t.cpu().numpy()


# ---- 1. rendered RGB ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [False, True])
def test_rendered_rgb(wfpt, fp16):
    import torch
    s = scene(wfpt, "cornell64", fp16)
    s.clear_film()
    s.render()
    straight = s.image_tensor()   # straight after render(), nothing in between
    want = s.image()
    assert straight.dtype == torch.float32 and tuple(straight.shape) == (64, 64, 3) and straight.device == torch.device("cuda", 0)
    assert np.isfinite(want).all() and want.mean() > 0.01
    same_bits(host_of(straight), want)
    same_bits(host_of(s.image_tensor()), want)
    out = torch.full((64, 64, 3), -1.0, dtype=torch.float32, device="cuda:0")
    assert s.image_tensor(out=out) is out
    same_bits(host_of(out), want)
    assert s.nan_values == 0
    names, t = s.film_channels_tensor()
    assert names == ["R", "G", "B"]
    same_bits(host_of(t), want)
    if fp16:   # the image holds half values
        assert (want.astype(np.float16).astype(np.float32) == want).all()


# ---- 2. fabricated RGB --------------------------------------------------------------------------------------------------------------
def fabricated_rgb():
    rng = np.random.default_rng(20240611)
    a = np.empty((64, 64, 4), np.float64)
    a[..., :3] = 10.0 ** rng.uniform(-9, 6, (64, 64, 3))
    a[..., 3] = rng.uniform(0.5, 4.0, (64, 64))
    nan, inf = np.nan, np.inf
    special = [
        (1.5, 2.5, 3.5, 0.0),                      # weightSum == 0 with nonzero sums: not divided
        (nan, 1.0, 1.0, 2.0),                      # NaN in one sum channel
        (1.0, 1.0, nan, 0.0),
        (0.25, nan, 0.5, 1.0),
        (inf, 0.0, 0.0, 1.0),                      # +inf, one channel (no inf - inf: every matrix entry is nonzero, asserted by the test)
        (0.0, 0.0, inf, 2.0),
        (-1.0, -2.0, -3.0, 4.0),                   # negative sums
        (-1e-7, 3.0, -2e5, 0.5),
        (65504.0, 65504.0, 65504.0, 1.0),          # around the clamp and the overflow threshold
        (65510.0, 65510.0, 65510.0, 1.0),
        (65520.0, 65520.0, 65520.0, 1.0),
        (131040.0, 131040.0, 131040.0, 2.0),
        (7e4, 7e4, 7e4, 1.0),
        (1e6, 2e6, 3e6, 1.0),
        (3e-5, 2e-6, 5e-8, 1.0),                   # quotients in the half-subnormal range
        (6.1e-5, 6.0e-5, 5.96e-8, 1.0),
        (2.98e-8, 2.99e-8, 8.9e-8, 1.0),           # around half of the smallest subnormal: ties at 2^-25
        (1.0 + 2.0 ** -30, 1.0 / 3.0, 1e-46, 1.0),  # fp64 values that fp32 does not hold
        (0.1, 0.7, 1e-40, 3.0),
        (1e300, 1.0, 1.0, 1e-300),                 # (float) of the sum is inf, of the weight 0
    ]
    n_nan = 0
    for k, px in enumerate(special):
        y, x = (7 * k + 3) % 64, (37 * k + 11) % 64   # spread over several blocks
        a[y, x] = px
        n_nan += any(v != v for v in px)
    return a, n_nan


@pytest.mark.parametrize("fp16", [False, True])
def test_fabricated_rgb(wfpt, fp16):
    import torch
    _, hip = wfpt.libs()
    s = scene(wfpt, "cornell64", fp16)
    # the film's output matrix, one column per unit pixel: every entry nonzero, so an infinite sum in one channel meets no 0 * inf and
    # the NaN values are exactly three per pixel that was given a NaN
    unit = np.zeros((64, 64, 4), np.float64)
    unit[..., 3] = 1
    for c in range(3):
        unit[0, c, c] = 1
    assert (s.film_to_rgb(unit)[0, :3] != 0).all()
    a, n_nan = fabricated_rgb()
    want = s.film_to_rgb(a)
    assert np.isinf(want).any()   # (an infinite value of either sign without savefp16, -inf with it: only values above 65504 are clamped)
    s.film_from_tensor(torch.from_numpy(a).to("cuda:0"))
    same_bits(host_of(s.image_tensor()), want)
    assert s.nan_values == 3 * n_nan
    s.clear_film()
    wfpt._check(hip.wf_film_upload(s.ctx, a.ctypes.data), "wf_film_upload")
    names, t = s.film_channels_tensor()
    assert names == ["R", "G", "B"] and s.nan_values == 3 * n_nan
    same_bits(host_of(t), want)
    same_bits(s.image(), want)   # (the upload itself: the host path sees the same accumulators)


# ---- 3. rendered spectral and GBuffer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("name,channels", [("spectral_film", 11), ("gbuffer_film", 25)])
def test_rendered_channels(wfpt, name, channels, fp16):
    import torch
    s = rendered(wfpt, name, fp16)
    names, t = s.film_channels_tensor()
    want_names, want = s.film_channels()
    assert names == want_names and len(names) == channels
    assert t.dtype == torch.float32 and tuple(t.shape) == (64, 64, channels)
    assert want[..., :3].mean() > 0.01
    same_bits(host_of(t), want)
    assert s.nan_values == 0
    out = torch.full((64, 64, channels), -1.0, dtype=torch.float32, device="cuda:0")
    s.film_channels_tensor(out=out)
    same_bits(host_of(out), want)
    same_bits(host_of(s.image_tensor()), s.image())
    same_bits(host_of(s.image_tensor()), want[..., :3])


# ---- 4. fabricated spectral ----------------------------------------------------------------------------------------------------------
def half_probe_values():
    """fp32-exact bucket values for RoundToHalf: every finite half, the midpoint to the next one (a tie), one fp32 ulp either side of the
    midpoint — the subnormal halves are the first 1024 — 65504, 65519.996, 65520 and above, each with both signs"""
    h = np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float32)
    nxt = np.append(h[1:], np.float32(65536.0))          # (the half after 65504 would be 65536: the midpoint is 65520)
    mid = ((h.astype(np.float64) + nxt.astype(np.float64)) / 2).astype(np.float32)
    assert (mid.astype(np.float64) * 2 == h.astype(np.float64) + nxt.astype(np.float64)).all() and mid[-1] == 65520.0
    below, above = np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))
    extra = np.array([65504.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e9, 3.4e38, np.inf, 1e-30, 1e-42], np.float32)
    v = np.concatenate([h, below, mid, above, extra])
    return np.concatenate([v, -v]).astype(np.float32)


@pytest.mark.parametrize("fp16", [False, True])
def test_fabricated_spectral(wfpt, fp16):
    _, hip = wfpt.libs()
    s = rendered(wfpt, "spectral_film", fp16)
    assert np.isfinite(s.film()).all()   # the RGB part adds no NaN values
    nb = 8
    acc = np.empty((64, 64, 2 * nb), np.float64)
    wfpt._check(hip.wf_film_spectral_download(s.ctx, acc.ctypes.data), "wf_film_spectral_download")
    probes = half_probe_values()
    slots = 64 * 64 * nb
    # special slots of every round: weight 0, weight < 0 (channel 0), a NaN sum and inf / inf (stored as 0 and counted)
    special = {5: (3.0, 0.0), 6: (3.0, -1.0), 7: (np.nan, 1.0), 9: (np.inf, np.inf), 4001: (-2.0, -0.0), 30000: (np.nan, 2.0)}
    free = np.array([i for i in range(slots) if i not in special])
    rounds = 0
    for start in range(0, len(probes), len(free)):
        chunk = probes[start:start + len(free)]
        sums, weights = np.ones(slots, np.float64), np.ones(slots, np.float64)
        sums[free[:len(chunk)]] = chunk
        for i, (sm, wt) in special.items():
            sums[i], weights[i] = sm, wt
        acc[..., :nb] = sums.reshape(64, 64, nb)
        acc[..., nb:] = weights.reshape(64, 64, nb)
        wfpt._check(hip.wf_film_spectral_upload(s.ctx, acc.ctypes.data), "wf_film_spectral_upload")
        names, t = s.film_channels_tensor()
        got = host_of(t)
        assert s.nan_values == 3   # slots 7, 9 and 30000
        want_names, want = s.film_channels()
        assert names == want_names
        same_bits(got, want)
        buckets = got[..., 3:].reshape(slots)
        assert (bits(buckets[list(special)]) == 0).all()
        if not fp16:   # the values pass through unchanged
            assert (bits(buckets[free[:len(chunk)]]) == bits(chunk)).all()
        else:          # ... or are what numpy's float16 makes of them (round to nearest even, overflow to inf from 65520), clamped above
            with np.errstate(over="ignore"):
                expect = np.minimum(chunk, np.float32(65504.0)).astype(np.float16).astype(np.float32)
            assert (bits(buckets[free[:len(chunk)]]) == bits(expect)).all()
        rounds += 1
    assert rounds == -(-len(probes) // len(free)) and rounds >= 7


# ---- 5. fabricated GBuffer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [False, True])
def test_fabricated_gbuffer(wfpt, fp16):
    _, hip = wfpt.libs()
    s = rendered(wfpt, "gbuffer_film", fp16)
    assert np.isfinite(s.film()).all()
    gb = np.empty((64, 64), GB_DTYPE)
    wfpt._check(hip.wf_film_gbuffer_download(s.ctx, gb.ctypes.data), "wf_film_gbuffer_download")
    assert np.isfinite(gb["p_sum"]).all() and np.isfinite(gb["uv_sum"]).all() and gb["gbuffer_weight_sum"].max() > 0
    gb["gbuffer_weight_sum"][3, 5] = 0                      # geometry sums not divided
    gb["n_sum"][9, 60] = 0                                  # zero-length normals: (0, 0, 0)
    gb["ns_sum"][17, 1] = 0
    gb["n_sum"][17, 2] = (1e-30, 0, 0)                      # the squared length underflows to 0
    gb["var_n"][25, 33] = (0, 1, 2)
    gb["var_n"][25, 34] = (2, 0, 1)
    gb["var_mean"][31, 7] = 0
    gb["var_mean"][31, 8] = (0, -0.0, 1.0)
    gb["dzdx_sum"][40, 40] = -3.25
    gb["dzdy_sum"][40, 40] = -0.0
    gb["p_sum"][47, 63] = np.nan                            # three NaN values: P.X P.Y P.Z
    gb["uv_sum"][63, 0] = (np.nan, 0.5)                     # one more
    gb["var_s"][50, 50] = (1e30, 7e4, 65520.0)              # channels that are NOT clamped: above the half range they become inf
    gb["var_n"][50, 50] = 2
    gb["var_mean"][50, 50] = (1e-20, 1.0, 1.0)
    gb["rgb_albedo_sum"][55, 21] = (1e300, 1.0 / 3.0, 1e-46)
    wfpt._check(hip.wf_film_gbuffer_upload(s.ctx, gb.ctypes.data), "wf_film_gbuffer_upload")
    names, t = s.film_channels_tensor()
    assert s.nan_values == 4
    want_names, want = s.film_channels()
    assert names == want_names
    got = host_of(t)
    same_bits(got, want)
    ch = {n: got[..., i] for i, n in enumerate(names)}
    assert all(ch[n][9, 60] == 0 for n in ("N.X", "N.Y", "N.Z")) and all(ch[n][17, 1] == 0 for n in ("Ns.X", "Ns.Y", "Ns.Z"))
    assert ch["dzdx"][40, 40] > 0 and ch["P.X"][47, 63] == 0 and ch["Variance.R"][25, 33] == 0 and ch["Variance.G"][25, 33] == 0
    assert np.isinf(ch["RelativeVariance.R"][50, 50]) and np.isinf(ch["Variance.R"][50, 50]) == fp16 and np.isinf(ch["Variance.G"][50, 50]) == fp16


# ---- 6. upload / download round trip -------------------------------------------------------------------------------------------------
def test_upload_download_round_trip(wfpt):
    _, hip = wfpt.libs()
    rng = np.random.default_rng(5)
    s = scene(wfpt, "spectral_film", False)
    a = rng.standard_normal((64, 64, 16))
    a[1, 2, 3] = np.nan
    back = np.zeros_like(a)
    wfpt._check(hip.wf_film_spectral_upload(s.ctx, a.ctypes.data), "wf_film_spectral_upload")
    wfpt._check(hip.wf_film_spectral_download(s.ctx, back.ctypes.data), "wf_film_spectral_download")
    assert a.tobytes() == back.tobytes()
    g = scene(wfpt, "gbuffer_film", False)
    rec = np.frombuffer(rng.bytes(64 * 64 * 136), GB_DTYPE).reshape(64, 64).copy()
    rec_back = np.zeros_like(rec)
    wfpt._check(hip.wf_film_gbuffer_upload(g.ctx, rec.ctypes.data), "wf_film_gbuffer_upload")
    wfpt._check(hip.wf_film_gbuffer_download(g.ctx, rec_back.ctypes.data), "wf_film_gbuffer_download")
    assert rec.tobytes() == rec_back.tobytes()
    # each upload on the wrong film type: the download's wording
    rgb = scene(wfpt, "cornell64", False)
    for ctx in (rgb.ctx, g.ctx):
        assert hip.wf_film_spectral_upload(ctx, a.ctypes.data) != 0
        assert b"wf_film_spectral_upload: the scene's film is not a spectral film" in hip.wf_last_error()
        assert hip.wf_film_spectral_download(ctx, back.ctypes.data) != 0
        assert b"wf_film_spectral_download: the scene's film is not a spectral film" in hip.wf_last_error()
    for ctx in (rgb.ctx, s.ctx):
        assert hip.wf_film_gbuffer_upload(ctx, rec.ctypes.data) != 0
        assert b"wf_film_gbuffer_upload: the scene's film is not a gbuffer film" in hip.wf_last_error()
        assert hip.wf_film_gbuffer_download(ctx, rec_back.ctypes.data) != 0
        assert b"wf_film_gbuffer_download: the scene's film is not a gbuffer film" in hip.wf_last_error()


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(wfpt):
    import torch
    _, hip = wfpt.libs()
    s = rendered(wfpt, "cornell64", True)
    want = s.image()
    good = torch.empty((64, 64, 3), dtype=torch.float32, device="cuda:0")
    n = C.c_int(0)
    wfpt._check(hip.wf_film_channel_count(s.ctx, C.byref(n)), "wf_film_channel_count")
    assert n.value == 3
    for f in (hip.wf_film_develop_device, hip.wf_film_develop_rgb_device):
        for floats in (64 * 64 * 3 - 1, 64 * 64 * 3 + 1, 0, 64 * 64 * 25):
            with pytest.raises(wfpt.WfError, match="dst_floats"):
                wfpt._check(f(s.ctx, good.data_ptr(), floats, 1, None), f.__name__)
        with pytest.raises(wfpt.WfError, match="null argument"):
            wfpt._check(f(s.ctx, None, 64 * 64 * 3, 1, None), f.__name__)
        with pytest.raises(wfpt.WfError):
            wfpt._check(f(None, good.data_ptr(), 64 * 64 * 3, 1, None), f.__name__)
        same_bits(host_of(s.image_tensor()), want)
    bad_outs = [torch.empty((64, 64, 3), dtype=torch.float64, device="cuda:0"),      # dtype
                torch.empty((64, 64, 4), dtype=torch.float32, device="cuda:0"),      # shape
                torch.empty((64 * 64 * 3,), dtype=torch.float32, device="cuda:0"),
                torch.empty((64, 64, 3), dtype=torch.float32),                       # device
                torch.empty((64, 64, 6), dtype=torch.float32, device="cuda:0")[:, :, ::2],   # not contiguous
                np.empty((64, 64, 3), np.float32)]                                   # not a tensor
    for out in bad_outs:
        with pytest.raises(wfpt.WfError, match="out is a contiguous float32 tensor"):
            s.image_tensor(out=out)
        with pytest.raises(wfpt.WfError, match="out is a contiguous float32 tensor"):
            s.film_channels_tensor(out=out)
        same_bits(host_of(s.image_tensor(out=good)), want)
    g = rendered(wfpt, "gbuffer_film", False)
    _, want_g = g.film_channels()
    with pytest.raises(wfpt.WfError, match="out is a contiguous float32 tensor"):
        g.film_channels_tensor(out=good)   # 25 channels, not 3
    with pytest.raises(wfpt.WfError, match="dst_floats"):
        wfpt._check(hip.wf_film_develop_device(g.ctx, good.data_ptr(), 64 * 64 * 3, 0, None), "wf_film_develop_device")
    same_bits(host_of(g.film_channels_tensor()[1]), want_g)
    same_bits(host_of(g.image_tensor(out=good)), g.image())
    # before create_renderer()
    fresh = wfpt.Scene(path=os.path.join(GOLDEN, "cornell64.pbrt"), spp=4)
    with pytest.raises(wfpt.WfError, match=r"create_renderer\(\) first"):
        fresh.image_tensor()
    with pytest.raises(wfpt.WfError, match=r"create_renderer\(\) first"):
        fresh.film_channels_tensor()
    fresh.close()
    same_bits(host_of(s.image_tensor()), want)
