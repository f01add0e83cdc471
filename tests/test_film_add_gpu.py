"""wf_film_add_samples_device and wf_camera_samples_device on the MI355X: Film::AddSample as a device-buffer call, and the camera rays
with the three weights it needs.

The pin is a REPLAY: a render of one sample index per pass leaves every pixel sample's radiance, wavelengths, PDF, pixel and weights in
the pixel sample state; fed through Scene.film_add_device on a second context of the same scene, sample index by sample index, they must
give the film the render gave — every accumulator bit for bit, on RGB, sensor / white-balance, clamped, spectral, GBuffer, realistic-camera
and crop-window scenes.  Beside it: the camera samples against camera_rays_device and the pixel sample state, the weight channel against
a closed form in numpy fp64 (no code shared with the render), the one-sample-per-pixel contract (duplicates rejected and counted, the
next call adds again), the shapes around the wave and the block with items outside a crop window, the device-side count, the argument
checks, and a call after a render."""
import ctypes as C
import os

import numpy as np
import pytest

from boundary_helpers import _np, open_scene, renderer_before_torch  # noqa: F401 (the fixture)
from conftest import GOLDEN, read_pfm

pytestmark = pytest.mark.gpu

# scene -> (spp the scene is loaded with, whether the existing parity tests hold the render's image to the committed *_ref.pfm bit for bit)
REPLAY = {"cornell64": (4, True), "film_sensor_wb": (4, True), "parser_torture": (4, False), "spectral_film": (4, False), "gbuffer_film": (4, False),
          "realistic_camera": (4, True), "fuzz/s6300016": (0, True)}
# scenes with a `glass-*` dielectric, for the zero-PDF precondition if parser_torture's glass gives none
DISPERSIVE_SPARES = ["fuzz/s6100015", "fuzz/s400039", "fuzz/s6100011"]
MEMBERS = (("L", np.float32, 4), ("lambda", np.float32, 4), ("lambda_pdf", np.float32, 4), ("pPixel", np.int32, 2), ("filterWeight", np.float32, 0),
           ("cameraRayWeight", np.float32, 4))


def pixel_state(wfpt, s):
    """the pixel sample state of the last pass: {member: array [W * H, ...]} (wf_queue_download)"""
    _, hip = wfpt.libs()
    hip.wf_queue_download.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_uint64]
    n = s.width * s.height
    out = {}
    for member, dtype, cols in MEMBERS:
        a = np.empty((n, cols) if cols else (n,), dtype)
        wfpt._check(hip.wf_queue_download(s.ctx, b"pixel", member.encode(), a.ctypes.data, a.nbytes), "wf_queue_download")
        out[member] = a
    return out


def spectral_sums(wfpt, s):
    _, hip = wfpt.libs()
    nc = C.c_int32(0)
    hip.wf_film_channel_count.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    wfpt._check(hip.wf_film_channel_count(s.ctx, C.byref(nc)), "wf_film_channel_count")
    a = np.empty((s.height, s.width, 2 * (nc.value - 3)), np.float64)
    hip.wf_film_spectral_download.argtypes = [C.c_void_p, C.c_void_p]
    wfpt._check(hip.wf_film_spectral_download(s.ctx, a.ctypes.data), "wf_film_spectral_download")
    return a


def add_state(s, st, dev, rejected=None, n_device=None, rows=None):
    """one film_add_device call from a downloaded pixel sample state (Lw = L * cameraRayWeight in torch fp32, on the device)"""
    import torch
    sel = (lambda a: a) if rows is None else (lambda a: a[rows])
    t = {k: torch.from_numpy(np.ascontiguousarray(sel(v))).to(dev) for k, v in st.items()}
    Lw = t["L"] * t["cameraRayWeight"]
    s.film_add_device(t["pPixel"], Lw, t["lambda"], t["lambda_pdf"], t["filterWeight"], n_device=n_device, rejected=rejected)


_replays = {}


def replay(wfpt, name, spp):
    """render `name` one sample index at a time on one context, feed every pass's pixel samples to film_add_device on a second one;
    computed once per scene"""
    import torch
    if name in _replays:
        return _replays[name]
    dev = torch.device("cuda", 0)
    a, b = open_scene(wfpt, name, spp), open_scene(wfpt, name, spp)
    a.clear_film(); b.clear_film()
    rejected = torch.zeros(1, dtype=torch.int32, device=dev)
    r = {"pdf_zero_beside_nonzero": 0, "camera_weight_not_one": 0, "n": a.width * a.height, "spp": a.spp}
    states = []
    for k in range(a.spp):
        a.render(k, k + 1)
        st = pixel_state(wfpt, a)
        add_state(b, st, dev, rejected=rejected)
        pdf = st["lambda_pdf"]
        r["pdf_zero_beside_nonzero"] += int((((pdf == 0).any(axis=1)) & ((pdf != 0).any(axis=1))).sum())
        r["camera_weight_not_one"] += int((st["cameraRayWeight"] != 1).any(axis=1).sum())
        states.append(st)
    torch.cuda.synchronize()
    r.update(film_render=a.film(), film_added=b.film(), image_added=b.image(), rejected=int(rejected.item()), states=states,
             image_tensor_added=_np(b.image_tensor()))
    if "spectral" in name:
        r.update(spectral_render=spectral_sums(wfpt, a), spectral_added=spectral_sums(wfpt, b))
    a.close(); b.close()
    _replays[name] = r
    return r


# ---- 1: the replay ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(REPLAY))
def test_replayed_samples_give_the_renders_film(wfpt, name):
    spp, pinned = REPLAY[name]
    r = replay(wfpt, name, spp)
    assert r["film_render"][..., 3].any(), "the render added nothing"
    assert r["film_added"].tobytes() == r["film_render"].tobytes(), int((r["film_added"].view(np.uint64) != r["film_render"].view(np.uint64)).sum())
    assert r["rejected"] == 0
    if "spectral" in name:
        assert r["spectral_render"].any() and r["spectral_added"].tobytes() == r["spectral_render"].tobytes()
    if pinned:
        ref = read_pfm(os.path.join(GOLDEN, name + "_ref.pfm"))
        assert ref.shape == r["image_added"].shape
        assert (r["image_added"].view(np.uint32) == ref.view(np.uint32)).all()
        assert (r["image_tensor_added"].view(np.uint32) == ref.view(np.uint32)).all()   # ... and developed on the device


def test_replay_scenes_cover_their_cases(wfpt):
    """a zero PDF beside non-zero ones (a dispersive refraction), a sensor maximum above max_component_value, camera weights != 1"""
    zero = replay(wfpt, "parser_torture", 4)["pdf_zero_beside_nonzero"]
    for name in DISPERSIVE_SPARES:
        if zero:
            break
        r = replay(wfpt, name, 0)
        assert r["film_added"].tobytes() == r["film_render"].tobytes() and r["rejected"] == 0, name
        zero = r["pdf_zero_beside_nonzero"]
    assert zero > 0
    assert replay(wfpt, "realistic_camera", 4)["camera_weight_not_one"] > 0
    # the clamp: with max_component_value lifted the same samples give another film, so some sample's sensor maximum exceeds it
    import torch
    dev = torch.device("cuda", 0)
    r = replay(wfpt, "parser_torture", 4)
    text = open(os.path.join(GOLDEN, "parser_torture.pbrt")).read()
    assert '"float maxcomponentvalue" 3.5' in text
    cwd = os.getcwd()
    os.chdir(GOLDEN)   # (the scene includes a file beside it)
    try:
        s = open_scene(wfpt, None, 4, text=text.replace('"float maxcomponentvalue" 3.5', '"float maxcomponentvalue" 1e30'))
    finally:
        os.chdir(cwd)
    s.clear_film()
    for st in r["states"]:
        add_state(s, st, dev)
    unclamped = s.film()
    s.close()
    assert (unclamped[..., 3] == r["film_render"][..., 3]).all() and (unclamped[..., :3] != r["film_render"][..., :3]).any()


# ---- 2: the camera samples ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tris", "realistic", "animated"])
def test_camera_samples_equal_camera_rays_and_the_pixel_state(wfpt, name):
    import torch
    path = os.path.join(GOLDEN, "intr_%s.pbrt" % name)
    s = wfpt.Scene(path=path, spp=4)
    s.create_renderer(0)
    n_pix = s.width * s.height
    assert s.query("pixels_per_pass") >= n_pix
    s.clear_film()
    s.render(0, 2)
    film_before = s.film()
    rays, pix, lam = (_np(t).copy() for t in s.camera_rays_device(0))
    got = [_np(t).copy() for t in s.camera_samples_device(0)]
    torch.cuda.synchronize()
    assert len(got) == 6 and got[0].shape == rays.shape
    # a realistic camera's rays enter the queue in no fixed order: both calls' items by pixel (every pixel has at most one ray)
    key = lambda p: p[:, 1].astype(np.int64) * 65536 + p[:, 0]
    assert len(np.unique(key(pix))) == len(pix)
    o1, o2 = np.argsort(key(pix)), np.argsort(key(got[1]))
    if name != "realistic":
        assert (o1 == np.arange(len(pix))).all() and (o2 == o1).all()   # pixel order
    rays, pix, lam = rays[o1], pix[o1], lam[o1]
    got = [g[o2] for g in got]
    for a, b in zip(got[:3], (rays, pix, lam)):
        assert a.tobytes() == b.tobytes()
    if name == "realistic":
        assert len(rays) < n_pix
    else:
        assert len(rays) == n_pix
    st = pixel_state(wfpt, s)
    # the pixel sample state is indexed by the band's pixel: row by row from the film's first scanline
    index = {(int(x), int(y)): i for i, (x, y) in enumerate(st["pPixel"][:n_pix])}
    rows = np.array([index[(int(x), int(y))] for x, y in pix])
    assert len(set(rows.tolist())) == len(rows)
    assert got[3].tobytes() == st["lambda_pdf"][rows].tobytes()
    assert got[4].tobytes() == st["cameraRayWeight"][rows].tobytes()
    assert got[5].tobytes() == st["filterWeight"][rows].tobytes()
    assert (got[3] > 0).all() and np.isfinite(got[5]).all()
    # the host-side pass settings are as they were: the same render gives the same film with and without the calls in between
    s.clear_film()
    s.render(0, 2)
    assert s.film().tobytes() == film_before.tobytes()
    s.close()


# ---- 3: the weight channel in closed form ----------------------------------------------------------------------------------------------
def test_weight_sums_equal_numpy_fp64(wfpt):
    import torch
    dev = torch.device("cuda", 0)
    s = open_scene(wfpt, "cornell64", 4)
    s.clear_film()
    n = s.width * s.height
    g = torch.Generator().manual_seed(20)
    w = (torch.rand((3, n), generator=g, dtype=torch.float32) * 2 - 0.5)   # negatives included
    assert (w < 0).any()
    ys, xs = np.divmod(np.arange(n, dtype=np.int32), s.width)
    pix = torch.from_numpy(np.stack([xs, ys + s.info.y0], axis=1).astype(np.int32)).to(dev)
    lam = torch.tensor([[450., 520., 590., 660.]], dtype=torch.float32).repeat(n, 1).to(dev)
    pdf = torch.full((n, 4), 1 / 470., dtype=torch.float32, device=dev)
    L = torch.rand((n, 4), generator=g, dtype=torch.float32).to(dev)
    rejected = torch.zeros(1, dtype=torch.int32, device=dev)
    for k in range(3):
        s.film_add_device(pix, L, lam, pdf, w[k].contiguous().to(dev), rejected=rejected)
    film = s.film()
    want = np.zeros(n, np.float64)
    for k in range(3):
        want = want + w[k].numpy().astype(np.float64)
    assert film[..., 3].reshape(-1).tobytes() == want.tobytes()
    assert int(rejected.item()) == 0 and np.isfinite(film).all() and (film[..., :3] != 0).any()
    s.close()


# ---- 4: duplicates ---------------------------------------------------------------------------------------------------------------------
def test_duplicates_are_rejected_and_counted(wfpt):
    import torch
    dev = torch.device("cuda", 0)
    r = replay(wfpt, "cornell64", 4)
    st = r["states"][0]
    n = r["n"]
    dup = np.array([0, 63, 64, 65, 1000, 2047, n - 1])
    rows = np.concatenate([np.arange(n), dup])
    rng = np.random.default_rng(3)
    rng.shuffle(rows)   # the second items anywhere in the call, identical values: whichever is kept, the film is the same
    a, b = open_scene(wfpt, "cornell64", 4), open_scene(wfpt, "cornell64", 4)
    a.clear_film(); b.clear_film()
    ra, rb = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
    add_state(a, st, dev, rejected=ra)
    add_state(b, st, dev, rejected=rb, rows=rows)
    assert int(ra.item()) == 0 and int(rb.item()) == 7
    assert a.film().tobytes() == b.film().tobytes()
    # the next call names the same pixels again: the epoch advanced, nothing is rejected, the counter is added to
    add_state(a, r["states"][1], dev, rejected=ra)
    add_state(b, r["states"][1], dev, rejected=rb)
    assert int(ra.item()) == 0 and int(rb.item()) == 7
    fa = a.film()
    assert fa.tobytes() == b.film().tobytes()
    # ... which is the render's film after two sample indices
    c = open_scene(wfpt, "cornell64", 4)
    c.clear_film()
    c.render(0, 2)
    assert c.film().tobytes() == fa.tobytes()
    for s in (a, b, c):
        s.close()


# ---- 5: shapes and arguments -----------------------------------------------------------------------------------------------------------
CROP = (7, 40, 5, 24)   # x0 x1 y0 y1: 33 x 19 pixels


@pytest.fixture(scope="module")
def crop(wfpt):
    text = open(os.path.join(GOLDEN, "cornell64.pbrt")).read()
    film = '"integer xresolution" [ 64 ] "integer yresolution" [ 64 ]'
    assert film in text
    s = open_scene(wfpt, None, 4, text=text.replace(film, film + ' "integer pixelbounds" [ %d %d %d %d ]' % CROP))
    assert (s.width, s.height, s.info.y0) == (33, 19, 5)
    yield s
    s.close()


def crop_items(n, seed):
    """n items, one pixel each: the window's pixels in a shuffled order, every fifth item moved outside the window"""
    import torch
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1 = CROP
    cells = rng.permutation(33 * 19)[:n]
    pix = np.stack([x0 + cells % 33, y0 + cells // 33], axis=1).astype(np.int32)
    outside = np.array([(x0 - 1, y0), (x1, y0 + 3), (x0 + 2, y0 - 1), (x0 + 5, y1), (-3, -3), (64, 64), (x1, y1)], np.int32)
    inside = np.ones(n, bool)
    for k in range(0, n, 5):
        pix[k] = outside[(k // 5) % len(outside)]
        inside[k] = False
    L = (rng.random((n, 4)) * 3).astype(np.float32)
    lam = (400 + rng.random((n, 4)) * 300).astype(np.float32)
    pdf = np.full((n, 4), 1 / 470., np.float32)
    w = (rng.random(n) * 1.5 - 0.25).astype(np.float32)
    return pix, L, lam, pdf, w, inside


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_around_the_wave_and_the_block_with_items_outside_the_window(wfpt, crop, n):
    import torch
    dev = torch.device("cuda", 0)
    pix, L, lam, pdf, w, inside = crop_items(n, n)
    t = [torch.from_numpy(a).to(dev) for a in (pix, L, lam, pdf, w)]
    rejected = torch.zeros(1, dtype=torch.int32, device=dev)
    crop.clear_film()
    crop.film_add_device(*t, rejected=rejected)
    film = crop.film()
    assert int(rejected.item()) == 0
    want = np.zeros((19, 33), np.float64)
    want[pix[inside, 1] - CROP[2], pix[inside, 0] - CROP[0]] = w[inside].astype(np.float64)
    assert film[..., 3].tobytes() == want.tobytes()           # the items outside changed nothing; every item inside landed on its pixel
    touched = np.zeros((19, 33), bool)
    touched[pix[inside, 1] - CROP[2], pix[inside, 0] - CROP[0]] = True
    assert (film[~touched] == 0).all()
    if inside.any():
        assert (film[touched][:, :3] != 0).any()
    # the same items without the ones outside give the same film
    crop.clear_film()
    crop.film_add_device(*[x[torch.from_numpy(inside).to(dev)].contiguous() for x in t])
    assert crop.film().tobytes() == film.tobytes()


def test_the_device_count_caps_the_items(wfpt, crop):
    import torch
    dev = torch.device("cuda", 0)
    pix, L, lam, pdf, w, inside = crop_items(257, 9)
    t = [torch.from_numpy(a).to(dev) for a in (pix, L, lam, pdf, w)]
    crop.clear_film()
    crop.film_add_device(*[x[:100].contiguous() for x in t])
    first100 = crop.film()
    for count, want in ((100, first100), (0, np.zeros_like(first100)), (-5, np.zeros_like(first100))):
        crop.clear_film()
        crop.film_add_device(*t, n_device=torch.tensor([count], dtype=torch.int32, device=dev))
        assert crop.film().tobytes() == want.tobytes(), count
    crop.clear_film()
    crop.film_add_device(*t, n_device=torch.tensor([100000], dtype=torch.int32, device=dev))   # more than n: n items
    full = crop.film()
    crop.clear_film()
    crop.film_add_device(*t)
    assert crop.film().tobytes() == full.tobytes() and full.tobytes() != first100.tobytes()
    # n = 0 touches nothing (and checks nothing but the context)
    _, hip = wfpt.libs()
    hip.wf_film_add_samples_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    assert hip.wf_film_add_samples_device(crop.ctx, 0, None, None, None, None, None, None, None) == 0
    crop.film_add_device(*[x[:0].contiguous() for x in t])
    assert crop.film().tobytes() == full.tobytes()


def test_arguments_are_refused_before_any_launch(wfpt, crop):
    import torch
    dev = torch.device("cuda", 0)
    pix, L, lam, pdf, w, _ = crop_items(64, 4)
    room = [torch.zeros(a.size + 8, dtype=torch.from_numpy(a).dtype, device=dev) for a in (pix, L, lam, pdf, w)]   # (room for a misaligned copy)
    t = []
    for r, a in zip(room, (pix, L, lam, pdf, w)):
        r[:a.size] = torch.from_numpy(a).reshape(-1).to(dev)
        t.append(r)
    count, rej = torch.tensor([64], dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    _, hip = wfpt.libs()
    f = hip.wf_film_add_samples_device
    f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    crop.clear_film()
    good = [count.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), rej.data_ptr()]
    names = ["n_device", "pixel_xy", "L4", "lambda4", "lambda_pdf4", "filter_weight", "rejected_device"]
    for k, name in enumerate(names):
        if name not in ("n_device", "rejected_device"):
            bad = list(good); bad[k] = None
            assert f(crop.ctx, 64, *bad) != 0
            assert b"wf_film_add_samples_device" in hip.wf_last_error() and name.encode() in hip.wf_last_error(), hip.wf_last_error()
        for off in ((4, 8) if name in ("L4", "lambda4", "lambda_pdf4") else (4,) if name == "pixel_xy" else (1, 2)):
            bad = list(good); bad[k] = good[k] + off
            assert f(crop.ctx, 64, *bad) != 0, (name, off)
            assert b"wf_film_add_samples_device" in hip.wf_last_error() and name.encode() in hip.wf_last_error(), hip.wf_last_error()
    assert f(None, 0, *good) != 0 and b"wf_film_add_samples_device: null context" in hip.wf_last_error()
    g = hip.wf_camera_samples_device
    g.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7
    cap = crop.query("pixels_per_pass")
    big = torch.zeros(cap * 8 + 8, dtype=torch.float32, device=dev)
    ok = [big.data_ptr()] * 6 + [count.data_ptr()]
    for k in range(7):
        bad = list(ok); bad[k] = None
        assert g(crop.ctx, crop.info.y0, 0, cap, *bad) != 0 and b"wf_camera_samples_device: null" in hip.wf_last_error(), k
    for k, off in ((3, 8), (4, 4), (5, 2), (0, 4)):
        bad = list(ok); bad[k] = ok[k] + off
        assert g(crop.ctx, crop.info.y0, 0, cap, *bad) != 0 and b"wf_camera_samples_device: misaligned" in hip.wf_last_error(), k
    assert g(crop.ctx, crop.info.y0, 0, cap - 1, *ok) != 0 and b"wf_camera_samples_device: n_max" in hip.wf_last_error()
    torch.cuda.synchronize()
    assert not crop.film().any() and int(rej.item()) == 0


# ---- 6: after a render -----------------------------------------------------------------------------------------------------------------
def test_samples_added_after_a_render(wfpt):
    import torch
    dev = torch.device("cuda", 0)
    r = replay(wfpt, "cornell64", 4)
    st = r["states"][2]
    a, b = open_scene(wfpt, "cornell64", 4), open_scene(wfpt, "cornell64", 4)
    a.clear_film(); b.clear_film()
    a.render(0, 2)
    rendered = a.film()
    add_state(a, st, dev)
    after = a.film()
    # the weight channel: the render's sum plus the sample's filter weight, in numpy fp64
    want = rendered[..., 3].reshape(-1).copy()
    px = st["pPixel"]
    want[(px[:, 1] - a.info.y0) * a.width + px[:, 0]] += st["filterWeight"].astype(np.float64)
    assert after[..., 3].reshape(-1).tobytes() == want.tobytes()
    # the colour channels: a context that adds the same things in the same order
    for k in (0, 1, 2):
        add_state(b, r["states"][k], dev)
    assert b.film().tobytes() == after.tobytes()
    # ... and the render's own third sample index gives the same film
    a.clear_film()
    a.render(0, 3)
    assert a.film().tobytes() == after.tobytes()
    a.close(); b.close()
