"""The transmittance wavefront on scenes with animated primitives (k_tr_trace<8 | 9, true>, k_tr_segment<*, true>, k_tr_rest<true>) and
wf_trace_shadow_tr_device on the scene's planned route (ScenePlan::trRoute), on the MI355X.  Every image is compared bit for bit with
the CPU checker and the reference's render, every device call bit for bit with the host-array call of the same items, which runs one
reference-order (or per-lane production) walk per lane whatever the plan says: the independent witness."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from boundary_helpers import _dev, _launch_names, _rays8, _shadow_rays, _tr_device
from suite_helpers import _check_image_vs_oracle_and_reference

pytestmark = pytest.mark.gpu

SCENES = ["animated_interface", "animated_tr_routes"]   # GEN 0 + lean media; GEN 1 + an RGB grid (tests/test_transmittance_route_host.py)
WAVEFRONT = ["Intersect shadow (Tr): begin", "Intersect shadow (Tr): trace", "Intersect shadow (Tr): segment", "Intersect shadow (Tr): rest"]
DEVICE_WAVEFRONT = ["shadow Tr (device rays): begin", "shadow Tr (device rays): trace", "shadow Tr (device rays): segment", "shadow Tr (device rays): rest"]
CAMERA = np.array([0, -7, 3], dtype=np.float32)   # of both scenes: rendering space is world space minus the camera position
# animated_tr_routes: the louvres instance sits at LOUVRES_T0 + time * LOUVRES_DT (a translation is interpolated linearly); in the
# definition slab k spans x = 0.3 k .. 0.3 k + 0.1, y = -0.5 .. 0.5, z = 0 .. 1; media in the order of the file: mist 0 (the slabs'), ember 1
LOUVRES_T0 = np.array([0.8, -1.4, 0.05], dtype=np.float32)
LOUVRES_DT = np.array([0.5, 0.4, 0.3], dtype=np.float32)
MIST = 0


def _open(wfpt, name, samples_per_pass=0):
    s = wfpt.Scene(path=os.path.join(GOLDEN, name + ".pbrt"), spp=4)
    s.create_renderer(0, samples_per_pass=samples_per_pass)
    return s


def _set_switch(monkeypatch, switch):
    if switch is None:
        monkeypatch.delenv("WF_TR_WAVEFRONT", raising=False)
    else:
        monkeypatch.setenv("WF_TR_WAVEFRONT", switch)


# ---- 1. the render ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch,route", [("1", 2), (None, 2), ("0", 0)])
@pytest.mark.parametrize("name", SCENES)
def test_render_is_the_reference_on_every_route(wfpt, tmp_path, monkeypatch, name, switch, route):
    """bit identity with wf_cpu and the golden, equal ray counts, no stack overflow — under the wavefront (forced and by default) and
    under the reference-order walk per lane; one profiled render shows which of the two ran"""
    _set_switch(monkeypatch, switch)
    _check_image_vs_oracle_and_reference(wfpt, tmp_path, name)
    s = _open(wfpt, name)
    assert s.query("tr_route") == s.plan("tr_route") == route
    s.enable_profile(2)
    s.render()
    names = _launch_names(s)
    s.close()
    if route == 2:
        assert all(n in names for n in WAVEFRONT) and "Intersect shadow (Tr)" not in names, names
    else:
        assert "Intersect shadow (Tr)" in names and not any(n in names for n in WAVEFRONT), names


# ---- 2. the device call on animated scenes ------------------------------------------------------------------------------------------
def _raw_device_call(wfpt, ctx, n, tensors):
    """wf_trace_shadow_tr_device through ctypes: (rays8, medium, lambda, Ld, r_u, r_l, out_L) device tensors, n items of them"""
    import torch
    _, hip = wfpt.libs()
    f = hip.wf_trace_shadow_tr_device
    f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    torch.cuda.synchronize()
    rc = f(ctx, n, *[t.data_ptr() for t in tensors])
    assert hip.wf_sync(ctx) == 0
    return rc


@pytest.mark.parametrize("name", SCENES)
def test_device_call_runs_the_wavefront_at_the_items_times(wfpt, monkeypatch, name):
    import torch
    _set_switch(monkeypatch, "1")
    s = _open(wfpt, name)
    assert s.query("tr_route") == 2 and s.query("anim_fast") == 1
    n = 20000
    lo, hi = s.bounds()
    rays = _shadow_rays(lo, hi, n, 4, 2)
    times = {"0": np.zeros(n, dtype=np.float32), "1": np.ones(n, dtype=np.float32), "random": np.random.default_rng(7).uniform(0, 1, size=n).astype(np.float32)}
    ref = {k: s.trace_shadow_tr(*rays, time=t) for k, t in times.items()}
    s.enable_profile(1)
    got = {k: _tr_device(s, rays, t) for k, t in times.items()}
    names = _launch_names(s)
    s.enable_profile(0)
    # sizes: one item, less than a wave, none (a sentinel-filled out_L stays as it is)
    t = times["random"]
    one = _tr_device(s, tuple(a[:1] for a in rays), t[:1])
    part = _tr_device(s, tuple(a[:63] for a in rays), t[:63])
    o, d, tmax, medium, lam, Ld, r_u, r_l = rays
    sentinel = torch.full((4, 4), 123.5, dtype=torch.float32, device="cuda:0")
    args = [_dev(_rays8(o, d, tmax, t)[:4]), _dev(medium[:4]), _dev(lam[:4]), _dev(Ld[:4]), _dev(r_u[:4]), _dev(r_l[:4]), sentinel]
    assert _raw_device_call(wfpt, s.ctx, 0, args) == 0
    assert (sentinel.cpu().numpy() == 123.5).all()
    s.close()
    assert all(x in names for x in DEVICE_WAVEFRONT), names
    assert "shadow Tr (device rays, timed)" not in names and "shadow Tr (device rays)" not in names, names
    for k in times:
        assert np.isfinite(got[k]).all(), k
        assert (got[k].view(np.uint32) == ref[k].view(np.uint32)).all(), (k, (got[k] != ref[k]).any(axis=1).mean())
    assert one.tobytes() == ref["random"][:1].tobytes() and part.tobytes() == ref["random"][:63].tobytes()
    # the moving boundaries are elsewhere at time 1; some rays arrive, some are blocked
    differ = (got["0"] != got["1"]).any(axis=1).mean()
    print(name, "lit %.3f, black %.3f, time 0 and time 1 differ on %.3f of the items" % ((got["0"] > 0).any(axis=1).mean(), (got["0"] == 0).all(axis=1).mean(), differ))
    assert differ > 0.01
    assert (got["0"] > 0).any() and (got["0"] == 0).all(axis=1).any()


def test_device_call_follows_the_switch_back_to_the_reference_order_walk(wfpt, monkeypatch):
    _set_switch(monkeypatch, "0")
    s = _open(wfpt, "animated_tr_routes")
    assert s.query("tr_route") == 0
    n = 4000
    lo, hi = s.bounds()
    rays = _shadow_rays(lo, hi, n, 4, 2)
    t = np.random.default_rng(7).uniform(0, 1, size=n).astype(np.float32)
    ref = s.trace_shadow_tr(*rays, time=t)
    s.enable_profile(1)
    got = _tr_device(s, rays, t)
    names = _launch_names(s)
    s.close()
    assert "shadow Tr (device rays, timed)" in names and not any(x in names for x in DEVICE_WAVEFRONT), names
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()


# ---- 3. k_tr_rest<true> -------------------------------------------------------------------------------------------------------------
def _louvre_items(n, seed):
    """n shadow items along the louvres' axis at their own times.  The first half crosses all five slabs at the instance's position at
    the item's time — even items from the vacuum in front of slab 0 (ten interface surfaces), odd items from inside slab 0's mist (nine)
    — the second half, the control group, ends in the vacuum in front of slab 0"""
    rng = np.random.RandomState(seed)
    time = rng.uniform(0, 1, size=n).astype(np.float32)
    yz = rng.uniform([-0.4, 0.1], [0.4, 0.9], size=(n, 2)).astype(np.float32)
    at = LOUVRES_T0[None, :] + time[:, None] * LOUVRES_DT[None, :] - CAMERA[None, :]
    crossing = np.arange(n) < n // 2
    inside = crossing & (np.arange(n) % 2 == 1)
    x0 = np.where(crossing, np.where(inside, 0.05, -0.2), -0.9).astype(np.float32)
    x1 = np.where(crossing, 1.5, -0.1).astype(np.float32)
    o = (at + np.stack([x0, yz[:, 0], yz[:, 1]], axis=1)).astype(np.float32)
    d = np.stack([x1 - x0, np.zeros(n, np.float32), np.zeros(n, np.float32)], axis=1).astype(np.float32)
    medium = np.where(inside, MIST, -1).astype(np.int32)
    lam = np.sort(rng.uniform(380, 780, size=(n, 4)), axis=1).astype(np.float32)
    Ld = rng.uniform(0.1, 2, size=(n, 4)).astype(np.float32)
    ones = np.ones((n, 4), dtype=np.float32)
    return (o, d, np.full(n, 0.9999, dtype=np.float32), medium, lam, Ld, ones, ones.copy()), time, crossing, inside


def test_rays_that_outlive_the_wavefront_rounds_are_finished_by_the_rest_kernel(wfpt, monkeypatch):
    """A shadow ray along x through the five louvres meets ten (from inside slab 0: nine) interface surfaces and nothing else: it is
    alive after the wavefront's WF_TR_SEGMENTS = 4 rounds and k_tr_rest<true> walks the rest, at the item's time.  Such a ray arrives
    unless the ratio tracking through 0.5 (0.45) units of mist ends it — exp(-sigma_t x 0.5) with sigma_t = 0.7 .. 1.0 over the
    wavelengths.  Measured with the host-array call on these items (MI355X): 0.6685 of the crossing items arrive (0.6640 of those
    from the vacuum, 0.6730 of those from inside slab 0), and every control item, which ends in front of the first slab, arrives
    with T = 1: Ld / (r_u + r_l).Average() = Ld / 2."""
    ARRIVE = 0.6685
    _set_switch(monkeypatch, "1")
    s = _open(wfpt, "animated_tr_routes")
    assert s.query("tr_route") == 2
    n = 4000
    rays, time, crossing, inside = _louvre_items(n, 21)
    ref = s.trace_shadow_tr(*rays, time=time)
    s.enable_profile(1)
    got = _tr_device(s, rays, time)
    names = _launch_names(s)
    s.close()
    arrived = (ref > 0).any(axis=1)
    print("louvres: arriving fraction of the crossing items %.4f (from the vacuum %.4f, from inside slab 0 %.4f), of the control items %.4f" %
          (arrived[crossing].mean(), arrived[crossing & ~inside].mean(), arrived[inside].mean(), arrived[~crossing].mean()))
    assert "shadow Tr (device rays): rest" in names, names
    assert (got.view(np.uint32) == ref.view(np.uint32)).all(), (got != ref).any(axis=1).mean()
    assert (got[crossing] > 0).any(axis=1).mean() > ARRIVE / 2
    assert (got[crossing & ~inside] > 0).any() and (got[inside] > 0).any()
    # the control group is untouched (T = 1), the crossing group is attenuated and partly ended
    Ld = rays[5]
    assert np.allclose(got[~crossing], 0.5 * Ld[~crossing], rtol=1e-6, atol=0)
    assert got[crossing].mean() < 0.9 * got[~crossing].mean()


# ---- 4. the device call on static scenes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["media_instances", "media_box"])
def test_device_call_on_a_static_scene_runs_the_wavefront_too(wfpt, monkeypatch, name):
    _set_switch(monkeypatch, None)
    s = _open(wfpt, name)
    assert s.query("tr_route") == 2 and s.query("anim_fast") == 0
    lo, hi = s.bounds()
    n = 20000
    rays = _shadow_rays(lo, hi, n, 3, 2)
    time = np.random.default_rng(3).uniform(0, 1, size=n).astype(np.float32)   # ignored: the scene is static
    ref = s.trace_shadow_tr(*rays)
    s.enable_profile(1)
    got = _tr_device(s, rays, time)
    names = _launch_names(s)
    s.close()
    assert all(x in names for x in DEVICE_WAVEFRONT) and "shadow Tr (device rays)" not in names, names
    assert (got > 0).any(axis=1).any() and (got == 0).all(axis=1).any()
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()


# ---- 5. the scratch -----------------------------------------------------------------------------------------------------------------
def test_scratch_is_the_calls_own_and_grows_past_the_render_queues(wfpt, monkeypatch):
    """a renderer made with samples_per_pass = 1 has queues of 96 x 64 items at the most: a call of 20 000 items cannot be using them"""
    _set_switch(monkeypatch, "1")
    s = _open(wfpt, "animated_tr_routes", samples_per_pass=1)
    assert s.query("tr_route") == 2 and s.samples_per_pass == 1 and s.width * s.height < 20000
    n = 20000
    lo, hi = s.bounds()
    rays = _shadow_rays(lo, hi, n, 4, 2)
    time = np.random.default_rng(7).uniform(0, 1, size=n).astype(np.float32)
    small = tuple(a[:64] for a in rays)
    first = _tr_device(s, small, time[:64])
    big = _tr_device(s, rays, time)
    third = _tr_device(s, small, time[:64])
    ref = s.trace_shadow_tr(*rays, time=time)
    s.close()
    assert first.tobytes() == third.tobytes() == ref[:64].tobytes()
    assert (big.view(np.uint32) == ref.view(np.uint32)).all()
    assert (big > 0).any()


def test_device_call_needs_no_render_queues(wfpt, monkeypatch):
    """wf_trace_shadow_tr_device on a context with an uploaded scene and NO wf_queues_alloc: the wavefront's state is the call's scratch"""
    import torch
    _set_switch(monkeypatch, "1")
    host, hip = wfpt.libs()
    scene = wfpt.Scene(path=os.path.join(GOLDEN, "animated_tr_routes.pbrt"), spp=4)
    witness = _open(wfpt, "animated_tr_routes")
    n = 2000
    lo, hi = witness.bounds()
    rays = _shadow_rays(lo, hi, n, 4, 2)
    time = np.random.default_rng(9).uniform(0, 1, size=n).astype(np.float32)
    ref = witness.trace_shadow_tr(*rays, time=time)
    witness.close()
    hip.wf_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    hip.wf_scene_upload.argtypes = [C.c_void_p, C.c_void_p]
    ctx = C.c_void_p()
    assert hip.wf_ctx_create(0, C.byref(ctx)) == 0 and ctx.value, hip.wf_last_error()
    try:
        assert hip.wf_scene_upload(ctx, host.wfh_scene_desc(scene.h)) == 0, hip.wf_last_error()
        o, d, tmax, medium, lam, Ld, r_u, r_l = rays
        out = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda:0")
        args = [_dev(_rays8(o, d, tmax, time)), _dev(medium), _dev(lam), _dev(Ld), _dev(r_u), _dev(r_l), out]
        assert _raw_device_call(wfpt, ctx, n, args) == 0, hip.wf_last_error()
        got = out.cpu().numpy()
    finally:
        hip.wf_ctx_destroy(ctx)
        scene.close()
    assert np.isfinite(got).all()
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()
