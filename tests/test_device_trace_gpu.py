"""The device-buffer boundary on the MI355X: wf_trace_closest_device_t / wf_trace_any_device_t (rays with times, any scene),
wf_trace_shadow_tr_device and wf_trace_one_random_device, through wfpt.Scene.trace_device / trace_shadow_tr_device /
trace_one_random_device on torch tensors.  Every result is compared bit for bit: with the CPU checker's walk at the rays' times, or with
the host-array call of the same method."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from boundary_helpers import _dev, _launch_names, _rays8, _shadow_rays, _tr_device
from conftest import GOLDEN, WF_CPU

pytestmark = pytest.mark.gpu

BITS = ("t", "b0", "b1", "b2")
# the rendering-space box of the animated_* scenes' ray tests: the world box (-7.2, -7.2, -0.5) .. (7.2, 7.2, 5.5) minus the camera position (0, -7, 3)
ANIM_LO = np.array([-7.2, -0.2, -3.5], dtype=np.float32)
ANIM_HI = np.array([7.2, 14.2, 2.5], dtype=np.float32)
N_ANIM = 20001


def _random_rays(n, bounds_lo, bounds_hi, seed):
    rng = np.random.RandomState(seed)
    o = rng.uniform(bounds_lo, bounds_hi, size=(n, 3)).astype(np.float32)
    t = rng.uniform(bounds_lo, bounds_hi, size=(n, 3)).astype(np.float32)
    d = (t - o).astype(np.float32)
    d[::3] /= np.linalg.norm(d[::3], axis=1, keepdims=True)
    tmax = np.full(n, np.inf, dtype=np.float32)
    tmax[::4] = rng.uniform(0.1, 2.0, size=tmax[::4].shape).astype(np.float32)
    return o, d.astype(np.float32), tmax


def _open(wfpt, name):
    s = wfpt.Scene(path=os.path.join(GOLDEN, name + ".pbrt"), spp=4)
    s.create_renderer(0)
    return s


def _closest(wfpt, s, rays8):
    return wfpt.hit_records(s.trace_device(_dev(rays8)))


def _any(s, rays8):
    return s.trace_device(_dev(rays8), any_hit=True).cpu().numpy()


def _same_hits(got, ref):
    for f in ("prim", "instance"):
        assert (got[f] == ref[f]).all(), f
    for f in BITS:
        assert (got[f].view(np.uint32) == ref[f].view(np.uint32)).all(), f
    # the records of the device calls with times carry no visit counts, on any walk
    assert (got["nodes_visited"] == 0).all() and (got["tris_tested"] == 0).all()


def _untimed_device(wfpt, s, rays7, any_hit):
    """wf_trace_closest_device / wf_trace_any_device (7 floats per ray, no times) on the same device rays"""
    import torch
    _, hip = wfpt.libs()
    r = _dev(rays7)
    n = r.shape[0]
    out = torch.empty((n,) if any_hit else (n, 8), dtype=torch.int32, device=r.device)
    torch.cuda.synchronize()
    f = hip.wf_trace_any_device if any_hit else hip.wf_trace_closest_device
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert f(s.ctx, n, r.data_ptr(), out.data_ptr()) == 0, hip.wf_last_error()
    assert hip.wf_sync(s.ctx) == 0
    return out.cpu().numpy() if any_hit else wfpt.hit_records(out)


@pytest.fixture(scope="module")
def anim_rays():
    o, d, tmax = _random_rays(N_ANIM, ANIM_LO, ANIM_HI, 11)
    time = np.random.default_rng(5).uniform(0, 1, size=N_ANIM).astype(np.float32)
    return o, d, tmax, time


@pytest.fixture(scope="module")
def cpu_hits(wfpt, anim_rays, tmp_path_factory):
    """the CPU checker's walk of the anim_rays at their times, and at time 0: computed once per scene, read by every test"""
    o, d, tmax, time = anim_rays
    td = tmp_path_factory.mktemp("device_trace")
    cache = {}

    def get(name, at_zero=False):
        key = (name, at_zero)
        if key not in cache:
            rays = _rays8(o, d, tmax, np.zeros_like(time) if at_zero else time)
            rays.tofile(td / "rays8.bin")
            subprocess.run([WF_CPU, "--quiet", "--trace-timed", str(td / "rays8.bin"), str(td / "hits.bin"), os.path.join(GOLDEN, name + ".pbrt")], check=True)
            ref = np.fromfile(td / "hits.bin", dtype=wfpt.HIT_DTYPE)
            ref.setflags(write=False)
            cache[key] = ref
        return cache[key]
    return get


def _assert_not_vacuous(name, cpu_hits):
    """the figures of these inputs on the CPU checker: animated_tris 0.227 / 0.040 / 0.041, animated_tris_alpha 0.236 / 0.034 / 0.037,
    animated 0.229 / 0.044 / 0.041 (hits, hits inside instances, rays whose (prim, t) differs from time 0; fractions of all rays)"""
    ref, ref0 = cpu_hits(name), cpu_hits(name, at_zero=True)
    hits, inst = (ref["prim"] >= 0).mean(), (ref["instance"] >= 0).mean()
    differs = ((ref["prim"] != ref0["prim"]) | (ref["t"].view(np.uint32) != ref0["t"].view(np.uint32))).mean()
    print(name, "hits %.3f, inside instances %.3f, differs from time 0 %.3f" % (hits, inst, differs))
    assert 0.1 < hits < 0.9 and inst > 0.02 and differs > 0.02


# ---- 1. static scenes: the time is ignored --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blobs_small", "instances"])
def test_static_scene_answers_like_the_untimed_device_calls(wfpt, name):
    s = _open(wfpt, name)
    n = 5000
    lo, hi = s.bounds()
    o, d, tmax = _random_rays(n, lo, hi, 3)
    time = np.random.default_rng(3).uniform(0, 1, size=n).astype(np.float32)
    rays8 = _rays8(o, d, tmax, time)
    got, occ = _closest(wfpt, s, rays8), _any(s, rays8)
    ref, occ_ref = _untimed_device(wfpt, s, rays8[:, :7], False), _untimed_device(wfpt, s, rays8[:, :7], True)
    s.close()
    assert 0.1 < (ref["prim"] >= 0).mean() < 1.0
    if name == "instances":
        assert (ref["instance"] >= 0).mean() > 0.02
    _same_hits(got, ref)
    assert (occ == occ_ref).all() and ((occ != 0) == (ref["prim"] >= 0)).all()


# ---- 2. the production ANIM walk against the CPU checker -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["animated_tris", "animated_tris_alpha"])
def test_anim_fast_scene_takes_the_production_walk_and_matches_the_cpu_checker(wfpt, anim_rays, cpu_hits, name):
    import torch
    _assert_not_vacuous(name, cpu_hits)
    ref = cpu_hits(name)
    s = _open(wfpt, name)
    assert s.query("anim_fast") == 1 and s.query("fast_ok") == 1
    rays8 = _rays8(*anim_rays)
    s.enable_profile(1)
    s.debug_counters(reset=True)
    got, occ = _closest(wfpt, s, rays8), _any(s, rays8)
    names = _launch_names(s)
    dbg = s.debug_counters(reset=True)
    s.enable_profile(0)
    # sizes: one ray, less than a wave, none
    dev = _dev(rays8)
    one, part = wfpt.hit_records(s.trace_device(dev[:1])), wfpt.hit_records(s.trace_device(dev[:63]))
    occ_part = s.trace_device(dev[:63], any_hit=True).cpu().numpy()
    sentinel = torch.full((4, 8), 0x5A5A5A5A, dtype=torch.int32, device=dev.device)
    sentinel_occ = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device=dev.device)
    s.trace_device(dev[:0], out=sentinel)
    s.trace_device(dev[:0], any_hit=True, out=sentinel_occ)
    untouched = bool((sentinel == 0x5A5A5A5A).all()) and bool((sentinel_occ == 0x5A5A5A5A).all())
    with pytest.raises(wfpt.WfError, match="animated"):   # the calls without times keep refusing the scene
        _untimed_device_checked(wfpt, s, rays8[:64, :7])
    s.close()
    _same_hits(got, ref)
    assert ((occ != 0) == (ref["prim"] >= 0)).all()
    assert "trace closest fast (device rays, timed)" in names and "trace any fast (device rays, timed)" in names, names
    assert not any(n_ in names for n_ in ("trace closest (device rays, timed)", "trace any (device rays, timed)")), names
    assert dbg["overflow"] == 0
    assert one.tobytes() == got[:1].tobytes() and part.tobytes() == got[:63].tobytes() and (occ_part == occ[:63]).all()
    assert untouched


def _untimed_device_checked(wfpt, s, rays7):
    _, hip = wfpt.libs()
    import torch
    r = _dev(rays7)
    out = torch.empty((r.shape[0], 8), dtype=torch.int32, device=r.device)
    torch.cuda.synchronize()
    hip.wf_trace_closest_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    if hip.wf_trace_closest_device(s.ctx, r.shape[0], r.data_ptr(), out.data_ptr()) != 0:
        raise wfpt.WfError(hip.wf_last_error().decode())


# ---- 3. the animated scenes the production walk does not take: the reference-order walk on the caller's buffers ---------------------------
def test_scene_with_moving_quadrics_takes_the_reference_order_walk(wfpt, anim_rays, cpu_hits):
    name = "animated"
    _assert_not_vacuous(name, cpu_hits)
    ref = cpu_hits(name)
    s = _open(wfpt, name)
    assert s.query("anim_fast") == 0
    rays8 = _rays8(*anim_rays)
    s.enable_profile(1)
    got, occ = _closest(wfpt, s, rays8), _any(s, rays8)
    names = _launch_names(s)
    s.close()
    _same_hits(got, ref)
    assert ((occ != 0) == (ref["prim"] >= 0)).all()
    assert "trace closest (device rays, timed)" in names and "trace any (device rays, timed)" in names, names
    assert not any("fast" in n_ for n_ in names), names


def test_nested_placements_answer_like_the_host_array_call(wfpt):
    s = _open(wfpt, "animated_in_definition")
    assert s.query("nested_animated") > 0 and s.query("anim_fast") == 0
    n = 20000
    lo, hi = s.bounds()
    pad = 0.1 * (hi - lo)
    o, d, tmax = _random_rays(n, lo - pad, hi + pad, 11)
    time = np.random.default_rng(5).uniform(0, 1, size=n).astype(np.float32)
    ref = s.trace_timed(o, d, tmax, time)
    occ_ref = s.trace_timed(o, d, tmax, time, any_hit=True)
    at0 = s.trace_timed(o, d, tmax, np.zeros(n, dtype=np.float32))
    rays8 = _rays8(o, d, tmax, time)
    got, occ = _closest(wfpt, s, rays8), _any(s, rays8)
    s.close()
    # (what tests/test_animated_in_definition_gpu.py asks of its rays: they hit, inside the definition too, and the time matters)
    assert 0.1 < (ref["prim"] >= 0).mean() < 1.0 and (ref["instance"] >= 0).any()
    assert ((at0["prim"] != ref["prim"]) | (at0["t"] != ref["t"])).mean() > 0.005
    _same_hits(got, ref)
    assert (occ == occ_ref).all()


def test_anim_fast_switched_off_gives_the_same_records(wfpt, anim_rays, cpu_hits, monkeypatch):
    monkeypatch.setenv("WF_ANIM_FAST", "0")
    s = _open(wfpt, "animated_tris")
    assert s.query("anim_fast") == 0
    rays8 = _rays8(*anim_rays)
    s.enable_profile(1)
    got, occ = _closest(wfpt, s, rays8), _any(s, rays8)
    names = _launch_names(s)
    s.close()
    ref = cpu_hits("animated_tris")
    _same_hits(got, ref)
    assert ((occ != 0) == (ref["prim"] >= 0)).all()
    assert "trace closest (device rays, timed)" in names and not any("fast" in n_ for n_ in names), names


# ---- 4. transmittance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["media_box", "media_instances"])
def test_transmittance_on_a_static_scene_is_the_untimed_host_array_call(wfpt, name):
    s = _open(wfpt, name)
    lo, hi = s.bounds()
    n = 20000
    rays = _shadow_rays(lo, hi, n, 3, 2)
    time = np.random.default_rng(3).uniform(0, 1, size=n).astype(np.float32)
    ref = s.trace_shadow_tr(*rays)
    got = _tr_device(s, rays, time)
    s.close()
    print(name, "lit %.3f, black %.3f" % ((ref > 0).any(axis=1).mean(), (ref == 0).all(axis=1).mean()))
    assert np.isfinite(got).all()
    if name == "media_box":   # (tests/test_animated_materials_gpu.py asks this of the host-array call on these rays)
        assert (got > 0).any(axis=1).mean() > 0.1 and (got == 0).all(axis=1).mean() > 0.05
    else:                     # some rays arrive, some are blocked
        assert (got > 0).any(axis=1).any() and (got == 0).all(axis=1).any()
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()


def _animated_tr_rays(s, name, n):
    lo, hi = s.bounds()
    if name == "animated_interface":
        return _shadow_rays(lo, hi, n, 4, 2)
    # animated_in_definition_media: the rays of tests/test_animated_in_definition_gpu.py (one medium)
    rng = np.random.RandomState(4)
    o = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = (rng.uniform(lo, hi, size=(n, 3)).astype(np.float32) - o).astype(np.float32)
    rng = np.random.RandomState(4)
    medium = rng.randint(-1, 1, size=n).astype(np.int32)
    lam = np.sort(rng.uniform(380, 780, size=(n, 4)), axis=1).astype(np.float32)
    Ld = rng.uniform(0.1, 2, size=(n, 4)).astype(np.float32)
    ones = np.ones((n, 4), dtype=np.float32)
    return o, d, np.full(n, 0.9999, dtype=np.float32), medium, lam, Ld, ones, ones.copy()


@pytest.mark.parametrize("name", ["animated_interface", "animated_in_definition_media"])
def test_transmittance_on_an_animated_scene_is_the_timed_host_array_call(wfpt, name):
    s = _open(wfpt, name)
    n = 20000
    rays = _animated_tr_rays(s, name, n)
    times = {"0": np.zeros(n, dtype=np.float32), "1": np.ones(n, dtype=np.float32), "random": np.random.default_rng(7).uniform(0, 1, size=n).astype(np.float32)}
    ref = {k: s.trace_shadow_tr(*rays, time=t) for k, t in times.items()}
    got = {k: _tr_device(s, rays, t) for k, t in times.items()}
    s.close()
    for k in times:
        assert np.isfinite(got[k]).all(), k
        assert (got[k].view(np.uint32) == ref[k].view(np.uint32)).all(), k
    # (the existing host-array tests: the moving boundaries are elsewhere at time 1)
    assert (got["0"] != got["1"]).any(axis=1).mean() > 0.01
    assert (got["0"] > 0).any()


# ---- 5. one random intersection --------------------------------------------------------------------------------------------------
def _one_random_device(wfpt, s, p0, p1, material, time):
    segs7 = np.concatenate([p0, p1, time[:, None]], axis=1).astype(np.float32)
    rec, pdf = s.trace_one_random_device(_dev(segs7), _dev(material))
    return wfpt.hit_records(rec), pdf.cpu().numpy()


def test_one_random_on_a_moving_surface_is_the_timed_host_array_call(wfpt):
    """the construction of test_one_random_host_t_matches_the_timed_closest_hit_on_a_moving_surface: vertical probe segments down to the
    middle height of animated_subsurface's moving block at the segment's time"""
    s = _open(wfpt, "animated_subsurface")
    n = 4000
    rng = np.random.RandomState(9)
    time = rng.uniform(0, 1, size=n).astype(np.float32)
    xy = rng.uniform([-1.9, -1.0], [1.1, 1.0], size=(n, 2)).astype(np.float32)
    camera = np.array([0, -6, 3.5], dtype=np.float32)
    p0 = (np.concatenate([xy, np.full((n, 1), 3.5, np.float32)], axis=1) - camera).astype(np.float32)
    p1 = (np.concatenate([xy, (1.5 + 0.5 * time)[:, None]], axis=1) - camera).astype(np.float32)
    found = {}
    for m in range(16):
        rec, pdf = s.trace_one_random(p0, p1, np.full(n, m, dtype=np.int32), time=time)
        if (pdf > 0).any():
            found[m] = (rec, pdf)
    assert len(found) == 1, sorted(found)
    (m, (ref, ref_pdf)), = found.items()
    got, pdf = _one_random_device(wfpt, s, p0, p1, np.full(n, m, dtype=np.int32), time)
    s.close()
    assert 0.05 < (pdf > 0).mean() < 0.9
    assert got.tobytes() == ref.tobytes()
    assert (pdf.view(np.uint32) == ref_pdf.view(np.uint32)).all()


def test_one_random_on_a_static_scene_is_the_host_array_call(wfpt):
    """segments between random points of a box around the two subsurface blobs of `subsurface` (world (-3, -2, 0.1) .. (3, 2, 2.6); the
    camera stands at (0, -7.5, 3.2)).  Measured on the MI355X: see the printed fractions"""
    s = _open(wfpt, "subsurface")
    n = 4000
    rng = np.random.RandomState(13)
    camera = np.array([0, -7.5, 3.2], dtype=np.float32)
    p0 = (rng.uniform([-3, -2, 0.1], [3, 2, 2.6], size=(n, 3)).astype(np.float32) - camera).astype(np.float32)
    p1 = (rng.uniform([-3, -2, 0.1], [3, 2, 2.6], size=(n, 3)).astype(np.float32) - camera).astype(np.float32)
    time = rng.uniform(0, 1, size=n).astype(np.float32)   # ignored: the scene is static
    fractions = {}
    for m in range(16):
        mat = np.full(n, m, dtype=np.int32)
        ref, ref_pdf = s.trace_one_random(p0, p1, mat)
        got, pdf = _one_random_device(wfpt, s, p0, p1, mat, time)
        assert got.tobytes() == ref.tobytes(), m
        assert (pdf.view(np.uint32) == ref_pdf.view(np.uint32)).all(), m
        assert ((pdf > 0) == (got["prim"] >= 0)).all(), m
        if (pdf > 0).any():
            fractions[m] = float((pdf > 0).mean())
    s.close()
    print("hit fraction per material id:", fractions)
    assert fractions and max(fractions.values()) > 0.05


# ---- 6. scratch reuse and stream order -------------------------------------------------------------------------------------------
def test_the_transmittance_scratch_is_reused_by_calls_of_other_sizes(wfpt):
    s = _open(wfpt, "animated_interface")
    n = 20000
    rays = _animated_tr_rays(s, "animated_interface", n)
    time = np.random.default_rng(7).uniform(0, 1, size=n).astype(np.float32)
    first = _tr_device(s, rays, time)
    small = _tr_device(s, tuple(a[:64] for a in rays), time[:64])
    third = _tr_device(s, rays, time)
    s.close()
    assert (first > 0).any()
    assert first.tobytes() == third.tobytes()
    assert small.tobytes() == first[:64].tobytes()


def test_torch_ops_before_and_after_the_call_need_no_synchronisation(wfpt, anim_rays, cpu_hits):
    import torch
    o, d, tmax, time = anim_rays
    ref = cpu_hits("animated_tris")
    s = _open(wfpt, "animated_tris")
    parts = [_dev(a) for a in (o, d, tmax[:, None], time[:, None])]
    torch.cuda.synchronize()
    for _ in range(3):   # (the later rounds reuse memory the allocator has just taken back from the previous round's tensors)
        rays8 = (torch.cat(parts, dim=1) * 1.0).contiguous()   # produced on torch's stream immediately before the call
        rec = s.trace_device(rays8)
        n_hits = (rec[:, 0] >= 0).sum()                          # consumed on torch's stream immediately after it
        prim_sum = rec[:, 0].to(torch.int64).sum()
        del rays8
        assert int(n_hits) == int((ref["prim"] >= 0).sum())
        assert int(prim_sum) == int(ref["prim"].astype(np.int64).sum())
    _same_hits(wfpt.hit_records(rec), ref)
    s.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_leave_the_context_usable(wfpt):
    import torch
    _, hip = wfpt.libs()
    s = _open(wfpt, "cornell64")
    n = 256
    lo, hi = s.bounds()
    o, d, tmax = _random_rays(n, lo, hi, 5)
    rays8 = _rays8(o, d, tmax, np.zeros(n, dtype=np.float32))
    dev = _dev(rays8)
    f4 = torch.ones((n, 4), dtype=torch.float32, device=dev.device)
    with pytest.raises(wfpt.WfError, match="no media"):
        s.trace_shadow_tr_device(dev, torch.zeros(n, dtype=torch.int32, device=dev.device), f4, f4, f4, f4)
    flat = torch.zeros(8 * n + 1, dtype=torch.float32, device=dev.device)
    shifted = flat[1:].view(n, 8)   # four bytes past an aligned address
    shifted.copy_(dev)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    with pytest.raises(wfpt.WfError, match="aligned to 16 bytes"):
        s.trace_device(shifted)
    with pytest.raises(wfpt.WfError, match="aligned to 16 bytes"):
        s.trace_device(shifted, any_hit=True)
    torch.cuda.synchronize()
    hip.wf_trace_closest_device_t.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert hip.wf_trace_closest_device_t(s.ctx, n, dev.data_ptr(), None) != 0
    assert "null out" in hip.wf_last_error().decode()
    hip.wf_trace_one_random_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    assert hip.wf_trace_one_random_device(s.ctx, n, dev.data_ptr(), dev.data_ptr(), None, None) != 0
    assert "null output" in hip.wf_last_error().decode()
    # a valid call on the same context afterwards
    got = wfpt.hit_records(s.trace_device(dev))
    ref = s.trace_closest(o, d, tmax, reference_order=False)
    s.close()
    assert (got["prim"] >= 0).mean() > 0.3
    _same_hits(got, ref)
