"""The two device-buffer calls that close the loop for a GPU-resident caller — wf_hit_interaction_device (hit records to
SurfaceInteractions) and wf_camera_rays_device (the scene's own camera rays) — without a GPU: declared, exported, refusing a null context
by name, bound by wfpt.Scene, the kernel variant the plan chooses for every fixture scene, and the fixtures themselves
(tests/golden/intr_<name>/: what the reference's queues hold, tools/make_interaction_goldens.py).  What the calls compute is checked on
the GPU (tests/test_interaction_device_gpu.py)."""
import ctypes as C
import os
import re
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import make_interaction_goldens as goldens

NEW = {"wf_hit_interaction_device": [C.c_void_p, C.c_int] + [C.c_void_p] * 4,
       "wf_camera_rays_device": [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4}
# "intr_variant": bit 0 GENERAL, bit 1 CURVE_ALPHA, bit 2 ANIM — each fixture keeps the variant that serves it
VARIANT = {"tris": 0, "instances": 0, "general": 1, "curve_alpha": 3, "animated": 4, "nested": 4, "realistic": 0}
TAGS = {1.0, 2.0, 3.0, 6.0, 7.0}   # the material types ref_stages dumps = wf_material_type of diffuse, conductor, dielectric, coated diffuse, coated conductor


def test_header_declares_and_library_exports_both_calls(wfpt):
    text = open(os.path.join(ROOT, "include", "wf_abi.h")).read()
    _, hip = wfpt.libs()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*wf_ctx\s*\*ctx," % name, text), name
        assert hasattr(hip, name), name
        assert name in wfpt.ABI_SYMBOLS, name
    assert re.search(r"#define\s+WF_INTR_FPLANES\s+11\b", text) and re.search(r"#define\s+WF_INTR_IPLANES\s+2\b", text)
    assert (wfpt.INTR_FPLANES, wfpt.INTR_IPLANES) == (11, 2)


def test_abi_version_is_unchanged(wfpt):
    _, hip = wfpt.libs()
    assert hip.wf_abi_version() == 12
    assert re.search(r"#define\s+WF_ABI_VERSION\s+12\b", open(os.path.join(ROOT, "include", "wf_abi.h")).read())


def test_a_null_context_is_refused_with_the_calls_name(wfpt):
    """no device is needed to be told so: the check comes before anything touches the runtime, and before n <= 0 returns 0"""
    _, hip = wfpt.libs()
    for name, argtypes in NEW.items():
        f = getattr(hip, name)
        f.argtypes = argtypes
        f.restype = C.c_int
        for n in (0, 1, 64):
            args = [None, n] if name == "wf_hit_interaction_device" else [None, 0, 0, n]
            assert f(*args, None, None, None, None) != 0, (name, n)
            msg = hip.wf_last_error().decode()
            assert msg and name in msg, (name, msg)


def test_scene_binds_the_three_methods(wfpt):
    for m in ("interactions_device", "camera_rays_device", "first_hit"):
        assert callable(getattr(wfpt.Scene, m, None)), m


@pytest.mark.parametrize("name", goldens.NAMES)
def test_plan_names_the_fixtures_variant(wfpt, name):
    s = wfpt.Scene(path=os.path.join(GOLDEN, "intr_%s.pbrt" % name))
    try:
        assert s.plan("intr_variant") == VARIANT[name]
        assert (s.info.width, s.info.height) == (goldens.WIDTH, goldens.HEIGHT)
    finally:
        s.close()


def test_plan_keeps_the_lean_variant_for_a_triangle_scene(wfpt):
    s = wfpt.Scene(path=os.path.join(GOLDEN, "cornell64.pbrt"))
    try:
        assert s.plan("intr_variant") == 0
    finally:
        s.close()


@pytest.mark.parametrize("name", goldens.NAMES)
def test_fixture_covers_its_rays(name):
    """mat_items.bin holds a record for at least 95 % of the fixture's pixels (the realistic camera: of the rays camera_rays.bin holds):
    the scenes are closed rooms of the five dumped material types.  A pixel without a record is skipped by the GPU test, never compared
    loosely — so a fixture that falls short is a wrong scene."""
    d = os.path.join(GOLDEN, "intr_%s" % name)
    rays, items, need = goldens.coverage(d, name)
    assert items >= goldens.MIN_COVERAGE * need, (name, rays, items, need)
    assert rays == need if name != "realistic" else rays < goldens.WIDTH * goldens.HEIGHT, (name, rays)
    r = np.fromfile(os.path.join(d, "camera_rays.bin"), dtype=np.float32).reshape(-1, 8)
    m = np.fromfile(os.path.join(d, "mat_items.bin"), dtype=np.float32).reshape(-1, 28)
    assert set(np.unique(m[:, 0])) <= TAGS
    assert set(m[:, 1].astype(int)) <= set(r[:, 0].astype(int)) and len(set(m[:, 1])) == len(m)
    assert os.path.getsize(os.path.join(d, "camera_rays.bin")) < 64 << 10 and os.path.getsize(os.path.join(d, "mat_items.bin")) < 64 << 10


@pytest.mark.parametrize("name", goldens.NAMES)
def test_fixture_is_the_references_output(name):
    """where the reference tools are built: a fresh ref_stages run, its records in pixel order (the reference's threads push them in
    no fixed order: make_interaction_goldens.run_ref_stages), equals the committed files byte for byte"""
    if not os.path.exists(goldens.REF_STAGES):
        pytest.skip("oracle/_ref not built")
    with tempfile.TemporaryDirectory() as td:
        goldens.run_ref_stages(name, td)
        for f in goldens.FILES:
            assert open(os.path.join(td, f), "rb").read() == open(os.path.join(GOLDEN, "intr_%s" % name, f), "rb").read(), (name, f)
