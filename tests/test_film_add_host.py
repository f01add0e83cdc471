"""wf_camera_samples_device and wf_film_add_samples_device without a GPU: declared, exported, listed, refusing a null context by name, bound
by Scene — and the per-item bodies the film-add kernel runs (pbrt-v4_amd/csrc/hip/wf_film_add.h), compiled for the host as the
stand-alone program tools/film_add_check.cpp, against the render's own KUpdateFilm: accumulators equal byte for byte, also under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from suite_helpers import declared

NEW_ABI = ["wf_camera_samples_device", "wf_film_add_samples_device"]
SRC = os.path.join(ROOT, "pbrt-v4_amd")


def test_new_symbols_declared_exported_and_listed(wfpt):
    _, hip = wfpt.libs()
    abi = declared("wf_abi.h")
    for name in NEW_ABI:
        assert name in abi and name in wfpt.ABI_SYMBOLS and hasattr(hip, name), name
    assert sorted(wfpt.ABI_SYMBOLS) == abi
    hip.wf_abi_version.restype = C.c_int
    assert hip.wf_abi_version() == 12
    assert re.search(r"#define\s+WF_ABI_VERSION\s+12\b", open(os.path.join(ROOT, "include", "wf_abi.h")).read())


def test_null_context_is_refused_by_name_before_anything_else(wfpt):
    _, hip = wfpt.libs()
    f = hip.wf_film_add_samples_device
    f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    for n in (0, -3, 16):   # before n <= 0 returns 0
        assert f(None, n, None, None, None, None, None, None, None) != 0
        assert b"wf_film_add_samples_device: null context" in hip.wf_last_error()
    g = hip.wf_camera_samples_device
    g.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7
    assert g(None, 0, 0, 0, None, None, None, None, None, None, None) != 0
    assert b"wf_camera_samples_device: null context" in hip.wf_last_error()


def test_scene_binds_the_two_calls(wfpt):
    for name in ("camera_samples_device", "film_add_device"):
        assert callable(getattr(wfpt.Scene, name))


@pytest.fixture(scope="module")
def check_program(built):
    """pbrt-v4_amd/_build/film_add_check: part of the Makefile's `all` (an up-to-date build makes this a no-op)"""
    subprocess.run(["make", "-C", SRC, "_build/film_add_check"], check=True, capture_output=True)
    return os.path.join(SRC, "_build", "film_add_check")


def _assert_clean(p):
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if "no difference; 7 duplicates rejected; the epoch wrap adds every item" in l]
    assert [l.split(":")[0] for l in lines] == ["film type 0", "film type 1", "film type 2"], p.stdout


def test_per_item_bodies_match_the_renders_film_update(check_program):
    """KUpdateFilm into one film, filmadd::AddItem into another, for an RGB, a spectral and a GBuffer film with a crop window: the clamp
    threshold one ulp either side, PDFs with zeros, wavelengths on every bucket boundary, pixels on and outside every edge, negative and
    zero weights, infinite and NaN radiance — byte for byte"""
    _assert_clean(subprocess.run([check_program], capture_output=True, text=True))


def test_per_item_bodies_under_the_sanitizers(built, tmp_path):
    """the same program, a plain executable built with -fsanitize=address,undefined, run in the environment as it is: no report.  Both
    runtimes are linked into the executable, so it neither needs one preloaded nor minds what else a process here has preloaded"""
    exe = str(tmp_path / "film_add_check_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-mfma", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "film_add_check.cpp"),
                    "-o", exe], check=True, capture_output=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    _assert_clean(p)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
