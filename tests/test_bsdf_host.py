"""wf_bsdf_make_device and wf_bsdf_eval_device without a GPU: declared, exported, listed, refusing a null context by name, bound by
Scene — and the per-row bodies their kernels run (pbrt-v4_amd/csrc/hip/wf_boundary_bsdf.h), compiled for the host as the stand-alone
program tools/bsdf_check.cpp, against a direct composition of the render's own material functions (ResolveMix, MatBxDF<T>::Get,
BSDF<T>::f / PDF / Sample_f) on the first hits of twelve scenes: every output word equal, also under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from suite_helpers import declared

NEW_ABI = ["wf_bsdf_make_device", "wf_bsdf_eval_device"]
SRC = os.path.join(ROOT, "pbrt-v4_amd")
FIXTURES = ["matrix_lean", "matrix_lean_tex", "mix_materials", "materials_lights", "textures_bump", "alpha_normalmap", "displacement", "hair",
            "measured", "subsurface", "textures_noise", "parser_torture"]
ROWS = 20000


def test_new_symbols_declared_exported_and_listed(wfpt):
    _, hip = wfpt.libs()
    abi = declared("wf_abi.h")
    for name in NEW_ABI:
        assert name in abi and name in wfpt.ABI_SYMBOLS and hasattr(hip, name), name
    assert sorted(wfpt.ABI_SYMBOLS) == abi and len(abi) == 87
    hip.wf_abi_version.restype = C.c_int
    assert hip.wf_abi_version() == 12
    header = open(os.path.join(ROOT, "include", "wf_abi.h")).read()
    assert re.search(r"#define\s+WF_ABI_VERSION\s+12\b", header)
    assert re.search(r"#define\s+WF_BSDF_PLANES\s+10\b", header) and wfpt.BSDF_PLANES == 10


def test_null_context_is_refused_by_name_before_anything_else(wfpt):
    _, hip = wfpt.libs()
    f = hip.wf_bsdf_make_device
    f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
    g = hip.wf_bsdf_eval_device
    g.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 12
    for n in (0, -3, 16):
        assert f(None, n, *[None] * 8) != 0
        assert b"wf_bsdf_make_device: null context" in hip.wf_last_error()
        assert g(None, n, *[None] * 12) != 0
        assert b"wf_bsdf_eval_device: null context" in hip.wf_last_error()


def test_scene_binds_the_two_calls_and_the_plan_names_the_types(wfpt):
    for name in ("bsdf_device", "bsdf_eval_device"):
        assert callable(getattr(wfpt.Scene, name))
    s = wfpt.Scene(path=os.path.join(GOLDEN, "matrix_lean.pbrt"), spp=1)
    assert s.plan("bsdf_planes") == 10
    assert s.plan("material_types") == sum(1 << t for t in range(1, 11))      # the matrix holds every type
    s.close()
    s = wfpt.Scene(path=os.path.join(GOLDEN, "cornell64.pbrt"), spp=1)
    assert s.plan("material_types") == 1 << 1                                  # diffuse walls only
    s.close()


@pytest.fixture(scope="module")
def check_program(built):
    """pbrt-v4_amd/_build/bsdf_check: part of the Makefile's `all` (an up-to-date build makes this a no-op)"""
    subprocess.run(["make", "-C", SRC, "_build/bsdf_check"], check=True, capture_output=True)
    return os.path.join(SRC, "_build", "bsdf_check")


@pytest.fixture(scope="module")
def self_results(check_program):
    """--self on every fixture, once: {name: the program's JSON line}"""
    out = {}
    for name in FIXTURES:
        p = subprocess.run([check_program, "--self", os.path.join(GOLDEN, name + ".pbrt"), str(ROWS)], capture_output=True, text=True)
        assert p.returncode == 0, name + ": " + p.stdout + p.stderr
        out[name] = json.loads(p.stdout.strip().splitlines()[-1])
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_per_row_bodies_match_the_renders_material_functions(self_results, name):
    """RouteRow / MakeRow / RecordType / EvalRow, run pass by pass as the kernels run them, against the direct composition: 20 000 rows
    from the scene's own first hits, misses, invalid records, interface rows and stale material ids between them, every other row
    regularised, wi and u seeded — 0 mismatches, and the rows reach BSDFs at all"""
    r = self_results[name]
    assert r["rows"] == ROWS and r["mismatches"] == 0, r
    assert r["hits"] > ROWS // 10 and r["zero_rows"] > 0 and sum(r["type_rows"]) + r["zero_rows"] == ROWS, r
    assert r["valid_samples"] > 0 and r["f_nonzero"] > 0, r


def test_the_rows_cover_what_a_silent_skip_would_hide(self_results):
    a, b = self_results["matrix_lean"], self_results["matrix_lean_tex"]
    for t in range(1, 11):                                                      # every one of the ten types, over the two matrix scenes
        assert a["type_rows"][t] + b["type_rows"][t] > 0, (t, a["type_rows"], b["type_rows"])
    for k in ("valid_samples", "transmitted", "specular", "proportional", "f_nonzero"):
        assert a[k] > 0, (k, a)
    m = self_results["mix_materials"]
    assert m["mix_rows"] > 0 and m["mix_child"][0] > 0 and m["mix_child"][1] > 0, m    # the mix resolves to both children ...
    assert m["mix_against_render"] == m["mix_rows"], m                                  # ... as the render's ResolveMix does from the hit itself
    assert self_results["parser_torture"]["terminated"] > 0                             # "spectrum eta" "glass-BK7": dispersion
    r = self_results["materials_lights"]                                                # a smooth conductor: Regularize changes the BxDF
    assert r["regularized"] > 0 and r["regularized_differ"] > 0, r
    assert self_results["hair"]["type_rows"][9] > 0 and self_results["measured"]["type_rows"][10] > 0 and self_results["subsurface"]["type_rows"][8] > 0


@pytest.fixture(scope="module")
def sanitized_program(built, tmp_path_factory):
    """the same program with the host units it links, every one compiled by g++ with -fsanitize=address,undefined: a plain executable
    with both runtimes linked in, so it neither needs one preloaded nor minds what else a process here has preloaded"""
    out = str(tmp_path_factory.mktemp("bsdf_check_san"))
    san = "-g -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan"
    subprocess.run(["make", "-C", SRC, "-j8", "OUT=" + out, "CXX=g++", "CXXFLAGS=-std=c++17 -O1 -mfma -ffp-contract=off -fPIC -pthread -I ../include",
                    "SAN=" + san, os.path.join(out, "bsdf_check")], check=True, capture_output=True)
    return os.path.join(out, "bsdf_check")


@pytest.mark.parametrize("name", ["matrix_lean_tex", "mix_materials"])
def test_per_row_bodies_under_the_sanitizers(sanitized_program, name):
    p = subprocess.run([sanitized_program, "--datadir", os.path.join(SRC, "data"), "--self", os.path.join(GOLDEN, name + ".pbrt"), str(ROWS)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["rows"] == ROWS and r["mismatches"] == 0, r
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr


def test_eval_answers_with_the_direct_composition(wfpt, check_program, tmp_path):
    """--eval, the expected-output side of the GPU tests: one hand-made Lambertian row on cornell64's white floor and a miss"""
    import numpy as np
    s = wfpt.Scene(path=os.path.join(GOLDEN, "cornell64.pbrt"), spp=1)
    assert s.plan("material_types") == 2
    s.close()
    n = 2
    rays = np.zeros((n, 8), np.float32)
    rays[:, 3:6] = (0, -1, 0)
    pf = np.zeros((11, n, 4), np.float32)
    pi = np.zeros((2, n, 4), np.int32)
    pf[0, :, :3] = pf[1, :, :3] = (0.0, -2.73, 10.795)                         # (rendering space: the camera (2.78 2.73 -8) is the origin; the floor is y = 0)
    pf[0, :, 1] -= 1e-4                                                         # (an interval with some width, as a hit has it)
    pf[1, :, 1] += 1e-4
    pf[2, :, :3] = pf[3, :, :3] = (0, 1, 0)
    pf[2, :, 3] = 0.25
    pf[4, :, :3] = (0, 1, 0)
    pf[5, :, :3] = pf[7, :, :3] = (1, 0, 0)
    pf[6, :, :3] = pf[8, :, :3] = (0, 0, 1)
    pi[0] = -1
    white = None
    # the white material's id: the one whose reflectance is the same at every wavelength (found by asking the program itself below)
    lam = np.tile(np.array([450, 520, 590, 660], np.float32), (n, 1))
    wi = np.tile(np.array([0.6, 0.8, 0.0, 0.0], np.float32), (n, 1))
    u4 = np.tile(np.array([0.5, 0.3, 0.7, 0.0], np.float32), (n, 1))
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for material in range(8):
        pi[0, 0, 0] = material
        pi[1, 0, 1] = 1                                                         # row 0 a hit, row 1 a miss
        head = np.array([0x42534431, n, 0, 1, 1, 0, 0, 0], np.int32)
        with open(a, "wb") as f:
            for x in (head, rays, pf, pi, lam, wi, u4):
                f.write(x.tobytes())
        subprocess.run([check_program, "--eval", os.path.join(GOLDEN, "cornell64.pbrt"), a, b], check=True)
        raw = open(b, "rb").read()
        assert len(raw) == n * 16 * (10 + 1 + 2 + 2 + 3)
        off = 0
        def take(dtype, rows, cols=4):
            nonlocal off
            v = np.frombuffer(raw, dtype, rows * cols, off).reshape(rows, cols)
            off += rows * cols * 4
            return v
        rec = take(np.float32, 10 * n).reshape(10, n, 4)
        b4, f4, pdf4 = take(np.int32, n), take(np.float32, n), take(np.float32, n)
        nxt, sf, sp, si = take(np.float32, n, 8), take(np.float32, n), take(np.float32, n), take(np.int32, n)
        if b4[0, 3] == 0:
            break                                                               # past the scene's material table: a zero row
        assert tuple(b4[0]) == (1 | 4, 1, material, 1)                          # diffuse reflection, side +1, the material, type diffuse
        if len(set(f4[0].tolist())) == 1:
            white = material
            break
    assert white is not None, "cornell64 has a white wall"
    assert f4[0, 0] > 0 and (f4[0] == f4[0, 0]).all() and (sf[0] == f4[0]).all()            # f is the same on all four wavelengths, sampled or given
    assert pdf4[0, 1] == np.float32(0.8) and abs(pdf4[0, 0] - 0.8 / math.pi) < 1e-7          # |wi . ns| and the cosine-hemisphere PDF
    assert tuple(si[0]) == (1, 1 | 4, -1, 0) and sp[0, 0] == sp[0, 1] and sp[0, 3] == 1
    # cos / pdf is pi to within fp32 rounding: pdf = cos * InvPi, so three roundings of half an ulp each (the constant, the product, the
    # quotient taken here in fp32) — under 2 ulp of pi
    assert abs(float(np.float32(sp[0, 2]) / np.float32(sp[0, 0])) - math.pi) < 2 * math.pi * 2 ** -23
    d = nxt[0, 3:6]
    assert d[1] > 0 and abs(np.linalg.norm(d) - 1) < 1e-6                                    # the sampled wi lies in wo's hemisphere
    assert nxt[0, 1] >= pf[1, 0, 1] and np.isinf(nxt[0, 6]) and nxt[0, 7] == np.float32(0.25)  # the origin left the floor along n; tMax, the row's time
    assert rec[0, 0].view(np.int32).tolist() == [1, 5, white, 0] and tuple(rec[1, 0]) == (0, 1, 0, 0)
    for x in (rec[:, 1], b4[1], f4[1], pdf4[1], nxt[1], sf[1], sp[1], si[1]):                 # the miss row is all zeros
        assert not x.any()
