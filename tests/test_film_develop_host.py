"""The device film develop without a GPU: its entry points are declared and exported, the Python calls fail loudly without a renderer,
and the per-pixel bodies the kernels run (pbrt-v4_amd/csrc/hip/wf_film_develop.h), compiled for the host as the stand-alone program
tools/film_develop_check.cpp, agree with csrc/host/image_io.cpp's loops bit for bit."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from suite_helpers import declared

NEW_ABI = ["wf_film_channel_count", "wf_film_develop_device", "wf_film_develop_rgb_device", "wf_film_spectral_upload", "wf_film_gbuffer_upload"]
NEW_HOST = ["wfh_film_image_device"]


def test_new_symbols_declared_and_exported(wfpt):
    host, hip = wfpt.libs()
    abi, hst = declared("wf_abi.h"), declared("wf_host.h")
    for name in NEW_ABI:
        assert name in abi and name in wfpt.ABI_SYMBOLS and hasattr(hip, name), name
    for name in NEW_HOST:
        assert name in hst and name in wfpt.HOST_SYMBOLS and hasattr(host, name), name
    assert sorted(wfpt.ABI_SYMBOLS) == abi and sorted(wfpt.HOST_SYMBOLS) == hst   # (test_abi.py's check of the lists)


def test_tensor_calls_need_a_renderer(wfpt):
    s = wfpt.Scene(path=os.path.join(GOLDEN, "cornell64.pbrt"), spp=4)
    with pytest.raises(wfpt.WfError, match=r"create_renderer\(\) first"):
        s.image_tensor()
    with pytest.raises(wfpt.WfError, match=r"create_renderer\(\) first"):
        s.film_channels_tensor()
    host, _ = wfpt.libs()
    assert host.wfh_film_image_device(s.h, None, 0, 0, None) != 0
    assert b"no renderer" in host.wfh_last_error()
    s.close()


@pytest.fixture(scope="module")
def check_program(built):
    """pbrt-v4_amd/_build/film_develop_check: part of the Makefile's `all` (an up-to-date build makes this a no-op)"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "pbrt-v4_amd"), "_build/film_develop_check"], check=True, capture_output=True)
    return os.path.join(ROOT, "pbrt-v4_amd", "_build", "film_develop_check")


def test_round_to_half_twin_over_every_float(check_program):
    """the header's RoundToHalf against image_io.cpp's over all 2^32 bit patterns (threaded; exits non-zero at the first difference)"""
    p = subprocess.run([check_program, "round", str(min(16, os.cpu_count() or 1))], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "4294967296 bit patterns, no difference" in p.stdout


def test_per_pixel_bodies_match_the_host_loops(check_program):
    """DevelopRGB / DevelopBucket / DevelopGBuffer against FilmToRGB / SpectralFilmImage / GBufferFilmImage over fabricated accumulators
    (every half value, tie and neighbour of a tie; zero and negative weights; NaN and infinite sums; ...), savefp16 off and on"""
    p = subprocess.run([check_program, "arrays"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lines = [l for l in p.stdout.splitlines() if "no difference" in l]
    assert len(lines) == 2 and lines[0].startswith("savefp16 0") and lines[1].startswith("savefp16 1")
