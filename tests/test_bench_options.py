"""bench.py's options on the CPU: what --dump-outputs writes (sizes, types, the fixed sample of a large image) and the options a plain run
refuses.  The GPU runs of the benchmark are in test_gpu_parity.py."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_whole_image_and_rays(tmp_path):
    bench = load_bench()
    img = np.random.default_rng(1).random((1080, 1920, 3), dtype=np.float32)
    bench.dump_outputs(str(tmp_path), img, [1.0, 2.0, 3.0])
    assert sorted(os.listdir(tmp_path)) == ["image.npy", "rays.npy"]
    out = np.load(tmp_path / "image.npy")
    assert out.dtype == np.float32 and (out == img).all()
    rays = np.load(tmp_path / "rays.npy")
    assert rays.dtype == np.float64 and rays.tolist() == [1.0, 2.0, 3.0]


def test_dump_outputs_of_a_4k_image_is_a_fixed_sample_within_64_mb(tmp_path):
    bench = load_bench()
    img = np.random.default_rng(2).random((2160, 3840, 3), dtype=np.float32)
    outs = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), img, [0.0, 0.0, 0.0])
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["image_sample.npy", "image_sample_pixels.npy", "rays.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in files) <= 64 << 20
        outs.append([np.load(tmp_path / d / f) for f in files])
    sample, pix = outs[0][0], outs[0][1]
    assert sample.dtype == np.float32 and pix.dtype == np.float64 and sample.shape == (pix.shape[0], 3) == (bench.DUMP_MAX_PIXELS, 3)
    assert (np.diff(pix) > 0).all() and pix[0] >= 0 and pix[-1] < 3840 * 2160
    assert (sample == img.reshape(-1, 3)[pix.astype(np.int64)]).all()
    assert all((x == y).all() for x, y in zip(outs[0], outs[1]))   # the same pixels every run


def test_plain_run_refuses_full_only_breakdown_and_zero_steps():
    for args in (["--breakdown"], ["--steps", "0"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert p.returncode == 2 and "error" in p.stderr, (args, p.stderr[-500:])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout
