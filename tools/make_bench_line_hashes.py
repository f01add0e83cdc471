#!/usr/bin/env python3
"""tests/golden/bench_line_ref_hashes.json: what the reference renders of the scenes bench.py's workload-line test benchmarks.

For each workload, the scene file bench.py generates for `--workload W --steps 2 --warmup 1` (2 spp, 1920x1080) is rendered by the
reference's CPU wavefront path (oracle/_ref/pbrt_ref --wavefront --seed 0 --spp 2).  Recorded: the sha1 of the scene file (generator
drift check) and the sha256 of the reference image's float32 pixels, top row first (the layout of bench.py --dump-outputs image.npy).
The GPU suite compares the image bench.py dumps with it, so that the bench line is checked against the reference without the reference
build on the machine that runs it.

    python tools/make_bench_line_hashes.py [--ref oracle/_ref/pbrt_ref] [killeroo-like cloud-like]
"""
import argparse
import hashlib
import importlib.util
import json
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "bench_line_ref_hashes.json")
SPP = 2   # bench.py --steps 2 --warmup 1 generates its scene with 2 spp


def load_bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def file_sha1(path):
    h = hashlib.sha1()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def image_sha256(img):
    return hashlib.sha256(np.ascontiguousarray(img, dtype="<f4").tobytes()).hexdigest()


def read_pfm(path):
    with open(path, "rb") as f:
        magic = f.readline().strip()
        assert magic == b"PF", magic
        w, h = map(int, f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), dtype="<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return data[::-1].astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.path.join(ROOT, "oracle", "_ref", "pbrt_ref"))
    ap.add_argument("workloads", nargs="*", default=["killeroo-like", "cloud-like"])
    a = ap.parse_args()
    bench = load_bench()
    table = json.load(open(OUT)) if os.path.exists(OUT) else {}
    for w in a.workloads:
        with tempfile.TemporaryDirectory() as td:
            scene = os.path.join(td, w + ".pbrt")
            bench.make_scene(scene, SPP, w)
            out = os.path.join(td, "ref.pfm")
            subprocess.run([a.ref, "--wavefront", "--quiet", "--seed", "0", "--spp", str(SPP), "--outfile", out, scene], check=True, cwd=td)
            img = read_pfm(out)
            table[w] = {"spp": SPP, "resolution": [img.shape[1], img.shape[0]], "scene_sha1": file_sha1(scene), "image_sha256": image_sha256(img),
                        "image_mean": float(img.astype(np.float64).mean())}
            print(w, table[w], flush=True)
    with open(OUT, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
