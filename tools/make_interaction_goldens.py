#!/usr/bin/env python3
"""tools/make_interaction_goldens.py — the fixtures of tests/test_interaction_device_*.py: for every scene tests/golden/intr_<name>.pbrt the
queue contents the REFERENCE holds after "Generate camera rays" and after IntersectClosest at depth 0 of sample index 0, as
oracle/_ref/ref_stages dumps them (oracle/ref_build/ref_stages.cpp), copied to tests/golden/intr_<name>/:

  camera_rays.bin  per ray of ray queue 0, 8 float32: pixelIndex, o.xyz, d.xyz, time
  mat_items.bin    per MaterialEvalWorkItem, 28 float32: material type tag (1 diffuse, 2 conductor, 3 dielectric, 6 coated diffuse,
                   7 coated conductor), pixelIndex, pi lower xyz, pi upper xyz, n, ns, dpdus, wo, uv, dpdu, dpdv

pixelIndex counts the pixels of the pass row by row from the film's first scanline.  The scenes are closed rooms whose every surface has
one of the five dumped material types, so every camera ray leaves a record; a fixture with records for fewer than 95 % of its rays is a
wrong scene and is refused.  The records are stored in pixel order (run_ref_stages).

usage: make_interaction_goldens.py [name ...]      (default: all seven)"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_STAGES = os.path.join(ROOT, "oracle", "_ref", "ref_stages")
NAMES = ("tris", "instances", "general", "curve_alpha", "animated", "nested", "realistic")
WIDTH, HEIGHT = 24, 16
FILES = ("camera_rays.bin", "mat_items.bin")
MIN_COVERAGE = 0.95


def run_ref_stages(name, outdir):
    """ref_stages on the fixture scene `name`: the two dumps, outdir/camera_rays.bin and outdir/mat_items.bin, with their records put in
    PIXEL ORDER.  The reference pushes its queue items from a pool of threads, in whatever order they get there, so two runs write the
    same records in different orders; a pixel has at most one record in either file, so the order by pixelIndex is the one canonical
    form of what it wrote — the records themselves are copied bit for bit."""
    subprocess.run([REF_STAGES, os.path.join(GOLDEN, "intr_%s.pbrt" % name), outdir], check=True, cwd=GOLDEN, stdout=subprocess.DEVNULL)
    for f, width, key in (("camera_rays.bin", 8, 0), ("mat_items.bin", 28, 1)):
        path = os.path.join(outdir, f)
        a = np.fromfile(path, dtype=np.uint32).reshape(-1, width)
        pixel = a[:, key].view(np.float32)
        assert len(np.unique(pixel)) == len(pixel), "%s: a pixel with two records" % f
        a[np.argsort(pixel, kind="stable")].tofile(path)


def coverage(directory, name):
    """(rays, records, rays the records must cover): the realistic camera's rays are fewer than its pixels"""
    rays = np.fromfile(os.path.join(directory, "camera_rays.bin"), dtype=np.float32).reshape(-1, 8)
    items = np.fromfile(os.path.join(directory, "mat_items.bin"), dtype=np.float32).reshape(-1, 28)
    return len(rays), len(items), (len(rays) if name == "realistic" else WIDTH * HEIGHT)


def main(names):
    if not os.path.exists(REF_STAGES):
        sys.exit("%s is missing: build the reference tools first (make -C oracle ref)" % REF_STAGES)
    for name in names:
        with tempfile.TemporaryDirectory() as td:
            run_ref_stages(name, td)
            rays, items, need = coverage(td, name)
            if items < MIN_COVERAGE * need:
                sys.exit("intr_%s: %d material records for %d rays: below %.0f %% — fix the scene" % (name, items, need, 100 * MIN_COVERAGE))
            dst = os.path.join(GOLDEN, "intr_%s" % name)
            os.makedirs(dst, exist_ok=True)
            for f in FILES:
                shutil.copyfile(os.path.join(td, f), os.path.join(dst, f))
            print("intr_%-12s %4d rays, %4d material records (%.1f %%)" % (name, rays, items, 100.0 * items / need))


if __name__ == "__main__":
    main(sys.argv[1:] or NAMES)
