#!/usr/bin/env python3
"""tools/measure_film_develop.py — the film developed on the device against the host path, on one GPU (DESIGN 4.4,
profiles/film_develop_device.txt): the Cornell box of tests/golden/cornell64.pbrt with `Film "gbuffer"`, then `Film "rgb"`, at
3840 x 2160 and 1 spp, savefp16 on.  Four alternating runs of: Scene.film_channels() / image() (download + host loop, wall time),
Scene.film_channels_tensor() / image_tensor() (wall time, synchronised), and wf_film_develop_device alone between two events on the
context's stream, with the bytes the kernel moves (accumulators read + image written, from the struct sizes) over that time."""
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest

wfpt = conftest.load_pkg()
host, hip = wfpt.libs()
text = open(os.path.join(conftest.GOLDEN, "cornell64.pbrt")).read()
film_re = re.compile(r'Film "rgb".*?"bool savefp16" \[ false \]', re.S)
assert film_re.search(text)
FILMS = {"gbuffer": 'Film "gbuffer" "string filename" [ "m.exr" ] "integer xresolution" [ 3840 ] "integer yresolution" [ 2160 ] "bool savefp16" [ true ]',
         "rgb": 'Film "rgb" "string filename" [ "m.exr" ] "integer xresolution" [ 3840 ] "integer yresolution" [ 2160 ] "bool savefp16" [ true ]'}
for kind, film in FILMS.items():
    s = wfpt.Scene(text=film_re.sub(film, text), spp=1)
    s.create_renderer(0)
    s.render()
    H, W = s.height, s.width
    nc = 25 if kind == "gbuffer" else 3
    in_bytes = H * W * (32 + (136 if kind == "gbuffer" else 0))
    out_bytes = H * W * nc * 4
    out = torch.empty((H, W, nc), dtype=torch.float32, device="cuda:0")
    ext = torch.cuda.ExternalStream(hip.wf_stream(s.ctx), device=torch.device("cuda:0"))
    print("%s film %d x %d, %d channels: accumulators read %d B + image written %d B = %d B" % (kind, W, H, nc, in_bytes, out_bytes, in_bytes + out_bytes), flush=True)
    for run in range(4):
        line = "  run %d:" % run
        t0 = time.perf_counter()
        ref = s.film_channels()[1] if kind == "gbuffer" else s.image()
        t1 = time.perf_counter()
        line += " host path (download + host loop) %.1f ms;" % ((t1 - t0) * 1e3)
        t0 = time.perf_counter()
        if kind == "gbuffer":
            s.film_channels_tensor(out=out)
        else:
            s.image_tensor(out=out)
        t1 = time.perf_counter()
        line += " device path (tensor call, synchronised) %.3f ms;" % ((t1 - t0) * 1e3)
        if run == 0:
            same = bool((out.cpu().numpy().view(np.uint32) == ref.view(np.uint32)).all())
            line += " bit-identical %s;" % same
        del ref
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        f = hip.wf_film_develop_device
        e0.record(ext)
        rc = f(s.ctx, out.data_ptr(), out.numel(), 1, None)
        e1.record(ext)
        e1.synchronize()
        assert rc == 0
        ms = e0.elapsed_time(e1)
        line += " kernel %.4f ms = %.2f TB/s = %.1f %% of 8 TB/s" % (ms, (in_bytes + out_bytes) / ms * 1e-9, (in_bytes + out_bytes) / ms * 1e-9 / 8 * 100)
        print(line, flush=True)
    s.close()
    del out
    torch.cuda.empty_cache()
