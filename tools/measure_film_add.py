#!/usr/bin/env python3
"""tools/measure_film_add.py — wf_film_add_samples_device against the render's own "Update film" launch, on one GPU (DESIGN 4.4,
profiles/film_add_device.txt): the Cornell box of tests/golden/cornell64.pbrt at 1920 x 1080 and 3840 x 2160, one sample per pixel.
Four alternating rounds of: one render pass at samples_per_pass = 1 with the profile on, its "Update film" time from wf_kernel_time_ms;
and wf_film_add_samples_device over the scene's own camera samples (Scene.camera_samples_device, every pixel once) between two events on
the context's stream.  Bytes per item, from the kernels' loads and stores:
  film add      8 pixel + 16 L4 + 16 lambda4 + 16 lambda_pdf4 + 4 weight = 60 read, 4 + 4 the stamp's atomic and its old value, 32 + 32 the film record
  update film   8 pPixel + 16 L + 16 cameraRayWeight + 16 lambda + 16 lambdaPdf + 4 filterWeight = 76 read, 32 + 32 the film record
(the twelve sensor-table loads of either kernel hit a table of 3 x 471 floats and are not counted)."""
import ctypes as C
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest

ADD_BYTES, UPDATE_BYTES = 60 + 8 + 64, 76 + 64
wfpt = conftest.load_pkg()
host, hip = wfpt.libs()
text = open(os.path.join(conftest.GOLDEN, "cornell64.pbrt")).read()
film_re = re.compile(r'Film "rgb".*?"bool savefp16" \[ false \]', re.S)
assert film_re.search(text)
for W, H in ((1920, 1080), (3840, 2160)):
    film = 'Film "rgb" "string filename" [ "m.pfm" ] "integer xresolution" [ %d ] "integer yresolution" [ %d ] "bool savefp16" [ false ]' % (W, H)
    s = wfpt.Scene(text=film_re.sub(film, text), spp=1)
    s.create_renderer(0, samples_per_pass=1)
    dev = torch.device("cuda", 0)
    rays, pix, lam, pdf, camw, fw = s.camera_samples_device(0)
    n = pix.shape[0]
    assert n == W * H
    Lw = torch.rand((n, 4), dtype=torch.float32, device=dev) * camw
    rejected = torch.zeros(1, dtype=torch.int32, device=dev)
    ext = torch.cuda.ExternalStream(hip.wf_stream(s.ctx), device=dev)
    f = hip.wf_film_add_samples_device
    f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    torch.cuda.synchronize()
    print("%d x %d, %d items: film add %d B/item = %d B, update film %d B/item = %d B, byte ratio %.3f" % (W, H, n, ADD_BYTES, ADD_BYTES * n, UPDATE_BYTES,
                                                                                                      UPDATE_BYTES * n, ADD_BYTES / UPDATE_BYTES), flush=True)
    s.enable_profile(True)
    for run in range(4):
        s.clear_film()
        s.profile_report()   # (forgets the launches recorded so far)
        s.render(0, 1)
        ms, launches = C.c_double(0), C.c_int(0)
        wfpt._check(hip.wf_kernel_time_ms(s.ctx, b"Update film", C.byref(ms), C.byref(launches)), "wf_kernel_time_ms")
        up = ms.value
        s.enable_profile(False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ext)
        rc = f(s.ctx, n, None, pix.data_ptr(), Lw.data_ptr(), lam.data_ptr(), pdf.data_ptr(), fw.data_ptr(), rejected.data_ptr())
        e1.record(ext)
        e1.synchronize()
        assert rc == 0
        add = e0.elapsed_time(e1)
        s.enable_profile(True)
        print("  run %d: update film %.4f ms in %d launch(es) = %.2f TB/s; film add %.4f ms = %.2f TB/s; time ratio add / update %.3f"
              % (run, up, launches.value, UPDATE_BYTES * n / up * 1e-9, add, ADD_BYTES * n / add * 1e-9, add / up), flush=True)
    assert int(rejected.item()) == 0
    s.close()
    del rays, pix, lam, pdf, camw, fw, Lw
    torch.cuda.empty_cache()
