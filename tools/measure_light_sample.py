#!/usr/bin/env python3
"""tools/measure_light_sample.py — wf_light_sample_device beside the render's own next-event-estimation kernel, on one GPU:
the Cornell box of tests/golden/cornell400.pbrt, one sample per pixel.  Four alternating rounds of: one render of sample index 0 with the
profile on — the time of "DiffuseMaterial: next-event estimation" (k_mat_nee<diffuse, RARE>: the light sample AND the BSDF, the MIS
weights and the shadow-queue push) from wf_kernel_time_ms, over all depths, divided by the diffuse items the material stage evaluated;
and wf_light_sample_device over the first hits of the scene's camera rays (every pixel one row; the light sample and the shadow ray
alone) between two events on the context's stream.  For orientation: the two kernels do not do the same work, and nothing is a target."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest

wfpt = conftest.load_pkg()
host, hip = wfpt.libs()
s = wfpt.Scene(path=os.path.join(conftest.GOLDEN, "cornell400.pbrt"), spp=1)
s.create_renderer(0, samples_per_pass=1)
dev = torch.device("cuda", 0)
fh = s.first_hit(0)
n = fh["rays8"].shape[0]
u4 = torch.rand((n, 4), dtype=torch.float32, device=dev)
side = torch.ones(n, dtype=torch.int32, device=dev)
out = s.sample_lights_device(fh, fh["lambda4"], u4, side)
ext = torch.cuda.ExternalStream(hip.wf_stream(s.ctx), device=dev)
torch.cuda.synchronize()
usable = int((out["pdf"] != 0).sum().item())
print("cornell400: %d rows (%d usable), light_sample_rare = %d" % (n, usable, s.query("light_sample_rare")), flush=True)
f = hip.wf_light_sample_device
f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 10
args = [None, fh["planes_f"].data_ptr(), fh["planes_i"].data_ptr(), fh["lambda4"].data_ptr(), u4.data_ptr(), side.data_ptr(), out["shadow_rays8"].data_ptr(),
        out["L4"].data_ptr(), out["wi_pdf4"].data_ptr(), out["light4"].data_ptr()]
for run in range(4):
    s.enable_profile(True)
    s.clear_film()
    s.profile_report()   # (forgets the launches recorded so far)
    s.render(0, 1)
    ms, launches = C.c_double(0), C.c_int(0)
    wfpt._check(hip.wf_kernel_time_ms(s.ctx, b"DiffuseMaterial: next-event estimation", C.byref(ms), C.byref(launches)), "wf_kernel_time_ms")
    items = s.material_items()[1]
    s.enable_profile(False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ext)
    rc = f(s.ctx, n, *args)
    e1.record(ext)
    e1.synchronize()
    assert rc == 0
    t = e0.elapsed_time(e1)
    print("  run %d: k_mat_nee (diffuse) %.4f ms in %d launches over %d items = %.4f ms per million items; wf_light_sample_device %.4f ms = %.4f ms per million rows"
          % (run, ms.value, launches.value, items, ms.value / max(items, 1) * 1e6, t, t / n * 1e6), flush=True)
s.close()
