#!/usr/bin/env python3
"""tools/measure_bsdf_device.py [OUT [COMMIT]] — wf_bsdf_make_device and wf_bsdf_eval_device on one GPU, for orientation: nobody has
measured these kernels and nothing is a target.  Two scenes: tests/golden/cornell400.pbrt (160 000 first hits, one material type: two
launches per call) and tests/golden/matrix_lean_tex.pbrt (4 096 first hits, all ten types, image textures and a bump map: eleven
launches per call, every one scanning all rows).  Per scene: three warm-up rounds, then five timed rounds of each call between two
events on the context's stream — eval with both halves (wi = the scene's light directions, u4 random).  Writes the lines to OUT
(default profiles/bsdf_device.txt) with the GPU's name and the commit the tree is at."""
import ctypes as C
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest

wfpt = conftest.load_pkg()
host, hip = wfpt.libs()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def commit():
    if len(sys.argv) > 2:
        return sys.argv[2]   # (a tree without its git metadata: the caller says where it is)
    try:
        p = subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True)
        return p.stdout.strip() or "unknown (no git metadata beside the tree)"
    except OSError:
        return "unknown (no git)"


first = True
for name in ("cornell400", "matrix_lean_tex"):
    s = wfpt.Scene(path=os.path.join(conftest.GOLDEN, name + ".pbrt"), spp=1)
    s.create_renderer(0, samples_per_pass=1)
    dev = torch.device("cuda", 0)
    if first:
        say("box: %s, torch %s, HIP %s; commit %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip, commit()))
        first = False
    fh = s.first_hit(0)
    n = fh["rays8"].shape[0]
    b = s.bsdf_device(fh["rays8"], fh, fh["lambda4"])
    ls = s.sample_lights_device((s.light_planes(fh, b), fh["planes_i"]), fh["lambda4"], torch.rand((n, 4), device=dev), b["side"].contiguous())
    u4 = torch.rand((n, 4), dtype=torch.float32, device=dev)
    e = s.bsdf_eval_device(b, fh, wi=ls["wi_pdf4"], u4=u4)
    ext = torch.cuda.ExternalStream(hip.wf_stream(s.ctx), device=dev)
    torch.cuda.synchronize()
    types = s.query("material_types")
    say("%s: %d rows, %d with a BSDF, %d valid samples, material_types = 0x%x (%d launches per call)"
        % (name, n, int((b["type"] != 0).sum()), int((e["sample_valid"] == 1).sum()), types, 1 + bin(types).count("1")))
    mk, ev = hip.wf_bsdf_make_device, hip.wf_bsdf_eval_device
    mk.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
    ev.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 12
    margs = [None, fh["rays8"].data_ptr(), fh["planes_f"].data_ptr(), fh["planes_i"].data_ptr(), fh["lambda4"].data_ptr(), None, b["rec"].data_ptr(), b["bsdf4"].data_ptr()]
    eargs = [None, b["rec"].data_ptr(), fh["planes_f"].data_ptr(), fh["planes_i"].data_ptr(), ls["wi_pdf4"].data_ptr(), u4.data_ptr(), e["f4"].data_ptr(), e["pdf4"].data_ptr(),
             e["next_rays8"].data_ptr(), e["sample_f4"].data_ptr(), e["sample_pdf4"].data_ptr(), e["sample_i4"].data_ptr()]
    for run in range(-3, 5):
        t = []
        for f, a in ((mk, margs), (ev, eargs)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext)
            rc = f(s.ctx, n, *a)
            e1.record(ext)
            e1.synchronize()
            assert rc == 0
            t.append(e0.elapsed_time(e1))
        if run >= 0:
            say("  run %d: wf_bsdf_make_device %.4f ms = %.3f ms per million rows; wf_bsdf_eval_device (both halves) %.4f ms = %.3f ms per million rows"
                % (run, t[0], t[0] / n * 1e6, t[1], t[1] / n * 1e6))
    s.close()
say("NOT measured: either call under rocprofv3, the per-type kernels one by one, scenes with a moving camera (k_bsdf_make<t, true>).")
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bsdf_device.txt")
with open(out, "w") as fobj:
    fobj.write("tools/measure_bsdf_device.py — orientation only, no target (DESIGN 4.4)\n" + "\n".join(lines) + "\n")
