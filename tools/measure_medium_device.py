#!/usr/bin/env python3
"""tools/measure_medium_device.py [OUT [COMMIT]] — wf_medium_sample_device and wf_phase_device on one GPU, for orientation:
nobody has measured these kernels and nothing is a target.  Three scenes: tests/golden/cloud_medium.pbrt, tests/golden/media_box.pbrt and
the cloud-like generator's small scene (tools/make_scenes.py bench_small("cloud_like_small"), generated into a temporary directory).
Per scene: 2^18 seeded rows — origins inside the scene's bounds, unit-spectra rays to their closest hits, the scene's media in turn —
three warm-up rounds, then five timed rounds of each call between two events on the context's stream; and beside them, in the same
process, the render's own "Sample medium interaction" kernel (k_medium_sample, unchanged by this unit) from wf_kernel_time_ms over one
sample of the image, divided by the items its queue held: five rounds, to show its spread.  The render's items are its paths' rays, the
call's rows are seeded ones: the two columns are beside each other for orientation, not as a comparison of equal work — the tentative
collisions per row are printed for the call; the render does not count its own.  Writes the lines to OUT (default
profiles/medium_device.txt) with the GPU's name and the commit the tree is at."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import conftest
import make_scenes

wfpt = conftest.load_pkg()
host, hip = wfpt.libs()
lines = []
N = 1 << 18


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


tmp = tempfile.mkdtemp(prefix="measure_medium_")
scenes = [("cloud_medium", os.path.join(conftest.GOLDEN, "cloud_medium.pbrt")), ("media_box", os.path.join(conftest.GOLDEN, "media_box.pbrt")),
          ("cloud_like_small", make_scenes.bench_small("cloud_like_small", tmp))]
first = True
for name, path in scenes:
    s = wfpt.Scene(path=path, spp=1)
    s.create_renderer(0, samples_per_pass=1)
    dev = torch.device("cuda", 0)
    if first:
        say("box: %s, torch %s, HIP %s; commit %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip, commit()))
        first = False
    media = s.query("media")
    rng = np.random.RandomState(1)
    lo, hi = s.bounds()
    o = rng.uniform(lo, hi, size=(N, 3)).astype(np.float32)
    d = rng.normal(size=(N, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = torch.from_numpy(np.concatenate([o, d, np.full((N, 1), np.inf, np.float32), np.zeros((N, 1), np.float32)], axis=1).astype(np.float32)).to(dev)
    hits = s.trace_device(rays)
    t = hits[:, 1].contiguous().view(torch.float32)
    rays[:, 6] = torch.where(hits[:, 0] >= 0, t, torch.full_like(t, float("inf")))
    medium = torch.from_numpy((np.arange(N) % media).astype(np.int32)).to(dev)
    lam = torch.from_numpy(np.sort(rng.uniform(380, 780, size=(N, 4)), axis=1).astype(np.float32)).to(dev)
    one = torch.ones((N, 4), dtype=torch.float32, device=dev)
    ev = s.medium_sample_device(rays, medium, lam, one, one.clone(), one.clone())
    u4 = torch.rand((N, 4), dtype=torch.float32, device=dev)
    ph = s.phase_device(rays, ev["p_g4"], wi=u4, u4=u4)
    ext = torch.cuda.ExternalStream(hip.wf_stream(s.ctx), device=dev)
    torch.cuda.synchronize()
    kinds = torch.bincount(ev["kind"], minlength=4).tolist()
    steps = int(ev["steps"].sum())
    say("%s: %d rows, kinds 0 - 3 = %s, %d tentative collisions (%.2f per row, most %d), medium_sample_variant = %d, %d media"
        % (name, N, kinds, steps, steps / N, int(ev["steps"].max()), s.query("medium_sample_variant"), media))
    ms_, pf = hip.wf_medium_sample_device, hip.wf_phase_device
    ms_.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 14
    pf.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
    margs = [None, rays.data_ptr(), medium.data_ptr(), lam.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), None, ev["event4"].data_ptr(), ev["p_g4"].data_ptr(),
             ev["beta"].data_ptr(), ev["r_u"].data_ptr(), ev["r_l"].data_ptr(), ev["L"].data_ptr()]
    pargs = [None, rays.data_ptr(), ev["p_g4"].data_ptr(), u4.data_ptr(), u4.data_ptr(), ph["p_pdf4"].data_ptr(), ph["sample4"].data_ptr(), ph["next_rays8"].data_ptr()]
    for run in range(-3, 5):
        tms = []
        for f, a in ((ms_, margs), (pf, pargs)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext)
            rc = f(s.ctx, N, *a)
            e1.record(ext)
            e1.synchronize()
            assert rc == 0
            tms.append(e0.elapsed_time(e1))
        if run >= 0:
            say("  run %d: wf_medium_sample_device %.4f ms = %.3f ms per million rows; wf_phase_device (both halves) %.4f ms = %.3f ms per million rows"
                % (run, tms[0], tms[0] / N * 1e6, tms[1], tms[1] / N * 1e6))
    for run in range(5):
        s.enable_profile(True)
        s.clear_film()
        s.profile_report()   # (forgets the launches recorded so far)
        s.render(0, 1)
        ms, launches = C.c_double(0), C.c_int(0)
        wfpt._check(hip.wf_kernel_time_ms(s.ctx, b"Sample medium interaction", C.byref(ms), C.byref(launches)), "wf_kernel_time_ms")
        items = s.material_items()["medium_sample"]
        s.enable_profile(False)
        say("  render %d: \"Sample medium interaction\" %.4f ms in %d launches over %d items = %.3f ms per million items"
            % (run, ms.value, launches.value, items, ms.value / max(items, 1) * 1e6))
    s.close()
say("NOT measured: either call under rocprofv3, other launch bounds than the render's (2 waves, 3 for the lean kernel), n_device, the kernels on the benchmark's 512^3 cloud.")
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "medium_device.txt")
with open(out, "w") as fobj:
    fobj.write("tools/measure_medium_device.py — orientation only, no target (DESIGN 4.4)\n" + "\n".join(lines) + "\n")
