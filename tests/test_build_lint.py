"""Build-time lint for the toolchain defect of DESIGN.md 4.6 (CPU suite: it only disassembles the built objects).

Every kernel of the shipped build keeps the VGPRs that carry its spilled SGPRs in registers; the three wrong-code incidents of rounds
3-4 were all builds in which such a carrier register was itself spilled to scratch (tools/check_spill_carriers.py).  A source change that
pushes a kernel over that edge fails here, before it reaches the GPU."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_kernel_spills_an_sgpr_spill_carrier():
    build = os.path.join(ROOT, "pbrt-v4_amd", "_build")
    assert os.path.exists(os.path.join(build, "wf_backend.o")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_spill_carriers.py"), build], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "0 of them also spill a carrier register" in p.stdout


def test_scratch_allocations_cover_call_chains_and_lane_saves_are_whole_wave():
    """tools/stack_audit.py: no kernel's deepest direct call chain needs more scratch than the kernel is allocated, and no kernel can reach a
    recursive device function (which would make it a dynamically-sized-stack kernel: Log2IntF was one until round 5).
    tools/carrier_audit.py: every save / reload of a VGPR whose lanes hold spilled SGPRs is done with all lanes enabled."""
    build = os.path.join(ROOT, "pbrt-v4_amd", "_build")
    assert os.path.exists(os.path.join(build, "wf_backend.o")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", t)] + a, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for t, a in (("stack_audit.py", [build]), ("carrier_audit.py", [build, "-q"]))]
    outs = [p.communicate(timeout=1200)[0] for p in procs]
    assert procs[0].returncode == 0 and ": 0 whose deepest direct call chain needs more scratch" in outs[0], outs[0][-3000:]
    assert "recursion" not in outs[0], outs[0][-3000:]
    assert procs[1].returncode == 0 and "\n0 save / reload of live lanes under a partial EXEC" in outs[1], outs[1][-3000:]


def _device_functions(obj, tmp_path):
    """The names of the gfx950 device functions (kernels and out-of-line device functions) of an object file: tools/isa_dump.py"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_dump
    finally:
        sys.path.pop(0)
    out = tmp_path / os.path.basename(obj)
    isa_dump.main(obj, str(out))
    return sorted(f[:-2] for f in os.listdir(out))


def test_units_behind_wf_ctx_keep_their_boundaries(tmp_path):
    """The four units behind csrc/hip/wf_ctx.h: the boundary and read-back calls hold no device code, so an edit to them leaves every
    code object as the GPU suite last verified it; the three probe kernels of the tests have a code object of their own; and the render's
    code object carries none of them.  (k_subsurface_probe, the render's SampleSubsurface probe-ray stage, is no test probe and stays.)"""
    build = os.path.join(ROOT, "pbrt-v4_amd", "_build")
    for unit in ("wf_backend", "wf_boundary", "wf_results", "wf_probe"):
        assert os.path.exists(os.path.join(build, unit + ".o")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    names = {unit: _device_functions(os.path.join(build, unit + ".o"), tmp_path) for unit in ("wf_backend", "wf_boundary", "wf_results", "wf_probe")}
    assert names["wf_boundary"] == [] and names["wf_results"] == [], (names["wf_boundary"], names["wf_results"])
    probes = ("k_sampler_probe", "k_libm_probe", "k_kat_probe")
    kernels = [n for n in names["wf_probe"] if any(p in n for p in probes)]
    assert len(kernels) == 3 and all(sum(p in n for n in kernels) == 1 for p in probes), names["wf_probe"]
    # whatever else the unit holds is an out-of-line device function the probes reach: no kernel (k_*)
    assert not [n for n in names["wf_probe"] if n not in kernels and re.match(r"(_Z\d+)?k_", n)], names["wf_probe"]
    assert len(names["wf_backend"]) > 100, len(names["wf_backend"])   # (the dump found the render's kernels at all)
    assert not [n for n in names["wf_backend"] if "_probe" in n and "k_subsurface_probe" not in n], [n for n in names["wf_backend"] if "_probe" in n]
