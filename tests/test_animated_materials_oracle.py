"""Interface, mix and subsurface materials on AnimatedPrimitives, and lights under an animated CTM (CPU checker, no GPU).

The consumers of a hit before the material stage (the interface skip, the MixMaterial resolve, the medium stage's interface continuation)
rebuild the hit's interaction at the ray's time; the scene builder admits these materials on moving shapes and instances; a LightSource
under an animated CTM takes its start transformation with the reference's warning (BasicScene::AddLight, scene.cpp:1007-1009)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, WF_CPU, read_pfm, run_wf_cpu

SCENES = ["animated_interface", "animated_interface_sphere", "animated_mix", "animated_subsurface", "animated_light"]
LIGHT_WARNING = "Animated lights aren't supported. Using the start transform."


@pytest.mark.parametrize("scene", SCENES)
def test_cpu_checker_renders_animated_materials_like_the_reference(built, tmp_path, scene):
    """oracle/wf_cpu against pbrt_ref --wavefront (tests/golden/<scene>_ref.pfm): bit-identical"""
    ref = read_pfm(os.path.join(GOLDEN, scene + "_ref.pfm"))
    out = str(tmp_path / "cpu.pfm")
    run_wf_cpu(os.path.join(GOLDEN, scene + ".pbrt"), out, 4)
    img = read_pfm(out)
    assert img.shape == ref.shape
    assert (img.view(np.uint32) == ref.view(np.uint32)).all(), "fraction identical: %f" % (img == ref).mean()


@pytest.mark.parametrize("scene", SCENES[:4])
def test_scene_loader_admits_the_materials_on_moving_primitives(wfpt, scene):
    """the loader builds the scenes (it refused every one of them before) and they do hold animated primitives"""
    s = wfpt.Scene(path=os.path.join(GOLDEN, scene + ".pbrt"), spp=4)
    text = open(os.path.join(GOLDEN, scene + ".pbrt")).read()
    assert "ActiveTransform EndTime" in text
    assert s.width > 0 and s.height > 0


def _static_twin(text):
    """the scene with every animated CTM replaced by its start transformation: `ActiveTransform StartTime` lines dropped, and each
    `ActiveTransform EndTime ... ActiveTransform All` section (which moves the end transformation only) removed"""
    out, skipping = [], False
    for line in text.splitlines():
        key = line.strip()
        if key == "ActiveTransform StartTime":
            continue
        if key == "ActiveTransform EndTime":
            skipping = True
            continue
        if key == "ActiveTransform All":
            skipping = False
            continue
        if not skipping:
            out.append(line)
    return "\n".join(out) + "\n"


def test_animated_light_warns_and_uses_the_start_transform(built, tmp_path):
    path = os.path.join(GOLDEN, "animated_light.pbrt")
    text = open(path).read()
    static = _static_twin(text)
    assert "ActiveTransform" not in static and static.count("LightSource") == 3
    static_path = tmp_path / "animated_light_static.pbrt"
    static_path.write_text(static)
    out_a, out_s = str(tmp_path / "a.pfm"), str(tmp_path / "s.pfm")
    p = subprocess.run([WF_CPU, "--spp", "4", "--outfile", out_a, path], check=True, capture_output=True, text=True)
    warnings = [l for l in p.stderr.splitlines() if LIGHT_WARNING in l]
    assert len(warnings) == 3, p.stderr
    assert all(l.startswith("Warning: ") and "animated_light.pbrt" in l for l in warnings), warnings
    p = subprocess.run([WF_CPU, "--spp", "4", "--outfile", out_s, str(static_path)], check=True, capture_output=True, text=True)
    assert LIGHT_WARNING not in p.stderr
    a, s = read_pfm(out_a), read_pfm(out_s)
    assert a.mean() > 0.01
    assert (a.view(np.uint32) == s.view(np.uint32)).all()
