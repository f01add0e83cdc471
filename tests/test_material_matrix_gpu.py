"""Every material kernel variant on the device.  The material stage is 60 separately compiled kernels — k_mat_shade<type, variant> for
ten types and four variants, k_mat_nee<type, rare> for ten types and two — of which a scene's plan picks one shade and one NEE kernel
per type; the variants are meant to agree bit for bit.  Each case of tests/variant_matrix_cases.py (scene, environment switches, the
cells it claims) is rendered here: the uploaded scene must run the claimed kernels, the image must be bit-identical with the scene's
committed reference render, the ray counts of every stage and depth and the per-type item counts of the material queues must equal the
CPU port's, and no traversal stack may overflow.  tests/test_variant_census_host.py shows on the host that the cases cover all 60.

(No torch in this module: DESIGN 8, renderer creation after torch initialises.)"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, read_pfm, run_wf_cpu
from suite_helpers import assert_image_parity
from variant_matrix_cases import CASES, SWITCHES, TYPES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def port(built, tmp_path_factory):
    """scene -> (the port's image, its JSON line) of the 4 spp render, made once per scene and shared by the scene's cases"""
    cache = {}

    def get(scene):
        if scene not in cache:
            out = str(tmp_path_factory.mktemp("port") / (scene + ".pfm"))
            j = run_wf_cpu(os.path.join(GOLDEN, scene + ".pbrt"), out, 4)
            img = read_pfm(out)
            img.setflags(write=False)
            cache[scene] = (img, j)
        return cache[scene]
    return get


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_material_kernel_variants_bit_identical(wfpt, monkeypatch, port, case):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    s = wfpt.Scene(path=os.path.join(GOLDEN, case.scene + ".pbrt"), spp=4)
    try:
        s.create_renderer(0)
        # the kernels the case is responsible for are the ones the uploaded scene runs
        assert {t: s.query("shade_variant_%d" % t) for t in case.shade} == case.shade, case.id
        assert s.query("rare_lights") == case.rare, case.id
        s.debug_counters(reset=True)
        s.clear_film()
        s.render(0, 4, 1)
        img = s.image()
        dbg = s.debug_counters(reset=True)
        st = s.stats()
        items = s.material_items()
    finally:
        s.close()
    cpu, j = port(case.scene)
    ref = read_pfm(os.path.join(GOLDEN, case.scene + "_ref.pfm"))   # the reference's own CPU wavefront render
    assert (cpu.view(np.uint32) == ref.view(np.uint32)).all()       # the port IS the reference, bit for bit
    print(case.id, "items", [items[t] for t in range(11)], "port", j["material_items"])
    assert dbg["overflow"] == 0, dbg
    # integer work: identical ray counts stage by stage and depth by depth
    assert st["camera_rays"] == j["camera_rays"]
    n = min(len(st["indirect_rays"]), len(j["indirect_rays"]))
    assert st["indirect_rays"][:n] == j["indirect_rays"][:n] and not any(st["indirect_rays"][n:]) and not any(j["indirect_rays"][n:])
    n = min(len(st["shadow_rays"]), len(j["shadow_rays"]))
    assert st["shadow_rays"][:n] == j["shadow_rays"][:n] and not any(st["shadow_rays"][n:]) and not any(j["shadow_rays"][n:])
    # every claimed kernel saw the items it should have: the queues' item counts, type by type
    assert [items[t] for t in range(11)] == j["material_items"], case.id
    assert all(items[t] > 0 for t in case.shade) and all((items[t] > 0) == (t in case.shade) for t in TYPES), (case.id, items)
    assert_image_parity(case.scene, img, ref)   # bit-identical: NOT_BIT_IDENTICAL is empty
