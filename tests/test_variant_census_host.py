"""The census of the material-kernel matrix on the HOST (no GPU): every case of tests/variant_matrix_cases.py plans the cells it claims
(Scene.plan under the case's environment), the claimed cells cover all 40 k_mat_shade<type, variant> and all 20 k_mat_nee<type, rare>
kernels, every claimed type's queue holds items (the CPU port's "material_items"), and the two matrix scenes meet the item floor.
The table — cell, then the cases that cover it — is profiles/variant_census.txt."""
import os

import pytest

from conftest import GOLDEN, ROOT, run_wf_cpu
from variant_matrix_cases import BLOCK, CASES, ITEM_FLOOR, MATRIX_SCENES, NEE_CELLS, SHADE_CELLS, SWITCHES, TYPES, nee_cells, shade_cells

CENSUS = os.path.join(ROOT, "profiles", "variant_census.txt")
TYPE_NAMES = {1: "diffuse", 2: "conductor", 3: "dielectric", 4: "thin dielectric", 5: "diffuse transmission", 6: "coated diffuse", 7: "coated conductor", 8: "subsurface",
              9: "hair", 10: "measured"}


@pytest.fixture(scope="module")
def port_items(built, tmp_path_factory):
    """scene -> the port's JSON line of its 4 spp render, made once per scene"""
    cache = {}

    def get(scene):
        if scene not in cache:
            cache[scene] = run_wf_cpu(os.path.join(GOLDEN, scene + ".pbrt"), str(tmp_path_factory.mktemp("census") / (scene + ".pfm")), 4)
        return cache[scene]
    return get


def test_case_ids_are_unique():
    assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_plans_the_cells_it_claims(wfpt, monkeypatch, port_items, case):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    s = wfpt.Scene(path=os.path.join(GOLDEN, case.scene + ".pbrt"), spp=4)
    try:
        planned = {t: s.plan("shade_variant_%d" % t) for t in case.shade}
        rare = s.plan("rare_lights")
    finally:
        s.close()
    assert planned == case.shade, case.id
    assert rare == case.rare, case.id
    # a claimed kernel must have work: the type's queue holds items in the port's render of the scene, and is evaluated
    items = port_items(case.scene)
    assert all(items["material_items_evaluated"][t] > 0 for t in case.shade), (case.id, items["material_items_evaluated"])
    # ... and a type the case does not name has none (the table names every kernel a case runs)
    assert all((items["material_items"][t] > 0) == (t in case.shade) for t in TYPES), (case.id, items["material_items"])


def test_cases_cover_every_material_kernel():
    shade, nee = set(), set()
    for c in CASES:
        shade |= shade_cells(c)
        nee |= nee_cells(c)
    assert shade == SHADE_CELLS, sorted(SHADE_CELLS - shade)
    assert nee == NEE_CELLS, sorted(NEE_CELLS - nee)
    # the matrix scenes alone cover them, on triangles
    shade_m, nee_m = set(), set()
    for c in CASES:
        if c.scene in MATRIX_SCENES:
            shade_m |= shade_cells(c)
            nee_m |= nee_cells(c)
    assert shade_m == SHADE_CELLS and nee_m == NEE_CELLS


@pytest.mark.parametrize("scene", MATRIX_SCENES)
def test_matrix_scene_meets_the_item_floor(port_items, scene):
    """every one of the ten types gets at least two full workgroups of items that the material stage evaluates, and at least one type's count
    leaves a ragged last block"""
    j = port_items(scene)
    queued, evaluated = j["material_items"], j["material_items_evaluated"]
    assert len(queued) == len(evaluated) == 11 and queued[0] == 0   # (interface surfaces have no queue)
    print(scene, "queued", queued, "evaluated", evaluated)
    assert all(evaluated[t] >= ITEM_FLOOR for t in TYPES), evaluated
    assert all(queued[t] >= evaluated[t] for t in TYPES)   # (the last depth's queue is filled and not evaluated)
    assert any(evaluated[t] % BLOCK != 0 for t in TYPES), evaluated


def _census_text(port_items):
    lines = ["# The material-kernel census: each of the 60 separately compiled material kernels, then the cases of tests/variant_matrix_cases.py that run it",
             "# (written by tests/test_variant_census_host.py; a case is <scene>-<switches, without their WF_ prefix>).",
             "# Items per type in the two matrix scenes (the CPU port, 4 spp; queued / evaluated by the material stage):"]
    for scene in MATRIX_SCENES:
        j = port_items(scene)
        lines.append("#   %s: %s" % (scene, ", ".join("%s %d / %d" % (TYPE_NAMES[t], j["material_items"][t], j["material_items_evaluated"][t]) for t in TYPES)))
    for t in TYPES:
        for v in range(4):
            lines.append("k_mat_shade<%s, %d>: %s" % (TYPE_NAMES[t], v, " ".join(c.id for c in CASES if (t, v) in shade_cells(c))))
    for t in TYPES:
        for r in range(2):
            lines.append("k_mat_nee<%s, %s>: %s" % (TYPE_NAMES[t], "true" if r else "false", " ".join(c.id for c in CASES if (t, r) in nee_cells(c))))
    return "\n".join(lines) + "\n"


def test_census_table_is_written_and_committed(port_items):
    """profiles/variant_census.txt is this table; a run that finds it out of date rewrites it and fails, so that the new one is committed"""
    text = _census_text(port_items)
    old = open(CENSUS).read() if os.path.exists(CENSUS) else None
    if old != text:
        try:
            with open(CENSUS, "w") as f:
                f.write(text)
        except OSError:
            pass
    assert old == text, "profiles/variant_census.txt was out of date (rewritten where possible): commit it"
