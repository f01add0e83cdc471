"""Stage grids (DESIGN.md 4.7 "Stage grids"): every stage kernel of the render pass is a grid-stride loop, launched on
min(ceil(maxQueueSize / block), R x resident x CUs) workgroups (WF_STAGE_ROUNDS = R; 0: the fixed bound of 2048 workgroups) and, for
tests, on at most WF_STAGE_GRID_CAP workgroups.  The grid may not change a bit of the film, a ray count or an item count.

Four settings, ONE PROCESS EACH (the switches are read at upload; a fresh interpreter per setting, started as a child and never exec'd in
place, each under its own time limit): the fixed bound (WF_STAGE_ROUNDS=0), the default, four rounds, and three workgroups per launch.
After a leg that failed no further leg is started: the legs behind it are skipped with the reason.

What each leg renders:
  * the goldens cornell64 and sanmiguel_like_small at golden resolution;
  * "wall" scenes whose material queues have sizes known by construction: an orthographic camera in front of one large quad of one
    material, maxdepth 1 (one material stage: the camera rays' hits), W x 1 pixels at 1 spp, so the type's queue holds exactly W items.
    W = 200 (below one block), 768 (= cap x 256: the last grid-stride iteration is full) and 769 (= cap x 256 + 1: one item in an
    iteration of its own), for a diffuse, a conductor and a coated-diffuse wall.  A golden's queue sizes follow from its geometry and
    cannot be set by band and spp to a prime like 769, hence these scenes; their sizes are asserted from material_items().
With the cap a golden's launches run up to 4096 x 4 / (3 x 256) = 22 grid-stride iterations per workgroup."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 3
BLOCK = 256
# leg -> the environment it adds (everything else as the suite's)
LEGS = {"bound": {"WF_STAGE_ROUNDS": "0"}, "default": {}, "rounds4": {"WF_STAGE_ROUNDS": "4"}, "cap3": {"WF_STAGE_GRID_CAP": str(CAP)}}
LEG_TIMEOUT_S = 120
WALL_SIZES = (200, CAP * BLOCK, CAP * BLOCK + 1)
WALL_MATERIALS = {"diffuse": ('"diffuse" "rgb reflectance" [ 0.6 0.5 0.4 ]', 1),
                  "conductor": ('"conductor" "float roughness" [ 0.2 ]', 2),
                  "coateddiffuse": ('"coateddiffuse" "rgb reflectance" [ 0.3 0.5 0.4 ] "float roughness" [ 0.1 ]', 6)}   # -> wf_material_type
WALL = """
LookAt 0 0 0  0 0 1  0 1 0
Camera "orthographic" "float screenwindow" [ -1 1 -1 1 ]
Sampler "zsobol" "integer pixelsamples" [ 1 ]
Integrator "volpath" "integer maxdepth" [ 1 ]
Film "rgb" "string filename" [ "wall.pfm" ] "integer xresolution" [ %d ] "integer yresolution" [ 1 ] "bool savefp16" [ false ]
WorldBegin
LightSource "point" "point3 from" [ 0.3 0.4 0 ] "rgb I" [ 5 5 5 ]
Material %s
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -5 -5 2  5 -5 2  5 5 2  -5 5 2 ]
"""


def _child(sm_path, sm_spp, out_dir):
    """one leg: render every scene under the environment the parent set, leave films and counts in out_dir"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import GOLDEN, load_pkg
    wfpt = load_pkg()
    wfpt.libs()
    scenes = [("cornell64", dict(path=os.path.join(GOLDEN, "cornell64.pbrt"), spp=4)),
              ("sanmiguel_like_small", dict(path=sm_path, spp=sm_spp))]
    for mat, (decl, _) in WALL_MATERIALS.items():
        for w in WALL_SIZES:
            scenes.append(("wall_%s_%d" % (mat, w), dict(text=WALL % (w, decl), spp=1)))
    report = {}
    for name, kw in scenes:
        s = wfpt.Scene(**kw)
        s.create_renderer(0)
        s.render()
        np.save(os.path.join(out_dir, name + ".npy"), s.film())
        nsites = s.query("stage_grid_sites")
        report[name] = dict(stats=s.stats(), items=s.material_items(), rounds=s.query("stage_rounds"), cap=s.query("stage_grid_cap"),
                            fallbacks=s.query("stage_grid_fallbacks"),
                            sites=[[s.query("stage_%s_%d" % (k, i)) for k in ("grid", "need", "resident")] for i in range(nsites)])
        s.close()
    with open(os.path.join(out_dir, "report.json"), "w") as f:
        json.dump(report, f)


@pytest.fixture(scope="module")
def legs(built, tmp_path_factory):
    """leg -> dict(report, dir), or dict(failed=reason) / dict(skipped=reason)"""
    from conftest import bench_small_scene
    sm, sm_spp = bench_small_scene("sanmiguel_like_small", tmp_path_factory.mktemp("sm"))
    out, broken = {}, None
    for leg, extra in LEGS.items():
        if broken:
            out[leg] = dict(skipped="not started: leg '%s' failed before it" % broken)
            continue
        d = str(tmp_path_factory.mktemp("leg_" + leg))
        env = {k: v for k, v in os.environ.items() if k not in ("WF_STAGE_ROUNDS", "WF_STAGE_GRID_CAP")}
        env.update(extra)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), sm, str(sm_spp), d], env=env, capture_output=True, text=True, timeout=LEG_TIMEOUT_S)
            why = None if p.returncode == 0 else "exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-2000:])
        except subprocess.TimeoutExpired:
            why = "no result after %d s" % LEG_TIMEOUT_S
        if why:
            out[leg] = dict(failed=why)
            broken = leg
        else:
            out[leg] = dict(report=json.load(open(os.path.join(d, "report.json"))), dir=d)
    return out


def leg_of(legs, name):
    r = legs[name]
    if "skipped" in r:
        pytest.skip(r["skipped"])
    assert "failed" not in r, "leg '%s': %s" % (name, r["failed"])
    return r


def film(leg, scene):
    return np.load(os.path.join(leg["dir"], scene + ".npy"))


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


SCENES = ["cornell64", "sanmiguel_like_small"] + ["wall_%s_%d" % (m, w) for m in WALL_MATERIALS for w in WALL_SIZES]


def test_legs_ran_under_their_switches(legs):
    for name, (rounds, cap) in {"bound": (0, 0), "rounds4": (4, 0), "cap3": (None, CAP), "default": (None, 0)}.items():
        rep = leg_of(legs, name)["report"]
        for scene in SCENES:
            assert rep[scene]["cap"] == cap, (name, scene)
            if rounds is not None:
                assert rep[scene]["rounds"] == rounds, (name, scene)
    default = leg_of(legs, "default")["report"]["cornell64"]["rounds"]
    assert default in (1, 2, 4) and leg_of(legs, "cap3")["report"]["cornell64"]["rounds"] == default


@pytest.mark.parametrize("leg", ["default", "rounds4", "cap3"])
def test_films_and_counts_do_not_depend_on_the_grid(legs, leg):
    base, other = leg_of(legs, "bound"), leg_of(legs, leg)
    for scene in SCENES:
        a, b = film(base, scene), film(other, scene)
        assert np.isfinite(a).all() and a[..., :3].mean() > 0, scene
        assert same_bits(a, b), (leg, scene, int((a.view(np.uint64) != b.view(np.uint64)).sum()))
        assert other["report"][scene]["stats"] == base["report"][scene]["stats"], (leg, scene)   # camera rays, indirect and shadow rays per depth
        assert other["report"][scene]["items"] == base["report"][scene]["items"], (leg, scene)


def test_serial_film_is_the_golden(legs, wfpt):
    """(the leg on the fixed bound against the reference's own render, so that the four equal films are the right one)"""
    from conftest import GOLDEN, read_pfm
    base = leg_of(legs, "bound")
    s = wfpt.Scene(path=os.path.join(GOLDEN, "cornell64.pbrt"), spp=4)
    try:
        img = s.film_to_rgb(film(base, "cornell64"))
    finally:
        s.close()
    ref = read_pfm(os.path.join(GOLDEN, "cornell64_ref.pfm"))
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()


@pytest.mark.parametrize("leg", list(LEGS))
def test_wall_queues_have_the_boundary_sizes(legs, leg):
    """below one block, exactly cap x 256, cap x 256 + 1: read back from the material stage's item counts, not assumed"""
    rep = leg_of(legs, leg)["report"]
    assert WALL_SIZES == (200, 768, 769) and WALL_SIZES[0] < BLOCK
    for mat, (_, mtype) in WALL_MATERIALS.items():
        for w in WALL_SIZES:
            r = rep["wall_%s_%d" % (mat, w)]
            assert r["stats"]["camera_rays"] == w
            assert {int(k): v for k, v in r["items"].items() if k != "medium_sample" and v} == {mtype: w}, (mat, w, r["items"])


def test_capped_grids_iterate(legs):
    """under the cap every launch site in use runs three workgroups wherever its queue holds more than two blocks: the goldens' sites
    take several grid-stride iterations, the walls' material kernels one full, one full + one item, or a partial one"""
    rep = leg_of(legs, "cap3")["report"]
    for scene in SCENES:
        used = [(g, need) for g, need, _ in rep[scene]["sites"] if g >= 0]
        assert used, scene
        for g, need in used:
            assert g == min(need, CAP), (scene, g, need)
    for scene in ("cornell64", "sanmiguel_like_small"):
        assert max(need for g, need, _ in rep[scene]["sites"] if g >= 0) >= 4 * CAP, scene


def test_default_grids_are_whole_rounds(legs):
    rep = leg_of(legs, "default")["report"]
    for scene in SCENES:
        assert rep[scene]["fallbacks"] == 0, scene
        rounds = rep[scene]["rounds"]
        used = [s for s in rep[scene]["sites"] if s[0] >= 0]
        assert len(used) >= 6, scene   # sampler prefixes or not, camera rays, ray samples, route hits, emitters, one shade and one NEE kernel
        for g, need, resident in used:
            assert resident > 0 and resident % 256 == 0, (scene, resident)   # whole workgroups per CU on the 256 CUs of an MI355X
            assert g == need or (g % resident == 0 and g == rounds * resident and g < need), (scene, g, need, resident)
    # ... and on the fixed bound nothing was asked: no site reports a resident count, none counts as a fallback
    bound = leg_of(legs, "bound")["report"]["cornell64"]
    assert bound["fallbacks"] == 0 and all(s[2] <= 0 for s in bound["sites"])


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]), sys.argv[3])
