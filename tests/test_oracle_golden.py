"""Pins the oracle (the CPU restatement, oracle/wf_cpu + the restated leaf functions) against golden
vectors produced by the REAL reference (tools/make_golden.sh: oracle/_ref/ref_probe and pbrt_ref
--wavefront, built from the unmodified sources under /root/reference)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, WF_PROBE, image_error, read_pfm, run_wf_cpu

LEAF = [("zsobol", 12), ("zsobol2", 8), ("triangle", 5), ("sphtri", 6), ("bxdf", 16), ("scalar", 4), ("instance", 60)]


@pytest.fixture(scope="module")
def probe_out(built, tmp_path_factory):
    out = tmp_path_factory.mktemp("probe")
    subprocess.run([WF_PROBE, GOLDEN, str(out)], check=True)
    return str(out)


@pytest.mark.parametrize("name,width", LEAF)
def test_leaf_functions_bit_exact_vs_reference(probe_out, name, width):
    """ZSobol sampler, watertight ray-triangle test, spherical-triangle sampling + inversion, the five BxDFs
    (f / PDF / Sample_f) and the scalar helpers reproduce the reference's outputs bit for bit."""
    ref = np.fromfile(os.path.join(GOLDEN, name + "_out.bin"), dtype=np.uint32).reshape(-1, width)
    got = np.fromfile(os.path.join(probe_out, name + "_out.bin"), dtype=np.uint32).reshape(-1, width)
    assert ref.shape == got.shape and ref.shape[0] >= 1000
    rf, gf = ref.view(np.float32), got.view(np.float32)
    same = (ref == got) | (np.isnan(rf) & np.isnan(gf))
    assert same.all(), "%d of %d values differ" % ((~same).sum(), same.size)


def test_triangle_golden_covers_hits_misses_edges():
    out = np.fromfile(os.path.join(GOLDEN, "triangle_out.bin"), dtype=np.float32).reshape(-1, 5)
    hits = out[:, 0] > 0
    assert 0.2 < hits.mean() < 0.9
    assert (out[hits, 4] > 0).all()
    b = out[hits, 1:4]
    assert np.allclose(b.sum(axis=1), 1, atol=1e-5)


@pytest.mark.parametrize("scene,spp", [("cornell64", 4), ("cornell400", 16), ("blobs_small", 4), ("materials_lights", 4), ("materials_lights_power", 4), ("media_box", 4), ("rgbgrid_medium", 4), ("tempgrid_medium", 4), ("envmap", 4), ("textures_bump", 4), ("spherical_camera", 4), ("image_textures", 4), ("alpha_normalmap", 4), ("spheres", 4), ("quadrics", 4), ("lights_extra", 4), ("texture_mappings", 4), ("textures_extra", 4), ("textures_deep", 4), ("textures_scale_fold", 4), ("tangents_s", 4), ("arealight_image", 4), ("instances", 4), ("subsurface", 4), ("blobs_hlbvh", 4), ("textures_noise", 4), ("cloud_medium", 4), ("media_instances", 4), ("hair", 4), ("measured", 4), ("bilinear", 4), ("bilinear_lights", 4), ("bilinear_emission", 4), ("instances_quadrics", 4), ("media_preset", 4), ("subsurface_named", 4), ("arealight_alpha", 4), ("png_textures", 4), ("textures_ewa", 4), ("curves", 4), ("realistic_camera", 4), ("realistic_camera_star", 4), ("portal_light", 4), ("portal_uniform", 4), ("loopsubdiv", 4), ("film_whitebalance", 4), ("film_sensor", 4), ("film_sensor_wb", 4), ("displacement", 4), ("plymesh_mixed", 4), ("camera_motion", 4), ("camera_motion_spherical", 4), ("rendercoordsys_camera", 4), ("rendercoordsys_world", 4), ("parser_torture", 4), ("empty_scene", 4), ("quadrics_alpha", 4), ("curves_alpha", 4), ("animated", 4), ("animated_sss", 4), ("animated_tris", 4), ("animated_tris_alpha", 4), ("face_indices", 4), ("goniometric_png", 4), ("matrix_lean", 4), ("matrix_lean_tex", 4),
                                       ("cornell64_independent", 0), ("cornell64_stratified", 0), ("cornell64_paddedsobol", 0), ("cornell64_halton", 0), ("cornell64_sobol", 0), ("cornell64_sobol_owen", 0)])
def test_cpu_checker_image_matches_reference_wavefront(built, tmp_path, scene, spp):
    """Whole path, sample-aligned: oracle/wf_cpu vs the reference's CPU WavefrontPathIntegrator
    (pbrt --wavefront) on the same .pbrt, same seed: BIT-IDENTICAL images — every material (incl. the
    hash-seeded layered BxDFs) and every light type implemented (materials_lights scene), and participating media
    (media_box: homogeneous emissive fog, a rotated grid medium, interface surfaces, glass and metal inside the fog),
    object instancing (instances: two-level BVH, TransformedPrimitive ray / interaction transforms, a mirroring instance)."""
    ref = read_pfm(os.path.join(GOLDEN, scene + "_ref.pfm"))
    out = str(tmp_path / "cpu.pfm")
    run_wf_cpu(os.path.join(GOLDEN, scene + ".pbrt"), out, spp)
    img = read_pfm(out)
    assert img.shape == ref.shape
    assert (img.view(np.uint32) == ref.view(np.uint32)).all(), "fraction identical: %f" % (img == ref).mean()


@pytest.mark.parametrize("name", ["sanmiguel_like_small", "tm_like_small", "cloud_like_small"])
def test_cpu_checker_matches_reference_on_benchmark_standins(built, tmp_path, name):
    """The BENCHMARKED workloads (bench.py: san-miguel-like = 500 k triangles in a two-level BVH with alpha cut-outs, image
    textures, sky + sun + emitters; tm-like = nested dielectric shells at maxdepth 50; cloud-like = a grid medium at
    maxdepth 20), downscaled: the port is bit-identical to `pbrt --wavefront` on them too."""
    from conftest import bench_small_scene
    path, spp = bench_small_scene(name, tmp_path / "scene")
    ref = read_pfm(os.path.join(GOLDEN, name + "_ref.pfm"))
    out = str(tmp_path / "cpu.pfm")
    run_wf_cpu(path, out, spp)
    img = read_pfm(out)
    assert img.shape == ref.shape
    assert (img.view(np.uint32) == ref.view(np.uint32)).all(), "fraction identical: %f" % (img == ref).mean()


def test_spectral_film_matches_reference(built, tmp_path):
    """SpectralFilm (film.h:401-530): uniform wavelength sampling over [lambdamin, lambdamax], the RGB accumulators plus the spectral
    buckets, GetImage's channel layout (R G B S0.<centre>nm ...) — the port's .exr against the one `pbrt --wavefront` wrote (through
    the oracle build's OpenEXR stand-in), every channel bit for bit."""
    from conftest import read_exr_channels
    out = str(tmp_path / "cpu.exr")
    run_wf_cpu(os.path.join(GOLDEN, "spectral_film.pbrt"), out, 4)
    ref, got = read_exr_channels(os.path.join(GOLDEN, "spectral_film_ref.exr")), read_exr_channels(out)
    assert sorted(ref) == sorted(got) and len(ref) == 11
    for k in ref:
        assert (ref[k].view(np.uint32) == got[k].view(np.uint32)).all(), k
    assert ref["S0.555,000nm"].mean() > 0.05


def test_gbuffer_film_matches_reference(built, tmp_path):
    """GBufferFilm (film.h:319-400): the visible surface recorded at the first intersection (surfscatter.cpp:147-180: position, normals,
    dpdx / dpdy, uv, the BSDF's albedo from BxDF::rho with the reference's 16 fixed samples — every material type of the
    materials_lights scene), transformed to camera space and accumulated with the Welford variance estimators; all 25 channels of the
    port's .exr against the reference's, bit for bit."""
    from conftest import read_exr_channels
    out = str(tmp_path / "cpu.exr")
    run_wf_cpu(os.path.join(GOLDEN, "gbuffer_film.pbrt"), out, 4)
    ref, got = read_exr_channels(os.path.join(GOLDEN, "gbuffer_film_ref.exr")), read_exr_channels(out)
    assert sorted(ref) == sorted(got) and len(ref) == 25
    for k in ref:
        assert (ref[k].view(np.uint32) == got[k].view(np.uint32)).all(), k
    assert ref["Albedo.G"].mean() > 0.2 and ref["Variance.R"].max() > 0


def test_mix_material_matches_reference_statistically(built, tmp_path):
    """MixMaterial::ChooseMaterial hashes the two materials' tagged POINTERS (materials.h:292): the reference's own
    choice changes with heap layout, so there is no sample-aligned comparison.  64 spp, 8x8-pixel block means of the
    port vs `pbrt --wavefront` within 3 % (image amount texture, nested mix, constant amount)."""
    ref = read_pfm(os.path.join(GOLDEN, "mix_materials_ref.pfm"))
    out = str(tmp_path / "cpu.pfm")
    run_wf_cpu(os.path.join(GOLDEN, "mix_materials.pbrt"), out, 0)
    img = read_pfm(out)
    def blocks(a):
        return a.reshape(8, 8, 8, 8, 3).mean(axis=(1, 3, 4))
    rel = np.abs(blocks(img) - blocks(ref)) / blocks(ref)
    assert rel.max() < 0.03, rel.max()
    assert abs(img.mean() - ref.mean()) < 3e-3 * ref.mean()


def test_cpu_checker_mean_matches_volpath(built, tmp_path):
    """The physical oracle named by north_star (VolPathIntegrator) is not sample-aligned with the wavefront
    estimator (SURVEY §8c caveat 1): compare converged means, in the spirit of CheckSceneAverage
    (cpu/integrators_test.cpp:50-65, +-2.5 %)."""
    ref = read_pfm(os.path.join(GOLDEN, "cornell64_volpath256.pfm"))
    out = str(tmp_path / "cpu.pfm")
    run_wf_cpu(os.path.join(GOLDEN, "cornell64.pbrt"), out, 64)
    img = read_pfm(out)
    assert abs(img.mean() - ref.mean()) / ref.mean() < 0.025


def test_compact_texel_store_equals_the_float_store(built, tmp_path, monkeypatch):
    """8-bit and half image maps keep their source format in table_data (WF_TEXEL_U8 + the encoding's 256-entry table, WF_TEXEL_HALF: a quarter /
    half of the bytes per texel, what the reference's MIP levels hold) — the png_textures scene (every PNG colour type and depth, sRGB / linear /
    gamma encodings, RGBA alpha, resampled non-power-of-two maps) renders the reference's image with either store."""
    ref = read_pfm(os.path.join(GOLDEN, "png_textures_ref.pfm"))
    for mode in ("compact", "float"):
        if mode == "float":
            monkeypatch.setenv("WF_TEXELS_FLOAT", "1")
        out = str(tmp_path / (mode + ".pfm"))
        run_wf_cpu(os.path.join(GOLDEN, "png_textures.pbrt"), out, 4)
        assert (read_pfm(out).view(np.uint32) == ref.view(np.uint32)).all(), mode


def test_partial_medium_interface_is_deterministic_here(built, tmp_path):
    """A medium-transition surface with an empty inside (see the scene's header): the reference's wavefront path gives a different image on
    every run there (found by tools/diff_fuzz_scenes.py), so there is nothing to match; this build's result must not depend on the run or
    on the thread count."""
    path = os.path.join(GOLDEN, "open_partial_medium_interface.pbrt")
    imgs = []
    for threads in (1, 3, 8, 8):
        out = str(tmp_path / ("cpu%d.pfm" % len(imgs)))
        j = run_wf_cpu(path, out, extra=("--nthreads", str(threads)))
        assert j["indirect_rays"][1:6] == [865, 215, 111, 48, 19]
        imgs.append(read_pfm(out).copy())
    assert all((im.view(np.uint32) == imgs[0].view(np.uint32)).all() for im in imgs)


def test_nan_ray_in_a_grid_medium_ends(built, tmp_path):
    """tests/golden/nan_ray_grid_medium.pbrt (fuzz scene s2400094 reduced): a shadow ray with a NaN direction reaches a grid medium.  The
    reference segfaults there (its DDA iterator turns the NaN grid coordinate into a voxel index, media.h:141-178), so there is no image to
    match; the restated iterator used to do the same on the host and would have walked the grid's memory on the device.  It must end."""
    out = str(tmp_path / "c.pfm")
    j = run_wf_cpu(os.path.join(GOLDEN, "nan_ray_grid_medium.pbrt"), out, None)
    assert j["camera_rays"] > 0 and os.path.exists(out)


# the fuzz corpus of the GPU leg (tests/golden/fuzz, tools/make_fuzz_goldens.py): the CPU port reproduces the reference's renders bit for bit
FUZZ = os.path.join(GOLDEN, "fuzz")


def test_fuzz_corpus_cpu_port(built, tmp_path):
    names = open(os.path.join(FUZZ, "CORPUS.txt")).read().split()
    assert len(names) >= 40
    for name in names:
        out = str(tmp_path / "c.pfm")
        run_wf_cpu(os.path.join(FUZZ, name + ".pbrt"), out, None)
        ref, cpu = read_pfm(os.path.join(FUZZ, name + "_ref.pfm")), read_pfm(out)
        assert ref.shape == cpu.shape and (ref.view(np.uint32) == cpu.view(np.uint32)).all(), name


def test_stale_medium_depth_finding_is_the_reference_defect(built, tmp_path):
    """tests/golden/fuzz/stale_depth_s1300285.pbrt (fuzz seed 13 of round 4, left open there): the reference's
    MediumSampleQueue::Push(RayWorkItem, tMax) — the push of a ray in a medium that missed every surface — never writes the item's
    `depth` (wavefront/workitems.h:466-491; read at wavefront/media.cpp:75,163,331,346), so SampleMediumInteraction sees the depth of
    the slot's previous occupant.  The golden is pbrt_ref --wavefront --nthreads 1 (4 threads give the same image on this scene).
    Sequentially, with the material stage run in the order of the reference's Material::Types (which fixes the order of the next ray
    queue and with it the medium-sample slot of every ray), the emulation reproduces the reference bit for bit; without it exactly the
    two pixels whose paths leave the scene through the fog at depth >= 1 differ."""
    path = os.path.join(FUZZ, "stale_depth_s1300285.pbrt")
    ref = read_pfm(os.path.join(FUZZ, "stale_depth_s1300285_ref.pfm"))
    out = str(tmp_path / "emu.pfm")
    run_wf_cpu(path, out, None, extra=("--emulate-stale-medium-depth",))
    emu = read_pfm(out)
    assert ref.shape == emu.shape and (ref.view(np.uint32) == emu.view(np.uint32)).all()
    out2 = str(tmp_path / "plain.pfm")
    run_wf_cpu(path, out2, None, extra=("--nthreads", "4"))
    plain = read_pfm(out2)
    differ = np.argwhere((ref.view(np.uint32) != plain.view(np.uint32)).any(axis=2)).tolist()
    assert differ == [[0, 19], [5, 25]], differ   # (row, column): the two paths that read a stale depth in the reference


@pytest.mark.parametrize("name", ["sanmiguel_like_small", "cloud_like_small", "killeroo_like_small"])
def test_volpath_in_expectation_cpu_port(built, tmp_path, name):
    """The physical oracle of the north_star — pbrt's CPU VolPathIntegrator (cpu/integrators.cpp:953-1390) — in expectation, on the CPU
    port of the wavefront path (the stage bodies the HIP kernels run; the GPU leg is tests/test_gpu_parity.py::test_volpath_in_expectation
    at 1024 spp).  tests/golden/volpath/<scene>.json = block means of two independent VolPath renders (tools/make_volpath_goldens.py);
    the port renders 256 spp (the GPU 8192, with a block tolerance of 2 %).  Tolerances here: image mean within 2.5 % (the reference's
    CheckSceneAverage, cpu/integrators_test.cpp:50-65), every block of the 8 x 8 grid within 5 % + 8 x the goldens' own disagreement (the goldens
    are 8192-spp renders since round 6: their disagreement is half of what it was, this render's noise is not)."""
    import json
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "tools"))
    from make_volpath_goldens import block_means, scene_for
    gold = json.load(open(os.path.join(GOLDEN, "volpath", name + ".json")))
    sd = tmp_path / "scene"
    sd.mkdir()
    path = scene_for(name, str(sd))
    out = str(tmp_path / "port.pfm")
    run_wf_cpu(path, out, 256, extra=("--nthreads", str(min(8, os.cpu_count() or 1))))
    img = read_pfm(out).astype(np.float64)
    a, b = np.array(gold["blocks_a"]), np.array(gold["blocks_b"])
    ref, g = 0.5 * (a + b), block_means(img, gold["grid"])
    mean_ref = 0.5 * (np.array(gold["mean_a"]) + np.array(gold["mean_b"]))
    assert np.abs(img.mean(axis=(0, 1)) / mean_ref - 1).max() <= 0.025
    noise = np.abs(a - b)
    noise = np.maximum(noise, np.median(noise))
    assert (np.abs(g - ref) <= 0.05 * ref + 8 * noise).all()
