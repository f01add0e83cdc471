"""Host logic: .pbrt parsing, flat-table construction (BVH, light BVH, film/sampler/camera), wavefront pass
geometry.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_pkg, read_pfm
from suite_helpers import BvhNode, desc_fields




def test_cornell_tables(wfpt):
    s = wfpt.Scene(path=os.path.join(ROOT, "scenes", "cornell-box.pbrt"))
    assert (s.width, s.height, s.spp) == (400, 400, 16)
    assert s.info.n_triangles == 2 + 5 * 2 + 2 * 10
    assert s.info.n_lights == 2  # one DiffuseAreaLight per emissive triangle (scene.cpp:1290-1340)
    assert s.info.max_depth == 5
    # wavefront/integrator.cpp:227-236
    assert (s.info.max_queue_size, s.info.n_passes, s.info.scanlines_per_pass) == (160000, 1, 400)
    h = desc_fields(wfpt, s)
    assert h.abi_version == 12 and h.n_triangles == 32
    nodes = (BvhNode * h.n_bvh_nodes).from_address(h.bvh_nodes)
    prims = np.ctypeslib.as_array((C.c_int32 * h.n_triangles).from_address(h.bvh_prims))
    assert sorted(prims.tolist()) == list(range(32))  # every triangle exactly once
    # LinearBVHNode invariants (cpu/aggregates.cpp:129-137,505-521): children inside the parent, leaves cover all prims
    covered = 0
    for i in range(h.n_bvh_nodes):
        nd = nodes[i]
        if nd.nprims > 0:
            covered += nd.nprims
            assert nd.nprims <= 4
        else:
            assert nd.axis in (0, 1, 2)
            for c in (i + 1, nd.offset):
                ch = nodes[c]
                for k in range(3):
                    assert ch.bmin[k] >= nd.bmin[k] and ch.bmax[k] <= nd.bmax[k]
    assert covered == 32
    s.close()


def test_1080p_wavefront_geometry(wfpt):
    text = open(os.path.join(ROOT, "scenes", "cornell-box.pbrt")).read().replace(
        '"integer xresolution" [ 400 ] "integer yresolution" [ 400 ]', '"integer xresolution" [ 1920 ] "integer yresolution" [ 1080 ]')
    s = wfpt.Scene(text=text, spp=64)
    assert (s.info.max_queue_size, s.info.n_passes, s.info.scanlines_per_pass) == (1036800, 2, 540)
    assert s.spp == 64
    s.close()


def test_spp_override_and_blobs_scene(wfpt):
    s = wfpt.Scene(path=os.path.join(GOLDEN, "blobs_small.pbrt"), spp=8)
    assert s.spp == 8
    assert s.info.n_triangles == 2 * (2 * 20 * 13) + 2 + 10 + 4
    assert s.info.n_lights == 4
    s.close()


def test_film_to_rgb_matches_getpixelrgb(wfpt):
    """RGBFilm::GetPixelRGB (film.h:258-275): rgb = outputRGBFromSensorRGB * (rgbSum / weightSum)"""
    s = wfpt.Scene(path=os.path.join(GOLDEN, "cornell64.pbrt"))
    film = np.zeros((64, 64, 4))
    film[..., :3] = 2.0
    film[..., 3] = 4.0
    film[0, 0] = 0  # weightSum == 0 -> no division
    rgb = s.film_to_rgb(film)
    assert rgb.shape == (64, 64, 3)
    assert (rgb[0, 0] == 0).all()
    assert np.allclose(rgb[1, 1], rgb[5, 7])
    # sRGB output space: X=Y=Z=0.5 maps to a slightly pink-ish white; luminance row sums to ~0.5
    assert 0.3 < rgb[1, 1].mean() < 0.7
    s.close()


# ---- the BVH and its visit counts against the reference's own statistics ----------------------
def _bvh_stat_scenes(tmp_path):
    import make_scenes
    from conftest import GOLDEN
    out = [(n, os.path.join(GOLDEN, n + ".pbrt"), 4) for n in ("cornell64", "blobs_small", "materials_lights", "alpha_normalmap", "instances", "envmap", "blobs_hlbvh")]
    for m in ("middle", "equal"):   # SplitMethod::Middle / EqualCounts (cpu/aggregates.cpp:239-263)
        v = str(tmp_path / ("blobs_%s.pbrt" % m))
        open(v, "w").write(open(os.path.join(GOLDEN, "blobs_small.pbrt")).read().replace("\nWorldBegin", '\nAccelerator "bvh" "string splitmethod" "%s"\nWorldBegin' % m, 1))
        out.append(("blobs_" + m, v, 4))
    k = str(tmp_path / "killeroo_like_240.pbrt")
    make_scenes.killeroo_like(k, (240, 135), 1)
    out.append(("killeroo_like_240x135_1spp", k, 1))
    s = str(tmp_path / "sanmiguel_like_small.pbrt")
    make_scenes.sanmiguel_like(s, (240, 135), 1, n_meshes=100, n_defs=10, tex_res=64, sky_res=64)
    out.append(("sanmiguel_like_100meshes_240x135_1spp", s, 1))
    return out


def test_bvh_and_visit_counts_equal_the_references(built, tmp_path):
    """tests/golden/bvh_stats.json holds what `pbrt --wavefront --stats` reports for its BVHAggregate (interior / leaf
    nodes, primitives in leaves — over the top-level tree and every instance definition's — and the render's total
    "Nodes visited" and ray-triangle tests, closest-hit + shadow).  The restated SAH builder and the reference-order walk
    must reproduce every number EXACTLY: the N_nodes / N_tris behind bench.py's roofline are the reference's."""
    import json
    from conftest import GOLDEN, run_wf_cpu
    golden = json.load(open(os.path.join(GOLDEN, "bvh_stats.json")))
    keys = ("bvh_interior_nodes", "bvh_leaf_nodes", "bvh_leaf_prims", "bvh_nodes_visited", "tri_tests")
    for name, path, spp in _bvh_stat_scenes(tmp_path):
        j = run_wf_cpu(path, str(tmp_path / "o.pfm"), spp)
        got = {k: j[k] for k in keys}
        want = {k: golden[name][k] for k in keys}
        assert got == want, (name, got, want)


def test_bvh_stats_golden_is_the_live_references(tmp_path):
    """where the shimmed reference build is present (this container): the golden IS what it prints today"""
    import json
    from conftest import GOLDEN, ROOT
    ref = os.path.join(ROOT, "oracle", "_ref", "pbrt_ref")
    if not os.path.exists(ref):
        pytest.skip("oracle/_ref/pbrt_ref not built (no /root/reference)")
    import make_bvh_stats_golden as mk
    golden = json.load(open(os.path.join(GOLDEN, "bvh_stats.json")))
    for name in ("blobs_small", "instances", "blobs_hlbvh"):
        live = mk.ref_stats(os.path.join(GOLDEN, name + ".pbrt"), 4)
        assert all(live[k] == golden[name][k] for k in live), (name, live, golden[name])


def test_scene_table_cache_round_trip(wfpt, tmp_path, monkeypatch):
    """WF_TABLE_CACHE: the second load of a scene comes from the on-disk table file and is the same
    scene — every geometry / BVH array byte for byte, same counts (instances scene: two-level BVH, textures, alpha)."""
    path = os.path.join(GOLDEN, "instances.pbrt")
    monkeypatch.setenv("WF_TABLE_CACHE", str(tmp_path))
    a = wfpt.Scene(path=path, spp=4)
    files = [f for f in os.listdir(tmp_path) if f.endswith(".wftab")]
    assert len(files) == 1
    mtime = os.path.getmtime(os.path.join(tmp_path, files[0]))
    b = wfpt.Scene(path=path, spp=4)   # served by the cache
    assert os.path.getmtime(os.path.join(tmp_path, files[0])) == mtime and len(os.listdir(tmp_path)) == 1
    c = wfpt.Scene(path=path, spp=8)   # another key
    assert len([f for f in os.listdir(tmp_path) if f.endswith(".wftab")]) == 2
    ha, hb = desc_fields(wfpt, a), desc_fields(wfpt, b)
    for f in ("abi_version", "n_vertices", "n_triangles", "n_meshes", "n_bvh_nodes"):
        assert getattr(ha, f) == getattr(hb, f)
    def arr(h, field, n, ctype):
        return np.ctypeslib.as_array((ctype * n).from_address(getattr(h, field))).copy()
    for field, n, ct in (("P", 3 * ha.n_vertices, C.c_float), ("N", 3 * ha.n_vertices, C.c_float), ("UV", 2 * ha.n_vertices, C.c_float),
                         ("tri_indices", 3 * ha.n_triangles, C.c_int32), ("bvh_nodes", 8 * ha.n_bvh_nodes, C.c_uint32)):
        assert (arr(ha, field, n, ct).view(np.uint32) == arr(hb, field, n, ct).view(np.uint32)).all(), field
    for f in ("width", "height", "spp", "max_queue_size", "n_passes", "scanlines_per_pass", "n_triangles", "n_bvh_nodes", "n_lights", "max_depth"):
        assert getattr(a.info, f) == getattr(b.info, f)
    a.close(); b.close(); c.close()


def test_scene_errors_are_returned_not_fatal(wfpt):
    """ErrorExit of the reference = an error RETURN of the C API here: a bad scene raises in the caller (message from
    wfh_last_error) and the process — pytest, bench.py, a host application — lives on."""
    with pytest.raises(wfpt.WfError) as e:
        wfpt.Scene(text='Film "rgb"\nWorldBegin\nShape "bogus"\n', spp=1)
    assert "bogus" in str(e.value) and "not supported" in str(e.value)
    base = open(os.path.join(GOLDEN, "cornell64.pbrt")).read()
    with pytest.raises(wfpt.WfError) as e:   # the whole Cornell box under an animated CTM: its emitter is the reference's ErrorExit (scene.cpp:1485-1488)
        wfpt.Scene(text=base.replace("WorldBegin", "WorldBegin\nActiveTransform EndTime\nTranslate 1 0 0\nActiveTransform All", 1), spp=1)
    assert "Animated area lights are not supported" in str(e.value)
    with pytest.raises(wfpt.WfError) as e:   # CreateAccelerator (cpu/aggregates.cpp:1163-1171)
        wfpt.Scene(text=base.replace("WorldBegin", 'Accelerator "octree"\nWorldBegin', 1), spp=1)
    assert "accelerator type unknown" in str(e.value)
    with pytest.raises(wfpt.WfError) as e:   # wavefront/integrator.cpp:179
        wfpt.Scene(text='Film "rgb"\nWorldBegin\nShape "sphere"\n', spp=1)
    assert "No light sources specified" in str(e.value)
    for bad in ("nan", "inf", "-inf"):       # a vertex that is not finite: an error before any BVH builder indexes a bucket with it (fuzzing, round 3)
        with pytest.raises(wfpt.WfError) as e:
            wfpt.Scene(text='Film "rgb"\nWorldBegin\nLightSource "infinite"\nShape "trianglemesh" "integer indices" [0 1 2] "point3 P" [0 0 0 1 %s 0 0 1 0]\n' % bad, spp=1)
        assert "not finite" in str(e.value)
    with pytest.raises(wfpt.WfError) as e:
        wfpt.Scene(text='Film "rgb"\nWorldBegin\nLightSource "infinite"\nScale 1e30 1e30 1e30\nShape "sphere" "float radius" 1e30\n', spp=1)
    assert "not finite" in str(e.value) or "overflows single precision" in str(e.value)
    with pytest.raises(wfpt.WfError) as e:   # finite, but the SAH costs (count x surface area) are not: no split would ever be chosen
        wfpt.Scene(text='Film "rgb"\nWorldBegin\nLightSource "infinite"\nShape "trianglemesh" "integer indices" [0 1 2 1 2 3] "point3 P" [0 0 0 1 1e38 0 0 1 0 1 1 1]\n', spp=1)
    assert "overflows single precision" in str(e.value)
    s = wfpt.Scene(text='Film "rgb"\nWorldBegin\nLightSource "infinite"\n', spp=1)   # no geometry at all: fine (the reference's empty aggregate)
    assert s.info.n_triangles == 1
    s.close()
    s = wfpt.Scene(text=base, spp=1)   # and the library is still usable
    assert s.info.n_triangles > 0
    s.close()


def test_parallel_bvh_build_is_deterministic(wfpt, tmp_path, monkeypatch):
    """The task-parallel SAH build (a helper thread per large span, the instance definitions built concurrently) writes every leaf's
    primitives at the span's own offset: node and primitive arrays are the sequential build's for any thread count — checked on the
    500 k-triangle two-level stand-in through the table cache (the cache file holds every flat table)."""
    from conftest import bench_small_scene
    path, spp = bench_small_scene("sanmiguel_like_small", tmp_path / "scene")
    blobs = []
    for threads in ("1", "7"):
        d = tmp_path / ("cache" + threads)
        os.makedirs(d)
        monkeypatch.setenv("WF_TABLE_CACHE", str(d))
        monkeypatch.setenv("WF_BUILD_THREADS", threads)
        s = wfpt.Scene(path=path, spp=spp)
        s.close()
        files = [f for f in os.listdir(d) if f.endswith(".wftab")]
        assert len(files) == 1
        blobs.append(np.frombuffer(open(os.path.join(d, files[0]), "rb").read(), dtype=np.uint8))
    assert blobs[0].size > 10 << 20 and blobs[0].size == blobs[1].size
    # (the file starts with the wf_scene_desc struct, whose pointer members are the saving process's addresses — patched on load —:
    # those few bytes differ between any two runs; every table behind it must be identical)
    diff = np.nonzero(blobs[0] != blobs[1])[0]
    assert diff.size < 256 and (diff.size == 0 or diff.max() < 2048), (diff.size, diff[:8], diff[-4:])


def _nanovdb_scene(tmp_path, spp, res=(96, 72)):
    import make_scenes
    d = tmp_path / "nv"
    os.makedirs(d, exist_ok=True)
    path = str(d / "nanovdb_smoke.pbrt")
    make_scenes.nanovdb_smoke(path, res, spp)
    return path


def test_nanovdb_reader_round_trip(wfpt, tmp_path):
    """The own NanoVDB reader (csrc/host/nanovdb_io.cpp; PARITY UNPINNED — third-party format, stubbed in the oracle) against files
    tools/make_nanovdb.py writes in the same restated 32.x layout: uncompressed and ZIP codec, two grids per file, index bounding box,
    map, every voxel value; malformed files are errors, not crashes."""
    import make_nanovdb
    dens, temp = make_nanovdb.smoke_grid()
    org, vox, tr = (-20, -6, -20), 0.05, (0.0, 0.3, 0.0)
    for codec in ("none", "zip"):
        fn = str(tmp_path / ("smoke_%s.nvdb" % codec))
        make_nanovdb.write_nvdb(fn, [("density", dens, org, vox, tr), ("temperature", temp, org, vox, tr)], codec=codec)
        for name, arr in (("density", dens), ("temperature", temp)):
            g = wfpt.read_nanovdb(fn, name)
            zz, yy, xx = np.nonzero(arr)
            assert g["min"] == [int(xx.min()) + org[0], int(yy.min()) + org[1], int(zz.min()) + org[2]]
            assert g["dim"] == [int(xx.max() - xx.min()) + 1, int(yy.max() - yy.min()) + 1, int(zz.max() - zz.min()) + 1]
            sub = arr[zz.min():zz.max() + 1, yy.min():yy.max() + 1, xx.min():xx.max() + 1]
            assert (g["values"] == sub).all()
            assert g["background"] == 0 and np.allclose(g["inv_mat"], [20, 0, 0, 0, 20, 0, 0, 0, 20]) and np.allclose(g["vec"], tr)
        assert wfpt.read_nanovdb(fn, "no-such-grid") is None
    raw = open(fn, "rb").read()
    bad = tmp_path / "bad.nvdb"
    for blob, what in ((b"XXXXXXXX" + raw[8:], "magic"), (raw[:8] + (31 << 21).to_bytes(4, "little") + raw[12:], "version"), (raw[:300], "truncated")):
        bad.write_bytes(blob)
        with pytest.raises(wfpt.WfError):
            wfpt.read_nanovdb(str(bad), "density")


def test_nanovdb_medium_agrees_with_the_pinned_grid_medium(built, tmp_path):
    """An indirect pin for the unpinned NanoVDB medium: the same density field as a `uniformgrid` medium whose cell centres are the
    NanoVDB voxels (bounds = index bounding box widened by half a voxel) interpolates identically (SampledGrid::Lookup at p * res - 0.5
    = SampleFromVoxels at the index coordinates); only the majorant grids differ (64^3 over the world box vs 16^3), i.e. the tracking
    sample sequence, so the two renders agree in expectation: 8x8 block means within 4 % at 256 spp, image means within 1 %.  The
    GridMedium path is bit-identical to the reference (goldens)."""
    import make_nanovdb
    from conftest import run_wf_cpu
    path = _nanovdb_scene(tmp_path, 256, res=(48, 40))
    text = open(path).read().replace('"float Lescale" [ 0.6 ]', '"float Lescale" [ 0 ]')
    open(path, "w").write(text)
    g = load_pkg().read_nanovdb(os.path.join(os.path.dirname(path), "smoke.nvdb"), "density")
    vox, tr = 0.05, (0.0, 0.3, 0.0)
    p0 = [vox * (g["min"][a] - 0.5) + tr[a] for a in range(3)]
    p1 = [vox * (g["min"][a] + g["dim"][a] - 0.5) + tr[a] for a in range(3)]
    dens = " ".join("%.9g" % v for v in g["values"].reshape(-1))
    grid_medium = ('MakeNamedMedium "smoke" "string type" [ "uniformgrid" ] "integer nx" [ %d ] "integer ny" [ %d ] "integer nz" [ %d ] "point3 p0" [ %.9g %.9g %.9g ] '
                   '"point3 p1" [ %.9g %.9g %.9g ] "rgb sigma_a" [ 0.6 0.6 0.6 ] "rgb sigma_s" [ 2.5 2.6 2.8 ] "float scale" [ 4 ] "float g" [ 0.4 ] "float density" [ %s ]\n'
                   % (g["dim"][0], g["dim"][1], g["dim"][2], *p0, *p1, dens))
    lines = text.splitlines(keepends=True)
    i0 = next(i for i, l in enumerate(lines) if l.lstrip().startswith("MakeNamedMedium"))
    grid_path = os.path.join(os.path.dirname(path), "grid_smoke.pbrt")
    open(grid_path, "w").write("".join(lines[:i0]) + grid_medium + "".join(lines[i0 + 2:]))
    a_out, b_out = str(tmp_path / "a.pfm"), str(tmp_path / "b.pfm")
    run_wf_cpu(path, a_out, 256)
    run_wf_cpu(grid_path, b_out, 256)
    a, b = read_pfm(a_out), read_pfm(b_out)
    assert np.isfinite(a).all() and a.shape == b.shape
    assert abs(a.mean() - b.mean()) < 0.01 * b.mean(), (a.mean(), b.mean())
    blocks = lambda im: im.reshape(5, 8, 6, 8, 3).mean(axis=(1, 3, 4))
    rel = np.abs(blocks(a) - blocks(b)) / blocks(b)
    assert rel.max() < 0.04, rel.max()


def test_measured_brdf_files_are_validated(wfpt, tmp_path):
    """The .bsdf tensor reader (csrc/host/measured_io.cpp): the fixtures of tools/make_bsdf.py load into table_data with the layout
    include/wf_abi.h describes; truncated files, a wrong magic, a field that points outside the file, a missing field, an unsupported
    phi_i span and a missing filename are scene errors — never a read outside the file."""
    import shutil
    import struct
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_bsdf
    scene = 'Film "rgb" "integer xresolution" 8 "integer yresolution" 8\nWorldBegin\nLightSource "infinite"\nMaterial "measured" "string filename" "%s"\nShape "sphere"\n'
    good = str(tmp_path / "good.bsdf")
    shutil.copy(os.path.join(GOLDEN, "measured_aniso.bsdf"), good)
    s = wfpt.Scene(text=scene % good, spp=1)
    assert s.info.n_lights == 1
    s.close()
    blob = open(good, "rb").read()

    def refused(data, needle):
        fn = str(tmp_path / "bad.bsdf")
        open(fn, "wb").write(data)
        with pytest.raises(wfpt.WfError) as e:
            wfpt.Scene(text=scene % fn, spp=1)
        assert needle in str(e.value), str(e.value)
    refused(blob[:10], "too small")
    refused(b"tensor_fiel\0" + blob[12:], "invalid header")
    refused(blob[:len(blob) // 2], "Unable to read")
    # the first field's byte offset moved past the end of the file
    name_len = struct.unpack_from("<H", blob, 18)[0]
    at = 18 + 2 + name_len + 2 + 1
    refused(blob[:at] + struct.pack("<Q", len(blob) - 3) + blob[at + 8:], "Unable to read")
    # a shape whose product overflows / exceeds the file
    refused(blob[:at + 8] + struct.pack("<Q", 1 << 62) + blob[at + 16:], "larger than the file")
    refused(blob.replace(b"sigma", b"sigmb", 1), 'no field "sigma"')
    fn = str(tmp_path / "half.bsdf")
    make_bsdf.synth(fn, n_phi=5, n_theta=3, res=4)
    data = bytearray(open(fn, "rb").read())
    # phi_i spanning only half the circle: "reduction 2 (!= 1) not supported" (bxdfs.cpp:931-935)
    import numpy as np
    phi = np.linspace(-np.pi, np.pi, 5).astype(np.float32).tobytes()
    k = bytes(data).find(phi)
    assert k > 0
    data[k:k + 20] = np.linspace(0, np.pi, 5).astype(np.float32).tobytes()
    refused(bytes(data), "reduction 2")
    with pytest.raises(wfpt.WfError) as e:
        wfpt.Scene(text='Film "rgb"\nWorldBegin\nMaterial "measured"\nShape "sphere"\n', spp=1)
    assert "Filename must be provided" in str(e.value)


def test_8bit_image_maps_take_a_quarter_of_the_table(wfpt, tmp_path, monkeypatch):
    """The compact texel store (WF_TEXEL_U8 / WF_TEXEL_HALF, include/wf_abi.h): the table file of the PNG-textured golden scene is less than
    half the file of the all-float store (its maps are 8-bit, a few are 16-bit; the rest of the file is the scene's other tables)."""
    path = os.path.join(GOLDEN, "png_textures.pbrt")
    sizes = {}
    for mode in ("compact", "float"):
        d = tmp_path / mode
        d.mkdir()
        monkeypatch.setenv("WF_TABLE_CACHE", str(d))
        if mode == "float":
            monkeypatch.setenv("WF_TEXELS_FLOAT", "1")
        wfpt.Scene(path=path, spp=1).close()
        files = [f for f in os.listdir(d) if f.endswith(".wftab")]
        assert len(files) == 1
        sizes[mode] = os.path.getsize(d / files[0])
    assert sizes["compact"] < 0.5 * sizes["float"], sizes


def test_reference_parameter_names_are_looked_up():
    """ParameterDictionary::ReportUnused is an ErrorExit in the reference and here: every parameter name the reference's Create() functions
    read on this path must be looked up by this build too, or a valid scene fails with "unused parameter" ("faceIndices").
    tools/param_audit.py compares the names (from /root/reference where present, else the committed list) with the host sources."""
    import subprocess, sys
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(GOLDEN), "..", "tools", "param_audit.py")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout
