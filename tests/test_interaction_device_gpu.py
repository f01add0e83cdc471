"""The closed loop of the device-buffer boundary on the MI355X, against what the REFERENCE's queues hold (tests/golden/intr_<name>/,
tools/make_interaction_goldens.py): Scene.camera_rays_device gives the rays of the reference's ray queue after "Generate camera rays",
and those rays through Scene.trace_device and Scene.interactions_device give the fields of its MaterialEvalWorkItems after
IntersectClosest — bit for bit, pixel by pixel, on seven scenes that between them reach every variant of k_hit_interaction
(wf_boundary_intr.hip).  Then the shapes at which the kernel itself can go wrong: sizes around the wave and the block, misses between
hits, a caller's buffer with a guard band, the ray's time reaching both transformations of a nested placement, and the stream ordering
of the two calls between torch ops."""
import ctypes as C
import os

import numpy as np
import pytest

from boundary_helpers import _f32_bits as _bits, _np
from conftest import GOLDEN

import make_interaction_goldens as goldens

pytestmark = pytest.mark.gpu

W = goldens.WIDTH
# mat_items.bin: type tag, pixelIndex, then these fields (oracle/ref_build/ref_stages.cpp dumpMat)
FIELDS = (("pi_lo", 2, 3), ("pi_hi", 5, 3), ("n", 8, 3), ("ns", 11, 3), ("dpdus", 14, 3), ("wo", 17, 3), ("uv", 20, 2), ("dpdu", 22, 3), ("dpdv", 25, 3))


class Mesh(C.Structure):   # wf_mesh
    _fields_ = [(n, C.c_int32) for n in ("first_tri", "ntris", "first_vertex", "nverts", "flags", "material", "first_light", "alpha_tex",
                                         "medium_inside", "medium_outside", "first_s", "pad")]


class DescHead(C.Structure):   # the leading members of wf_scene_desc
    _fields_ = [("abi_version", C.c_int32), ("n_vertices", C.c_int32), ("n_triangles", C.c_int32), ("n_meshes", C.c_int32), ("n_bvh_nodes", C.c_int32),
                ("P", C.c_void_p), ("N", C.c_void_p), ("UV", C.c_void_p), ("tri_indices", C.c_void_p), ("tri_mesh", C.c_void_p), ("meshes", C.c_void_p),
                ("bvh_nodes", C.c_void_p), ("bvh_prims", C.c_void_p), ("scene_bounds", C.c_float * 6),
                ("n_spectra", C.c_int32), ("n_spectrum_floats", C.c_int32), ("n_textures", C.c_int32), ("n_materials", C.c_int32),
                ("spectra", C.c_void_p), ("spectrum_data", C.c_void_p), ("textures", C.c_void_p), ("materials", C.c_void_p)]


MATERIAL_WORDS = 25   # sizeof(wf_material) / 4; word 0 = type


class Case:
    """One fixture scene on the device: its camera rays, their hits and the hits' interactions, computed once and left unchanged."""

    def __init__(self, wfpt, name):
        import torch
        self.name = name
        self.scene = wfpt.Scene(path=os.path.join(GOLDEN, "intr_%s.pbrt" % name), spp=4)
        self.scene.create_renderer(0)
        self.rays, self.pixel_xy, self.lambda4 = self.scene.camera_rays_device(0)
        self.hits = self.scene.trace_device(self.rays)
        self.intr = self.scene.interactions_device(self.rays, self.hits)
        torch.cuda.synchronize()
        self.n = self.rays.shape[0]
        self.planes_f = _np(self.intr["planes_f"]).copy()
        self.planes_i = _np(self.intr["planes_i"]).copy()
        self.np = {k: _np(v).copy() for k, v in self.intr.items()}
        self.rec = wfpt.hit_records(self.hits)
        xy = _np(self.pixel_xy)
        self.pixel = xy[:, 1].astype(np.int64) * W + xy[:, 0]      # the reference's pixelIndex: row by row from the film's first scanline
        self.row_of = {int(p): i for i, p in enumerate(self.pixel)}
        d = os.path.join(GOLDEN, "intr_%s" % name)
        self.ref_rays = np.fromfile(os.path.join(d, "camera_rays.bin"), dtype=np.float32).reshape(-1, 8)
        self.ref_items = np.fromfile(os.path.join(d, "mat_items.bin"), dtype=np.float32).reshape(-1, 28)
        # the scene's tables, as the host library built them
        host, _ = wfpt.libs()
        h = DescHead.from_address(host.wfh_scene_desc(self.scene.h))
        self.meshes = (Mesh * h.n_meshes).from_address(h.meshes)
        self.material_type = np.ctypeslib.as_array((C.c_int32 * (MATERIAL_WORDS * h.n_materials)).from_address(h.materials)).reshape(-1, MATERIAL_WORDS)[:, 0].copy()
        self.tri_mesh = h.tri_mesh

    def mesh_of(self, prim):
        return C.c_int32.from_address(self.tri_mesh + 4 * int(prim)).value

    def item_rows(self):
        """(rows of ours, records of the reference) for every pixel that has a material record; a pixel without one is skipped"""
        rows = np.array([self.row_of[int(p)] for p in self.ref_items[:, 1]], dtype=np.int64)
        return rows, self.ref_items


@pytest.fixture(scope="module")
def case(request, wfpt):
    """the fixture scene named by the test's (indirect) parameter; pytest runs the tests of one scene together, so one renderer lives at a time"""
    c = Case(wfpt, request.param)
    yield c
    c.scene.close()


every_fixture = pytest.mark.parametrize("case", goldens.NAMES, indirect=True)


def on(*names):
    return pytest.mark.parametrize("case", names, indirect=True)


# ---- 1: the camera rays ------------------------------------------------------------------------------------------------------------
@every_fixture
def test_camera_rays_equal_the_references_queue(case):
    ref = case.ref_rays
    assert case.n == len(ref), (case.n, len(ref))
    if case.name == "realistic":
        assert case.n < W * goldens.HEIGHT
    order = np.argsort(case.pixel, kind="stable")
    assert np.array_equal(case.pixel[order], ref[:, 0].astype(np.int64))          # the pixel set (the fixture is in pixel order)
    rays = _np(case.rays)[order]
    assert np.array_equal(_bits(rays[:, 0:6]), _bits(ref[:, 1:7]))                # o, d
    assert np.array_equal(_bits(rays[:, 7]), _bits(ref[:, 7]))                    # time
    assert np.all(np.isposinf(rays[:, 6]))                                        # tMax
    lam = _np(case.lambda4)
    assert np.all((lam >= 360) & (lam <= 830))


# ---- 2, 3: the interactions ----------------------------------------------------------------------------------------------------------
@every_fixture
def test_interactions_equal_the_references_material_items(case):
    rows, ref = case.item_rows()
    assert len(rows) >= goldens.MIN_COVERAGE * case.n
    assert np.all(case.np["valid"][rows] == 1)
    bad = {}
    for name, col, width in FIELDS:
        same = np.all(_bits(case.np[name][rows]) == _bits(ref[:, col:col + width]), axis=1)
        if not same.all():
            i = int(np.where(~same)[0][0])
            bad[name] = (int((~same).sum()), "pixel %d: %s, reference %s" % (int(ref[i, 1]), case.np[name][rows[i]], ref[i, col:col + width]))
    assert not bad, bad


@every_fixture
def test_ids_follow_the_scenes_tables_and_inputs_are_echoed(case):
    rows, ref = case.item_rows()
    rays = _np(case.rays)
    v = case.np
    assert np.array_equal(_bits(v["time"][rows]), _bits(rays[rows, 7]))
    assert np.array_equal(_bits(v["t"][rows]), _bits(case.rec["t"][rows]))
    assert np.all(v["planes_f"][4:, :, 3] == 0) and np.all(v["planes_i"][1, :, 3] == 0)
    for k, i in enumerate(rows):
        mesh = case.mesh_of(case.rec["prim"][i])
        m = case.meshes[mesh]
        assert v["mesh"][i] == mesh and v["mesh_flags"][i] == m.flags, (case.name, i)
        assert v["material"][i] == m.material and case.material_type[m.material] == int(ref[k, 0]), (case.name, i, m.material, ref[k, 0])
        assert v["area_light"][i] == (m.first_light + (case.rec["prim"][i] - m.first_tri) if m.first_light >= 0 else -1)
        assert (v["medium_inside"][i], v["medium_outside"][i]) == (m.medium_inside, m.medium_outside)
    if case.name in ("instances", "general", "curve_alpha", "animated", "nested"):
        assert np.any(case.rec["instance"][rows] >= 0), "no hit inside an object instance"


# ---- 4: shapes at which the kernel itself can go wrong ---------------------------------------------------------------------------------
@every_fixture
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_a_prefix_gives_the_same_rows(case, n):
    """the grid-stride tail and the plane addressing with n no multiple of 4, of the wave or of the block"""
    assert n <= case.n
    r = case.scene.interactions_device(case.rays[:n].contiguous(), case.hits[:n].contiguous())
    assert np.array_equal(_bits(_np(r["planes_f"])), _bits(case.planes_f[:, :n]))
    assert np.array_equal(_np(r["planes_i"]), case.planes_i[:, :n])


@every_fixture
def test_misses_between_hits(case):
    """every other ray with tMax = 0 finds nothing: its row is valid = 0, ids -1 and zeros, and the neighbours are untouched"""
    n = min(case.n, 130)
    rays = case.rays[:n].clone()
    rays[0::2, 6] = 0
    hits = case.scene.trace_device(rays)
    rec = np.ascontiguousarray(_np(hits)).view(np.int32)
    assert np.all(rec[0::2, 0] == -1)
    r = case.scene.interactions_device(rays, hits)
    pf, pi = _np(r["planes_f"]), _np(r["planes_i"])
    assert np.all(_bits(pf[:, 0::2]) == 0)
    assert np.all(pi[0, 0::2] == -1)
    assert np.all(pi[1, 0::2] == np.array([-1, 0, 0, 0], dtype=np.int32))
    assert np.array_equal(_bits(pf[:, 1::2]), _bits(case.planes_f[:, 1:n:2]))
    assert np.array_equal(pi[:, 1::2], case.planes_i[:, 1:n:2])


@every_fixture
def test_a_callers_buffer_is_not_written_past_its_planes(case, wfpt):
    import torch
    n, guard = 65, 1024
    nf, ni = wfpt.INTR_FPLANES * n * 4, wfpt.INTR_IPLANES * n * 4
    of = torch.full((nf + guard,), -12345.5, dtype=torch.float32, device="cuda:0")
    oi = torch.full((ni + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    r = case.scene.interactions_device(case.rays[:n].contiguous(), case.hits[:n].contiguous(), out=(of, oi))
    assert r["planes_f"].data_ptr() == of.data_ptr() and r["planes_i"].data_ptr() == oi.data_ptr()
    assert np.all(_np(of[nf:]) == -12345.5) and np.all(_np(oi[ni:]) == 0x5A5A5A5A)
    assert np.array_equal(_bits(_np(of[:nf]).reshape(wfpt.INTR_FPLANES, n, 4)), _bits(case.planes_f[:, :n]))
    assert np.array_equal(_np(oi[:ni]).reshape(wfpt.INTR_IPLANES, n, 4), case.planes_i[:, :n])


# ---- 5: the ray's time reaches the transformations ------------------------------------------------------------------------------------
@on("animated", "nested")
def test_the_rays_time_moves_an_animated_hit(case):
    """The same hit records at times 0, 0.5 and 1.  The coated-diffuse surfaces (tag 6) are a rotating animated shape — in intr_nested
    one inside an instance definition, used statically and under an animated transformation (a nested placement: two transformations
    per hit): three different pi.  The room is static: the same pi at any time.  At the camera ray's own time the rows are the
    fixture's."""
    c, name = case, case.name
    rows, ref = c.item_rows()
    moving = rows[ref[:, 0] == 6.0]
    room = rows[c.rec["instance"][rows] < 0]   # (an animated shape is an instance of its own: what is left at the top level is the room)
    assert len(moving) >= 4 and len(room) >= 100
    at = {}
    for t in (0.0, 0.5, 1.0):
        rays = c.rays.clone()
        rays[:, 7] = t
        r = c.scene.interactions_device(rays, c.hits)
        at[t] = np.concatenate([_np(r["pi_lo"]), _np(r["pi_hi"])], axis=1)
        assert np.all(_np(r["time"])[rows] == np.float32(t))
    for a, b in ((0.0, 0.5), (0.5, 1.0), (0.0, 1.0)):
        assert np.all(np.any(at[a][moving] != at[b][moving], axis=1)), (name, a, b)
        assert np.array_equal(_bits(at[a][room]), _bits(at[b][room]))
    if name == "nested":
        assert c.scene.query("nested_animated") > 0
        assert np.any(c.rec["instance"][moving] >= 0)
    own = c.scene.interactions_device(c.rays, c.hits)
    k = ref[:, 0] == 6.0
    assert np.array_equal(_bits(_np(own["pi_lo"])[moving]), _bits(ref[k, 2:5]))
    assert np.array_equal(_bits(_np(own["pi_hi"])[moving]), _bits(ref[k, 5:8]))


# ---- 6: stream ordering ------------------------------------------------------------------------------------------------------------------
@on("instances")
def test_the_calls_queue_behind_torchs_stream_without_a_host_sync(case):
    """rays written by a torch op on a side stream immediately before the call, results consumed by a torch op immediately after it"""
    import torch
    c = case
    side = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.ones((4096, 4096), dtype=torch.float32, device="cuda:0")
        for _ in range(8):                                    # work the producer has to wait behind
            big = big @ big * (1.0 / 4096)
        rays = c.rays * big[0, 0]                             # = the rays, once the products are done
        hits = c.scene.trace_device(rays)
        r = c.scene.interactions_device(rays, hits)
        total = r["planes_f"].sum(dtype=torch.float64) + r["planes_i"].sum(dtype=torch.float64)
        planes_f = r["planes_f"].clone()
    side.synchronize()
    assert np.array_equal(_bits(_np(planes_f)), _bits(c.planes_f))
    want = c.planes_f.astype(np.float64).sum() + c.planes_i.astype(np.float64).sum()
    assert abs(float(total) - want) <= 1e-6 * abs(want) + 1e-6
    # ... and the camera rays, consumed at once on the same stream
    with torch.cuda.stream(side):
        rays2, pix2, _ = c.scene.camera_rays_device(0)
        s = rays2[:, :6].sum(dtype=torch.float64)
    side.synchronize()
    assert np.array_equal(_bits(_np(rays2)), _bits(_np(c.rays))) and np.array_equal(_np(pix2), _np(c.pixel_xy))
    assert np.isfinite(float(s))


@on("tris")
def test_first_hit_chains_the_three_calls(case):
    c = case
    r = c.scene.first_hit(0)
    assert np.array_equal(_bits(_np(r["planes_f"])), _bits(c.planes_f)) and np.array_equal(_np(r["planes_i"]), c.planes_i)
    assert np.array_equal(_np(r["pixel_xy"]), _np(c.pixel_xy)) and np.array_equal(_np(r["hits"]), _np(c.hits))
    assert c.scene.query("intr_variant") == c.scene.plan("intr_variant") == 0


@on("tris")
def test_arguments_are_checked_before_anything_is_launched(case, wfpt):
    import torch
    _, hip = wfpt.libs()
    c = case
    f = hip.wf_hit_interaction_device
    f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    of = torch.zeros((wfpt.INTR_FPLANES * 4 * 4 + 4,), dtype=torch.float32, device="cuda:0")
    oi = torch.zeros((wfpt.INTR_IPLANES * 4 * 4,), dtype=torch.int32, device="cuda:0")
    rays, hits = c.rays[:4].contiguous(), c.hits[:4].contiguous()
    assert f(c.scene.ctx, 0, None, None, None, None) == 0
    assert f(c.scene.ctx, 4, rays.data_ptr(), hits.data_ptr(), None, oi.data_ptr()) != 0 and b"wf_hit_interaction_device" in hip.wf_last_error()
    assert f(c.scene.ctx, 4, rays.data_ptr(), hits.data_ptr(), of.data_ptr() + 4, oi.data_ptr()) != 0 and b"aligned" in hip.wf_last_error()
    g = hip.wf_camera_rays_device
    g.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
    cap = c.scene.query("pixels_per_pass")
    assert cap == W * goldens.HEIGHT
    assert g(c.scene.ctx, 0, 0, cap - 1, of.data_ptr(), oi.data_ptr(), of.data_ptr(), oi.data_ptr()) != 0 and b"wf_camera_rays_device" in hip.wf_last_error()
    torch.cuda.synchronize()
    assert float(of.abs().sum()) == 0 and int(oi.abs().sum()) == 0


@on("tris")
def test_the_camera_rays_call_stays_out_of_the_renders_statistic(case):
    """the rays handed to a caller are not the render's: wf_render_stats.camera_rays does not move, and a render after the call is the
    render before it"""
    case.scene.clear_film()
    case.scene.render()
    before, image = case.scene.stats()["camera_rays"], case.scene.image()
    assert before == W * goldens.HEIGHT * 4
    case.scene.camera_rays_device(1)
    assert case.scene.stats()["camera_rays"] == before
    case.scene.clear_film()
    case.scene.render()
    assert case.scene.stats()["camera_rays"] == before
    assert np.array_equal(_bits(case.scene.image()), _bits(image))
