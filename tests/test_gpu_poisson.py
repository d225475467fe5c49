"""The Poisson surface reconstruction (csrc/poisson.hip, csrc/poisson_node.h) on the device, on every case of tests/poisson_cases.py:
every stage against the numpy restatement (tests/poisson_oracle.py), two point orders, two runs against each other, the refusals, and the
Python routes (`poisson_reconstruct`, `TriangleMesh.create_from_point_cloud_poisson`, `MeshingPoisson` with the hook bound,
`meshing.poisson_mesh_series`).

Bounds. Everything is equality: W, V, the right-hand side, chi after every cycle, the iso-value, vertices, triangles, weights and
densities are bit-identical to the restatement. Derived, not measured: the kernels and the restatement perform the same IEEE float64
operations in the same order with contraction off (float64 division and square root are correctly rounded on the device, the library is
built without a fast-math flag); the splat adds integers, so its sums are order-free; the scans are integer prefix sums. The host build of
the same header agrees with the restatement (tests/test_poisson_cpu.py); what only this file can show is the launch code, the atomics,
the scans, the reduction in LDS and a lost `#pragma clang fp contract(off)`.

The cases: a sphere at depth 4 (17 nodes per axis: one block along x, five along y) and at depth 5 with and without noise, a half sphere
(an open surface), depth 2 (one smoothed level above the direct solve), a sloped front of 20 000 points at depth 6 (65 nodes per axis:
two blocks along x, the second with one node; 2^d + 1 is never a multiple of a block edge), a single sample in a given grid, samples on
nodes and on the upper faces of the cube with scale = 1 (the cell index clamps), one cycle and eight. No case asks for a depth above 6."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import poisson_cases as PC  # noqa: E402
import poisson_oracle as O  # noqa: E402

from icepy4d_amd.post_processing import poisson as P  # noqa: E402

pytestmark = pytest.mark.gpu

BAND, SENT, FILL = 4096, 0xA5, 0x5A
REFUSED = -80


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def host(t):
    return t.cpu().numpy()


def device_run(eng, name, points=None, normals=None):
    c = PC.case(name)
    trace = {}
    f = P.poisson_field(c["points"] if points is None else points, c["normals"] if normals is None else normals, depth=c["depth"], scale=c["scale"],
                        cycles=c["cycles"], grid=c["grid"], engine=eng, trace=trace)
    v, t, w = P.extract_surface(f, engine=eng)
    return f, trace, host(v), host(t), host(w)


def check_against_oracle(name, f, trace, v, t, w):
    o = PC.oracle(name)
    assert same(f.origin, o["origin"]) and f.h == o["h"] and f.depth == o["depth"], name
    assert same(host(trace["W"]), o["W"]), (name, "W")
    assert same(host(trace["V"]), o["V"]), (name, "V")
    assert same(host(trace["rhs"]), o["rhs"]), (name, "rhs")
    assert len(trace["chis"]) == len(o["chis"]) == PC.case(name)["cycles"]
    for k, (got, want) in enumerate(zip(trace["chis"], o["chis"])):
        assert same(host(got), want), (name, "chi after cycle", k + 1)
    assert same(host(f.chi), o["chi"]) and same(host(f.W), o["W"]), name
    assert f.iso == o["iso"], (name, "iso", f.iso, o["iso"])
    assert t.dtype == np.int32 and same(v, o["vertices"]) and same(t, o["triangles"]) and same(w, o["weights"]), (name, "surface")
    assert same(P.density_of(w, f.depth), o["density"]), (name, "density")


@pytest.mark.parametrize("name", PC.ALL)
def test_every_stage_equals_the_restatement_bit_for_bit(eng, name):
    check_against_oracle(name, *device_run(eng, name))


def test_two_point_orders_and_two_runs(eng):
    name = "sphere_d5_noise"
    c = PC.case(name)
    perm = np.random.default_rng(9).permutation(len(c["points"]))
    first = device_run(eng, name)
    again = device_run(eng, name)
    other = device_run(eng, name, c["points"][perm], c["normals"][perm])
    check_against_oracle(name, *other)
    for a, b in ((first, again), (first, other)):
        assert same(host(a[0].chi), host(b[0].chi)) and a[0].iso == b[0].iso and same(a[2], b[2]) and same(a[3], b[3]) and same(a[4], b[4])


def test_torch_inputs_and_the_reduction_over_several_chunks(eng):
    import torch
    c, o = PC.case("front_d6"), PC.oracle("front_d6")
    f = P.poisson_field(torch.from_numpy(c["points"]).to(eng.device), torch.from_numpy(c["normals"]).to(eng.device), depth=6, engine=eng)
    assert same(host(f.chi), o["chi"]) and f.iso == o["iso"] and same(f.origin, o["origin"]) and f.h == o["h"]
    x = np.random.default_rng(3).normal(size=3 * 1024 * 1024 + 17)         # three levels of partial sums
    assert P._ordered_sum(eng, torch.from_numpy(x).to(eng.device)) == O.ordered_sum(x)
    assert P._ordered_sum(eng, torch.from_numpy(x).to(eng.device), torch.from_numpy(x[::-1].copy()).to(eng.device)) == O.ordered_sum(x * x[::-1])
    assert P.max_depth(eng) == 9


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------------
class Framed:
    """An output of `shape` x `dtype` between two bands of sentinel bytes, in one device allocation, pre-filled."""

    def __init__(self, eng, shape, dtype):
        import torch
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        h = np.full(2 * BAND + self.n, SENT, np.uint8)
        h[BAND:BAND + self.n] = FILL
        self.buf = torch.from_numpy(h).to(eng.device)
        self.ptr = self.buf.data_ptr() + BAND

    def untouched(self, what):
        h = self.buf.cpu().numpy()
        assert (h[:BAND] == SENT).all() and (h[BAND + self.n:] == SENT).all() and (h[BAND:BAND + self.n] == FILL).all(), what

    def framed(self, what):
        h = self.buf.cpu().numpy()
        assert (h[:BAND] == SENT).all() and (h[BAND + self.n:] == SENT).all(), (what, "a byte outside the output was written")
        return h[BAND:BAND + self.n].view(self.dtype).reshape(self.shape)


def raw(eng, name, *args):
    return getattr(eng.ctx.lib, name)(eng.ctx.h, *args)


def test_refusals_leave_the_outputs_untouched(eng):
    import torch
    from icepy4d_amd._lib import ptr
    st = eng.stream_ptr()
    depth, M = 2, 5
    N = M ** 3
    pts = torch.from_numpy(np.array([[0.4, 0.6, 0.3]])).to(eng.device)
    nrm = torch.from_numpy(np.array([[0.0, 0.0, 2.0]])).to(eng.device)
    grid = np.array([0.0, 0.0, 0.0, 0.25])
    src = torch.zeros(4 * N, dtype=torch.float64, device=eng.device)
    mask_in, base_in = torch.zeros(N, dtype=torch.uint8, device=eng.device), torch.zeros(N, dtype=torch.int32, device=eng.device)
    fields, one, coarse = Framed(eng, (4, N), np.float64), Framed(eng, (N,), np.float64), Framed(eng, (27,), np.float64)
    mask, base, counts = Framed(eng, (N,), np.uint8), Framed(eng, (N,), np.int32), Framed(eng, (2,), np.int64)
    vert, wgt, tri = Framed(eng, (8, 3), np.float64), Framed(eng, (8,), np.float64), Framed(eng, (8, 3), np.int32)
    g, bad_grid, nan_grid = grid.ctypes.data, np.array([0.0, 0.0, 0.0, 0.0]), np.array([np.nan, 0.0, 0.0, 0.25])
    for what, rc in [
        ("splat depth 1", raw(eng, "im_poisson_splat", ptr(pts), ptr(nrm), 1, g, 1, fields.ptr, st)),
        ("splat depth 10", raw(eng, "im_poisson_splat", ptr(pts), ptr(nrm), 1, g, 10, fields.ptr, st)),
        ("splat above the cap", raw(eng, "im_poisson_splat", ptr(pts), ptr(nrm), 2 ** 26 + 1, g, depth, fields.ptr, st)),
        ("splat negative count", raw(eng, "im_poisson_splat", ptr(pts), ptr(nrm), -1, g, depth, fields.ptr, st)),
        ("splat null points", raw(eng, "im_poisson_splat", None, ptr(nrm), 1, g, depth, fields.ptr, st)),
        ("splat null normals", raw(eng, "im_poisson_splat", ptr(pts), None, 1, g, depth, fields.ptr, st)),
        ("splat null grid", raw(eng, "im_poisson_splat", ptr(pts), ptr(nrm), 1, None, depth, fields.ptr, st)),
        ("splat null fields", raw(eng, "im_poisson_splat", ptr(pts), ptr(nrm), 1, g, depth, None, st)),
        ("splat h = 0", raw(eng, "im_poisson_splat", ptr(pts), ptr(nrm), 1, bad_grid.ctypes.data, depth, fields.ptr, st)),
        ("splat NaN origin", raw(eng, "im_poisson_splat", ptr(pts), ptr(nrm), 1, nan_grid.ctypes.data, depth, fields.ptr, st)),
        ("divergence depth 10", raw(eng, "im_poisson_divergence", ptr(src), 10, 0.25, one.ptr, st)),
        ("divergence null", raw(eng, "im_poisson_divergence", None, depth, 0.25, one.ptr, st)),
        ("jacobi depth 1", raw(eng, "im_poisson_jacobi", ptr(src), ptr(src), 1, 1.0, one.ptr, st)),
        ("jacobi null f", raw(eng, "im_poisson_jacobi", ptr(src), None, depth, 1.0, one.ptr, st)),
        ("jacobi in place", raw(eng, "im_poisson_jacobi", one.ptr, ptr(src), depth, 1.0, one.ptr, st)),
        ("restrict depth 0", raw(eng, "im_poisson_restrict", ptr(src), ptr(src[N:]), 0, 1.0, one.ptr, coarse.ptr, st)),
        ("restrict null coarse", raw(eng, "im_poisson_restrict", ptr(src), ptr(src[N:]), depth, 1.0, one.ptr, None, st)),
        ("restrict residual over u", raw(eng, "im_poisson_restrict", one.ptr, ptr(src), depth, 1.0, one.ptr, coarse.ptr, st)),
        ("prolong depth 10", raw(eng, "im_poisson_prolong", ptr(src), 10, one.ptr, st)),
        ("prolong null", raw(eng, "im_poisson_prolong", None, depth, one.ptr, st)),
        ("coarse null", raw(eng, "im_poisson_coarse", None, 1.0, coarse.ptr, st)),
        ("reduce negative", raw(eng, "im_poisson_reduce", ptr(src), None, -1, one.ptr, st)),
        ("reduce too many", raw(eng, "im_poisson_reduce", ptr(src), None, 4 * 513 ** 3 + 1, one.ptr, st)),
        ("reduce null", raw(eng, "im_poisson_reduce", None, None, 5, one.ptr, st)),
        ("census depth 10", raw(eng, "im_poisson_census", ptr(src), 0.0, 10, mask.ptr, base.ptr, counts.ptr, st)),
        ("census null chi", raw(eng, "im_poisson_census", None, 0.0, depth, mask.ptr, base.ptr, counts.ptr, st)),
        ("census null counts", raw(eng, "im_poisson_census", ptr(src), 0.0, depth, mask.ptr, base.ptr, None, st)),
        ("extract depth 1", raw(eng, "im_poisson_extract", ptr(src), ptr(src), 0.0, 1, g, ptr(mask_in), ptr(base_in), 8, 8, vert.ptr, wgt.ptr, tri.ptr, st)),
        ("extract above the cap", raw(eng, "im_poisson_extract", ptr(src), ptr(src), 0.0, depth, g, ptr(mask_in), ptr(base_in), 2 ** 26 + 1, 8, vert.ptr, wgt.ptr, tri.ptr, st)),
        ("extract negative", raw(eng, "im_poisson_extract", ptr(src), ptr(src), 0.0, depth, g, ptr(mask_in), ptr(base_in), 8, -1, vert.ptr, wgt.ptr, tri.ptr, st)),
        ("extract null mask", raw(eng, "im_poisson_extract", ptr(src), ptr(src), 0.0, depth, g, None, ptr(base_in), 8, 8, vert.ptr, wgt.ptr, tri.ptr, st)),
        ("extract null triangles", raw(eng, "im_poisson_extract", ptr(src), ptr(src), 0.0, depth, g, ptr(mask_in), ptr(base_in), 8, 8, vert.ptr, wgt.ptr, None, st)),
    ]:
        assert rc == REFUSED, (what, rc)
    # zero-size calls return 0 and launch nothing
    assert raw(eng, "im_poisson_splat", None, None, 0, g, depth, fields.ptr, st) == 0
    assert raw(eng, "im_poisson_reduce", None, None, 0, one.ptr, st) == 0
    assert raw(eng, "im_poisson_extract", ptr(src), ptr(src), 0.0, depth, g, ptr(mask_in), ptr(base_in), 0, 0, None, None, None, st) == 0
    eng.synchronize()
    for fr in (fields, one, coarse, mask, base, counts, vert, wgt, tri):
        fr.untouched("a refused or empty call wrote an output")
    assert b"depth" in eng.ctx.lib.im_last_error(eng.ctx.h) or b"null" in eng.ctx.lib.im_last_error(eng.ctx.h)
    # the accepted calls write their outputs and nothing else; a census that is not the field's own leads to no access outside a buffer
    o = PC.oracle("single")
    assert raw(eng, "im_poisson_splat", ptr(pts), ptr(nrm), 1, g, depth, fields.ptr, st) == 0
    eng.synchronize()
    got = fields.framed("splat")
    assert same(got[0].reshape(M, M, M), o["W"]) and same(got[1:].reshape(3, M, M, M), o["V"])
    chi, W = torch.from_numpy(o["chi"].copy()).to(eng.device), torch.from_numpy(o["W"].copy()).to(eng.device)
    assert raw(eng, "im_poisson_census", ptr(chi), o["iso"], depth, mask.ptr, base.ptr, counts.ptr, st) == 0
    eng.synchronize()
    nv, nt = (int(x) for x in counts.framed("counts"))
    assert (nv, nt) == (len(o["vertices"]), len(o["triangles"]))
    d_mask, d_base = torch.from_numpy(mask.framed("mask").copy()).to(eng.device), torch.from_numpy(base.framed("base").copy()).to(eng.device)
    vert, wgt, tri = Framed(eng, (nv + 3, 3), np.float64), Framed(eng, (nv + 3,), np.float64), Framed(eng, (nt + 3, 3), np.int32)
    assert raw(eng, "im_poisson_extract", ptr(chi), ptr(W), o["iso"], depth, g, ptr(d_mask), ptr(d_base), nv, nt, vert.ptr, wgt.ptr, tri.ptr, st) == 0
    eng.synchronize()
    gv, gw, gt = vert.framed("vertices"), wgt.framed("weights"), tri.framed("triangles")
    assert same(gv[:nv], o["vertices"]) and same(gw[:nv], o["weights"]) and same(gt[:nt], o["triangles"])
    assert (gv[nv:].view(np.uint8) == FILL).all() and (gw[nv:].view(np.uint8) == FILL).all() and (gt[nt:].view(np.uint8) == FILL).all()
    # fewer rows than the surface has, and a mask of all ones over a base of large numbers: rows beyond the counts stay as they were
    all_ones = torch.full((N,), 127, dtype=torch.uint8, device=eng.device)
    far = torch.full((N,), 2 ** 30, dtype=torch.int32, device=eng.device)
    for m_, b_, rows in ((d_mask, d_base, 2), (all_ones, d_base, nv), (d_mask, far, nv), (all_ones, far, 2)):
        vert, wgt, tri = Framed(eng, (nv, 3), np.float64), Framed(eng, (nv,), np.float64), Framed(eng, (nt, 3), np.int32)
        assert raw(eng, "im_poisson_extract", ptr(chi), ptr(W), o["iso"], depth, g, ptr(m_), ptr(b_), rows, min(rows, nt), vert.ptr, wgt.ptr, tri.ptr, st) == 0
        eng.synchronize()
        gv, gt = vert.framed("vertices"), tri.framed("triangles")
        wgt.framed("weights")
        assert (gv[rows:].view(np.uint8) == FILL).all() and (gt[min(rows, nt):].view(np.uint8) == FILL).all()


def test_python_layer_refuses_on_the_device_too(eng):
    c = PC.case("sphere_d2")
    with pytest.raises(ValueError):
        P.poisson_field(c["points"], c["normals"], grid=(np.zeros(3), 0.1, 2), engine=eng)        # points outside the given grid
    with pytest.raises(ValueError):
        P.poisson_reconstruct(c["points"], c["normals"], depth=10, engine=eng)
    with pytest.raises(ValueError):
        P.poisson_reconstruct(c["points"], c["normals"] * 0.0, depth=2, engine=eng)


# ---- the Python routes -----------------------------------------------------------------------------------------------------------------------------
def test_reconstruct_and_the_open3d_name(eng):
    from icepy4d_amd.core import PointCloud
    from icepy4d_amd.post_processing import TriangleMesh, poisson_reconstruct
    c, o = PC.case("half_sphere_d5"), PC.oracle("half_sphere_d5")
    v, t, d = poisson_reconstruct(c["points"], c["normals"], depth=5, width=0, scale=1.1, linear_fit=False, engine=eng)
    assert v.dtype == np.float64 and t.dtype == np.int32 and d.dtype == np.float64
    assert same(v, o["vertices"]) and same(t, o["triangles"]) and same(d, o["density"])
    v2, t2, d2 = poisson_reconstruct(c["points"], c["normals"], depth=5, linear_fit=True, engine=eng)
    assert same(v2, v) and same(t2, t) and same(d2, d)                      # both values interpolate linearly
    once, paired, _ = PC.edge_census(t)
    assert once and paired
    pcd = PointCloud(points3d=c["points"])
    pcd.normals = c["normals"]
    mesh, dens = TriangleMesh.create_from_point_cloud_poisson(pcd, depth=5, engine=eng)
    assert same(mesh.vertices, v) and same(mesh.triangles, t) and same(dens, d) and same(mesh.attributes["density"], d)
    wv, wt, wd = poisson_reconstruct(c["points"], c["normals"], depth=8, width=o["h"], engine=eng)       # the width asks for depth 5
    assert same(wv, v) and same(wt, t) and same(wd, d)


def test_meshing_poisson_end_to_end(eng, tmp_path):
    import mesh_oracle as MO
    from icepy4d_amd import meshing
    from icepy4d_amd.core import PointCloud
    from icepy4d_amd.core.point_cloud import read_ply
    from icepy4d_amd.post_processing import MeshingPoisson, poisson_reconstruct, read_triangle_mesh
    from icepy4d_amd.post_processing.triangle_mesh import compute_convex_hull
    c = PC.case("sphere_d4")
    pcd = PointCloud(points3d=c["points"])
    pcd.normals = c["normals"]
    pcd.write_ply(tmp_path / "dense_2022_05_01.ply")
    cfg = {"do_SOR": False, "poisson_depth": 4, "min_mesh_denisty": 3.0, "num_sampled_points": 3000, "save_mesh": True, "sample_mesh": True}
    m = MeshingPoisson(tmp_path / "dense_2022_05_01.ply", tmp_path / "out", cfg, reconstruct=poisson_reconstruct, engine=eng)
    assert m.run() is True
    assert sorted(f.name for f in (tmp_path / "out").iterdir()) == ["mesh_2022_05_01.ply", "sampled_2022_05_01.ply"]
    pts, _, nrm = read_ply(tmp_path / "out" / "sampled_2022_05_01.ply")
    assert len(pts) == 3000 and len(nrm) == 3000 and np.isfinite(pts).all()
    # the restatement's surface through the restatement of the filters
    assert same(m.pcd.points, c["points"]) and same(m.pcd.normals, c["normals"])
    ov, ot, od = O.reconstruct(c["points"], c["normals"], depth=4, width=0, scale=1.1)
    mesh, origin = MO.Mesh(ov, ot), np.arange(len(ov))
    for op, args in (("remove_vertices_by_mask", (od < 3.0,)), ("remove_degenerate_triangles", ()), ("remove_duplicated_triangles", ()),
                     ("remove_duplicated_vertices", ()), ("remove_non_manifold_edges", ())):
        mesh, vlist, _ = getattr(mesh, op)(*args)
        origin = origin[vlist]
    inside = MO.point_in_hull(mesh.vertices, MO.hull_facets(compute_convex_hull(c["points"])))
    mesh, vlist, _ = mesh.select_by_index(np.nonzero(inside)[0], True)
    origin = origin[vlist]
    assert 0 < len(mesh.vertices) < len(ov) and len(mesh.triangles) > 0
    assert same(m.mesh.vertices, mesh.vertices) and same(m.mesh.triangles, mesh.triangles) and same(m.density, od[origin])
    back = read_triangle_mesh(tmp_path / "out" / "mesh_2022_05_01.ply")
    assert same(back.vertices, mesh.vertices) and same(back.triangles, mesh.triangles)
    want = MO.sample(mesh.vertices, mesh.triangles, 3000, 0)
    assert same(pts, want["points"])
    # the series function: the same files from the same hook
    out = meshing.poisson_mesh_series([tmp_path / "dense_2022_05_01.ply"], tmp_path / "series", {**cfg, "crop_polyline_path": ""}, engine=eng)   # no outline to crop by
    assert out == [tmp_path / "series" / "sampled_2022_05_01.ply"] and same(read_ply(out[0])[0], pts)
    assert same(read_triangle_mesh(tmp_path / "series" / "mesh_2022_05_01.ply").vertices, mesh.vertices)
