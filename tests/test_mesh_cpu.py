"""Mesh filters, the convex-hull crop and uniform mesh sampling without a device: the kernels' own arithmetic compiled for the host
(csrc/mesh_tri.h through tests/mesh_host_harness.cpp) against the numpy restatement (tests/mesh_oracle.py) on the shared case list
(tests/mesh_cases.py), the restatement against independent facts, the half-space hull test against scipy's Delaunay, the reference's call
chain recorded in tests/golden/g20_meshing.npz (tools/gen_golden_mesh.py), the refusals of the Python layer, the ABI, the scratch layout,
the imports and the PLY reader and writer.

Bounds. Host build against the restatement: equality of bits (a NaN equals a NaN). Derived, not measured: a triangle's sample count is
within 1 of its area share times N (the issue's bound, asserted as it stands: rint(c_t / C N) is within 1/2 of c_t / C N at both ends); a + b + c is within 2 ulp of 1 (three roundings of exact 1); the mean of N
uniform samples of a triangle lies within six standard errors of its centroid, the standard error per axis sqrt(var / N) with var =
(|v0 - g|^2 + |v1 - g|^2 + |v2 - g|^2) / 12 per axis, the second moment of a uniform triangle about its centroid g."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import toolchain  # noqa: E402
import mesh_cases as MC  # noqa: E402
import mesh_oracle as O  # noqa: E402

from icepy4d_amd.post_processing import triangle_mesh as TM  # noqa: E402  (the feature under test: without it nothing here can pass)

MODULES = ["icepy4d_amd.post_processing.triangle_mesh", "icepy4d_amd.meshing", "icepy4d_amd.post_processing.open3d_fun", "icepy4d_amd.post_processing"]
NAMES = ["im_mesh_max_items", "im_mesh_hull_chunk", "im_mesh_select", "im_mesh_triangle_keys", "im_mesh_vertex_keys", "im_mesh_edge_keys",
         "im_mesh_first_of_segment", "im_mesh_edge_census", "im_mesh_in_hull", "im_mesh_sample_table", "im_mesh_sample"]


@pytest.fixture(scope="module")
def g20():
    with np.load(O.GOLDEN, allow_pickle=False) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    lib = toolchain.host_library(str(tmp_path_factory.mktemp("mesh_host")), "mesh_host_harness.cpp")
    P, I, L, U, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_double
    for name in ("mesh_host_max_items", "mesh_host_hull_chunk", "mesh_host_max_facets", "mesh_host_nan_key"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [], L
    lib.mesh_host_triangle_keys.argtypes = [P, L, P, P]
    lib.mesh_host_vertex_keys.argtypes = [P, L, P, P, P]
    lib.mesh_host_edge_keys.argtypes = [P, L, P]
    lib.mesh_host_areas.argtypes = [P, L, P, L, P]
    lib.mesh_host_table.argtypes, lib.mesh_host_table.restype = [P, L, L, P, P, P], L
    lib.mesh_host_hull.argtypes = [P, L, P, L, P, P]
    lib.mesh_host_uniform.argtypes, lib.mesh_host_uniform.restype = [U, U, I], D
    lib.mesh_host_sample.argtypes = [P, L, P, L, P, L, U, P, P, P, P, P, P, P]
    for name, n in (("carve_mesh_select", 2), ("carve_mesh_segment", 1), ("carve_mesh_hull", 1), ("carve_mesh_sample", 1)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [L] * n, U
    return lib


def same(a, b):
    """equal bits, a NaN equal to a NaN"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def data(a):
    return None if a is None else a.ctypes.data


# ---- (a) the host build of mesh_tri.h ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.names())
def test_host_build_equals_the_oracle(host_lib, name):
    c = MC.by_name(name)
    v, t = c["vertices"], c["triangles"]
    V, T = len(v), len(t)
    k = [np.full(T, -7, np.int64) for _ in range(2)]
    host_lib.mesh_host_triangle_keys(t.ctypes.data, T, k[0].ctypes.data, k[1].ctypes.data)
    assert all(np.array_equal(a, b) for a, b in zip(k, O.triangle_keys(t))), name
    k = [np.full(V, -7, np.int64) for _ in range(3)]
    host_lib.mesh_host_vertex_keys(v.ctypes.data, V, *(a.ctypes.data for a in k))
    assert all(np.array_equal(a, b) for a, b in zip(k, O.vertex_keys(v))), name
    e = np.full(3 * T, -7, np.int64)
    host_lib.mesh_host_edge_keys(t.ctypes.data, T, e.ctypes.data)
    assert np.array_equal(e, O.edge_keys(t)), name
    area = np.full(T, -7.0)
    host_lib.mesh_host_areas(v.ctypes.data, V, t.ctypes.data, T, area.ctypes.data)
    want_area = O.areas(v, t)
    assert same(area, want_area) and np.isfinite(area).all() and (area >= 0).all(), name
    for N in c["samples"]:
        q, cum, end = (np.full(T, -7, np.int64) for _ in range(3))
        C = host_lib.mesh_host_table(area.ctypes.data, T, N, q.ctypes.data, cum.ctypes.data, end.ctypes.data)
        if C == 0:
            assert N == 0 or want_area.max(initial=0.0) == 0.0, name
            continue
        wq, wc, wC, wend = O.sample_table(want_area, N)
        assert C == wC and np.array_equal(q, wq) and np.array_equal(cum, wc) and np.array_equal(end, wend), (name, N)
        if N == 0 or V == 0:
            continue
        want = O.sample(v, t, N, c["seed"], c["colors"], c["normals"])
        pts, col, nrm, w = (np.full((N, 3), -7.0) for _ in range(4))
        which = np.full(N, -7, np.int32)
        host_lib.mesh_host_sample(v.ctypes.data, V, t.ctypes.data, T, end.ctypes.data, N, c["seed"], data(c["colors"]), data(c["normals"]), pts.ctypes.data,
                                  col.ctypes.data, nrm.ctypes.data, which.ctypes.data, w.ctypes.data)
        assert np.array_equal(which, want["triangle"]) and same(w, want["weights"]) and same(pts, want["points"]) and same(nrm, want["normals"]), (name, N)
        assert (want["colors"] is None and (col == -7.0).all()) or same(col, want["colors"]), (name, N)


@pytest.mark.parametrize("F", MC.HULL_FACETS)
def test_host_hull_equals_the_oracle(host_lib, F):
    facets = MC.tangent_facets(F)
    q = MC.hull_queries(facets)
    value, inside = np.full(len(q), -7.0), np.full(len(q), 7, np.uint8)
    host_lib.mesh_host_hull(q.ctypes.data, len(q), facets.ctypes.data, F, value.ctypes.data, inside.ctypes.data)
    assert same(value, O.hull_values(q, facets)) and np.array_equal(inside.astype(bool), O.point_in_hull(q, facets))
    assert 0 < inside.sum() < len(q) and not inside[np.isnan(q).any(1)].any()


def test_the_generator_is_a_function_of_seed_and_index(host_lib):
    i = np.array([0, 1, 2, 63, 64, 2 ** 26 - 1, 2 ** 40], np.uint64)
    for seed in (0, 1, 7, 2 ** 63, 2 ** 64 - 1):
        for k in (0, 1):
            got = np.array([host_lib.mesh_host_uniform(seed, int(j), k) for j in i])
            assert same(got, O.uniform(seed, i, k)) and (got >= 0).all() and (got < 1).all()
    r = np.concatenate([O.uniform(3, np.arange(200000), 0), O.uniform(3, np.arange(200000), 1)])
    assert abs(r.mean() - 0.5) < 6 * np.sqrt(1 / 12 / len(r)) and len(np.unique(r)) == len(r)


# ---- (b) the restatement against independent facts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v3_t1", "special", "strip_257", "strip_65537", "field_with_duplicates", "bad_triangles_between"])
def test_oracle_sample_counts_weights_and_positions(name):
    c = MC.by_name(name)
    v, t = c["vertices"], c["triangles"]
    area = O.areas(v, t)
    for N in c["samples"]:
        if N == 0:
            continue
        r = O.sample(v, t, N, c["seed"], c["colors"], c["normals"])
        per = np.bincount(r["triangle"], minlength=len(t))
        assert np.array_equal(per, np.diff(np.concatenate([[0], r["count_end"]]))) and per.sum() == N and (np.diff(r["count_end"]) >= 0).all(), (name, N)
        deviation = np.abs(per - area / area.sum() * N)
        print(f"{name} N={N}: largest |count - area share x N| = {deviation.max():.5f}")
        assert (deviation <= 1.0).all() and (per[area == 0] == 0).all(), (name, N)
        w = r["weights"]
        assert (w >= 0).all() and (np.abs(w.sum(1) - 1.0) <= 2 * np.spacing(1.0)).all(), (name, N)
        tt = t[r["triangle"]]
        p = r["points"]
        v0, v1, v2 = v[tt[:, 0]], v[tt[:, 1]], v[tt[:, 2]]
        n = np.cross(v1 - v0, v2 - v0)
        scale = np.abs(np.stack([v0, v1, v2])).max() + 1.0
        assert (np.abs(((p - v0) * n).sum(1)) <= 1e-12 * scale * np.linalg.norm(n, axis=1).max()).all(), (name, N)      # in the plane
        for a, b, cc in ((v0, v1, v2), (v1, v2, v0), (v2, v0, v1)):                                                       # on the inner side of every edge
            assert ((np.cross(b - a, p - a) * n).sum(1) >= -1e-9 * scale * scale * (n * n).sum(1).max() ** 0.5).all(), (name, N)


def test_oracle_sample_mean_is_the_centroid_and_seeds_differ():
    v = np.array([(0.0, 0.0, 0.0), (4.0, 0.0, 1.0), (1.0, 3.0, -2.0)])
    t = np.array([(0, 1, 2)], np.int32)
    N = 65537
    r = O.sample(v, t, N, seed=11)
    g = v.mean(0)
    se = np.sqrt(((v - g) ** 2).sum(0) / 12.0 / N)
    assert (np.abs(r["points"].mean(0) - g) <= 6 * se).all()
    again, other = O.sample(v, t, N, seed=11), O.sample(v, t, N, seed=12)
    assert same(again["points"], r["points"]) and not np.array_equal(other["points"], r["points"])
    assert same(O.sample(v, t, 100, seed=11)["points"], r["points"][:100])                    # a function of (seed, i) alone
    unit = np.cross(v[1] - v[0], v[2] - v[0])
    assert np.allclose(r["normals"], unit / np.linalg.norm(unit), rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        O.sample(v, np.array([(0, 0, 1)], np.int32), 5)
    assert len(O.sample(v, t, 0)["points"]) == 0


def test_oracle_filters_do_what_they_are_named_for():
    m = MC.mesh_of(MC.by_name("special_plain"))
    out, vl, pos = m.remove_degenerate_triangles()
    assert pos.tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 10, 11, 12] and len(out.vertices) == 13
    out, vl, pos = m.remove_duplicated_triangles()
    assert pos.tolist() == [0, 2, 3, 4, 5, 6, 7, 8, 9, 11]                       # (1,2,0), (10,11,1), the last (0,1,2) are rotations; (2,1,0) is flipped
    out, vl, pos = m.remove_duplicated_vertices()
    assert vl.tolist() == [0, 1, 2, 3, 6, 7, 8, 10, 11] and out.triangles[4].tolist() == [0, 1, 2] and out.triangles[11].tolist() == [0, 1, 2]
    out, vl, pos = m.remove_unreferenced_vertices()
    assert vl.tolist() == [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12]
    out, vl, pos = m.remove_vertices_by_mask(np.arange(13) == 1)
    assert pos.tolist() == [4, 9, 11] and len(out.vertices) == 12 and out.triangles.tolist() == [[3, 4, 1], [2, 2, 2], [11, 8, 1]]
    out, vl, pos = m.select_by_index([2, 0, 1, 1, 7])
    assert vl.tolist() == [0, 1, 2] and pos.tolist() == [0, 1, 2, 5, 12]
    out, vl, pos = m.select_by_index([2, 0, 1, 1, 7], cleanup=False)
    assert vl.tolist() == [0, 1, 2, 7]
    assert [O.edge_census(MC.by_name(n)["triangles"]) for n in ("fan_3", "fan_4", "two_fans", "strip_257", "v0_t0")] == [1, 1, 2, 0, 0]
    for name, left in (("fan_3", 2), ("fan_4", 2), ("fan_4_equal_areas", 2), ("two_fans", 4)):
        mesh = MC.mesh_of(MC.by_name(name))
        out, vl, pos = mesh.remove_non_manifold_edges()
        assert len(pos) == left and O.edge_census(out.triangles) == 0, name
        assert np.array_equal(TM.non_manifold_rounds(mesh.vertices, mesh.triangles), np.isin(np.arange(len(mesh.triangles)), pos)), name
    assert MC.mesh_of(MC.by_name("fan_4_equal_areas")).remove_non_manifold_edges()[2].tolist() == [2, 3]          # ties: the lowest index goes first


@pytest.mark.parametrize("n_hull", [40, 300, 2000])
def test_half_space_test_agrees_with_delaunay(host_lib, n_hull):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(20)
    hull = rng.normal(0, 1, (n_hull, 3))
    q = rng.normal(0, 1, (20000, 3))
    facets = O.hull_facets(hull)
    value = O.hull_values(q, facets)
    excluded = np.abs(value) <= 1e-9
    want = Delaunay(hull).find_simplex(q) >= 0
    print(f"hull of {n_hull}: {len(facets)} facets, {int(excluded.sum())} of {len(q)} excluded, {int(((value <= 0) != want)[~excluded].sum())} disagreements")
    assert excluded.sum() == 0
    assert np.array_equal((value <= 0)[~excluded], want[~excluded])
    # the placed points lie on the boundary: excluded from the comparison with Delaunay, still a definite answer of the restatement
    from scipy.spatial import ConvexHull
    h = ConvexHull(hull)
    placed = np.concatenate([hull[h.vertices], hull[h.simplices].mean(1)])
    placed = np.ascontiguousarray(placed)
    pv = O.hull_values(placed, facets)
    value, inside = np.full(len(placed), -7.0), np.full(len(placed), 7, np.uint8)
    host_lib.mesh_host_hull(placed.ctypes.data, len(placed), facets.ctypes.data, len(facets), value.ctypes.data, inside.ctypes.data)
    assert (np.abs(pv) <= 1e-9).all() and same(value, pv) and np.array_equal(inside.astype(bool), O.point_in_hull(placed, facets))
    assert same(TM.hull_facets(hull), facets) and same(TM.compute_convex_hull(hull), hull[np.sort(h.vertices)])


# ---- (c) the reference's call chain (g20) ------------------------------------------------------------------------------------------------------
def test_g20_calls_order_survivors_and_names(g20, tmp_path):
    from icepy4d_amd import meshing
    from icepy4d_amd.post_processing import MeshingPoisson
    calls = json.loads(g20["calls"].tobytes().decode())
    assert [c[0] for c in calls] == [
        "io.read_point_cloud", "PointCloud.remove_statistical_outlier", "PointCloud.compute_convex_hull", "PointCloud.estimate_normals",
        "TriangleMesh.create_from_point_cloud_poisson", "TriangleMesh.orient_triangles", "TriangleMesh.remove_vertices_by_mask",
        "TriangleMesh.remove_degenerate_triangles", "TriangleMesh.remove_duplicated_triangles", "TriangleMesh.remove_duplicated_vertices",
        "TriangleMesh.remove_non_manifold_edges", "point_in_hull", "TriangleMesh.select_by_index", "TriangleMesh.sample_points_uniformly",
        "PointCloud.select_by_index", "io.write_triangle_mesh", "io.write_point_cloud"]
    args = dict((c[0], c[1]) for c in calls)
    assert args["PointCloud.remove_statistical_outlier"] == {"nb_neighbors": 50, "std_ratio": 1.5}
    assert args["PointCloud.estimate_normals"] == {"radius": 1, "max_nn": 30}
    poisson = args["TriangleMesh.create_from_point_cloud_poisson"]
    assert (poisson["depth"], poisson["width"], poisson["scale"], poisson["linear_fit"], poisson["has_normals"]) == (9, 0, 1.1, False, True)
    assert args["TriangleMesh.remove_vertices_by_mask"]["type"] == "list" and args["TriangleMesh.sample_points_uniformly"] == {"number_of_points": 2000}
    assert json.loads(g20["files"].tobytes().decode()) == ["mesh_2022_05_01.ply", "sampled_2022_05_01.ply"]
    cfg = json.loads(g20["cfg"].tobytes().decode())
    m = MeshingPoisson(O.GOLDEN, tmp_path / "out", {"num_sampled_points": 2000})
    assert {k: m.cfg[k] for k in cfg} == cfg and m.cfg.num_sampled_points == 2000 and cfg["min_mesh_denisty"] == 11 and cfg["poisson_depth"] == 9 and cfg["do_SOR"] is True
    assert meshing.CFG["num_sampled_points"] == 4 * 10 ** 6 and meshing.CFG["min_mesh_denisty"] == 9 and meshing.CFG["do_SOR"] is False
    labels = json.loads(g20["timer_labels"].tobytes().decode())
    assert labels == ["Read pcd", "SOR", "Normals estimation", "Poisson meshing", "Filter by density", "Filter by location", "crop by polyline", "save outputs"]
    # the survivors of every step, through the restatement
    mesh = O.Mesh(g20["surface_vertices"], g20["surface_triangles"])
    origin = np.arange(len(mesh.vertices))
    assert np.array_equal(g20["density_mask"], g20["surface_density"] < 11)
    steps = [("by_mask", lambda m: m.remove_vertices_by_mask(g20["density_mask"])), ("degenerate_triangles", O.Mesh.remove_degenerate_triangles),
             ("duplicated_triangles", O.Mesh.remove_duplicated_triangles), ("duplicated_vertices", O.Mesh.remove_duplicated_vertices),
             ("non_manifold_edges", O.Mesh.remove_non_manifold_edges), ("by_hull", lambda m: m.select_by_index(g20["hull_index"]))]
    for name, step in steps:
        mesh, vlist, _ = step(mesh)
        origin = origin[vlist]
        assert np.array_equal(origin, g20[name + "_vertices"]) and np.array_equal(mesh.triangles, g20[name + "_triangles"]), name
        assert same(mesh.vertices, g20["surface_vertices"][origin]), name
    assert len(g20["duplicated_triangles_triangles"]) == len(g20["degenerate_triangles_triangles"]) - 3          # the three planted copies go
    assert len(g20["degenerate_triangles_triangles"]) < len(g20["by_mask_triangles"]) and len(g20["duplicated_vertices_vertices"]) < len(g20["by_mask_vertices"])
    r = O.sample(mesh.vertices, mesh.triangles, 2000, 0)
    assert same(r["points"], g20["sampled_points"]) and same(r["normals"], g20["sampled_normals"])
    assert same(g20["sampled_points"][g20["crop_index"]], g20["cropped_points"]) and same(g20["sampled_normals"][g20["crop_index"]], g20["cropped_normals"])
    assert 0 < len(g20["crop_index"]) < 2000


# ---- (d) refusals before any device work -------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_device(tmp_path):
    from icepy4d_amd.post_processing import MeshingPoisson
    v, t = MC.strip(4)
    with pytest.raises(ValueError):
        TM.TriangleMesh(v, t, vertex_colors=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        TM.TriangleMesh(v, t, attributes={"density": np.zeros(2)})
    m = TM.TriangleMesh(v, t)
    with pytest.raises(ValueError):
        m.remove_vertices_by_mask(np.zeros(3, bool))
    with pytest.raises(ValueError):
        m.select_by_index([0, 6])
    with pytest.raises(ValueError):
        m.sample_points_uniformly(-1)
    with pytest.raises(ValueError):
        m.sample_points_uniformly(2 ** 26 + 1)
    with pytest.raises(ValueError):
        TM.TriangleMesh(v, np.zeros((0, 3))).sample_points_uniformly(5)
    empty = m.sample_points_uniformly(0)
    assert len(empty) == 0 and empty.normals.shape == (0, 3)
    for bad in (np.zeros((0, 4)), np.array([[1.0, 0, 0, np.nan]]), np.array([[np.inf, 0, 0, 1.0]])):
        with pytest.raises(ValueError):
            TM.point_in_hull(np.zeros((2, 3)), facets=bad)
    with pytest.raises(ValueError):
        TM.point_in_hull(np.zeros((2, 2)), facets=MC.tangent_facets(4))
    with pytest.raises(ValueError):
        TM.point_in_hull(np.zeros((2, 3)))
    assert TM.point_in_hull(np.zeros((0, 3)), facets=MC.tangent_facets(4)).shape == (0,)
    assert repr(m) == "TriangleMesh with 6 points and 4 triangles." and len(m) == 6 and m.has_triangles() and not m.has_vertex_colors() and not m.has_vertex_normals()
    lo, hi = m.get_axis_aligned_bounding_box()
    assert same(lo, v.min(0)) and same(hi, v.max(0))
    # MeshingPoisson without a hook or a mesh path names both routes
    from icepy4d_amd.core import PointCloud
    pcd = PointCloud(points3d=np.random.default_rng(1).normal(0, 1, (30, 3)))
    pcd.normals = np.zeros((30, 3))
    pcd.write_ply(tmp_path / "dense_2022_01_01.ply")
    mp = MeshingPoisson(tmp_path / "dense_2022_01_01.ply", tmp_path / "out", {"do_SOR": False})
    mp.read_pcd()
    assert len(mp.convex_hull) >= 4
    with pytest.raises(NotImplementedError) as e:
        mp.poisson_meshing()
    assert "reconstruct" in str(e.value) and "mesh_path" in str(e.value)
    with pytest.raises(AssertionError):
        MeshingPoisson(tmp_path / "missing.ply", tmp_path / "out", {})


# ---- (e) ABI, scratch layout, resources, imports, PLY ------------------------------------------------------------------------------------------
def test_abi_is_declared_bound_and_exported(host_lib):
    import re
    from icepy4d_amd import _lib
    with open(os.path.join(ROOT, "include", "icematch.h")) as f:
        header = f.read()
    for n in NAMES:
        m = re.search(r"\n(?:int|long long) " + n + r"\(([^;]*)\);", header)
        assert m and n in _lib.SIGNATURES, n
        args = [a for a in m.group(1).split(",") if a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES[n]), (n, len(args), len(_lib.SIGNATURES[n]))
    assert "-78" in header
    lib = _lib.load()
    assert lib.im_mesh_max_items() == O.MAX_ITEMS == host_lib.mesh_host_max_items() == TM.max_items()
    assert lib.im_mesh_hull_chunk() == O.HULL_CHUNK == host_lib.mesh_host_hull_chunk() and host_lib.mesh_host_max_facets() == TM.MAX_FACETS
    assert host_lib.mesh_host_nan_key() == O.NAN_KEY


def test_scratch_layouts_are_pinned(host_lib):
    def up256(b):
        return (b + 255) // 256 * 256

    def blocks_of(n, per):
        return (n + per - 1) // per

    for V, T in ((0, 1), (1, 0), (255, 300), (257, 256), (65537, 131070), (2 ** 26, 2 ** 26)):
        assert host_lib.carve_mesh_select(V, T) == up256(T) + 2 * up256(V) + up256(blocks_of(max(V, T, 1), 256) * 8), (V, T)
    for n in (1, 255, 256, 257, 2 ** 26):
        assert host_lib.carve_mesh_segment(n) == up256((n + 1) * 4) + up256(n * 4) + up256(blocks_of(n, 256) * 8) + 256, n
        assert host_lib.carve_mesh_sample(n) == 2 * up256(n * 8) + up256(blocks_of(n, 256) * 8) + 512, n
    for F in (1, 4, 512, 2 ** 22):
        assert host_lib.carve_mesh_hull(F) == up256(32 * F), F


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    res = toolchain.kernel_resources(toolchain.device_listing("mesh.hip", str(tmp_path)))
    mine = {k: v for k, v in res.items() if "mesh_" in k or "Mesh" in k}
    assert len(mine) >= 11 + 8, sorted(res)                       # eleven kernels and the four scans' templates
    for k, f in mine.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (k, dict(f))
    lds = [f["group_segment_fixed_size"] for k, f in mine.items() if "in_hull" in k]
    assert lds == [4 * 8 * O.HULL_CHUNK]


@pytest.mark.parametrize("module", MODULES)
def test_module_imports_as_the_first_import(module):
    r = subprocess.run([sys.executable, "-c", f"import {module}"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("ascii", [False, True])
@pytest.mark.parametrize("density", [False, True])
def test_ply_round_trip(tmp_path, ascii, density):
    c = MC.by_name("strip_257")
    attributes = {"density": np.random.default_rng(4).uniform(5, 15, len(c["vertices"]))} if density else None
    m = TM.TriangleMesh(c["vertices"], c["triangles"], np.round(np.random.default_rng(5).uniform(0, 1, c["vertices"].shape) * 255) / 255, c["normals"], attributes)
    TM.write_mesh(tmp_path / "a" / "m.ply", m, ascii=ascii)
    r = TM.read_triangle_mesh(tmp_path / "a" / "m.ply")
    assert same(r.vertices, m.vertices) and np.array_equal(r.triangles, m.triangles) and r.triangles.dtype == np.int32
    assert same(r.vertex_normals, m.vertex_normals) and np.array_equal(np.round(r.vertex_colors * 255), np.round(m.vertex_colors * 255))
    assert ("density" in r.attributes) == density and (not density or same(r.attributes["density"], attributes["density"]))
    plain = TM.TriangleMesh(c["vertices"], c["triangles"])
    TM.write_mesh(tmp_path / "p.ply", plain, ascii=ascii)
    r = TM.read_triangle_mesh(tmp_path / "p.ply")
    assert same(r.vertices, plain.vertices) and r.vertex_colors is None and r.vertex_normals is None and r.attributes == {}
    from icepy4d_amd.post_processing.voxel_grid import write_triangle_mesh
    write_triangle_mesh(tmp_path / "v.ply", c["vertices"], None, c["triangles"])           # the tuple writer's files are read too
    r = TM.read_triangle_mesh(tmp_path / "v.ply")
    assert same(r.vertices, c["vertices"]) and np.array_equal(r.triangles, c["triangles"])
    box = TM.TriangleMesh.from_arrays(c["vertices"], None, c["triangles"])
    assert same(box.vertices, c["vertices"]) and box.vertex_colors is None
