"""Point-cloud filtering without a device: the kernels' own arithmetic compiled for the host (csrc/knn_point.h through
tests/knn_host_harness.cpp) against the brute-force restatement (tests/knn_oracle.py) on the shared case list (tests/knn_cases.py), the
restatement against an independent implementation (scipy's cKDTree), the host logic of `PointCloud` and of the SOR rule, and the
reference's outputs in tests/golden/g16_pointcloud.npz (tools/gen_golden_pointcloud.py: the reference's modules with a stub open3d
whose filter IS the restatement).

Bounds. Host build against the restatement: equality of bits (cell coordinates, cells, keys, d2, the bound, its decisions, covariance
sums, and the neighbours of a ring search that uses the header's stop rule): the same IEEE float64 operations in the same order; the host
build is for plain x86-64 without fused multiply-add, so a lost `#pragma clang fp contract(off)` shows on the device only
(tests/test_gpu_pointcloud.py). Restatement against cKDTree: sqrt(d2) within 4 ulp (relative 4 * 2^-52) - three squares and two adds
round at most 2 ulp, the square root halves that and adds half an ulp, cKDTree may sum in another order. Normals: the restatement alone
must leave at most 1 % of a case's points under the eigenvalue gap of 1e-6 that the device test conditions on, and the host build's
Jacobi vector must lie within 1e-8 of eigh's for the others (Davis-Kahan: a few hundred eps over a gap of 1e-6)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_cases as KC  # noqa: E402
import knn_oracle as O  # noqa: E402
import toolchain  # noqa: E402

# 4099 x 4099 x rings in a scalar loop, and 2^24 rings for a lone point (the host search has no step budget): the device test covers them
HOST_SKIP = {"n4099", "cell_cap_lone_z", "cell_cap_lone_y"}
GAP = 1e-6


@pytest.fixture(scope="module")
def g16():
    with np.load(O.GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """tests/knn_host_harness.cpp + csrc/knn_point.h as a shared library, behind a stub <hip/hip_runtime.h>."""
    lib = toolchain.host_library(str(tmp_path_factory.mktemp("knn_host")), "knn_host_harness.cpp")
    P, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    lib.knn_host_cells.argtypes = [P, L, P, P, P, P, P]
    lib.knn_host_d2.argtypes, lib.knn_host_d2.restype = [P, P], D
    lib.knn_host_ring_bound2.argtypes, lib.knn_host_ring_bound2.restype = [P, P, I, P, P], D
    lib.knn_host_done.argtypes, lib.knn_host_done.restype = [P, P, I, P, P, D, D], I
    lib.knn_host_covariance.argtypes = [P, I, P, P, P]
    lib.knn_host_self.argtypes = [P, L, P, P, I, D, P, P, P, P, P]
    return lib


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def host_self(lib, case, k, radius2):
    p = case["points"]
    n = len(p)
    grid, dims = KC.grid(case)
    idx, d2 = np.full((n, k), -7, np.int32), np.full((n, k), -7.0)
    count, mean, rings = np.full(n, -7, np.int32), np.full(n, -7.0), np.full(n, -7, np.int32)
    lib.knn_host_self(p.ctypes.data, n, grid.ctypes.data, dims.ctypes.data, k, radius2, count.ctypes.data, idx.ctypes.data, d2.ctypes.data,
                      mean.ctypes.data, rings.ctypes.data)
    return idx, d2, count, mean, rings


# ---- (a) the host build of knn_point.h -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KC.names())
def test_host_cells_and_keys_equal_the_oracle(host_lib, name):
    case = KC.by_name(name)
    p = case["points"]
    n = len(p)
    grid, dims = KC.grid(case)
    t, c, key = np.zeros((n, 3)), np.zeros((n, 3), np.int32), np.zeros(n, np.int64)
    host_lib.knn_host_cells(p.ctypes.data, n, grid.ctypes.data, dims.ctypes.data, t.ctypes.data, c.ctypes.data, key.ctypes.data)
    ot = O.cell_coords(p, grid[:3], grid[3])
    oc = O.cells(ot, dims)
    assert np.array_equal(bits(t), bits(ot)) and np.array_equal(c, oc) and np.array_equal(key, O.keys(oc, dims.astype(np.int64)))
    assert key.min() >= 0 and key.max() < int(np.prod(dims.astype(np.int64))) <= 2 ** 24
    assert (oc.max(0) == dims - 1).all()                     # the grid is exactly as large as the cloud needs
    # the bound after rings 0..2 and its decisions, for a sample of queries and k-th distances
    rng = np.random.default_rng(n)
    for i in rng.integers(0, n, min(n, 12)):
        ci = np.ascontiguousarray(c[i])
        for r in range(3):
            b2 = host_lib.knn_host_ring_bound2(t[i].ctypes.data, ci.ctypes.data, r, grid.ctypes.data, dims.ctypes.data)
            want = O.ring_bound2(t[i], oc[i], r, dims, grid[3])
            assert bits(b2) == bits(want), (name, i, r, b2, want)
            for kth in (0.0, b2, np.nextafter(b2, 0.0), np.inf):
                for radius2 in (np.inf, b2, 0.0):
                    got = host_lib.knn_host_done(t[i].ctypes.data, ci.ctypes.data, r, grid.ctypes.data, dims.ctypes.data, kth, radius2)
                    assert bool(got) == O.done(t[i], oc[i], r, dims, grid[3], kth, radius2), (name, i, r, kth, radius2)


@pytest.mark.parametrize("name", [n for n in KC.names() if n not in HOST_SKIP])
def test_host_ring_search_equals_brute_force(host_lib, name):
    """The header's stop rule on the host: a ring search that ends by knn_done finds exactly the brute-force neighbours."""
    case = KC.by_name(name)
    full = KC.full(name)
    for k in case["ks"]:
        for radius2 in case["radius2s"]:
            idx, d2, count, mean, rings = host_self(host_lib, case, k, radius2)
            oidx, od2, ocount, omean = O.cut(full, k, radius2)
            what = (name, k, radius2)
            assert np.array_equal(count, ocount), what
            assert np.array_equal(idx, oidx), what
            assert np.array_equal(bits(d2), bits(od2)) and np.array_equal(bits(mean), bits(omean)), what
            assert (rings >= 1).all()
    if name == "sparse_cells":
        assert np.median(rings) >= 5
    if name.startswith("far_outlier"):
        assert rings[-1] == 41 == KC.grid(case)[1].max() and O.rings_needed(case["points"], len(rings) - 1, case["ks"][-1], case["s"]) == rings[-1]


def test_host_d2_and_covariance_equal_the_oracle(host_lib):
    rng = np.random.default_rng(0)
    for scale in (1.0, 1e6, 1e-3):
        p, q = rng.normal(0, scale, (200, 3)), rng.normal(0, scale, (200, 3))
        got = np.array([host_lib.knn_host_d2(p[i].ctypes.data, q[i].ctypes.data) for i in range(200)])
        d = p - q
        assert np.array_equal(bits(got), bits(((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])))
    for count in (1, 2, 3, 10, 30, 64):
        nb = np.ascontiguousarray(rng.normal(0, 1, (count, 3)) * (1.0, 1.0, 0.01) + (1e3, -2e3, 50.0))
        mean, cov, nrm = np.zeros(3), np.zeros(6), np.zeros(3)
        host_lib.knn_host_covariance(nb.ctypes.data, count, mean.ctypes.data, cov.ctypes.data, nrm.ctypes.data)
        omean, ocov = O.covariance(nb)
        assert np.array_equal(bits(mean), bits(omean)) and np.array_equal(bits(cov), bits(ocov)), count
        if count < 3:
            assert tuple(nrm) == (0.0, 0.0, 1.0)


def normal_cases(g16):
    return {"noisy_plane": (KC.noisy_plane(), 0.3, 30), "sphere_patch": (KC.sphere_patch(), 0.5, 30), "g16": (g16["points"], 3.0, 30)}


@pytest.mark.parametrize("name", ["noisy_plane", "sphere_patch", "g16"])
def test_normals_host_jacobi_against_eigh(host_lib, g16, name):
    pts, radius, max_nn = normal_cases(g16)[name]
    idx, d2, count, _ = O.knn_self(pts, max_nn, radius * radius)
    ref, gap = O.normals(pts, idx, count)
    clear = gap >= GAP
    assert (~clear).mean() <= 0.01, (name, float((~clear).mean()))          # the cloud suits the device test's condition
    assert (count >= 3).mean() > 0.95
    worst = 0.0
    for i in np.nonzero(clear)[0][::7]:
        c = int(count[i])
        nb = np.ascontiguousarray(pts[idx[i, :c]])
        mean, cov, nrm = np.zeros(3), np.zeros(6), np.zeros(3)
        host_lib.knn_host_covariance(nb.ctypes.data, c, mean.ctypes.data, cov.ctypes.data, nrm.ctypes.data)
        assert abs(np.linalg.norm(nrm) - 1.0) < 1e-14
        worst = max(worst, float(np.linalg.norm(np.cross(nrm, ref[i]))))
        if c >= 3 and abs(ref[i][2]) > 1e-6:
            assert nrm[2] > 0 and ref[i][2] > 0
    assert worst <= 1e-8, (name, worst)


# ---- (b) the oracle against an independent implementation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,seed", [(500, 10, 1), (2000, 30, 2), (1000, 50, 3), (300, 64, 4)])
def test_oracle_distances_equal_ckdtree(n, k, seed):
    from scipy.spatial import cKDTree
    pts = np.random.default_rng(seed).uniform(-5, 5, (n, 3))                # seeded, continuous: no ties
    idx, d2, count, mean = O.knn_self(pts, k)
    dist, ti = cKDTree(pts).query(pts, k)
    dist, ti = dist.reshape(n, k), ti.reshape(n, k)
    assert (count == k).all() and (np.diff(d2, axis=1) > 0).all()           # indeed no ties
    assert np.array_equal(idx, ti)
    assert (np.abs(np.sqrt(d2) - dist) <= 4 * 2.0 ** -52 * dist).all()
    assert np.array_equal(idx[:, 0], np.arange(n)) and (d2[:, 0] == 0).all()


def test_oracle_radius_and_order():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 2], [0, 0, 0]], np.float64)
    idx, d2, count, mean = O.knn_self(pts, 4, 1.0)
    assert idx[0].tolist() == [0, 4, 1, 2] and count.tolist() == [4, 3, 3, 1, 4]       # the lower index first; d2 == radius2 is kept
    assert idx[4].tolist() == [0, 4, 1, 2] and idx[3].tolist() == [3, -1, -1, -1] and np.isinf(d2[3, 1:]).all()
    assert mean[0] == (0.0 + 0.0 + 1.0 + 1.0) / 4.0 and mean[3] == 0.0


# ---- (c) PointCloud host logic -------------------------------------------------------------------------------------------------------------
def test_point_cloud_ply_round_trip_and_header(tmp_path, g16):
    from icepy4d_amd.core import PointCloud
    from icepy4d_amd.core.point_cloud import ply_header
    pts, col = g16["points"][:50], g16["colors"][:50]
    pc = PointCloud(points3d=pts, points_col=col)
    assert len(pc) == 50 and repr(pc) == "PointCloud with 50 points" and pc.get_points().dtype == np.float64
    path = tmp_path / "sub" / "cloud.ply"
    assert pc.write_ply(path) is True
    raw = path.read_bytes()
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 50\nproperty double x\nproperty double y\nproperty double z\n"
              b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert raw.startswith(header) and header == ply_header(50, True, False) and len(raw) == len(header) + 50 * 27
    back = PointCloud(pcd_path=str(path))
    assert np.array_equal(back.get_points(), pts) and back.normals is None
    c8 = np.clip(np.round(col * 255.0), 0, 255)
    assert np.array_equal(back.colors, c8 / 255.0)
    path2 = tmp_path / "again.ply"
    back.write_ply(path2)
    assert path2.read_bytes() == raw                                        # byte-stable
    # normals and no colours
    pc2 = PointCloud(points3d=pts)
    pc2.normals = np.tile([0.0, 0.6, 0.8], (50, 1))
    pc2.write_ply(tmp_path / "n.ply")
    raw2 = (tmp_path / "n.ply").read_bytes()
    assert raw2.startswith(ply_header(50, False, True)) and b"property double nx" in raw2 and len(raw2) == len(ply_header(50, False, True)) + 50 * 48
    b2 = PointCloud(pcd_path=tmp_path / "n.ply")
    assert b2.colors is None and np.array_equal(b2.normals, pc2.normals) and b2.get_colors() is None
    # an ascii file with float coordinates
    (tmp_path / "a.ply").write_text("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n1 2 3\n4 5 6.5\n")
    assert np.array_equal(PointCloud(pcd_path=tmp_path / "a.ply").get_points(), [[1, 2, 3], [4, 5, 6.5]])
    assert len(PointCloud()) == 0


def test_point_cloud_colours_and_g16_arguments(g16):
    import inspect
    from icepy4d_amd.core import PointCloud
    pc = PointCloud(points3d=g16["points"], points_col=g16["colors"])
    assert np.array_equal(pc.get_colors(), g16["colors_int"]) and pc.get_colors().dtype == np.dtype(int)
    assert pc.get_colors(as_float=True).dtype == np.float32 and np.array_equal(pc.get_colors(as_float=True), g16["colors"].astype(np.float32))
    assert np.array_equal((g16["colors"] * 255.0).astype(int), g16["colors_int"])
    sig = inspect.signature(PointCloud.sor_filter).parameters
    assert (sig["nb_neighbors"].default, sig["std_ratio"].default) == (10, 3.0) == tuple(g16["args"][0])
    assert tuple(g16["args"][1]) == (50, 1.5)
    sig = inspect.signature(PointCloud.estimate_normals).parameters
    assert (sig["radius"].default, sig["max_nn"].default) == (1.0, 30)
    assert list(inspect.signature(PointCloud.__init__).parameters)[1:] == ["points3d", "pcd_path", "points_col", "verbose"]
    # the fixture is the oracle's filter of the stored cloud, and the planted outliers are gone
    for tag, (nb, ratio) in (("sor10", (10, 3.0)), ("sor50", (50, 1.5))):
        kept, ind = O.remove_statistical_outlier(g16["points"], nb, ratio)
        assert np.array_equal(ind, g16[f"{tag}_ind"]) and np.array_equal(kept, g16[f"{tag}_points"])
        assert not set(ind.tolist()) & set(g16["planted"].tolist()) and len(ind) >= len(g16["points"]) - 2 * len(g16["planted"])
    assert np.array_equal(g16["sor10_colors_int"], g16["colors_int"][g16["sor10_ind"]])


def test_point_cloud_refusals(tmp_path):
    from icepy4d_amd.core import PointCloud
    from icepy4d_amd.utils import point_cloud_filters as F
    pc = PointCloud(points3d=np.zeros((3, 3)))
    with pytest.raises(NotImplementedError, match="laspy"):
        pc.write_las(tmp_path / "x.las")
    with pytest.raises(NotImplementedError, match="laspy"):
        PointCloud(pcd_path=tmp_path / "x.las")
    with pytest.raises(ValueError):
        PointCloud(pcd_path=tmp_path / "x.xyz")
    with pytest.raises(ValueError):
        PointCloud(points3d=np.zeros((3, 3)), points_col=np.zeros((2, 3)))
    (tmp_path / "bad.ply").write_bytes(b"not a ply")
    with pytest.raises(ValueError):
        PointCloud(pcd_path=tmp_path / "bad.ply")
    # argument checks come before any device work
    for bad in ((0, 1.0), (10, 0.0), (10, -1.0), (65, 1.0)):
        with pytest.raises(ValueError):
            F.remove_statistical_outlier(np.zeros((5, 3)), *bad)
    for k in (0, 65):
        with pytest.raises(ValueError):
            F.knn_search(np.zeros((5, 3)), k)
    with pytest.raises(ValueError):
        F.knn_search(np.zeros((5, 3)), 3, radius=-1.0)
    with pytest.raises(ValueError):
        F.knn_search(np.zeros((5, 3)), 3, cell_size=0.0)


def test_cell_size_fitting():
    from icepy4d_amd.utils import point_cloud_filters as F
    lo, hi = np.zeros(3), np.array([1.0, 2.0, 0.0])
    assert F.grid_dims(lo, hi, 0.5) == [3, 5, 1]
    s = F.fit_cell_size(lo, hi, 1e-9, 2 ** 24)
    d = F.grid_dims(lo, hi, s)
    assert s > 1e-9 and d[0] * d[1] * d[2] <= 2 ** 24 and d[2] == 1
    assert F.fit_cell_size(lo, hi, 0.5, 2 ** 24) == 0.5
    s = F.fit_cell_size(np.full(3, -1e300), np.full(3, 1e300), 1e-300, 2 ** 24)
    assert np.prod(F.grid_dims(np.full(3, -1e300), np.full(3, 1e300), s)) <= 2 ** 24


# ---- (d) the SOR rule's edge cases ---------------------------------------------------------------------------------------------------------
def test_sor_rule_edge_cases():
    from icepy4d_amd.utils.point_cloud_filters import sor_indices
    # valid == 1: one point is its own only neighbour, avg 0 -> nothing positive, nothing kept
    _, _, count, mean = O.knn_self(np.array([[1.0, 2.0, 3.0]]), 10)
    assert count.tolist() == [1] and mean.tolist() == [0.0]
    for fn in (O.sor, sor_indices):
        ind, thr = fn(mean, count, 3.0)
        assert len(ind) == 0 and ind.dtype == np.int64
    # valid == 1 with a positive statistic: the standard deviation divides by zero, the threshold is NaN, nothing is kept
    for fn in (O.sor, sor_indices):
        ind, thr = fn(np.array([0.5]), np.array([2]), 3.0)
        assert len(ind) == 0 and np.isnan(thr)
    # all points identical: every avg == 0
    _, _, count, mean = O.knn_self(np.tile([[1.0, 2.0, 3.0]], (20, 1)), 10)
    assert (count == 10).all() and (mean == 0).all()
    for fn in (O.sor, sor_indices):
        assert len(fn(mean, count, 3.0)[0]) == 0
    # n < nb_neighbors: every point has n neighbours
    pts = np.random.default_rng(3).uniform(0, 1, (7, 3))
    pts[6] = (30.0, 30.0, 30.0)
    _, _, count, mean = O.knn_self(pts, 10)
    assert (count == 7).all()
    a, b = O.sor(mean, count, 1.0), sor_indices(mean, count, 1.0)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[0].tolist() == [0, 1, 2, 3, 4, 5]
    # the mean divides by the number of points with a neighbour, not by the number of positive terms
    mean, count = np.array([0.0, 1.0, 2.0, 0.0]), np.array([3, 3, 3, 3])
    ind, thr = sor_indices(mean, count, 1.0)
    cm = 3.0 / 4.0
    assert thr == cm + np.sqrt(((1.0 - cm) ** 2 + (2.0 - cm) ** 2) / 3.0) and ind.tolist() == [1]
    assert O.sor(mean, count, 1.0)[1] == thr
    assert O.remove_statistical_outlier(np.zeros((0, 3)), 10, 3.0)[1].shape == (0,)
