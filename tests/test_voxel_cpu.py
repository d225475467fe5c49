"""Voxel grids, voxel down-sampling and voxel box meshes without a device: the kernels' own arithmetic compiled for the host
(csrc/voxel_cell.h through tests/voxel_host_harness.cpp) against the numpy restatement (tests/voxel_oracle.py) on the shared case list
(tests/voxel_cases.py), the restatement against independent facts, the reference script's behaviour recorded in
tests/golden/g19_voxel.npz (tools/gen_golden_voxel.py: the reference's `voxelize()` behind a stub open3d that IS the restatement), the
refusals of the Python layer, the ABI, the scratch layout and the kernels' resources.

Bounds. Host build against the restatement: equality of bits (sizes, kept flags, keys, indices, counts, first indices, every mean, centres,
corner keys, positions, vertex colours, triangles): the same IEEE float64 operations in the same order. A NaN compares equal to a NaN: its
sign and payload are not part of the definition (x86 and gfx950 differ in the NaN that inf - inf makes). The host build is for plain
x86-64 without fused multiply-add, so a lost `#pragma clang fp contract(off)` shows on the device only (tests/test_gpu_voxel.py).
Derived, not measured: a kept point lies in its voxel within 1 ulp of |p| + |origin|; a cube's signed volume is s^3 within 8 ulp; the
mesh positions of the script's translate / scale / translate chain EQUAL origin + c * s (see `test_g19_...`)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import toolchain  # noqa: E402
import voxel_cases as VC  # noqa: E402
import voxel_oracle as O  # noqa: E402

from icepy4d_amd.post_processing import voxel_grid as VG  # noqa: E402  (the feature under test: without it nothing here can pass)

MODULES = ["icepy4d_amd.post_processing.voxel_grid", "icepy4d_amd.voxelization", "icepy4d_amd.post_processing", "icepy4d_amd.utils.point_cloud_filters"]
NAMES = ["im_voxel_max_points", "im_voxel_bounds", "im_voxel_keys", "im_voxel_reduce", "im_voxel_mesh_corners", "im_voxel_mesh"]


@pytest.fixture(scope="module")
def g19():
    with np.load(O.GOLDEN, allow_pickle=False) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """tests/voxel_host_harness.cpp + csrc/voxel_cell.h + csrc/stage_scratch.h as a shared library, behind a stub <hip/hip_runtime.h>."""
    lib = toolchain.host_library(str(tmp_path_factory.mktemp("voxel_host")), "voxel_host_harness.cpp")
    P, I, L, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong
    for name in ("vox_host_max_cells", "vox_host_max_points", "vox_host_max_mesh_items", "vox_host_dropped_key"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [], L
    lib.vox_host_dims.argtypes, lib.vox_host_dims.restype = [P, P, I], L
    lib.vox_host_keys.argtypes, lib.vox_host_keys.restype = [P, L, P, P, P], L
    lib.vox_host_voxels.argtypes, lib.vox_host_voxels.restype = [P, P, P, L, P, P] + [P] * 7, L
    lib.vox_host_mesh.argtypes, lib.vox_host_mesh.restype = [P, P, L, P, P, P, P, P], L
    lib.carve_voxel.argtypes, lib.carve_voxel.restype = [L, L, L], U
    lib.carve_voxel_mesh.argtypes, lib.carve_voxel_mesh.restype = [L], U
    return lib


def same(a, b):
    """equal bits, a NaN equal to a NaN"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def data(a):
    return None if a is None else a.ctypes.data


def host_voxels(lib, points, grid, colors=None, normals=None):
    """The host build on one cloud: a dict like tests/voxel_oracle.py's voxelize."""
    pts, grid = np.ascontiguousarray(points, np.float64), np.ascontiguousarray(grid, np.float64)
    n = len(pts)
    dims = np.zeros(3, np.int64)
    assert lib.vox_host_dims(grid.ctypes.data, dims.ctypes.data, 0) == int(np.prod(dims, dtype=object))
    key, kept = np.full(n, -7, np.int64), np.full(n, 7, np.uint8)
    dropped = lib.vox_host_keys(pts.ctypes.data, n, grid.ctypes.data, key.ctypes.data, kept.ctypes.data)
    gi, cnt, first = np.zeros((n, 3), np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    mp, mc, mn, ctr = (np.zeros((n, 3)) for _ in range(4))
    col = None if colors is None else np.ascontiguousarray(colors, np.float64)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float64)
    V = lib.vox_host_voxels(pts.ctypes.data, data(col), data(nrm), n, grid.ctypes.data, key.ctypes.data, gi.ctypes.data, cnt.ctypes.data, first.ctypes.data,
                            mp.ctypes.data, mc.ctypes.data, mn.ctypes.data, ctr.ctypes.data)
    return {"keys": key, "kept": kept.astype(bool), "dropped": dropped, "dims": tuple(int(d) for d in dims), "grid_index": gi[:V], "counts": cnt[:V],
            "first": first[:V], "points": mp[:V], "colors": None if col is None else mc[:V], "normals": None if nrm is None else mn[:V], "centres": ctr[:V]}


def host_mesh(lib, grid, grid_index, colors):
    grid, gi, col = np.ascontiguousarray(grid, np.float64), np.ascontiguousarray(grid_index, np.int32), np.ascontiguousarray(colors, np.float64)
    V = len(gi)
    ckey, vert, vcol, tri = np.zeros(8 * V, np.int64), np.zeros((8 * V, 3)), np.zeros((8 * V, 3)), np.zeros((12 * V, 3), np.int32)
    U = lib.vox_host_mesh(grid.ctypes.data, gi.ctypes.data, V, col.ctypes.data, ckey.ctypes.data, vert.ctypes.data, vcol.ctypes.data, tri.ctypes.data)
    return ckey, vert[:U], vcol[:U], tri


# ---- (a) the host build of voxel_cell.h ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.names())
def test_host_build_equals_the_oracle(host_lib, name):
    case = VC.by_name(name)
    assert host_lib.vox_host_max_cells() == O.MAX_CELLS and host_lib.vox_host_dropped_key() == O.DROPPED
    for e, want in enumerate(VC.full(name)):
        grid = VC.grid_of(case, e)
        got = host_voxels(host_lib, case["clouds"][e], grid, VC.attr(case, "colors", e), VC.attr(case, "normals", e))
        what = (name, e)
        assert got["dims"] == want["dims"] and got["dropped"] == want["dropped"], what
        assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["kept"], O.kept_mask(case["clouds"][e], grid)), what
        for k in ("grid_index", "counts", "first"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
        for k in ("points", "colors", "normals"):
            assert (got[k] is None and want[k] is None) or same(got[k], want[k]), (what, k)
        assert same(got["centres"], O.centers(grid, want["grid_index"])), what


@pytest.mark.parametrize("name", VC.mesh_names())
def test_host_mesh_equals_the_oracle(host_lib, name):
    c = VC.mesh_by_name(name)
    vert, vcol, tri = VC.mesh_full(name)
    ckey, hv, hc, ht = host_mesh(host_lib, c["grid"], c["grid_index"], c["colors"])
    n = O.grid_dims(c["grid"], corners=True)
    corners = c["grid_index"].astype(np.int64)[:, None, :] + O.CORNERS[None]
    assert np.array_equal(ckey, ((corners[..., 0] * (n[1] + 1) + corners[..., 1]) * (n[2] + 1) + corners[..., 2]).ravel()), name
    assert same(hv, vert) and same(hc, vcol) and np.array_equal(ht, tri) and ht.dtype == tri.dtype, name
    if c["vertices"] is not None:
        assert len(vert) == c["vertices"], name


def test_refused_grids(host_lib):
    dims = np.zeros(3, np.int64)

    def cells(grid, corners=0):
        return host_lib.vox_host_dims(np.ascontiguousarray(grid, np.float64).ctypes.data, dims.ctypes.data, corners)

    good = O.make_grid((0, 0, 0), (1, 1, 1), 0.25)
    assert cells(good) == 125 and cells(good, 1) == 216
    for k, v in ((6, 0.0), (6, -1.0), (6, np.nan), (6, np.inf), (0, np.nan), (4, np.inf), (2, -np.inf), (3, -0.5), (0, 1.5)):
        bad = good.copy()
        bad[k] = v
        assert cells(bad) == -1, (k, v)
        with pytest.raises(ValueError):
            O.grid_dims(bad)
        with pytest.raises(ValueError):
            VG.make_grid(bad[:3], bad[3:6], bad[6])
    assert cells(VC.cap_grid(0)[0]) == 2 ** 62 and tuple(dims) == VC.cap_grid(0)[1] and O.grid_dims(VC.cap_grid(0)[0]) == VC.cap_grid(0)[1]
    assert cells(VC.cap_grid(1)[0]) == -1 and cells(VC.cap_grid(0)[0], 1) == -1
    assert cells(O.make_grid((0, 0, 0), (1e300, 1, 1), 1e-300)) == -1          # the size overflows a double
    for bad in (VC.cap_grid(1)[0], O.make_grid((0, 0, 0), (1e300, 1, 1), 1e-300)):
        with pytest.raises(ValueError):
            O.grid_dims(bad)
        with pytest.raises(ValueError):
            VG.make_grid(bad[:3], bad[3:6], bad[6])
    with pytest.raises(ValueError):
        O.grid_dims(VC.cap_grid(0)[0], corners=True)
    assert O.key_bases([VC.cap_grid_3(0)[0]], False, 3)[-1] == 2 ** 62 - 2 ** 40
    with pytest.raises(ValueError):
        O.key_bases([VC.cap_grid_3(1)[0]], False, 3)
    per = VC.by_name("cap_per_cloud_3")["grids"]
    assert O.key_bases(per, True, 3) == [0, 2 ** 61, 2 ** 61 + 2 ** 60, 2 ** 62]
    with pytest.raises(ValueError):
        O.key_bases([per[0], per[1], O.make_grid((0, 0, 0), (VC.S20 - 0.5, VC.S20 - 0.5, VC.S20 + 0.5), 1.0)], True, 3)


# ---- (b) the restatement against independent facts -----------------------------------------------------------------------------------------
def test_the_cases_reach_what_they_are_named_for():
    r = {n: VC.full(n) for n in VC.names()}
    assert [len(r[n][0]["counts"]) for n in ("n0", "n1", "n2")] == [0, 1, 2]
    for n in (1, 63, 64, 65, 1025):
        assert r[f"one_voxel_{n}"][0]["counts"].tolist() == [n] and r[f"one_voxel_{n}"][0]["grid_index"].tolist() == [[1, 0, 1]]
    for V in (255, 256, 257, 65537):
        assert len(r[f"voxels_{V}"][0]["counts"]) == V and r[f"voxels_{V}"][0]["counts"].max() > 1
    assert r["grid_1x1x1"][0]["dims"] == (1, 1, 1) and r["grid_1x1xN"][0]["dims"] == (1, 1, 8) and r["grid_Nx1x1"][0]["dims"] == (8, 1, 1)
    assert len(r["grid_1x1xN"][0]["counts"]) > 4 and len(r["grid_Nx1x1"][0]["counts"]) > 4
    assert r["grid_2p20"][0]["dims"] == (2 ** 20,) * 3 and r["grid_2p20"][0]["voxel_keys"].max() == 2 ** 60 - 1
    assert r["cap_exact"][0]["voxel_keys"].max() == 2 ** 62 - 1
    assert r["cap_under_3_clouds"][2]["voxel_keys"].max() == (2 ** 62 - 2 ** 40) // 3 - 1
    # the division: 0.3, 0.6 and 0.7 at s = 0.1; the reciprocal would put them one voxel higher
    div = VC.by_name("division_s01")["clouds"][0]
    assert VC.full("division_s01")[0]["keys"][:3].tolist() == [(i * 11) * 11 for i in (2, 5, 6)]
    assert np.floor(div[:3, 0] * (1.0 / 0.1)).tolist() == [3.0, 6.0, 7.0] and np.floor(div[:3, 0] / 0.1).tolist() == [2.0, 5.0, 6.0]
    on = r["on_bounds_and_faces"][0]
    assert on["dropped"] == 0 and [0, 0, 0] in on["grid_index"].tolist() and [4, 4, 4] in on["grid_index"].tolist() and [1, 2, 3] in on["grid_index"].tolist()
    assert r["one_ulp_outside"][0]["dropped"] == 6 and len(VC.by_name("one_ulp_outside")["clouds"][0]) == 15
    assert r["nonfinite_points"][0]["dropped"] == 9
    nf = r["nonfinite_attributes"][0]
    assert np.isnan(nf["colors"]).any() and np.isinf(nf["colors"]).any() and np.isnan(nf["normals"]).any()
    sz = r["signed_zeros"][0]
    assert sz["dropped"] == 0 and not np.signbit(sz["colors"]).any() and (sz["colors"] == 0).all()          # a sum from +0.0 never ends at -0.0
    assert np.signbit(VC.by_name("negative_zero_origin")["grids"][0][:3]).all() and r["negative_zero_origin"][0]["dropped"] == 0
    assert np.isinf(r["colour_sum_overflows"][0]["colors"]).all() and (r["colour_sum_overflows"][0]["colors"][0] > 0).tolist() == [True, False, True]
    den = r["colour_sum_denormal"][0]["colors"][0]
    assert 0 < den[0] < 2.3e-308 and 0 < den[1] < 2.3e-308 and den[2] > 2.3e-308
    assert r["colours_absent"][0]["colors"] is None
    b = r["batch_3_one_empty"]
    assert len(b[1]["counts"]) == 0 and b[0]["dropped"] > 1 and b[2]["dropped"] > 1 and len(VC.by_name("batch_3_one_empty")["clouds"][0]) < 64
    assert VC.by_name("batch_3_per_cloud")["per_cloud"] and len({tuple(g) for g in VC.by_name("batch_3_per_cloud")["grids"]}) == 3


@pytest.mark.parametrize("name", VC.names())
def test_oracle_points_lie_in_their_voxels_and_counts_add_up(name):
    case = VC.by_name(name)
    for e, res in enumerate(VC.full(name)):
        pts, grid = case["clouds"][e], VC.grid_of(case, e)
        s, origin = grid[6], grid[:3]
        assert int(res["counts"].sum()) == len(pts) - res["dropped"], (name, e)
        kept = res["keys"] != O.DROPPED
        p = pts[kept]
        idx = np.searchsorted(res["voxel_keys"], res["keys"][kept])
        centre = O.centers(grid, res["grid_index"])[idx].reshape(-1, 3)
        ulp = np.spacing(np.abs(p) + np.abs(origin))
        assert (centre - s / 2 - ulp <= p).all() and (p <= centre + s / 2 + ulp).all(), (name, e)
        assert (res["grid_index"] >= 0).all() and (res["grid_index"] < np.array(res["dims"], dtype=object)).all(), (name, e)
        assert np.array_equal(res["first"], [np.nonzero(res["keys"] == k)[0][0] for k in res["voxel_keys"][:50]] + list(res["first"][50:])), (name, e)


@pytest.mark.parametrize("name", ["voxels_257", "batch_3_one_empty", "on_bounds_and_faces", "n1", "nonfinite_points", "signed_zeros"])
def test_oracle_down_sampled_points_lie_in_their_voxels(name):
    case = VC.by_name(name)
    for e, pts in enumerate(case["clouds"]):
        s = 0.3
        r = O.down_sample(pts, s, VC.attr(case, "colors", e), VC.attr(case, "normals", e))
        finite = np.isfinite(pts).all(1)
        assert int(r["counts"].sum()) == int(finite.sum())              # the grid holds every finite point
        if r["grid"] is None:
            continue
        centre = O.centers(r["grid"], r["grid_index"]).reshape(-1, 3)
        ulp = np.spacing(np.abs(r["points"]) + np.abs(r["grid"][:3])) * (1 + r["counts"][:, None])          # a mean of m points: m roundings more
        assert (centre - s / 2 - ulp <= r["points"]).all() and (r["points"] <= centre + s / 2 + ulp).all(), (name, e)
        assert len(r["points"]) <= max(1, finite.sum())


@pytest.mark.parametrize("name", VC.mesh_names())
def test_oracle_cubes_face_outward(name):
    c = VC.mesh_by_name(name)
    vert, vcol, tri = VC.mesh_full(name)
    s3 = c["grid"][6] ** 3
    V = len(c["grid_index"])
    for v in list(range(min(V, 40))) + [V - 1]:
        vol = O.signed_volume(vert, tri[12 * v:12 * v + 12])
        assert abs(vol - s3) <= 8 * np.spacing(s3), (name, v, vol, s3)
    assert tri.min() == 0 and tri.max() == len(vert) - 1 and len(tri) == 12 * V
    lo, hi = VC.mesh_by_name(name)["grid_index"].min(0), VC.mesh_by_name(name)["grid_index"].max(0) + 1
    assert same(vert.min(0), c["grid"][:3] + lo * c["grid"][6]) and same(vert.max(0), c["grid"][:3] + hi * c["grid"][6])


def test_oracle_mesh_facts():
    vert, vcol, tri = VC.mesh_full("one_voxel")
    edges = {tuple(sorted((int(t[a]), int(t[b])))) for t in tri for a, b in ((0, 1), (1, 2), (2, 0))}
    assert len(vert) - len(edges) + len(tri) == 2 and (len(vert), len(edges), len(tri)) == (8, 18, 12)
    assert same(vcol, np.tile(VC.mesh_by_name("one_voxel")["colors"], (8, 1)))
    c = VC.mesh_by_name("block_2x2x2")
    vert, vcol, tri = VC.mesh_full("block_2x2x2")
    mid = np.nonzero((vert == c["grid"][:3] + np.array([3, 2, 5]) * c["grid"][6]).all(1))[0]
    total = np.zeros(3)
    for col in c["colors"]:
        total = total + col
    assert len(mid) == 1 and same(vcol[mid[0]], total / 8.0)                                              # the centre vertex averages 8 colours
    assert sorted(np.bincount(np.unique(tri.reshape(-1, 12, 3).reshape(8, -1), axis=1).ravel()).tolist()) == sorted([1] * 8 + [2] * 12 + [4] * 6 + [8])
    with pytest.raises(ValueError):
        O.box_mesh(VC.cap_grid(0)[0], np.zeros((1, 3), np.int32))


# ---- (c) the reference's behaviour (g19) ---------------------------------------------------------------------------------------------------
def test_g19_script_arguments_text_voxels_and_mesh(host_lib, g19, tmp_path):
    from icepy4d_amd import voxelization as VX
    assert g19["voxel_size"].tolist() == [0.2] == [VX.VOXEL_SIZE] and g19["bb_min"].dtype == np.float64 and g19["bb_max"].dtype == np.float64
    assert g19["bb_min"].tolist() == [-100.0, 130.0, 60.0] == list(VX.BB_MIN) and g19["bb_max"].tolist() == [30.0, 330.0, 120.0] == list(VX.BB_MAX)
    assert g19["text_name"].tobytes().decode() == f"dense_2022_05_01_voxel_{VX.VOXEL_SIZE}m.txt"
    grid = VG.make_grid(g19["bb_min"], g19["bb_max"], 0.2)
    colors = g19["colors_u8"] / 255.0
    got = host_voxels(host_lib, g19["points"], grid, colors)
    assert np.array_equal(got["grid_index"], g19["grid_index"]) and same(got["colors"], g19["voxel_colors"]) and np.array_equal(got["counts"], g19["counts"])
    assert got["dropped"] == 120 and len(got["counts"]) == 780
    vg = VG.VoxelGrid(grid, got)
    VG.write_voxel_centers(tmp_path / "out.txt", vg)
    assert (tmp_path / "out.txt").read_bytes() == g19["text"].tobytes()
    assert vg.has_colors() and len(vg.get_voxels()) == 780 and same(vg.get_voxel_center_coordinate(vg.get_voxels()[5].grid_index), got["centres"][5])
    lo, hi = vg.get_axis_aligned_bounding_box()
    assert (lo <= got["points"].min(0)).all() and (hi >= got["points"].max(0)).all() and same(vg.centers(), got["centres"])
    # The script's chain gives, per corner c = grid_index + d: ((d + (index - 0.5)) + 0.5) * s + origin. The centre of create_box's
    # vertices is 4 / 8 = 0.5 exactly, d + (index - 0.5) and + 0.5 are sums of small multiples of 0.5 (exact), scale(s, 0) is one
    # rounding of c * s (then - 0 and + 0, exact) and the last translate one rounding of the sum: the two roundings of origin + c * s. So
    # the positions are EQUAL, not within 1 ulp of |origin| + n s, and they are compared as sets of rows (the stub's order is first
    # occurrence).
    _, vert, vcol, tri = host_mesh(host_lib, grid, got["grid_index"], got["colors"])
    assert len(vert) == len(g19["mesh_vertices"]) == 1791 and len(tri) == len(g19["mesh_triangles"]) == 12 * 780
    mine = {v.tobytes(): c for v, c in zip(vert, vcol)}
    theirs = {v.tobytes(): c for v, c in zip(g19["mesh_vertices"], g19["mesh_vertex_colors"])}
    assert set(mine) == set(theirs) and len(mine) == len(vert)
    assert all(same(mine[k], theirs[k]) for k in mine)
    assert same(vert[tri], g19["mesh_vertices"][g19["mesh_triangles"]])                                     # triangle by triangle the same corners


# ---- (d) refusals before any device work ---------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_device():
    from icepy4d_amd import voxelization as VX
    from icepy4d_amd.core import PointCloud
    from icepy4d_amd.utils.point_cloud_filters import voxel_down_sample
    a = np.zeros((4, 3))
    for s in (0.0, -0.2, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            VG.VoxelGrid.create_from_point_cloud_within_bounds(a, s, (0, 0, 0), (1, 1, 1))
        with pytest.raises(ValueError):
            VG.VoxelGrid.create_from_point_cloud(a, s)
        with pytest.raises(ValueError):
            voxel_down_sample(a, s)
        with pytest.raises(ValueError):
            PointCloud(points3d=a).voxel_down_sample(s)
        with pytest.raises(ValueError):
            VX.voxel_series([a], s)
    for lo, hi in (((0, 0, 0), (1, -1, 1)), ((0, 0, np.nan), (1, 1, 1)), ((0, 0, 0), (np.inf, 1, 1)), ((0, 0), (1, 1, 1)), ((0, 0, 0), (2.0 ** 21, 2.0 ** 21, 2.0 ** 20))):
        with pytest.raises(ValueError):
            VG.VoxelGrid.create_from_point_cloud_within_bounds(a, 1.0, lo, hi)
        with pytest.raises(ValueError):
            VX.voxel_series([a], 1.0, lo, hi)
    with pytest.raises(ValueError):
        VG.VoxelGrid.create_from_point_cloud_within_bounds(np.zeros((4, 2)), 1.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        VG.VoxelGrid.create_from_point_cloud_within_bounds(a, 1.0, (0, 0, 0), (1, 1, 1), colors=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        voxel_down_sample(a, 1.0, normals=np.zeros((4, 2)))
    with pytest.raises(ValueError):
        VX.voxelize([a])                                                 # nowhere to write
    assert VX.voxel_series([]) == []
    cap = VC.cap_grid(0)[0]
    vg = VG.VoxelGrid(cap, {"grid_index": np.zeros((1, 3), np.int32), "counts": np.ones(1, np.int32), "dropped": 0, "colors": None})
    with pytest.raises(ValueError):
        vg.to_box_mesh()                                                 # 2^62 voxels, more corner keys
    assert not vg.has_colors() and vg.colors.tolist() == [[0.0, 0.0, 0.0]]
    with pytest.raises(ValueError):
        VG._batches([5, 11, 3], 10)
    assert VG._batches([5, 5, 3, 0, 10], 10) == [[0, 1], [2, 3], [4]]


# ---- (e) ABI, scratch layout, resources, imports, the mesh writer --------------------------------------------------------------------------
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
    assert "-77" in header
    lib = _lib.load()
    assert lib.im_voxel_max_points() == O.MAX_POINTS == host_lib.vox_host_max_points() == VG.max_points()
    assert host_lib.vox_host_max_mesh_items() == O.MAX_MESH_ITEMS == VG.MAX_MESH_ITEMS and VG.MAX_CELLS == O.MAX_CELLS


def test_scratch_layouts_are_pinned(host_lib):
    def up256(b):
        return (b + 255) // 256 * 256

    def blocks_of(n, per):
        return (n + per - 1) // per

    for E, G, n in ((1, 0, 0), (1, 1, 1), (3, 1, 255), (3, 3, 256), (100, 100, 100003), (65535, 65535, 2 ** 26)):
        want = (up256((2 * (E + 1) + 3 * G) * 8) + up256(7 * G * 8) + up256(6 * E * 8) + up256((n + 1) * 4) + up256(blocks_of(n + 1, 256) * 8) + 256)
        assert host_lib.carve_voxel(E, G, n) == want, (E, G, n)
    for items in (8, 248, 256, 264, 2 ** 27):
        assert host_lib.carve_voxel_mesh(items) == up256((items + 1) * 4) + up256(items * 4) + up256(blocks_of(items + 1, 256) * 8), items


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    res = toolchain.kernel_resources(toolchain.device_listing("voxel.hip", str(tmp_path)))
    mine = {k: v for k, v in res.items() if "vox_" in k or "Vox" in k}
    assert len(mine) >= 8 + 4, sorted(res)                        # eight kernels and the two scans' templates
    for k, f in mine.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (k, dict(f))


@pytest.mark.parametrize("module", MODULES)
def test_module_imports_as_the_first_import(module):
    r = subprocess.run([sys.executable, "-c", f"import {module}"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def read_mesh_ply(path):
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").splitlines()
    assert head[:2] == ["ply", "format binary_little_endian 1.0"]
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[2])
    nf = int([h for h in head if h.startswith("element face")][0].split()[2])
    coloured = "property uchar red" in head
    vt = np.dtype([("p", "<f8", (3,))] + ([("c", "u1", (3,))] if coloured else []))
    v = np.frombuffer(raw, vt, nv, end)
    f3 = np.frombuffer(raw, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), nf, end + nv * vt.itemsize)
    assert end + nv * vt.itemsize + nf * 13 == len(raw) and (f3["n"] == 3).all()
    return v["p"], (v["c"] if coloured else None), f3["i"]


def test_mesh_and_grid_writers_round_trip(tmp_path):
    vert, vcol, tri = VC.mesh_full("block_2x2x2")
    VG.write_triangle_mesh(tmp_path / "a" / "mesh.ply", vert, vcol, tri)
    p, c, f = read_mesh_ply(tmp_path / "a" / "mesh.ply")
    assert same(p, vert) and np.array_equal(f, tri) and np.array_equal(c, np.clip(np.round(vcol * 255.0), 0, 255).astype(np.uint8))
    VG.write_triangle_mesh(tmp_path / "plain.ply", vert, None, tri)
    p, c, f = read_mesh_ply(tmp_path / "plain.ply")
    assert same(p, vert) and c is None and np.array_equal(f, tri)
    case = VC.mesh_by_name("block_2x2x2")
    vg = VG.VoxelGrid(case["grid"], {"grid_index": case["grid_index"], "counts": np.ones(8, np.int32), "dropped": 0, "colors": case["colors"]})
    VG.write_voxel_grid(tmp_path / "grid.ply", vg)
    lines = (tmp_path / "grid.ply").read_text().splitlines()
    body = lines[lines.index("end_header") + 1:]
    assert lines[1] == "format ascii 1.0" and "element vertex 8" in lines and len(body) == 2 + 8
    assert same(np.array(body[0].split(), np.float64), case["grid"][:3]) and float(body[1]) == 0.5
    rows = np.array([r.split() for r in body[2:]], np.int64)
    assert np.array_equal(rows[:, :3], case["grid_index"]) and np.array_equal(rows[:, 3:], np.round(case["colors"] * 255).astype(np.int64))
