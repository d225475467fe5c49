"""The cross-cloud distances without a device: the cylinder arithmetic compiled for the host (csrc/cyl_point.h through
tests/cyl_host_harness.cpp) against the brute-force restatement (tests/cloud_distance_oracle.py) on the shared case list
(tests/cloud_distance_cases.py), the restatement against plain float64 numpy, the host logic of the Python layers, the declarations, and
what the compiler made of the kernels.

Bounds. Host build against the restatement: equality of bits (membership, projection, quantised projection, the three sums, mean, std,
dist, lod, sig, the box's half-extents): the same IEEE float64 operations in the same order, exact integer sums. A NaN equals a NaN
whatever its payload. Restatement against numpy's mean and std(ddof=1) of the unquantised projections over the same membership mask:
every projection moves by at most h / 2 (h = L 2^-18), so the mean moves by at most h / 2, plus 4 ulp of L for the float64 rounding of
both sides; a shift of every value by at most h / 2 moves the root of the sum of squared deviations by at most sqrt(n) h / 2 (triangle
inequality in R^n, the deviations' vector moves by a vector of norm <= sqrt(n) h / 2 and centring is a projection), hence the sample std
by at most sqrt(n / (n - 1)) h / 2 <= h."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cloud_distance_cases as CC  # noqa: E402
import cloud_distance_oracle as O  # noqa: E402
import toolchain  # noqa: E402

NEW_SYMBOLS = ("im_knn_cross", "im_ball_cross", "im_cyl_stats", "im_m3c2_finish")


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """tests/cyl_host_harness.cpp + csrc/cyl_point.h as a shared library, behind a stub <hip/hip_runtime.h>."""
    lib = toolchain.host_library(str(tmp_path_factory.mktemp("cyl_host")), "cyl_host_harness.cpp")
    P, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    lib.cyl_host_inside.argtypes = [P, L, P, P, D, D, P, P, P]
    lib.cyl_host_stats.argtypes = [P, L, P, P, L, D, D, P, P, P, P]
    lib.cyl_host_finish.argtypes = [P, P, P, P, L, D, D, I, P, P, P]
    lib.cyl_host_extent.argtypes = [P, D, D, P]
    for f in (lib.cyl_host_inside, lib.cyl_host_stats, lib.cyl_host_finish, lib.cyl_host_extent):
        f.restype = None
    return lib


def same(a, b):
    """Equality of bits, a NaN equal to a NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


# ---- (a) the host build of cyl_point.h ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.names())
def test_host_build_equals_the_restatement_bit_for_bit(host_lib, name):
    case = CC.by_name(name)
    p, q, nr, rho, L = case["points"], case["queries"], case["normals"], case["rho"], case["L"]
    n, m = len(p), len(q)
    want = CC.expected_cyl(name)
    count, sums, mean, sd = np.full(m, -7, np.int32), np.full((m, 2), -7, np.int64), np.full(m, -7.0), np.full(m, -7.0)
    host_lib.cyl_host_stats(p.ctypes.data, n, q.ctypes.data, nr.ctypes.data, m, rho, L, count.ctypes.data, sums.ctypes.data, mean.ctypes.data,
                            sd.ctypes.data)
    assert np.array_equal(count, want["count"]) and np.array_equal(sums, want["sums"]), name
    assert same(mean, want["mean"]) and same(sd, want["std"]), name
    assert np.array_equal(np.isnan(mean), count < 1) and np.array_equal(np.isnan(sd), count < 2), name
    # membership, projection and quantised projection of a few queries, and the box that must hold every inside point
    for i in np.random.default_rng(m).integers(0, m, min(m, 4)):
        inside, t, it = np.full(n, -7, np.int32), np.full(n, -7.0), np.full(n, -7, np.int32)
        qi, ni = q[i].copy(), nr[i].copy()                             # held: the library reads them through bare pointers
        host_lib.cyl_host_inside(p.ctypes.data, n, qi.ctypes.data, ni.ctypes.data, rho, L, inside.ctypes.data, t.ctypes.data, it.ctypes.data)
        mask, ot = O.cyl_inside(p, q[i], nr[i], rho, L)
        assert np.array_equal(inside.astype(bool), mask) and same(t, ot), (name, int(i))
        assert np.array_equal(it[mask], O.B.quantise(ot[mask], O.cyl_step(L))) and (it[~mask] == 0).all(), (name, int(i))
        assert np.abs(it).max(initial=0) <= 2 ** 18
        e = np.full(3, -7.0)
        host_lib.cyl_host_extent(ni.ctypes.data, rho, L, e.ctypes.data)
        assert same(e, O.cyl_extent(nr[i], rho, L)), (name, int(i))
    CC.expected_cyl_walk(name)                                         # asserts that no inside point lies in a cell outside the box
    assert int(np.prod(CC.grid(case)[1].astype(np.int64))) <= 2 ** 24


def test_the_cases_are_what_they_claim():
    c = CC.expected_cyl
    for axis in range(3):
        want = c(f"exact_axis{axis}")
        # cap +-L and three wall points inside with the two interior points, the four nextafter neighbours and the far corner outside
        # (the copy shifted by 100 rounds the four neighbours onto cap and wall)
        assert want["count"].tolist() == [7, 11], (axis, want["count"])
        case = CC.by_name(f"exact_axis{axis}")
        mask, t = O.cyl_inside(case["points"][:12], case["queries"][0], case["normals"][0], case["rho"], case["L"])
        assert mask.tolist() == [True, True, False, False, True, True, True, False, False, True, True, False]
        assert np.abs(t[:2]).tolist() == [1.0, 1.0]
    ob = c("exact_oblique")
    assert ob["count"][2] == 4 and ob["count"][0] >= 1                 # along -y: the origin, two wall points and the neighbour on the axis
    few = c("few_points")
    assert few["count"].tolist() == [4, 2, 1, 0, 5, 0, 3, 0, 0, 0]    # min_points - 1, 2, 1, 0; z axis; NaN normal; zero normal: the ball of rho; inf
    assert np.isnan(few["std"][2]) and not np.isnan(few["mean"][2]) and np.isnan(few["mean"][3]) and few["std"][1] > 0
    whole = c("whole_cloud")
    assert whole["count"].tolist() == [5200, 5200, 0]
    assert (c("long_thin")["count"] > 0).any() and CC.by_name("long_thin")["L"] == 64 * CC.by_name("long_thin")["rho"]
    # the walks: which queries give their box or their rings up
    assert CC.expected_cyl_walk("plane_x_fine").any() and not CC.expected_cyl_walk("plane_x_coarse").any()
    assert CC.expected_ball_walk("plane_x_fine").any() and not CC.expected_ball_walk("plane_x_mid").any()
    fo = CC.expected_ball_walk("far_outlier_y")
    assert fo.any() and not fo.all()
    rings = CC.expected_rings("line_x", 64, np.inf)
    assert (rings < 0).sum() >= 4 and (CC.expected_rings("line_x", 1, np.inf) > 0).all()
    assert (CC.expected_rings("far_queries", 64, np.inf) > 0).all()
    grids = {n: CC.grid(CC.by_name(n))[1].tolist() for n in ("one_cell", "line_x", "plane_x_mid")}
    assert grids["one_cell"] == [1, 1, 1] and grids["line_x"] == [5001, 1, 1] and grids["plane_x_mid"][0] == 1 and min(grids["plane_x_mid"][1:]) > 40
    idx, d2, count = CC.expected_knn("coincident", 5, np.inf)
    assert idx[0, 0] == 0 and idx[0, 1] == 40 and d2[0, 0] == 0.0 == d2[0, 1]                    # a tie: the lower index first
    assert (CC.expected_knn("coincident", 5, 0.0)[2][:11] >= 2).all() and (CC.expected_knn("n129", 64, 1.0e-12)[2] == 0).all()
    assert (CC.expected_knn("n2", 64, np.inf)[2] == 2).all() and CC.expected_knn("few_points", 3, np.inf)[2].tolist()[-2:] == [0, 0]
    assert CC.by_name("world_frame")["points"][:, 1].min() >= 4.9e6


def test_host_finish_equals_the_restatement(host_lib):
    L, f = CC.finish_inputs()
    m = len(f["count1"])
    dist, lod, sig = np.full(m, -7.0), np.full(m, -7.0), np.full(m, 7, np.uint8)
    args = [np.ascontiguousarray(f[k]) for k in ("count1", "sums1", "count2", "sums2")]
    host_lib.cyl_host_finish(*[a.ctypes.data for a in args], m, L, CC.REG_ERROR, CC.MIN_POINTS, dist.ctypes.data, lod.ctypes.data, sig.ctypes.data)
    odist, olod, osig = CC.expected_finish()
    assert same(dist, odist) and same(lod, olod) and np.array_equal(sig, osig)
    c1, c2 = f["count1"], f["count2"]
    assert np.array_equal(np.isnan(dist), (c1 < 1) | (c2 < 1)) and np.array_equal(np.isnan(lod), (c1 < CC.MIN_POINTS) | (c2 < CC.MIN_POINTS))
    assert not sig[np.isnan(lod)].any() and sig.any() and (sig == 0).any()
    for low in (0, 1, 2, CC.MIN_POINTS - 1):
        assert (c1 == low).any() and (c2 == low).any()
    both = ~np.isnan(lod)
    assert both.sum() >= 20 and (lod[both] >= 1.96 * CC.REG_ERROR).all()


# ---- (b) the restatement against plain float64 numpy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["world_frame", "front_1000", "long_thin", "whole_cloud", "n129"])
def test_restatement_against_plain_numpy(name):
    case = CC.by_name(name)
    p, q, nr, rho, L = case["points"], case["queries"], case["normals"], case["rho"], case["L"]
    got = CC.expected_cyl(name)
    h = float(O.cyl_step(L))
    ulp = 2.0 ** -52 * L
    worst_m, worst_s, seen = 0.0, 0.0, 0
    for i in range(min(len(q), 200)):
        mask, t = O.cyl_inside(p, q[i], nr[i], rho, L)
        assert mask.sum() == got["count"][i]
        if mask.sum() >= 1:
            dm = abs(got["mean"][i] - np.mean(t[mask]))
            assert dm <= h / 2 + 4 * ulp, (name, i, dm, h)
            worst_m = max(worst_m, dm / (h / 2 + 4 * ulp))
        if mask.sum() >= 2:
            ds = abs(got["std"][i] - np.std(t[mask], ddof=1))
            assert ds <= h, (name, i, ds, h)
            worst_s = max(worst_s, ds / h)
            seen += 1
    print(f"{name}: worst |d mean| = {worst_m:.3f} of its bound, worst |d std| = {worst_s:.3f} of its bound, {seen} cylinders with two points or more")
    assert seen >= 1


def test_python_integer_sums_do_not_overflow_int64():
    n = 2 ** 26
    assert n * (2 ** 18 + 1) ** 2 < 2 ** 63


# ---- (c) the Python layers' host logic -------------------------------------------------------------------------------------------------------
def test_orientation_flips_and_unit_normals():
    from icepy4d_amd.post_processing import cloud_distance as D
    rng = np.random.default_rng(3)
    n = rng.normal(0, 1, (50, 3))
    n[0] = (0.0, 0.0, 0.0)
    u = D.unit_normals(n)
    ln = np.sqrt(((n[:, 0] * n[:, 0]) + (n[:, 1] * n[:, 1])) + (n[:, 2] * n[:, 2]))
    assert np.isnan(u[0]).all() and same(u[1:], n[1:] / ln[1:, None])
    core = rng.uniform(0, 10, (50, 3))
    up = D.orient_normals(u, core, orientation=(0, 0, 1))
    dot = ((u[:, 0] * 0.0) + (u[:, 1] * 0.0)) + (u[:, 2] * 1.0)
    assert same(up, np.where((dot < 0)[:, None], -u, u)) and (up[1:, 2] >= 0).all() and np.isnan(up[0]).all()
    assert same(np.abs(up), np.abs(u))                                  # flipping is exact
    down = D.orient_normals(u, core, orientation=(0, 0, -1))
    assert same(down[1:], -up[1:])
    view = np.array([5.0, 5.0, 100.0])
    o = view - core
    dot = ((u[:, 0] * o[:, 0]) + (u[:, 1] * o[:, 1])) + (u[:, 2] * o[:, 2])
    assert same(D.orient_normals(u, core, viewpoint=view), np.where((dot < 0)[:, None], -u, u))
    flat = np.array([[1.0, 0.0, 0.0]])
    assert same(D.orient_normals(flat, core[:1], orientation=(0, 0, 1)), flat)                   # a zero product does not flip


def test_m3c2_table_equals_plain_numpy(tmp_path):
    from icepy4d_amd import change_detection as C
    from icepy4d_amd.post_processing.cloud_distance import M3C2Result
    rng = np.random.default_rng(4)
    results = []
    for m in (40, 1, 0):
        dist = rng.normal(0.1, 0.2, m)
        lod = np.abs(rng.normal(0.1, 0.02, m))
        dist[::7] = np.nan
        lod[::5] = np.nan
        with np.errstate(invalid="ignore"):
            sig = np.abs(dist) > lod
        z = np.zeros(m)
        results.append(M3C2Result(np.zeros((m, 3)), np.zeros((m, 3)), dist, lod, sig, z.astype(np.int32), z.astype(np.int32), z, z))
    table = C.m3c2_table(results, names=[("a", "b"), ("b", "c"), ("c", "d")], dates=[("2022-05-01", "2022-05-02")] * 3, out_path=tmp_path / "o" / "m3c2.csv")
    assert list(table.columns) == C.CSV_COLUMNS + ["date_in", "date_fin"] and len(table) == 3
    r = results[0]
    d = r.distance[r.significant]
    row = table.iloc[0]
    assert row["n_core"] == 40 and row["n_distance"] == (~np.isnan(r.distance)).sum() and row["n_significant"] == r.significant.sum() == len(d) > 2
    assert row["mean"] == np.mean(d) and row["median"] == np.median(d) and row["std"] == np.std(d, ddof=1)
    assert row["lod_mean"] == np.mean(r.lod[~np.isnan(r.lod)])
    assert table.iloc[2]["n_core"] == 0 and np.isnan(table.iloc[2]["mean"]) and np.isnan(table.iloc[2]["lod_mean"])
    lines = (tmp_path / "o" / "m3c2.csv").read_text().splitlines()
    assert lines[0] == C.HEADER and len(lines) == 4 and lines[1].startswith(f"a,b,40,{row['n_distance']},{len(d)},{np.mean(d):.4f},")
    assert lines[3] == "c,d,0,0,0,NaN,NaN,NaN,NaN"
    with pytest.raises(ValueError, match="names"):
        C.m3c2_table(results, names=[("a", "b")])


def test_python_layers_refuse_before_any_device_work():
    from icepy4d_amd import change_detection as C
    from icepy4d_amd.post_processing import cloud_distance as D
    from icepy4d_amd.utils import point_cloud_filters as F
    pts, q = np.zeros((5, 3)), np.zeros((2, 3))
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="k must be"):
            F.knn_cross(q, pts, k)
    with pytest.raises(ValueError, match="radius"):
        F.knn_cross(q, pts, 1, radius=-1.0)
    with pytest.raises(ValueError, match="unknown outputs"):
        F.knn_cross(q, pts, 1, want=("mean",))
    for bad in (0.0, -1.0, np.inf, np.nan, 1e-305):
        with pytest.raises(ValueError, match="radius"):
            F.ball_cross(q, pts, bad)
        with pytest.raises(ValueError, match="half_length"):
            F.cylinder_stats(q, q, pts, 1.0, bad)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="radius"):
            F.cylinder_stats(q, q, pts, bad, 1.0)
    with pytest.raises(ValueError, match="unknown outputs"):
        F.ball_cross(q, pts, 1.0, want=("feat",))
    with pytest.raises(ValueError, match="unknown outputs"):
        F.cylinder_stats(q, q, pts, 1.0, 1.0, want=("eig",))
    good = dict(normal_scale=1.0, search_scale=1.0, search_depth=1.0)
    for key in good:
        for bad in (0.0, -2.0, np.inf, np.nan):
            with pytest.raises(ValueError, match=key):
                D.m3c2(pts, pts, **{**good, key: bad})
    with pytest.raises(ValueError, match="registration_error"):
        D.m3c2(pts, pts, registration_error=-0.1, **good)
    for bad in (1, 0, 2.5):
        with pytest.raises(ValueError, match="min_points"):
            D.m3c2(pts, pts, min_points=bad, **good)
    with pytest.raises(ValueError, match="search_scale"):
        C.m3c2_series([pts, pts], [(0, 1)], normal_scale=1.0, search_scale=0.0, search_depth=1.0)


# ---- (d) the declarations and what the compiler made of the kernels --------------------------------------------------------------------------
def test_the_new_symbols_are_declared_and_bound():
    from icepy4d_amd import _lib
    header = open(os.path.join(ROOT, "include", "icematch.h")).read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and name in _lib.SIGNATURES, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), (name, len(m.group(1).split(",")), len(_lib.SIGNATURES[name]))
    assert "-79" in header
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW_SYMBOLS)


def test_the_query_kernels_keep_their_sums_in_registers(tmp_path):
    res = toolchain.kernel_resources(toolchain.device_listing("cloud_distance.hip", str(tmp_path)))
    for kernel in ("knn_cross_kernel", "ball_cross_kernel", "cyl_stats_kernel"):
        r = res[next(k for k in res if kernel in k)]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, kernel      # no per-thread array
        assert r["group_segment_fixed_size"] == 0, kernel                                                                 # no LDS
        assert r["vgpr_count"] <= 128, kernel                                                                             # four waves per SIMD
