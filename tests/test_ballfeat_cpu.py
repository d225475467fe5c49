"""The ball features without a device: the kernel's own arithmetic compiled for the host (csrc/ball_point.h through
tests/ball_host_harness.cpp) against the brute-force restatement (tests/ball_oracle.py) on the shared case list (tests/ball_cases.py), the
restatement against an independent float64 decomposition, the chain of filters of `icepy4d_amd/top_border.py` against plain numpy and
against the reference's outputs in tests/golden/g18_top_border.npz (tools/gen_golden_border.py: the reference's script with a stub
cloudComPy whose features ARE the restatement), and what the compiler made of the kernel.

Bounds. Host build against the restatement: equality of bits (quantised offsets, the ten sums, covariance, eigenvalues, normal, every
arithmetic feature) and equality of the box half-width: the same IEEE float64 operations in the same order, exact integer sums.
Restatement against np.cov(bias=True) + eigvalsh of the unquantised offsets: |d lambda| <= 4 r^2 2^-18. Each offset component moves by at
most h / 2 = r 2^-19, so each covariance entry (a mean of products of two offsets of magnitude <= r, minus a product of two means) moves
by at most about r h = r^2 2^-18; the 2-norm of a symmetric 3 x 3 perturbation is at most 3 times its largest entry, and by Weyl's
inequality so is the move of every eigenvalue; one more unit covers the float64 rounding of both sides. Normals: for the points whose
gap min(l1 - l2, l2 - l3) in the independent decomposition is at least 1e-3 r^2, |e3 x e3_ref| <= 2 * 4 r^2 2^-18 / gap (Davis-Kahan);
at most 5 % of a cloud's points (of those with three neighbours or more) may lie under that gap."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ball_cases as BC  # noqa: E402
import ball_oracle as B  # noqa: E402
import toolchain  # noqa: E402


@pytest.fixture(scope="module")
def g18():
    with np.load(B.GOLDEN, allow_pickle=False) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """tests/ball_host_harness.cpp + csrc/ball_point.h as a shared library, behind a stub <hip/hip_runtime.h>."""
    lib = toolchain.host_library(str(tmp_path_factory.mktemp("ball_host")), "ball_host_harness.cpp")
    P, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    lib.ball_host_quantise.argtypes, lib.ball_host_quantise.restype = [D, D], I
    lib.ball_host_offsets.argtypes = [P, L, L, D, P, P]
    lib.ball_host_all.argtypes = [P, L, D, P, P, P, P, P]
    lib.ball_host_rings.argtypes = [P, L, P, P, D, P]
    return lib


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- (a) the host build of ball_point.h ----------------------------------------------------------------------------------------------------
def test_the_codes_of_the_header_the_oracle_and_the_python_layer_agree(host_lib):
    from icepy4d_amd.post_processing.cloudcompare_fun import GeomFeature
    from icepy4d_amd.utils import point_cloud_filters as F
    header = open(os.path.join(ROOT, "include", "icematch.h")).read()
    codes = {name: int(v) for name, v in re.findall(r"IM_BALL_([A-Z0-9_]+) = (\d+)", header)}
    assert codes.pop("KINDS") == len(B.KINDS) == host_lib.ball_host_kinds() == len(F.BALL_KINDS) == 13
    squash = lambda s: s.replace("_", "").lower()      # noqa: E731
    assert {squash(k): v for k, v in codes.items()} == {squash(k): i for i, k in enumerate(B.KINDS)} == {squash(k): v for k, v in F.BALL_KINDS.items()}
    assert {f.name for f in GeomFeature} == set(B.KINDS) | set(F.BALL_DERIVED)
    assert host_lib.ball_host_qmax() == B.QMAX == 2 ** 18 + 1


def test_host_quantisation_equals_the_oracle(host_lib):
    rng = np.random.default_rng(0)
    for r in (2.0, 0.5, 0.15, 1e-3, 123.456):
        h = float(B.step(r))
        u = np.concatenate([rng.uniform(-r, r, 2000), [0.0, -0.0, r, -r, np.nextafter(r, 2 * r), 3 * r, -3 * r, 1e300, -1e300],
                            (np.arange(-6, 7) + 0.5) * h, (np.arange(-6, 7) + 0.5) * h * (1 + 2.0 ** -52)])          # ties go to even
        got = np.array([host_lib.ball_host_quantise(float(x), r) for x in u])
        assert np.array_equal(got, B.quantise(u, h)), r
        assert got[2000 + 2] == 2 ** 18 and got[2000 + 3] == -2 ** 18 and got[2000 + 5] == B.QMAX and got[2000 + 8] == -B.QMAX
    assert B.quantise([0.5, 1.5, 2.5, -0.5, -1.5], 1.0).tolist() == [0, 2, 2, 0, -2]


@pytest.mark.parametrize("name", BC.names())
def test_host_build_equals_the_restatement_bit_for_bit(host_lib, name):
    case = BC.by_name(name)
    p, r = case["points"], case["r"]
    n = len(p)
    want = BC.expected(name)
    sums, cov = np.full((n, 10), -7, np.int64), np.full((n, 6), -7.0)
    eig, e3, feat = np.full((n, 3), -7.0), np.full((n, 3), -7.0), np.full((n, len(B.KINDS)), -7.0)
    host_lib.ball_host_all(p.ctypes.data, n, r, sums.ctypes.data, cov.ctypes.data, eig.ctypes.data, e3.ctypes.data, feat.ctypes.data)
    assert np.array_equal(sums, want["sums"]), name
    assert np.array_equal(bits(cov), bits(want["cov"])), name
    assert np.array_equal(bits(eig), bits(want["eig"])) and np.array_equal(bits(e3), bits(want["normal"])), name
    for k, kind in enumerate(B.KINDS):
        assert np.array_equal(bits(feat[:, k]), bits(want[kind])), (name, kind)
    # the offsets themselves, and the same sums with Python integers, for a few queries
    for q in np.random.default_rng(n).integers(0, n, min(n, 4)):
        inside, off = np.full(n, -7, np.int32), np.full((n, 3), -7, np.int32)
        host_lib.ball_host_offsets(p.ctypes.data, n, int(q), r, inside.ctypes.data, off.ctypes.data)
        m, i = B.offsets(p, int(q), r)
        assert np.array_equal(inside.astype(bool), m) and np.array_equal(off[m], i[m]) and (off[~m] == 0).all(), (name, int(q))
        assert B.python_int_sums(p, int(q), r) == [int(v) for v in want["sums"][q]], (name, int(q))
        assert np.abs(i[m]).max() <= 2 ** 18
    # the box of cells: the header's binary search finds what trying R = 0, 1, 2, ... finds
    grid, dims = BC.grid(case)
    rings = np.full(n, -7, np.int32)
    host_lib.ball_host_rings(p.ctypes.data, n, grid.ctypes.data, dims.ctypes.data, r, rings.ctypes.data)
    R, falls_back = BC.expected_walk(name)
    assert np.array_equal(rings, R), name
    assert int(np.prod(dims.astype(np.int64))) <= 2 ** 24
    # the cases are what they claim
    count = want["count"]
    checks = {"whole_cloud": lambda: (count == n).all(), "only_query": lambda: (count == 1).all() and np.isnan(want["Linearity"]).all(),
              "coincident": lambda: (count[-5:] == 5).all() and np.isnan(want["eig"][-5:]).all() and (count[:80] >= 2).all(),
              # the centre of 9^3: the lattice points with dx^2 + dy^2 + dz^2 <= 25 in integers, (0, 3, 4) and its kin on the boundary kept
              "lattice_r5": lambda: count[364] == sum(x * x + y * y + z * z <= 25 for x in range(-4, 5) for y in range(-4, 5) for z in range(-4, 5)),
              "exact_radius": lambda: count[0] == 9 and np.abs(B.offsets(p, 0, r)[1][1:7]).max() == 2 ** 18,
              "one_cell_700": lambda: (dims == 1).all(), "ball_5000": lambda: 4500 < count.mean() < 5200,
              "plane_x": lambda: dims[0] == 1 and dims[1] > 10 and dims[2] > 10, "line_x": lambda: dims[0] > 50 and dims[1] == 1 and dims[2] == 1,
              "far_outlier_y": lambda: falls_back.any() and not falls_back.all() and count[-1] == 1,
              "far_outlier_z": lambda: falls_back.any() and not falls_back.all(), "far_outlier_x": lambda: not falls_back.any() and dims[0] > 5000,
              "world_frame": lambda: p.min() >= 5e6 and count.mean() > 30}
    if name in checks:
        assert checks[name](), name
    if not name.startswith("far_outlier"):
        assert not falls_back.any(), name


def test_features_of_known_shapes():
    """A line, a flat square and an isotropic blob: the formulas give what their names say."""
    t = np.linspace(-1, 1, 201)
    mid = 100
    f = B.ball_features(np.column_stack([t, 0 * t, 0 * t]), 0.5)
    assert f["Linearity"][mid] == 1.0 and f["Planarity"][mid] == 0.0 and f["Sphericity"][mid] == 0.0 and f["PCA1"][mid] == 1.0
    f = B.ball_features(np.column_stack([t, 2 * t, 0.5 * t]), 0.5)        # tilted: collinear up to the quantisation, (2^-18)^2 of l1
    assert 0.0 <= 1.0 - f["Linearity"][mid] < 1e-10 and f["Anisotropy"][mid] > 1.0 - 1e-10
    g = np.linspace(-1, 1, 21)
    square = np.column_stack([np.repeat(g, 21), np.tile(g, 21), np.zeros(441)])
    f = B.ball_features(square, 0.55)
    c = 220
    assert f["Verticality"][c] == 0.0 and f["EigenValue3"][c] == 0.0 and abs(f["Linearity"][c]) < 1e-12 and abs(f["Planarity"][c] - 1) < 1e-12
    assert np.array_equal(f["normal"][c], [0.0, 0.0, 1.0]) and f["NumberOfNeighbors"][c] == f["count"][c] == 97
    wall = square[:, [2, 0, 1]]                                            # the same square, vertical
    assert B.ball_features(wall, 0.55)["Verticality"][c] == 1.0
    assert B.omnivariance(np.array([[8.0, 1.0, 1.0]]))[0] == 2.0
    ent, mag = B.eigen_entropy(np.array([[1.0, 0.5, 0.0]]))
    assert ent[0] == -(0.5 * np.log(0.5)) and mag[0] == abs(0.5 * np.log(0.5))


# ---- (b) the restatement against an independent float64 decomposition ----------------------------------------------------------------------
@pytest.mark.parametrize("r", [2.0, 0.5, 0.15])
def test_restatement_against_independent_float64(r):
    pts = BC.front(2000)
    got = B.ball_features(pts, r)
    valid = np.nonzero(got["count"] >= 3)[0]
    assert len(valid) >= 0.9 * len(pts)
    bound = 4.0 * r * r * 2.0 ** -18
    worst, under, worst_n = 0.0, 0, 0.0
    for i in valid:
        u = pts[B.inside(pts, int(i), r)] - pts[i]
        assert len(u) == got["count"][i]
        w, v = np.linalg.eigh(np.cov(u.T, bias=True))
        ref = w[::-1]
        assert not np.isnan(got["eig"][i]).any()
        worst = max(worst, float(np.abs(got["eig"][i] - ref).max()))
        gap = min(ref[0] - ref[1], ref[1] - ref[2])
        if gap < 1e-3 * r * r:
            under += 1
            continue
        cross = float(np.linalg.norm(np.cross(got["normal"][i], v[:, 0])))
        assert cross <= 2.0 * bound / gap, (r, int(i), cross, gap)
        worst_n = max(worst_n, cross * gap / (2.0 * bound))
        assert abs(np.linalg.norm(got["normal"][i]) - 1.0) < 1e-14
    print(f"r = {r}: worst |d lambda| = {worst / bound:.3f} of the bound, normals {worst_n:.3f} of theirs, {under} of {len(valid)} under the gap")
    assert worst <= bound, (r, worst, bound)
    assert under <= 0.05 * len(valid), (r, under, len(valid))


# ---- (c) the filters and the golden --------------------------------------------------------------------------------------------------------
def test_filter_by_sf_value_and_the_percentile_chain_equal_plain_numpy():
    from icepy4d_amd import top_border as T
    from icepy4d_amd.post_processing.cloudcompare_fun import filter_by_sf_value
    rng = np.random.default_rng(5)
    v = rng.normal(0, 1, 500)
    v[::7] = np.nan
    got = filter_by_sf_value(v, -0.5, 0.25)
    assert got.dtype == np.int64 and got.tolist() == [i for i, x in enumerate(v) if -0.5 <= x <= 0.25]
    assert filter_by_sf_value(v, v[1], v[1]).tolist() == [1]                                          # both limits are kept
    for empty in (filter_by_sf_value([], 0, 1), filter_by_sf_value(np.full(5, np.nan), 0, 1), filter_by_sf_value(v, np.nan, 1),
                  filter_by_sf_value(v, 1, np.nan), filter_by_sf_value(v, 1, -1)):
        assert empty.shape == (0,) and empty.dtype == np.int64
    assert np.array_equal(got, B.filter_by_value(v, -0.5, 0.25))
    lo, hi = T.percentile_window(v, (95, 100))
    assert (lo, hi) == (np.nanpercentile(v, 95), np.nanpercentile(v, 100)) == tuple(B.percentile_window(v, (95, 100)))
    assert np.isnan(T.percentile_window([], (5, 95))).all() and np.isnan(T.percentile_window(np.full(4, np.nan), (5, 95))).all()
    # the chain: plain numpy, step by step
    pts = rng.uniform(0, 10, (500, 3))
    a, b = v, rng.uniform(0, 1, 500)
    b[3::11] = np.nan
    keep = np.arange(500)
    for col in (a, b):
        c = col[keep]
        keep = keep[(c >= np.nanpercentile(c, 95)) & (c <= np.nanpercentile(c, 100))]
    z = pts[keep, 2]
    keep = keep[(z >= np.nanpercentile(z, 60)) & (z <= np.nanpercentile(z, 95))]
    assert np.array_equal(T.border_indices(pts, [a, b]), keep) and len(keep) >= 1
    assert T.border_indices(pts, [np.full(500, np.nan), b]).shape == (0,)
    assert T.border_indices(np.zeros((0, 3)), [np.zeros(0), np.zeros(0)]).shape == (0,)
    assert T.border_indices(pts[:1], [a[:1], b[:1]]).tolist() == ([0] if not np.isnan(a[0] + b[0]) else [])


def test_g18_is_reproduced(g18, tmp_path):
    from icepy4d_amd import top_border as T
    from icepy4d_amd.core import PointCloud
    sig = inspect.signature(T.detect_border_by_geometry).parameters
    assert tuple(sig["radius_list"].default) == tuple(g18["args"]) == (2.0, 0.15)
    assert sig["lim_percentile"].default == (95, 100) and sig["z_percentile"].default == (60, 95)
    assert [f.name for f in T.FEATURES] == ["Linearity", "Verticality"]
    sig = inspect.signature(T.extract_glacier_border).parameters
    assert sig["ylims"].default == (224.0, 228.0) and sig["half_width"].default == 10.0
    text = bytes(g18["csv"]).decode("ascii")
    assert text.splitlines()[0] == T.HEADER
    paths = []
    for k, date in enumerate(g18["dates"]):
        pts = g18[f"points{k}"]
        border = T.border_indices(pts, [g18[f"linearity{k}"], g18[f"verticality{k}"]])
        assert np.array_equal(border, g18[f"border{k}"]), k
        colours = np.random.default_rng(k).uniform(0, 1, (len(pts), 3))
        cloud = T.select_by_index(PointCloud(points3d=pts, points_col=colours), border)
        assert np.array_equal(cloud.colors, colours[border])                                      # colours follow the points
        paths.append(tmp_path / f"border_{date}.ply")
        cloud.write_ply(paths[-1])
    table = T.border_table(paths, out_path=tmp_path / "out" / "top_border_coords.txt")
    assert (tmp_path / "out" / "top_border_coords.txt").read_text() == text                      # the rows equal as text
    assert list(table.columns) == T.HEADER.split(",") and table["date"].tolist() == [str(d) for d in g18["dates"]]
    assert table["pcd_name"].tolist() == [p.name for p in paths]
    row = text.splitlines()[1].split(",")
    assert f"{table['x_mean'][0]:.3f}" == row[2] and f"{table['z_std'][0]:.3f}" == row[10]
    # a sample of the stored scalar fields is the restatement's, ball by ball
    pts = np.array(g18["points0"])
    for q in (0, 1234, 5999):
        S = np.array([B.python_int_sums(pts, q, 2.0)], np.int64)
        eig, e3 = B.finish(S, 2.0)
        assert bits(B.features(eig, e3, S[:, 0])["Linearity"])[0] == bits(g18["linearity0"])[q]


def test_an_empty_border_gives_the_nan_row(tmp_path):
    from icepy4d_amd import top_border as T
    from icepy4d_amd.core import PointCloud
    outside = PointCloud(points3d=np.array([[1.0, 100.0, 3.0], [2.0, 300.0, 4.0]]))
    stats = T.extract_glacier_border(outside)
    assert stats["n"] == 0 and np.isnan(stats["x_mean"]) and np.isnan(stats["z_std"])
    assert T.format_row("border_x.ply", "x", stats) == "border_x.ply,x" + ",NaN" * 9
    inside = np.array([[0.0, 225.0, 1.0], [1.0, 226.0, 2.0], [2.0, 227.0, 6.0], [50.0, 227.5, 9.0], [1.0, 229.0, 7.0]])
    stats = T.extract_glacier_border(inside)                                # y window, then median(x) = 1.5 +- 10
    assert stats["n"] == 3 and stats["x_mean"] == 1.0 and stats["z_median"] == 2.0 and stats["z_std"] == np.std([1.0, 2.0, 6.0])
    table = T.border_table([outside, inside], out_path=tmp_path / "t.csv", names=["border_a.ply", "border_b.ply"])
    lines = (tmp_path / "t.csv").read_text().splitlines()
    assert lines[0] == T.HEADER and lines[1] == "border_a.ply,a" + ",NaN" * 9 and lines[2].startswith("border_b.ply,b,1.000,1.000,")
    assert len(table) == 2 and np.isnan(table["x_mean"][0])


def test_python_layer_refuses_before_any_device_work():
    from icepy4d_amd.utils import point_cloud_filters as F
    from icepy4d_amd.post_processing.cloudcompare_fun import compute_feature
    pts = np.zeros((5, 3))
    for bad in (0.0, -1.0, np.inf, np.nan, 1e-305):
        with pytest.raises(ValueError, match="radius"):
            F.ball_features(pts, bad)
    with pytest.raises(ValueError, match="unknown features"):
        F.ball_features(pts, 1.0, features=("Roughness",))
    with pytest.raises(ValueError, match="unknown outputs"):
        F.ball_features(pts, 1.0, want=("idx",))
    with pytest.raises(ValueError, match="cell_size"):
        F.ball_features(pts, 1.0, cell_size=0.0)
    with pytest.raises(KeyError):
        compute_feature("Roughness", 1.0, pts)


# ---- (d) what the compiler made of the kernel ------------------------------------------------------------------------------------------------
def test_the_kernel_keeps_its_sums_in_registers(tmp_path):
    text = toolchain.device_listing("ballfeat.hip", str(tmp_path))
    res = toolchain.kernel_resources(text)
    name = next(k for k in res if "ball_features_kernel" in k)
    r = res[name]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0      # no per-thread array
    assert r["group_segment_fixed_size"] == 0                                                                     # no LDS
    assert r["vgpr_count"] <= 128                                                                                 # four waves per SIMD
    body = toolchain.kernel_body(text, name)
    assert body.count("v_mad_i64_i32") >= 6 and "s_barrier" not in body and "atomic" not in body
