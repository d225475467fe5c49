"""DSM and orthophoto without a device: the numpy + scipy oracle (tests/dsm_oracle.py) against the reference's own outputs
(tests/golden/g12_dsm_orthophoto.npz, tools/gen_golden_dsm.py), the kernels' own arithmetic compiled for the host (csrc/dsm_cell.h
through tests/dsm_host_harness.cpp) against the oracle on the shared case list (tests/dsm_cases.py), the case list itself, and the host
side of the public API (validation, no CPU fallback).

Bounds. Host build against the oracle: equality of bits on every binned x / y / z and the group count, every grid cell and its winning
triangle, every projection, colour and orthophoto byte: the same IEEE operations in the same order; the host build is for plain x86-64
without fused multiply-add, so a lost `#pragma clang fp contract(off)` shows on the device only (tests/test_gpu_dsm_edges.py). NaNs
included: the host build and numpy run on one processor and agree in the sign and payload of every NaN too."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dsm_cases as DC  # noqa: E402
import dsm_oracle as O  # noqa: E402
import toolchain  # noqa: E402


@pytest.fixture(scope="module")
def g12():
    return O.load_g12(os.path.join(ROOT, "tests", "golden", "g12_dsm_orthophoto.npz"))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """tests/dsm_host_harness.cpp + csrc/dsm_cell.h as a shared library, behind a stub <hip/hip_runtime.h>."""
    lib = toolchain.host_library(str(tmp_path_factory.mktemp("dsm_host")), "dsm_host_harness.cpp")
    P, I, L, D, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_float
    lib.dsm_host_win_none.argtypes, lib.dsm_host_win_none.restype = [], I
    lib.dsm_host_floor_index.argtypes, lib.dsm_host_floor_index.restype = [F], L
    lib.dsm_host_to_u8.argtypes, lib.dsm_host_to_u8.restype = [D], ctypes.c_ubyte
    lib.dsm_host_round.argtypes, lib.dsm_host_round.restype = [P, L, F, P, P, P, P, P], None
    lib.dsm_host_group_mean.argtypes, lib.dsm_host_group_mean.restype = [P, P, P, P, P, P, L, P, P, P], L
    lib.dsm_host_rasterize.argtypes, lib.dsm_host_rasterize.restype = [P, P, P, P, P, L, P, P, I, P, I, D, D, D, D, D, P, P], L
    lib.dsm_host_project_colors.argtypes = [P, L, L, P, L, L, P, L, L, I, I, I, P, P, I, I, I, P, I, P, P, P]
    lib.dsm_host_project_colors.restype = None
    return lib


def camera(g, dist="d5"):
    return types.SimpleNamespace(K=g["cam_K"], dist=g["dist_" + dist], R=g["cam_R"], t=g["cam_t"])


@pytest.mark.parametrize("case", O.G12_CASES)
def test_oracle_equals_reference_dsm(g12, case):
    pts, step, xlim, ylim, fill, xq, yq = O.g12_case(g12, case)
    r = O.build_dsm(pts, step, xlim, ylim, fill)
    for k in ("bx", "by", "bz"):
        assert O.bits_equal(r[k], g12[f"{case}_{k}"]), k
    ref = g12[case + "_z"]
    assert ref.shape == (len(yq), len(xq)) and ref.dtype == np.float64
    assert np.array_equal(np.isnan(r["z"]), np.isnan(ref))
    assert O.bits_equal(r["z"], ref)


def test_fixture_covers_the_cases(g12):
    """Signed zero keys, an all-NaN group, fills of every kind, a footprint that leaves the image, black cells."""
    assert np.signbit(g12["neg_bx"][g12["neg_bx"] == 0]).any() or np.signbit(g12["neg_by"][g12["neg_by"] == 0]).any()
    assert np.isnan(g12["nanz_bz"]).any() and np.isnan(g12["s05_z"]).any() and not np.isnan(g12["narrow_z"]).any()
    assert (g12["wide_z"] == -9999.0).any() and not np.isnan(g12["wide_z"]).any() and not np.isnan(g12["s1_z"]).any()
    assert (g12["ortho"] == 0).all(axis=2).any() and (g12["ortho"] > 0).any()
    p = g12["pc_proj_d5"]
    assert ((p[:, 0] < 0) | (p[:, 0] >= g12["image"].shape[1])).any()


def test_oracle_equals_reference_orthophoto(g12):
    pts, step, xlim, ylim, fill, xq, yq = O.g12_case(g12, "s05")
    xx, yy = np.meshgrid(xq, yq)
    c = camera(g12)
    o = O.orthophoto(xx, yy, g12["s05_z"], g12["image"], c.K, c.dist, c.R, c.t)
    assert O.bits_equal(o, g12["ortho"])


@pytest.mark.parametrize("dist", O.G12_DISTS)
def test_oracle_equals_reference_colours(g12, dist):
    c = camera(g12, dist)
    assert O.bits_equal(O.project_points(g12["pc_points"], c.K, c.dist, c.R, c.t), g12["pc_proj_" + dist])
    cols = O.interpolate_point_colors(g12["pc_points"], g12["image"], c.K, c.dist, c.R, c.t)
    assert O.bits_equal(cols, g12["pc_cols_" + dist])
    if dist == "d5":
        bgr = O.interpolate_point_colors(g12["pc_points"], g12["image"], c.K, c.dist, c.R, c.t, convert_BRG2RGB=False)
        assert O.bits_equal(bgr, g12["pc_cols_d5_bgr"])


def test_uint8_cast_matches_numpy(host_lib):
    edge = np.array([2.0 ** 31, -2.0 ** 31, 2.0 ** 31 + 1.0, -2.0 ** 31 - 1.0, 2.0 ** 31 - 1.0, 2.0 ** 31 - 0.5, -2.0 ** 31 - 0.5])
    a = np.concatenate([[-1.5, -0.7, 0.0, 0.99, 127.5, 255.9, 256.2, 511.0, 1e10, -1e10, np.nan, np.inf, -np.inf, 2.0 ** 32 + 77.0, -300.5],
                        edge, np.nextafter(edge, np.inf), np.nextafter(edge, -np.inf)])
    with np.errstate(invalid="ignore"):
        want = np.uint8(a)
    assert np.array_equal(O.to_uint8(a), want)
    assert [host_lib.dsm_host_to_u8(float(v)) for v in a] == want.tolist()


def test_floor_index_matches_numpy(host_lib):
    """np.floor(float32).astype(int64): valid below 2^63 in magnitude, INT64_MIN beyond and for NaN."""
    f = np.array([0.0, -0.0, 0.5, -0.5, -1.0, 5.99, 2.0 ** 31, -2.0 ** 31 - 256, 1e12, DC.KERNEL_BOUND, -DC.KERNEL_BOUND, DC.BELOW_TWO63,
                  -DC.BELOW_TWO63, DC.TWO63, -DC.TWO63, 1e30, -1e30, np.inf, -np.inf, np.nan], np.float32)
    with np.errstate(invalid="ignore"):
        want = np.floor(f).astype(np.int64)
    assert want[11] == 2 ** 63 - 2 ** 39 and want[13] == want[-1] == -2 ** 63
    assert [host_lib.dsm_host_floor_index(v) for v in f] == want.tolist()


# ---- the host build of csrc/dsm_cell.h against the oracle, bit for bit, on the shared case list (tests/dsm_cases.py) ---------------------
PREFILL = 0x5A


def out(shape, dtype):
    return np.frombuffer(bytes([PREFILL]) * (int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize), dtype).reshape(shape).copy()


def host_bin(lib, points, step):
    """The binning through the host build: the header's keys, numpy's stable sorts where the device uses torch's."""
    pts = np.ascontiguousarray(points, np.float64)
    n = len(pts)
    xr, yr = out(n, np.float32), out(n, np.float32)
    xykey, ykey, zkey = out(n, np.int64), out(n, np.int64), out(n, np.int64)
    lib.dsm_host_round(pts.ctypes.data, n, float(np.float32(step)), xr.ctypes.data, yr.ctypes.data, xykey.ctypes.data, ykey.ctypes.data, zkey.ctypes.data)
    pa = np.argsort(ykey, kind="stable")
    pb = np.ascontiguousarray(pa[np.argsort(zkey[pa], kind="stable")])
    pc = np.ascontiguousarray(pb[np.argsort(xykey[pb], kind="stable")])
    bx, by, bz = out(n, np.float32), out(n, np.float32), out(n, np.float32)
    G = lib.dsm_host_group_mean(pts.ctypes.data, xr.ctypes.data, yr.ctypes.data, xykey.ctypes.data, pb.ctypes.data, pc.ctypes.data, n,
                                bx.ctypes.data, by.ctypes.data, bz.ctypes.data)
    assert (bx[G:].view(np.uint8) == PREFILL).all() and (bz[G:].view(np.uint8) == PREFILL).all()
    return (bx[:G], by[:G], bz[:G]), (xr, yr)


def host_raster(lib, c):
    ny, nx = len(c["yq"]), len(c["xq"])
    z, win = out((ny, nx), np.float64), out((ny, nx), np.int32)
    spans = lib.dsm_host_rasterize(c["bx"].ctypes.data, c["by"].ctypes.data, c["bz"].ctypes.data, c["simplices"].ctypes.data, c["transform"].ctypes.data,
                                   len(c["simplices"]), c["bounds"].ctypes.data, c["xq"].ctypes.data, nx, c["yq"].ctypes.data, ny, float(c["xq"][0]),
                                   abs(c["step"]), float(c["yq"][0]), abs(c["step"]), c["fill"], z.ctypes.data, win.ctypes.data)
    return z, win, spans


def host_colours(lib, c, chmap, mode):
    """`im_project_colors` through the host build: 'points' (one row of n points, z's NaN goes through the arithmetic), 'dense' and
    'broadcast' (a grid of cells with full planes, or with the axes' own strides (0, 1) / (1, 0))."""
    rows, cols = c["z"].shape
    n, cout = rows * cols, len(chmap)
    proj, col, ortho = out((n, 2), np.float32), out((n, cout), np.float64), out((n, 3), np.uint8)
    im = c["image"]
    tail = (c["cam"].ctypes.data, im.ctypes.data, im.shape[0], im.shape[1], im.shape[2], chmap.ctypes.data, cout, proj.ctypes.data, col.ctypes.data,
            ortho.ctypes.data if cout == 3 else None)
    if mode == "points":
        pts = DC.colour_points(c)
        b = pts.ctypes.data
        lib.dsm_host_project_colors(b, 0, 3, b + 8, 0, 3, b + 16, 0, 3, 1, n, 0, *tail)
    elif mode == "dense":
        gx, gy = (np.ascontiguousarray(a) for a in np.meshgrid(c["xq"], c["yq"]))
        lib.dsm_host_project_colors(gx.ctypes.data, cols, 1, gy.ctypes.data, cols, 1, c["z"].ctypes.data, cols, 1, rows, cols, 1, *tail)
    else:
        lib.dsm_host_project_colors(c["xq"].ctypes.data, 0, 1, c["yq"].ctypes.data, 1, 0, c["z"].ctypes.data, cols, 1, rows, cols, 1, *tail)
    return proj, col, ortho


def check_colours(got, want, z, cells, what):
    """Outputs against the oracle's; in cell mode the items with a NaN z keep their pre-fill in proj and col and are black."""
    proj, col, ortho = got
    wproj, wcol, wortho = want
    live = np.ones(len(wproj), bool) if not cells else ~np.isnan(z.ravel())
    assert O.bits_equal(proj[live], wproj[live]) and O.bits_equal(col[live], wcol[live]), what
    assert (proj[~live].view(np.uint8) == PREFILL).all() and (col[~live].view(np.uint8) == PREFILL).all(), what
    if wortho is None:
        assert (ortho == PREFILL).all(), what
    else:
        assert np.array_equal(ortho, wortho), what                  # as a point a NaN z makes NaN colours, and those are black too


@pytest.mark.parametrize("name", DC.binning_names())
def test_host_build_equals_the_oracle_binning(host_lib, name):
    c = DC.binning_case(name)
    (bx, by, bz), (xr, yr) = host_bin(host_lib, c["points"], c["step"])
    assert O.bits_equal(xr, O.round_to_step(c["points"][:, 0], c["step"])) and O.bits_equal(yr, O.round_to_step(c["points"][:, 1], c["step"]))
    wx, wy, wz = DC.binned(name)
    assert len(bx) == len(wx), (len(bx), len(wx))
    assert O.bits_equal(bx, wx) and O.bits_equal(by, wy) and O.bits_equal(bz, wz)


@pytest.mark.parametrize("name", DC.raster_names())
def test_host_build_equals_the_oracle_raster(host_lib, name):
    c = DC.raster_case(name)
    z, win, spans = host_raster(host_lib, c)
    assert spans == DC.spans_of(c)
    assert O.bits_equal(z, DC.raster_expected(name)), int((z != DC.raster_expected(name)).sum())
    gx, gy = np.meshgrid(c["xq"], c["yq"])
    s = O.lowest_simplex(c["transform"], gx.ravel(), gy.ravel())
    assert np.array_equal(np.where(win.ravel() == host_lib.dsm_host_win_none(), -1, win.ravel()), s)


@pytest.mark.parametrize("name", DC.colour_names())
def test_host_build_equals_the_oracle_colours(host_lib, name):
    c = DC.colour_case(name)
    for k, chmap in enumerate(c["chmaps"]):
        want = DC.colour_expected(name, k)
        for mode in ("points", "dense", "broadcast"):
            check_colours(host_colours(host_lib, c, chmap, mode), want, c["z"], mode != "points", (name, k, mode))


def test_the_cases_are_what_they_claim():
    """The case lists themselves: the sizes and properties the kernels' paths turn on are really there."""
    # binning
    b = {n: DC.binned(n) for n in DC.binning_names()}
    for G in (1, 255, 256, 257):
        assert len(b[f"groups_{G}"][0]) == G
    assert len(b["one_bin_257"][0]) == 1 and len(DC.binning_case("one_bin_257")["points"]) == 257
    assert len(b["n65537"][0]) > 256 and len(DC.binning_case("n65537")["points"]) == 65537
    h = DC.binning_case("half_step_ties")
    t = h["points"][:, 0].astype(np.float32) / np.float32(0.5)
    assert np.array_equal(np.abs(t - np.trunc(t)), np.full(len(t), 0.5)) and len(b["half_step_ties"][0]) < 64
    for axis in (0, 1):
        neg, pos = b[f"zero_key_{'xy'[axis]}_neg_first"][axis], b[f"zero_key_{'xy'[axis]}_pos_first"][axis]
        assert (neg == 0).sum() == 1 and np.signbit(neg[neg == 0]).all() and (pos == 0).sum() == 1 and not np.signbit(pos[pos == 0]).any()
    assert np.isnan(b["all_nan_group"][2]).sum() == 2 and not np.isnan(b["nan_z_in_group"][2]).any()
    assert np.isinf(b["inf_in_group"][2]).all() and np.isnan(b["inf_and_minf"][2][0]) and b["inf_and_minf"][2][1] == 2.5
    sz = b["signed_zero_z"][2]
    assert (sz == 0).all() and not np.signbit(sz).any()                                        # a Kahan sum from +0.0 never ends at -0.0
    eq = DC.binning_case("equal_z_in_a_bin")["points"]
    assert b["equal_z_in_a_bin"][2][0] != np.float32(eq[:7, 2].sum() / 7)                      # the Kahan order is not the naive sum
    w = DC.binning_case("world_frame_1e6")
    exact = np.unique(np.round(w["points"][:, :2] / 0.1), axis=0)
    assert len(b["world_frame_1e6"][0]) < len(exact)                                            # float32 merges bins float64 keeps apart
    assert DC.binning_case("negative_step")["step"] < 0 and len(b["negative_step"][0]) > 10
    t = DC.binning_case("float64_next_to_a_tie")["points"][:, 0]
    assert (t.astype(np.float32).astype(np.float64) != t).any() and (np.round(t / 0.5) != np.round(t.astype(np.float32) / np.float32(0.5))).any()
    # raster
    share, inside = DC.non_unique_share(DC.raster_case("lattice_step_1"))
    assert share == 1.0 and inside >= 100
    assert DC.non_unique_share(DC.raster_case("lattice_step_05"))[0] >= 0.5
    assert DC.non_unique_share(DC.raster_case("lattice_step_025"))[0] >= 0.3
    for T in (1, 2, 255, 256, 257, 65537):
        c = DC.raster_case(f"strip_{T}" + ("_cropped" if T == 65537 else ""))
        assert len(c["simplices"]) == T and not np.isnan(DC.raster_expected(c["name"])).all()
    c = DC.raster_case("strip_65537_cropped")
    r0, r1 = O.span_rows(c["by"], c["simplices"], c["transform"], float(c["yq"][0]), c["step"], len(c["yq"]))
    live = np.flatnonzero(r1 >= r0)
    assert c["xq"].shape == c["yq"].shape == (8,) and 0 < len(live) < 40 and live[0] > 30000 and live[-1] < 36000
    c = DC.raster_case("strip_65537_far_end")
    r0, r1 = O.span_rows(c["by"], c["simplices"], c["transform"], float(c["yq"][0]), c["step"], len(c["yq"]))
    live = np.flatnonzero(r1 >= r0)
    gx, gy = np.meshgrid(c["xq"], c["yq"])
    assert live[-1] == 65536 and live[0] > 65500 and (O.lowest_simplex(c["transform"], gx.ravel(), gy.ravel()) == 65536).sum() >= 4
    zoo = DC.raster_case("zoo")
    r0, r1 = O.span_rows(zoo["by"], zoo["simplices"], zoo["transform"], float(zoo["yq"][0]), zoo["step"], len(zoo["yq"]))
    empty = r1 < r0
    assert empty[0] and empty[-2:].all() and empty[4:7].all() and not empty[3] and not empty[7]
    assert np.isnan(zoo["transform"][2]).all() and np.isnan(zoo["transform"][9]).all() and not np.isnan(zoo["transform"][[1, 3]]).any()
    gx, gy = np.meshgrid(zoo["xq"], zoo["yq"])
    s = O.lowest_simplex(zoo["transform"], gx.ravel(), gy.ravel())
    assert {1, 3, 7, 8, 11} <= set(s.tolist()) and 12 not in s and 10 not in s                # 12 repeats 11; 10 lies between two grid rows
    both = O.lowest_simplex(zoo["transform"][8:9], gx.ravel(), gy.ravel()) == 0
    assert (s[both] == 7).any() and (s[both] == 8).any()                                        # the overlap goes to the lower index
    inside = DC.raster_expected("zoo_bounds_inside")
    assert ((inside == -9999.0) & ~np.isnan(DC.raster_expected("zoo"))).any()                   # in a triangle, outside the bounds: fill
    assert np.isnan(DC.raster_expected("zoo_nan_vertex")).sum() > np.isnan(DC.raster_expected("zoo")).sum()
    assert (DC.raster_expected("zoo_fill_zero") == 0.0).any()
    assert DC.raster_expected("grid_1x1").shape == (1, 1) and DC.raster_expected("grid_1xN").shape == (1, 16) and DC.raster_expected("grid_Nx1").shape == (12, 1)
    assert (DC.raster_expected("xlim_outside") == -9999.0).all() and (DC.raster_expected("ylim_outside") == 0.0).all()
    st = DC.raster_case("stride_256_cus")
    assert DC.spans_of(st) > 16 * 256 * 256 and len(st["xq"]) == 3 and not np.isnan(DC.raster_expected("stride_256_cus")).any()
    beyond, inside = DC.second_turn_cells(st, 256)
    assert beyond == inside == len(st["xq"]) * len(st["yq"])                                   # every cell is won in a second turn of the loop
    for cus in (64, 304):
        other = DC.stride_case(cus)
        assert DC.second_turn_cells(other, cus)[0] == len(other["xq"]) * len(other["yq"]) and DC.spans_of(other) > 16 * 256 * cus
    # colours
    p = DC.probe_positions(6)
    for v in (5.0, 6.0, -1.0, -0.5, DC.KERNEL_BOUND, DC.BELOW_TWO63, DC.TWO63, -DC.BELOW_TWO63, -DC.TWO63, 2.0 ** 31):
        assert v in p
    assert np.isnan(p).any() and np.signbit(p[p == 0]).any() and not np.signbit(p[p == 0]).all()
    proj, col, ortho = DC.colour_expected("probe_cin3", 0)
    live = (DC.colour_case("probe_cin3")["z"].ravel() == 1.0) & np.repeat(np.abs(p) < 1e38, len(p)) & np.tile(~np.isnan(p), len(p))
    with np.errstate(over="ignore"):
        assert np.array_equal(proj[live, 0], np.tile(p.astype(np.float32), len(p))[live])                # u is X itself (-0.0 reads +0.0)
        assert np.array_equal(proj[live, 1], np.repeat(p.astype(np.float32), len(p))[live])
    assert np.isinf(proj).any() and np.isnan(proj).any()
    assert (col > 1.0).any() and (col < 0.0).any()
    proj, col, ortho = DC.colour_expected("far_outside_residues", 0)
    assert (ortho[col > 1.01] > 0).sum() >= 10 and (ortho[col < -0.01] > 0).sum() >= 10                   # the uint8 cast wraps, both ways
    rz = DC.colour_expected("rational_denominator_0", 0)[0]
    assert np.isinf(rz).any() and np.isnan(rz).any()
    assert {len(m) for n in DC.colour_names() for m in DC.colour_case(n)["chmaps"]} == {1, 2, 3, 4}
    assert {DC.colour_case(n)["image"].shape[2] for n in DC.colour_names()} == {1, 3, 4}
    assert DC.colour_case("probe_image_1x1")["image"].shape == (1, 1, 3) and np.isnan(DC.colour_case("one_cell_nan_z")["z"]).all()
    assert np.count_nonzero(DC.colour_case("camera_thin_prism")["cam"][24:28]) == 4
    cam = DC.colour_expected("camera_d5", 0)[0]
    assert (cam[:, 0] < 0).any() and (cam[:, 0] >= 64).any() and (cam[:, 1] < 0).any() and (cam[:, 1] >= 48).any()
    assert ((cam[:, 0] > 1) & (cam[:, 0] < 62) & (cam[:, 1] > 1) & (cam[:, 1] < 46)).sum() > 50


def test_kahan_mean_is_not_a_naive_sum():
    v = np.array([9.561, 9.97, 10.961, 10.923, 10.45, 10.082, 9.554])
    naive = 0.0
    for x in v:
        naive += x
    assert O.kahan_group_mean(v, [0, len(v)])[0] != naive / len(v)
    assert np.isnan(O.kahan_group_mean(np.array([np.nan, np.nan, 1.0]), [0, 2, 3])[0])


def test_validation_errors_without_a_device(tmp_path):
    from icepy4d_amd.utils.dsm_orthophoto import DSM, build_dsm, generate_ortophoto
    from icepy4d_amd.sfm import interpolate_point_colors, project_points
    pts = np.random.default_rng(0).uniform(0, 10, (50, 3))
    with pytest.raises(AssertionError, match="Invalid size of input points"):
        build_dsm(np.zeros((10, 4)))
    bad = pts.copy()
    bad[3, 0] = np.nan
    with pytest.raises(ValueError):
        build_dsm(bad)
    bad[3, 0] = np.inf
    with pytest.raises(ValueError):
        build_dsm(bad)
    try:
        import rasterio  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):
            build_dsm(pts, save_path=str(tmp_path / "dsm.tif"))
        d = DSM(*np.meshgrid(np.arange(3.0), np.arange(2.0)), np.zeros((2, 3)), 1.0)
        with pytest.raises(ImportError):
            generate_ortophoto(np.zeros((4, 4, 3), np.uint8), d, types.SimpleNamespace(K=np.eye(3), dist=None, R=np.eye(3), t=np.zeros(3)),
                               save_path=str(tmp_path / "o"))
    cam = types.SimpleNamespace(K=np.eye(3), dist=np.zeros(6), R=np.eye(3), t=np.zeros(3))
    with pytest.raises(ValueError, match="distortion"):
        project_points(pts, cam)
    with pytest.raises(AssertionError, match="invalid input image"):
        interpolate_point_colors(pts, np.zeros((4, 4), np.uint8), types.SimpleNamespace(K=np.eye(3), dist=None, R=np.eye(3), t=np.zeros(3)))


def test_dsm_class_keeps_its_arrays():
    from icepy4d_amd.utils.dsm_orthophoto import DSM
    xx, yy = np.meshgrid(np.arange(3.0), np.arange(2.0))
    d = DSM(xx, yy, np.ones((2, 3)), 0.5)
    assert d.x is xx and d.y is yy and d.res == 0.5 and d.z.shape == (2, 3)


def test_no_cpu_fallback_without_device():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from icepy4d_amd.utils.dsm_orthophoto import DSM, build_dsm, generate_ortophoto
    from icepy4d_amd.sfm import interpolate_point_colors, project_points
    pts = np.random.default_rng(0).uniform(0, 10, (50, 3))
    cam = types.SimpleNamespace(K=np.eye(3), dist=None, R=np.eye(3), t=np.zeros(3))
    with pytest.raises(RuntimeError):
        build_dsm(pts)
    d = DSM(*np.meshgrid(np.arange(3.0), np.arange(2.0)), np.zeros((2, 3)), 1.0)
    with pytest.raises(RuntimeError):
        generate_ortophoto(np.zeros((4, 4, 3), np.uint8), d, cam)
    with pytest.raises(RuntimeError):
        project_points(pts, cam)
    with pytest.raises(RuntimeError):
        interpolate_point_colors(pts, np.zeros((4, 4, 3), np.uint8), cam)
