"""The DEM of difference and the polygon crop (csrc/dod.hip, csrc/dod_cell.h) on the device, on every case of tests/dod_cases.py (each
size at which a kernel takes another path: see that file), through the C entry points and through `DemOfDifference` and `dod_series`, a
batch against its single-pair calls, two runs against each other, the reference's outputs in tests/golden/g17_dod.npz, the refusals, and
the crop at every polygon and cloud size around the block and the LDS stage.

Bounds. Everything is equality: cloud bounds, dropped counts, grids, keys, H and every field of the report are bit-identical to the numpy
restatement (tests/dod_oracle.py). Derived, not measured: the kernels and the restatement perform the same IEEE float64 operations in the
same order with contraction off (float64 division is correctly rounded on the device, the library is built without a fast-math flag), the
minima and maxima and the integer counts are order-free, and the order of the three sums over cells is fixed by the chunk size alone. The
host build of the same text agrees with the restatement on the same cases (tests/test_dod_cpu.py); what only this file can show is the
launch code, the segment order the sort and the scan produce, and a lost `#pragma clang fp contract(off)`: gfx950 has fused multiply-add.

Every output of a C ABI call lies between two guard bands of sentinel bytes in one allocation and is itself pre-filled; the bands must
come back untouched."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dod_cases as DC  # noqa: E402
import dod_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

BAND, SENT, FILL = 4096, 0xA5, 0x5A
REFUSED = -76


@pytest.fixture(scope="module")
def g17():
    with np.load(O.GOLDEN, allow_pickle=False) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


def p(t):
    from icepy4d_amd._lib import ptr
    return ptr(t)


def dev(eng, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(eng.device)          # a copy: the shared inputs are read-only


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Framed:
    """An output of `shape` x `dtype` between two bands of sentinel bytes, in one device allocation, pre-filled."""

    def __init__(self, eng, shape, dtype):
        import torch
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        host = np.full(2 * BAND + self.n, SENT, np.uint8)
        host[BAND:BAND + self.n] = FILL
        self.buf = torch.from_numpy(host).to(eng.device)
        self.ptr = self.buf.data_ptr() + BAND

    def result(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all(), (what, "a byte outside the output was written")
        return host[BAND:BAND + self.n].view(self.dtype).reshape(self.shape)

    def untouched(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all() and (host[BAND:BAND + self.n] == FILL).all(), what


class Series:
    """A case through the three C entry points, every output framed. `pairs`: a subset of the case's pairs (default: all)."""

    def __init__(self, eng, case, pairs=None):
        import torch
        self.case = case
        self.pts, self.offsets, all_pairs = DC.packed(case)
        self.pairs = np.ascontiguousarray(all_pairs if pairs is None else all_pairs[pairs], np.int32)
        self.E, self.P, self.d, self.s = len(self.offsets) - 1, len(self.pairs), case["d"], case["s"]
        self.d_pts = dev(eng, self.pts)
        st = eng.stream_ptr()
        name = case["name"]
        bounds, dropped = Framed(eng, (self.E, 4), np.float64), Framed(eng, (self.E,), np.int64)
        eng.ctx.call("im_dod_bounds", p(self.d_pts), self.offsets.ctypes.data, self.E, self.d, bounds.ptr, dropped.ptr, st)
        self.bounds, self.dropped = np.ascontiguousarray(bounds.result((name, "bounds"))), dropped.result((name, "dropped"))
        self.grids = np.full((self.P, 4), -7.0)
        sizes = np.diff(self.offsets)
        self.items = int(sizes[self.pairs.ravel()].sum())
        key = Framed(eng, (self.items,), np.int64)
        eng.ctx.call("im_dod_keys", *self.head(), self.grids.ctypes.data, key.ptr, st)
        self.key = key.result((name, "keys"))
        self.skey, self.perm = torch.sort(dev(eng, self.key), stable=True)
        self.n_cells = (self.grids[:, 2] * self.grids[:, 3]).astype(np.int64)
        self.H, self.report = Framed(eng, (int(self.n_cells.sum()),), np.float64), Framed(eng, (self.P, 16), np.float64)
        self.eng = eng

    def head(self):
        return (p(self.d_pts), self.offsets.ctypes.data, self.E, self.pairs.ctypes.data, self.P, self.d, self.s, self.bounds.ctypes.data)

    def reduce(self, want_H=True):
        self.eng.ctx.call("im_dod_reduce", *self.head(), p(self.skey), p(self.perm), self.H.ptr if want_H else None, self.report.ptr, self.eng.stream_ptr())
        name = self.case["name"]
        H = self.H.result((name, "H")) if want_H else None
        at = np.concatenate([[0], np.cumsum(self.n_cells)])
        rasters = [H[at[k]:at[k + 1]].reshape(int(self.grids[k, 3]), int(self.grids[k, 2])) for k in range(self.P)] if want_H else None
        return rasters, self.report.result((name, "report"))


def check_against_oracle(series, rasters, report, wants, what):
    case = series.case
    for e, cloud in enumerate(case["clouds"]):
        ob, od = O.bounds(cloud, case["d"])
        assert np.array_equal(bits(series.bounds[e]), bits(ob)) and series.dropped[e] == od, (what, "bounds of cloud", e, series.bounds[e], ob)
    seg, at, n_seg = 0, 0, 2 * int(series.n_cells.sum())
    for k, ((g, c), want) in enumerate(zip(series.pairs, wants)):
        min_x, min_y, w, h = want["grid"]
        assert np.array_equal(bits(series.grids[k]), bits([min_x, min_y, w, h])), (what, k, series.grids[k], want["grid"])
        for side, cloud in enumerate((g, c)):
            n = len(case["clouds"][cloud])
            cells = want["cells"][side]
            assert np.array_equal(series.key[at:at + n], np.where(cells >= 0, seg + cells, n_seg)), (what, k, side, "keys")
            at, seg = at + n, seg + w * h
        if rasters is not None:
            assert rasters[k].shape == want["H"].shape and np.array_equal(bits(rasters[k]), bits(want["H"])), (what, k, "H")
        assert np.array_equal(bits(report[k]), bits(want["report_row"])), (what, k, dict(zip(O.FIELDS, report[k])), want["report"])


# ---- (a) every case through the C entry points -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.names())
def test_c_entry_points_equal_the_oracle(eng, name):
    from icepy4d_amd import volume_variations as VV
    assert VV.chunk() == O.CHUNK and VV.max_cells() == O.MAX_CELLS
    series = Series(eng, DC.by_name(name))
    rasters, report = series.reduce()
    check_against_oracle(series, rasters, report, DC.full(name), name)


@pytest.mark.parametrize("name", ["batch_5_pairs_4_clouds", "batch_with_empty", "cells_3075_3x1025", "n0_n0"])
def test_report_without_rasters_and_two_runs_are_identical(eng, name):
    series = Series(eng, DC.by_name(name))
    rasters, report = series.reduce()
    again = Series(eng, DC.by_name(name))
    _, report_only = again.reduce(want_H=False)
    again.H.untouched((name, "H not asked for"))
    assert np.array_equal(bits(report_only), bits(report))
    rasters2, report2 = again.reduce()
    assert np.array_equal(again.key, series.key) and np.array_equal(bits(report2), bits(report))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(rasters, rasters2))


@pytest.mark.parametrize("name", ["batch_5_pairs_4_clouds", "batch_with_empty"])
def test_a_batch_equals_its_single_pair_calls(eng, name):
    case = DC.by_name(name)
    rasters, report = Series(eng, case).reduce()
    for k in range(len(case["pairs"])):
        r1, rep1 = Series(eng, case, pairs=[k]).reduce()
        assert np.array_equal(bits(rep1[0]), bits(report[k])) and np.array_equal(bits(r1[0]), bits(rasters[k])), (name, k)
    rev = list(range(len(case["pairs"])))[::-1]                       # and in another order
    r2, rep2 = Series(eng, case, pairs=rev).reduce()
    assert np.array_equal(bits(rep2[::-1]), bits(report)) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(r2[::-1], rasters))


# ---- (b) the same cases through the Python entry points --------------------------------------------------------------------------------------
def check_report(rep, want, what):
    from icepy4d_amd.volume_variations import FIELDS
    got = np.array([getattr(rep, k) for k in FIELDS], np.float64)
    assert np.array_equal(bits(got), bits(want["report_row"])), (what, rep.as_dict(), want["report"])
    assert (rep.droppedGround, rep.droppedCeil) == tuple(want["dropped"]), what
    assert isinstance(rep.validCells, int) and isinstance(rep.gridWidth, int)


@pytest.mark.parametrize("name", DC.names())
def test_python_entry_points_equal_the_oracle(eng, name):
    from icepy4d_amd.post_processing import DemOfDifference
    from icepy4d_amd.volume_variations import dod_series
    case, wants = DC.by_name(name), DC.full(name)
    direction = "xyz"[case["d"]]
    reports, rasters = dod_series(case["clouds"], case["pairs"], direction=direction, grid_step=case["s"], engine=eng, rasters=True)
    assert len(reports) == len(rasters) == len(wants)
    for k, want in enumerate(wants):
        check_report(reports[k], want, (name, k))
        H, origin, step = rasters[k]
        assert H.shape == want["H"].shape and np.array_equal(bits(H), bits(want["H"])) and step == case["s"], (name, k)
        assert np.array_equal(bits(origin), bits(want["grid"][:2]))
    only = dod_series(case["clouds"], case["pairs"], direction=direction, grid_step=case["s"], engine=eng)
    for k, want in enumerate(wants):
        check_report(only[k], want, (name, k, "without rasters"))
    g, c = case["pairs"][-1]
    dod = DemOfDifference((case["clouds"][g], case["clouds"][c]))
    assert dod.compute_volume(direction=direction, grid_step=case["s"], engine=eng) is True and dod.direction == case["d"]
    check_report(dod.report, wants[-1], (name, "DemOfDifference"))
    assert np.array_equal(bits(dod.grid()[0]), bits(wants[-1]["H"]))


def test_a_series_longer_than_one_batch_is_split(eng, monkeypatch):
    from icepy4d_amd import volume_variations as VV
    case, wants = DC.by_name("batch_5_pairs_4_clouds"), DC.full("batch_5_pairs_4_clouds")
    cells = wants[0]["H"].size
    monkeypatch.setattr(VV, "max_batch_cells", lambda: 2 * cells + 100)                      # two pairs per call
    reports, rasters = VV.dod_series(case["clouds"], case["pairs"], direction="x", grid_step=case["s"], engine=eng, rasters=True)
    for k, want in enumerate(wants):
        check_report(reports[k], want, k)
        assert np.array_equal(bits(rasters[k][0]), bits(want["H"]))


# ---- (c) the reference's outputs -------------------------------------------------------------------------------------------------------------
def test_g17_volume_series_through_the_python_entry_points(eng, g17, tmp_path):
    from icepy4d_amd.core import PointCloud
    from icepy4d_amd.post_processing import DemOfDifference
    from icepy4d_amd.volume_variations import FIELDS, dod_series
    paths = []
    for t, c in enumerate(g17["clouds"]):
        paths.append(str(tmp_path / f"sampled_2022_05_0{t + 1}.ply"))
        PointCloud(points3d=c).write_ply(paths[-1])
    csv = tmp_path / "out.csv"
    for k, ((g, c), args) in enumerate(zip(g17["volume_pairs"], g17["volume_args"])):
        dod = DemOfDifference((paths[g], paths[c]))
        kw = {} if k == 0 else {"direction": "xyz"[int(args[0])], "grid_step": float(args[1])}          # k == 0: the defaults, "x" and 1
        assert dod.compute_volume(engine=eng, **kw) is True
        got = np.array([getattr(dod.report, f) for f in FIELDS])
        assert np.array_equal(bits(got), bits(g17["volume_reports"][k])), k
        dod.write_result_to_file(str(csv), mode="a+", header=(k != 0))
        dod.clear()
    assert csv.read_bytes() == g17["csv_append"].tobytes()
    reports = dod_series(paths, [(0, 1)], direction="x", grid_step=1, engine=eng)
    assert np.array_equal(bits([getattr(reports[0], f) for f in FIELDS]), bits(g17["volume_reports"][0]))
    assert reports[0].droppedCeil == 1 and reports[0].droppedGround == 0


@pytest.mark.parametrize("kind", ["hexagon", "star64"])
def test_g17_filter_pcd_by_polyline(eng, g17, tmp_path, kind):
    from icepy4d_amd.core import PointCloud
    from icepy4d_amd.post_processing.cloudcompare_fun import cut_point_cloud_by_polyline
    from icepy4d_amd.post_processing.open3d_fun import filter_pcd_by_polyline
    pts, col = g17["crop_points"], g17["crop_colors"]
    np.savetxt(tmp_path / "poly.txt", g17[f"polyline_{kind}"], delimiter=" ", fmt="%.17g")
    pc = PointCloud(points3d=pts, points_col=col)
    pc.normals = pts[:, ::-1] * 0.5
    out = filter_pcd_by_polyline(pc, str(tmp_path / "poly.txt"), engine=eng)
    poly = g17[f"polygon_{kind}"]
    mask = O.in_polygon(poly, pts[:, 1], pts[:, 2])
    assert np.array_equal(out.points, pts[mask]) and np.array_equal(out.colors, col[mask]) and np.array_equal(out.normals, pts[mask][:, ::-1] * 0.5)
    d = np.full(len(pts), np.inf)
    for a, b in zip(np.roll(poly, 1, axis=0), poly):
        t = np.clip(((pts[:, 1:] - a) @ (b - a)) / ((b - a) @ (b - a)), 0.0, 1.0)
        d = np.minimum(d, np.linalg.norm(pts[:, 1:] - (a + t[:, None] * (b - a)), axis=1))
    clear = d > 1e-9
    assert (~clear).mean() <= 0.01 and np.array_equal(mask[clear], g17[f"mask_{kind}"][clear])
    assert len(pc) == len(pts)                                        # the input is left alone
    # the CloudCompare-style crop: direction "x" looks along axis 1 (the reference's swapped mapping), the polygon in file order
    ordered = np.column_stack([poly[:, 0], np.full(len(poly), 7.0), poly[:, 1]])          # a simple polygon in (x, z)
    np.savetxt(tmp_path / "xz.txt", ordered, delimiter=" ", fmt="%.17g")
    shifted = pts - (85.0, 0.0, 0.0)
    for inside in (True, False):
        cut = cut_point_cloud_by_polyline(PointCloud(points3d=shifted, points_col=col), str(tmp_path / "xz.txt"), direction="x", inside=inside, engine=eng)
        want = O.in_polygon(poly, shifted[:, 0], shifted[:, 2]) == inside
        assert np.array_equal(cut.points, shifted[want]) and np.array_equal(cut.colors, col[want]) and 0 < want.sum() < len(want)


# ---- (d) the crop at every size ---------------------------------------------------------------------------------------------------------------
def polygon(rng, nv):
    a = np.sort(rng.uniform(0, 2 * np.pi, nv))
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], 1) * rng.uniform(0.5, 1.5, (nv, 1)) + (3.0, -2.0))


@pytest.mark.parametrize("nv", [3, 4, 63, 64, 65, 1024])
def test_crop_equals_the_oracle(eng, nv):
    rng = np.random.default_rng(nv)
    poly = polygon(rng, nv)
    st = eng.stream_ptr()
    for n in (0, 1, 255, 256, 257, 5000):
        pts = np.ascontiguousarray(rng.uniform(-1.6, 1.6, (n, 3)) + (3.0, 100.0, -2.0))
        if n >= 255:
            pts[7] = (np.nan, 0.0, -2.0)
            pts[9] = (3.0, 0.0, np.inf)
            pts[11] = poly[0, 0], 5.0, poly[0, 1]                      # on a vertex: whatever the rule says, the oracle says it too
        d_pts = dev(eng, pts)
        for inside in (1, 0):
            mask, index, count = Framed(eng, (n,), np.uint8), Framed(eng, (n,), np.int64), Framed(eng, (1,), np.int64)
            eng.ctx.call("im_crop_polygon", p(d_pts), n, 0, 2, poly.ctypes.data, nv, inside, mask.ptr, index.ptr, count.ptr, st)
            want = O.in_polygon(poly, pts[:, 0], pts[:, 2]) == bool(inside)
            what = (nv, n, inside)
            m, k = mask.result(what), int(count.result(what)[0])
            assert np.array_equal(m.astype(bool), want) and set(np.unique(m).tolist()) <= {0, 1}, what
            idx = index.result(what)
            assert k == want.sum() and np.array_equal(idx[:k], np.nonzero(want)[0]) and (idx.view(np.uint8)[8 * k:] == FILL).all(), what
        if n == 5000:
            assert 0 < want.sum() < n
    from icepy4d_amd.post_processing.open3d_fun import crop_indices
    got = crop_indices(pts, poly, 0, 2, engine=eng)
    assert got.dtype == np.int64 and np.array_equal(got, np.nonzero(O.in_polygon(poly, pts[:, 0], pts[:, 2]))[0])


# ---- (e) refusals ---------------------------------------------------------------------------------------------------------------------------
def refused(eng, name, *args):
    from icepy4d_amd._lib import IcematchError
    with pytest.raises(IcematchError) as e:
        eng.ctx.call(name, *args)
    assert e.value.rc == REFUSED, (name, e.value)


def test_refusals_leave_the_outputs_alone(eng):
    case = DC.by_name("batch_5_pairs_4_clouds")
    s = Series(eng, case)
    st = eng.stream_ptr()
    E, P, d, step = s.E, s.P, s.d, s.s
    off, pairs, hb = s.offsets, s.pairs, s.bounds
    bounds, dropped = Framed(eng, (E, 4), np.float64), Framed(eng, (E,), np.int64)
    descending, shifted = off.copy(), off + 1
    descending[2] = descending[1] - 1
    for args in ((None, off.ctypes.data, E, d, bounds.ptr, dropped.ptr), (p(s.d_pts), None, E, d, bounds.ptr, dropped.ptr),
                 (p(s.d_pts), off.ctypes.data, 0, d, bounds.ptr, dropped.ptr), (p(s.d_pts), off.ctypes.data, 65536, d, bounds.ptr, dropped.ptr),
                 (p(s.d_pts), off.ctypes.data, E, -1, bounds.ptr, dropped.ptr), (p(s.d_pts), off.ctypes.data, E, 3, bounds.ptr, dropped.ptr),
                 (p(s.d_pts), off.ctypes.data, E, d, None, dropped.ptr), (p(s.d_pts), off.ctypes.data, E, d, bounds.ptr, None),
                 (p(s.d_pts), descending.ctypes.data, E, d, bounds.ptr, dropped.ptr), (p(s.d_pts), shifted.ctypes.data, E, d, bounds.ptr, dropped.ptr)):
        refused(eng, "im_dod_bounds", *args, st)
        bounds.untouched(("im_dod_bounds", args[2:4]))
        dropped.untouched(("im_dod_bounds", args[2:4]))
    oc = DC.over_the_cap()                                              # a pair one column over the cell cap, bounds from the oracle
    opts, ooff, opairs = DC.packed(oc)
    ob = np.ascontiguousarray([O.bounds(c, oc["d"])[0] for c in oc["clouds"]])
    d_opts = dev(eng, opts)
    bad_pairs = [pairs.copy() for _ in range(3)]
    bad_pairs[0][1, 0], bad_pairs[1][4, 1], bad_pairs[2][0, 0] = -1, E, 2 ** 30
    nan_bounds = hb.copy()
    nan_bounds[1, 2] = np.nan
    good = (p(s.d_pts), off.ctypes.data, E, pairs.ctypes.data, P, d, step, hb.ctypes.data)

    def variants():
        yield (None,) + good[1:]
        yield good[:1] + (None,) + good[2:]
        yield good[:3] + (None,) + good[4:]
        yield good[:7] + (None,)
        yield good[:7] + (nan_bounds.ctypes.data,)
        for bad_step in (0.0, -0.3, float("nan"), float("inf")):
            yield good[:6] + (bad_step,) + good[7:]
        for bad_d in (-1, 3):
            yield good[:5] + (bad_d,) + good[6:]
        for bp in bad_pairs:
            yield good[:3] + (bp.ctypes.data,) + good[4:]
        yield good[:1] + (descending.ctypes.data,) + good[2:]
        yield good[:2] + (0,) + good[3:]
        yield good[:4] + (-1,) + good[5:]
        yield good[:4] + (65536,) + good[5:]
        yield (p(d_opts), ooff.ctypes.data, 2, opairs.ctypes.data, 1, oc["d"], oc["s"], ob.ctypes.data)

    grids = np.full((P, 4), -7.0)
    key = Framed(eng, (s.items,), np.int64)
    H, report = Framed(eng, (int(s.n_cells.sum()),), np.float64), Framed(eng, (P, 16), np.float64)
    n = 0
    for head in variants():
        refused(eng, "im_dod_keys", *head, grids.ctypes.data, key.ptr, st)
        refused(eng, "im_dod_reduce", *head, p(s.skey), p(s.perm), H.ptr, report.ptr, st)
        key.untouched(("im_dod_keys", n))
        H.untouched(("im_dod_reduce", n))
        report.untouched(("im_dod_reduce", n))
        assert (grids == -7.0).all(), n
        n += 1
    refused(eng, "im_dod_keys", *good, None, key.ptr, st)
    for tail in ((None, p(s.perm), H.ptr, report.ptr), (p(s.skey), None, H.ptr, report.ptr), (p(s.skey), p(s.perm), H.ptr, None)):
        refused(eng, "im_dod_reduce", *good, *tail, st)
    key.untouched("im_dod_keys, null grids")
    H.untouched("im_dod_reduce, null pointer")
    report.untouched("im_dod_reduce, null pointer")
    # P == 0 returns 0 and launches nothing; keys without a key buffer fill the grids alone
    eng.ctx.call("im_dod_keys", *good[:4], 0, *good[5:], grids.ctypes.data, key.ptr, st)
    eng.ctx.call("im_dod_reduce", *good[:4], 0, *good[5:], p(s.skey), p(s.perm), H.ptr, report.ptr, st)
    assert (grids == -7.0).all()
    eng.ctx.call("im_dod_keys", *good, grids.ctypes.data, None, st)
    assert np.array_equal(bits(grids), bits(s.grids))
    key.untouched("P == 0")
    H.untouched("P == 0")
    report.untouched("P == 0")
    # the crop
    poly = polygon(np.random.default_rng(1), 5)
    nan_poly = poly.copy()
    nan_poly[3, 1] = np.inf
    npts = len(s.pts)
    mask, index, count = Framed(eng, (npts,), np.uint8), Framed(eng, (npts,), np.int64), Framed(eng, (1,), np.int64)
    ok = (p(s.d_pts), npts, 0, 1, poly.ctypes.data, 5, 1, mask.ptr, index.ptr, count.ptr)
    for k, args in enumerate((ok[:1] + (-1,) + ok[2:], ok[:1] + (2 ** 31,) + ok[2:], ok[:2] + (1, 1) + ok[4:], ok[:2] + (0, 3) + ok[4:], ok[:2] + (-1, 1) + ok[4:],
                              ok[:4] + (None,) + ok[5:], ok[:5] + (2,) + ok[6:], ok[:5] + (1025,) + ok[6:], ok[:4] + (nan_poly.ctypes.data,) + ok[5:],
                              (None,) + ok[1:], ok[:7] + (None,) + ok[8:], ok[:8] + (None,) + ok[9:], ok[:9] + (None,))):
        refused(eng, "im_crop_polygon", *args, st)
        for f in (mask, index, count):
            f.untouched(("im_crop_polygon", k))
