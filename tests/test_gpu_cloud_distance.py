"""The cross-cloud kernels (csrc/cloud_distance.hip: im_knn_cross, im_ball_cross, im_cyl_stats, im_m3c2_finish) on the device, at every
boundary between two code paths (tests/cloud_distance_cases.py: target sizes around the 64-candidate batch, queries inside the grid, on
cell faces, just outside every face of the target's box and 10^3 and 10^7 cells away, coincident points, radii that drop everything,
cylinders whose cap and wall hold points exactly, a NaN and a zero normal, degenerate grids, grids so fine that a query gives its walk up
for a scan of the whole cloud, a world frame), the Python layers at any cell size and query order, exact end-to-end checks of
`cloud_to_cloud_distance`, `m3c2`, `PointCloud.compute_point_cloud_distance` and `m3c2_series`, and the refusals of the C entry points.

Bounds. Every output of the four entry points: equality of bits with the brute-force restatement (tests/cloud_distance_oracle.py) for
every query of every case, a NaN equal to a NaN whatever its payload. Derived, not measured: the neighbours are selected and ordered by
exact comparisons of the same float64 d2; the sums are exact integers, a function of the input alone whatever the grid, the lanes, the
query order and the order of the reduction; everything after them is the same IEEE float64 operations in the same order with contraction
off, and float64 division and sqrt are correctly rounded on the device. The host build of the same text agrees with the restatement on the
same cases (tests/test_cloud_distance_cpu.py); what only this file can show is the wave-level walks, the clamped cell of a query outside
the grid, the reductions and a lost `#pragma clang fp contract(off)`. d_rings equals the restatement's count of rings, sign included;
the sign of d_steps equals the restatement's prediction of which queries give their box up.

Every output of a C ABI call lies between two guard bands of sentinel bytes in one allocation and is itself pre-filled; the bands must
come back untouched."""
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ball_cases as BC  # noqa: E402
import cloud_distance_cases as CC  # noqa: E402
import knn_oracle as K  # noqa: E402

pytestmark = pytest.mark.gpu

BAND, SENT, FILL = 4096, 0xA5, 0x5A
REFUSED = -79
LIMIT_S = 5.0             # every launch of a case, outputs downloaded: a walk whose work grows with the grid would take minutes
INF = float("inf")


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


def same(a, b):
    """Equality of bits, a NaN equal to a NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


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


KNN_OUT = ("count", "idx", "d2", "rings")
BALL_OUT = ("count", "sums", "eig", "normal", "steps")
CYL_OUT = ("count", "sums", "mean", "std", "steps")
FIN_OUT = ("dist", "lod", "sig")


def outputs(eng, kind, m, k=1):
    shapes = {"knn": {"count": ((m,), np.int32), "idx": ((m, k), np.int32), "d2": ((m, k), np.float64), "rings": ((m,), np.int32)},
              "ball": {"count": ((m,), np.int32), "sums": ((m, 10), np.int64), "eig": ((m, 3), np.float64), "normal": ((m, 3), np.float64),
                       "steps": ((m,), np.int32)},
              "cyl": {"count": ((m,), np.int32), "sums": ((m, 2), np.int64), "mean": ((m,), np.float64), "std": ((m,), np.float64),
                      "steps": ((m,), np.int32)},
              "fin": {"dist": ((m,), np.float64), "lod": ((m,), np.float64), "sig": ((m,), np.uint8)}}[kind]
    return {name: Framed(eng, *sd) for name, sd in shapes.items()}


class Target:
    """A case's target cloud on the device, binned and sorted once by the calls the k-NN uses, with the case's queries and normals."""

    def __init__(self, eng, case):
        import torch
        self.case, self.n, self.m = case, len(case["points"]), len(case["queries"])
        self.grid, self.dims = CC.grid(case)
        self.cells = int(np.prod(self.dims.astype(np.int64)))
        self.d_pts, self.d_q, self.d_nrm = dev(eng, case["points"]), dev(eng, case["queries"]), dev(eng, case["normals"])
        key = torch.empty(self.n, dtype=torch.int64, device=eng.device)
        eng.ctx.call("im_knn_cells", p(self.d_pts), self.n, self.grid.ctypes.data, *[int(v) for v in self.dims], p(key), eng.stream_ptr())
        self.skey, self.perm = torch.sort(key, stable=True)
        self.start = torch.empty(self.cells + 1, dtype=torch.int32, device=eng.device)
        eng.ctx.call("im_knn_cell_ranges", p(self.skey), self.n, self.cells, p(self.start), eng.stream_ptr())
        # the three query orders: as given, by the key of the query's clamped cell, and that reversed
        with np.errstate(all="ignore"):
            qc = K.cells(K.cell_coords(case["queries"], self.grid[:3], self.grid[3]), self.dims.astype(np.int64))
        by_key = np.argsort(K.keys(qc, self.dims.astype(np.int64)), kind="stable").astype(np.int64)
        self.orders = {"given": None, "sorted": dev(eng, by_key), "reversed": dev(eng, by_key[::-1])}

    def head(self, n=None):
        return (p(self.d_pts), p(self.perm), p(self.start), self.n if n is None else n, self.grid.ctypes.data, *[int(v) for v in self.dims])

    def knn(self, eng, k, radius2, order=None):
        out = outputs(eng, "knn", self.m, k)
        eng.ctx.call("im_knn_cross", *self.head(), p(self.d_q), p(order), self.m, k, radius2, *[out[o].ptr for o in KNN_OUT],
                     eng.stream_ptr())
        return {name: f.result((self.case["name"], "knn", name)) for name, f in out.items()}

    def ball(self, eng, order=None):
        out = outputs(eng, "ball", self.m)
        eng.ctx.call("im_ball_cross", *self.head(), p(self.d_q), p(order), self.m, self.case["r"], *[out[o].ptr for o in BALL_OUT], eng.stream_ptr())
        return {name: f.result((self.case["name"], "ball", name)) for name, f in out.items()}

    def cyl(self, eng, order=None):
        out = outputs(eng, "cyl", self.m)
        eng.ctx.call("im_cyl_stats", *self.head(), p(self.d_q), p(self.d_nrm), p(order), self.m, self.case["rho"], self.case["L"],
                     *[out[o].ptr for o in CYL_OUT], eng.stream_ptr())
        return {name: f.result((self.case["name"], "cyl", name)) for name, f in out.items()}


@pytest.fixture(scope="module")
def targets(eng):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Target(eng, CC.by_name(name))
        return cache[name]
    return get


def finite_queries(case):
    return np.isfinite(case["queries"]).all(1)


# ---- every case of the shared list: bits, for the three query orders ------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.names())
def test_knn_cross_equals_the_restatement_bit_for_bit(eng, targets, name):
    t = targets(name)
    case = t.case
    for k in case["ks"]:
        for radius2 in case["radius2s"]:
            oidx, od2, ocount = CC.expected_knn(name, k, radius2)
            orings = CC.expected_rings(name, k, radius2)
            for tag, order in t.orders.items():
                what = (name, k, radius2, tag)
                eng.synchronize()
                t0 = time.perf_counter()
                got = t.knn(eng, k, radius2, order)                    # downloads the outputs: the launch has finished
                assert time.perf_counter() - t0 < LIMIT_S, (what, "the launch took", time.perf_counter() - t0)
                assert np.array_equal(got["count"], ocount), what
                bad = np.nonzero((got["idx"] != oidx).any(1))[0]
                assert len(bad) == 0, (what, f"{len(bad)} queries differ, first {int(bad[0])}: {got['idx'][bad[0]].tolist()} != {oidx[bad[0]].tolist()}")
                assert same(got["d2"], od2), what
                assert np.array_equal(got["rings"], orings), (what, got["rings"].tolist(), orings.tolist())
    if name == "line_x":
        assert (CC.expected_rings(name, 64, INF) < 0).any()
    if name == "few_points":
        assert CC.expected_rings(name, 1, INF).tolist()[-2:] == [0, 0]


@pytest.mark.parametrize("name", CC.names())
def test_ball_cross_equals_the_restatement_bit_for_bit(eng, targets, name):
    t = targets(name)
    want, falls_back, fin = CC.expected_ball(name), CC.expected_ball_walk(name), finite_queries(t.case)
    for tag, order in t.orders.items():
        what = (name, tag)
        eng.synchronize()
        t0 = time.perf_counter()
        got = t.ball(eng, order)
        assert time.perf_counter() - t0 < LIMIT_S, (what, "the launch took", time.perf_counter() - t0)
        assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["sums"], want["sums"]), what
        assert same(got["eig"], want["eig"]) and same(got["normal"], want["normal"]), what
        steps = got["steps"]
        assert np.array_equal(steps < 0, falls_back) and np.array_equal(steps == 0, ~fin), (what, steps.tolist(), falls_back.tolist())
        assert (steps[falls_back] == -((t.n + 63) // 64)).all(), what
        assert (steps[~falls_back] <= 1024 + t.n // 32 + (t.n + 63) // 64 + t.n).all(), what      # bounded work: lookups, batches, a part batch per row


@pytest.mark.parametrize("name", CC.names())
def test_cyl_stats_equals_the_restatement_bit_for_bit(eng, targets, name):
    t = targets(name)
    case = t.case
    want, falls_back = CC.expected_cyl(name), CC.expected_cyl_walk(name)
    fin = finite_queries(case) & np.isfinite(case["normals"]).all(1)
    for tag, order in t.orders.items():
        what = (name, tag)
        eng.synchronize()
        t0 = time.perf_counter()
        got = t.cyl(eng, order)
        assert time.perf_counter() - t0 < LIMIT_S, (what, "the launch took", time.perf_counter() - t0)
        assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["sums"], want["sums"]), what
        assert same(got["mean"], want["mean"]) and same(got["std"], want["std"]), what
        steps = got["steps"]
        assert np.array_equal(steps < 0, falls_back) and np.array_equal(steps == 0, ~fin), (what, steps.tolist(), falls_back.tolist())
        assert (steps[falls_back] == -((t.n + 63) // 64)).all(), what
        assert (steps[~falls_back] <= 1024 + t.n // 32 + (t.n + 63) // 64 + t.n).all(), what


def test_m3c2_finish_equals_the_restatement_bit_for_bit(eng):
    L, f = CC.finish_inputs()
    m = len(f["count1"])
    d = [dev(eng, f[k]) for k in ("count1", "sums1", "count2", "sums2")]
    out = outputs(eng, "fin", m)
    eng.ctx.call("im_m3c2_finish", *[p(a) for a in d], m, L, CC.REG_ERROR, CC.MIN_POINTS, *[out[o].ptr for o in FIN_OUT], eng.stream_ptr())
    odist, olod, osig = CC.expected_finish()
    assert same(out["dist"].result("dist"), odist) and same(out["lod"].result("lod"), olod) and np.array_equal(out["sig"].result("sig"), osig)
    # each output alone
    for alone in FIN_OUT:
        out = outputs(eng, "fin", m)
        eng.ctx.call("im_m3c2_finish", *[p(a) for a in d], m, L, CC.REG_ERROR, CC.MIN_POINTS, *[out[o].ptr if o == alone else None for o in FIN_OUT],
                     eng.stream_ptr())
        res = out[alone].result(alone)
        assert np.array_equal(res, osig) if alone == "sig" else same(res, {"dist": odist, "lod": olod}[alone])
        for o in FIN_OUT:
            if o != alone:
                out[o].untouched((alone, o))


def test_zero_sizes_launch_nothing(eng, targets):
    t = targets("n65")
    st = eng.stream_ptr()
    for n, m in ((0, t.m), (t.n, 0), (0, 0)):
        kn, ba, cy, fi = outputs(eng, "knn", 4, 3), outputs(eng, "ball", 4), outputs(eng, "cyl", 4), outputs(eng, "fin", 4)
        eng.ctx.call("im_knn_cross", *t.head(n), p(t.d_q), None, m, 3, INF, *[kn[o].ptr for o in KNN_OUT], st)
        eng.ctx.call("im_ball_cross", *t.head(n), p(t.d_q), None, m, 0.4, *[ba[o].ptr for o in BALL_OUT], st)
        eng.ctx.call("im_cyl_stats", *t.head(n), p(t.d_q), p(t.d_nrm), None, m, 0.25, 0.5, *[cy[o].ptr for o in CYL_OUT], st)
        for group in (kn, ba, cy):
            for name, f in group.items():
                f.untouched(((n, m), name))
    counts, sums = dev(eng, np.zeros(4, np.int32)), dev(eng, np.zeros((4, 2), np.int64))
    eng.ctx.call("im_m3c2_finish", p(counts), p(sums), p(counts), p(sums), 0, 1.0, 0.0, 5, *[fi[o].ptr for o in FIN_OUT], st)
    for name, f in fi.items():
        f.untouched(("m == 0", name))


def test_every_output_is_optional(eng, targets):
    name = "n129"
    t = targets(name)
    st = eng.stream_ptr()
    oidx, od2, ocount = CC.expected_knn(name, 5, INF)
    wants = {"knn": {"count": ocount, "idx": oidx, "d2": od2}, "ball": CC.expected_ball(name), "cyl": CC.expected_cyl(name)}
    for kind, names in (("knn", KNN_OUT), ("ball", BALL_OUT), ("cyl", CYL_OUT)):
        for alone in names:
            out = outputs(eng, kind, t.m, 5)
            ptrs = [out[o].ptr if o == alone else None for o in names]
            if kind == "knn":
                eng.ctx.call("im_knn_cross", *t.head(), p(t.d_q), None, t.m, 5, INF, *ptrs, st)
            elif kind == "ball":
                eng.ctx.call("im_ball_cross", *t.head(), p(t.d_q), None, t.m, t.case["r"], *ptrs, st)
            else:
                eng.ctx.call("im_cyl_stats", *t.head(), p(t.d_q), p(t.d_nrm), None, t.m, t.case["rho"], t.case["L"], *ptrs, st)
            res = out[alone].result((kind, alone))
            if alone in wants[kind]:
                w = wants[kind][alone]
                assert same(res, w) if w.dtype == np.float64 else np.array_equal(res, w), (kind, alone)
            for o in names:
                if o != alone:
                    out[o].untouched((kind, alone, o))


# ---- the Python layers: the result depends neither on the grid nor on the query order --------------------------------------------------------
def test_python_layers_with_any_cell_size_and_order(eng):
    import torch
    from icepy4d_amd.utils import point_cloud_filters as F
    name = "plane_x_mid"
    case = CC.by_name(name)
    pts, q, nr = case["points"], case["queries"], case["normals"]
    oidx, od2, ocount = CC.expected_knn(name, 8, INF)
    oball, ocyl = CC.expected_ball(name), CC.expected_cyl(name)
    signs = {}
    for kw in ({}, {"cell_size": 0.25}, {"cell_size": 0.02}, {"cell_size": 0.001}, {"cell_size": 0.02, "sort_queries": False}):
        t0 = time.perf_counter()
        kn = F.knn_cross(q, pts, 8, engine=eng, want=("idx", "d2", "count", "rings"), **kw)
        ba = F.ball_cross(q, pts, case["r"], want=("count", "sums", "eig", "normal", "steps"), engine=eng, **kw)
        cy = F.cylinder_stats(q, nr, pts, case["rho"], case["L"], want=("count", "sums", "mean", "std", "steps"), engine=eng, **kw)
        assert time.perf_counter() - t0 < 3 * LIMIT_S, kw
        assert all(isinstance(v, np.ndarray) for r in (kn, ba, cy) for v in r.values())
        assert np.array_equal(kn["idx"], oidx) and same(kn["d2"], od2) and np.array_equal(kn["count"], ocount), kw
        assert np.array_equal(ba["sums"], oball["sums"]) and same(ba["eig"], oball["eig"]) and same(ba["normal"], oball["normal"]), kw
        assert np.array_equal(cy["count"], ocyl["count"]) and np.array_equal(cy["sums"], ocyl["sums"]), kw
        assert same(cy["mean"], ocyl["mean"]) and same(cy["std"], ocyl["std"]), kw
        signs[kw.get("cell_size")] = (ba["steps"] < 0, cy["steps"] < 0)
    # the three cases of the list are this cloud at these three cell sizes: the finest forces the scan of the whole cloud
    for tag, s in (("coarse", 0.25), ("mid", 0.02), ("fine", 0.001)):
        assert np.array_equal(signs[s][0], CC.expected_ball_walk(f"plane_x_{tag}")) and np.array_equal(signs[s][1], CC.expected_cyl_walk(f"plane_x_{tag}"))
    assert signs[0.001][0].any() and signs[0.001][1].any() and not signs[0.25][0].any()
    # tensors in, tensors out; a cloud binned once serves all three
    b = F.bin_cloud(pts, 0.05, engine=eng)
    dq, dn = dev(eng, q), dev(eng, nr)
    kn = F.knn_cross(dq, None, 8, binned=b, engine=eng)
    ba = F.ball_cross(dq, None, case["r"], binned=b, engine=eng)
    cy = F.cylinder_stats(dq, dn, None, case["rho"], case["L"], binned=b, engine=eng)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for r in (kn, ba, cy) for v in r.values())
    assert np.array_equal(kn["idx"].cpu().numpy(), oidx) and same(ba["normal"].cpu().numpy(), oball["normal"]) and same(cy["std"].cpu().numpy(), ocyl["std"])
    # an empty target and no queries
    e = F.knn_cross(q, np.zeros((0, 3)), 3, engine=eng)
    assert (e["count"] == 0).all() and (e["idx"] == -1).all() and np.isinf(e["d2"]).all()
    e = F.cylinder_stats(q, nr, np.zeros((0, 3)), 1.0, 1.0, engine=eng)
    assert (e["count"] == 0).all() and np.isnan(e["mean"]).all() and np.isnan(e["std"]).all()
    e = F.ball_cross(np.zeros((0, 3)), pts, 1.0, engine=eng)
    assert e["count"].shape == (0,) and e["normal"].shape == (0, 3)
    with pytest.raises(ValueError, match="non-finite"):
        F.knn_cross(q, np.array([[0.0, np.nan, 0.0]]), 1, engine=eng)


# ---- exact end-to-end checks ---------------------------------------------------------------------------------------------------------------
def lattice(z):
    g = np.arange(40, dtype=np.float64) / 8.0
    return np.column_stack([np.repeat(g, 40), np.tile(g, 40), np.full(1600, z)])


def test_m3c2_of_two_parallel_lattices_is_exact(eng):
    import torch
    from icepy4d_amd.post_processing import m3c2
    c1, c2 = lattice(0.0), lattice(0.25)
    t0 = time.perf_counter()
    r = m3c2(c1, c2, normal_scale=1.0, search_scale=1.0, search_depth=1.0, registration_error=0.01, engine=eng)
    assert time.perf_counter() - t0 < LIMIT_S
    assert all(isinstance(v, np.ndarray) for v in r) and np.array_equal(r.core_points, c1)
    assert np.array_equal(r.normals, np.tile([0.0, 0.0, 1.0], (1600, 1)))
    assert (r.count1 >= 5).all() and (r.count2 >= 5).all() and np.array_equal(r.count1, r.count2)      # the corner's quarter disc of radius 4 steps holds 17 points
    assert (r.distance == 0.25).all() and (r.std1 == 0.0).all() and (r.std2 == 0.0).all()
    assert (r.lod == np.float64(1.96) * np.float64(0.01)).all() and r.significant.dtype == bool and r.significant.all()
    down = m3c2(c1, c2, normal_scale=1.0, search_scale=1.0, search_depth=1.0, registration_error=0.01, orientation=(0, 0, -1), engine=eng)
    assert (down.distance == -0.25).all() and np.array_equal(down.normals, np.tile([0.0, 0.0, -1.0], (1600, 1))) and down.significant.all()
    # a viewpoint below flips as well; supplied normals are scaled to unit length; too few points give NaN lod and nothing significant
    view = m3c2(c1, c2, core_points=c1[::50], normal_scale=1.0, search_scale=1.0, search_depth=1.0, viewpoint=(2.0, 2.0, -50.0), engine=eng)
    assert (view.distance == -0.25).all() and len(view.distance) == 32
    given = m3c2(dev(eng, c1), c2, normals=np.tile([0.0, 0.0, 4.0], (1600, 1)), normal_scale=1.0, search_scale=1.0, search_depth=1.0, engine=eng)
    assert isinstance(given.distance, torch.Tensor) and (given.distance.cpu().numpy() == 0.25).all() and (given.normals.cpu().numpy()[:, 2] == 1.0).all()
    many = m3c2(c1, c2, normal_scale=1.0, search_scale=1.0, search_depth=1.0, min_points=2000, engine=eng)
    assert np.isnan(many.lod).all() and not many.significant.any() and (many.distance == 0.25).all()
    # a degenerate ball: NaN normal, NaN distance, not significant
    lone = m3c2(c1, c2, core_points=np.array([[100.0, 100.0, 0.0]]), normal_scale=1.0, search_scale=1.0, search_depth=1.0, engine=eng)
    assert np.isnan(lone.normals).all() and np.isnan(lone.distance).all() and not lone.significant.any() and lone.count1[0] == 0


def test_cloud_to_cloud_distance_is_exact(eng):
    from icepy4d_amd.core import PointCloud
    from icepy4d_amd.post_processing import cloud_to_cloud_distance
    c1, c2 = lattice(0.0), lattice(0.25)
    r = cloud_to_cloud_distance(c1, c2, engine=eng)
    assert (r.distance == 0.25).all() and np.array_equal(r.index, np.arange(1600)) and np.array_equal(r.split, np.tile([0.0, 0.0, 0.25], (1600, 1)))
    assert np.array_equal(PointCloud(points3d=c1).compute_point_cloud_distance(PointCloud(points3d=c2), engine=eng), r.distance)
    assert np.array_equal(PointCloud(points3d=c1).compute_point_cloud_distance(c2, engine=eng), r.distance)
    # against the restatement on a case with queries far outside
    case = CC.by_name("far_queries")
    got = cloud_to_cloud_distance(case["queries"], case["points"], engine=eng)
    oidx, od2, _ = CC.expected_knn("far_queries", 1, INF)
    assert np.array_equal(got.index, oidx[:, 0]) and same(got.distance, np.sqrt(od2[:, 0])) and same(got.split, case["points"][oidx[:, 0]] - case["queries"])
    none = cloud_to_cloud_distance(c1[:3], np.zeros((0, 3)), engine=eng)
    assert np.isinf(none.distance).all() and (none.index == -1).all() and np.isnan(none.split).all()


def test_m3c2_series_equals_the_per_pair_calls(eng):
    from icepy4d_amd import change_detection as C
    from icepy4d_amd.post_processing import m3c2
    fronts = [BC.front(1200, seed=40 + k) + np.array([0.2 * k, 0.0, 0.0]) for k in range(3)]
    kw = dict(normal_scale=1.0, search_scale=0.5, search_depth=1.0, registration_error=0.02)
    pairs = [(0, 1), (1, 2), (0, 2)]
    t0 = time.perf_counter()
    series = C.m3c2_series(fronts, pairs, engine=eng, **kw)
    assert time.perf_counter() - t0 < LIMIT_S and len(series) == 3
    for (a, b), got in zip(pairs, series):
        want = m3c2(fronts[a], fronts[b], engine=eng, **kw)
        for name, x, y in zip(got._fields, got, want):
            assert isinstance(x, np.ndarray) and (np.array_equal(x, y) if x.dtype != np.float64 else same(x, y)), ((a, b), name)
    table = C.m3c2_table(series, names=[(f"e{a}", f"e{b}") for a, b in pairs])
    assert table["n_core"].tolist() == [1200] * 3 and (table["n_distance"] > 600).all() and (table["n_significant"] > 0).all()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(eng, targets):
    from icepy4d_amd._lib import IcematchError
    t = targets("n65")
    n, m, st = t.n, t.m, eng.stream_ptr()
    nx, ny, nz = (int(v) for v in t.dims)
    good, pts, perm, start, q, nrm = t.grid.ctypes.data, p(t.d_pts), p(t.perm), p(t.start), p(t.d_q), p(t.d_nrm)
    grids = {"s = 0": [0, 0, 0, 0.0], "s < 0": [0, 0, 0, -1.0], "s = inf": [0, 0, 0, np.inf], "s = nan": [0, 0, 0, np.nan],
             "origin nan": [np.nan, 0, 0, 1.0], "origin inf": [0, np.inf, 0, 1.0]}
    held = {what: np.array(g, np.float64) for what, g in grids.items()}

    def heads():
        """What the three query calls refuse in common: (what, the target arguments, d_q, m)."""
        out = [("null points", (None, perm, start, n, good, nx, ny, nz), q, m), ("null permutation", (pts, None, start, n, good, nx, ny, nz), q, m),
               ("null ranges", (pts, perm, None, n, good, nx, ny, nz), q, m), ("null grid", (pts, perm, start, n, None, nx, ny, nz), q, m),
               ("null queries", (pts, perm, start, n, good, nx, ny, nz), None, m), ("n < 0", (pts, perm, start, -1, good, nx, ny, nz), q, m),
               ("n = 2^26 + 1", (pts, perm, start, 2 ** 26 + 1, good, nx, ny, nz), q, m), ("m < 0", (pts, perm, start, n, good, nx, ny, nz), q, -1),
               ("m = 2^26 + 1", (pts, perm, start, n, good, nx, ny, nz), q, 2 ** 26 + 1), ("nx = 0", (pts, perm, start, n, good, 0, ny, nz), q, m),
               ("nz < 0", (pts, perm, start, n, good, nx, ny, -3), q, m), ("cells above the cap", (pts, perm, start, n, good, 4096, 4096, 2), q, m),
               ("cells overflow", (pts, perm, start, n, good, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), q, m)]
        return out + [(what, (pts, perm, start, n, arr.ctypes.data, nx, ny, nz), q, m) for what, arr in held.items()]

    ok_head = (pts, perm, start, n, good, nx, ny, nz)
    kn, ba, cy, fi = outputs(eng, "knn", m, 4), outputs(eng, "ball", m), outputs(eng, "cyl", m), outputs(eng, "fin", m)
    ko, bo, co, fo = ([g[o].ptr for o in names] for g, names in ((kn, KNN_OUT), (ba, BALL_OUT), (cy, CYL_OUT), (fi, FIN_OUT)))
    calls = []
    for what, head, dq, mm in heads():
        calls += [("im_knn_cross", what, (*head, dq, None, mm, 4, INF, *ko)), ("im_ball_cross", what, (*head, dq, None, mm, 0.4, *bo)),
                  ("im_cyl_stats", what, (*head, dq, nrm, None, mm, 0.25, 0.5, *co))]
    for k in (0, 65, -1):
        calls.append(("im_knn_cross", f"k = {k}", (*ok_head, q, None, m, k, INF, *ko)))
    for r2 in (-1.0, np.nan):
        calls.append(("im_knn_cross", f"radius2 = {r2}", (*ok_head, q, None, m, 4, r2, *ko)))
    for r in (0.0, -1.0, np.inf, np.nan, 2.0 ** -1010):
        calls.append(("im_ball_cross", f"r = {r}", (*ok_head, q, None, m, r, *bo)))
        calls.append(("im_cyl_stats", f"L = {r}", (*ok_head, q, nrm, None, m, 0.25, r, *co)))
    for r in (0.0, -1.0, np.inf, np.nan):
        calls.append(("im_cyl_stats", f"rho = {r}", (*ok_head, q, nrm, None, m, r, 0.5, *co)))
    calls.append(("im_cyl_stats", "null normals", (*ok_head, q, None, None, m, 0.25, 0.5, *co)))
    counts, sums = dev(eng, np.full(m, 6, np.int32)), dev(eng, np.ones((m, 2), np.int64))
    c, s = p(counts), p(sums)
    for what, args in (("null count1", (None, s, c, s, m, 1.0, 0.0, 5)), ("null sums1", (c, None, c, s, m, 1.0, 0.0, 5)),
                       ("null count2", (c, s, None, s, m, 1.0, 0.0, 5)), ("null sums2", (c, s, c, None, m, 1.0, 0.0, 5)),
                       ("m < 0", (c, s, c, s, -1, 1.0, 0.0, 5)), ("m = 2^26 + 1", (c, s, c, s, 2 ** 26 + 1, 1.0, 0.0, 5)),
                       ("L = 0", (c, s, c, s, m, 0.0, 0.0, 5)), ("L = nan", (c, s, c, s, m, np.nan, 0.0, 5)), ("L = inf", (c, s, c, s, m, np.inf, 0.0, 5)),
                       ("h denormal", (c, s, c, s, m, 2.0 ** -1010, 0.0, 5)), ("reg < 0", (c, s, c, s, m, 1.0, -0.1, 5)),
                       ("reg = nan", (c, s, c, s, m, 1.0, np.nan, 5)), ("reg = inf", (c, s, c, s, m, 1.0, np.inf, 5)),
                       ("min_points = 1", (c, s, c, s, m, 1.0, 0.0, 1)), ("min_points < 0", (c, s, c, s, m, 1.0, 0.0, -5))):
        calls.append(("im_m3c2_finish", what, (*args, *fo)))
    for fn, what, args in calls:
        with pytest.raises(IcematchError) as e:
            eng.ctx.call(fn, *args, st)
        assert e.value.rc == REFUSED, (fn, what, e.value)
    for group in (kn, ba, cy, fi):
        for name, f in group.items():
            f.untouched(name)
    # the smallest half-length whose step is a normal number is served
    ok = outputs(eng, "cyl", m)
    eng.ctx.call("im_cyl_stats", *ok_head, q, nrm, None, m, 0.25, 2.0 ** -1004, *[ok[o].ptr for o in CYL_OUT], st)
    assert (ok["count"].result("tiny half-length") >= 0).all()
