"""The point-cloud neighbourhood kernels (csrc/knn.hip, csrc/knn_point.h) on the device, at every boundary between two code paths
(tests/knn_cases.py: cloud sizes around the 64-candidate batch and around k, every k at a boundary of the list, degenerate and sparse
grids, cells larger than a block's worth of candidates, a grid at the cell cap, points exactly on cell faces, lattices and coincident
points that tie at the k-th place, far outliers along every axis whose search ends by covering the grid, a lone point 2^24 cells from a
cluster whose search must end by the whole-cloud scan within seconds, radii between, on and below neighbours' d2, a world frame), the
number of rings every search visits, statistical outlier removal and `PointCloud.sor_filter` against tests/golden/g16_pointcloud.npz, the normals, and the
refusals of the C entry points.

Bounds. Neighbour indices and counts: equality. d2 and the mean neighbour distance: equality of bits with the brute-force restatement
(tests/knn_oracle.py), for every point of every case. Derived, not measured: the kernels and the restatement perform the same IEEE
float64 operations in the same order with contraction off, float64 sqrt and division are correctly rounded on the device, and the library
is built without a fast-math flag; the neighbours themselves are a function of the input alone (ascending d2, the lower index first).
The host build of the same text agrees with the restatement on the same case list (tests/test_pointcloud_cpu.py); what only this file can
show is the wave-level search itself and a lost `#pragma clang fp contract(off)`: gfx950 has fused multiply-add.
Normals: |n_dev x n_ref| <= 1e-8 against numpy.linalg.eigh for every point whose eigenvalue gap (l1 - l0) / l2 is at least 1e-6, which
must be at least 99 % of a case (Davis-Kahan: the rounding of a float64 covariance and of Jacobi is a few hundred eps relative, over a
gap of 1e-6 below 1e-8), and the sign convention where |n_z| > 1e-6.

Every output of a C ABI call lies between two guard bands of sentinel bytes in one allocation and is itself pre-filled; the bands must
come back untouched."""
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_cases as KC  # noqa: E402
import knn_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

BAND, SENT, FILL = 4096, 0xA5, 0x5A
REFUSED = -75
LIMIT_S = 5.0             # every launch of every case, outputs downloaded: a search whose work grows with the grid would take minutes
INF = float("inf")


@pytest.fixture(scope="module")
def g16():
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


def outputs(eng, n, k):
    return {"count": Framed(eng, (n,), np.int32), "idx": Framed(eng, (n, k), np.int32), "d2": Framed(eng, (n, k), np.float64),
            "mean": Framed(eng, (n,), np.float64), "normal": Framed(eng, (n, 3), np.float64), "rings": Framed(eng, (n,), np.int32)}


def call_self(eng, d_pts, perm, start, n, grid, dims, k, radius2, out):
    eng.ctx.call("im_knn_self", p(d_pts), p(perm), start, n, grid.ctypes.data, int(dims[0]), int(dims[1]), int(dims[2]), k, radius2,
                 out["count"].ptr, out["idx"].ptr, out["d2"].ptr, out["mean"].ptr, out["normal"].ptr, out["rings"].ptr, eng.stream_ptr())


class Sorted:
    """A case's cloud on the device, binned and sorted once: keys and cell ranges come back through guard bands."""

    def __init__(self, eng, case):
        import torch
        self.case, self.n = case, len(case["points"])
        self.grid, self.dims = KC.grid(case)
        self.cells = int(np.prod(self.dims.astype(np.int64)))
        self.d_pts = dev(eng, case["points"])
        key = Framed(eng, (self.n,), np.int64)
        eng.ctx.call("im_knn_cells", p(self.d_pts), self.n, self.grid.ctypes.data, *[int(v) for v in self.dims], key.ptr, eng.stream_ptr())
        self.key = key.result((case["name"], "keys"))
        self.skey, self.perm = torch.sort(dev(eng, self.key), stable=True)
        self.start = Framed(eng, (self.cells + 1,), np.int32)
        eng.ctx.call("im_knn_cell_ranges", p(self.skey), self.n, self.cells, self.start.ptr, eng.stream_ptr())

    def run(self, eng, k, radius2):
        out = outputs(eng, self.n, k)
        call_self(eng, self.d_pts, self.perm, self.start.ptr, self.n, self.grid, self.dims, k, radius2, out)
        return {name: f.result((self.case["name"], k, radius2, name)) for name, f in out.items()}


# ---- every case of the shared list: bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KC.names())
def test_neighbours_equal_the_oracle_bit_for_bit(eng, name):
    case = KC.by_name(name)
    pts = case["points"]
    s = Sorted(eng, case)
    oc = O.cells(O.cell_coords(pts, s.grid[:3], s.grid[3]), s.dims)
    assert np.array_equal(s.key, O.keys(oc, s.dims.astype(np.int64))), (name, "keys")
    start = s.start.result((name, "ranges"))
    assert np.array_equal(start, np.searchsorted(np.sort(s.key), np.arange(s.cells + 1)).astype(np.int32)), (name, "ranges")
    full = KC.full(name)
    rings = None
    for k in case["ks"]:
        for radius2 in case["radius2s"]:
            what = (name, k, radius2)
            eng.synchronize()
            t0 = time.perf_counter()
            got = s.run(eng, k, radius2)                              # downloads the outputs: the launch has finished
            oidx, od2, ocount, omean = O.cut(full, k, radius2)
            assert np.array_equal(got["count"], ocount), what
            bad = np.nonzero((got["idx"] != oidx).any(1))[0]
            assert len(bad) == 0, (what, f"{len(bad)} points differ, first {int(bad[0])}: {got['idx'][bad[0]].tolist()} != {oidx[bad[0]].tolist()}")
            assert np.array_equal(bits(got["d2"]), bits(od2)), what
            assert np.array_equal(bits(got["mean"]), bits(omean)), what
            few = ocount < 3
            assert (got["normal"][few] == (0.0, 0.0, 1.0)).all(), what
            assert (np.abs(np.linalg.norm(got["normal"], axis=1) - 1.0) < 1e-12).all(), what
            assert time.perf_counter() - t0 < LIMIT_S, (what, "the launch took", time.perf_counter() - t0)
            rings = got["rings"]
            assert (rings != 0).all() and (np.abs(rings) <= int(s.dims.max())).all(), what
    # the rings a search visits follow from the stop rule alone; a negative count marks a search that spent its step budget on the rings
    # and ended by scanning the whole cloud, which no case but the lone points at the cell cap may need
    k, radius2 = case["ks"][-1], case["radius2s"][-1]
    lone = name.startswith("cell_cap_lone")
    assert (rings[:len(pts) - 1 if lone else len(pts)] > 0).all(), name
    for i in np.random.default_rng(len(pts)).integers(0, len(pts) - 1 if lone else len(pts), 8):
        assert rings[i] == O.rings_needed(pts, int(i), k, case["s"], radius2), (name, int(i))
    if lone:
        assert -2048 < rings[-1] < 0, (name, int(rings[-1]))
    if name == "sparse_cells":
        assert np.median(rings) >= 5
    if name.startswith("far_outlier"):
        assert rings[-1] == 41 == s.dims.max()
    if name == "radius":
        assert (O.cut(full, 10, 0.0)[2] == 1).all() and (O.cut(full, 10, case["radius2s"][1])[2][0] == 4)      # the cases are what they claim


def test_null_outputs_are_optional(eng):
    case = KC.by_name("n257")
    s = Sorted(eng, case)
    idx = Framed(eng, (s.n, 10), np.int32)
    eng.ctx.call("im_knn_self", p(s.d_pts), p(s.perm), s.start.ptr, s.n, s.grid.ctypes.data, *[int(v) for v in s.dims], 10, INF,
                 None, idx.ptr, None, None, None, None, eng.stream_ptr())
    assert np.array_equal(idx.result("idx alone"), O.cut(KC.full("n257"), 10)[0])


# ---- the Python layer: the result does not depend on the grid ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("n4099", 10), ("lattice_s1", 30), ("far_outlier", 10), ("world_frame", 10), ("plane_z", 50), ("n1", 1)])
def test_knn_search_with_any_cell_size(eng, name, k):
    import torch
    from icepy4d_amd.utils import point_cloud_filters as F
    pts = KC.by_name(name)["points"]
    oidx, od2, ocount, omean = O.cut(KC.full(name), k)
    for kw in ({}, {"occupancy": 4.0}, {"occupancy": 0.01}, {"cell_size": 1e-9}, {"cell_size": 1e9}):
        idx, d2, count = F.knn_search(pts, k, engine=eng, **kw)
        assert isinstance(idx, torch.Tensor) and idx.dtype == torch.int32 and d2.dtype == torch.float64 and count.dtype == torch.int32
        assert np.array_equal(idx.cpu().numpy(), oidx) and np.array_equal(bits(d2.cpu().numpy()), bits(od2)), (name, kw)
        assert np.array_equal(count.cpu().numpy(), ocount), (name, kw)
    idx, d2, count = F.knn_search(dev(eng, pts), k, radius=0.05, engine=eng)                       # a device tensor in
    ridx, rd2, rcount, _ = O.cut(KC.full(name), k, 0.05 * 0.05)
    assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(bits(d2.cpu().numpy()), bits(rd2)) and np.array_equal(count.cpu().numpy(), rcount)


def test_python_layer_refuses_before_any_launch(eng):
    from icepy4d_amd.utils import point_cloud_filters as F
    bad = np.zeros((5, 3))
    bad[2, 1] = np.nan
    for fn in (lambda q: F.knn_search(q, 3, engine=eng), lambda q: F.remove_statistical_outlier(q, 3, 1.0, engine=eng),
               lambda q: F.estimate_normals(q, engine=eng)):
        with pytest.raises(ValueError, match="non-finite"):
            fn(bad)
        with pytest.raises(ValueError, match="non-finite"):
            fn(dev(eng, np.where(np.isnan(bad), np.inf, bad)))
        with pytest.raises(ValueError):
            fn(np.zeros((5, 2)))
    idx, d2, count = F.knn_search(np.zeros((0, 3)), 5, engine=eng)
    assert tuple(idx.shape) == (0, 5) and tuple(count.shape) == (0,)
    kept, ind = F.remove_statistical_outlier(np.zeros((0, 3)), 10, 3.0, engine=eng)
    assert kept.shape == (0, 3) and ind.shape == (0,)
    assert F.estimate_normals(np.zeros((0, 3)), engine=eng).shape == (0, 3)


# ---- statistical outlier removal -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,nb,ratio", [("sor10", 10, 3.0), ("sor50", 50, 1.5)])
def test_sor_equals_the_oracle_on_g16(eng, g16, tag, nb, ratio):
    import torch
    from icepy4d_amd.utils import point_cloud_filters as F
    pts = g16["points"]
    kept, ind = F.remove_statistical_outlier(pts, nb, ratio, engine=eng)
    assert isinstance(ind, np.ndarray) and ind.dtype == np.int64
    assert np.array_equal(ind, g16[f"{tag}_ind"]) and np.array_equal(kept, g16[f"{tag}_points"])
    assert not set(ind.tolist()) & set(g16["planted"].tolist())                                    # the planted outliers are gone
    # the statistic itself, bit for bit, and the threshold
    r = F.knn_self(pts, nb, want=("count", "mean"), engine=eng)
    _, _, ocount, omean = O.knn_self(pts, nb)
    assert np.array_equal(bits(r["mean"].cpu().numpy()), bits(omean)) and np.array_equal(r["count"].cpu().numpy(), ocount)
    assert F.sor_indices(omean, ocount, ratio)[1] == O.sor(omean, ocount, ratio)[1]
    # device tensors in, device tensors out, equal results
    d_kept, d_ind = F.remove_statistical_outlier(dev(eng, pts), nb, ratio, engine=eng)
    assert isinstance(d_kept, torch.Tensor) and d_kept.is_cuda and d_ind.dtype == torch.int64
    assert np.array_equal(d_ind.cpu().numpy(), ind) and np.array_equal(d_kept.cpu().numpy(), kept)


def test_point_cloud_sor_filter_end_to_end(eng, g16):
    from icepy4d_amd.core import PointCloud
    pc = PointCloud(points3d=g16["points"], points_col=g16["colors"], verbose=True)
    pc.sor_filter(engine=eng)
    assert np.array_equal(pc.get_points(), g16["sor10_points"]) and np.array_equal(pc.get_colors(), g16["sor10_colors_int"])
    assert len(pc) == len(g16["sor10_ind"])
    pc = PointCloud(points3d=g16["points"])
    pc.sor_filter(nb_neighbors=50, std_ratio=1.5, engine=eng)
    assert np.array_equal(pc.get_points(), g16["sor50_points"]) and pc.get_colors() is None
    # edge cases of the rule on the device: one point, identical points, fewer points than neighbours
    one = PointCloud(points3d=np.array([[1.0, 2.0, 3.0]]))
    one.sor_filter(engine=eng)
    assert len(one) == 0
    same = PointCloud(points3d=np.tile([[1.0, 2.0, 3.0]], (20, 1)))
    same.sor_filter(engine=eng)
    assert len(same) == 0
    few = np.random.default_rng(3).uniform(0, 1, (7, 3))
    few[6] = (30.0, 30.0, 30.0)
    pc = PointCloud(points3d=few)
    pc.sor_filter(nb_neighbors=10, std_ratio=1.0, engine=eng)
    assert np.array_equal(pc.get_points(), few[:6]) and np.array_equal(pc.get_points(), O.remove_statistical_outlier(few, 10, 1.0)[0])


# ---- normals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noisy_plane", "sphere_patch", "g16"])
def test_normals_against_eigh(eng, g16, name):
    from icepy4d_amd.core import PointCloud
    from icepy4d_amd.utils import point_cloud_filters as F
    pts, radius, max_nn = {"noisy_plane": (KC.noisy_plane(), 0.3, 30), "sphere_patch": (KC.sphere_patch(), 0.5, 30),
                           "g16": (g16["points"], 3.0, 30)}[name]
    idx, d2, count, _ = O.knn_self(pts, max_nn, radius * radius)
    ref, gap = O.normals(pts, idx, count)
    got = F.estimate_normals(pts, radius=radius, max_nn=max_nn, engine=eng)
    assert isinstance(got, np.ndarray) and got.shape == ref.shape and got.dtype == np.float64
    clear = gap >= 1e-6
    assert (~clear).mean() <= 0.01, (name, float((~clear).mean()))
    cross = np.linalg.norm(np.cross(got, ref), axis=1)
    print(f"{name}: worst |n_dev x n_ref| {cross[clear].max():.3e} over {int(clear.sum())} of {len(pts)} points")
    assert (cross[clear] <= 1e-8).all(), (name, float(cross[clear].max()))
    assert (np.abs(np.linalg.norm(got, axis=1) - 1.0) < 1e-12).all()
    signed = clear & (np.abs(ref[:, 2]) > 1e-6)
    assert (got[signed, 2] > 0).all() and (got[count < 3] == (0.0, 0.0, 1.0)).all()
    if name == "g16":
        assert (count < 3).any()                                                                   # the planted outliers are alone
        pc = PointCloud(points3d=pts)
        assert np.array_equal(pc.estimate_normals(radius=radius, max_nn=max_nn, engine=eng), got) and pc.get_normals() is pc.normals
        d_got = F.estimate_normals(dev(eng, pts), radius=radius, max_nn=max_nn, engine=eng)
        assert np.array_equal(d_got.cpu().numpy(), got)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def refused(eng, name, *args):
    from icepy4d_amd._lib import IcematchError
    with pytest.raises(IcematchError) as e:
        eng.ctx.call(name, *args)
    assert e.value.rc == REFUSED, (name, e.value)


def test_refusals_leave_the_outputs_alone(eng):
    case = KC.by_name("n65")
    s = Sorted(eng, case)
    n, k, st = s.n, 10, eng.stream_ptr()
    good = s.grid
    nx, ny, nz = (int(v) for v in s.dims)
    out = outputs(eng, n, k)
    o = [out[name].ptr for name in ("count", "idx", "d2", "mean", "normal", "rings")]
    grids = {"s = 0": [0, 0, 0, 0.0], "s < 0": [0, 0, 0, -1.0], "s = inf": [0, 0, 0, INF], "s = nan": [0, 0, 0, np.nan], "origin nan": [np.nan, 0, 0, 1.0]}
    bad_self = [("null points", (None, p(s.perm), s.start.ptr, n, good.ctypes.data, nx, ny, nz, k, INF)),
                ("null permutation", (p(s.d_pts), None, s.start.ptr, n, good.ctypes.data, nx, ny, nz, k, INF)),
                ("null ranges", (p(s.d_pts), p(s.perm), None, n, good.ctypes.data, nx, ny, nz, k, INF)),
                ("null grid", (p(s.d_pts), p(s.perm), s.start.ptr, n, None, nx, ny, nz, k, INF)),
                ("n < 0", (p(s.d_pts), p(s.perm), s.start.ptr, -1, good.ctypes.data, nx, ny, nz, k, INF)),
                ("n = 2^31", (p(s.d_pts), p(s.perm), s.start.ptr, 2 ** 31, good.ctypes.data, nx, ny, nz, k, INF)),
                ("k = 0", (p(s.d_pts), p(s.perm), s.start.ptr, n, good.ctypes.data, nx, ny, nz, 0, INF)),
                ("k = 65", (p(s.d_pts), p(s.perm), s.start.ptr, n, good.ctypes.data, nx, ny, nz, 65, INF)),
                ("nx = 0", (p(s.d_pts), p(s.perm), s.start.ptr, n, good.ctypes.data, 0, ny, nz, k, INF)),
                ("nz < 0", (p(s.d_pts), p(s.perm), s.start.ptr, n, good.ctypes.data, nx, ny, -3, k, INF)),
                ("cells above the cap", (p(s.d_pts), p(s.perm), s.start.ptr, n, good.ctypes.data, 4096, 4096, 2, k, INF)),
                ("cells overflow", (p(s.d_pts), p(s.perm), s.start.ptr, n, good.ctypes.data, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, k, INF)),
                ("radius2 < 0", (p(s.d_pts), p(s.perm), s.start.ptr, n, good.ctypes.data, nx, ny, nz, k, -1e-300)),
                ("radius2 nan", (p(s.d_pts), p(s.perm), s.start.ptr, n, good.ctypes.data, nx, ny, nz, k, np.nan))]
    for what, g in grids.items():
        arr = np.array(g, np.float64)
        bad_self.append((what, (p(s.d_pts), p(s.perm), s.start.ptr, n, arr.ctypes.data, nx, ny, nz, k, INF)))
    for what, args in bad_self:
        refused(eng, "im_knn_self", *args, *o, st)
        for f in out.values():
            f.untouched(("im_knn_self", what))
    key = Framed(eng, (n,), np.int64)
    bad_cells = [(None, n, good.ctypes.data, nx, ny, nz, key.ptr), (p(s.d_pts), n, good.ctypes.data, nx, ny, nz, None),
                 (p(s.d_pts), -1, good.ctypes.data, nx, ny, nz, key.ptr), (p(s.d_pts), 2 ** 31, good.ctypes.data, nx, ny, nz, key.ptr),
                 (p(s.d_pts), n, None, nx, ny, nz, key.ptr), (p(s.d_pts), n, good.ctypes.data, nx, 0, nz, key.ptr),
                 (p(s.d_pts), n, good.ctypes.data, 2 ** 12, 2 ** 12, 2, key.ptr)]
    for g in grids.values():
        arr = np.array(g, np.float64)
        bad_cells.append((p(s.d_pts), n, arr.ctypes.data, nx, ny, nz, key.ptr))
    for args in bad_cells:
        refused(eng, "im_knn_cells", *args, st)
        key.untouched(("im_knn_cells", args[1:]))
    start = Framed(eng, (s.cells + 1,), np.int32)
    for args in ((None, n, s.cells, start.ptr), (p(s.skey), n, s.cells, None), (p(s.skey), -1, s.cells, start.ptr), (p(s.skey), 2 ** 31, s.cells, start.ptr),
                 (p(s.skey), n, 0, start.ptr), (p(s.skey), n, 2 ** 24 + 1, start.ptr)):
        refused(eng, "im_knn_cell_ranges", *args, st)
        start.untouched(("im_knn_cell_ranges", args[1:]))
    from icepy4d_amd.utils.point_cloud_filters import max_cells
    assert max_cells() == 2 ** 24


def test_an_empty_cloud_launches_nothing(eng):
    case = KC.by_name("n65")
    s = Sorted(eng, case)
    out = outputs(eng, 4, 10)
    call_self(eng, s.d_pts, s.perm, s.start.ptr, 0, s.grid, s.dims, 10, INF, out)
    for name, f in out.items():
        f.untouched(("n == 0", name))
    key, start = Framed(eng, (4,), np.int64), Framed(eng, (s.cells + 1,), np.int32)
    eng.ctx.call("im_knn_cells", p(s.d_pts), 0, s.grid.ctypes.data, *[int(v) for v in s.dims], key.ptr, eng.stream_ptr())
    eng.ctx.call("im_knn_cell_ranges", p(s.skey), 0, s.cells, start.ptr, eng.stream_ptr())
    key.untouched("im_knn_cells, n == 0")
    start.untouched("im_knn_cell_ranges, n == 0")
