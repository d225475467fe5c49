"""The ball-feature kernel (csrc/ballfeat.hip, csrc/ball_point.h) on the device, at every boundary between two code paths
(tests/ball_cases.py: cloud sizes around the 64-candidate batch, a radius that holds the whole cloud and one that holds only the query,
coincident points, a lattice whose boundary distance is exact, offsets of exactly +-2^18 steps, a cell of 700 points and a ball of 5000,
degenerate grids, far outliers whose stretched grid makes queries give the box up for a scan of the whole cloud, a world frame, points
on cell faces), the Python layer at any cell size, the top border of tests/golden/g18_top_border.npz through
`detect_border_by_geometry`, and the refusals of the C entry point.

Bounds. count, the ten sums, eig, normal and the thirteen arithmetic features: equality of bits with the brute-force restatement
(tests/ball_oracle.py) for every point of every case. Derived, not measured: the sums are exact integers, a function of the input alone
whatever the grid, the lanes and the order of the reduction; everything after them is the same IEEE float64 operations in the same order
with contraction off, and float64 division and sqrt are correctly rounded on the device. The host build of the same text agrees with the
restatement on the same cases (tests/test_ballfeat_cpu.py); what only this file can show is the wave-level walk, the reduction, the
int64 -> float64 conversion of the device and a lost `#pragma clang fp contract(off)`. The sign of `steps` equals the restatement's
prediction of which queries give their box up. Omnivariance and EigenEntropy, which call cbrt and log, are compared with numpy on the
device's own eig: relative 64 * 2^-52, and absolute 64 * 2^-52 * sum |l ln l| (both libraries document about 2 ulp, three terms).

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
import ball_oracle as B  # noqa: E402

pytestmark = pytest.mark.gpu

BAND, SENT, FILL = 4096, 0xA5, 0x5A
REFUSED = -75
LIMIT_S = 5.0             # every launch of a case, outputs downloaded: a walk whose work grows with the grid would take minutes
NK = len(B.KINDS)
ULP64 = 64 * 2.0 ** -52


@pytest.fixture(scope="module")
def g18():
    with np.load(B.GOLDEN, allow_pickle=False) as z:
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


def outputs(eng, n, n_kinds):
    return {"count": Framed(eng, (n,), np.int32), "sums": Framed(eng, (n, 10), np.int64), "eig": Framed(eng, (n, 3), np.float64),
            "normal": Framed(eng, (n, 3), np.float64), "feat": Framed(eng, (n, n_kinds), np.float64), "steps": Framed(eng, (n,), np.int32)}


ORDER = ("count", "sums", "eig", "normal", "feat", "steps")


class Sorted:
    """A case's cloud on the device, binned and sorted once by the calls the k-NN uses."""

    def __init__(self, eng, case):
        import torch
        self.case, self.n = case, len(case["points"])
        self.grid, self.dims = BC.grid(case)
        self.cells = int(np.prod(self.dims.astype(np.int64)))
        self.d_pts = dev(eng, case["points"])
        key = torch.empty(self.n, dtype=torch.int64, device=eng.device)
        eng.ctx.call("im_knn_cells", p(self.d_pts), self.n, self.grid.ctypes.data, *[int(v) for v in self.dims], p(key), eng.stream_ptr())
        self.skey, self.perm = torch.sort(key, stable=True)
        self.start = torch.empty(self.cells + 1, dtype=torch.int32, device=eng.device)
        eng.ctx.call("im_knn_cell_ranges", p(self.skey), self.n, self.cells, p(self.start), eng.stream_ptr())

    def args(self, radius=None, n=None):
        return (p(self.d_pts), p(self.perm), p(self.start), self.n if n is None else n, self.grid.ctypes.data, *[int(v) for v in self.dims],
                self.case["r"] if radius is None else radius)

    def run(self, eng, kinds):
        kinds = np.array(kinds, np.int32)
        out = outputs(eng, self.n, len(kinds))
        eng.ctx.call("im_ball_features", *self.args(), kinds.ctypes.data, len(kinds), *[out[k].ptr for k in ORDER], eng.stream_ptr())
        return {name: f.result((self.case["name"], name)) for name, f in out.items()}


def check_against(got, want, kinds, what):
    assert np.array_equal(got["count"], want["count"]), what
    assert np.array_equal(got["sums"], want["sums"]), what
    assert np.array_equal(bits(got["eig"]), bits(want["eig"])), what
    assert np.array_equal(bits(got["normal"]), bits(want["normal"])), what
    for j, k in enumerate(kinds):
        assert np.array_equal(bits(got["feat"][:, j]), bits(want[B.KINDS[k]])), (what, B.KINDS[k])


# ---- every case of the shared list: bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.names())
def test_features_equal_the_restatement_bit_for_bit(eng, name):
    case = BC.by_name(name)
    s = Sorted(eng, case)
    want = BC.expected(name)
    eng.synchronize()
    t0 = time.perf_counter()
    got = s.run(eng, list(range(NK)))                                  # downloads the outputs: the launch has finished
    took = time.perf_counter() - t0
    check_against(got, want, list(range(NK)), name)
    R, falls_back = BC.expected_walk(name)
    steps = got["steps"]
    assert (steps != 0).all() and np.array_equal(steps < 0, falls_back), (name, int((steps < 0).sum()), int(falls_back.sum()))
    assert (steps[falls_back] == -((s.n + 63) // 64)).all()
    budget = 1024 + s.n // 32
    assert (steps[~falls_back] <= budget + (s.n + 63) // 64 + s.n).all(), name      # bounded work: the lookups, the batches, a part batch per row
    assert took < LIMIT_S, (name, "the launch took", took)
    if name.startswith("far_outlier") and name != "far_outlier_x":
        assert (steps < 0).any() and (steps > 0).any()


def test_an_empty_cloud_launches_nothing(eng):
    s = Sorted(eng, BC.by_name("n65"))
    kinds = np.arange(NK, dtype=np.int32)
    out = outputs(eng, 4, NK)
    eng.ctx.call("im_ball_features", *s.args(n=0), kinds.ctypes.data, NK, *[out[k].ptr for k in ORDER], eng.stream_ptr())
    for name, f in out.items():
        f.untouched(("n == 0", name))


def test_every_output_is_optional_and_kinds_may_repeat(eng):
    name = "n129"
    s = Sorted(eng, BC.by_name(name))
    want = BC.expected(name)
    st = eng.stream_ptr()
    # sixteen kinds, in another order and with repeats: column j is kind j of the list
    kinds = np.array([8, 4, 12, 0, 11, 4, 1, 2, 3, 5, 6, 7, 9, 10, 8, 4], np.int32)
    feat = Framed(eng, (s.n, 16), np.float64)
    eng.ctx.call("im_ball_features", *s.args(), kinds.ctypes.data, 16, None, None, None, None, feat.ptr, None, st)
    got = feat.result("features alone")
    for j, k in enumerate(kinds):
        assert np.array_equal(bits(got[:, j]), bits(want[B.KINDS[k]])), (j, k)
    # one kind: a row is one value
    one = Framed(eng, (s.n, 1), np.float64)
    k1 = np.array([4], np.int32)
    eng.ctx.call("im_ball_features", *s.args(), k1.ctypes.data, 1, None, None, None, None, one.ptr, None, st)
    assert np.array_equal(bits(one.result("one kind")[:, 0]), bits(want["Linearity"]))
    # no kinds at all, and each other output alone
    for alone in ("count", "sums", "eig", "normal", "steps"):
        out = outputs(eng, s.n, 1)
        ptrs = [out[k].ptr if k == alone else None for k in ORDER]
        eng.ctx.call("im_ball_features", *s.args(), None, 0, *ptrs, st)
        res = out[alone].result(alone)
        if alone in ("count", "sums"):
            assert np.array_equal(res, want[alone])
        elif alone != "steps":
            assert np.array_equal(bits(res), bits(want[alone]))
        for k in ORDER:
            if k != alone:
                out[k].untouched((alone, k))


# ---- the Python layer: the result does not depend on the grid ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n129", "coincident", "far_outlier_y", "exact_radius", "world_frame"])
def test_ball_features_with_any_cell_size(eng, name):
    import torch
    from icepy4d_amd.utils import point_cloud_filters as F
    case = BC.by_name(name)
    pts, r = case["points"], case["r"]
    want = BC.expected(name)
    names = ("Linearity", "Verticality", "EigenValuesSum", "NumberOfNeighbors")
    sizes = [{}, {"cell_size": r / 8}, {"cell_size": 4 * r}]
    if len(pts) <= 301:
        sizes += [{"cell_size": 1e-9}, {"cell_size": 1e9}]
    for kw in sizes:
        t0 = time.perf_counter()
        got = F.ball_features(pts, r, features=names, engine=eng, want=("count", "sums", "eig", "normal", "steps"), **kw)
        assert time.perf_counter() - t0 < LIMIT_S, (name, kw)
        assert all(isinstance(v, np.ndarray) for v in got.values())
        assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["sums"], want["sums"]), (name, kw)
        assert np.array_equal(bits(got["eig"]), bits(want["eig"])) and np.array_equal(bits(got["normal"]), bits(want["normal"])), (name, kw)
        for f in names:
            assert got[f].shape == (len(pts),) and np.array_equal(bits(got[f]), bits(want[f])), (name, kw, f)
        if kw.get("cell_size") == 1e9:
            assert (got["steps"] == (len(pts) + 63) // 64 + 1).all()           # one cell: one lookup, then the whole cloud
    d = F.ball_features(dev(eng, pts), r, features="Planarity", engine=eng)                      # a device tensor in, a name alone
    assert isinstance(d["Planarity"], torch.Tensor) and d["Planarity"].is_cuda and list(d) == ["Planarity"]
    assert np.array_equal(bits(d["Planarity"].cpu().numpy()), bits(want["Planarity"]))


def test_omnivariance_and_eigen_entropy(eng):
    from icepy4d_amd.post_processing.cloudcompare_fun import GeomFeature, compute_feature
    from icepy4d_amd.utils import point_cloud_filters as F
    for name in ("world_frame", "ball_5000", "coincident"):
        case = BC.by_name(name)
        got = F.ball_features(case["points"], case["r"], features=("Omnivariance", "EigenEntropy", "Sphericity"), engine=eng, want=("eig",))
        eig = got["eig"]
        assert np.array_equal(bits(eig), bits(BC.expected(name)["eig"]))
        ok = ~np.isnan(eig[:, 0])
        assert ok.any() and np.isnan(got["Omnivariance"][~ok]).all() and np.isnan(got["EigenEntropy"][~ok]).all()
        omni = B.omnivariance(eig[ok])
        ent, mag = B.eigen_entropy(eig[ok])
        eo, ee = np.abs(got["Omnivariance"][ok] - omni), np.abs(got["EigenEntropy"][ok] - ent)
        print(f"{name}: Omnivariance worst {np.max(eo / np.maximum(omni, 1e-300)) / 2.0 ** -52:.2f} ulp, "
              f"EigenEntropy worst {np.max(ee / np.maximum(mag, 1e-300)) / 2.0 ** -52:.2f} ulp of sum |l ln l|")
        assert (eo <= ULP64 * omni).all(), (name, float(np.max(eo / np.maximum(omni, 1e-300))))
        assert (ee <= ULP64 * mag).all(), (name, float(np.max(ee / np.maximum(mag, 1e-300))))
    case = BC.by_name("n129")
    one = compute_feature(GeomFeature.Verticality, case["r"], case["points"], engine=eng)
    assert isinstance(one, np.ndarray) and np.array_equal(bits(one), bits(BC.expected("n129")["Verticality"]))
    assert np.array_equal(bits(compute_feature("Sphericity", case["r"], case["points"], engine=eng)), bits(BC.expected("n129")["Sphericity"]))
    empty = F.ball_features(np.zeros((0, 3)), 1.0, features=("Linearity", "Omnivariance"), engine=eng, want=("count", "sums"))
    assert empty["Linearity"].shape == (0,) and empty["Omnivariance"].shape == (0,) and empty["sums"].shape == (0, 10)


# ---- the top border: two radii in one call, against the golden --------------------------------------------------------------------------
def test_detect_border_by_geometry_reproduces_g18(eng, g18, tmp_path):
    from icepy4d_amd import top_border as T
    from icepy4d_amd.core import PointCloud
    from icepy4d_amd.utils import point_cloud_filters as F
    borders = []
    for k, date in enumerate(g18["dates"]):
        pts = np.array(g18[f"points{k}"])
        lin = F.ball_features(pts, 2.0, features=("Linearity",), engine=eng)["Linearity"]
        ver = F.ball_features(pts, 0.15, features=("Verticality",), engine=eng)["Verticality"]
        assert np.array_equal(bits(lin), bits(g18[f"linearity{k}"])) and np.array_equal(bits(ver), bits(g18[f"verticality{k}"])), k
        colours = np.random.default_rng(k).uniform(0, 1, (len(pts), 3))
        cloud = PointCloud(points3d=pts, points_col=colours)
        cloud.normals = np.random.default_rng(10 + k).normal(0, 1, (len(pts), 3))
        border = T.detect_border_by_geometry(cloud, engine=eng)
        idx = g18[f"border{k}"]
        assert np.array_equal(border.points, pts[idx]) and np.array_equal(border.colors, colours[idx]), k
        assert np.array_equal(border.normals, cloud.normals[idx]) and len(cloud) == len(pts)
        borders.append(border)
    names = [f"border_{d}.ply" for d in g18["dates"]]
    T.border_table(borders, out_path=tmp_path / "top_border_coords.txt", names=names)
    assert (tmp_path / "top_border_coords.txt").read_bytes() == bytes(g18["csv"])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(eng):
    from icepy4d_amd._lib import IcematchError
    s = Sorted(eng, BC.by_name("n65"))
    n, r, st = s.n, s.case["r"], eng.stream_ptr()
    nx, ny, nz = (int(v) for v in s.dims)
    good, pts, perm, start = s.grid.ctypes.data, p(s.d_pts), p(s.perm), p(s.start)
    kinds = np.arange(NK, dtype=np.int32)
    K = kinds.ctypes.data
    out = outputs(eng, n, NK)
    o = [out[k].ptr for k in ORDER]
    bad_kind, neg_kind = np.array([4, NK], np.int32), np.array([-1], np.int32)
    grids = {"s = 0": [0, 0, 0, 0.0], "s < 0": [0, 0, 0, -1.0], "s = inf": [0, 0, 0, np.inf], "s = nan": [0, 0, 0, np.nan],
             "origin nan": [np.nan, 0, 0, 1.0], "origin inf": [0, np.inf, 0, 1.0]}
    held = {what: np.array(g, np.float64) for what, g in grids.items()}
    bad = [("null points", (None, perm, start, n, good, nx, ny, nz, r, K, NK)),
           ("null permutation", (pts, None, start, n, good, nx, ny, nz, r, K, NK)),
           ("null ranges", (pts, perm, None, n, good, nx, ny, nz, r, K, NK)),
           ("null grid", (pts, perm, start, n, None, nx, ny, nz, r, K, NK)),
           ("null kinds", (pts, perm, start, n, good, nx, ny, nz, r, None, 3)),
           ("n < 0", (pts, perm, start, -1, good, nx, ny, nz, r, K, NK)),
           ("n = 2^26 + 1", (pts, perm, start, 2 ** 26 + 1, good, nx, ny, nz, r, K, NK)),
           ("r = 0", (pts, perm, start, n, good, nx, ny, nz, 0.0, K, NK)),
           ("r < 0", (pts, perm, start, n, good, nx, ny, nz, -1.0, K, NK)),
           ("r = inf", (pts, perm, start, n, good, nx, ny, nz, np.inf, K, NK)),
           ("r = nan", (pts, perm, start, n, good, nx, ny, nz, np.nan, K, NK)),
           ("h denormal", (pts, perm, start, n, good, nx, ny, nz, 2.0 ** -1010, K, NK)),
           ("nx = 0", (pts, perm, start, n, good, 0, ny, nz, r, K, NK)),
           ("nz < 0", (pts, perm, start, n, good, nx, ny, -3, r, K, NK)),
           ("cells above the cap", (pts, perm, start, n, good, 4096, 4096, 2, r, K, NK)),
           ("cells overflow", (pts, perm, start, n, good, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, r, K, NK)),
           ("n_kinds < 0", (pts, perm, start, n, good, nx, ny, nz, r, K, -1)),
           ("n_kinds = 17", (pts, perm, start, n, good, nx, ny, nz, r, K, 17)),
           ("unknown kind", (pts, perm, start, n, good, nx, ny, nz, r, bad_kind.ctypes.data, 2)),
           ("negative kind", (pts, perm, start, n, good, nx, ny, nz, r, neg_kind.ctypes.data, 1))]
    for what, arr in held.items():
        bad.append((what, (pts, perm, start, n, arr.ctypes.data, nx, ny, nz, r, K, NK)))
    for what, args in bad:
        with pytest.raises(IcematchError) as e:
            eng.ctx.call("im_ball_features", *args, *o, st)
        assert e.value.rc == REFUSED, (what, e.value)
        for f in out.values():
            f.untouched(what)
    # the smallest radius whose step is a normal number is served
    ok = outputs(eng, n, NK)
    eng.ctx.call("im_ball_features", pts, perm, start, n, good, nx, ny, nz, 2.0 ** -1004, K, NK, *[ok[k].ptr for k in ORDER], st)
    assert (ok["count"].result("tiny radius") >= 1).all()
