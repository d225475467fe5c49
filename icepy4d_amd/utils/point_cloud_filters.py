"""Neighbourhood work on point clouds, on the device: `knn_search` (the exact k nearest neighbours of every point within its own cloud),
`remove_statistical_outlier` (SOR; the reference's `core/point_cloud.py::PointCloud.sor_filter` with 10 / 3.0 and
`post_processing/open3d_fun.py::MeshingPoisson.SOR` with 50 / 1.5) and `estimate_normals` (`open3d_fun.py:178-180`, hybrid search with
radius 1 and 30 neighbours). One primitive carries all three: csrc/knn.hip (`im_knn_cells`, `im_knn_cell_ranges`, `im_knn_self`; the one
stable sort by cell key is torch's). Every entry point takes an optional `engine=` (default: the shared engine of device 0) and numpy
arrays or device tensors; there is no CPU fallback: without a HIP device the calls raise. Non-finite coordinates raise ValueError before
any launch.

Numerics (tests/test_gpu_pointcloud.py): neighbour indices, counts, squared distances and the mean neighbour distance are bit-identical to
the brute-force restatement tests/knn_oracle.py: float64, d2 = ((dx*dx) + (dy*dy)) + (dz*dz), ascending, the lower index first among
equal distances, the point itself included at distance 0. That holds for any cell size: the grid decides the speed, never the result.

PARITY WITH AN OPEN3D BINARY IS UNPINNED. Open3D is not a dependency; its published algorithms are restated:
  - remove_statistical_outlier: avg_i = mean distance to the nb_neighbors nearest (the point itself among them), cloud mean and sample
    standard deviation over the avg_i > 0 (the mean divided by the number of points with a neighbour), kept iff 0 < avg_i < mean +
    std_ratio * std. What could differ from a binary: its KD-tree's choice among neighbours at exactly equal distance (ours: the lower
    index), the order and width of its sums (ours: float64, left to right, on the host), hence a point whose avg_i lies within rounding
    of the threshold.
  - estimate_normals: the eigenvector of the smallest eigenvalue of the two-pass covariance of the neighbours with d2 <= radius^2, at most
    max_nn of them, by cyclic Jacobi; fewer than three neighbours give (0, 0, 1). Open3D's closed-form eigen solver and its sign are not
    reproduced: ours makes the first non-zero of (n_z, n_y, n_x) positive. What could differ: the sign, and the direction where two
    eigenvalues nearly coincide.

`ball_features` (csrc/ballfeat.hip, `im_ball_features`) serves the reference's `scripts/pcd_postprocessing/top_border.py`, which asks
CloudCompare for `computeFeature(Linearity, 2.0)` and `computeFeature(Verticality, 0.15)`: the eigen-decomposition of the covariance of ALL
points within a radius of each point, hundreds to thousands of them, which the 64-slot list above cannot hold. CloudCompare is not a
dependency and the features have a definition of their own: offsets quantised to r * 2^-18 and summed exactly in int64, so
that the result is a function of the input alone, bit-identical to tests/ball_oracle.py for any cell size. PARITY WITH A CLOUDCOMPARE
BINARY IS UNPINNED: what could differ is its float32 storage of coordinates, its eigen solver and, at the scale of the quantisation step
(7.6 um at r = 2 m), which points lie in a ball.

`voxel_down_sample` (csrc/voxel.hip) thins a cloud before any of the above: one output point per filled voxel of the grid of
`post_processing/voxel_grid.py`, the mean of the voxel's points (the reference: `scripts/tracking_experimental.py:462,602`). Bit-identical
to tests/voxel_oracle.py; parity with an Open3D binary is unpinned (its output order is a hash map's, ours ascending voxel key).

`knn_cross`, `ball_cross` and `cylinder_stats` (csrc/cloud_distance.hip) ask a TARGET cloud at external queries: the nearest target
points, the ball's sums and normal, and the statistics of the target inside a cylinder along a normal, the pieces of cloud-to-cloud
distances and M3C2 (`post_processing/cloud_distance.py`). The grid comes from the target; the queries may lie anywhere. Bit-identical to
tests/cloud_distance_oracle.py for any cell size and any query order; parity with CloudCompare or Open3D is unpinned."""
import math

import numpy as np
import torch

from .._lib import ptr
from ..engine import default_engine, to_device

MAX_K = 64
MAX_BALL_POINTS = 2 ** 26
# the kind codes of include/icematch.h (im_ball_kind), CloudCompare's member names
BALL_KINDS = {"EigenValuesSum": 0, "PCA1": 1, "PCA2": 2, "SurfaceVariation": 3, "Linearity": 4, "Planarity": 5, "Anisotropy": 6,
              "Sphericity": 7, "Verticality": 8, "EigenValue1": 9, "EigenValue2": 10, "EigenValue3": 11, "NumberOfNeighbors": 12}
BALL_DERIVED = ("Omnivariance", "EigenEntropy")      # from `eig` with torch on the device: cbrt and log are not bit-pinned
CELL_OCCUPANCY = 0.25      # tunable: the cell size is chosen so that an occupied cell holds about CELL_OCCUPANCY * k points


def max_cells() -> int:
    """The largest grid (in cells) `im_knn_self` accepts."""
    from .._lib import load
    return int(load().im_knn_max_cells())


def _device_points(points, dev):
    pts = points.to(device=dev, dtype=torch.float64).contiguous() if isinstance(points, torch.Tensor) else to_device(points, dev, np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be [n, 3] (got {tuple(pts.shape)})")
    if pts.shape[0] >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 points")
    if pts.shape[0] and not bool(torch.isfinite(pts).all()):
        raise ValueError("points hold non-finite coordinates")
    return pts


def grid_dims(lo, hi, s):
    """Cells per axis of the grid of cell size s over the box [lo, hi]: floor((hi - lo) / s) + 1, the kernels' own arithmetic."""
    return [int(v) + 1 for v in np.floor((np.asarray(hi, np.float64) - np.asarray(lo, np.float64)) / np.float64(s))]


def fit_cell_size(lo, hi, s, cap):
    """s, enlarged until the grid over [lo, hi] holds at most `cap` cells."""
    s = float(s)
    for _ in range(200):
        with np.errstate(over="ignore"):
            n = np.floor((np.asarray(hi, np.float64) - np.asarray(lo, np.float64)) / np.float64(s)) + 1.0
        cells = float(n[0]) * float(n[1]) * float(n[2])
        if cells <= cap:
            return s
        s *= max(1.05, min(2.0 ** 300, (cells / cap) ** (1.0 / 3.0)))
    raise ValueError("no cell size fits the grid under the cell cap")


def _occupied(eng, pts, lo, s, dims):
    key = torch.empty(pts.shape[0], dtype=torch.int64, device=pts.device)
    grid = np.array([lo[0], lo[1], lo[2], s], np.float64)
    eng.ctx.call("im_knn_cells", ptr(pts), pts.shape[0], grid.ctypes.data, dims[0], dims[1], dims[2], ptr(key), eng.stream_ptr())
    return int(torch.unique(key).numel())


def choose_cell_size(eng, pts, lo, hi, k, occupancy=None):
    """The heuristic behind `cell_size=None`: two coarse binnings (64 and 128 cells along the longest axis) give the number of occupied
    cells m at two sizes, hence the cloud's box-counting dimension D in 1..3 (a surface: about 2); m(s) ~ s^-D is then solved for
    n / m(s) = occupancy * k points per occupied cell. A tunable, not a condition of correctness."""
    n = pts.shape[0]
    ext = float(np.max(np.asarray(hi) - np.asarray(lo)))
    if n < 2 or not ext > 0.0:
        return 1.0
    target = max(1.0, (CELL_OCCUPANCY if occupancy is None else float(occupancy)) * k)
    s1, s2 = ext / 64.0, ext / 128.0
    if not (s2 > 0.0 and math.isfinite(s1)):
        return ext
    m1 = _occupied(eng, pts, lo, s1, grid_dims(lo, hi, s1))
    m2 = _occupied(eng, pts, lo, s2, grid_dims(lo, hi, s2))
    D = min(3.0, max(1.0, math.log2(max(m2, 1) / max(m1, 1)))) if m2 > m1 else 1.0
    s = s2 * (m2 * target / n) ** (1.0 / D)
    return s if (s > 0.0 and math.isfinite(s)) else ext


def _bounds(pts):
    return pts.min(0).values.cpu().numpy(), pts.max(0).values.cpu().numpy()


def _binned(eng, pts, lo, hi, s):
    """The cloud binned into the grid of cell size s (enlarged to fit the cell cap) over [lo, hi]: (s, dims, h_grid, perm, start), what
    `im_knn_self` and `im_ball_features` take: keys by `im_knn_cells`, one stable sort, cell ranges by `im_knn_cell_ranges`."""
    n, dev = pts.shape[0], pts.device
    s = fit_cell_size(lo, hi, s, max_cells())
    dims = grid_dims(lo, hi, s)
    cells = dims[0] * dims[1] * dims[2]
    st = eng.stream_ptr()
    grid = np.array([lo[0], lo[1], lo[2], s], np.float64)
    key = torch.empty(n, dtype=torch.int64, device=dev)
    eng.ctx.call("im_knn_cells", ptr(pts), n, grid.ctypes.data, dims[0], dims[1], dims[2], ptr(key), st)
    skey, perm = torch.sort(key, stable=True)
    start = torch.empty(cells + 1, dtype=torch.int32, device=dev)
    eng.ctx.call("im_knn_cell_ranges", ptr(skey), n, cells, ptr(start), st)
    return s, dims, grid, perm, start


def knn_self(points, k, radius=None, cell_size=None, want=("idx", "d2", "count"), occupancy=None, engine=None):
    """The primitive: {name: device tensor} for the names in `want` out of idx [n, k] int32, d2 [n, k] float64, count [n] int32, mean [n]
    float64 (SOR's statistic), normal [n, 3] float64, rings [n] int32 (rings of cells the search visited, the query's cell counted; negated where
    the search spent its step budget and ended by a scan of the whole cloud),
    plus "cell_size" and "dims" (host values). All are addressed by the original point index."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be 1..{MAX_K} (got {k})")
    if radius is not None and not float(radius) >= 0.0:
        raise ValueError(f"radius must be >= 0 (got {radius})")
    if cell_size is not None and not (float(cell_size) > 0.0 and math.isfinite(float(cell_size))):
        raise ValueError(f"cell_size must be finite and positive (got {cell_size})")
    unknown = set(want) - {"idx", "d2", "count", "mean", "normal", "rings"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    eng = default_engine(engine)
    dev = eng.device
    pts = _device_points(points, dev)
    n = pts.shape[0]
    shapes = {"idx": ((n, k), torch.int32), "d2": ((n, k), torch.float64), "count": ((n,), torch.int32), "mean": ((n,), torch.float64),
              "normal": ((n, 3), torch.float64), "rings": ((n,), torch.int32)}
    out = {name: torch.empty(shapes[name][0], dtype=shapes[name][1], device=dev) for name in want}
    if n == 0:
        out["cell_size"], out["dims"] = 1.0 if cell_size is None else float(cell_size), [1, 1, 1]
        return out
    lo, hi = _bounds(pts)
    s = choose_cell_size(eng, pts, lo, hi, k, occupancy) if cell_size is None else float(cell_size)
    s, dims, grid, perm, start = _binned(eng, pts, lo, hi, s)
    st = eng.stream_ptr()
    r2 = math.inf if radius is None else float(radius) * float(radius)
    eng.ctx.call("im_knn_self", ptr(pts), ptr(perm), ptr(start), n, grid.ctypes.data, dims[0], dims[1], dims[2], k, r2,
                 ptr(out.get("count")), ptr(out.get("idx")), ptr(out.get("d2")), ptr(out.get("mean")), ptr(out.get("normal")),
                 ptr(out.get("rings")), st)
    out["cell_size"], out["dims"] = s, dims
    return out


def knn_search(points, k, radius=None, cell_size=None, engine=None, occupancy=None):
    """(idx [n, k] int32, d2 [n, k] float64, count [n] int32), device tensors: for every point its `count` nearest points of the same
    cloud, itself first at distance 0, ascending by squared distance with the lower index first among equal distances; unused slots are
    -1 / +inf. count = min(k, n), or fewer under `radius` (a neighbour is dropped iff d2 > radius^2). `cell_size=None` chooses the grid
    from the cloud (`choose_cell_size`; `occupancy` overrides CELL_OCCUPANCY); the result does not depend on it."""
    r = knn_self(points, k, radius=radius, cell_size=cell_size, want=("idx", "d2", "count"), occupancy=occupancy, engine=engine)
    return r["idx"], r["d2"], r["count"]


def sor_indices(avg, count, std_ratio):
    """Open3D's published rule on the downloaded statistic: (ind ascending int64, threshold). The two sums run in index order on the host
    (np.cumsum adds left to right), which keeps the threshold bit-identical to the restatement; eight bytes per point is nothing next to
    the search."""
    avg = np.asarray(avg, np.float64)
    valid = int((np.asarray(count) > 0).sum())
    pos = avg > 0
    if valid == 0 or not pos.any():
        return np.zeros(0, np.int64), math.nan
    with np.errstate(invalid="ignore", divide="ignore"):
        cloud_mean = np.cumsum(avg[pos])[-1] / np.float64(valid)
        dev = avg[pos] - cloud_mean
        std_dev = np.sqrt(np.cumsum(dev * dev)[-1] / np.float64(valid - 1))       # valid == 1: NaN, nothing is kept
        threshold = cloud_mean + np.float64(std_ratio) * std_dev
        keep = pos & (avg < threshold)
    return np.nonzero(keep)[0].astype(np.int64), float(threshold)


def remove_statistical_outlier(points, nb_neighbors, std_ratio, engine=None, cell_size=None):
    """Statistical outlier removal as Open3D publishes it (module docstring; parity with an Open3D binary is unpinned):
    (kept_points [m, 3], ind [m] ascending). numpy in, numpy out; device tensors in, device tensors out."""
    if int(nb_neighbors) < 1 or not float(std_ratio) > 0.0:
        raise ValueError("remove_statistical_outlier: nb_neighbors must be >= 1 and std_ratio > 0")
    if int(nb_neighbors) > MAX_K:
        raise ValueError(f"remove_statistical_outlier: nb_neighbors above {MAX_K} is not supported")
    is_tensor = isinstance(points, torch.Tensor)
    r = knn_self(points, int(nb_neighbors), cell_size=cell_size, want=("count", "mean"), engine=engine)
    ind, _ = sor_indices(r["mean"].cpu().numpy(), r["count"].cpu().numpy(), std_ratio)
    if is_tensor:
        d_ind = to_device(ind, points.device)
        return points.reshape(-1, 3)[d_ind], d_ind
    return np.asarray(points).reshape(-1, 3)[ind], ind


def estimate_normals(points, radius=1.0, max_nn=30, engine=None, cell_size=None):
    """Normals [n, 3] float64 of the hybrid neighbourhoods (d2 <= radius^2, at most max_nn, the point itself among them); `radius=None`
    is a plain k-nearest search. See the module docstring for what is and is not Open3D's. numpy in, numpy out; tensor in, tensor out."""
    r = knn_self(points, int(max_nn), radius=radius, cell_size=cell_size, want=("normal",), engine=engine)
    return r["normal"] if isinstance(points, torch.Tensor) else r["normal"].cpu().numpy()


def _cbrt(x):
    """Cube root of x >= 0 (torch has none): pow with the rounded exponent 1 / 3, then one Newton step, which leaves about an ulp."""
    y = torch.pow(x, 1.0 / 3.0)
    return torch.where(y > 0.0, y - (y * y * y - x) / (3.0 * y * y), y)


def ball_features(points, radius, features=("Linearity",), cell_size=None, engine=None, want=()):
    """Geometric features of the ball of `radius` around every point (module docstring): {name: [n] float64} for the names in
    `features` (CloudCompare's: the keys of BALL_KINDS, plus "Omnivariance" = cbrt(l1 l2 l3) and "EigenEntropy" = -sum l ln l, a zero term
    counting 0), plus any of `want`: count [n] int32, sums [n, 10] int64, eig [n, 3] float64 (descending, m^2), normal [n, 3] float64,
    steps [n] int32 (the query's work; negative where it scanned the whole cloud). A ball of fewer than three points or without extent gives
    NaN. Several features of one radius cost one launch. `cell_size` (default radius / 2, enlarged to fit the cell cap) is a tunable: the
    result does not depend on it. numpy in, numpy out; tensor in, tensors out."""
    radius = float(radius)
    if not (radius > 0.0 and math.isfinite(radius)) or radius * 2.0 ** -18 < 2.2250738585072014e-308:
        raise ValueError(f"radius must be finite and positive, and radius * 2^-18 a normal number (got {radius})")
    if cell_size is not None and not (float(cell_size) > 0.0 and math.isfinite(float(cell_size))):
        raise ValueError(f"cell_size must be finite and positive (got {cell_size})")
    features = (features,) if isinstance(features, str) else tuple(features)
    unknown = [f for f in features if f not in BALL_KINDS and f not in BALL_DERIVED]
    if unknown:
        raise ValueError(f"unknown features {unknown}")
    unknown = set(want) - {"count", "sums", "eig", "normal", "steps"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    eng = default_engine(engine)
    dev = eng.device
    pts = _device_points(points, dev)
    n = pts.shape[0]
    if n > MAX_BALL_POINTS:
        raise ValueError("at most 2^26 points")
    kinds = sorted({BALL_KINDS[f] for f in features if f in BALL_KINDS})
    derived = any(f in BALL_DERIVED for f in features)
    shapes = {"count": ((n,), torch.int32), "sums": ((n, 10), torch.int64), "eig": ((n, 3), torch.float64), "normal": ((n, 3), torch.float64),
              "steps": ((n,), torch.int32)}
    raw = {name: torch.empty(shapes[name][0], dtype=shapes[name][1], device=dev) for name in set(want) | ({"eig"} if derived else set())}
    feat = torch.empty((n, len(kinds)), dtype=torch.float64, device=dev) if kinds else None
    if n > 0:
        lo, hi = _bounds(pts)
        _, dims, grid, perm, start = _binned(eng, pts, lo, hi, radius / 2.0 if cell_size is None else float(cell_size))
        h_kinds = np.array(kinds, np.int32)
        eng.ctx.call("im_ball_features", ptr(pts), ptr(perm), ptr(start), n, grid.ctypes.data, dims[0], dims[1], dims[2], radius,
                     h_kinds.ctypes.data if kinds else None, len(kinds), ptr(raw.get("count")), ptr(raw.get("sums")), ptr(raw.get("eig")),
                     ptr(raw.get("normal")), ptr(feat), ptr(raw.get("steps")), eng.stream_ptr())
    out = {}
    for f in features:
        if f in BALL_KINDS:
            out[f] = feat[:, kinds.index(BALL_KINDS[f])].contiguous()
        elif f == "Omnivariance":
            e = raw["eig"]
            out[f] = _cbrt(e[:, 0] * e[:, 1] * e[:, 2])
        else:
            e = raw["eig"]
            terms = torch.where(e == 0.0, torch.zeros_like(e), e * torch.log(e))
            out[f] = -((terms[:, 0] + terms[:, 1]) + terms[:, 2])
    for name in want:
        out[name] = raw[name]
    return out if isinstance(points, torch.Tensor) else {k: v.cpu().numpy() for k, v in out.items()}


# ---- a target cloud asked at external queries (csrc/cloud_distance.hip) ------------------------------------------------------------------
class BinnedCloud:
    """A target cloud on the device, binned once into a grid over its own bounds by `bin_cloud`: what `knn_cross`, `ball_cross` and
    `cylinder_stats` take as `binned=`, so that a cloud binned once serves several calls. `pts` [n, 3] float64 device tensor, `cell_size`,
    `dims`, `grid` (host, origin and cell size), `perm` and `start` (device) as `_binned` returns them; all None but `pts` for n == 0."""

    def __init__(self, pts, cell_size=None, dims=None, grid=None, perm=None, start=None):
        self.pts, self.cell_size, self.dims, self.grid, self.perm, self.start = pts, cell_size, dims, grid, perm, start

    def __len__(self):
        return self.pts.shape[0]


def bin_cloud(points, cell_size, engine=None):
    """`points` (numpy or tensor, finite: ValueError otherwise) uploaded and binned into the grid of `cell_size` (enlarged to fit the cell cap)."""
    if not (float(cell_size) > 0.0 and math.isfinite(float(cell_size))):
        raise ValueError(f"cell_size must be finite and positive (got {cell_size})")
    eng = default_engine(engine)
    pts = _device_points(points, eng.device)
    if pts.shape[0] > MAX_BALL_POINTS:
        raise ValueError("at most 2^26 points")
    if pts.shape[0] == 0:
        return BinnedCloud(pts)
    lo, hi = _bounds(pts)
    return BinnedCloud(pts, *_binned(eng, pts, lo, hi, float(cell_size)))


def _device_queries(queries, dev, what="queries"):
    q = queries.to(device=dev, dtype=torch.float64).contiguous() if isinstance(queries, torch.Tensor) else to_device(queries, dev, np.float64)
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError(f"{what} must be [m, 3] (got {tuple(q.shape)})")
    if q.shape[0] > MAX_BALL_POINTS:
        raise ValueError(f"at most 2^26 {what}")
    return q


def query_order(eng, q, target):
    """The order in which the waves take the queries: ascending key of the query's (clamped) cell in the target's grid, so that neighbouring
    waves read the same cells. A tunable: no result depends on it."""
    m = q.shape[0]
    key = torch.empty(m, dtype=torch.int64, device=q.device)
    eng.ctx.call("im_knn_cells", ptr(q), m, target.grid.ctypes.data, target.dims[0], target.dims[1], target.dims[2], ptr(key), eng.stream_ptr())
    return torch.sort(key, stable=True)[1]


def _cross(eng, queries, points, binned, default_cell_size, cell_size, sort_queries):
    """(q device [m, 3], target BinnedCloud, d_qorder or None) of a cross call."""
    if cell_size is not None and not (float(cell_size) > 0.0 and math.isfinite(float(cell_size))):
        raise ValueError(f"cell_size must be finite and positive (got {cell_size})")
    q = _device_queries(queries, eng.device)
    if binned is None:
        pts = _device_points(points, eng.device)
        if pts.shape[0] > MAX_BALL_POINTS:
            raise ValueError("at most 2^26 points")
        if pts.shape[0] == 0:
            binned = BinnedCloud(pts)
        else:
            lo, hi = _bounds(pts)
            s = default_cell_size(pts, lo, hi) if cell_size is None else float(cell_size)
            binned = BinnedCloud(pts, *_binned(eng, pts, lo, hi, s))
    order = query_order(eng, q, binned) if sort_queries and len(binned) > 0 and q.shape[0] > 1 else None
    return q, binned, order


def _target_args(t):
    return (ptr(t.pts), ptr(t.perm), ptr(t.start), len(t), t.grid.ctypes.data, t.dims[0], t.dims[1], t.dims[2])


def _result(out, queries):
    return out if isinstance(queries, torch.Tensor) else {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def knn_cross(queries, points, k, radius=None, cell_size=None, engine=None, want=("idx", "d2", "count"), binned=None, sort_queries=True):
    """The k (1..64) nearest points of the target cloud `points` for every row of `queries` [m, 3], which may lie anywhere: {name: ...} for
    the names in `want` out of idx [m, k] int32 (indices into `points`), d2 [m, k] float64, count [m] int32, rings [m] int32, with the
    order, tie rule, radius cut and unused slots of `knn_self`. A query with a non-finite coordinate has no neighbours. The target must be
    finite (ValueError). `binned` (a `bin_cloud` result) replaces `points`; `cell_size` and `sort_queries` are tunables: the result does
    not depend on them. numpy queries in, numpy out; tensor in, tensors out."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be 1..{MAX_K} (got {k})")
    if radius is not None and not float(radius) >= 0.0:
        raise ValueError(f"radius must be >= 0 (got {radius})")
    unknown = set(want) - {"idx", "d2", "count", "rings"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    eng = default_engine(engine)
    q, t, order = _cross(eng, queries, points, binned, lambda pts, lo, hi: choose_cell_size(eng, pts, lo, hi, k), cell_size, sort_queries)
    m, dev = q.shape[0], eng.device
    fill = {"idx": ((m, k), torch.int32, -1), "d2": ((m, k), torch.float64, math.inf), "count": ((m,), torch.int32, 0), "rings": ((m,), torch.int32, 0)}
    out = {name: torch.full(fill[name][0], fill[name][2], dtype=fill[name][1], device=dev) for name in want}      # what an empty target leaves
    if len(t) > 0 and m > 0:
        r2 = math.inf if radius is None else float(radius) * float(radius)
        eng.ctx.call("im_knn_cross", *_target_args(t), ptr(q), ptr(order), m, k, r2, ptr(out.get("count")), ptr(out.get("idx")),
                     ptr(out.get("d2")), ptr(out.get("rings")), eng.stream_ptr())
    return _result(out, queries)


def _check_radius(radius, what="radius"):
    radius = float(radius)
    if not (radius > 0.0 and math.isfinite(radius)) or radius * 2.0 ** -18 < 2.2250738585072014e-308:
        raise ValueError(f"{what} must be finite and positive, and {what} * 2^-18 a normal number (got {radius})")
    return radius


def ball_cross(queries, points, radius, want=("count", "normal"), cell_size=None, engine=None, binned=None, sort_queries=True):
    """The ball of `radius` in the target cloud `points` around every row of `queries`, by the definitions of `ball_features` with offsets
    relative to the query (which is no neighbour unless a target point coincides with it): {name: ...} for the names in `want` out of
    count [m] int32, sums [m, 10] int64, eig [m, 3], normal [m, 3] float64 and steps [m] int32. A ball of fewer than three points or
    without extent, and a query with a non-finite coordinate, give NaN. `binned`, `cell_size` (default radius / 2) and `sort_queries` as
    in `knn_cross`."""
    radius = _check_radius(radius)
    unknown = set(want) - {"count", "sums", "eig", "normal", "steps"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    eng = default_engine(engine)
    q, t, order = _cross(eng, queries, points, binned, lambda pts, lo, hi: radius / 2.0, cell_size, sort_queries)
    m, dev = q.shape[0], eng.device
    fill = {"count": ((m,), torch.int32, 0), "sums": ((m, 10), torch.int64, 0), "eig": ((m, 3), torch.float64, math.nan),
            "normal": ((m, 3), torch.float64, math.nan), "steps": ((m,), torch.int32, 0)}
    out = {name: torch.full(fill[name][0], fill[name][2], dtype=fill[name][1], device=dev) for name in want}
    if len(t) > 0 and m > 0:
        eng.ctx.call("im_ball_cross", *_target_args(t), ptr(q), ptr(order), m, radius, ptr(out.get("count")), ptr(out.get("sums")),
                     ptr(out.get("eig")), ptr(out.get("normal")), ptr(out.get("steps")), eng.stream_ptr())
    return _result(out, queries)


def cylinder_stats(queries, normals, points, radius, half_length, want=("count", "mean", "std"), cell_size=None, engine=None, binned=None,
                   sort_queries=True):
    """The points of the target cloud `points` inside the cylinder of `radius` and `half_length` around every row of `queries` along the
    matching row of `normals` (used as given; csrc/cyl_point.h): {name: ...} for the names in `want` out of count [m] int32,
    sums [m, 2] int64 (St, Stt of the projections quantised to half_length * 2^-18), mean [m] and std [m] float64 in metres (NaN for count 0
    and count < 2), steps [m] int32. A query or normal with a non-finite component gives count 0 and NaN. `binned`, `cell_size` (default:
    the radius) and `sort_queries` as in `knn_cross`."""
    radius = float(radius)
    if not (radius > 0.0 and math.isfinite(radius)):
        raise ValueError(f"radius must be finite and positive (got {radius})")
    half_length = _check_radius(half_length, "half_length")
    unknown = set(want) - {"count", "sums", "mean", "std", "steps"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    eng = default_engine(engine)
    q, t, order = _cross(eng, queries, points, binned, lambda pts, lo, hi: radius, cell_size, sort_queries)
    nrm = _device_queries(normals, eng.device, "normals")
    if nrm.shape[0] != q.shape[0]:
        raise ValueError(f"{q.shape[0]} queries but {nrm.shape[0]} normals")
    m, dev = q.shape[0], eng.device
    fill = {"count": ((m,), torch.int32, 0), "sums": ((m, 2), torch.int64, 0), "mean": ((m,), torch.float64, math.nan),
            "std": ((m,), torch.float64, math.nan), "steps": ((m,), torch.int32, 0)}
    out = {name: torch.full(fill[name][0], fill[name][2], dtype=fill[name][1], device=dev) for name in want}
    if len(t) > 0 and m > 0:
        eng.ctx.call("im_cyl_stats", *_target_args(t), ptr(q), ptr(nrm), ptr(order), m, radius, half_length, ptr(out.get("count")),
                     ptr(out.get("sums")), ptr(out.get("mean")), ptr(out.get("std")), ptr(out.get("steps")), eng.stream_ptr())
    return _result(out, queries)


def voxel_down_sample(points, voxel_size, colors=None, normals=None, engine=None):
    """(points [V, 3], colors [V, 3] or None, normals [V, 3] or None, counts [V] int32, first_index [V] int32): per filled voxel of the grid
    min(points) - 0.5 voxel_size .. max(points) + 0.5 voxel_size the mean of its points, of their colours and of their normals (not
    renormalised), each column summed in ascending point index; the voxels in ascending key. `counts` and `first_index` (the voxel's first
    input point) let a caller carry other per-point fields along. Points with a non-finite coordinate are ignored."""
    from ..post_processing.voxel_grid import cloud_arrays, device_pass, make_grid
    make_grid((0, 0, 0), (0, 0, 0), voxel_size)                      # a bad voxel_size raises before any device work
    cloud = cloud_arrays(points, colors, normals)
    results, _ = device_pass(default_engine(engine), [cloud], None, voxel_size, want_points=True)
    r = results[0]
    return r["points"], r["colors"], r["normals"], r["counts"], r["first"]
