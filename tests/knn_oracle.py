"""Brute-force numpy restatement of the point-cloud neighbourhood kernels (csrc/knn.hip, csrc/knn_point.h) and of what is built on them:
the k nearest neighbours of every point within its own cloud, the radius cut of the hybrid search, the mean neighbour distance,
statistical outlier removal as Open3D publishes it, two-pass covariances and normals (numpy.linalg.eigh). It also restates, operation
by operation, the grid arithmetic of knn_point.h (cell coordinate, cell, key, the bound that ends the ring search), so that a host build
of that header can be compared bit for bit (tests/test_pointcloud_cpu.py).

Definitions (the issue's): d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float64; neighbours ascend by d2 with the lower index first among
equal distances (np.lexsort((index, d2))); the point itself is a neighbour at distance 0; a neighbour is dropped iff d2 > radius2;
mean = the left-to-right sum of sqrt(d2_j) from 0.0 divided by float(count), -1.0 for an empty neighbourhood.

Imports nothing from the package under test and nothing from the reference."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_pointcloud.npz")
MARGIN = 2.0 ** -40
BLOCK = 512               # queries per block of the brute force


def neighbours(points, kmax):
    """The min(kmax, n) nearest of every point without a radius: (idx int64 [n, m], d2 float64 [n, m]), rows ascending by (d2, index)."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n = len(p)
    m = min(kmax, n)
    idx = np.zeros((n, m), np.int64)
    d2o = np.zeros((n, m), np.float64)
    index = np.arange(n)
    for b in range(0, n, BLOCK):
        q = p[b:b + BLOCK]
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
        for i in range(len(q)):
            order = np.lexsort((index, d2[i]))[:m]
            idx[b + i], d2o[b + i] = order, d2[i][order]
    return idx, d2o


def cut(full, k, radius2=np.inf):
    """The outputs of a search for k <= kmax neighbours under radius2 from `neighbours(points, kmax)` (a prefix of every row):
    (idx int32 [n, k], d2 float64 [n, k], count int32 [n], mean float64 [n]); unused slots are -1 / +inf."""
    fidx, fd2 = full
    n, m = fidx.shape[0], min(k, fidx.shape[1])
    idx = np.full((n, k), -1, np.int32)
    d2o = np.full((n, k), np.inf, np.float64)
    mean = np.full(n, -1.0, np.float64)
    keep = ~(fd2[:, :m] > radius2)                      # rows ascend: the kept ones are a prefix
    count = keep.sum(1).astype(np.int32)
    idx[:, :m][keep] = fidx[:, :m][keep]
    d2o[:, :m][keep] = fd2[:, :m][keep]
    if m:
        sums = np.cumsum(np.sqrt(fd2[:, :m]), axis=1)   # cumsum adds left to right from the first term (0.0 + x == x)
        has = count > 0
        mean[has] = sums[has, count[has] - 1] / count[has].astype(np.float64)
    return idx, d2o, count, mean


def knn_self(points, k, radius2=np.inf):
    """(idx, d2, count, mean) of the search for k neighbours under radius2."""
    return cut(neighbours(points, k), k, radius2)


def sor(mean, count, std_ratio):
    """Open3D's published remove_statistical_outlier on the per-point statistic: (ind ascending int64, threshold)."""
    avg = np.asarray(mean, np.float64)
    valid = int((np.asarray(count) > 0).sum())
    if len(avg) == 0 or valid == 0:
        return np.zeros(0, np.int64), np.nan
    pos = avg > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        cloud_mean = (np.cumsum(avg[pos])[-1] if pos.any() else 0.0) / np.float64(valid)
        dev = avg[pos] - cloud_mean
        sq_sum = np.cumsum(dev * dev)[-1] if pos.any() else np.float64(0.0)
        std_dev = np.sqrt(sq_sum / np.float64(valid - 1))
        threshold = cloud_mean + np.float64(std_ratio) * std_dev
        keep = pos & (avg < threshold)
    return np.nonzero(keep)[0].astype(np.int64), float(threshold)


def remove_statistical_outlier(points, nb_neighbors, std_ratio):
    """(kept points, ind) of the whole filter."""
    if nb_neighbors < 1 or not std_ratio > 0:
        raise ValueError("nb_neighbors must be >= 1 and std_ratio > 0")
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    if len(p) == 0:
        return p.copy(), np.zeros(0, np.int64)
    _, _, count, mean = knn_self(p, nb_neighbors)
    ind, _ = sor(mean, count, std_ratio)
    return p[ind], ind


def covariance(nb):
    """Two-pass mean [3] and covariance (xx xy xz yy yz zz) of the rows of nb [count, 3], sums left to right from 0.0."""
    cnt = np.float64(len(nb))
    mean = np.array([np.cumsum(nb[:, a])[-1] for a in range(3)]) / cnt
    d = nb - mean
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    return mean, np.array([np.cumsum(d[:, a] * d[:, b])[-1] for a, b in pairs]) / cnt


def normals(points, idx, count):
    """(normals [n, 3], gap [n]): the eigh eigenvector of the smallest eigenvalue of every neighbourhood's covariance, signed so that the
    first non-zero of (n_z, n_y, n_x) is positive; (0, 0, 1) for count < 3. gap = (l1 - l0) / l2 (inf where undefined or count < 3)."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    out = np.zeros((len(p), 3))
    gap = np.full(len(p), np.inf)
    for i in range(len(p)):
        c = int(count[i])
        if c < 3:
            out[i] = (0.0, 0.0, 1.0)
            continue
        _, cv = covariance(p[idx[i, :c]])
        M = np.array([[cv[0], cv[1], cv[2]], [cv[1], cv[3], cv[4]], [cv[2], cv[4], cv[5]]])
        w, v = np.linalg.eigh(M)
        nrm = v[:, 0]
        gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
        out[i] = sign_fixed(nrm)
    return out, gap


def sign_fixed(nrm):
    x, y, z = nrm
    flip = z < 0 if z != 0 else (y < 0 if y != 0 else x < 0)
    return -np.asarray(nrm) if flip else np.asarray(nrm)


# ---- the grid arithmetic of knn_point.h, one operation at a time ------------------------------------------------------------------------
def grid_of(points, s):
    """(origin [3], dims [3]) of the uniform grid of cell size s over the cloud."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    o = p.min(0)
    dims = np.floor((p.max(0) - o) / np.float64(s)).astype(np.int64) + 1
    return o, dims


def cell_coords(points, o, s):
    return (np.ascontiguousarray(points, np.float64).reshape(-1, 3) - o) / np.float64(s)


def cells(t, dims):
    f = np.floor(t)
    c = np.where(f > 0, np.minimum(f, np.asarray(dims, np.float64) - 1), 0.0)
    return c.astype(np.int64)


def keys(c, dims):
    return (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]


def face_bound2(gap, n_axis, s):
    g = (np.float64(gap) - np.float64(MARGIN) * np.float64(n_axis)) * (1.0 - np.float64(MARGIN))
    if not g > 0.0:
        return 0.0
    d = g * np.float64(s)
    return float(d * d)


def ring_bound2(t, c, r, dims, s):
    best = np.inf
    for a in range(3):
        if c[a] - r > 0:
            best = min(best, face_bound2(np.float64(t[a]) - np.float64(c[a] - r), dims[a], s))
        if c[a] + r < dims[a] - 1:
            best = min(best, face_bound2(np.float64(c[a] + r + 1) - np.float64(t[a]), dims[a], s))
    return best


def covers(c, r, dims):
    return all(c[a] - r <= 0 and c[a] + r >= dims[a] - 1 for a in range(3))


def done(t, c, r, dims, s, kth_d2, radius2):
    if covers(c, r, dims):
        return True
    b2 = ring_bound2(t, c, r, dims, s)
    return bool(kth_d2 < b2 or b2 > radius2)


def rings_needed(points, i, k, s, radius2=np.inf):
    """How many rings (the query's cell counts as one) the search of point i visits: from the brute-force k-th distance within each box."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    o, dims = grid_of(p, s)
    t = cell_coords(p, o, s)
    c = cells(t, dims)
    d = p[i] - p
    d2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
    r = 0
    while True:
        inside = (np.abs(c - c[i]) <= r).all(1) & ~(d2 > radius2)
        dd = np.sort(d2[inside])
        kth = dd[k - 1] if len(dd) >= k else np.inf
        if done(t[i], c[i], r, dims, s, kth, radius2):
            return r + 1
        r += 1
