"""Brute-force numpy restatement of the ball features (csrc/ballfeat.hip, csrc/ball_point.h): for every point the ten exact integer sums
of the quantised offsets of its ball, the covariance, the eigenvalues by cyclic Jacobi, the normal and CloudCompare's published list of
features, operation by operation in the header's order, so that a host build of the header (tests/test_ballfeat_cpu.py) and the kernel
(tests/test_gpu_ballfeat.py) can be compared bit for bit.

The definition (the issue's): the neighbours of q are the points p, q among them, with d2 = ((dx*dx) + (dy*dy)) + (dz*dz) <=
fl(r * r), d = q - p in float64; u = fl(p - q) per axis; i = rint(u / h), h = r * 2^-18, clamped to +-(2^18 + 1); count, Sx Sy Sz, Sxx Sxy
Sxz Syy Syz Szz as integers (int64 here: a product is at most (2^18 + 1)^2 and a cloud at most 2^26 points, so nothing overflows;
`python_int_sums` does one ball with Python integers as a cross-check); cnt = float(count), m_a = float(S_a) / cnt, c_ab = float(S_ab) / cnt
- m_a * m_b; Jacobi as knn_point.h's knn_rotate; the smallest diagonal entry by the `<=` chain, of the other two the larger first (the
lower index on a tie); eigenvalues not above 0 become 0.0, then * (h * h); count < 3 or l1 == 0: NaN everywhere.

Imports nothing from the package under test and nothing from the reference."""
import os

import numpy as np

import knn_oracle as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_top_border.npz")
QBITS = 18
QMAX = 2 ** QBITS + 1
EPS = 2.220446049250313e-16
MAX_SWEEPS = 30
MIN_STEPS, WAVE = 1024, 64
BLOCK = 256                # queries per block of the brute force
KINDS = ("EigenValuesSum", "PCA1", "PCA2", "SurfaceVariation", "Linearity", "Planarity", "Anisotropy", "Sphericity", "Verticality",
         "EigenValue1", "EigenValue2", "EigenValue3", "NumberOfNeighbors")          # the codes of include/icematch.h, in order


def step(r):
    return np.float64(r) * np.float64(2.0 ** -QBITS)


def quantise(u, h):
    with np.errstate(over="ignore"):
        return np.clip(np.rint(np.asarray(u, np.float64) / np.float64(h)), -float(QMAX), float(QMAX)).astype(np.int64)


def inside(points, q, r):
    """The mask of the ball of point q."""
    r2 = np.float64(r) * np.float64(r)
    d = points[q] - points
    d2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
    return ~(d2 > r2)


def offsets(points, q, r):
    """(mask [n], quantised offsets [n, 3] int64) of every point against query q."""
    return inside(points, q, r), quantise(points - points[q], step(r))


def python_int_sums(points, q, r):
    """The ten sums of one ball with Python integers."""
    m, i = offsets(points, q, r)
    rows = [tuple(int(v) for v in row) for row in i[m]]
    s = [len(rows)] + [0] * 9
    for x, y, z in rows:
        for k, v in enumerate((x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
            s[1 + k] += v
    return s


def sums(points, r):
    """[n, 10] int64: count, Sx Sy Sz, Sxx Sxy Sxz Syy Syz Szz of every point's ball."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n = len(p)
    out = np.zeros((n, 10), np.int64)
    r2, h = np.float64(r) * np.float64(r), step(r)
    for b in range(0, n, BLOCK):
        q = p[b:b + BLOCK]
        d = q[:, None, :] - p[None, :, :]
        d2 = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
        m = ~(d2 > r2)
        i = quantise(p[None, :, :] - q[:, None, :], h) * m[..., None]
        x, y, z = i[..., 0], i[..., 1], i[..., 2]
        out[b:b + BLOCK, 0] = m.sum(1)
        for k, v in enumerate((x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
            out[b:b + BLOCK, 1 + k] = v.sum(1)
    return out


def covariance(S):
    """[n, 6] (xx xy xz yy yz zz) in quantised units from the sums."""
    S = np.asarray(S, np.int64).reshape(-1, 10)
    with np.errstate(invalid="ignore", divide="ignore"):
        cnt = S[:, 0].astype(np.float64)
        D = S.astype(np.float64)                            # int64 -> float64: correctly rounded
        m = [D[:, 1] / cnt, D[:, 2] / cnt, D[:, 3] / cnt]
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        return np.stack([D[:, 4 + k] / cnt - m[a] * m[b] for k, (a, b) in enumerate(pairs)], 1)


def _rotate(a, v, P, Q, R):
    apq, app, aqq = a[:, P, Q].copy(), a[:, P, P].copy(), a[:, Q, Q].copy()
    small = np.where(np.abs(app) < np.abs(aqq), np.abs(app), np.abs(aqq))
    with np.errstate(all="ignore"):
        act = np.abs(apq) > (0.125 * EPS) * small
        theta = (aqq - app) / (2.0 * apq)
        tt = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(1.0 + theta * theta))
        cs = 1.0 / np.sqrt(1.0 + tt * tt)
        sn = cs * tt
        new_pp, new_qq = app - tt * apq, aqq + tt * apq
        arp, arq = a[:, R, P].copy(), a[:, R, Q].copy()
        new_rp, new_rq = cs * arp - sn * arq, sn * arp + cs * arq
        a[:, P, P] = np.where(act, new_pp, app)
        a[:, Q, Q] = np.where(act, new_qq, aqq)
        a[:, P, Q] = a[:, Q, P] = np.where(act, 0.0, apq)
        a[:, R, P] = a[:, P, R] = np.where(act, new_rp, arp)
        a[:, R, Q] = a[:, Q, R] = np.where(act, new_rq, arq)
        for k in range(3):
            x, y = v[:, k, P].copy(), v[:, k, Q].copy()
            v[:, k, P] = np.where(act, cs * x - sn * y, x)
            v[:, k, Q] = np.where(act, sn * x + cs * y, y)
    return act


def jacobi(cov):
    """(a [n, 3, 3], v [n, 3, 3]) after the cyclic sweeps. A ball that did not rotate in one sweep does not rotate in a later one (its
    state is unchanged), so sweeping all balls until none rotates equals the header's break per ball."""
    cov = np.asarray(cov, np.float64).reshape(-1, 6)
    a = np.empty((len(cov), 3, 3))
    for (i, j), k in {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}.items():
        a[:, i, j] = a[:, j, i] = cov[:, k]
    v = np.tile(np.eye(3), (len(cov), 1, 1))
    for _ in range(MAX_SWEEPS):
        r01 = _rotate(a, v, 0, 1, 2)
        r02 = _rotate(a, v, 0, 2, 1)
        r12 = _rotate(a, v, 1, 2, 0)
        if not (r01 | r02 | r12).any():
            break
    return a, v


def unit_signed(x, y, z):
    with np.errstate(all="ignore"):
        ln = np.sqrt(((x * x) + (y * y)) + (z * z))
        ok = ln > 0.0
        x, y, z = x / ln, y / ln, z / ln
        flip = np.where(z != 0.0, z < 0.0, np.where(y != 0.0, y < 0.0, x < 0.0))
        out = np.stack([np.where(flip, -x, x), np.where(flip, -y, y), np.where(flip, -z, z)], 1)
    out[~ok] = (0.0, 0.0, 1.0)
    return out


def finish(S, r):
    """(eig [n, 3] descending in m^2, e3 [n, 3]) from the sums; NaN for a degenerate ball."""
    S = np.asarray(S, np.int64).reshape(-1, 10)
    h = step(r)
    hh = h * h
    a, v = jacobi(covariance(S))
    d = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], 1)
    with np.errstate(invalid="ignore"):
        k = np.where((d[:, 0] <= d[:, 1]) & (d[:, 0] <= d[:, 2]), 0, np.where(d[:, 1] <= d[:, 2], 1, 2))
        ia = np.where(k == 0, 1, 0)
        ib = np.where(k == 2, 1, 2)
        rows = np.arange(len(S))
        la, lb, l3 = d[rows, ia], d[rows, ib], d[rows, k]
        first = la >= lb
        l1, l2 = np.where(first, la, lb), np.where(first, lb, la)
        eig = np.stack([np.where(l > 0.0, l, 0.0) * hh for l in (l1, l2, l3)], 1)
        e3 = unit_signed(v[rows, 0, k], v[rows, 1, k], v[rows, 2, k])
        bad = (S[:, 0] < 3) | ~(eig[:, 0] > 0.0)
    eig[bad] = np.nan
    e3[bad] = np.nan
    return eig, e3


def features(eig, e3, count):
    """{name: [n]} of the thirteen arithmetic features, NaN for a degenerate ball."""
    l1, l2, l3 = eig[:, 0], eig[:, 1], eig[:, 2]
    with np.errstate(all="ignore"):
        total = (l1 + l2) + l3
        out = {"EigenValuesSum": total, "PCA1": l1 / total, "PCA2": l2 / total, "SurfaceVariation": l3 / total,
               "Linearity": (l1 - l2) / l1, "Planarity": (l2 - l3) / l1, "Anisotropy": (l1 - l3) / l1, "Sphericity": l3 / l1,
               "Verticality": 1.0 - np.abs(e3[:, 2]), "EigenValue1": l1, "EigenValue2": l2, "EigenValue3": l3,
               "NumberOfNeighbors": np.asarray(count).astype(np.float64)}
    bad = (np.asarray(count) < 3) | ~(l1 > 0.0)
    return {k: np.where(bad, np.nan, v) for k, v in out.items()}


def ball_features(points, r):
    """Everything of every point: {"sums", "count", "cov", "eig", "normal", and the thirteen features}."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    S = sums(p, r)
    eig, e3 = finish(S, r)
    out = {"sums": S, "count": S[:, 0].astype(np.int32), "cov": covariance(S), "eig": eig, "normal": e3}
    out.update(features(eig, e3, S[:, 0]))
    return out


def omnivariance(eig):
    return np.cbrt(eig[:, 0] * eig[:, 1] * eig[:, 2])


def eigen_entropy(eig):
    """(-sum l ln l with a zero term counting 0, sum |l ln l|)."""
    with np.errstate(all="ignore"):
        terms = np.where(eig == 0.0, 0.0, eig * np.log(eig))
    return -((terms[:, 0] + terms[:, 1]) + terms[:, 2]), np.abs(terms).sum(1)


# ---- the box of cells a query walks ----------------------------------------------------------------------------------------------------
def rings_needed(t, c, dims, s, r):
    """The smallest R at which the k-NN's stop rule holds with no k-th distance, by trying R = 0, 1, 2, ..."""
    r2 = float(np.float64(r) * np.float64(r))
    R = 0
    while not K.done(t, c, R, dims, s, np.inf, r2):
        R += 1
    return R


def walk(points, s, r):
    """(R [n], falls_back [n] bool) of every query on the grid of cell size s: the half-width of its box, and whether the row lookups of
    the clipped box, 64 at a time, exceed the step budget 1024 + n // 32."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    o, dims = K.grid_of(p, s)
    t = K.cell_coords(p, o, s)
    c = K.cells(t, dims)
    budget = MIN_STEPS + len(p) // (WAVE // 2)
    R = np.array([rings_needed(t[i], c[i], dims, s, r) for i in range(len(p))], np.int64)
    lo = np.maximum(0, c - R[:, None])
    hi = np.minimum(dims[None, :] - 1, c + R[:, None])
    w = hi - lo + 1
    rows = w[:, 1] * w[:, 2]
    return R, (rows + WAVE - 1) // WAVE > budget


# ---- the filters of the top-border script ------------------------------------------------------------------------------------------------
def filter_by_value(values, lo, hi):
    v = np.asarray(values, np.float64)
    with np.errstate(invalid="ignore"):
        return np.nonzero((v >= lo) & (v <= hi))[0]


def percentile_window(values, lim):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanpercentile(values, lim[0]), np.nanpercentile(values, lim[1])
