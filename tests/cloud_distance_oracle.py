"""Brute-force numpy restatement of the cross-cloud kernels (csrc/cloud_distance.hip, csrc/cyl_point.h): for external queries the k
nearest points of a target cloud (the rule of tests/knn_oracle.py against another cloud), the sums of the ball around a query (the
arithmetic of tests/ball_oracle.py with offsets from the query), the points of the target inside a cylinder along a normal with the
three exact sums of their quantised projections, mean and sample standard deviation, and M3C2's finish; operation by operation in the
headers' order, so that a host build of cyl_point.h (tests/test_cloud_distance_cpu.py) and the kernels (tests/test_gpu_cloud_distance.py)
can be compared bit for bit. It also restates the walks (rings, boxes, steps) far enough to predict which queries give them up for a scan
of the whole cloud.

Definitions (the issue's). Cylinder: u = fl(p - c) per axis, t = ((ux*nx) + (uy*ny)) + (uz*nz), d2 = ((ux*ux) + (uy*uy)) +
(uz*uz), rad2 = d2 - t*t; inside iff |t| <= L and rad2 <= fl(rho*rho); it = rint(t / h) clamped to +-(2^18 + 1), h = L * 2^-18; count, St,
Stt as Python integers; m = float(St) / cnt, mean = m * h (NaN for count 0), v = max(0, float(Stt) / cnt - m*m), std = sqrt(v * (cnt /
(cnt - 1))) * h (NaN for count < 2); dist = mean2 - mean1, lod = 1.96 * (sqrt(std1*std1/cnt1 + std2*std2/cnt2) + reg), NaN when a count
is below min_points; significant = |dist| > lod. A query with a non-finite coordinate (or normal) has an empty result everywhere.

Imports nothing from the package under test and nothing from the reference."""
import numpy as np

import ball_oracle as B
import knn_oracle as K

WAVE, MIN_STEPS = 64, 1024
PAD, SLACK, UNIT = 1.0 + 2.0 ** -18, 2.0 ** -18, 2.0 ** -21


def _f(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1, 3)


def budget(n):
    return MIN_STEPS + n // (WAVE // 2)


# ---- cross k-NN ------------------------------------------------------------------------------------------------------------------------------
def d2_to(q, p):
    """[n] squared distances of one query to every target point, the kernel's order of operations."""
    d = q[None, :] - p
    return ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])


def knn_cross(queries, points, k, radius2=np.inf):
    """(idx int32 [m, k], d2 float64 [m, k], count int32 [m]); unused slots -1 / +inf."""
    q, p = _f(queries), _f(points)
    m, n = len(q), len(p)
    idx, d2o, count = np.full((m, k), -1, np.int32), np.full((m, k), np.inf), np.zeros(m, np.int32)
    index = np.arange(n)
    for i in range(m):
        if n == 0 or not np.isfinite(q[i]).all():
            continue
        with np.errstate(over="ignore"):
            d2 = d2_to(q[i], p)
        order = np.lexsort((index, d2))[:k]
        order = order[~(d2[order] > radius2)]
        count[i] = len(order)
        idx[i, :len(order)], d2o[i, :len(order)] = order, d2[order]
    return idx, d2o, count


def _strip_steps(pc, xa, xb, ya, yb, za, zb):
    """The steps knn_strip takes over the rows (ya..yb, za..zb) of cells xa..xb, and the mask of the target points it reads."""
    if ya > yb or za > zb:
        return 0, np.zeros(len(pc), bool)
    rows = (yb - ya + 1) * (zb - za + 1)
    m = (pc[:, 0] >= xa) & (pc[:, 0] <= xb) & (pc[:, 1] >= ya) & (pc[:, 1] <= yb) & (pc[:, 2] >= za) & (pc[:, 2] <= zb)
    _, per_row = np.unique(pc[m][:, 1:], axis=0, return_counts=True) if m.any() else (None, np.zeros(0, np.int64))
    return (rows + WAVE - 1) // WAVE + int(((per_row + WAVE - 1) // WAVE).sum()), m


def knn_rings(queries, points, s, k, radius2=np.inf):
    """[m] the rings every search visits on the grid of cell size s over the target (the query's cell counted), negated where the search
    spends its step budget and scans the whole cloud; 0 for a non-finite query. The ring loop of knn_list.h, step by step."""
    q, p = _f(queries), _f(points)
    o, dims = K.grid_of(p, s)
    pc = K.cells(K.cell_coords(p, o, s), dims)
    with np.errstate(over="ignore", invalid="ignore"):
        tq = K.cell_coords(q, o, s)
    cq = K.cells(tq, dims)
    out = np.zeros(len(q), np.int64)
    for i in range(len(q)):
        if not np.isfinite(q[i]).all():
            continue
        with np.errstate(over="ignore"):
            d2 = d2_to(q[i], p)
        ok = ~(d2 > radius2)
        c, t = [int(v) for v in cq[i]], tq[i]
        steps, seen = _strip_steps(pc, c[0], c[0], c[1], c[1], c[2], c[2])
        rings, r = 1, 1
        while True:
            dd = np.sort(d2[seen & ok])
            kth = dd[k - 1] if len(dd) >= k else np.inf
            if K.done(t, c, r - 1, dims, s, kth, radius2):
                break
            if steps > budget(len(p)):
                rings = -rings
                break
            x0, x1 = max(0, c[0] - r), min(dims[0] - 1, c[0] + r)
            y0, y1 = max(0, c[1] - r), min(dims[1] - 1, c[1] + r)
            yi0, yi1 = max(0, c[1] - r + 1), min(dims[1] - 1, c[1] + r - 1)
            zi0, zi1 = max(0, c[2] - r + 1), min(dims[2] - 1, c[2] + r - 1)
            strips = []
            if c[2] - r >= 0: strips.append((x0, x1, y0, y1, c[2] - r, c[2] - r))
            if c[2] + r <= dims[2] - 1: strips.append((x0, x1, y0, y1, c[2] + r, c[2] + r))
            if c[1] - r >= 0: strips.append((x0, x1, c[1] - r, c[1] - r, zi0, zi1))
            if c[1] + r <= dims[1] - 1: strips.append((x0, x1, c[1] + r, c[1] + r, zi0, zi1))
            if c[0] - r >= 0: strips.append((c[0] - r, c[0] - r, yi0, yi1, zi0, zi1))
            if c[0] + r <= dims[0] - 1: strips.append((c[0] + r, c[0] + r, yi0, yi1, zi0, zi1))
            for st in strips:
                n_steps, m = _strip_steps(pc, *st)
                steps += n_steps
                seen |= m
            rings = r + 1
            r += 1
        out[i] = rings
    return out


# ---- cross ball ------------------------------------------------------------------------------------------------------------------------------
def ball_cross(queries, points, r):
    """{"sums" [m, 10] int64, "count", "eig", "normal"}: ball_oracle's arithmetic around external queries."""
    q, p = _f(queries), _f(points)
    m = len(q)
    S = np.zeros((m, 10), np.int64)
    r2, h = np.float64(r) * np.float64(r), B.step(r)
    for i in range(m):
        if len(p) == 0 or not np.isfinite(q[i]).all():
            continue
        inside = ~(d2_to(q[i], p) > r2)
        off = B.quantise(p - q[i], h)[inside]
        x, y, z = off[:, 0], off[:, 1], off[:, 2]
        S[i, 0] = inside.sum()
        for j, v in enumerate((x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
            S[i, 1 + j] = v.sum()
    eig, e3 = B.finish(S, r)
    return {"sums": S, "count": S[:, 0].astype(np.int32), "eig": eig, "normal": e3}


def _box_falls_back(lo, hi, n):
    rows = (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1)
    return (rows + WAVE - 1) // WAVE > budget(n)


def ball_walk(queries, points, s, r):
    """[m] bool: the queries whose box of cells costs more row lookups than the step budget (steps < 0); non-finite queries take no step."""
    q, p = _f(queries), _f(points)
    o, dims = K.grid_of(p, s)
    with np.errstate(over="ignore", invalid="ignore"):
        t = K.cell_coords(q, o, s)
    c = K.cells(t, dims)
    out = np.zeros(len(q), bool)
    for i in range(len(q)):
        if not np.isfinite(q[i]).all():
            continue
        R = B.rings_needed(t[i], c[i], dims, s, r)
        out[i] = _box_falls_back(np.maximum(0, c[i] - R), np.minimum(dims - 1, c[i] + R), len(p))
    return out


# ---- cylinders -------------------------------------------------------------------------------------------------------------------------------
def cyl_step(L):
    return np.float64(L) * np.float64(2.0 ** -B.QBITS)


def cyl_inside(points, c, nrm, rho, L):
    """(mask [n], t [n]) of every target point against one cylinder."""
    p = _f(points)
    with np.errstate(all="ignore"):
        u = p - np.asarray(c, np.float64)[None, :]
        t = ((u[:, 0] * nrm[0]) + (u[:, 1] * nrm[1])) + (u[:, 2] * nrm[2])
        d2 = ((u[:, 0] * u[:, 0]) + (u[:, 1] * u[:, 1])) + (u[:, 2] * u[:, 2])
        rad2 = d2 - t * t
        return (np.abs(t) <= np.float64(L)) & (rad2 <= np.float64(rho) * np.float64(rho)), t


def cyl_sums(points, c, nrm, rho, L):
    """(count, St, Stt) of one cylinder as Python integers."""
    if not (np.isfinite(c).all() and np.isfinite(nrm).all()):
        return 0, 0, 0
    m, t = cyl_inside(points, c, nrm, rho, L)
    it = [int(v) for v in B.quantise(t[m], cyl_step(L))]
    return len(it), sum(it), sum(v * v for v in it)


def cyl_finish(count, St, Stt, L):
    """(mean, std) float64 of one cylinder from its sums."""
    h = cyl_step(L)
    with np.errstate(all="ignore"):
        cnt = np.float64(count)
        m = np.float64(St) / cnt                             # int -> float64: correctly rounded (the sums stay below 2^63)
        mean = m * h if count >= 1 else np.float64(np.nan)
        v = np.float64(Stt) / cnt - m * m
        v = np.float64(0.0) if v < 0.0 else v
        std = np.sqrt(v * (cnt / (cnt - np.float64(1.0)))) * h if count >= 2 else np.float64(np.nan)
    return np.float64(mean), np.float64(std)


def cylinder_stats(queries, normals, points, rho, L):
    """{"count" int32 [m], "sums" int64 [m, 2], "mean", "std" float64 [m]}."""
    q, nr, p = _f(queries), _f(normals), _f(points)
    m = len(q)
    out = {"count": np.zeros(m, np.int32), "sums": np.zeros((m, 2), np.int64), "mean": np.full(m, np.nan), "std": np.full(m, np.nan)}
    for i in range(m):
        cnt, St, Stt = cyl_sums(p, q[i], nr[i], rho, L) if len(p) else (0, 0, 0)
        out["count"][i], out["sums"][i] = cnt, (St, Stt)
        out["mean"][i], out["std"][i] = cyl_finish(cnt, St, Stt, L)
    return out


def m3c2_finish(count1, sums1, count2, sums2, L, reg_error, min_points):
    """(dist float64 [m], lod float64 [m], sig uint8 [m])."""
    m = len(count1)
    dist, lod, sig = np.zeros(m), np.zeros(m), np.zeros(m, np.uint8)
    for i in range(m):
        c1, c2 = int(count1[i]), int(count2[i])
        mean1, std1 = cyl_finish(c1, int(sums1[i][0]), int(sums1[i][1]), L)
        mean2, std2 = cyl_finish(c2, int(sums2[i][0]), int(sums2[i][1]), L)
        with np.errstate(all="ignore"):
            dist[i] = mean2 - mean1
            var = (std1 * std1) / np.float64(c1) + (std2 * std2) / np.float64(c2)
            lod[i] = np.nan if (c1 < min_points or c2 < min_points) else np.float64(1.96) * (np.sqrt(var) + np.float64(reg_error))
            sig[i] = 1 if np.abs(dist[i]) > lod[i] else 0
    return dist, lod, sig


def cyl_extent(nrm, rho, L):
    """[3] the half-extents of the box of one cylinder: cyl_point.h's cyl_extent, operation by operation."""
    rho, L = np.float64(rho), np.float64(L)
    n = np.asarray(nrm, np.float64)
    with np.errstate(all="ignore"):
        s = ((n[0] * n[0]) + (n[1] * n[1])) + (n[2] * n[2])
        ball = (rho if s == 0.0 else np.sqrt(L * L + rho * rho)) * np.float64(PAD)
        unit = np.abs(s - 1.0) <= UNIT
        wall = np.sqrt(rho * rho + np.float64(SLACK) * (L * L))
        e = np.zeros(3)
        for a in range(3):
            c2 = 1.0 - n[a] * n[a]
            f = (L * np.abs(n[a]) + wall * np.sqrt((c2 if c2 > 0.0 else 0.0) + np.float64(SLACK))) * np.float64(PAD)
            e[a] = f if (unit and f < ball) else ball
    return e


def cyl_box(q, nrm, rho, L, o, dims, s):
    """(lo [3], hi [3]) the box of cells the kernel walks for one finite query."""
    e = cyl_extent(nrm, rho, L)
    with np.errstate(all="ignore"):
        lo = K.cells(K.cell_coords((q - e)[None, :], o, s), dims)[0]
        hi = K.cells(K.cell_coords((q + e)[None, :], o, s), dims)[0]
    return lo, np.maximum(lo, hi)


def cyl_walk(queries, normals, points, s, rho, L):
    """[m] bool: the queries whose box costs more row lookups than the step budget; also asserts the box holds every inside point."""
    q, nr, p = _f(queries), _f(normals), _f(points)
    o, dims = K.grid_of(p, s)
    pc = K.cells(K.cell_coords(p, o, s), dims)
    out = np.zeros(len(q), bool)
    for i in range(len(q)):
        if not (np.isfinite(q[i]).all() and np.isfinite(nr[i]).all()):
            continue
        lo, hi = cyl_box(q[i], nr[i], rho, L, o, dims, s)
        inside, _ = cyl_inside(p, q[i], nr[i], rho, L)
        assert ((pc[inside] >= lo) & (pc[inside] <= hi)).all(), ("an inside point outside the box", i)
        out[i] = _box_falls_back(lo, hi, len(p))
    return out
