"""The definition of the Poisson surface reconstruction of csrc/poisson.hip, in plain numpy: float64, one IEEE operation per
numpy operation, in the order the kernels follow (csrc/poisson_node.h, contraction off). It is a reconstruction on the dense grid of the
finest octree level - the same bounding cube and finest cell size as Open3D's `create_from_point_cloud_poisson` - and not Open3D's
adaptive solver: parity with an Open3D binary is unpinned.

Arrays of node values are [z, y, x] (x fastest), M = 2^depth + 1 nodes per axis. The splat sums integers: every addend is
rint(value * 2^32) as int64. A trilinear weight lies in [0, 1] (the fraction is clamped) and a unit normal's component in [-1, 1], so an
addend is at most 2^32 in size and the 2^26 samples one call accepts stay below 2^58: no sum overflows, and none depends on an order."""
import itertools

import numpy as np

MIN_DEPTH, MAX_DEPTH = 2, 9
MAX_POINTS = 1 << 26
QUANTUM = 4294967296.0
CHUNK = 1024
OMEGA = 6.0 / 7.0
CYCLES = 8


# ---- (a) the grid ---------------------------------------------------------------------------------------------------------------------------
def check_inputs(points, normals, scale=1.1):
    points = np.asarray(points, np.float64)
    normals = np.asarray(normals, np.float64)
    if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape:
        raise ValueError("points and normals must both be [n, 3]")
    if len(points) == 0:
        raise ValueError("no points")
    if len(points) > MAX_POINTS:
        raise ValueError("more than 2^26 points")
    if not (np.isfinite(points).all() and np.isfinite(normals).all()):
        raise ValueError("non-finite points or normals")
    if ((normals * normals).sum(1) == 0).any():
        raise ValueError("a zero-length normal")
    if not scale >= 1:
        raise ValueError("scale must be >= 1")
    return points, normals


def check_depth(depth):
    if int(depth) != depth or not MIN_DEPTH <= depth <= MAX_DEPTH:
        raise ValueError(f"depth must lie in [{MIN_DEPTH}, {MAX_DEPTH}]")
    return int(depth)


def grid_of(points, depth=8, width=0, scale=1.1):
    """(origin [3], h, depth) of the cube: centre of the bounding box, side scale * largest extent, 2^depth cells per axis."""
    mn, mx = points.min(0), points.max(0)
    extent = float((mx - mn).max())
    if not extent > 0:
        raise ValueError("a degenerate cloud: its largest extent is 0")
    centre = (mn + mx) * 0.5
    L = scale * extent
    if width > 0:
        depth = int(np.ceil(np.log2(L / width)))
    depth = check_depth(depth)
    h = L / float(2 ** depth)
    return centre - L * 0.5, h, depth


# ---- (b) the splat --------------------------------------------------------------------------------------------------------------------------
def cells(points, origin, h, depth):
    R = 2 ** depth
    u = (points - origin) / h
    f = np.clip(np.floor(u), 0.0, float(R - 1))
    t = np.clip(u - f, 0.0, 1.0)
    return f.astype(np.int64), t


def unit_normals(normals):
    n = normals
    return n / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]


def corner_weight(t, corner):
    wx = t[:, 0] if corner & 1 else 1.0 - t[:, 0]
    wy = t[:, 1] if corner & 2 else 1.0 - t[:, 1]
    wz = t[:, 2] if corner & 4 else 1.0 - t[:, 2]
    return (wx * wy) * wz


def quantise(v):
    return np.rint(v * QUANTUM).astype(np.int64)


def splat_sums(points, normals, origin, h, depth):
    """The int64 sums [4, M^3]: W, then V_x, V_y, V_z."""
    M = 2 ** depth + 1
    c, t = cells(points, origin, h, depth)
    unit = unit_normals(normals)
    acc = np.zeros((4, M * M * M), np.int64)
    for corner in range(8):
        w = corner_weight(t, corner)
        node = ((c[:, 2] + ((corner >> 2) & 1)) * M + (c[:, 1] + ((corner >> 1) & 1))) * M + (c[:, 0] + (corner & 1))
        np.add.at(acc[0], node, quantise(w))
        for a in range(3):
            np.add.at(acc[1 + a], node, quantise(w * unit[:, a]))
    return acc


def splat(points, normals, origin, h, depth):
    """W [M, M, M] and V [3, M, M, M]."""
    M = 2 ** depth + 1
    f = splat_sums(points, normals, origin, h, depth).astype(np.float64) * 2.0 ** -32
    f = f.reshape(4, M, M, M)
    return f[0], f[1:]


# ---- (c) the right-hand side ----------------------------------------------------------------------------------------------------------------
C = slice(1, -1)
LO = slice(0, -2)
HI = slice(2, None)


def divergence(V, h):
    two_h = 2.0 * h
    rhs = np.zeros(V.shape[1:])
    rhs[C, C, C] = (((V[0][C, C, HI] - V[0][C, C, LO]) + (V[1][C, HI, C] - V[1][C, LO, C])) + (V[2][HI, C, C] - V[2][LO, C, C])) / two_h
    return rhs


# ---- (d) the solve --------------------------------------------------------------------------------------------------------------------------
def sum6(u):
    return ((((u[C, C, LO] + u[C, C, HI]) + u[C, LO, C]) + u[C, HI, C]) + u[LO, C, C]) + u[HI, C, C]


def jacobi(u, f, h2):
    out = u.copy()
    j = (sum6(u) - h2 * f[C, C, C]) / 6.0
    out[C, C, C] = u[C, C, C] + OMEGA * (j - u[C, C, C])
    return out


def residual(u, f, h2):
    r = np.zeros_like(u)
    r[C, C, C] = f[C, C, C] - (sum6(u) - 6.0 * u[C, C, C]) / h2
    return r


def restrict(r):
    Mc = (r.shape[0] - 1) // 2 + 1
    a, b, c = slice(1, -2, 2), slice(2, -1, 2), slice(3, None, 2)
    x = (0.25 * r[:, :, a] + 0.5 * r[:, :, b]) + 0.25 * r[:, :, c]
    y = (0.25 * x[:, a] + 0.5 * x[:, b]) + 0.25 * x[:, c]
    z = (0.25 * y[a] + 0.5 * y[b]) + 0.25 * y[c]
    out = np.zeros((Mc, Mc, Mc))
    out[C, C, C] = z
    return out


def prolong(e):
    Mc = e.shape[0]
    M = 2 * (Mc - 1) + 1
    x = np.zeros((Mc, Mc, M))
    x[:, :, 0::2] = e
    x[:, :, 1::2] = 0.5 * (e[:, :, :-1] + e[:, :, 1:])
    y = np.zeros((Mc, M, M))
    y[:, 0::2] = x
    y[:, 1::2] = 0.5 * (x[:, :-1] + x[:, 1:])
    z = np.zeros((M, M, M))
    z[0::2] = y
    z[1::2] = 0.5 * (y[:-1] + y[1:])
    return z


def vcycle(u, f, hl):
    h2 = hl * hl
    if u.shape[0] == 3:
        out = np.zeros_like(u)
        out[1, 1, 1] = (h2 * f[1, 1, 1]) / -6.0
        return out
    for _ in range(2):
        u = jacobi(u, f, h2)
    fc = restrict(residual(u, f, h2))
    e = prolong(vcycle(np.zeros_like(fc), fc, hl * 2.0))
    u = u.copy()
    u[C, C, C] = u[C, C, C] + e[C, C, C]
    for _ in range(2):
        u = jacobi(u, f, h2)
    return u


def solve(rhs, h, cycles=CYCLES):
    """chi after every cycle."""
    u = np.zeros_like(rhs)
    out = []
    for _ in range(cycles):
        u = vcycle(u, rhs, h)
        out.append(u)
    return out


def residual_norm(u, f, h):
    return float(np.abs(residual(u, f, h * h)).max())


# ---- (e) the iso-value ----------------------------------------------------------------------------------------------------------------------
def chunk_sums(x):
    """One partial sum per chunk of 1024 items, zero-padded: lane t of 256 adds items t, t + 256, t + 512, t + 768 in that order, then the
    lanes halve (lane t += lane t + s, s = 128 .. 1)."""
    n = len(x)
    chunks = (n + CHUNK - 1) // CHUNK
    a = np.zeros(chunks * CHUNK)
    a[:n] = x
    a = a.reshape(chunks, 4, 256)
    s = ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]
    st = 128
    while st >= 1:
        s = s[:, :st] + s[:, st:2 * st]
        st //= 2
    return s[:, 0]


def ordered_sum(x):
    x = chunk_sums(np.ravel(x))
    while len(x) > 1:
        x = chunk_sums(x)
    return float(x[0])


def iso_value(W, chi):
    return ordered_sum(np.ravel(W) * np.ravel(chi)) / ordered_sum(W)


# ---- (f) the surface ------------------------------------------------------------------------------------------------------------------------
PERMS = sorted(itertools.permutations(range(3)))


def tet_corners(t):
    a = PERMS[t]
    return [0, 1 << a[0], (1 << a[0]) | (1 << a[1]), 7]


def corner_xyz(m):
    return np.array([(m >> x) & 1 for x in range(3)], np.float64)


def tet_case(corners, code):
    """The triangles of one tetrahedron whose corner p is inside iff bit p of `code`: each a list of three edges (lo, hi) of positions 0..3,
    wound by geometry so that the normal points from the inside corners to the outside ones."""
    P = [corner_xyz(m) for m in corners]
    ins = [p for p in range(4) if (code >> p) & 1]
    out = [p for p in range(4) if not (code >> p) & 1]
    if len(ins) in (0, 4):
        return []
    grad = np.mean([P[p] for p in out], 0) - np.mean([P[p] for p in ins], 0)
    if len(ins) == 2:
        q = [(ins[0], out[0]), (ins[0], out[1]), (ins[1], out[1]), (ins[1], out[0])]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    else:
        a, b = (ins[0], out) if len(ins) == 1 else (out[0], ins)
        tris = [[(a, b[0]), (a, b[1]), (a, b[2])]]
    res = []
    for tri in tris:
        m = [0.5 * (P[p] + P[q_]) for p, q_ in tri]
        s = float(np.dot(np.cross(m[1] - m[0], m[2] - m[0]), grad))
        assert s != 0
        if s < 0:
            tri = [tri[0], tri[2], tri[1]]
        res.append([(min(p, q_), max(p, q_)) for p, q_ in tri])
    return res


TET_CASES = [[tet_case(tet_corners(t), code) for code in range(16)] for t in range(6)]


def corner_offset(m, M):
    return (m & 1) + ((m >> 1) & 1) * M + ((m >> 2) & 1) * M * M


def extract(chi, W, iso, origin, h, depth):
    """vertices [V, 3] float64 in ascending edge key, triangles [T, 3] int32 by (cell, tetrahedron, triangle), weights [V], keys [V]."""
    R = 2 ** depth
    M = R + 1
    inside = chi < iso
    index = np.arange(M * M * M, dtype=np.int64).reshape(M, M, M)
    keys = []
    for d in range(1, 8):
        dx, dy, dz = d & 1, (d >> 1) & 1, (d >> 2) & 1
        lo = (slice(0, M - dz), slice(0, M - dy), slice(0, M - dx))
        hi = (slice(dz, M), slice(dy, M), slice(dx, M))
        cross = inside[lo] != inside[hi]
        keys.append(index[lo][cross] * 8 + d)
    keys = np.sort(np.concatenate(keys))
    node, d = keys // 8, keys % 8
    upper = node + (d & 1) + ((d >> 1) & 1) * M + ((d >> 2) & 1) * M * M
    cf, wf = np.ravel(chi), np.ravel(W)
    fa, fb = cf[node], cf[upper]
    t = (iso - fa) / (fb - fa)
    ijk = [node % M, (node // M) % M, node // (M * M)]
    vertices = np.zeros((len(keys), 3))
    for a in range(3):
        pa = origin[a] + ijk[a].astype(np.float64) * h
        vertices[:, a] = pa + t * (((d >> a) & 1).astype(np.float64) * h)
    weights = wf[node] + t * (wf[upper] - wf[node])

    cell_node = index[:R, :R, :R]
    cell_id = np.arange(R * R * R, dtype=np.int64).reshape(R, R, R)
    rows = []
    for tet in range(6):
        c = tet_corners(tet)
        code = np.zeros((R, R, R), np.int64)
        for p in range(4):
            dx, dy, dz = c[p] & 1, (c[p] >> 1) & 1, (c[p] >> 2) & 1
            code |= inside[dz:dz + R, dy:dy + R, dx:dx + R].astype(np.int64) << p
        for cd in range(1, 15):
            sel = code == cd
            if not sel.any():
                continue
            base, cid = cell_node[sel], cell_id[sel]
            for k, tri in enumerate(TET_CASES[tet][cd]):
                v = [np.searchsorted(keys, (base + corner_offset(c[lo], M)) * 8 + (c[hi] ^ c[lo])) for lo, hi in tri]
                rows.append(np.stack([cid, np.full_like(cid, tet), np.full_like(cid, k)] + v, 1))
    if rows:
        rows = np.concatenate(rows)
        rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
        triangles = rows[:, 3:].astype(np.int32)
    else:
        triangles = np.zeros((0, 3), np.int32)
    return vertices, triangles, weights, keys


# ---- (g) the density ------------------------------------------------------------------------------------------------------------------------
def density(weights, depth):
    """The depth at which the local sampling would put one sample per cell of a surface: depth + log2(max(weight, 4^-depth)) / 2."""
    return depth + np.log2(np.maximum(weights, 4.0 ** -depth)) / 2


# ---- the whole --------------------------------------------------------------------------------------------------------------------------------
def field(points, normals, depth=8, width=0, scale=1.1, cycles=CYCLES, grid=None):
    """Every stage: a dict with origin, h, depth, W, V, rhs, chis (chi after every cycle), chi and iso."""
    points, normals = check_inputs(points, normals, scale)
    if cycles < 1:
        raise ValueError("cycles must be >= 1")
    origin, h, depth = grid_of(points, depth, width, scale) if grid is None else (np.asarray(grid[0], np.float64), float(grid[1]), check_depth(grid[2]))
    if not (np.isfinite(origin).all() and np.isfinite(h) and h > 0):
        raise ValueError("the grid is not finite or its cell size is not positive")
    W, V = splat(points, normals, origin, h, depth)
    rhs = divergence(V, h)
    chis = solve(rhs, h, cycles)
    return dict(origin=origin, h=h, depth=depth, W=W, V=V, rhs=rhs, chis=chis, chi=chis[-1], iso=iso_value(W, chis[-1]))


def reconstruct(points, normals, depth=8, width=0, scale=1.1, linear_fit=False, cycles=CYCLES, grid=None):
    f = field(points, normals, depth, width, scale, cycles, grid)
    vertices, triangles, weights, _ = extract(f["chi"], f["W"], f["iso"], f["origin"], f["h"], f["depth"])
    return vertices, triangles, density(weights, f["depth"])
