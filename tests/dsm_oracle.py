"""Numpy + scipy restatement of the reference's DSM and orthophoto products (`src/icepy4d/utils/dsm_orthophoto.py`: `build_dsm`,
`generate_ortophoto`; `sfm/interpolate_colors.py`: `interpolate_point_colors`, `bilinear_interpolate`; `sfm/geometry.py`:
`project_points`), written from their description. It needs no pandas and no OpenCV: the group mean is pandas' Kahan sum restated,
and the projection is `cv2.projectPoints` restated in float64. Checked bit for bit against the reference's own outputs in
tests/golden/g12_dsm_orthophoto.npz (tests/test_dsm_cpu.py) and used for random device cases (tests/test_gpu_dsm.py).

`interpolate` finds each cell's triangle with scipy's own `find_simplex`, so it reproduces `LinearNDInterpolator` exactly. The
device takes the lowest simplex index that contains a cell instead; the two agree except on cells that lie on a shared edge or
vertex, where both are valid and the values differ in the last bits. `lowest_simplex` / `rasterize` restate the device's rule by
brute force over all triangles, `project_colors` / `ortho_bytes` the colouring from the 28-vector of the C entry point: what the
host build of csrc/dsm_cell.h (tests/test_dsm_cpu.py) and the kernels (tests/test_gpu_dsm_edges.py) are compared with bit for bit."""
import numpy as np
from scipy.spatial import Delaunay

EPS = 100 * np.finfo(np.float64).eps      # scipy's inside tolerance (`_find_simplex`, `_barycentric_inside`)


def load_g12(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def round_to_step(a, step):
    """`round_to_val` of `build_dsm`: float32(rint(float32(a) / float32(step)) * float32(step)), half to even."""
    s = np.float32(step)
    return np.round(np.asarray(a, np.float32) / s) * s


def kahan_group_mean(values, starts):
    """pandas' groupby mean over consecutive groups `values[starts[g]:starts[g + 1]]`: Kahan sum of the non-NaN values in order,
    divided by their count; NaN for a group without one. float64."""
    values = np.asarray(values, np.float64)
    starts = np.asarray(starts, np.int64)
    sizes = np.diff(starts)
    G = len(sizes)
    s, c, n = np.zeros(G), np.zeros(G), np.zeros(G, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(int(sizes.max(initial=0))):
            g = np.flatnonzero(sizes > k)
            v = values[starts[g] + k]
            ok = ~np.isnan(v)
            g, v = g[ok], v[ok]
            y = v - c[g]
            t = s[g] + y
            cg = (t - s[g]) - y
            cg[np.isnan(cg)] = 0.0          # pandas resets a NaN compensation (an infinite value)
            c[g], s[g] = cg, t
            n[g] += 1
        return np.where(n > 0, s / np.maximum(n, 1), np.nan)


def bin_points(points3d, step):
    """Rounding, sorting and grouping of `build_dsm`: (x, y, z) float32 of the groups in ascending (x, y)."""
    p = np.asarray(points3d)
    xr, yr = round_to_step(p[:, 0], step), round_to_step(p[:, 1], step)
    z = p[:, 2].astype(np.float64)
    ind = np.lexsort((yr, z))                       # the reference's d_sort: z first, then y, stable
    xs, ys, zs = xr[ind], yr[ind], z[ind]
    grp = np.lexsort((ys, xs))                      # groupby(sort=True): groups by (x, y), rows kept in d_sort order
    gx, gy, gz = xs[grp], ys[grp], zs[grp]
    new = np.ones(len(gx), bool)
    new[1:] = (gx[1:] != gx[:-1]) | (gy[1:] != gy[:-1])     # -0.0 == 0.0: one group
    starts = np.r_[np.flatnonzero(new), len(gx)]
    bx, by = gx[new].copy(), gy[new].copy()
    # a key value of zero keeps the sign of its first occurrence in d_sort (pandas factorises each key column on its own)
    for b, col in ((bx, xs), (by, ys)):
        zero = np.flatnonzero(col == 0)
        if len(zero):
            b[b == 0] = col[zero[0]]
    return bx, by, kahan_group_mean(gz, starts).astype(np.float32)


def default_limits(points3d):
    p = np.asarray(points3d)
    x, y = p[:, 0], p[:, 1]
    return [np.floor(x.min()), np.ceil(x.max())], [np.floor(y.min()), np.ceil(y.max())]


def grid_axes(xlim, ylim, step):
    return np.arange(xlim[0], xlim[1], step), np.arange(ylim[0], ylim[1], step)


def triangulate(bx, by):
    """scipy's Delaunay on float64 of the float32 binned (x, y), default options: the triangulation `LinearNDInterpolator` builds."""
    return Delaunay(np.ascontiguousarray(np.stack([bx, by], 1), dtype=np.float64))


def barycentric_of(T, qx, qy):
    """(c0, c1, c2) of cells (qx, qy) under the transforms T [..., 3, 2], in scipy's operation order (no fused multiply-add in numpy)."""
    dx, dy = qx - T[..., 2, 0], qy - T[..., 2, 1]
    c0 = (0.0 + T[..., 0, 0] * dx) + T[..., 0, 1] * dy
    c1 = (0.0 + T[..., 1, 0] * dx) + T[..., 1, 1] * dy
    return c0, c1, (1.0 - c0) - c1


def barycentric(tri, simplex, qx, qy):
    """(c0, c1, c2) of cells (qx, qy) in `simplex` of a `Delaunay` object."""
    return barycentric_of(tri.transform[simplex], qx, qy)


def eval_cells_of(simplices, transform, values, simplex, qx, qy, fill):
    """z of cells whose simplex is known (-1: outside): ((0 + c0 v0) + c1 v1) + c2 v2 in float64."""
    out = np.full(len(qx), float(fill))
    ok = simplex >= 0
    s = simplex[ok]
    with np.errstate(invalid="ignore", over="ignore"):
        c0, c1, c2 = barycentric_of(np.asarray(transform)[s], qx[ok], qy[ok])
        v = np.asarray(values, np.float64)[np.asarray(simplices)[s]]
        out[ok] = ((0.0 + c0 * v[:, 0]) + c1 * v[:, 1]) + c2 * v[:, 2]
    return out


def eval_cells(tri, values, simplex, qx, qy, fill):
    return eval_cells_of(tri.simplices, tri.transform, values, simplex, qx, qy, fill)


def lowest_simplex(transform, qx, qy, block=1 << 21):
    """The lowest index t whose three barycentric coordinates of the cell lie in [-EPS, 1 + EPS]; -1 if none. Brute force over all
    triangles; a NaN transform never contains a cell (every comparison with it is false)."""
    T = np.asarray(transform, np.float64).reshape(-1, 3, 2)
    qx, qy = np.asarray(qx, np.float64), np.asarray(qy, np.float64)
    out = np.full(len(qx), -1, np.int64)
    if not len(qx):
        return out
    per = max(1, block // len(qx))
    with np.errstate(invalid="ignore", over="ignore"):
        for t0 in range(0, len(T), per):
            c0, c1, c2 = barycentric_of(T[t0:t0 + per, None], qx[None, :], qy[None, :])
            inside = (c0 >= -EPS) & (c0 <= 1.0 + EPS) & (c1 >= -EPS) & (c1 <= 1.0 + EPS) & (c2 >= -EPS) & (c2 <= 1.0 + EPS)
            hit = inside.any(axis=0) & (out < 0)
            out[hit] = t0 + inside[:, hit].argmax(axis=0)
    return out


def rasterize(bx, by, bz, simplices, transform, bounds, xq, yq, fill):
    """What `im_dsm_rasterize` computes: the lowest containing simplex of every cell, `fill` where there is none or the cell lies outside
    `bounds` (min x, min y, max x, max y) by more than EPS, else the interpolation of `eval_cells`. [len(yq), len(xq)] float64."""
    gx, gy = np.meshgrid(np.asarray(xq, np.float64), np.asarray(yq, np.float64))
    qx, qy = gx.ravel(), gy.ravel()
    s = lowest_simplex(transform, qx, qy)
    b = np.asarray(bounds, np.float64)
    s[(qx < b[0] - EPS) | (qx > b[2] + EPS) | (qy < b[1] - EPS) | (qy > b[3] + EPS)] = -1
    return eval_cells_of(simplices, transform, bz, s, qx, qy, fill).reshape(gx.shape)


def span_rows(by, simplices, transform, y0, dy, ny):
    """(r0, r1) per triangle: the grid rows its spans cover (its rows and one row of margin on each side), r1 < r0 where it has none."""
    T = np.asarray(transform, np.float64).reshape(-1, 6)
    y = np.asarray(by, np.float64)[np.asarray(simplices).reshape(-1, 3)]
    with np.errstate(invalid="ignore"):
        a = np.maximum(np.floor((y.min(axis=1) - y0) / dy) - 1.0, 0.0)
        b = np.minimum(np.ceil((y.max(axis=1) - y0) / dy) + 1.0, float(ny - 1))
        none = np.isnan(T[:, 0]) | ~(a <= b)
    return np.where(none, 0, a).astype(np.int64), np.where(none, -1, b).astype(np.int64)


def span_count(by, simplices, transform, y0, dy, ny):
    """The number of (triangle, grid row) spans `im_dsm_rasterize` walks: only to assert what the scan and stride cases claim."""
    r0, r1 = span_rows(by, simplices, transform, y0, dy, ny)
    return int((r1 - r0 + 1).sum())


def transforms_of(bx, by, simplices):
    """Barycentric transforms of hand-made triangles as scipy lays them out, [T, 3, 2]: the inverse of [[x0 - x2, x1 - x2],
    [y0 - y2, y1 - y2]], then the third vertex; NaN throughout for a singular triangle, as scipy leaves a degenerate simplex."""
    p = np.stack([np.asarray(bx, np.float64), np.asarray(by, np.float64)], 1)[np.asarray(simplices).reshape(-1, 3)]
    out = np.full((len(p), 3, 2), np.nan)
    A = np.swapaxes(p[:, :2] - p[:, 2:3], 1, 2)
    ok = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0] != 0
    out[ok, :2] = np.linalg.inv(A[ok])
    out[ok, 2] = p[ok, 2]
    return out


def min_barycentric(tri, simplex, qx, qy):
    """The smallest barycentric coordinate of each cell in its simplex (inf outside): above ~1e-12 the containing triangle is unique."""
    out = np.full(len(qx), np.inf)
    ok = simplex >= 0
    c0, c1, c2 = barycentric(tri, simplex[ok], qx[ok], qy[ok])
    out[ok] = np.minimum(np.minimum(c0, c1), c2)
    return out


def interpolate(tri, values, xq, yq, fill):
    """`LinearNDInterpolator(points, values, fill_value=fill)(*np.meshgrid(xq, yq))`: [len(yq), len(xq)] float64."""
    gx, gy = np.meshgrid(xq, yq)
    qx, qy = gx.ravel(), gy.ravel()
    s = tri.find_simplex(np.stack([qx, qy], 1)).astype(np.int64)
    return eval_cells(tri, values, s, qx, qy, fill).reshape(gx.shape)


def fill_of(fill_value, bz):
    if isinstance(fill_value, str) and fill_value == "mean":
        return bz.mean()
    return fill_value


def build_dsm(points3d, step, xlim=None, ylim=None, fill_value=np.nan):
    """Everything `build_dsm` computes: dict of binned x / y / z (float32), xq, yq and z ([len(yq), len(xq)] float64)."""
    p = np.asarray(points3d)
    dx, dy = default_limits(p)
    xlim = dx if xlim is None else xlim
    ylim = dy if ylim is None else ylim
    bx, by, bz = bin_points(p, step)
    xq, yq = grid_axes(xlim, ylim, step)
    tri = triangulate(bx, by)
    return {"bx": bx, "by": by, "bz": bz, "xq": xq, "yq": yq, "tri": tri,
            "z": interpolate(tri, bz, xq, yq, fill_of(fill_value, bz))}


def project_points_f64(points3d, K, dist, R, t):
    """`cv2.projectPoints` restated elementwise in float64: R X + t, the perspective divide, Brown k1 k2 p1 p2 [k3 [k4 k5 k6]]
    (rational), fx x + cx (the skew of K is not used, as in OpenCV). No Rodrigues round trip: R is used as given. [n, 2] float64."""
    P = np.asarray(points3d, np.float64)
    K = np.asarray(K, np.float64)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    k = np.zeros(12)
    d = np.zeros(0) if dist is None else np.asarray(dist, np.float64).ravel()
    k[:len(d)] = d
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    x = ((R[0, 0] * X + R[0, 1] * Y) + R[0, 2] * Z) + t[0]
    y = ((R[1, 0] * X + R[1, 1] * Y) + R[1, 2] * Z) + t[1]
    z = ((R[2, 0] * X + R[2, 1] * Y) + R[2, 2] * Z) + t[2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = np.where(z != 0, 1.0 / np.where(z != 0, z, 1.0), 1.0)
        x, y = x * z, y * z
        r2 = x * x + y * y
        r4 = r2 * r2
        r6 = r4 * r2
        a1 = 2 * x * y
        a2 = r2 + 2 * x * x
        a3 = r2 + 2 * y * y
        cdist = ((1 + k[0] * r2) + k[1] * r4) + k[4] * r6
        icdist2 = 1.0 / (((1 + k[5] * r2) + k[6] * r4) + k[7] * r6)
        xd = ((((x * cdist) * icdist2 + k[2] * a1) + k[3] * a2) + k[8] * r2) + k[9] * r4
        yd = ((((y * cdist) * icdist2 + k[2] * a3) + k[3] * a1) + k[10] * r2) + k[11] * r4
        return np.stack([xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]], 1)


def project_points(points3d, K, dist, R, t):
    """`project_points` of the reference: the projection above cast to float32."""
    return project_points_f64(points3d, K, dist, R, t).astype(np.float32)


def bilinear(im, x, y):
    """`bilinear_interpolate` of one float32 channel at float32 (x, y): clipped corners, weights from the unclipped position, float64."""
    x, y = np.asarray(x), np.asarray(y)
    with np.errstate(invalid="ignore"):
        x0 = np.floor(x).astype(np.int64)
        y0 = np.floor(y).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    x0, x1 = np.clip(x0, 0, im.shape[1] - 1), np.clip(x1, 0, im.shape[1] - 1)
    y0, y1 = np.clip(y0, 0, im.shape[0] - 1), np.clip(y1, 0, im.shape[0] - 1)
    Ia, Ib, Ic, Id = im[y0, x0], im[y1, x0], im[y0, x1], im[y1, x1]
    wa = (x1 - x) * (y1 - y)
    wb = (x1 - x) * (y - y0)
    wc = (x - x0) * (y1 - y)
    wd = (x - x0) * (y - y0)
    return ((wa * Ia + wb * Ib) + wc * Ic) + wd * Id


def interpolate_point_colors(points3d, image, K, dist, R, t, convert_BRG2RGB=True):
    """[n, channels] float64 colours in [0, 1] (before any cast)."""
    img = np.asarray(image)
    if convert_BRG2RGB:
        img = img[:, :, ::-1]
    uv = project_points(points3d, K, dist, R, t)
    f = img.astype(np.float32) / np.float32(255.0)
    return np.stack([bilinear(f[:, :, ch], uv[:, 0], uv[:, 1]) for ch in range(f.shape[2])], 1).reshape(len(uv), f.shape[2])


def to_uint8(a):
    """np.uint8 of a float64 array on x86: truncation to int32 (0x80000000 for NaN or out of range), low byte."""
    a = np.asarray(a, np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(a) & (a > -2147483649.0) & (a < 2147483648.0)
        i = np.where(ok, np.trunc(np.where(ok, a, 0.0)), 0).astype(np.int64)
    return np.where(ok, i & 0xFF, 0).astype(np.uint8)


def project_colors(points3d, cam, image, chmap):
    """`im_project_colors` on points: cam [28] = fx fy cx cy, R row-major, t, k[12] (thin-prism terms included); (proj [n, 2] float32,
    col [n, len(chmap)] float64), output channel ch sampled from image channel chmap[ch]."""
    cam = np.asarray(cam, np.float64)
    K = np.array([[cam[0], 0.0, cam[2]], [0.0, cam[1], cam[3]], [0.0, 0.0, 1.0]])
    with np.errstate(invalid="ignore", over="ignore"):
        uv = project_points(points3d, K, cam[16:28], cam[4:13], cam[13:16])
        f = np.asarray(image).astype(np.float32) / np.float32(255.0)
        col = np.stack([bilinear(f[:, :, int(m)], uv[:, 0], uv[:, 1]) for m in chmap], 1).reshape(len(uv), len(chmap))
    return uv, col


def ortho_bytes(col, z):
    """The orthophoto bytes of cells with the float64 colours `col` [n, 3]: float32, times 255, the uint8 cast; black where z is NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        out = to_uint8(np.asarray(col).astype(np.float32).astype(np.float64) * 255)
    out[np.isnan(np.asarray(z))] = 0
    return out


def orthophoto(xx, yy, zz, image, K, dist, R, t):
    """`generate_ortophoto`: [rows, cols, 3] uint8; cells with NaN z are black."""
    zz = np.asarray(zz, np.float64)
    xyz = np.stack([np.asarray(xx, np.float64).ravel(), np.asarray(yy, np.float64).ravel(), zz.ravel()], 1)
    valid = ~np.isnan(xyz[:, 2])
    cols = np.zeros((len(xyz), 3), np.float32)
    cols[valid] = interpolate_point_colors(xyz[valid], image, K, dist, R, t)
    return to_uint8(cols.astype(np.float64) * 255).reshape(zz.shape + (3,))


G12_CASES = ("s05", "s1", "narrow", "wide", "neg", "nanz", "nanz_mean")
G12_DISTS = ("d0", "d4", "d5", "d8")


def g12_case(g, name):
    """The arguments of a g12 `build_dsm` case: (points, step, xlim, ylim, fill_value) as the reference was called, plus the grid axes."""
    pts = g["pts_" + bytes(g[name + "_src"]).decode()]
    step = float(g[name + "_step"].reshape(-1)[0])
    lim = g[name + "_lim"]
    given = g[name + "_lim_given"]
    xlim = [float(lim[0]), float(lim[1])] if given[0] else None
    ylim = [float(lim[2]), float(lim[3])] if given[1] else None
    kind, num = g[name + "_fill"]
    fill = {0: np.nan, 1: "mean", 2: float(num)}[int(kind)]
    xq, yq = grid_axes(lim[:2], lim[2:], step)
    return pts, step, xlim, ylim, fill, xq, yq


def same_bits(a, b):
    """Same shape, dtype and bit pattern on every element (signed zeros included), a NaN equal to a NaN: IEEE 754 leaves the sign and
    payload of a NaN result open, whether an invalid operation makes it (inf - inf, 0 * inf) or a NaN operand passes through an
    addition or a product (a subtraction done as an addition of the negated operand flips its sign), and processors differ."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | both_nan).all())


def bits_equal(a, b):
    """Same shape, dtype and bit pattern (NaN payloads and signed zeros included)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
