"""The clouds, triangle lists, grids, cameras and images at which the DSM and orthophoto kernels (csrc/dsm.hip, csrc/dsm_cell.h) can go
wrong, shared by tests/test_dsm_cpu.py (a host build of dsm_cell.h) and tests/test_gpu_dsm_edges.py (the kernels through the C ABI):
the smallest shapes at every boundary between two code paths. Three lists, every array read-only:

  binning   name, points [n, 3] float64, step                          expected: dsm_oracle.bin_points
  raster    name, bx by bz [m] float32, simplices [T, 3] int32, transform [T, 3, 2] float64, bounds [4], xq, yq, step, fill
                                                                       expected: dsm_oracle.rasterize
  colours   name, xq [cols], yq [rows], z [rows, cols] float64 (the item (r, c) is the point (xq[c], yq[r], z[r, c])), cam [28],
            image [h, w, cin] uint8, chmaps (tuple of int32 arrays)    expected: dsm_oracle.project_colors, dsm_oracle.ortho_bytes

The transforms of hand-made triangles are data, computed with numpy the way scipy lays them out (dsm_oracle.transforms_of). Expected
results are computed once per case and shared."""
import functools

import numpy as np

import dsm_oracle as O

F32 = np.float32
TWO63 = 2.0 ** 63
BELOW_TWO63 = float(np.nextafter(F32(TWO63), F32(0)))           # 2^63 - 2^39: the largest float32 that numpy casts to int64
KERNEL_BOUND = float(F32(9.2e18))                                # the float32 literal `floor_index` compared against before this list


def _ro(a, dtype=None):
    a = np.array(a, dtype=dtype, order="C")
    a.setflags(write=False)
    return a


# ---- binning ---------------------------------------------------------------------------------------------------------------------------
def _bin_case(name, points, step):
    return {"name": name, "points": _ro(points, np.float64), "step": float(step)}


def _cloud(n, seed, extent):
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(-extent, extent, (n, 2)), rng.normal(5.0, 1.0, n)]


def _lattice_groups(G, per, seed):
    """G bins of `per` points each at step 1: the bins (i mod 16, i div 16), the points within 0.3 of their bin."""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(G), per)
    xy = np.stack([i % 16, i // 16], 1) + rng.uniform(-0.3, 0.3, (G * per, 2))
    p = np.c_[xy, rng.normal(0.0, 1.0, G * per)]
    return p[rng.permutation(len(p))]


@functools.lru_cache(maxsize=None)
def binning():
    cases = []
    for n in (1, 2, 255, 256, 257, 65536, 65537):                # the scan's block of 256 items, and 256 blocks of them (scan_top loops)
        cases.append(_bin_case(f"n{n}", _cloud(n, 10 + n, 2.0 + n ** 0.5 / 8), 0.5))
    for G in (1, 255, 256, 257):
        cases.append(_bin_case(f"groups_{G}", _lattice_groups(G, 3, 20 + G), 1.0))
    rng = np.random.default_rng(3)
    cases.append(_bin_case("one_bin_257", np.c_[rng.uniform(-0.2, 0.2, (257, 2)) + [3.0, -2.0], rng.normal(0, 1, 257)], 1.0))
    half = np.array([0.25, 0.75, -0.25, -0.75, 1.25, 1.75, 2.25, -1.25])                       # exactly half a step: half to even
    cases.append(_bin_case("half_step_ties", np.c_[np.repeat(half, 8), np.tile(half, 8), np.arange(64.0)], 0.5))
    # +-0 keys: -0.04 and +0.04 round to -0.0 and +0.0 at step 0.1; the bin keeps the sign of the row with the lowest z
    for axis in (0, 1):
        for first in (-1.0, 1.0):
            p = np.array([[0.04 * first, 0.04 * first, 1.0], [-0.04 * first, -0.04 * first, 2.0], [0.52, 0.31, 0.5], [-0.04 * first, 0.04 * first, 3.0]])
            p[:, 1 - axis] = [0.7, 0.7, 0.2, 0.7]
            cases.append(_bin_case(f"zero_key_{'xy'[axis]}_{'neg' if first < 0 else 'pos'}_first", p, 0.1))
    nan, inf = np.nan, np.inf

    def groups(*zs):
        return np.array([[float(g), 1.0, z] for g, col in enumerate(zs) for z in col])

    cases.append(_bin_case("nan_z_in_group", groups([1.5, nan, 2.5, nan], [3.0]), 1.0))
    cases.append(_bin_case("all_nan_group", groups([nan, nan], [1.0, 2.0], [nan]), 1.0))
    cases.append(_bin_case("inf_in_group", groups([1.0, inf, 2.0], [0.1, 0.2, inf, 0.3], [-inf, 5.0, 1e300]), 1.0))
    cases.append(_bin_case("inf_and_minf", groups([inf, -inf, 1.0], [2.0, 3.0]), 1.0))
    cases.append(_bin_case("signed_zero_z", groups([-0.0, 0.0, -0.0], [0.0, -0.0], [-0.0, -0.0]), 1.0))
    cases.append(_bin_case("equal_z_in_a_bin", groups([0.1, 0.1, 0.1, 1e16, 0.1, -1e16, 0.1], [0.3, 0.3, 0.7, 0.7, 0.3]), 1.0))
    rng = np.random.default_rng(4)
    world = np.c_[rng.uniform(0, 3, (300, 2)) + [1.0e6, 2.5e6], rng.normal(2000.0, 3.0, 300)]
    cases.append(_bin_case("world_frame_1e6", world, 0.1))
    cases.append(_bin_case("negative_step", _cloud(300, 5, 4.0), -0.5))
    tie = np.array([0.25, 0.75, 1.25, 100.25])
    near = np.concatenate([np.nextafter(tie, np.inf), np.nextafter(tie, -np.inf), tie + tie * 2.0 ** -26, tie - tie * 2.0 ** -26])
    cases.append(_bin_case("float64_next_to_a_tie", np.c_[near, near[::-1], np.arange(len(near), dtype=np.float64)], 0.5))
    return tuple(cases)


def binning_names():
    return [c["name"] for c in binning()]


def binning_case(name):
    return next(c for c in binning() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def binned(name):
    """(bx, by, bz) of a binning case from the oracle."""
    c = binning_case(name)
    return tuple(_ro(a) for a in O.bin_points(c["points"], c["step"]))


# ---- raster ----------------------------------------------------------------------------------------------------------------------------
def _raster_case(name, bx, by, bz, simplices, xlim, ylim, step, fill=np.nan, transform=None, bounds=None):
    bx, by, bz = _ro(bx, F32), _ro(by, F32), _ro(bz, F32)
    simplices = _ro(np.asarray(simplices).reshape(-1, 3), np.int32)
    transform = O.transforms_of(bx, by, simplices) if transform is None else transform
    if bounds is None:
        used = np.unique(simplices)
        bounds = [bx[used].min(), by[used].min(), bx[used].max(), by[used].max()]
    xq, yq = O.grid_axes(xlim, ylim, step)
    return {"name": name, "bx": bx, "by": by, "bz": bz, "simplices": simplices, "transform": _ro(transform, np.float64),
            "bounds": _ro(bounds, np.float64), "xq": _ro(xq, np.float64), "yq": _ro(yq, np.float64), "step": float(step), "fill": float(fill)}


def lattice_cloud(n, seed, extent=12.0):
    """Half the points on integer coordinates, as the random clouds of tests/test_gpu_dsm.py: cocircular quadruples everywhere."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, extent, (n, 2))
    xy[:n // 2] = rng.integers(0, int(extent) + 1, (n // 2, 2))
    z = 5 + np.sin(xy[:, 0] / 7) * 3 + np.cos(xy[:, 1] / 5) + rng.normal(0, 0.1, n)
    z[rng.random(n) < 0.02] = np.nan
    return _ro(np.c_[xy, z])


LATTICE = {"lattice_step_1": (400, 1, 1.0), "lattice_step_05": (400, 2, 0.5), "lattice_step_025": (400, 3, 0.25)}


def _qhull_case(name, points, step, xlim=None, ylim=None, fill=np.nan):
    bx, by, bz = O.bin_points(points, step)
    tri = O.triangulate(bx, by)
    dx, dy = O.default_limits(points)
    return _raster_case(name, bx, by, bz, tri.simplices, dx if xlim is None else xlim, dy if ylim is None else ylim, step, fill,
                        transform=tri.transform, bounds=np.r_[tri.min_bound, tri.max_bound])


def _strip(T, along_y=False, height=2.0, pitch=0.5):
    """T triangles (k, k + 1, k + 2) over the zigzag vertices (k * pitch, (k mod 2) * height), or the same turned by 90 degrees."""
    k = np.arange(T + 2)
    a, b = k * pitch, (k % 2) * height
    bz = np.sin(k * 0.37) + 0.01 * k
    simp = np.stack([k[:-2], k[1:-1], k[2:]], 1)
    return (b, a, bz, simp) if along_y else (a, b, bz, simp)


def _zoo():
    """Hand-made triangles on a grid of step 0.5 over [0, 8) x [0, 6): index order, degenerate and overlapping ones, rows and edges."""
    v = [(0.0, 20.0), (1.0, 20.0), (0.5, 21.0),        # 0-2    triangle 0: above the grid, no span
         (0.0, 0.0), (3.0, 0.0), (0.0, 3.0),           # 3-5    a live triangle, vertices exactly on cells
         (1.0, 1.0), (2.0, 2.0), (3.0, 3.0),           # 6-8    collinear: a NaN transform between two live ones
         (3.0, 0.0), (3.0, 3.0), (0.0, 3.0),           # 9-11   live, shares the diagonal with the first live one
         (0.25, 30.0), (1.0, 31.0), (2.0, 30.5),       # 12-14  a run of triangles above the grid (used three times)
         (4.0, 1.0), (7.0, 1.0), (5.5, 4.0),           # 15-17  a horizontal edge on the grid row y = 1
         (4.5, 0.0), (7.5, 0.5), (5.5, 3.0),           # 18-20  overlaps the one before: the lower index wins where both contain a cell
         (4.0, 5.0), (5.0, 5.0), (7.0, 5.0),           # 21-23  zero height, on the grid row y = 5
         (0.1, 4.1), (2.9, 4.2), (1.5, 4.4),           # 24-26  between the grid rows y = 4 and y = 4.5: no row inside it
         (6.0, 2.0), (7.5, 2.0), (7.5, 5.5),           # 27-29  live, then once more as an identical triangle
         (0.3, -9.0), (0.9, -9.0), (0.6, -8.0)]        # 30-32  the last triangles: below the grid
    bx, by = np.array(v).T
    bz = np.arange(len(v)) * 0.25 - 2.0
    simp = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11), (12, 13, 14), (12, 13, 14), (12, 13, 14), (15, 16, 17), (18, 19, 20), (21, 22, 23),
            (24, 25, 26), (27, 28, 29), (27, 28, 29), (30, 31, 32), (30, 32, 31)]
    return bx, by, bz, simp


def stride_case(cus):
    """More spans than the 16 * cus blocks of 256 threads of `dsm_raster_kernel` cover at once: 260 triangles as tall as a grid of
    ny x 3 cells, every one with a span on every row. Spans are numbered in triangle order, so the triangles that reach one of the three
    grid columns are listed last and ny is chosen so that the last STRIDE_TAIL triangles lie wholly beyond the first 16 * 256 * cus
    spans: every cell is won by a span that a thread takes in its second turn of the grid-stride loop (`second_turn_cells`)."""
    T = 260
    ny = (16 * 256 * cus) // (T - STRIDE_TAIL) + 8
    step = 0.25
    pitch = 0.75 / (T + 1)
    bx, by, bz, simp = _strip(T, height=(ny + 1) * step, pitch=pitch)
    xq = np.arange(0.125, 0.875, step)
    k = np.arange(T)
    reaches = ((k[:, None] * pitch <= xq[None, :]) & (xq[None, :] <= (k[:, None] + 2) * pitch)).any(axis=1)
    assert 3 <= reaches.sum() <= STRIDE_TAIL
    simp = np.concatenate([simp[~reaches], simp[reaches]])
    return _raster_case(f"stride_{cus}_cus", bx, by - step, bz, simp, [0.125, 0.875], [0.0, ny * step], step)


STRIDE_TAIL = 12


def second_turn_cells(c, cus):
    """(cells won by a span whose number offs[t] + (r - r0[t]) is at least 16 * 256 * cus, cells inside a triangle): the spans beyond the
    raster kernel's grid, which a thread reaches only by going round its loop again."""
    r0, r1 = O.span_rows(c["by"], c["simplices"], c["transform"], float(c["yq"][0]), abs(c["step"]), len(c["yq"]))
    counts = r1 - r0 + 1
    offs = np.cumsum(counts) - counts
    gx, gy = np.meshgrid(c["xq"], c["yq"])
    s = O.lowest_simplex(c["transform"], gx.ravel(), gy.ravel())
    row = np.repeat(np.arange(len(c["yq"])), len(c["xq"]))
    ok = s >= 0
    span = offs[s[ok]] + (row[ok] - r0[s[ok]])
    return int((span >= 16 * 256 * cus).sum()), int(ok.sum())


@functools.lru_cache(maxsize=None)
def raster():
    cases = []
    for name, (n, seed, step) in LATTICE.items():
        cases.append(_qhull_case(name, lattice_cloud(n, seed), step))
    for T in (1, 2, 255, 256, 257):                              # the scan's block of 256 triangles
        bx, by, bz, simp = _strip(T)
        cases.append(_raster_case(f"strip_{T}", bx, by, bz, simp, [-0.5, 0.5 * (T + 2) + 0.5], [-0.5, 2.75], 0.25))
    # 65 537 triangles down a vertical strip, a grid of 8 x 8 cells across its middle: scan_top_kernel loops, and all but a few
    # triangles have no span (leading and trailing runs of equal offsets in the binary search)
    bx, by, bz, simp = _strip(65537, along_y=True)
    mid = 0.5 * 32768
    cases.append(_raster_case("strip_65537_cropped", bx, by, bz, simp, [0.0, 2.0], [mid, mid + 2.0], 0.25))
    # the same strip cropped at its far end: the live triangles include index 65 536, whose offset is written in scan_top_kernel's second
    # round (block sum 256) and needs the carry of the first
    end = 0.5 * 65536
    cases.append(_raster_case("strip_65537_far_end", bx, by, bz, simp, [0.0, 2.0], [end - 0.5, end + 1.5], 0.25))
    zx, zy, zz, zs = _zoo()
    cases.append(_raster_case("zoo", zx, zy, zz, zs, [0.0, 8.0], [0.0, 6.0], 0.5))
    cases.append(_raster_case("zoo_bounds_inside", zx, zy, zz, zs, [0.0, 8.0], [0.0, 6.0], 0.5, fill=-9999.0, bounds=[1.0, 0.5, 6.5, 4.0]))
    cases.append(_raster_case("zoo_fill_zero", zx, zy, zz, zs, [-1.0, 9.0], [-1.0, 7.0], 0.25, fill=0.0))
    nanz = zz.copy()
    nanz[[4, 16]] = np.nan
    cases.append(_raster_case("zoo_nan_vertex", zx, zy, nanz, zs, [0.0, 8.0], [0.0, 6.0], 0.5))
    cases.append(_raster_case("grid_1x1", zx, zy, zz, zs, [1.0, 1.5], [1.0, 1.5], 0.5))
    cases.append(_raster_case("grid_1xN", zx, zy, zz, zs, [0.0, 8.0], [1.0, 1.5], 0.5))
    cases.append(_raster_case("grid_Nx1", zx, zy, zz, zs, [5.5, 6.0], [0.0, 6.0], 0.5))
    cases.append(_raster_case("xlim_outside", zx, zy, zz, zs, [40.0, 44.0], [0.0, 6.0], 0.5, fill=-9999.0))
    cases.append(_raster_case("ylim_outside", zx, zy, zz, zs, [0.0, 8.0], [-60.0, -56.0], 0.5, fill=0.0))
    cases.append(stride_case(256))
    return tuple(cases)


def raster_names():
    return [c["name"] for c in raster()]


def raster_case(name):
    return next(c for c in raster() if c["name"] == name)


def rasterized(c):
    return O.rasterize(c["bx"], c["by"], c["bz"], c["simplices"], c["transform"], c["bounds"], c["xq"], c["yq"], c["fill"])


@functools.lru_cache(maxsize=None)
def raster_expected(name):
    z = rasterized(raster_case(name))
    z.setflags(write=False)
    return z


def spans_of(c):
    return O.span_count(c["by"], c["simplices"], c["transform"], float(c["yq"][0]), abs(c["step"]), len(c["yq"]))


def non_unique_share(c):
    """Of the cells inside the triangulation, the share whose smallest barycentric coordinate in their lowest simplex is <= 1e-12: on an
    edge or a vertex, where another triangle contains the cell too."""
    gx, gy = np.meshgrid(c["xq"], c["yq"])
    qx, qy = gx.ravel(), gy.ravel()
    s = O.lowest_simplex(c["transform"], qx, qy)
    ok = s >= 0
    c0, c1, c2 = O.barycentric_of(c["transform"][s[ok]], qx[ok], qy[ok])
    return float((np.minimum(np.minimum(c0, c1), c2) <= 1e-12).mean()), int(ok.sum())


# ---- colours ---------------------------------------------------------------------------------------------------------------------------
IDENTITY_CAM = np.r_[1.0, 1.0, 0.0, 0.0, np.eye(3).ravel(), np.zeros(3), np.zeros(12)]      # u = X / Z and v = Y / Z exactly at Z = 1


def camera_vector(K, R, t, k):
    kk = np.zeros(12)
    kk[:len(k)] = k
    K = np.asarray(K, np.float64)
    return np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64).ravel(), kk]


def image_bytes(h, w, cin, seed):
    """Random bytes; the first and last column and row differ from each other everywhere, 0 and 255 are present."""
    rng = np.random.default_rng(seed)
    im = rng.integers(1, 255, (h, w, cin), dtype=np.uint8)
    im[:, 0] = np.minimum(im[:, 0], 120)
    im[:, -1] = np.maximum(im[:, -1], 130) if w > 1 else im[:, -1]
    im[0] = (im[0] // 2) * 2
    im[-1] = (im[-1] // 2) * 2 + 1 if h > 1 else im[-1]
    im[h // 2, w // 2] = 255
    im[h // 2, max(w // 2 - 1, 0)] = 0 if w > 1 else im[h // 2, 0]
    return im


CHMAPS = {1: ((0,), (0, 0, 0), (0, 0), (0, 0, 0, 0)), 3: ((2, 1, 0), (0, 1, 2), (1,), (0, 2), (2, 2, 1, 0)),
          4: ((2, 1, 0), (0, 1, 2, 3), (3, 2, 1, 0), (3,), (3, 0))}


def _colour_case(name, xq, yq, z, cam, image, chmaps=None):
    image = _ro(image, np.uint8)
    chmaps = CHMAPS[image.shape[2]][:2] if chmaps is None else chmaps
    return {"name": name, "xq": _ro(xq, np.float64), "yq": _ro(yq, np.float64), "z": _ro(z, np.float64), "cam": _ro(cam, np.float64),
            "image": image, "chmaps": tuple(_ro(m, np.int32) for m in chmaps)}


def probe_positions(n):
    """u (and v) of the probe for an image of n columns (rows): every position the sampling treats differently, float32-exact."""
    f = lambda v: float(F32(v))      # noqa: E731
    near = [f(np.nextafter(F32(v), F32(s))) for v in (KERNEL_BOUND, TWO63, 2.0 ** 31) for s in (0.0, np.inf)]
    # 1 / 3 and e carry a full float32 mantissa: the products of the weights round, so that clipped corners cancel to a residue only
    pos = [f(1.0 / 3.0), f(np.e), 0.25, 1.0, 2.5, n - 2.0, n - 1.25, n - 1.0, n - 0.5, float(n), n + 1.25, 1e9, 2.0 ** 31, 3e9, f(1e12), KERNEL_BOUND, BELOW_TWO63, TWO63,
           1e39] + near
    neg = [-0.5, -1.0, -1.5, -5.0, -1e9, -2.0 ** 31, f(-3e9), -KERNEL_BOUND, -BELOW_TWO63, -TWO63, -1e39] + [-v for v in near]
    return np.array(sorted(set(neg + pos)) + [-0.0, 0.0, np.nan])


@functools.lru_cache(maxsize=None)
def colours():
    cases = []
    # the probe: the identity camera at Z = 1 puts (u, v) exactly on every pair of positions; some cells at Z = 0 (zz == 0: the divide is
    # skipped), behind the camera and NaN
    for cin in (1, 3, 4):
        p = probe_positions(6)
        z = np.ones((len(p), len(p)))
        z[3, 5], z[7, 2], z[20, 20], z[11, 13], z[0, 0] = 0.0, -1.0, np.nan, -0.0, -2.0
        cases.append(_colour_case(f"probe_cin{cin}", p, p, z, IDENTITY_CAM, image_bytes(6, 6, cin, 40 + cin), CHMAPS[cin]))
    p1 = probe_positions(1)
    cases.append(_colour_case("probe_image_1x1", p1, p1, np.ones((len(p1), len(p1))), IDENTITY_CAM, image_bytes(1, 1, 3, 50)))
    pw = probe_positions(9)
    cases.append(_colour_case("probe_image_4x9", pw, probe_positions(4), np.ones((len(probe_positions(4)), len(pw))), IDENTITY_CAM, image_bytes(4, 9, 3, 51)))
    # far outside the image along one axis (1e16 .. 1e19, full float32 mantissa) and inside it along the other: the two corners along
    # the far axis clip to one pixel and their weights cancel to the rounding residue of a sum near 1e16 .. 1e19, a few units to
    # thousands of either sign, far outside [0, 1]: the uint8 cast of the orthophoto wraps
    rng = np.random.default_rng(7)
    far = (10.0 ** rng.uniform(16.0, 18.9, 12) * rng.choice([-1.0, 1.0], 12)).astype(F32).astype(np.float64)
    near = rng.uniform(0.0, 5.0, 12).astype(F32).astype(np.float64)
    cases.append(_colour_case("far_outside_residues", np.r_[far[:6], near[:6]], np.r_[near[6:], far[6:]], np.ones((12, 12)), IDENTITY_CAM,
                              image_bytes(6, 6, 3, 52)))
    # a real camera: every distortion length, thin-prism terms, a footprint that leaves the image on every side
    a, b = 0.05, -0.03
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    K, t = [[60.0, 0.0, 31.5], [0.0, 62.0, 23.25], [0.0, 0.0, 1.0]], [0.1, -0.2, 12.0]
    rng = np.random.default_rng(6)
    xq, yq = np.linspace(-9.0, 9.0, 23), np.linspace(-7.0, 7.0, 19)
    z = rng.normal(0.0, 0.5, (19, 23))
    z[rng.random(z.shape) < 0.05] = np.nan
    z[4, 4] = -40.0                                               # behind the camera
    dists = {"d0": [], "d4": [-0.12, 0.03, 1e-3, -2e-3], "d5": [-0.12, 0.03, 1e-3, -2e-3, 0.01], "d8": [-0.12, 0.03, 1e-3, -2e-3, 0.01, 0.05, -0.01, 2e-3],
             "thin_prism": [-0.12, 0.03, 1e-3, -2e-3, 0.01, 0.05, -0.01, 2e-3, 3e-3, -1e-3, 2e-3, 4e-3]}
    for name, k in dists.items():
        cases.append(_colour_case(f"camera_{name}", xq, yq, z, camera_vector(K, R, t, k), image_bytes(48, 64, 3, 60)))
    # k[5] = -1: the rational denominator 1 + k[5] r2 is exactly 0 where r2 == 1 (1 / 0: inf, and 0 * inf: NaN)
    cam = IDENTITY_CAM.copy()
    cam[16 + 5] = -1.0
    unit = np.array([-1.0, 0.0, 1.0, 0.5])
    cases.append(_colour_case("rational_denominator_0", unit, unit, np.ones((4, 4)), cam, image_bytes(5, 5, 3, 61)))
    # zz == 0 under a real pose: t_z = 0 and points in the plane Z = 0
    cases.append(_colour_case("zz_0", xq[:5], yq[:5], np.zeros((5, 5)), camera_vector(K, np.eye(3), [0.0, 0.0, 0.0], dists["d5"]), image_bytes(48, 64, 3, 62)))
    cases.append(_colour_case("one_cell_nan_z", [1.0], [2.0], [[np.nan]], IDENTITY_CAM, image_bytes(6, 6, 3, 63)))
    cases.append(_colour_case("one_cell", [1.5], [2.25], [[1.0]], IDENTITY_CAM, image_bytes(6, 6, 3, 64)))
    return tuple(cases)


def colour_names():
    return [c["name"] for c in colours()]


def colour_case(name):
    return next(c for c in colours() if c["name"] == name)


def colour_points(c):
    """[rows * cols, 3] float64: item r * cols + c is (xq[c], yq[r], z[r, c])."""
    gx, gy = np.meshgrid(c["xq"], c["yq"])
    return np.ascontiguousarray(np.stack([gx.ravel(), gy.ravel(), c["z"].ravel()], 1))


@functools.lru_cache(maxsize=None)
def colour_expected(name, k):
    """(proj [n, 2] float32, col [n, cout] float64, ortho [n, 3] uint8 or None) of a case under its k-th channel map; proj and col as a
    cloud of points (a NaN z goes through the arithmetic), ortho as grid cells (a NaN z is black)."""
    c = colour_case(name)
    pts = colour_points(c)
    proj, col = O.project_colors(pts, c["cam"], c["image"], c["chmaps"][k])
    ortho = O.ortho_bytes(col, pts[:, 2]) if col.shape[1] == 3 else None
    for a in (proj, col, ortho):
        if a is not None:
            a.setflags(write=False)
    return proj, col, ortho
