"""The clouds, cell sizes, k and radii at which the neighbour search can go wrong, shared by tests/test_pointcloud_cpu.py (a host build
of csrc/knn_point.h) and tests/test_gpu_pointcloud.py (the kernels): the smallest shapes at every boundary between two code paths.
Every case is a dict: name, points [n, 3] float64 (read-only), s (cell size), ks (tuple), radius2s (tuple; inf = no radius).
The brute-force neighbours of a cloud are computed once (64 of them) and cut to every k and radius (knn_oracle.cut)."""
import functools

import numpy as np

import knn_oracle as O

KS = (1, 2, 10, 30, 50, 63, 64)
SIZES = tuple(sorted({n for k in KS for n in (k - 1, k, k + 1) if n >= 1} | {1, 2, 63, 64, 65, 257, 4099}))
INF = float("inf")


def _uniform(n, seed, scale=1.0):
    return np.random.default_rng(seed).uniform(0.0, scale, (n, 3))


def _lattice(m, step):
    g = np.arange(m, dtype=np.float64) * step            # i * step as a float64 product: on or next to the faces of cells of side `step`
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def _face_rounding(o, s, cells_wanted):
    """Triples (p, q, p') along x around faces of the grid (origin o, cell size s) at which the rounding of the cell assignment bites:
    p is the last float64 whose rounded cell coordinate fl(fl(p - o) / s) lies below the face L, q = p + d and p' = q + d lie in cell L
    (both sums exact), and the face distance computed without any safety margin, (fl(fl(q - o) / s) - L) * s, EXCEEDS d, the true
    distance to p. For k = 2 the query q ties p against p' at d * d; p, in the unvisited cell, carries the lower index and must win,
    which a search that trusts the unshrunk bound misses. Found by search, asserted here."""
    o, s = np.float64(o), np.float64(s)
    cell = lambda x: np.floor((x - o) / s)      # noqa: E731
    rows = []
    for L in cells_wanted:
        p = o + np.float64(L) * s
        for _ in range(64):
            if cell(p) >= L:
                p = np.nextafter(p, -np.inf)
        for _ in range(64):
            if cell(np.nextafter(p, np.inf)) < L:
                p = np.nextafter(p, np.inf)
        assert cell(p) == L - 1 and cell(np.nextafter(p, np.inf)) == L
        for j in range(1, 64):
            d = np.spacing(p) * j
            q, pp = p + d, p + d + d
            gap = (q - o) / s - np.float64(L)
            if q - p == d and pp - q == d and cell(q) == L and cell(pp) == L and d * d < (gap * s) * (gap * s):
                rows += [[p, 0, 0], [q, 0, 0], [pp, 0, 0]]
                break
        else:
            raise AssertionError(f"no triple at face {L}")
    return np.array(rows + [[o, 0, 0], [o + 100 * s, 0, 0]], np.float64)


def _case(name, points, s, ks=(10,), radius2s=(INF,)):
    p = np.ascontiguousarray(points, np.float64)
    p.setflags(write=False)
    return {"name": name, "points": p, "s": float(s), "ks": tuple(ks), "radius2s": tuple(radius2s)}


@functools.lru_cache(maxsize=None)
def build():
    cases = []
    # ---- every n at a boundary of the 64-candidate batch and of the list, every k; about four points per cell
    for n in SIZES:
        cases.append(_case(f"n{n}", _uniform(n, 100 + n), max(0.05, (4.0 / n) ** (1.0 / 3.0)), KS))
    # ---- grids
    cases.append(_case("one_cell_300", _uniform(300, 1), 10.0, (1, 10, 64)))                     # 1 x 1 x 1, more than 64 x 4 points in the cell
    line = np.zeros((200, 3))
    line[:, 2] = np.random.default_rng(2).uniform(0, 1, 200)
    cases.append(_case("line_z", line + 3.0, 0.01, (2, 10, 30)))                                   # 1 x 1 x N
    cases.append(_case("line_x", line[:, ::-1] - 2.0, 0.01, (2, 10, 30)))                          # N x 1 x 1
    plane = _uniform(400, 3)
    plane[:, 2] = 0.25
    cases.append(_case("plane_z", plane, 0.05, (10, 50)))                                          # an axis of zero extent
    plane_y = _uniform(400, 4)
    plane_y[:, 1] = -1.0
    cases.append(_case("plane_y", plane_y, 0.05, (10,)))
    plane_x = _uniform(400, 16)
    plane_x[:, 0] = 7.5
    cases.append(_case("plane_x", plane_x, 0.05, (10, 50)))                                        # 1 x N x N: no x faces at all
    cases.append(_case("sparse_cells", _uniform(200, 5), 0.02, (10,)))                             # most cells empty, five or more rings
    cases.append(_case("big_cells", _uniform(1500, 6), 0.5, (10, 64)))                             # 2 x 2 x 2 cells of about 190 points
    # two tight clusters at the ends of a line of 2^24 cells: the grid at the cell cap
    u = 2.0 ** -24
    i = np.arange(250, dtype=np.float64)
    cap = np.zeros((500, 3))
    cap[:250, 2] = i * (3 * u)
    cap[250:, 2] = (1.0 - u) - i * (3 * u)
    cases.append(_case("cell_cap", cap, u, (10,)))
    # a cluster at one end of such a line and a lone point at the other, along z and along y: 2^24 rings away, so its search must give the
    # rings up for a scan of the whole cloud (the device's step budget); the cluster's searches must not
    lone = np.zeros((301, 3))
    lone[:300, 2] = np.arange(300, dtype=np.float64) * (3 * u)
    lone[300, 2] = 1.0 - u
    cases.append(_case("cell_cap_lone_z", lone, u, (10,)))
    cases.append(_case("cell_cap_lone_y", lone[:, [0, 2, 1]], u, (10,)))
    # ---- points exactly on cell faces and on the grid's maximum corner; lattices tie at nearly every place
    cases.append(_case("faces_pow2", _lattice(6, 0.25), 0.25, (2, 10, 30)))
    cases.append(_case("faces_tenth", _lattice(6, 0.1), 0.1, (2, 10, 30)))
    cases.append(_case("faces_tenth_offset", _lattice(6, 0.1) + 0.3, 0.1, (10,)))
    cases.append(_case("face_rounding", _face_rounding(0.3, 0.01, (50, 61, 62, 63, 64)), 0.01, (2, 3)))
    cases.append(_case("lattice_s1", _lattice(7, 1.0), 1.0, (1, 2, 10, 30, 50, 64)))
    cases.append(_case("lattice_s2", _lattice(7, 1.0), 2.0, (10, 30)))
    cases.append(_case("lattice_s3_shuffled", _lattice(7, 1.0)[np.random.default_rng(7).permutation(343)], 3.0, (10, 30)))
    # ---- ties at distance 0 and between clusters
    rest = _uniform(60, 8)
    for k in (2, 10):
        for copies in (k + 1, 3 * k):
            pts = np.concatenate([rest[:20], np.repeat(rest[20:21], copies, 0), rest[21:]])
            cases.append(_case(f"identical_{copies}_k{k}", pts, 0.2, (k,)))
    cl = np.round(_uniform(40, 9) * 1024) / 1024                                                    # multiples of 2^-10: the shift below is exact
    cases.append(_case("coincident_clusters", np.concatenate([cl, cl]), 0.2, (2, 10, 50)))
    cases.append(_case("shifted_clusters", np.concatenate([cl, cl + np.array([5.0, 0.0, 0.0])])[np.random.default_rng(10).permutation(80)], 0.2,
                       (2, 10, 50)))
    # ---- a single point 40 rings from a dense cluster: its search ends by covering the grid
    far = np.concatenate([_uniform(300, 11) * np.array([0.2, 1.0, 1.0]), [[10.1, 0.5, 0.5]]])         # the cluster: one cell thick along x
    cases.append(_case("far_outlier", far, 0.25, (10, 30)))
    # the same along y and along z: the faces of a shell that lie outside a thin grid must cost nothing
    cases.append(_case("far_outlier_y", np.concatenate([_uniform(300, 14) * np.array([1.0, 0.2, 1.0]), [[0.5, 10.1, 0.5]]]), 0.25, (10, 30)))
    cases.append(_case("far_outlier_z", np.concatenate([_uniform(300, 15) * np.array([1.0, 1.0, 0.2]), [[0.5, 0.5, 10.1]]]), 0.25, (10, 30)))
    # ---- radii: between two neighbours of point 0, exactly one of its neighbours' d2, and only the point itself
    rad = _uniform(257, 12)
    _, d2 = O.neighbours(rad, 8)
    cases.append(_case("radius", rad, 0.15, (10, 30), (float((d2[0, 3] + d2[0, 4]) / 2), float(d2[0, 3]), float(d2[5, 6]), 0.0, 0.04)))
    # ---- a world frame: magnitude 1e6, spacing 1e-2
    world = 1.0e6 + np.random.default_rng(13).integers(0, 100, (500, 3)).astype(np.float64) * 1.0e-2
    cases.append(_case("world_frame", world, 0.05, (10, 30)))
    cases.append(_case("world_frame_offset", world + np.array([4.0e5, -2.0e6, 3.3e3]), 0.073, (10,)))
    return tuple(cases)


def names():
    return [c["name"] for c in build()]


def by_name(name):
    return next(c for c in build() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def full(name):
    """The 64 brute-force neighbours of a case's cloud: computed once, never changed."""
    idx, d2 = O.neighbours(by_name(name)["points"], 64)
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2


def grid(case):
    """(h_grid [4], dims [3] int32) as the entry points take them."""
    o, dims = O.grid_of(case["points"], case["s"])
    return np.array([o[0], o[1], o[2], case["s"]], np.float64), dims.astype(np.int32)


# ---- clouds for the normals: every neighbourhood a clear surface -------------------------------------------------------------------------
def noisy_plane(n=1500, seed=21):
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-1, 1, (n, 2))
    e1, e2, nrm = np.array([0.8, 0.0, 0.6]), np.array([0.0, 1.0, 0.0]), np.array([-0.6, 0.0, 0.8])
    return uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.normal(0, 0.002, (n, 1)) * nrm + np.array([10.0, -4.0, 2.0])


def sphere_patch(n=1500, seed=22):
    rng = np.random.default_rng(seed)
    th, ph = rng.uniform(0.2, 0.9, n), rng.uniform(0.0, 1.2, n)
    r = 5.0 + rng.normal(0, 0.001, n)
    return np.stack([r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), r * np.cos(th)], 1)
