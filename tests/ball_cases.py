"""The clouds, radii and cell sizes at which the ball features can go wrong, shared by tests/test_ballfeat_cpu.py (a host build of
csrc/ball_point.h) and tests/test_gpu_ballfeat.py (the kernel): the smallest shapes at every boundary between two code paths.
Every case is a dict: name, points [n, 3] float64 (read-only), r (radius), s (cell size of the grid the device test bins with).
The restatement of a case (tests/ball_oracle.py) is computed once and shared."""
import functools

import numpy as np

import ball_oracle as B
import knn_oracle as K


def _uniform(n, seed, scale=1.0):
    return np.random.default_rng(seed).uniform(0.0, scale, (n, 3))


def _lattice(m, step):
    g = np.arange(m, dtype=np.float64) * step
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def _case(name, points, r, s=None):
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    p.setflags(write=False)
    return {"name": name, "points": p, "r": float(r), "s": float(r) / 2.0 if s is None else float(s)}


def front(n=4000, seed=31, size=(6.0, 3.0), origin=(416000.0, 5091000.0, 1800.0)):
    """A synthetic glacier front in a world frame: a steep noisy surface with a sharp top edge (a plateau above a wall), x across the
    front, y along it."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0.0, size[0], n), rng.uniform(0.0, size[1], n)
    wall = u < 0.6 * size[0]
    x = np.where(wall, 0.15 * u, 0.15 * 0.6 * size[0] + (u - 0.6 * size[0]))
    z = np.where(wall, u, 0.6 * size[0] + 0.05 * (u - 0.6 * size[0]))
    pts = np.column_stack([x + 0.1 * np.sin(v), v, z]) + rng.normal(0.0, 0.01, (n, 3))
    return pts + np.asarray(origin)


@functools.lru_cache(maxsize=None)
def build():
    cases = []
    # ---- every n at a boundary of the 64-candidate batch; n = 0 is covered by the device test's own call
    for n in (1, 2, 3, 63, 64, 65, 129):
        cases.append(_case(f"n{n}", _uniform(n, 200 + n), 0.4))
    # ---- radii: the whole cloud in every ball; only the query in every ball
    cases.append(_case("whole_cloud", _uniform(300, 1), 2.0, 0.3))
    cases.append(_case("only_query", _uniform(300, 2), 1e-4, 0.05))
    # ---- coincident points: a ball of identical points has no extent (NaN), next to balls that have some
    cl = np.round(_uniform(40, 3) * 1024) / 1024
    cases.append(_case("coincident", np.concatenate([cl, cl, np.repeat(cl[:1] + 7.0, 5, 0)]), 0.25))
    # ---- an integer lattice with r = 5: d2 = 25 exactly for (3, 4, 0), (5, 0, 0), ...: the boundary is kept
    cases.append(_case("lattice_r5", _lattice(9, 1.0), 5.0, 2.0))
    # ---- points at exactly +-r along each axis: |i| = 2^18; one just beyond and one just inside
    r = 2.0
    axis = np.array([[0, 0, 0], [r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0], [0, 0, r], [0, 0, -r],
                     [np.nextafter(r, 3.0), 0, 0], [0, np.nextafter(r, 0.0), 0], [0.3, 0.2, 0.1]], np.float64)
    cases.append(_case("exact_radius", axis, r, 1.0))
    cases.append(_case("exact_radius_offset", axis * 0.15 / 2.0 + np.array([100.0, -50.0, 25.0]), 0.15, 0.1))
    # ---- one cell of about 700 points (eleven batches per lane), and a ball of about 5000 (several batches per lane in every row)
    cases.append(_case("one_cell_700", _uniform(700, 4), 0.3, 10.0))
    cases.append(_case("ball_5000", _uniform(5200, 5), 1.6, 0.5))
    # ---- degenerate grids
    plane = _uniform(400, 6)
    plane[:, 0] = 7.5
    cases.append(_case("plane_x", plane, 0.1, 0.04))                     # 1 x N x N
    line = np.zeros((200, 3))
    line[:, 0] = np.random.default_rng(7).uniform(0, 1, 200)
    cases.append(_case("line_x", line - 2.0, 0.05, 0.01))                # N x 1 x 1: every ball a line, l2 = l3 = 0
    # ---- a far outlier along each axis stretches the grid. Along y and z the box of a query holds more rows than the step budget allows
    # and the query scans the whole cloud (steps < 0) unless the grid's edge clips its box; along x the rows stay few and no query gives up
    slab = _uniform(300, 8) * np.array([0.0015, 1.0, 1.0])                # one cell thick: 1 x 10001 x 500 cells with the outlier
    far = np.concatenate([slab, [[0.001, 20.0, 0.5]]])
    cases.append(_case("far_outlier_y", far, 0.3, 0.002))
    cases.append(_case("far_outlier_z", far[:, [0, 2, 1]], 0.3, 0.002))
    flat = slab[:, [1, 2, 0]] * np.array([1.0, 1.0, 0.0])
    cases.append(_case("far_outlier_x", np.concatenate([flat, [[20.0, 0.5, 0.0]]]), 0.3, 0.002))
    # ---- a world frame: magnitude 5e6, spacing 1e-2
    world = np.random.default_rng(9).integers(0, 60, (600, 3)).astype(np.float64) * 1.0e-2 + 5.0e6
    cases.append(_case("world_frame", world, 0.15))
    # ---- points on cell faces
    cases.append(_case("cell_faces", _lattice(6, 0.25), 0.5, 0.25))
    cases.append(_case("cell_faces_tenth", _lattice(6, 0.1) + 0.3, 0.25, 0.1))
    return tuple(cases)


def names():
    return [c["name"] for c in build()]


def by_name(name):
    return next(c for c in build() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement of a case: computed once, never changed."""
    c = by_name(name)
    out = B.ball_features(c["points"], c["r"])
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_walk(name):
    c = by_name(name)
    return B.walk(c["points"], c["s"], c["r"])


def grid(case):
    """(h_grid [4], dims [3] int32) as the entry points take them."""
    o, dims = K.grid_of(case["points"], case["s"])
    return np.array([o[0], o[1], o[2], case["s"]], np.float64), dims.astype(np.int32)
