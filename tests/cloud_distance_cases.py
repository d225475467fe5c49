"""The target clouds, queries, normals, radii and cell sizes at which the cross-cloud kernels can go wrong, shared by
tests/test_cloud_distance_cpu.py (a host build of csrc/cyl_point.h) and tests/test_gpu_cloud_distance.py (the kernels): the smallest
shapes at every boundary between two code paths. Every case is a dict: name, points [n, 3] (the target), queries [m, 3], normals [m, 3],
s (cell size of the grid the device test bins with), ks and radius2s (cross k-NN), r (cross ball), rho and L (cylinders); all arrays
float64 and read-only. The restatement of a case (tests/cloud_distance_oracle.py) is computed once and shared."""
import functools

import numpy as np

import ball_cases as BC
import cloud_distance_oracle as O
import knn_oracle as K

WORLD = np.array([4.0e5, 5.0e6, 2.0e3])
MIN_POINTS, REG_ERROR = 5, 0.01


def _uniform(n, seed, lo=0.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3))


def _unit(m, seed):
    v = np.random.default_rng(seed).normal(0.0, 1.0, (m, 3))
    return v / np.sqrt(((v[:, 0] * v[:, 0]) + (v[:, 1] * v[:, 1])) + (v[:, 2] * v[:, 2]))[:, None]


def _case(name, points, queries, normals=None, s=0.25, ks=(1, 8), radius2s=(np.inf,), r=0.4, rho=0.25, L=0.5):
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    q = np.ascontiguousarray(queries, np.float64).reshape(-1, 3)
    nr = _unit(len(q), len(q) + len(p)) if normals is None else np.ascontiguousarray(np.broadcast_to(np.asarray(normals, np.float64), q.shape))
    for a in (p, q, nr):
        a.setflags(write=False)
    return {"name": name, "points": p, "queries": q, "normals": nr, "s": float(s), "ks": tuple(ks), "radius2s": tuple(radius2s),
            "r": float(r), "rho": float(rho), "L": float(L)}


def _around_box(p):
    """One query just outside each face of the target's box, at the centre of the face, and the eight corners pushed out by one ulp."""
    lo, hi, mid = p.min(0), p.max(0), (p.min(0) + p.max(0)) / 2.0
    out = []
    for a in range(3):
        for edge, to in ((lo, -np.inf), (hi, np.inf)):
            q = mid.copy()
            q[a] = np.nextafter(edge[a], to)
            out.append(q)
    return np.array(out)


def _far(p, s):
    """Queries 10^3 and 10^7 cells away from the target's box along every axis, to either side, and along the diagonal."""
    lo, hi, mid = p.min(0), p.max(0), (p.min(0) + p.max(0)) / 2.0
    out = []
    for cells in (1.0e3, 1.0e7):
        for a in range(3):
            for edge, sign in ((lo, -1.0), (hi, 1.0)):
                q = mid.copy()
                q[a] = edge[a] + sign * cells * s
                out.append(q)
        out.append(hi + cells * s)
    return np.array(out)


@functools.lru_cache(maxsize=None)
def build():
    cases = []
    # ---- every target size at a boundary of the 64-candidate batch, queries inside and outside the grid; k = 64 exceeds n for the small ones.
    # n = 0 and m = 0 are covered by the device test's own calls
    for n in (1, 2, 63, 64, 65, 129):
        p = _uniform(n, 300 + n)
        cases.append(_case(f"n{n}", p, _uniform(40, 400 + n, -0.3, 1.3), ks=(1, 64), radius2s=(np.inf, 0.09, 1.0e-12) if n == 129 else (np.inf,)))
    # ---- a lattice whose points sit on cell faces: queries on faces, coincident with target points, just outside every face of the box
    lat = BC._lattice(6, 0.25)
    on_faces = lat[::7] + np.array([0.125, 0.0, 0.0])
    cases.append(_case("cell_faces", lat, np.concatenate([on_faces, lat[::11], _around_box(lat)]), s=0.25, ks=(1, 7), r=0.5))
    # ---- coincident target points: ties go to the lower index; queries coincident with them and elsewhere
    cl = np.round(_uniform(40, 3) * 1024) / 1024
    cases.append(_case("coincident", np.concatenate([cl, cl, np.repeat(cl[:1] + 2.0, 5, 0)]), np.concatenate([cl[:10], cl[:1] + 2.0, _uniform(10, 4)]),
                       ks=(1, 5), radius2s=(np.inf, 0.0)))
    # ---- queries 10^3 and 10^7 cells away
    p = _uniform(129, 5)
    cases.append(_case("far_queries", p, np.concatenate([_far(p, 0.1), _uniform(5, 6)]), s=0.1, ks=(1, 64)))
    # ---- an N x 1 x 1 grid of 5001 cells with 65 points: a search for 64 of them walks most of the line, more steps than the whole cloud
    # costs, from inside and from 10^3 and 10^7 cells away
    line = np.zeros((65, 3))
    line[:, 0] = np.sort(np.random.default_rng(7).uniform(0.0, 50.0, 65))
    line[0, 0], line[-1, 0] = 0.0, 50.0
    lq = np.array([[25.0, 0, 0], [0.0, 0, 0], [-10.0, 0, 0], [-1.0e5, 0, 0], [60.0, 0, 0], [50.0 + 1.0e5, 0, 0], [25.0, 3.0, -2.0]])
    cases.append(_case("line_x", line, lq, s=0.01, ks=(1, 64), r=0.8, rho=0.5, L=4.0, normals=(1.0, 0.0, 0.0)))
    # ---- a 1 x N x N grid at three cell sizes; at the finest the boxes of the ball and of the cylinder hold more rows than the budget allows
    plane = _uniform(129, 8)
    plane[:, 0] = 7.5
    pq = np.concatenate([plane[:6] + np.array([0.0, 0.01, -0.01]), _uniform(6, 9) + np.array([7.0, 0.0, 0.0])])
    for tag, s in (("coarse", 0.25), ("mid", 0.02), ("fine", 0.001)):
        cases.append(_case(f"plane_x_{tag}", plane, pq, s=s, ks=(1, 8), r=0.2, rho=0.2, L=0.3))
    # ---- a far outlier stretches the grid (1 x 10001 x 500 cells): boxes inside the slab are given up, boxes the grid's edge clips are not
    far = BC.by_name("far_outlier_y")["points"]
    cases.append(_case("far_outlier_y", far, np.concatenate([far[:8], far[-1:], far[-1:] + np.array([0.0, 1.0, 0.0])]), s=0.002, ks=(1, 4), r=0.3,
                       rho=0.3, L=0.3))
    # ---- one cell
    cases.append(_case("one_cell", _uniform(200, 10), _uniform(30, 11, -0.5, 1.5), s=10.0, ks=(1, 64)))
    # ---- a world frame: magnitude 5e6, a noisy front and queries off it
    front = BC.front(1500, origin=tuple(WORLD))
    cases.append(_case("world_frame", front, BC.front(60, seed=32, origin=tuple(WORLD)) + np.array([0.05, 0.0, 0.02]), s=0.5, ks=(1, 8), r=0.5,
                       rho=0.25, L=1.0))
    # ---- about 1000 queries against about 5000 points
    big = BC.front(5000, seed=33, origin=tuple(WORLD))
    cases.append(_case("front_1000", big, BC.front(1000, seed=34, origin=tuple(WORLD)), s=0.4, ks=(8,), r=0.3, rho=0.2, L=0.8))
    # ---- about 5000 points in one cylinder, a ball that holds the whole cloud, an empty cylinder
    cube = _uniform(5200, 12)
    cases.append(_case("whole_cloud", cube, np.array([[0.5, 0.5, 0.5], [0.25, 0.5, 0.75], [40.0, 0.5, 0.5]]), s=0.5, ks=(64,), r=2.0, rho=2.0, L=2.0))
    # ---- cylinders in powers of two, every value exact: the cap (|t| == L) and the wall (rad2 == rho^2) are inside, their nextafter
    # neighbours outside; along each axis, and the same points under an oblique normal that is no unit vector. The copy at +100 rounds the
    # nextafter neighbours onto the cap and the wall: there they are inside
    up, out = np.nextafter(1.0, 2.0), np.nextafter(0.25, 1.0)
    shape = np.array([[0, 0, 1.0], [0, 0, -1.0], [0, 0, up], [0, 0, -up], [0.25, 0, 0.5], [0, -0.25, -0.5], [0.25, 0, 0], [out, 0, 0], [0, -out, 0],
                      [0.125, 0.125, 0.25], [0, 0, 0], [0.25, 0.25, 0.0]])
    for axis in range(3):
        perm = [(axis + 1) % 3, (axis + 2) % 3, axis]                       # the cylinder's axis becomes `axis`
        pts = np.zeros_like(shape)
        pts[:, perm] = shape
        nrm = np.zeros(3)
        nrm[axis] = 1.0
        qs = np.array([[0.0, 0.0, 0.0], [100.0, 100.0, 100.0]])
        cases.append(_case(f"exact_axis{axis}", np.concatenate([pts, pts + 100.0]), qs, normals=nrm, s=0.5, ks=(1,), r=1.0, rho=0.25, L=1.0))
    cases.append(_case("exact_oblique", shape, np.zeros((3, 3)), normals=np.array([[0.5, 0.5, 0.5], [0.6, 0.8, 0.0], [0.0, -1.0, 0.0]]), s=0.5, ks=(1,),
                       r=1.0, rho=0.25, L=1.0))
    # ---- L = 64 rho along an oblique unit normal through a cube of points
    cases.append(_case("long_thin", _uniform(3000, 13), _uniform(12, 14, 0.3, 0.7), s=1.0 / 16, ks=(1,), r=0.1, rho=1.0 / 64, L=1.0))
    # ---- a NaN normal, a zero normal, an infinite one, a NaN query; counts 0, 1, 2 and min_points - 1 for the NaN rules of std and lod
    col = np.array([[0, 0, 0], [0, 0, 0.25], [0, 0, 0.5], [0, 0, 0.75], [5.0, 0, 0], [5.0, 0, 0.25], [10.0, 0, 0], [0, 0, -0.25], [0, 0, -0.5]])
    cq = np.array([[0, 0, 0.5], [5.0, 0, 0], [10.0, 0, 0], [20.0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]])
    cn = np.array([[0, 0, 1.0]] * 4 + [[0, 0, 1.0], [np.nan, 0, 1.0], [0, 0, 0.0], [0, np.inf, 0.0], [0, 0, 1.0], [0, 0, 1.0]])
    cases.append(_case("few_points", col, cq, normals=cn, s=0.5, ks=(1, 3), r=0.6, rho=0.25, L=0.5))
    return tuple(cases)


def names():
    return [c["name"] for c in build()]


def by_name(name):
    return next(c for c in build() if c["name"] == name)


def _frozen(out):
    for v in out.values() if isinstance(out, dict) else out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_knn(name, k, radius2):
    c = by_name(name)
    return _frozen(O.knn_cross(c["queries"], c["points"], k, radius2))


@functools.lru_cache(maxsize=None)
def expected_rings(name, k, radius2):
    c = by_name(name)
    return _frozen((O.knn_rings(c["queries"], c["points"], c["s"], k, radius2),))[0]


@functools.lru_cache(maxsize=None)
def expected_ball(name):
    c = by_name(name)
    return _frozen(O.ball_cross(c["queries"], c["points"], c["r"]))


@functools.lru_cache(maxsize=None)
def expected_ball_walk(name):
    c = by_name(name)
    return O.ball_walk(c["queries"], c["points"], c["s"], c["r"])


@functools.lru_cache(maxsize=None)
def expected_cyl(name):
    c = by_name(name)
    return _frozen(O.cylinder_stats(c["queries"], c["normals"], c["points"], c["rho"], c["L"]))


@functools.lru_cache(maxsize=None)
def expected_cyl_walk(name):
    c = by_name(name)
    return O.cyl_walk(c["queries"], c["normals"], c["points"], c["s"], c["rho"], c["L"])


@functools.lru_cache(maxsize=None)
def finish_inputs():
    """The counts and sums of every cylinder of every case with L = 1 as cloud 1, the same rolled by one as cloud 2: every pairing of the
    counts 0, 1, 2, min_points - 1 and more that the list holds next to one another."""
    L = 1.0
    cs = [expected_cyl(c["name"]) for c in build() if c["L"] == L]
    count, sums = np.concatenate([c["count"] for c in cs]), np.concatenate([c["sums"] for c in cs])
    extra_c = np.array([0, 1, 2, 4, 5, 5, 4, 1], np.int32)                   # by hand: the NaN rules next to one another
    extra_s = np.array([[0, 0], [7, 49], [10, 52], [8, 30], [-20, 100], [1000, 200050], [9, 40], [-3, 9]], np.int64)
    count1, sums1 = np.concatenate([count, extra_c]), np.concatenate([sums, extra_s])
    out = {"count1": count1, "sums1": sums1, "count2": np.roll(count1, 1), "sums2": np.roll(sums1, 1, axis=0)}
    return L, _frozen(out)


@functools.lru_cache(maxsize=None)
def expected_finish():
    L, f = finish_inputs()
    return _frozen(O.m3c2_finish(f["count1"], f["sums1"], f["count2"], f["sums2"], L, REG_ERROR, MIN_POINTS))


def grid(case):
    """(h_grid [4], dims [3] int32) of the target, as the entry points take them."""
    o, dims = K.grid_of(case["points"], case["s"])
    return np.array([o[0], o[1], o[2], case["s"]], np.float64), dims.astype(np.int32)
