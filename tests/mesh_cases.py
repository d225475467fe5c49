"""The case list tests/test_mesh_cpu.py (host build of csrc/mesh_tri.h) and tests/test_gpu_mesh.py (csrc/mesh.hip on a device) share: the
smallest meshes, hulls and sample counts at which a path of the kernels can go wrong. Every case is a dict: vertices [V, 3], triangles
[T, 3] int32, colors / normals [V, 3] or None, mask [V] bool (the vertices `remove_vertices_by_mask` drops), index (the vertices
`select_by_index` keeps), samples (the N to draw). Expected values come from tests/mesh_oracle.py alone."""
import functools

import numpy as np

import mesh_oracle as O

NAN, INF = float("nan"), float("inf")


def _case(name, vertices, triangles, colors=False, normals=False, mask=None, index=None, samples=(0, 1, 65), seed=7):
    v, t = O.f64(vertices), O.i32(triangles)
    rng = np.random.default_rng(len(v) * 131 + len(t))
    V = len(v)
    return {"name": name, "vertices": v, "triangles": t, "colors": rng.uniform(0, 1, (V, 3)) if colors else None,
            "normals": rng.normal(0, 1, (V, 3)) if normals else None,
            "mask": rng.uniform(0, 1, V) < 0.3 if mask is None else np.asarray(mask, bool),
            "index": rng.permutation(V)[:max(0, (2 * V) // 3)] if index is None else np.asarray(index, np.int64), "samples": tuple(samples), "seed": seed}


def strip(T, seed=0):
    """T triangles over T + 2 vertices of a zig-zag strip with rough heights, orientation alternating so that all face one way"""
    rng = np.random.default_rng(seed + T)
    k = np.arange(T + 2)
    v = np.stack([0.5 * (k // 2) + 0.1 * rng.uniform(-1, 1, T + 2), (k % 2) + 0.1 * rng.uniform(-1, 1, T + 2), rng.uniform(0, 0.5, T + 2)], 1)
    i = np.arange(T)
    t = np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], 1), np.stack([i + 1, i, i + 2], 1))
    return v, t


def height_field(nx, ny, seed=0):
    """(nx + 1)(ny + 1) vertices, 2 nx ny triangles"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64), indexing="ij")
    z = np.sin(x / 3.0) + 0.5 * np.cos(y / 2.0) + 0.05 * rng.normal(0, 1, x.shape)
    v = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    a = (np.arange(nx)[:, None] * (ny + 1) + np.arange(ny)[None]).ravel()
    t = np.concatenate([np.stack([a, a + ny + 1, a + 1], 1), np.stack([a + 1, a + ny + 1, a + ny + 2], 1)])
    return v, t


SPECIAL_V = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0.5), (-0.0, 0.0, -0.0), (1, 0, 0), (NAN, 0, 0), (NAN, 0, 0), (2, 2, INF), (1, 0, 0), (3, 0, 0),
             (3, 1, 0), (0, 0, 0)]
SPECIAL_T = [(0, 1, 2), (1, 2, 0), (2, 1, 0), (1, 3, 2), (4, 5, 2), (0, 0, 1), (6, 1, 2), (1, 8, 3), (1, 10, 11), (3, 3, 3), (10, 11, 1), (12, 9, 2), (0, 1, 2)]


def fan(apexes, equal_areas=False):
    """`apexes` triangles on the edge (0, 1)"""
    square = [(0.5, 1.0, 0.0), (0.5, 0.0, 1.0), (0.5, -1.0, 0.0), (0.5, 0.0, -1.0)]                 # four triangles of area exactly 0.5
    v = [(0, 0, 0), (1, 0, 0)] + [square[k % 4] if equal_areas else (0.5, (1.0 + 0.25 * ((k * 5) % 7)) * np.cos(k), (1.0 + 0.25 * ((k * 5) % 7)) * np.sin(k))
                                  for k in range(apexes)]
    return v, [(0, 1, 2 + k) for k in range(apexes)]


@functools.lru_cache(maxsize=None)
def cases():
    out = [
        _case("v0_t0", np.zeros((0, 3)), np.zeros((0, 3)), samples=(0,)),
        _case("v1_t0", [(1, 2, 3)], np.zeros((0, 3)), samples=(0,)),
        _case("v2_t0", [(1, 2, 3), (1, 2, 3)], np.zeros((0, 3)), samples=(0,)),
        _case("v3_t1", [(0, 0, 0), (2, 0, 0), (0, 2, 0)], [(0, 1, 2)], colors=True, samples=(0, 1, 63, 64, 65, 257)),
        _case("v4_t2", [(0, 0, 0), (2, 0, 0), (0, 2, 0), (2, 2, 1)], [(0, 1, 2), (2, 1, 3)], normals=True, samples=(0, 1, 64)),
        _case("special", SPECIAL_V, SPECIAL_T, colors=True, normals=True, mask=[0] * 13, samples=(0, 1, 5, 257)),
        _case("special_plain", SPECIAL_V, SPECIAL_T, samples=(3, 65)),
        _case("fan_3", *fan(3), mask=[0] * 5, samples=(2,)),
        _case("fan_4", *fan(4), mask=[0] * 6, samples=(2,)),
        _case("fan_4_equal_areas", *fan(4, True), mask=[0] * 6, samples=(2,)),
        _case("two_fans", fan(4)[0] + [(5, 5, 5), (6, 5, 5), (5, 6, 5), (5, 5, 6), (6, 6, 6)], fan(4)[1] + [(6, 7, 8), (6, 7, 9), (7, 6, 10), (0, 1, 6)], mask=[0] * 11, samples=(9,)),
    ]
    for T in (253, 254, 255, 256, 257):
        out.append(_case(f"strip_{T}", *strip(T), colors=T % 2 == 0, normals=T % 2 == 1, samples=(T - 1, T, T + 1, 2 * T + 1)))
    for T in (65535, 65537):
        out.append(_case(f"strip_{T}", *strip(T), colors=True, samples=(257, 65537)))
    v, t = strip(300)
    out.append(_case("mask_keeps_nothing", v, t, mask=np.ones(len(v), bool), index=[], samples=(10,)))
    out.append(_case("mask_keeps_all", v, t, mask=np.zeros(len(v), bool), index=np.arange(len(v)), samples=(10,)))
    out.append(_case("select_with_duplicates", v, t, index=np.concatenate([np.arange(200)[::-1], np.arange(50, 120)]), samples=(10,)))
    # duplicates that cross the scan block and sit at the first and last positions
    v, t = height_field(20, 15, 3)
    dv = np.concatenate([v[-1:], v, v[:40], v[:1]])
    dt = np.concatenate([t[-1:] + 1, t + 1, t[:30, [1, 2, 0]] + 1, t[:20, [0, 2, 1]] + 1, t[:1] + 1])
    out.append(_case("field_with_duplicates", dv, dt, colors=True, samples=(300, 1001)))
    # zero-area and non-finite triangles between valid ones, N < T
    v, t = strip(40, 9)
    v[10], v[20] = v[9], (NAN, 0, 0)
    v[30, 2] = 1e308
    v[31, 2] = -1e308
    out.append(_case("bad_triangles_between", v, t, samples=(7, 39, 41, 500), mask=[0] * 42))
    out.append(_case("wrong_indices", strip(20)[0], np.concatenate([strip(20)[1][:10], [(-1, 0, 1), (0, 22, 1), (2 ** 31 - 1, 1, 2), (0, 1, -2 ** 31)], strip(20)[1][10:]]),
                     colors=True, samples=(50,), mask=[0] * 22))
    return tuple(out)


def names():
    return [c["name"] for c in cases()]


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def mesh_of(case):
    return O.Mesh(case["vertices"], case["triangles"], case["colors"], case["normals"])


# ---- hulls -------------------------------------------------------------------------------------------------------------------------------------
def tangent_facets(F, seed=1):
    """F half-spaces n . p - 1 <= 0 with unit normals: the planes tangent to the unit sphere; the first four are a tetrahedron's, so the set
    is bounded from F = 4 on"""
    rng = np.random.default_rng(seed)
    n = rng.normal(0, 1, (F, 3))
    n[:4] = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.float64)
    n /= np.linalg.norm(n, axis=1)[:, None]
    return np.ascontiguousarray(np.concatenate([n, -np.ones((F, 1))], 1))


def sphere_points(n, seed=2):
    p = np.random.default_rng(seed).normal(0, 1, (n, 3))
    return p / np.linalg.norm(p, axis=1)[:, None]


def hull_queries(facets, hull_points=None, n=700, seed=3):
    """random points around the hull, and points on facets (the foot of the origin on the plane), on hull vertices and one ulp either side, a
    NaN, an infinity and the origin"""
    rng = np.random.default_rng(seed)
    f = O.f64(facets, 4)
    feet = -f[:, :3] * f[:, 3:4]                                     # n . p + d = 0 for unit n
    on = feet[:: max(1, len(feet) // 40)]
    pts = [rng.normal(0, 0.8, (n, 3)), on, np.nextafter(on, 0.0), np.nextafter(on, on * 2), [(NAN, 0, 0), (0, INF, 0), (0, 0, 0), (0, 0, NAN), (-INF, 0, 0)]]
    if hull_points is not None:
        h = O.f64(hull_points)[:: max(1, len(hull_points) // 40)]
        pts += [h, np.nextafter(h, 0.0), np.nextafter(h, h * 2)]
    return np.ascontiguousarray(np.concatenate([O.f64(p) for p in pts]))


HULL_FACETS = (4, 5, O.HULL_CHUNK - 1, O.HULL_CHUNK, O.HULL_CHUNK + 1, 2 * O.HULL_CHUNK + 1)
