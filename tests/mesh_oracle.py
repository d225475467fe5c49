"""The numpy restatement of csrc/mesh.hip and csrc/mesh_tri.h: the mesh filters, the convex-hull crop and the uniform mesh sampling of the
reference's `MeshingPoisson`. Every function states one definition in plain numpy, one IEEE float64 operation per numpy
operation (numpy contracts nothing), so the kernels and the host build of mesh_tri.h are compared with it bit for bit. At the end the
definitions stand behind Open3D's names (`geometry`, `io`, `utility`): tools/gen_golden_mesh.py runs the reference's own class over that
stub. THE STUB IS NOT OPEN3D: parity with an Open3D binary is unpinned."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_meshing.npz")
MAX_ITEMS = 2 ** 26
HULL_CHUNK = 512
NAN_KEY = 0x7ff8000000000000
GOLDEN_RATIO = np.uint64(0x9E3779B97F4A7C15)


def f64(a, cols=3):
    return np.ascontiguousarray(a, np.float64).reshape(-1, cols)


def i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1, 3)


# ---- select / compact ---------------------------------------------------------------------------------------------------------------------
def select(V, triangles, vertex_keep=None, merge=None, triangle_keep=None, drop_degenerate=False, drop_unreferenced=False):
    """(vertex_map [V] int32, -1 = dropped; vertex_list int32; triangles_out [., 3] int32; triangle_pos int32)"""
    tri = i32(triangles).astype(np.int64)
    T = len(tri)
    vkeep = np.ones(V, bool) if vertex_keep is None else np.asarray(vertex_keep).astype(bool)
    ok = ((tri >= 0) & (tri < V)).all(1)
    corner = np.where(ok[:, None], tri, 0)
    if merge is not None:
        m = np.asarray(merge, np.int64)
        corner = m[corner] if V else corner
        ok &= ((corner >= 0) & (corner < V)).all(1)
        corner = np.where(ok[:, None], corner, 0)
    keep = ok.copy()
    if triangle_keep is not None:
        keep &= np.asarray(triangle_keep).astype(bool)
    if V:
        keep &= vkeep[corner].all(1)
    if drop_degenerate:
        keep &= (corner[:, 0] != corner[:, 1]) & (corner[:, 1] != corner[:, 2]) & (corner[:, 0] != corner[:, 2])
    ref = np.zeros(V, bool)
    ref[corner[keep].ravel()] = True
    vflag = vkeep & (ref if drop_unreferenced else True)
    vmap = np.where(vflag, np.cumsum(vflag) - 1, -1).astype(np.int32)
    vlist = np.nonzero(vflag)[0].astype(np.int32)
    tri_out = vmap[corner[keep]].astype(np.int32).reshape(-1, 3) if V else np.zeros((0, 3), np.int32)
    return vmap, vlist, tri_out, np.nonzero(keep)[0].astype(np.int32)


# ---- keys ------------------------------------------------------------------------------------------------------------------------------------
def pair_key(hi, lo):
    return ((hi.astype(np.int64).astype(np.uint64) & np.uint64(0xffffffff)) << np.uint64(32) | (lo.astype(np.int64).astype(np.uint64) & np.uint64(0xffffffff))).astype(np.int64)


def triangle_keys(triangles):
    """the index triple rotated to smallest-index-first: (a, b << 32 | c)"""
    t = i32(triangles)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    r0 = (a <= b) & (a <= c)
    r1 = ~r0 & (b <= a) & (b <= c)
    c0 = np.where(r0, a, np.where(r1, b, c))
    c1 = np.where(r0, b, np.where(r1, c, a))
    c2 = np.where(r0, c, np.where(r1, a, b))
    return c0.astype(np.int64), pair_key(c1, c2)


def vertex_keys(vertices):
    v = f64(vertices)
    z = np.where(v == 0.0, 0.0, v)                                   # -0.0 becomes +0.0
    k = np.ascontiguousarray(z).view(np.int64).copy()
    nan = np.isnan(v).any(1)
    k[nan, 0], k[nan, 1], k[nan, 2] = NAN_KEY, np.nonzero(nan)[0], 0
    return k[:, 0].copy(), k[:, 1].copy(), k[:, 2].copy()


def edge_keys(triangles):
    t = i32(triangles)
    u, v = t.ravel(), np.roll(t, -1, axis=1).ravel()
    return pair_key(np.minimum(u, v), np.maximum(u, v))


def first_of_segment(*keys):
    """(first [n] int32: the lowest index with the same keys, keep [n] bool)"""
    n = len(keys[0])
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, bool)
    order = np.lexsort((np.arange(n),) + tuple(reversed(keys)))
    head = np.ones(n, bool)
    head[1:] = np.any([k[order][1:] != k[order][:-1] for k in keys], axis=0)
    first = np.zeros(n, np.int32)
    first[order] = order[np.maximum.accumulate(np.where(head, np.arange(n), 0))]
    return first, first == np.arange(n)


def edge_census(triangles):
    """undirected edges on which more than two triangle sides lie"""
    _, counts = np.unique(edge_keys(triangles), return_counts=True)
    return int((counts > 2).sum())


# ---- areas, allocation, generator, samples ---------------------------------------------------------------------------------------------------
def cross(v0, v1, v2):
    a, b = v1 - v0, v2 - v0
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def norm(n):
    return np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])


def areas(vertices, triangles):
    """0.5 |(v1 - v0) x (v2 - v0)|; 0 when not finite or when an index lies outside [0, V)"""
    v, t = f64(vertices), i32(triangles)
    ok = ((t >= 0) & (t < len(v))).all(1)
    tt = np.where(ok[:, None], t, 0)
    if len(v) == 0:
        return np.zeros(len(t))
    with np.errstate(all="ignore"):
        a = 0.5 * norm(cross(v[tt[:, 0]], v[tt[:, 1]], v[tt[:, 2]]))
    return np.where(ok & np.isfinite(a), a, 0.0)


def sample_table(area, N):
    """(q [T] int64, c [T] int64 inclusive, C, count_end [T] int64 = rint(c / C * N))"""
    area = np.asarray(area, np.float64)
    mx = area.max() if len(area) else 0.0
    q = np.floor(area / mx * 4294967296.0).astype(np.int64) if mx > 0 else np.zeros(len(area), np.int64)
    c = np.cumsum(q)
    C = int(c[-1]) if len(c) else 0
    if C == 0:
        if N > 0:
            raise ValueError("no triangle has an area, nothing can be sampled")
        return q, c, 0, np.zeros(len(area), np.int64)
    return q, c, C, np.rint(c.astype(np.float64) / np.float64(C) * np.float64(N)).astype(np.int64)


def mix64(z):
    z = z.astype(np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniform(seed, i, k):
    """draw k (0 or 1) of sample i: the top 53 bits of mix64(seed + (2 i + 1 + k) g) times 2^-53"""
    i = np.asarray(i).astype(np.uint64)
    z = mix64(np.uint64(seed & (2 ** 64 - 1)) + (np.uint64(2) * i + np.uint64(1 + k)) * GOLDEN_RATIO)
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def weights(seed, n):
    i = np.arange(n)
    r1, r2 = uniform(seed, i, 0), uniform(seed, i, 1)
    s = np.sqrt(r1)
    return np.stack([1.0 - s, s * (1.0 - r2), s * r2], 1)


def blend(w, a0, a1, a2):
    return (w[:, 0:1] * a0 + w[:, 1:2] * a1) + w[:, 2:3] * a2


def sample(vertices, triangles, N, seed=0, colors=None, normals=None):
    """dict: points, colors (None without vertex colours), normals (vertex normals blended, else the triangles' unit normals), triangle"""
    v, t = f64(vertices), i32(triangles)
    _, _, _, count_end = sample_table(areas(v, t), N)
    if N == 0:
        e = np.zeros((0, 3))
        return {"points": e, "colors": None if colors is None else e.copy(), "normals": e.copy(), "triangle": np.zeros(0, np.int32), "count_end": count_end}
    which = np.minimum(np.searchsorted(count_end, np.arange(N), side="right"), len(t) - 1)
    tt = np.clip(t[which], 0, len(v) - 1)
    w = weights(seed, N)
    c0, c1, c2 = tt[:, 0], tt[:, 1], tt[:, 2]
    out = {"points": blend(w, v[c0], v[c1], v[c2]), "colors": None, "triangle": which.astype(np.int32), "count_end": count_end, "weights": w}
    if colors is not None:
        c = f64(colors)
        out["colors"] = blend(w, c[c0], c[c1], c[c2])
    if normals is not None:
        n = f64(normals)
        out["normals"] = blend(w, n[c0], n[c1], n[c2])
    else:
        with np.errstate(all="ignore"):
            cr = cross(v[c0], v[c1], v[c2])
            out["normals"] = cr / norm(cr)[:, None]
    return out


# ---- point in hull ---------------------------------------------------------------------------------------------------------------------------
def hull_facets(points):
    from scipy.spatial import ConvexHull
    return np.ascontiguousarray(ConvexHull(f64(points)).equations, np.float64)


def hull_values(p, facets):
    """max_f (((n_x x + n_y y) + n_z z) + d), running in facet order from -inf; a NaN sticks"""
    p, f = f64(p), f64(facets, 4)
    m = np.full(len(p), -np.inf)
    with np.errstate(all="ignore"):
        for k in range(len(f)):
            v = ((f[k, 0] * p[:, 0] + f[k, 1] * p[:, 1]) + f[k, 2] * p[:, 2]) + f[k, 3]
            m = np.where((v > m) | np.isnan(v), v, m)
    return m


def point_in_hull(p, facets):
    return hull_values(p, facets) <= 0.0


# ---- a mesh, and the operations on it ---------------------------------------------------------------------------------------------------------
class Mesh:
    def __init__(self, vertices=None, triangles=None, colors=None, normals=None):
        self.vertices = f64(vertices if vertices is not None else np.zeros((0, 3)))
        self.triangles = i32(triangles if triangles is not None else np.zeros((0, 3)))
        self.vertex_colors = None if colors is None else f64(colors)
        self.vertex_normals = None if normals is None else f64(normals)

    def _take(self, vlist, tri):
        out = Mesh(self.vertices[vlist], tri, None if self.vertex_colors is None else self.vertex_colors[vlist],
                   None if self.vertex_normals is None else self.vertex_normals[vlist])
        return out

    def _select(self, **kw):
        vmap, vlist, tri, pos = select(len(self.vertices), self.triangles, **kw)
        return self._take(vlist, tri), vlist, pos

    def remove_vertices_by_mask(self, mask):
        return self._select(vertex_keep=~np.asarray(mask).astype(bool))

    def select_by_index(self, idx, cleanup=True):
        keep = np.zeros(len(self.vertices), bool)
        keep[np.asarray(idx, np.int64)] = True
        return self._select(vertex_keep=keep, drop_unreferenced=cleanup)

    def remove_degenerate_triangles(self):
        return self._select(drop_degenerate=True)

    def remove_duplicated_triangles(self):
        _, keep = first_of_segment(*triangle_keys(self.triangles))
        return self._select(triangle_keep=keep)

    def remove_duplicated_vertices(self):
        first, keep = first_of_segment(*vertex_keys(self.vertices))
        return self._select(vertex_keep=keep, merge=first)

    def remove_unreferenced_vertices(self):
        return self._select(drop_unreferenced=True)

    def remove_non_manifold_edges(self):
        """rounds: every edge with more than two live triangles marks its live triangle of smallest area, ties to the lowest index"""
        live = np.ones(len(self.triangles), bool)
        area = areas(self.vertices, self.triangles)
        while True:
            idx = np.nonzero(live)[0]
            keys = edge_keys(self.triangles[idx])
            owner = np.repeat(idx, 3)
            uniq, inv, counts = np.unique(keys, return_inverse=True, return_counts=True)
            crowded = np.nonzero(counts > 2)[0]
            if len(crowded) == 0:
                break
            for e in crowded:
                ts = np.unique(owner[inv == e])
                live[ts[np.lexsort((ts, area[ts]))[0]]] = False
        return self._select(triangle_keep=live)

    def sample_points_uniformly(self, number_of_points, seed=0):
        return sample(self.vertices, self.triangles, number_of_points, seed, self.vertex_colors, self.vertex_normals)
