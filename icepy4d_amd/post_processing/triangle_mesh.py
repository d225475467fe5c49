"""Triangle meshes on the device, with Open3D's names: `TriangleMesh.remove_vertices_by_mask`, `remove_degenerate_triangles`,
`remove_duplicated_triangles`, `remove_duplicated_vertices`, `remove_unreferenced_vertices`, `remove_non_manifold_edges`,
`select_by_index`, `sample_points_uniformly`, and `point_in_hull` / `compute_convex_hull` of the reference's `MeshingPoisson`.
csrc/mesh.hip does the work (`im_mesh_*`, torch's stable sort between the calls). No CPU fallback: without a HIP device the
operations raise. Open3D is not imported. Two things run on the host: qhull (`scipy.spatial.ConvexHull`, as for `build_dsm`) gives a
hull's vertices and facets, and the rounds of `remove_non_manifold_edges` when the device census finds an edge with more than two
triangles, which an iso-surface with vertices removed does not have.

The definitions (tests/mesh_oracle.py, bit-identical): float64 attributes, int32 triangles; outputs keep input order, kept
vertices in ascending old index, kept triangles in their old order. A triangle with an index outside [0, V) is dropped by every filter
and has area 0. PARITY WITH AN OPEN3D BINARY IS UNPINNED, for every operation; the sampler cannot match it: Open3D draws the barycentric
pair from a Mersenne Twister, here it is a counter-based function of (seed, sample index)."""
from pathlib import Path

import numpy as np
import torch

from .._lib import load, ptr
from ..core.point_cloud import _PLY_TYPES, PointCloud
from ..engine import default_engine, to_device

MAX_FACETS = 2 ** 22


def max_items() -> int:
    """The most vertices, triangles or samples one device call takes."""
    return int(load().im_mesh_max_items())


def _check_counts(*counts):
    for c in counts:
        if c > 2 ** 26:
            raise ValueError(f"{c} items: a mesh call takes at most 2^26 vertices, triangles or samples")


# ---- device passes over torch tensors ----------------------------------------------------------------------------------------------------------
def device_select(eng, V, d_tri, vertex_keep=None, merge=None, triangle_keep=None, drop_degenerate=False, drop_unreferenced=False):
    """`im_mesh_select`: (vertex_map [V] int32, vertex_list [nv] int32, triangles [nt, 3] int32, triangle_pos [nt] int32), device tensors."""
    dev, T = eng.device, int(d_tri.shape[0])
    vmap, vlist = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
    tri_out, tri_pos = torch.empty((T, 3), dtype=torch.int32, device=dev), torch.empty(T, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    eng.ctx.call("im_mesh_select", ptr(vertex_keep), V, ptr(d_tri), T, ptr(merge), ptr(triangle_keep), int(drop_degenerate), int(drop_unreferenced),
                 ptr(vmap), ptr(vlist), ptr(tri_out), ptr(tri_pos), ptr(counts), eng.stream_ptr())
    nv, nt = (int(c) for c in counts.cpu())
    return vmap, vlist[:nv], tri_out[:nt], tri_pos[:nt]


def sort_keys(keys):
    """The permutation (sorted position -> item) of successive stable sorts, the last key first: torch's sort, plumbing."""
    perm = None
    for k in reversed(keys):
        if perm is None:
            _, perm = torch.sort(k, stable=True)
        else:
            _, p = torch.sort(k[perm], stable=True)
            perm = perm[p]
    return perm


def device_first_of_segment(eng, keys):
    """`im_mesh_first_of_segment` behind the sorts: (first [n] int32, keep [n] uint8)."""
    n, dev = int(keys[0].shape[0]), eng.device
    first, keep = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    if n:
        perm = sort_keys(keys)
        k = list(keys) + [None] * (3 - len(keys))
        eng.ctx.call("im_mesh_first_of_segment", n, ptr(k[0]), ptr(k[1]), ptr(k[2]), ptr(perm), ptr(first), ptr(keep), eng.stream_ptr())
    return first, keep


def device_triangle_keys(eng, d_tri):
    T = int(d_tri.shape[0])
    k0, k1 = (torch.empty(T, dtype=torch.int64, device=eng.device) for _ in range(2))
    eng.ctx.call("im_mesh_triangle_keys", ptr(d_tri), T, ptr(k0), ptr(k1), eng.stream_ptr())
    return k0, k1


def device_vertex_keys(eng, d_vert):
    V = int(d_vert.shape[0])
    k = [torch.empty(V, dtype=torch.int64, device=eng.device) for _ in range(3)]
    eng.ctx.call("im_mesh_vertex_keys", ptr(d_vert), V, ptr(k[0]), ptr(k[1]), ptr(k[2]), eng.stream_ptr())
    return k


def device_edge_census(eng, d_tri) -> int:
    """The undirected edges on which more than two triangle sides lie."""
    T = int(d_tri.shape[0])
    if T == 0:
        return 0
    keys = torch.empty(3 * T, dtype=torch.int64, device=eng.device)
    eng.ctx.call("im_mesh_edge_keys", ptr(d_tri), T, ptr(keys), eng.stream_ptr())
    skeys, _ = torch.sort(keys)
    count = torch.empty(1, dtype=torch.int64, device=eng.device)
    eng.ctx.call("im_mesh_edge_census", ptr(skeys), 3 * T, ptr(count), eng.stream_ptr())
    return int(count.cpu()[0])


def hull_facets(hull_points) -> np.ndarray:
    """[F, 4] float64: n_x, n_y, n_z, d of the facets of the convex hull of `hull_points`, qhull's on the host."""
    from scipy.spatial import ConvexHull
    facets = np.ascontiguousarray(ConvexHull(np.asarray(hull_points, np.float64).reshape(-1, 3)).equations, np.float64)
    if not np.isfinite(facets).all():
        raise ValueError("the hull has non-finite facets")
    if len(facets) > MAX_FACETS:
        raise ValueError(f"a hull of {len(facets)} facets: at most 2^22")
    return facets


def compute_convex_hull(pcd_or_points) -> np.ndarray:
    """The vertices [H, 3] of the convex hull of a cloud, in ascending point index, through scipy on the host."""
    from scipy.spatial import ConvexHull
    pts = pcd_or_points.points if isinstance(pcd_or_points, PointCloud) else np.asarray(pcd_or_points, np.float64).reshape(-1, 3)
    return pts[np.sort(ConvexHull(pts).vertices)].copy()


def device_in_hull(eng, d_pts, facets):
    n = int(d_pts.shape[0])
    inside = torch.empty(n, dtype=torch.uint8, device=eng.device)
    facets = np.ascontiguousarray(facets, np.float64).reshape(-1, 4)
    eng.ctx.call("im_mesh_in_hull", ptr(d_pts), n, facets.ctypes.data, len(facets), ptr(inside), eng.stream_ptr())
    return inside


def point_in_hull(p, hull_points=None, facets=None, engine=None) -> np.ndarray:
    """[n] bool: max_f (n_f . p + d_f) <= 0 over the facets of the hull of `hull_points` (or `facets` [F, 4] as given), on the device. A
    point with a NaN coordinate is outside. The reference's `Delaunay(hull).find_simplex(p) >= 0` is the same set away from the boundary."""
    p = np.asarray(p, np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"points must be [n, 3] (got {p.shape})")
    if facets is None:
        if hull_points is None:
            raise ValueError("a hull needs hull_points or facets")
        facets = hull_facets(hull_points)
    facets = np.ascontiguousarray(facets, np.float64).reshape(-1, 4)
    if len(facets) == 0 or len(facets) > MAX_FACETS or not np.isfinite(facets).all():
        raise ValueError("a hull has 1..2^22 finite facets")
    _check_counts(len(p))
    if len(p) == 0:
        return np.zeros(0, bool)
    eng = default_engine(engine)
    return device_in_hull(eng, to_device(p, eng.device, np.float64), facets).cpu().numpy().astype(bool)


def device_sample(eng, d_vert, d_tri, N, seed=0, d_col=None, d_nrm=None, want_triangle=False):
    """`im_mesh_sample_table` and `im_mesh_sample`: (points, colors or None, normals, triangle or None, count_end), device tensors."""
    dev, st = eng.device, eng.stream_ptr()
    V, T = int(d_vert.shape[0]), int(d_tri.shape[0])
    count_end = torch.empty(T, dtype=torch.int64, device=dev)
    eng.ctx.call("im_mesh_sample_table", ptr(d_vert), V, ptr(d_tri), T, N, None, ptr(count_end), None, st)
    pts, nrm = (torch.empty((N, 3), dtype=torch.float64, device=dev) for _ in range(2))
    col = torch.empty((N, 3), dtype=torch.float64, device=dev) if d_col is not None else None
    which = torch.empty(N, dtype=torch.int32, device=dev) if want_triangle else None
    seed = int(seed) & (2 ** 64 - 1)
    eng.ctx.call("im_mesh_sample", ptr(d_vert), V, ptr(d_tri), T, ptr(count_end), N, seed - 2 ** 64 if seed >= 2 ** 63 else seed, ptr(d_col), ptr(d_nrm),
                 ptr(pts), ptr(col), ptr(nrm), ptr(which), st)
    return pts, col, nrm, which, count_end


def non_manifold_rounds(vertices, triangles) -> np.ndarray:
    """The host path of `remove_non_manifold_edges`, numpy: [T] bool, the triangles that stay. In rounds, until no edge has more than two
    live triangles, every such edge marks its live triangle of smallest area (0.5 |cross|), ties to the lowest index."""
    v, t = np.asarray(vertices, np.float64), np.asarray(triangles, np.int64)
    ok = ((t >= 0) & (t < len(v))).all(1)
    tt = np.where(ok[:, None], t, 0)
    with np.errstate(all="ignore"):
        a, b = v[tt[:, 1]] - v[tt[:, 0]], v[tt[:, 2]] - v[tt[:, 0]]
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        area = 0.5 * np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    area = np.where(ok & np.isfinite(area), area, 0.0)
    u, w = t.ravel(), np.roll(t, -1, axis=1).ravel()
    key = ((np.minimum(u, w) & 0xffffffff) << 32) | (np.maximum(u, w) & 0xffffffff)
    owner = np.repeat(np.arange(len(t)), 3)
    live = np.ones(len(t), bool)
    while True:
        sel = live[owner]
        uniq, inv, counts = np.unique(key[sel], return_inverse=True, return_counts=True)
        crowded = counts > 2
        if not crowded.any():
            return live
        own, inv = owner[sel][crowded[inv]], inv[crowded[inv]]
        order = np.lexsort((own, area[own], inv))                # per edge: smallest area first, then lowest index
        firsts = np.ones(len(order), bool)
        firsts[1:] = inv[order][1:] != inv[order][:-1]
        live[own[order][firsts]] = False


class TriangleMesh:
    """`vertices` [V, 3] float64, `triangles` [T, 3] int32, optional `vertex_colors` and `vertex_normals` [V, 3] float64, and
    `attributes`: further per-vertex arrays (the Poisson `density`) that follow their vertices through every operation. The `remove_*`
    operations work in place and return the mesh, `select_by_index` returns a new one, as in Open3D; `kept_vertices` / `kept_triangles`
    hold the old indices of what the last operation kept. The arrays live on the host, as `VoxelGrid`'s do: every operation uploads what
    it needs and downloads its result."""

    def __init__(self, vertices=None, triangles=None, vertex_colors=None, vertex_normals=None, attributes=None, engine=None):
        self.vertices = np.ascontiguousarray(np.zeros((0, 3)) if vertices is None else vertices, np.float64).reshape(-1, 3)
        self.triangles = np.ascontiguousarray(np.zeros((0, 3)) if triangles is None else triangles, np.int32).reshape(-1, 3)
        V = len(self.vertices)
        _check_counts(V, len(self.triangles))

        def per_vertex(name, a, shape3=True):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float64)
            a = a.reshape(-1, 3) if shape3 else a
            if len(a) != V:
                raise ValueError(f"{V} vertices but {name} of shape {a.shape}")
            return a
        self.vertex_colors, self.vertex_normals = per_vertex("vertex_colors", vertex_colors), per_vertex("vertex_normals", vertex_normals)
        self.attributes = {k: per_vertex(k, a, False) for k, a in (attributes or {}).items()}
        self.kept_vertices = self.kept_triangles = self.inside_hull = None
        self._engine = engine

    @classmethod
    def from_arrays(cls, vertices, vertex_colors, triangles, engine=None):
        """From the tuple of `VoxelGrid.to_box_mesh`: `TriangleMesh.from_arrays(*vg.to_box_mesh())`."""
        return cls(vertices, triangles, vertex_colors, engine=engine)

    @classmethod
    def create_from_point_cloud_poisson(cls, pcd, depth=8, width=0, scale=1.1, linear_fit=False, engine=None):
        """(mesh, densities) under Open3D's name: the surface of `poisson.poisson_reconstruct` over the points and normals of `pcd`, with
        the densities also as the mesh's vertex attribute `density`. Not Open3D's solver (see `poisson.py`); the cloud needs normals."""
        from .poisson import poisson_reconstruct
        if pcd.normals is None:
            raise ValueError("the point cloud has no normals: estimate them first")
        vertices, triangles, densities = poisson_reconstruct(pcd.points, pcd.normals, depth=depth, width=width, scale=scale, linear_fit=linear_fit, engine=engine)
        return cls(vertices, triangles, attributes={"density": densities}, engine=engine), densities

    def __len__(self):
        return len(self.vertices)

    def __repr__(self):
        return f"TriangleMesh with {len(self.vertices)} points and {len(self.triangles)} triangles."

    def has_vertices(self) -> bool:
        return len(self.vertices) > 0

    def has_triangles(self) -> bool:
        return len(self.triangles) > 0

    def has_vertex_colors(self) -> bool:
        return self.vertex_colors is not None and len(self.vertex_colors) == len(self.vertices) > 0

    def has_vertex_normals(self) -> bool:
        return self.vertex_normals is not None and len(self.vertex_normals) == len(self.vertices) > 0

    def get_axis_aligned_bounding_box(self):
        """(min corner, max corner) over the vertices; zeros without one"""
        if not len(self.vertices):
            return np.zeros(3), np.zeros(3)
        return self.vertices.min(0), self.vertices.max(0)

    # ---- the filters --------------------------------------------------------------------------------------------------------------------------
    def _eng(self, engine):
        return default_engine(engine if engine is not None else self._engine)

    def _filtered(self, engine, in_place, vertex_keep=None, merge_keys=False, triangle_keys=False, triangle_keep=None, **options):
        eng = self._eng(engine)
        dev, V = eng.device, len(self.vertices)
        d_tri = to_device(self.triangles, dev, np.int32)
        if isinstance(vertex_keep, torch.Tensor):                     # a mask a kernel left on the device
            d_keep = vertex_keep
        else:
            d_keep = None if vertex_keep is None else to_device(np.asarray(vertex_keep).astype(np.uint8), dev, np.uint8)
        d_tkeep = None if triangle_keep is None else to_device(np.asarray(triangle_keep).astype(np.uint8), dev, np.uint8)
        merge = None
        if merge_keys:
            merge, d_keep = device_first_of_segment(eng, device_vertex_keys(eng, to_device(self.vertices, dev, np.float64)))
        if triangle_keys:
            _, d_tkeep = device_first_of_segment(eng, device_triangle_keys(eng, d_tri))
        _, vlist, tri, pos = device_select(eng, V, d_tri, d_keep, merge, d_tkeep, **options)
        vlist, tri, pos = vlist.cpu().numpy().astype(np.int64), tri.cpu().numpy(), pos.cpu().numpy().astype(np.int64)
        out = self if in_place else TriangleMesh(engine=self._engine)
        colors, normals, attributes = self.vertex_colors, self.vertex_normals, self.attributes
        out.vertices, out.triangles = self.vertices[vlist], tri
        out.vertex_colors = None if colors is None else colors[vlist]
        out.vertex_normals = None if normals is None else normals[vlist]
        out.attributes = {k: a[vlist] for k, a in attributes.items()}
        out.kept_vertices, out.kept_triangles = vlist, pos
        return out

    def remove_vertices_by_mask(self, mask, engine=None):
        """Drops the masked vertices and every triangle that references one; renumbers the rest."""
        mask = np.asarray(mask).astype(bool).reshape(-1)
        if len(mask) != len(self.vertices):
            raise ValueError(f"{len(self.vertices)} vertices but a mask of {len(mask)}")
        return self._filtered(engine, True, vertex_keep=~mask)

    def select_by_index(self, indices, cleanup=True, engine=None):
        """A new mesh of the listed vertices (a set: duplicates and order are ignored) and the triangles whose three vertices are all
        listed; with `cleanup` the vertices no kept triangle references are dropped too."""
        idx = np.asarray(indices, np.int64).reshape(-1)
        if len(idx) and (idx.min() < 0 or idx.max() >= len(self.vertices)):
            raise ValueError("select_by_index: an index outside the vertices")
        keep = np.zeros(len(self.vertices), bool)
        keep[idx] = True
        return self._filtered(engine, False, vertex_keep=keep, drop_unreferenced=bool(cleanup))

    def remove_degenerate_triangles(self, engine=None):
        """Drops every triangle with two equal indices."""
        return self._filtered(engine, True, drop_degenerate=True)

    def remove_duplicated_triangles(self, engine=None):
        """Triangles whose index triples are equal after rotation to smallest-index-first (orientation counts): the lowest position stays."""
        return self._filtered(engine, True, triangle_keys=True)

    def remove_duplicated_vertices(self, engine=None):
        """Vertices with equal coordinates (-0.0 equals 0.0, a NaN equals nothing) merge into the lowest index, whose attributes stay."""
        return self._filtered(engine, True, merge_keys=True)

    def remove_unreferenced_vertices(self, engine=None):
        return self._filtered(engine, True, drop_unreferenced=True)

    def count_non_manifold_edges(self, engine=None) -> int:
        """The undirected edges that more than two triangles share: the census on the device."""
        eng = self._eng(engine)
        return device_edge_census(eng, to_device(self.triangles, eng.device, np.int32))

    def remove_non_manifold_edges(self, engine=None):
        """Nothing changes when the device census counts no edge with more than two triangles (the normal case); otherwise the rounds of
        `non_manifold_rounds` run on the host."""
        if self.count_non_manifold_edges(engine) == 0:
            self.kept_vertices, self.kept_triangles = np.arange(len(self.vertices)), np.arange(len(self.triangles))
            return self
        return self._filtered(engine, True, triangle_keep=non_manifold_rounds(self.vertices, self.triangles))

    def filter_by_hull(self, hull_points=None, facets=None, cleanup=True, engine=None):
        """`select_by_index` of the vertices inside a convex hull (`point_in_hull`); the mask goes from the hull kernel to the select on the
        device. `inside_hull` of the result is the number of vertices inside, before the clean-up. Like every operation of this class it
        uploads the mesh's host arrays and downloads the result: a chain of operations pays that once per operation."""
        facets = hull_facets(hull_points) if facets is None else facets
        if not len(self.vertices):
            out = self._filtered(engine, False, drop_unreferenced=bool(cleanup))
            out.inside_hull = 0
            return out
        eng = self._eng(engine)
        inside = device_in_hull(eng, to_device(self.vertices, eng.device, np.float64), facets)
        out = self._filtered(eng, False, vertex_keep=inside, drop_unreferenced=bool(cleanup))
        out.inside_hull = int(inside.sum().item())
        return out

    def sample_points_uniformly(self, number_of_points, seed=0, engine=None) -> PointCloud:
        """A cloud of `number_of_points` samples: triangle t receives the samples rint(c_(t-1) / C N) .. rint(c_t / C N) - 1 of the exact
        cumulative quantised areas c, sample i the point (1 - s) v0 + s (1 - r2) v1 + s r2 v2, s = sqrt(r1), of a counter-based
        generator of (seed, i). Colours follow when the mesh has them; normals are the vertex normals blended (not renormalised) or the
        triangles' unit normals."""
        N = int(number_of_points)
        if N < 0:
            raise ValueError("number_of_points must be >= 0")
        _check_counts(N)
        out = PointCloud(points3d=np.zeros((0, 3)), points_col=np.zeros((0, 3)) if self.vertex_colors is not None else None)
        out.normals = np.zeros((0, 3))
        if N == 0:
            return out
        if not len(self.triangles) or not len(self.vertices):
            raise ValueError("no triangle has an area, nothing can be sampled")
        eng = self._eng(engine)
        dev = eng.device
        d_col = None if self.vertex_colors is None else to_device(self.vertex_colors, dev, np.float64)
        d_nrm = None if self.vertex_normals is None else to_device(self.vertex_normals, dev, np.float64)
        pts, col, nrm, _, _ = device_sample(eng, to_device(self.vertices, dev, np.float64), to_device(self.triangles, dev, np.int32), N, seed, d_col, d_nrm)
        out = PointCloud(points3d=pts.cpu().numpy(), points_col=None if col is None else col.cpu().numpy())
        out.normals = nrm.cpu().numpy()
        return out


# ---- PLY ---------------------------------------------------------------------------------------------------------------------------------------
def read_triangle_mesh(path, engine=None) -> TriangleMesh:
    """A PLY file, ascii or binary little-endian, with a vertex element (x y z; optional red green blue, nx ny nz and a scalar `density`,
    kept as `attributes["density"]`) and a face element of one list property; every face must be a triangle."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.index(b"\n", end) + 1
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property" and elements:
            elements[-1][2].append(("list", w[2], w[3], w[4]) if w[1] == "list" else (w[2], _PLY_TYPES[w[1]]))
    names = [e[0] for e in elements]
    if names[:2] != ["vertex", "face"]:
        raise ValueError(f"{path}: the elements must be vertex, then face")
    (_, nv, vprops), (_, nf, fprops) = elements[:2]
    if any(p[0] == "list" for p in vprops) or len(fprops) != 1 or fprops[0][0] != "list":
        raise ValueError(f"{path}: vertices with plain properties and faces with one list property are supported")
    if fmt == "ascii":
        tokens = data[body:].split()
        rows = np.array(tokens[:nv * len(vprops)], dtype=np.float64).reshape(nv, len(vprops))
        cols = {name: rows[:, j] for j, (name, _) in enumerate(vprops)}
        faces = np.array(tokens[nv * len(vprops):nv * len(vprops) + 4 * nf], dtype=np.int64).reshape(nf, 4)
        counts, tri = faces[:, 0], faces[:, 1:]
    elif fmt == "binary_little_endian":
        vt = np.dtype([(name, "<" + t) for name, t in vprops])
        rec = np.frombuffer(data, vt, nv, body)
        cols = {name: rec[name] for name, _ in vprops}
        ft = np.dtype([("n", "<" + _PLY_TYPES[fprops[0][1]]), ("i", "<" + _PLY_TYPES[fprops[0][2]], (3,))])
        frec = np.frombuffer(data, ft, nf, body + nv * vt.itemsize)
        counts, tri = frec["n"], frec["i"]
    else:
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported")
    if not (np.asarray(counts) == 3).all():
        raise ValueError(f"{path}: a face that is no triangle")
    if not all(a in cols for a in "xyz"):
        raise ValueError(f"{path}: no x y z")
    types = dict(vprops)

    def stack(keys, scale=1.0):
        return np.stack([np.asarray(cols[k], np.float64) for k in keys], 1) / scale if all(k in cols for k in keys) else None
    colors = stack(("red", "green", "blue"), 255.0 if types.get("red") == "u1" else 1.0)
    attributes = {"density": np.asarray(cols["density"], np.float64)} if "density" in cols else None
    return TriangleMesh(stack("xyz"), np.asarray(tri, np.int32), colors, stack(("nx", "ny", "nz")), attributes, engine=engine)


def write_mesh(path, mesh: TriangleMesh, ascii: bool = False) -> bool:
    """The mesh-object writer next to `voxel_grid.write_triangle_mesh`: vertex (double x y z, uchar red green blue with colours, double
    nx ny nz with normals, double density with that attribute), face (list uchar int vertex_indices); binary little-endian or ascii."""
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    V, T = len(mesh.vertices), len(mesh.triangles)
    fields, cols = [("x", "<f8", "double"), ("y", "<f8", "double"), ("z", "<f8", "double")], [mesh.vertices[:, j] for j in range(3)]
    if mesh.vertex_colors is not None:
        c8 = np.clip(np.round(mesh.vertex_colors * 255.0), 0, 255).astype(np.uint8)
        fields += [(c, "u1", "uchar") for c in ("red", "green", "blue")]
        cols += [c8[:, j] for j in range(3)]
    if mesh.vertex_normals is not None:
        fields += [(c, "<f8", "double") for c in ("nx", "ny", "nz")]
        cols += [mesh.vertex_normals[:, j] for j in range(3)]
    if "density" in mesh.attributes:
        fields.append(("density", "<f8", "double"))
        cols.append(mesh.attributes["density"])
    head = ["ply", "format ascii 1.0" if ascii else "format binary_little_endian 1.0", f"element vertex {V}"]
    head += [f"property {t} {name}" for name, _, t in fields] + [f"element face {T}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if ascii:
            lines = [" ".join(repr(float(c[i])) if c.dtype.kind == "f" else str(int(c[i])) for c in cols) for i in range(V)]
            lines += ["3 " + " ".join(str(int(i)) for i in t) for t in mesh.triangles]
            f.write(("\n".join(lines) + "\n").encode("ascii") if lines else b"")
        else:
            rec = np.zeros(V, np.dtype([(name, t) for name, t, _ in fields]))
            for (name, _, _), c in zip(fields, cols):
                rec[name] = c
            f3 = np.zeros(T, np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
            f3["n"], f3["i"] = 3, mesh.triangles
            f.write(rec.tobytes())
            f.write(f3.tobytes())
    return True
