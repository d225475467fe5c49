"""Voxel grids on the device, with Open3D's names: `VoxelGrid.create_from_point_cloud_within_bounds`, `create_from_point_cloud`,
`get_voxels`, `get_voxel_center_coordinate`, and the cube mesh the reference's `scripts/pcd_postprocessing/voxelization.py` assembles one
voxel at a time (`to_box_mesh`). csrc/voxel.hip does the work (`im_voxel_keys`, torch's stable sort, `im_voxel_reduce`,
`im_voxel_mesh_corners`, the sort again, `im_voxel_mesh`). No CPU fallback: without a HIP device these raise. Open3D is not imported.

The definition (tests/voxel_oracle.py, bit-identical): float64; n_a = floor((max_a - min_a) / s) + 1 voxels per axis; a point
is kept iff its coordinates are finite and min_a <= p_a <= max_a; its index is floor((p_a - min_a) / s), a true division; the voxel's
colour is the sum of its points' colours in ascending point index from +0.0, divided by their number; voxels are listed in ascending
(i_x n_y + i_y) n_z + i_z. PARITY WITH AN OPEN3D BINARY IS UNPINNED: whether Open3D discards points outside the bounds, the order of its
voxels (a hash map's) and the text of its PLY writers are not checked."""
from pathlib import Path

import numpy as np
import torch

from .._lib import load, ptr
from ..engine import default_engine, to_device

MAX_CELLS = 2 ** 62
MAX_MESH_ITEMS = 2 ** 27
MAX_CLOUDS = 65535


def max_points() -> int:
    """The most points one device call takes; `voxel_series` splits longer series."""
    return int(load().im_voxel_max_points())


class Voxel:
    """One filled voxel: `grid_index` (3 integers) and `color` (3 floats in 0..1)."""

    def __init__(self, grid_index, color):
        self.grid_index, self.color = grid_index, color

    def __repr__(self):
        return f"Voxel with grid_index: ({self.grid_index[0]}, {self.grid_index[1]}, {self.grid_index[2]}), color: ({self.color[0]}, {self.color[1]}, {self.color[2]})"


def make_grid(min_bound, max_bound, voxel_size) -> np.ndarray:
    """[7] float64 = min_bound, max_bound, voxel_size, or the ValueError of a grid the library refuses: before any device work."""
    s = float(voxel_size)
    mn, mx = np.asarray(min_bound, np.float64).reshape(-1), np.asarray(max_bound, np.float64).reshape(-1)
    if mn.shape != (3,) or mx.shape != (3,):
        raise ValueError("min_bound and max_bound must hold three values each")
    if not (np.isfinite(s) and s > 0.0):
        raise ValueError(f"voxel_size must be finite and positive (got {voxel_size})")
    if not (np.isfinite(mn).all() and np.isfinite(mx).all() and (mx >= mn).all()):
        raise ValueError("the bounds must be finite with max_bound >= min_bound")
    grid = np.concatenate([mn, mx, [s]])
    grid_dims(grid)
    return grid


def grid_dims(grid, corners=False):
    """(n_x, n_y, n_z) of a grid; ValueError over 2^62 voxels (`corners`: over 2^62 corner keys)."""
    with np.errstate(over="ignore"):
        nd = np.floor((grid[3:6] - grid[:3]) / grid[6]) + 1.0
    if not (np.isfinite(nd).all() and (nd <= MAX_CELLS).all()):
        raise ValueError("the grid holds more than 2^62 voxels")
    n = tuple(int(v) for v in nd)
    k = 1 if corners else 0
    if (n[0] + k) * (n[1] + k) * (n[2] + k) > MAX_CELLS:
        raise ValueError("the grid holds more than 2^62 voxels" if not corners else "the grid holds more than 2^62 mesh corners")
    return n


def cloud_arrays(pcd_or_points, colors=None, normals=None):
    """(points [n, 3], colors [n, 3] or None, normals [n, 3] or None) as float64 of a `core.PointCloud`, a `.ply` path or arrays."""
    from ..core.point_cloud import PointCloud, read_ply
    if isinstance(pcd_or_points, PointCloud):
        points = pcd_or_points.points
        colors = pcd_or_points.colors if colors is None else colors
        normals = pcd_or_points.normals if normals is None else normals
    elif isinstance(pcd_or_points, (str, bytes)) or hasattr(pcd_or_points, "__fspath__"):
        try:
            points, file_colors, file_normals = read_ply(pcd_or_points)
        except (OSError, ValueError, KeyError) as e:
            raise IOError(f"Unable to read point cloud {pcd_or_points}") from e
        colors = file_colors if colors is None else colors
        normals = file_normals if normals is None else normals
    else:
        points = pcd_or_points.detach().cpu().numpy() if isinstance(pcd_or_points, torch.Tensor) else np.asarray(pcd_or_points)
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"a cloud must be [n, 3] (got {points.shape})")
    out = [np.ascontiguousarray(points, np.float64)]
    for name, a in (("colors", colors), ("normals", normals)):
        if a is not None:
            a = np.ascontiguousarray(a, np.float64)
            if a.shape != points.shape:
                raise ValueError(f"{len(points)} points but {name} of shape {a.shape}")
        out.append(a)
    return tuple(out)


def _batches(sizes, cap):
    """consecutive runs of clouds that hold at most `cap` points together"""
    out, cur, n = [], [], 0
    for e, m in enumerate(sizes):
        if m > cap:
            raise ValueError(f"a cloud of {m} points exceeds the {cap} points of one device call")
        if cur and (n + m > cap or len(cur) == MAX_CLOUDS):
            out.append(cur)
            cur, n = [], 0
        cur.append(e)
        n += m
    return out + ([cur] if cur else [])


def _cat(arrays, dev):
    return to_device(np.concatenate(list(arrays) + [np.zeros((0, 3))]), dev, np.float64)


def device_pass(eng, clouds, grids=None, voxel_size=None, want_points=False):
    """One pass of csrc/voxel.hip over `clouds`, a list of (points, colors or None, normals or None) that either all or none carry colours
    (normals likewise). `grids`: [7] for all clouds, [E, 7] one per cloud, or None: then every cloud gets the grid of
    `create_from_point_cloud`, min(points) - 0.5 s .. max(points) + 0.5 s over its finite points. Returns (results, grids [E, 7]): per cloud
    a dict of grid_index, counts, first, dropped, colors / normals / points (the means; None where not asked for or absent)."""
    E = len(clouds)
    if E == 0:
        return [], np.zeros((0, 7))
    dev, st = eng.device, eng.stream_ptr()
    offsets = np.concatenate([[0], np.cumsum([len(c[0]) for c in clouds])]).astype(np.int64)
    n = int(offsets[-1])
    has_col, has_nrm = clouds[0][1] is not None, clouds[0][2] is not None
    pts = _cat([c[0] for c in clouds], dev)
    if grids is None:
        s = float(voxel_size)
        d_bounds = torch.empty((E, 6), dtype=torch.float64, device=dev)
        eng.ctx.call("im_voxel_bounds", ptr(pts), offsets.ctypes.data, E, ptr(d_bounds), st)
        b = d_bounds.cpu().numpy()
        grids = np.zeros((E, 7))
        for e in range(E):
            grids[e] = make_grid(b[e, :3] - 0.5 * s, b[e, 3:] + 0.5 * s, s) if np.isfinite(b[e]).all() else (0, 0, 0, 0, 0, 0, s)
    grids = np.ascontiguousarray(grids, np.float64)
    per_cloud = grids.ndim == 2
    cells = [int(np.prod(grid_dims(g), dtype=object)) for g in grids.reshape(-1, 7)]
    if (sum(cells) if per_cloud else cells[0] * E) > MAX_CELLS:
        raise ValueError("the grids of the clouds hold more than 2^62 voxels together: pass fewer clouds per call")
    key = torch.empty(n, dtype=torch.int64, device=dev)
    d_dropped = torch.empty(E, dtype=torch.int64, device=dev)
    head = (offsets.ctypes.data, E, grids.ctypes.data, int(per_cloud))
    eng.ctx.call("im_voxel_keys", ptr(pts), *head, ptr(key), ptr(d_dropped), st)
    skey, perm = torch.sort(key, stable=True)
    col = _cat([c[1] for c in clouds], dev) if has_col else None
    nrm = _cat([c[2] for c in clouds], dev) if has_nrm else None
    d_nvox = torch.empty(E + 1, dtype=torch.int64, device=dev)
    d_index = torch.empty((n, 3), dtype=torch.int32, device=dev)
    d_count, d_first = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    mean = [torch.empty((n, 3), dtype=torch.float64, device=dev) if want else None for want in (want_points, has_col, has_nrm)]
    eng.ctx.call("im_voxel_reduce", *head, ptr(skey), ptr(perm), ptr(pts) if want_points else None, ptr(col), ptr(nrm), ptr(d_nvox), ptr(d_index),
                 ptr(d_count), ptr(d_first), ptr(mean[0]), ptr(mean[1]), ptr(mean[2]), st)
    nvox, dropped = d_nvox.cpu().numpy(), d_dropped.cpu().numpy()
    V = int(nvox[E])
    index, count, first = d_index[:V].cpu().numpy(), d_count[:V].cpu().numpy(), d_first[:V].cpu().numpy()
    mean = [None if m is None else m[:V].cpu().numpy() for m in mean]
    out = []
    for e in range(E):
        a, b = int(nvox[e]), int(nvox[e + 1])
        out.append({"grid_index": index[a:b].copy(), "counts": count[a:b].copy(), "first": first[a:b].copy(), "dropped": int(dropped[e]),
                    "points": None if mean[0] is None else mean[0][a:b].copy(), "colors": None if mean[1] is None else mean[1][a:b].copy(),
                    "normals": None if mean[2] is None else mean[2][a:b].copy()})
    return out, (grids if per_cloud else np.tile(grids, (E, 1)))


class VoxelGrid:
    """The filled voxels of one cloud under one grid, in ascending voxel key: `origin` [3] = min_bound, `voxel_size`, `grid_indices`
    [V, 3] int32, `colors` [V, 3] float64 (zeros without colours), `counts` [V] the points per voxel, `dropped` the points outside the
    bounds or with a non-finite coordinate."""

    def __init__(self, grid, result, engine=None):
        self.grid = np.array(grid, np.float64)
        self.origin, self.max_bound, self.voxel_size = self.grid[:3].copy(), self.grid[3:6].copy(), float(self.grid[6])
        self.dims = grid_dims(self.grid)
        self.grid_indices, self.counts, self.dropped = result["grid_index"], result["counts"], result["dropped"]
        self._has_colors = result["colors"] is not None
        self.colors = result["colors"] if self._has_colors else np.zeros((len(self.counts), 3), np.float64)
        self._engine = engine

    @classmethod
    def create_from_point_cloud_within_bounds(cls, pcd_or_points, voxel_size, min_bound, max_bound, colors=None, engine=None):
        grid = make_grid(min_bound, max_bound, voxel_size)
        cloud = cloud_arrays(pcd_or_points, colors)
        eng = default_engine(engine)
        results, _ = device_pass(eng, [(cloud[0], cloud[1], None)], grid)
        return cls(grid, results[0], eng)

    @classmethod
    def create_from_point_cloud(cls, pcd_or_points, voxel_size, colors=None, engine=None):
        """The grid spans min(points) - 0.5 voxel_size .. max(points) + 0.5 voxel_size over the points with finite coordinates."""
        make_grid((0, 0, 0), (0, 0, 0), voxel_size)
        cloud = cloud_arrays(pcd_or_points, colors)
        eng = default_engine(engine)
        results, grids = device_pass(eng, [(cloud[0], cloud[1], None)], None, voxel_size)
        return cls(grids[0], results[0], eng)

    def __len__(self):
        return len(self.counts)

    def __repr__(self):
        return f"VoxelGrid with {len(self)} voxels."

    def has_colors(self) -> bool:
        return self._has_colors

    def has_voxels(self) -> bool:
        return len(self) > 0

    def get_voxels(self):
        return [Voxel(gi, c) for gi, c in zip(self.grid_indices, self.colors)]

    def get_voxel_center_coordinate(self, idx) -> np.ndarray:
        """origin + (idx + 0.5) * voxel_size"""
        return self.origin + (np.asarray(idx).astype(np.float64) + 0.5) * self.voxel_size

    def centers(self) -> np.ndarray:
        """[V, 3]: the centre of every filled voxel"""
        return self.get_voxel_center_coordinate(self.grid_indices).reshape(-1, 3)

    def get_axis_aligned_bounding_box(self):
        """(min corner, max corner) of the filled voxels; (origin, origin) without one"""
        if not len(self):
            return self.origin.copy(), self.origin.copy()
        gi = self.grid_indices.astype(np.float64)
        return self.origin + gi.min(0) * self.voxel_size, self.origin + (gi.max(0) + 1.0) * self.voxel_size

    def to_box_mesh(self, engine=None):
        """(vertices [U, 3] float64, vertex_colors [U, 3] float64, triangles [12 V, 3] int32): one cube per filled voxel, the corners that
        cubes share merged. Vertices in ascending corner key at origin + c * voxel_size, a vertex's colour the mean of the voxels that
        share it, 12 outward-facing triangles per voxel in voxel order (faces between neighbouring voxels are kept, as in the script)."""
        V = len(self)
        grid_dims(self.grid, corners=True)
        if 8 * V > MAX_MESH_ITEMS:
            raise ValueError(f"{V} voxels: a box mesh takes at most 2^24")
        if V == 0:
            return np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3), np.int32)
        eng = default_engine(engine if engine is not None else self._engine)
        dev, st = eng.device, eng.stream_ptr()
        d_index, d_col = to_device(self.grid_indices, dev, np.int32), to_device(self.colors, dev, np.float64)
        ckey = torch.empty(8 * V, dtype=torch.int64, device=dev)
        eng.ctx.call("im_voxel_mesh_corners", self.grid.ctypes.data, ptr(d_index), V, ptr(ckey), st)
        skey, perm = torch.sort(ckey, stable=True)
        d_nv = torch.empty(1, dtype=torch.int64, device=dev)
        d_vert, d_vcol = (torch.empty((8 * V, 3), dtype=torch.float64, device=dev) for _ in range(2))
        d_tri = torch.empty((12 * V, 3), dtype=torch.int32, device=dev)
        eng.ctx.call("im_voxel_mesh", self.grid.ctypes.data, V, ptr(d_col), ptr(skey), ptr(perm), ptr(d_nv), ptr(d_vert), ptr(d_vcol), ptr(d_tri), st)
        U = int(d_nv.cpu()[0])
        return d_vert[:U].cpu().numpy(), d_vcol[:U].cpu().numpy(), d_tri.cpu().numpy()


def voxel_center_lines(grid: VoxelGrid):
    """The script's text lines: `x,y,z,r,g,b` per voxel, the centre with 4 decimals, the colour as Python prints a float."""
    centers, colors = grid.centers().tolist(), grid.colors.tolist()
    return [f"{x:.4f},{y:.4f},{z:.4f},{r!r},{g!r},{b!r}\n" for (x, y, z), (r, g, b) in zip(centers, colors)]


def write_voxel_centers(path, grid: VoxelGrid) -> bool:
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as f:
        f.writelines(voxel_center_lines(grid))
    return True


def write_voxel_grid(path, grid: VoxelGrid) -> bool:
    """An ASCII PLY: elements origin (double x y z), voxel_size (double val) and vertex (int x y z, uchar red green blue), one vertex per
    voxel. Not checked against Open3D's writer."""
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    c8 = np.clip(np.round(grid.colors * 255.0), 0, 255).astype(np.uint8)
    head = ["ply", "format ascii 1.0", "comment voxel grid of icepy4d_amd", "element origin 1", "property double x", "property double y", "property double z",
            "element voxel_size 1", "property double val", f"element vertex {len(grid)}", "property int x", "property int y", "property int z",
            "property uchar red", "property uchar green", "property uchar blue", "end_header",
            " ".join(repr(float(v)) for v in grid.origin), repr(grid.voxel_size)]
    rows = [f"{i} {j} {k} {r} {g} {b}" for (i, j, k), (r, g, b) in zip(grid.grid_indices.tolist(), c8.tolist())]
    with open(path, "w") as f:
        f.write("\n".join(head + rows) + "\n")
    return True


def write_triangle_mesh(path, vertices, vertex_colors, triangles) -> bool:
    """A binary little-endian PLY: vertex (double x y z, uchar red green blue when colours are given), face (list uchar int vertex_indices)."""
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    vertices, triangles = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(triangles, np.int32).reshape(-1, 3)
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(vertices)}", "property double x", "property double y", "property double z"]
    if vertex_colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += [f"element face {len(triangles)}", "property list uchar int vertex_indices", "end_header"]
    v = np.zeros(len(vertices), np.dtype(fields))
    for j, a in enumerate("xyz"):
        v[a] = vertices[:, j]
    if vertex_colors is not None:
        c8 = np.clip(np.round(np.asarray(vertex_colors, np.float64) * 255.0), 0, 255).astype(np.uint8)
        for j, a in enumerate(("red", "green", "blue")):
            v[a] = c8[:, j]
    f3 = np.zeros(len(triangles), np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    f3["n"], f3["i"] = 3, triangles
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(v.tobytes())
        f.write(f3.tobytes())
    return True
