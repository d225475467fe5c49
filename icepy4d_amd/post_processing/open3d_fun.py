"""The point-cloud helpers of the reference's `post_processing/open3d_fun.py` that need no Open3D here: `filter_pcd_by_polyline` (the
crop of a cloud to the glacier outline, on the device: csrc/dod.hip `crop_polygon_kernel`) and `read_and_merge_point_clouds`, both on
`core.PointCloud`. `MeshingPoisson` is not provided: Poisson meshing is no data-parallel pass over points or cells.

The reference tests the points with matplotlib's `Path.contains_points`; here the even-odd crossing rule in float64 is restated
(include/icematch.h `im_crop_polygon`; tests/dod_oracle.py, bit-identical). The two agree on every point that does not lie on an edge
(tests/test_dod_cpu.py: equal masks farther than 1e-9 from every edge); on an edge matplotlib's answer is its own."""
from pathlib import Path
from typing import List

import numpy as np
import torch

from .._lib import ptr
from ..core.point_cloud import PointCloud
from ..engine import default_engine, to_device
from ..utils.geospatial import ccw_sort_points

MAX_VERTICES = 1024


def crop_indices(points, polygon, axis_x, axis_y, inside=True, engine=None):
    """The ascending indices (int64, numpy) of the points [n, 3] whose (axis_x, axis_y) coordinates lie inside (or, `inside=False`,
    outside) the closed `polygon` [nv, 2], nv <= 1024, by the even-odd rule, on the device. Fewer than three vertices hold nothing."""
    polygon = np.ascontiguousarray(polygon, np.float64).reshape(-1, 2)
    if len(polygon) > MAX_VERTICES:
        raise ValueError(f"a polygon has at most {MAX_VERTICES} vertices (got {len(polygon)})")
    if not np.isfinite(polygon).all():
        raise ValueError("the polygon holds non-finite vertices")
    if axis_x == axis_y or axis_x not in (0, 1, 2) or axis_y not in (0, 1, 2):
        raise ValueError("the axes must be two of 0, 1, 2")
    pts = points if isinstance(points, torch.Tensor) else np.asarray(points, np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be [n, 3] (got {tuple(pts.shape)})")
    n = pts.shape[0]
    if len(polygon) < 3:
        return np.arange(n, dtype=np.int64) if not inside else np.zeros(0, np.int64)
    if n == 0:
        return np.zeros(0, np.int64)
    eng = default_engine(engine)
    dev = eng.device
    d_pts = pts.to(device=dev, dtype=torch.float64).contiguous() if isinstance(pts, torch.Tensor) else to_device(pts, dev, np.float64)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    index = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    eng.ctx.call("im_crop_polygon", ptr(d_pts), n, int(axis_x), int(axis_y), polygon.ctypes.data, len(polygon), 1 if inside else 0, ptr(mask),
                 ptr(index), ptr(count), eng.stream_ptr())
    return index[:int(count.item())].cpu().numpy()


def select_by_index(pcd: PointCloud, idx) -> PointCloud:
    """A new cloud of the listed points, with their colours and normals."""
    out = PointCloud(points3d=pcd.points[idx], points_col=None if pcd.colors is None else pcd.colors[idx])
    out.normals = None if pcd.normals is None else pcd.normals[idx]
    return out


def read_polyline(polyline_path):
    with open(polyline_path, "r") as f:
        return np.loadtxt(f, delimiter=" ").reshape(-1, 3)


def filter_pcd_by_polyline(pcd: PointCloud, polyline_path: str, dir: str = "x", engine=None) -> PointCloud:
    """The points of `pcd` (with colours and normals) inside the outline in `polyline_path` (rows "x y z"), seen along `dir`. As in the
    reference only "x" is implemented, the Y-Z plane: the outline's (y, z) columns are ordered counter-clockwise around their mean
    (`ccw_sort_points`), closed, and tested against the points' (y, z)."""
    poly = read_polyline(polyline_path)
    if dir == "x":
        poly = poly[:, 1:]
    else:
        raise ValueError("Cutting point cloud implemented only on Y-Z plane")
    idx = crop_indices(pcd.points, ccw_sort_points(poly), 1, 2, engine=engine)
    return select_by_index(pcd, idx)


def read_and_merge_point_clouds(pcd_names: List[str]) -> PointCloud:
    """One cloud of all points of the listed files, in order, with their colours (zeros for a file without colours)."""
    clouds = []
    for path in pcd_names:
        if not Path(path).is_file():
            raise FileNotFoundError(f"File not found: {path}")
        clouds.append(PointCloud(pcd_path=path))
    pts_all = np.concatenate([c.points for c in clouds] + [np.zeros((0, 3))])
    col_all = np.concatenate([c.colors if c.colors is not None else np.zeros((len(c), 3)) for c in clouds] + [np.zeros((0, 3))])
    return PointCloud(points3d=pts_all, points_col=col_all)
