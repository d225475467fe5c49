"""The point-cloud helpers of the reference's `post_processing/open3d_fun.py` that need no Open3D here: `filter_pcd_by_polyline` (the
crop of a cloud to the glacier outline, on the device: csrc/dod.hip `crop_polygon_kernel`) and `read_and_merge_point_clouds`, both on
`core.PointCloud`, and `MeshingPoisson`: of its eight steps the Poisson solve is a hook (an octree solve is no data-parallel pass over
points or cells), everything behind it runs on the device (`triangle_mesh.py`, csrc/mesh.hip). `poisson.poisson_reconstruct`
has the hook's signature: a Poisson reconstruction on the dense grid of the finest octree level (csrc/poisson.hip), not Open3D's solver.

The reference tests the points with matplotlib's `Path.contains_points`; here the even-odd crossing rule in float64 is restated
(include/icematch.h `im_crop_polygon`; tests/dod_oracle.py, bit-identical). The two agree on every point that does not lie on an edge
(tests/test_dod_cpu.py: equal masks farther than 1e-9 from every edge); on an edge matplotlib's answer is its own."""
import logging
import multiprocessing
from pathlib import Path
from typing import List, Union

import numpy as np
import torch

from .._lib import ptr
from ..core.point_cloud import PointCloud
from ..engine import default_engine, to_device
from ..utils.geospatial import ccw_sort_points
from ..utils.timer import AverageTimer
from . import triangle_mesh as TM

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


class _Cfg(dict):
    """The options of `MeshingPoisson`, read as `cfg["key"]` or, as the reference's EasyDict allows, `cfg.key`."""

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key) from None


class MeshingPoisson:
    """The reference's class (`open3d_fun.py: MeshingPoisson`) with its defaults, cfg keys (its spelling `min_mesh_denisty` included),
    method names, step order, log and timer labels and output names `mesh_{date}.ply` / `sampled_{date}.ply`.

    The Poisson solve is not built in (`reconstruct=poisson.poisson_reconstruct` supplies one). `poisson_meshing` calls `reconstruct(points, normals, depth=cfg.poisson_depth, width=0, scale=1.1,
    linear_fit=False)`, which returns `(vertices, triangles, densities)`; without the hook it reads `cfg["mesh_path"]`, a PLY with a vertex
    property `density`. `orient_triangles` is not provided either: the supplied surface is taken as oriented. Everything else runs on the
    device: SOR (50, 1.5) and normals (radius 1, max_nn 30) of `utils/point_cloud_filters.py`, the mesh filters, the hull crop (qhull gives
    the hull on the host), the sampling and the polygon crop.

    One departure: the density array follows its vertices through every later step (`self.density` is the filtered mesh's), where the
    reference leaves it at the length of the density filter's output (the bug its `run()` notes)."""

    def __init__(self, pcd_path: Union[str, Path], out_dir: Union[str, Path], cfg: dict, reconstruct=None, engine=None) -> None:
        pcd_path = Path(pcd_path)
        assert pcd_path.exists(), "Input point cloud does not exists."
        self.pcd_path = pcd_path
        self.out_dir = Path(out_dir)
        self.out_dir.mkdir(parents=True, exist_ok=True)
        default_cfg = {
            "do_SOR": True,
            "poisson_depth": 9,
            "min_mesh_denisty": 11,
            "save_mesh": True,
            "sample_mesh": True,
            "num_sampled_points": 2 * 10**6,
        }
        self.cfg = _Cfg({**default_cfg, **{k: v for k, v in cfg.items()}})
        self.reconstruct = reconstruct
        self.engine = engine
        self.seed = int(self.cfg.get("seed", 0))
        self.logger = logging.getLogger(multiprocessing.current_process().name)
        self.timer = AverageTimer(logger=self.logger)

    def read_pcd(self) -> None:
        self.pcd = PointCloud(pcd_path=str(self.pcd_path))
        self.logger.info(f"Point cloud {self.pcd_path.stem} imported.")
        self.timer.update("Read pcd")
        if self.cfg["do_SOR"]:
            self.SOR()
        self.convex_hull = TM.compute_convex_hull(self.pcd)
        if self.pcd.normals is None:
            self.pcd.estimate_normals(radius=1, max_nn=30, engine=self.engine)
            self.logger.warning("Point cloud did not have normals. Normals computed.")
            self.timer.update("Normals estimation")

    def SOR(self) -> None:
        self.pcd.sor_filter(nb_neighbors=50, std_ratio=1.5, engine=self.engine)
        self.logger.info("Point cloud filtered with SOR.")
        self.timer.update("SOR")

    def poisson_meshing(self) -> None:
        if self.reconstruct is not None:
            vertices, triangles, density = self.reconstruct(self.pcd.points, self.pcd.normals, depth=self.cfg["poisson_depth"], width=0, scale=1.1,
                                                            linear_fit=False)
            self.mesh = TM.TriangleMesh(vertices, triangles, attributes={"density": np.asarray(density, np.float64).reshape(-1)}, engine=self.engine)
        elif self.cfg.get("mesh_path"):
            self.mesh = TM.read_triangle_mesh(self.cfg["mesh_path"], engine=self.engine)
            if "density" not in self.mesh.attributes:
                raise ValueError(f"{self.cfg['mesh_path']}: no vertex property `density`")
        else:
            raise NotImplementedError("Poisson reconstruction is not provided: pass reconstruct=f(points, normals, depth=, width=, scale=, linear_fit=) "
                                      "-> (vertices, triangles, densities), or set cfg['mesh_path'] to a PLY with a vertex property `density`")
        self.density = self.mesh.attributes["density"]
        self.logger.info("Point cloud meshed by Poisson mesh reconstruction.")
        self.timer.update("Poisson meshing")

    def filter_mesh_by_density(self) -> None:
        vertexes_to_remove = self.density < self.cfg["min_mesh_denisty"]
        self.mesh.remove_vertices_by_mask(vertexes_to_remove, engine=self.engine)
        self.mesh.remove_degenerate_triangles(engine=self.engine)
        self.mesh.remove_duplicated_triangles(engine=self.engine)
        self.mesh.remove_duplicated_vertices(engine=self.engine)
        self.mesh.remove_non_manifold_edges(engine=self.engine)
        self.density = self.mesh.attributes["density"]
        self.logger.info(f"Poisson mesh filtered by density. Removed vertex with density < {self.cfg['min_mesh_denisty']}")
        self.timer.update("Filter by density")

    def filter_mesh_by_convex_hull(self):
        n = len(self.mesh.vertices)
        self.mesh = self.mesh.filter_by_hull(self.convex_hull, engine=self.engine)
        self.density = self.mesh.attributes["density"]
        self.logger.info(f"Poisson mesh filtered by original pcd convex hull: removed points {self.mesh.inside_hull}/{n}")
        self.timer.update("Filter by location")

    def sample_mesh(self) -> None:
        self.sampled_pcd = self.mesh.sample_points_uniformly(number_of_points=self.cfg["num_sampled_points"], seed=self.seed, engine=self.engine)

    def filter_pcd_by_polygon(self, pcd: PointCloud, dir: str = "x", polygon: np.ndarray = None) -> PointCloud:
        pcd_out = filter_pcd_by_polyline(pcd, self.cfg["crop_polyline_path"], dir, engine=self.engine)
        self.logger.info("Point cloud cropped by polyline")
        self.timer.update("crop by polyline")
        return pcd_out

    def write_outputs(self) -> bool:
        idx = self.pcd_path.stem.find("202")
        base_name = self.pcd_path.stem[idx:]
        if self.cfg["save_mesh"]:
            TM.write_mesh(self.out_dir / f"mesh_{base_name}.ply", self.mesh)
        if self.cfg["sample_mesh"]:
            self.sampled_pcd.write_ply(self.out_dir / f"sampled_{base_name}.ply")
        self.timer.update("save outputs")
        return True

    def run(self) -> bool:
        self.read_pcd()
        self.poisson_meshing()
        self.filter_mesh_by_density()
        self.filter_mesh_by_convex_hull()
        if self.cfg["sample_mesh"]:
            self.sample_mesh()
        if self.cfg.get("crop_polyline_path"):
            self.sampled_pcd = self.filter_pcd_by_polygon(self.sampled_pcd)
        if self.write_outputs():
            self.logger.info("Outputs saved successfully.")
        else:
            self.logger.error("Unable to write outputs to disk.")
        self.timer.print()
        return True
