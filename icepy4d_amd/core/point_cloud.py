"""`PointCloud` with the reference's names (`src/icepy4d/core/point_cloud.py`), numpy-backed: the reference wraps an Open3D point cloud,
which is not a dependency here. `sor_filter` and `estimate_normals` run on the device (`utils/point_cloud_filters.py`, csrc/knn.hip), `voxel_down_sample` too (csrc/voxel.hip);
parity of either with an Open3D binary is unpinned (see that module).

PLY files are `binary_little_endian 1.0` with `double x y z`, then `uchar red green blue` when colours exist (round(c * 255) clipped to
0..255), then `double nx ny nz` when normals exist: the layout Open3D documents for its default writer. Byte parity with a file written
by Open3D is unpinned. `write_ply(scalars=...)` adds `float confidence` and / or `uchar views` behind them on request; the reader skips
properties it does not know, these two included. The reader takes that layout and its float / ascii variants. `.las` needs laspy, which is not a dependency:
reading and writing it raise NotImplementedError."""
import logging
from pathlib import Path
from typing import Union

import numpy as np

logger = logging.getLogger(__name__)

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


PLY_SCALARS = {"confidence": ("float", "<f4"), "views": ("uchar", "u1")}      # per-point attributes `write_ply(scalars=...)` may name: PLY type, numpy type


def ply_header(n: int, colors: bool, normals: bool, scalars=()) -> bytes:
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}", "property double x", "property double y", "property double z"]
    if colors:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    if normals:
        lines += ["property double nx", "property double ny", "property double nz"]
    lines += [f"property {t} {name}" for name, t in scalars]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def read_ply(path):
    """(points [n, 3] float64, colors [n, 3] float64 in 0..1 or None, normals [n, 3] float64 or None) of a PLY file's vertex element."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.index(b"\n", end) + 1
    fmt, n, props, element = None, 0, [], None
    for line in data[:end].decode("ascii", "replace").splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            element = w[1]
            if element == "vertex":
                n = int(w[2])
            elif not props:
                raise ValueError(f"{path}: the vertex element must come first")
        elif w[0] == "property" and element == "vertex":
            if w[1] == "list":
                raise ValueError(f"{path}: list properties on vertices are not supported")
            props.append((w[2], _PLY_TYPES[w[1]]))
    if fmt == "ascii":
        rows = np.array(data[body:].split()[:n * len(props)], dtype=np.float64).reshape(n, len(props))
        cols = {name: rows[:, j] for j, (name, _) in enumerate(props)}
    elif fmt in ("binary_little_endian", "binary_big_endian"):
        order = "<" if fmt == "binary_little_endian" else ">"
        rec = np.frombuffer(data, dtype=np.dtype([(name, order + t) for name, t in props]), count=n, offset=body)
        cols = {name: rec[name] for name, _ in props}
    else:
        raise ValueError(f"{path}: unknown PLY format {fmt!r}")
    if not all(a in cols for a in "xyz"):
        raise ValueError(f"{path}: no x y z")
    points = np.stack([np.asarray(cols[a], np.float64) for a in "xyz"], 1)
    colors = normals = None
    if all(c in cols for c in ("red", "green", "blue")):
        types = dict(props)
        scale = 255.0 if types["red"] == "u1" else 1.0
        colors = np.stack([np.asarray(cols[c], np.float64) for c in ("red", "green", "blue")], 1) / scale
    if all(c in cols for c in ("nx", "ny", "nz")):
        normals = np.stack([np.asarray(cols[c], np.float64) for c in ("nx", "ny", "nz")], 1)
    return points, colors, normals


class PointCloud:
    """Points [n, 3] float64, optional colours [n, 3] float64 in 0..1, optional normals [n, 3] float64."""

    def __init__(self, points3d: np.ndarray = None, pcd_path: str = None, points_col: np.ndarray = None, verbose: bool = False) -> None:
        self.points = np.zeros((0, 3), np.float64)
        self.colors = None
        self.normals = None
        self.confidence = None            # [n] float32 where the producer has one (`dense.build_dense_cloud`); written to PLY on request (`write_ply(scalars=...)`)
        self.views = None                 # [n] uint8, the number of depth maps that agreed on the point (`dense.build_dense_cloud(fuse=...)`); likewise
        if isinstance(points3d, np.ndarray):
            self.from_numpy(points3d, points_col)
        elif pcd_path is not None:
            pcd_path = Path(pcd_path)
            if pcd_path.suffix in (".las", ".laz"):
                self.read_las(pcd_path)
            elif pcd_path.suffix == ".ply":
                self.points, self.colors, self.normals = read_ply(pcd_path)
            else:
                raise ValueError("Invalid file format. It must be .ply (.las / .laz need laspy, which is not a dependency)")
        self._verbose = verbose

    def __repr__(self):
        return f"PointCloud with {len(self)} points"

    def __len__(self):
        return len(self.points)

    def get_points(self) -> np.ndarray:
        """Get point coordinates as nx3 numpy array"""
        return self.points

    def get_colors(self, as_float: bool = False) -> np.ndarray:
        """Get point colors as nx3 numpy array of integers values (0-255); as_float: float32 in 0..1"""
        if self.colors is None:
            return None
        if as_float:
            return self.colors.astype(np.float32)
        return (np.asarray(self.colors) * 255.0).astype(int)

    def get_normals(self) -> np.ndarray:
        return self.normals

    def read_las(self, path: Union[str, Path]):
        raise NotImplementedError("reading .las / .laz needs laspy, which is not a dependency of this library")

    def from_numpy(self, points3d: np.ndarray, points_col: np.ndarray = None) -> None:
        """points3d [n, 3]; points_col [n, 3] floats in the range [0, 1]."""
        points = np.array(points3d, dtype=np.float64).reshape(-1, 3)
        colors = None
        if points_col is not None:
            colors = np.array(points_col, dtype=np.float64).reshape(-1, 3)
            if len(colors) != len(points):
                raise ValueError(f"{len(points)} points but {len(colors)} colours")
        self.points, self.colors, self.normals = points, colors, None

    def sor_filter(self, nb_neighbors: int = 10, std_ratio: float = 3.0, engine=None):
        """Statistical outlier removal in place (points, colours and normals), on the device."""
        from ..utils.point_cloud_filters import remove_statistical_outlier
        self.points, ind = remove_statistical_outlier(self.points, nb_neighbors, std_ratio, engine=engine)
        if self.colors is not None:
            self.colors = self.colors[ind]
        if self.normals is not None:
            self.normals = self.normals[ind]
        for name in PLY_SCALARS:                              # the per-point scalars stay aligned with the points
            if getattr(self, name) is not None:
                setattr(self, name, getattr(self, name)[ind])
        if self._verbose:
            logger.info("Point cloud filtered by Statistical Oulier Removal")

    def estimate_normals(self, radius: float = 1.0, max_nn: int = 30, engine=None) -> np.ndarray:
        """Normals of the hybrid neighbourhoods (`open3d_fun.py:178-180`), on the device; stored and returned."""
        from ..utils.point_cloud_filters import estimate_normals
        self.normals = estimate_normals(self.points, radius=radius, max_nn=max_nn, engine=engine)
        return self.normals

    def compute_point_cloud_distance(self, target, engine=None) -> np.ndarray:
        """For every point its distance to the nearest point of `target` (a `PointCloud` or [n, 3] array), [n] float64, on the device
        (Open3D's name; `post_processing/cloud_distance.py`, whose definition it is: parity with an Open3D binary is unpinned)."""
        from ..post_processing.cloud_distance import cloud_to_cloud_distance
        return cloud_to_cloud_distance(self.points, target, engine=engine).distance

    def transform(self, T, engine=None) -> "PointCloud":
        """A new cloud under the rigid 4x4 `T` (last row (0, 0, 0, 1)), on the device (`utils/transformations.py`, csrc/icp.hip): the
        points transformed, the normals rotated without the translation, the colours kept."""
        from ..utils.transformations import check_transform, transform_points
        T = check_transform(T)
        out = PointCloud(points3d=transform_points(T, self.points, engine=engine), points_col=self.colors, verbose=self._verbose)
        if self.normals is not None:
            out.normals = transform_points(T, np.ascontiguousarray(self.normals, np.float64), as_vectors=True, engine=engine)
        return out

    def voxel_down_sample(self, voxel_size: float, engine=None) -> "PointCloud":
        """A new cloud with one point per filled voxel: the mean of the voxel's points, colours and normals (`utils/point_cloud_filters.py`,
        csrc/voxel.hip), in ascending voxel key."""
        from ..utils.point_cloud_filters import voxel_down_sample
        points, colors, normals, _, _ = voxel_down_sample(self.points, voxel_size, self.colors, self.normals, engine=engine)
        out = PointCloud(points3d=points, points_col=colors, verbose=self._verbose)
        out.normals = normals
        return out

    @staticmethod
    def check_scalars(scalars) -> tuple:
        """The names of `write_ply(scalars=...)` as a tuple; a name that is none of `PLY_SCALARS`, or one named twice, raises ValueError."""
        if isinstance(scalars, str):
            scalars = (scalars,)
        scalars = tuple(scalars)
        for s in scalars:
            if s not in PLY_SCALARS:
                raise ValueError(f"PointCloud: unknown per-point scalar {s!r}; the PLY writer knows {sorted(PLY_SCALARS)}")
        if len(set(scalars)) != len(scalars):
            raise ValueError(f"PointCloud: a per-point scalar is named twice in {scalars}")
        return scalars

    def write_ply(self, path: Union[str, Path], scalars=()) -> bool:
        """Write point cloud to disk as .ply format (module docstring). `scalars` names per-point attributes to write behind the other
        properties, in the order given: "confidence" (`float`) and / or "views" (`uchar`); the cloud must hold them, one per point."""
        scalars = self.check_scalars(scalars)
        n = len(self)
        extra = []
        for s in scalars:
            a = getattr(self, s)
            if a is None or np.shape(a) != (n,):
                raise ValueError(f"PointCloud.write_ply: this cloud holds no {s!r} per point")
            extra.append((s, PLY_SCALARS[s][1], np.asarray(a)))
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
        if self.colors is not None:
            fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        if self.normals is not None:
            fields += [("nx", "<f8"), ("ny", "<f8"), ("nz", "<f8")]
        fields += [(s, t) for s, t, _ in extra]
        rec = np.zeros(n, dtype=np.dtype(fields))
        for s, _, a in extra:
            rec[s] = a
        for j, a in enumerate("xyz"):
            rec[a] = self.points[:, j]
        if self.colors is not None:
            c8 = np.clip(np.round(self.colors * 255.0), 0, 255).astype(np.uint8)
            for j, a in enumerate(("red", "green", "blue")):
                rec[a] = c8[:, j]
        if self.normals is not None:
            for j, a in enumerate(("nx", "ny", "nz")):
                rec[a] = self.normals[:, j]
        with open(path, "wb") as f:
            f.write(ply_header(n, self.colors is not None, self.normals is not None, [(s, PLY_SCALARS[s][0]) for s in scalars]))
            f.write(rec.tobytes())
        return True

    def write_las(self, path: Union[str, Path]) -> bool:
        raise NotImplementedError("writing .las needs laspy, which is not a dependency of this library")
