"""`DemOfDifference` with the reference's names (`src/icepy4d/post_processing/cloudcompare_fun.py`), on the device: the reference goes
through CloudComPy (`cc.ComputeVolume25D`), which is not a dependency; the 2.5D volume has a definition of its own here
(`icepy4d_amd/volume_variations.py`, DESIGN §4, csrc/dod.hip). PARITY WITH A CLOUDCOMPARE BINARY IS UNPINNED. A series of pairs is served
faster by `volume_variations.dod_series`, which uploads every cloud once.

`GeomFeature`, `compute_feature` and `filter_by_sf_value` stand in for CloudComPy's `GeomFeature`, `computeFeature` and `filterBySFValue`
as `scripts/pcd_postprocessing/top_border.py` uses them (`icepy4d_amd/top_border.py`); the features are those of
`utils/point_cloud_filters.ball_features` (csrc/ballfeat.hip), with the same caveat about a CloudCompare binary."""
import enum
from pathlib import Path
from typing import Union

import numpy as np

from ..core.point_cloud import PointCloud
from ..volume_variations import cloud_points, direction_index, dod_series, format_row
from .open3d_fun import crop_indices, read_polyline, select_by_index

ALLOWED_PCD_EXT = [".asc", ".las", ".E57", ".ply", ".pcd", ".bin"]
HEADER = "pcd0,pcd1,volume,addedVolume,removedVolume,surface,matchingPercent,averageNeighborsPerCell\n"


class GeomFeature(enum.Enum):
    """CloudCompare's geometric features by its member names (the numbering is CCCoreLib's as recalled, from 1; nothing here depends on
    it). `NumberOfNeighbors` is CloudCompare's neighbour count at the same radius, listed with them."""
    EigenValuesSum = 1
    Omnivariance = 2
    EigenEntropy = 3
    Anisotropy = 4
    Planarity = 5
    Linearity = 6
    PCA1 = 7
    PCA2 = 8
    SurfaceVariation = 9
    Sphericity = 10
    Verticality = 11
    EigenValue1 = 12
    EigenValue2 = 13
    EigenValue3 = 14
    NumberOfNeighbors = 15


def compute_feature(feature, radius: float, pcd, engine=None) -> np.ndarray:
    """One feature ([n] float64, NaN where the ball defines none) of every point of `pcd` (a `.ply` path, a `core.PointCloud` or an
    [n, 3] array) over the ball of `radius`, on the device. `feature`: a `GeomFeature` or its name."""
    from ..utils.point_cloud_filters import ball_features
    name = feature.name if isinstance(feature, GeomFeature) else GeomFeature[str(feature)].name
    return ball_features(_as_cloud(pcd).points, radius, features=(name,), engine=engine)[name]


def filter_by_sf_value(values, lo: float, hi: float) -> np.ndarray:
    """The ascending indices (int64) of the values with lo <= v <= hi; NaN is dropped, as is everything when a limit is NaN."""
    v = np.asarray(values, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return np.nonzero((v >= lo) & (v <= hi))[0].astype(np.int64)


def _as_cloud(pcd) -> PointCloud:
    return pcd if isinstance(pcd, PointCloud) else PointCloud(points3d=cloud_points(pcd))


def cut_point_cloud_by_polyline(pcd, polyline_path: str, direction: str = "z", inside: bool = True, output_pah: Union[str, Path] = None,
                                delete_original: bool = False, engine=None) -> PointCloud:
    """Crop a cloud by the closed polyline of `polyline_path` (rows "x y z"), on the device. The reference marks its version "currently
    not working" (it hands CloudComPy's `crop2D` the axis below); this one works, and keeps the reference's mapping of `direction` to the
    axis the crop looks along, SWAPPED x / y INCLUDED: "y" -> axis 0, "x" -> axis 1, "z" -> axis 2. The polygon is the polyline's other two
    coordinates, in file order; `inside=False` keeps the points outside. `output_pah`: a .ply path the result is also written to."""
    assert direction in ["x", "y", "z"], \
        "Invalid direction provided. Provide the name of the axis as a string. The following directions are allowed: ['x', 'y', 'z']"
    axis = {"y": 0, "x": 1, "z": 2}[direction]
    ax, ay = [a for a in (0, 1, 2) if a != axis]
    pcd = _as_cloud(pcd)
    poly = read_polyline(polyline_path)[:, [ax, ay]]
    cropped = select_by_index(pcd, crop_indices(pcd.points, poly, ax, ay, inside=inside, engine=engine))
    if output_pah is not None:
        output_pah = Path(output_pah)
        assert output_pah.suffix in ALLOWED_PCD_EXT, f"Invalid point cloud extension. It must be one of the followings {ALLOWED_PCD_EXT}"
        if output_pah.suffix != ".ply":
            raise IOError(f"Unable to save cropped point cloud to {output_pah}.")
        cropped.write_ply(output_pah)
    return cropped


class DemOfDifference:
    """`pcd_pair`: two clouds (ground, ceil), each a `.ply` path, a `core.PointCloud` or an [n, 3] array."""

    def __init__(self, pcd_pair) -> None:
        self.pcd_pair = pcd_pair
        self.pcd0 = _as_cloud(pcd_pair[0])          # a path that cannot be read: IOError
        self.pcd1 = _as_cloud(pcd_pair[1])
        self.report = None
        self._raster = None

    def compute_volume(self, direction: str = "x", grid_step: float = 1, engine=None) -> bool:
        self.direction = direction_index(direction)
        reports, rasters = dod_series([self.pcd0, self.pcd1], [(0, 1)], direction=direction, grid_step=grid_step, engine=engine, rasters=True)
        self.report, self._raster = reports[0], rasters[0]
        return True

    def grid(self):
        """(H [h, w] float64 with NaN outside, (min_x, min_y), step) of the last `compute_volume`."""
        if self._raster is None:
            raise RuntimeError("compute_volume() has not run")
        return self._raster

    def cut_point_clouds_by_polyline(self, polyline_path: str, direction: str = "x", engine=None) -> None:
        """Both clouds cropped by `cut_point_cloud_by_polyline` (the reference's direction mapping, swapped x / y included)."""
        self.pcd0 = cut_point_cloud_by_polyline(self.pcd0, polyline_path, direction, engine=engine)
        self.pcd1 = cut_point_cloud_by_polyline(self.pcd1, polyline_path, direction, engine=engine)

    def print_result(self) -> None:
        """The six figures the reference prints, one per line."""
        r = self.report
        lines = [("Volume", r.volume, "m3"), ("Added volume", r.addedVolume, "m3"), ("Removed volume", r.removedVolume, "m3"),
                 ("Surface", r.surface, "m2")]
        print("Volume variation report:")
        for label, value, unit in lines:
            print(f"    {label}: {value:.2f} {unit}")
        print(f"    Matching percent: {r.matchingPercent:.1f} %")
        print(f"    Average neighbours per cell: {r.averageNeighborsPerCell:.1f}")

    def clear(self):
        """Drop the clouds, the raster and the report."""
        self.pcd0 = self.pcd1 = None
        self.report = self._raster = None

    def _names(self):
        return [Path(p).stem if isinstance(p, (str, Path)) else f"pcd{k}" for k, p in enumerate(self.pcd_pair)]

    def write_result_to_file(self, fname: str, mode="a+", header=True):
        """One CSV row behind what the file holds. The header line is written when `header` is True, except when an existing file is
        appended to (mode "a" or "a+"): the reference's rule, which g17 records."""
        appending = mode in ("a", "a+") and Path(fname).exists()
        text = format_row(*self._names(), self.report)
        if header is True and not appending:
            text = HEADER + text
        with open(fname, mode=mode) as f:
            f.write(text)
