"""The glacier's top border from a dense cloud, with the names of the reference's `scripts/pcd_postprocessing/top_border.py`, on the
device. The script asks CloudCompare for Linearity over balls of 2 m and Verticality over balls of 0.15 m on every point, keeps the 95-100
percentile of each in turn, then the 60-95 percentile of z, and reduces the border's points inside a y window and within 10 m of their
median x to mean / median / std per axis, one CSV row per epoch: the border's retreat from epoch to epoch.

The features are `utils/point_cloud_filters.ball_features` (csrc/ballfeat.hip; both on the full cloud), with a definition of their own:
PARITY WITH A CLOUDCOMPARE BINARY IS UNPINNED. The order of the filters, the call arguments and the row format are the
script's, pinned by tests/golden/g18_top_border.npz. The percentiles are `np.nanpercentile` on the host, on eight bytes per point."""
import warnings
from pathlib import Path

import numpy as np

from .core.point_cloud import PointCloud
from .post_processing.cloudcompare_fun import GeomFeature, compute_feature, filter_by_sf_value
from .post_processing.open3d_fun import select_by_index

FEATURES = (GeomFeature.Linearity, GeomFeature.Verticality)          # the script's, one per radius of `radius_list`
HEADER = "pcd_name,date,x_mean,x_median,x_std,y_mean,y_median,y_std,z_mean,z_median,z_std"
BORDER_PREFIX = "border_"                                            # the script names its border clouds border_<date>.ply


def _load(pcd) -> PointCloud:
    if isinstance(pcd, PointCloud):
        return pcd
    if isinstance(pcd, (str, bytes)) or hasattr(pcd, "__fspath__"):
        try:
            return PointCloud(pcd_path=pcd)
        except (OSError, ValueError, KeyError) as e:
            raise IOError(f"Unable to read point cloud {pcd}") from e
    return PointCloud(points3d=np.asarray(pcd, np.float64))


def percentile_window(values, lim):
    """(lo, hi) = the two nanpercentiles of `values`; (NaN, NaN), which keeps nothing, where no value is finite."""
    v = np.asarray(values, np.float64).reshape(-1)
    if v.size == 0 or np.isnan(v).all():
        return np.nan, np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return float(np.nanpercentile(v, lim[0])), float(np.nanpercentile(v, lim[1]))


def border_indices(points, features, lim_percentile=(95, 100), z_percentile=(60, 95)) -> np.ndarray:
    """The script's chain on per-point feature columns (each [n], computed on the full cloud): the indices (ascending, into `points`)
    that survive the percentile window of the first feature, then that of the second taken over the survivors, and so on, then the
    window of z over the survivors."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    keep = np.arange(len(points), dtype=np.int64)
    for column in features:
        v = np.asarray(column, np.float64)[keep]
        keep = keep[filter_by_sf_value(v, *percentile_window(v, lim_percentile))]
    z = points[keep, 2]
    return keep[filter_by_sf_value(z, *percentile_window(z, z_percentile))]


def detect_border_by_geometry(pcd, radius_list=(2.0, 0.15), lim_percentile=(95, 100), z_percentile=(60, 95), engine=None) -> PointCloud:
    """The border cloud of `pcd` (a `.ply` path, a `core.PointCloud` or an [n, 3] array): Linearity at radius_list[0] and Verticality at
    radius_list[1], both on the full cloud, then `border_indices`. Colours and normals follow the points."""
    if len(radius_list) != len(FEATURES):
        raise ValueError(f"radius_list holds one radius per feature {[f.name for f in FEATURES]}")
    pcd = _load(pcd)
    columns = [compute_feature(f, r, pcd, engine=engine) for f, r in zip(FEATURES, radius_list)]
    return select_by_index(pcd, border_indices(pcd.points, columns, lim_percentile, z_percentile))


def extract_glacier_border(border, ylims=(224.0, 228.0), half_width=10.0) -> dict:
    """The script's reduction of a border cloud: the points with ylims[0] <= y <= ylims[1], of those the ones within `half_width` of their
    median x, and mean / median / std (population) per axis: {"x_mean", "x_median", "x_std", "y_mean", ..., "z_std", "n", "cloud"}.
    An empty result gives NaN throughout."""
    border = _load(border)
    inside = select_by_index(border, filter_by_sf_value(border.points[:, 1], ylims[0], ylims[1]))
    if len(inside):
        median_x = np.median(inside.points[:, 0])
        inside = select_by_index(inside, filter_by_sf_value(inside.points[:, 0], median_x - half_width, median_x + half_width))
    out = {"n": len(inside), "cloud": inside}
    coords = inside.points
    for j, a in enumerate("xyz"):
        col = coords[:, j]
        out[f"{a}_mean"], out[f"{a}_median"], out[f"{a}_std"] = (float(np.mean(col)), float(np.median(col)), float(np.std(col))) if len(col) \
            else (np.nan, np.nan, np.nan)
    return out


def format_row(name: str, date: str, stats: dict) -> str:
    """One row of the script's file: three decimals, or the script's literal NaN row for an empty border."""
    keys = [f"{a}_{s}" for a in "xyz" for s in ("mean", "median", "std")]
    if stats["n"] == 0:
        return ",".join([name, date] + ["NaN"] * len(keys))
    return ",".join([name, date] + [f"{stats[k]:.3f}" for k in keys])


def border_table(paths_or_clouds, out_path=None, names=None, ylims=(224.0, 228.0), half_width=10.0):
    """The script's table of a series of border clouds (paths of `border_<date>.ply` files, `core.PointCloud`s or arrays): a DataFrame
    with the columns of HEADER, and, when `out_path` is given, the script's CSV file. `names`: the pcd_name of each cloud that is not a
    path (default pcd<k>); the date is the name's stem without `border_`."""
    import pandas as pd
    lines, rows = [], []
    for k, item in enumerate(paths_or_clouds):
        is_path = isinstance(item, (str, bytes)) or hasattr(item, "__fspath__")
        name = Path(item).name if is_path else (names[k] if names is not None else f"pcd{k}")
        stem = Path(name).stem
        date = stem.replace(BORDER_PREFIX, "")
        stats = extract_glacier_border(item, ylims=ylims, half_width=half_width)
        lines.append(format_row(name, date, stats))
        rows.append([name, date] + [stats[f"{a}_{s}"] for a in "xyz" for s in ("mean", "median", "std")])
    if out_path is not None:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join([HEADER] + lines) + "\n")
    return pd.DataFrame(rows, columns=HEADER.split(","))
