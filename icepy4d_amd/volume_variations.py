"""Volume variations between the clouds of a series, on the device: the reference's `scripts/pcd_postprocessing/volume_variations.py`
(one pool process per pair around CloudCompare's `ComputeVolume25D`, every cloud read from disk twice, one CSV row per pair, daily and
cumulated volumes with pandas) as two functions. `dod_series` uploads every cloud once and serves all pairs with one pass of
csrc/dod.hip (`im_dod_bounds`, `im_dod_keys`, torch's stable sort, `im_dod_reduce`); `dod_table` derives the reference's DataFrame. The
reference's plots are not provided. No CPU fallback: without a HIP device `dod_series` raises.

The definition (tests/dod_oracle.py, bit-identical): float64 coordinates, a point with a non-finite coordinate ignored, the
grid of a pair over the union box of its kept points with cells centred on min + k * step, the mean height per cloud and cell summed in
ascending point index, H = mean_ceil - mean_ground where both clouds fill a cell, the sums over cells in chunks of `chunk()` cells.
PARITY WITH A CLOUDCOMPARE BINARY IS UNPINNED: CloudCompare stores float32 coordinates after a global shift and sums in its own order."""
import numpy as np
import torch

from ._lib import load, ptr
from .engine import default_engine, to_device

DIRECTIONS = {"x": 0, "y": 1, "z": 2}
FIELDS = ("volume", "addedVolume", "removedVolume", "surface", "matchingPercent", "groundNonMatchingPercent", "ceilNonMatchingPercent",
          "averageNeighborsPerCell", "validCells", "cellCount", "gridWidth", "gridHeight", "minX", "minY", "step", "cellArea")
INTEGER_FIELDS = ("validCells", "cellCount", "gridWidth", "gridHeight")
CSV_COLUMNS = ["pcd0", "pcd1", "volume", "addedVolume", "removedVolume", "surface", "matchingPercent", "averageNeighborsPerCell"]


class ReportInfoVol:
    """The figures of one pair, named as the reference reads them off `cc.ReportInfoVol`, plus groundNonMatchingPercent,
    ceilNonMatchingPercent, gridWidth, gridHeight, validCells, cellCount, minX, minY, step, cellArea, droppedGround and droppedCeil (the
    points ignored for a non-finite coordinate)."""

    def __init__(self, row, dropped=(0, 0)):
        for name, v in zip(FIELDS, np.asarray(row, np.float64)):
            setattr(self, name, int(v) if name in INTEGER_FIELDS else float(v))
        self.droppedGround, self.droppedCeil = int(dropped[0]), int(dropped[1])

    def as_dict(self):
        return {k: getattr(self, k) for k in FIELDS + ("droppedGround", "droppedCeil")}

    def __repr__(self):
        return f"ReportInfoVol(volume={self.volume!r}, surface={self.surface!r}, matchingPercent={self.matchingPercent!r})"


def chunk() -> int:
    """B: the cells of one chunk of the three sums over cells."""
    return int(load().im_dod_chunk())


def max_cells() -> int:
    """The largest grid (in cells) of a pair."""
    return int(load().im_dod_max_cells())


def max_batch_cells() -> int:
    """The most cells the grids of one call hold together; `dod_series` splits longer series."""
    return int(load().im_dod_max_batch_cells())


def direction_index(direction) -> int:
    assert direction in ["x", "y", "z"], \
        "Invalid direction provided. Provide the name of the axis as a string. The following directions are allowed: ['x', 'y', 'z']"
    return DIRECTIONS[direction]


def cloud_points(cloud) -> np.ndarray:
    """[n, 3] float64 of a `.ply` path, a `core.PointCloud` or an array. A path that cannot be read raises IOError, as the reference does."""
    from .core.point_cloud import PointCloud, read_ply
    if isinstance(cloud, PointCloud):
        return np.ascontiguousarray(cloud.get_points(), np.float64).reshape(-1, 3)
    if isinstance(cloud, (str, bytes)) or hasattr(cloud, "__fspath__"):
        try:
            return np.ascontiguousarray(read_ply(cloud)[0], np.float64).reshape(-1, 3)
        except (OSError, ValueError, KeyError) as e:
            raise IOError(f"Unable to read point cloud {cloud}") from e
    a = cloud.detach().cpu().numpy() if isinstance(cloud, torch.Tensor) else np.asarray(cloud)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"a cloud must be [n, 3] (got {a.shape})")
    return np.ascontiguousarray(a, np.float64)


def check_arguments(n_clouds, pairs, direction, grid_step):
    """(vertDim, step, pairs [P, 2] int32) or the exception of a bad argument, before any device work."""
    d = direction_index(direction)
    step = float(grid_step)
    if not (np.isfinite(step) and step > 0.0):
        raise ValueError(f"grid_step must be finite and positive (got {grid_step})")
    pairs = np.asarray(list(pairs), np.int64).reshape(-1, 2)
    if len(pairs) and (pairs.min() < 0 or pairs.max() >= n_clouds):
        raise ValueError(f"a pair names a cloud outside 0..{n_clouds - 1}")
    return d, step, np.ascontiguousarray(pairs, np.int32)


def _batches(cells, items, cap):
    """consecutive runs of pairs whose grids hold at most `cap` cells and fewer than 2^31 points"""
    out, cur, c, n = [], [], 0, 0
    for p, (pc, pn) in enumerate(zip(cells, items)):
        if cur and (c + pc > cap or n + pn >= 2 ** 31):
            out.append(cur)
            cur, c, n = [], 0, 0
        cur.append(p)
        c, n = c + pc, n + pn
    return out + ([cur] if cur else [])


def dod_series(clouds, pairs, direction="x", grid_step=0.3, engine=None, rasters=False):
    """The DEM of difference of every pair (ground, ceil) of indices into `clouds` (paths, `PointCloud`s or [n, 3] arrays): a list of
    `ReportInfoVol`, one per pair; with `rasters=True` also the list of (H [h, w] float64 with NaN outside, (min_x, min_y), step) per pair,
    H[j, i] the cell centred on (min_x + i * step, min_y + j * step) along the axes X = (d + 1) % 3 and Y = (d + 2) % 3 of direction d.
    Every cloud is uploaded once; one device pass serves all pairs (series whose grids exceed the library's batch limit are split)."""
    host = [cloud_points(c) for c in clouds]
    d, step, pairs = check_arguments(len(host), pairs, direction, grid_step)
    P, E = len(pairs), len(host)
    if P == 0:
        return ([], []) if rasters else []
    eng = default_engine(engine)
    dev, st = eng.device, eng.stream_ptr()
    offsets = np.concatenate([[0], np.cumsum([len(a) for a in host])]).astype(np.int64)
    pts = to_device(np.concatenate(host + [np.zeros((0, 3))]), dev, np.float64)
    d_bounds = torch.empty((E, 4), dtype=torch.float64, device=dev)
    d_dropped = torch.empty(E, dtype=torch.int64, device=dev)
    eng.ctx.call("im_dod_bounds", ptr(pts), offsets.ctypes.data, E, d, ptr(d_bounds), ptr(d_dropped), st)
    bounds, dropped = np.ascontiguousarray(d_bounds.cpu().numpy()), d_dropped.cpu().numpy()

    def keys(sub, want_key=True):
        grids = np.zeros((len(sub), 4), np.float64)
        items = int(sum(offsets[c + 1] - offsets[c] for c in sub.ravel()))
        key = torch.empty(items, dtype=torch.int64, device=dev) if want_key else None
        eng.ctx.call("im_dod_keys", ptr(pts), offsets.ctypes.data, E, sub.ctypes.data, len(sub), d, step, bounds.ctypes.data, grids.ctypes.data,
                     ptr(key), st)
        return grids, key

    sizes = [int(offsets[g + 1] - offsets[g] + offsets[c + 1] - offsets[c]) for g, c in pairs]
    cells = [int(np.prod(keys(np.ascontiguousarray(pairs[p:p + 1]), False)[0][0, 2:])) for p in range(P)]      # host only: the grids decide the batches
    reports, grids_all, H_all = np.zeros((P, len(FIELDS))), np.zeros((P, 4)), [None] * P
    for batch in _batches(cells, sizes, max_batch_cells()):
        sub = np.ascontiguousarray(pairs[batch])
        grids, key = keys(sub)
        skey, perm = torch.sort(key, stable=True)
        n_cells = (grids[:, 2] * grids[:, 3]).astype(np.int64)
        d_H = torch.empty(int(n_cells.sum()), dtype=torch.float64, device=dev) if rasters else None
        d_report = torch.empty((len(sub), len(FIELDS)), dtype=torch.float64, device=dev)
        eng.ctx.call("im_dod_reduce", ptr(pts), offsets.ctypes.data, E, sub.ctypes.data, len(sub), d, step, bounds.ctypes.data, ptr(skey), ptr(perm),
                     ptr(d_H), ptr(d_report), st)
        reports[batch], grids_all[batch] = d_report.cpu().numpy(), grids
        if rasters:
            flat, at = d_H.cpu().numpy(), np.concatenate([[0], np.cumsum(n_cells)])
            for k, p in enumerate(batch):
                H_all[p] = flat[at[k]:at[k + 1]].reshape(int(grids[k, 3]), int(grids[k, 2]))
    out = [ReportInfoVol(reports[p], (dropped[pairs[p, 0]], dropped[pairs[p, 1]])) for p in range(P)]
    if rasters:
        return out, [(H_all[p], (float(grids_all[p, 0]), float(grids_all[p, 1])), step) for p in range(P)]
    return out


def format_row(name0, name1, report) -> str:
    """One row of the CSV of `DemOfDifference.write_result_to_file`: the two names, four figures with 4 decimals, two with 1."""
    figures = [(report.volume, 4), (report.addedVolume, 4), (report.removedVolume, 4), (report.surface, 4), (report.matchingPercent, 1),
               (report.averageNeighborsPerCell, 1)]
    return ",".join([str(name0), str(name1)] + [f"{v:.{digits}f}" for v, digits in figures]) + "\n"


DERIVED_COLUMNS = ["date_in", "date_fin", "dt", "volume_daily", "volume_daily_normalized", "volume_daily_cumul", "volume_daily_norm_cumul"]


def dod_table(reports_or_csv, names=None, dates=None, date_format="%Y_%m_%d", prefix=None):
    """The table the reference's script derives from its CSV, as a DataFrame sorted by date_in: the CSV's eight columns, then
    DERIVED_COLUMNS: date_in and date_fin, dt = their distance in days, volume_daily = volume / dt, volume_daily_normalized =
    volume_daily / matchingPercent * (the largest matchingPercent of the table), and the running sums of the last two.
    `reports_or_csv`: the path of a CSV written by `write_result_to_file` without a header, or a list of reports with `names` = the
    (pcd0, pcd1) stems of every pair. `dates` = (date_in, date_fin) per pair when given; otherwise both are read off the stems with
    `date_format`, after `prefix + "_"` has been removed from them."""
    import pandas as pd
    if isinstance(reports_or_csv, (str, bytes)) or hasattr(reports_or_csv, "__fspath__"):
        table = pd.read_csv(reports_or_csv, sep=",", names=CSV_COLUMNS)
    else:
        figures = [[r[k] if isinstance(r, dict) else getattr(r, k) for k in CSV_COLUMNS[2:]] for r in reports_or_csv]
        table = pd.DataFrame([list(n) + f for n, f in zip(names, figures)], columns=CSV_COLUMNS)

    def stem_dates(column):
        stems = table[column].astype(str)
        if prefix is not None:
            stems = stems.str.replace(prefix + "_", "", regex=False)
        return pd.to_datetime(stems, format=date_format)

    if dates is None:
        start, end = stem_dates("pcd0"), stem_dates("pcd1")
    else:
        start = pd.Series(pd.to_datetime([a for a, _ in dates]), index=table.index)
        end = pd.Series(pd.to_datetime([b for _, b in dates]), index=table.index)
    table = table.assign(date_in=start, date_fin=end).sort_values("date_in")
    days = (table["date_fin"] - table["date_in"]).dt.total_seconds() / 86400.0
    daily = table["volume"] / days
    best_match = table["matchingPercent"].max() if len(table) else np.nan
    normalised = daily / table["matchingPercent"] * best_match
    return table.assign(dt=days, volume_daily=daily, volume_daily_normalized=normalised, volume_daily_cumul=daily.cumsum(),
                        volume_daily_norm_cumul=normalised.cumsum())
