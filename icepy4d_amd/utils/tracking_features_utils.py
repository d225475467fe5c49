"""Tracked points over epochs (reference `src/icepy4d/utils/tracking_features_utils.py`): `tracked_points_time_series` and
`tracked_dict_to_df` with the reference's names and signatures, over `tracked_points_table`, which builds the whole table from arrays on
the device (csrc/binned.hip: `im_tracked_points`; the one stable sort of the track ids is torch's). The reference walks dicts of
containers in Python and derives the columns with pandas; the table here holds the same columns with the same bits. Every entry point
takes an optional `engine=`; there is no CPU fallback. `tracked_features_time_series` is not provided."""
from datetime import datetime
from typing import NamedTuple

import numpy as np
import torch

from .._lib import ptr
from ..engine import default_engine, to_device

INT_COLS = ("fid", "num_tracked_eps", "ep_ini", "ep_fin", "dt", "index")
F64_COLS = ("X_ini", "Y_ini", "Z_ini", "X_fin", "Y_fin", "Z_fin", "dX", "dY", "dZ", "vX", "vY", "vZ", "V")


class TrackedPoints(NamedTuple):
    """The table of `tracked_dict_to_df` as arrays of one length under the DataFrame's column names, rows in ascending fid. ep_ini /
    ep_fin are epoch indices and dt is in days; `index` is the row's position before the dt / velocity filters (the DataFrame's index);
    `image_points` holds the x_{cam}_ini, y_{cam}_ini, x_{cam}_fin, y_{cam}_fin columns by name; `series` maps every tracked id to its
    ascending list of epoch indices (what `tracked_points_time_series` returns)."""
    fid: np.ndarray
    num_tracked_eps: np.ndarray
    ep_ini: np.ndarray
    ep_fin: np.ndarray
    X_ini: np.ndarray
    Y_ini: np.ndarray
    Z_ini: np.ndarray
    X_fin: np.ndarray
    Y_fin: np.ndarray
    Z_fin: np.ndarray
    dt: np.ndarray
    dX: np.ndarray
    dY: np.ndarray
    dZ: np.ndarray
    vX: np.ndarray
    vY: np.ndarray
    vZ: np.ndarray
    V: np.ndarray
    index: np.ndarray
    image_points: dict
    series: dict

    def columns(self) -> dict:
        """Every column by name, in the DataFrame's order (without the dates), then `index`."""
        d = {k: getattr(self, k) for k in INT_COLS[:4]}
        d.update(self.image_points)
        d.update({k: getattr(self, k) for k in F64_COLS[:6] + ("dt",) + F64_COLS[6:] + ("index",)})
        return d

    def to_dataframe(self, epoch_dict, epochs=None):
        """The reference's DataFrame: its columns, dtypes and index. `epoch_dict` maps an epoch key to its date ("%Y_%m_%d"); `epochs`
        lists the key of every epoch index (default: the indices are the keys)."""
        import pandas as pd
        key = (lambda e: e) if epochs is None else (lambda e, keys=list(epochs): keys[e])
        d = {"fid": self.fid.tolist(), "num_tracked_eps": self.num_tracked_eps.tolist(),
             "ep_ini": [key(e) for e in self.ep_ini.tolist()], "ep_fin": [key(e) for e in self.ep_fin.tolist()]}
        d["date_ini"] = [epoch_dict[e] for e in d["ep_ini"]]
        d["date_fin"] = [epoch_dict[e] for e in d["ep_fin"]]
        d.update(self.image_points)
        for k in F64_COLS[:6]:
            d[k] = getattr(self, k)
        df = pd.DataFrame.from_dict(d)
        df["date_ini"] = pd.to_datetime(df["date_ini"], format="%Y_%m_%d")
        df["date_fin"] = pd.to_datetime(df["date_fin"], format="%Y_%m_%d")
        df["dt"] = pd.to_timedelta(self.dt, unit="D")
        for k in F64_COLS[6:]:
            df[k] = getattr(self, k)
        df.index = pd.Index(self.index, dtype="int64")
        return df


def _pack(track_ids, points3d):
    ids = [np.ascontiguousarray(np.asarray(t).ravel(), dtype=np.int64) for t in track_ids]
    xyz = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3) for p in points3d]
    if len(ids) != len(xyz) or any(len(i) != len(p) for i, p in zip(ids, xyz)):
        raise ValueError("tracked_points_table: every epoch needs as many track ids as points")
    for i in ids:
        if len(np.unique(i)) != len(i):
            raise ValueError("tracked_points_table: a track id occurs more than once in an epoch")
    return ids, xyz


def tracked_points_table(track_ids, points3d, days, min_tracked_epoches=1, volume=None, min_dt=None, vx_lims=None, vy_lims=None, vz_lims=None,
                         image_points=None, engine=None) -> TrackedPoints:
    """`tracked_points_time_series` + `tracked_dict_to_df` of the reference (`tracking_features_utils.py:123-169`, `:219-300`) from
    arrays. Per epoch e: `track_ids[e]` int [n_e] (each id at most once: ValueError otherwise), `points3d[e]` float64 [n_e, 3] (the
    per-epoch lists of `TableReconstruction.points3d` as they are), `days[e]` its integer day number. An id is tracked when it occurs in at
    least `min_tracked_epoches` epochs, counting only the epochs in which its point lies inside `volume` (any [k, 3] array: the
    inclusive box of its minima and maxima). ini / fin are the first / last such epoch; d = fin - ini, dt = day_fin - day_ini,
    v = d / dt (inf / NaN for dt = 0, as pandas), V = |v|. Rows with dt >= `min_dt` and lo <= v < hi for every given `v*_lims` are
    kept. `image_points` {cam: per-epoch [n_e, 2]} adds x_{cam}_ini, y_{cam}_ini, x_{cam}_fin, y_{cam}_fin."""
    ids, xyz = _pack(track_ids, points3d)
    E = len(ids)
    days = np.ascontiguousarray(days, dtype=np.int64).ravel()
    if E < 1 or len(days) != E:
        raise ValueError("tracked_points_table: one day number per epoch is needed")
    cams = tuple(image_points) if image_points else ()
    offs = np.concatenate([[0], np.cumsum([len(i) for i in ids])]).astype(np.int64)
    M = int(offs[-1])
    img = None
    if cams:
        img = np.empty((len(cams), M, 2), np.float64)
        for k, cam in enumerate(cams):
            per_epoch = [np.asarray(a, np.float64).reshape(-1, 2) for a in image_points[cam]]
            if [len(a) for a in per_epoch] != [len(i) for i in ids]:
                raise ValueError(f"tracked_points_table: image points of {cam!r} do not match the track ids")
            img[k] = np.concatenate(per_epoch) if M else np.zeros((0, 2))
    vol = None
    if volume is not None:
        volume = np.asarray(volume, np.float64).reshape(-1, 3)
        vol = np.ascontiguousarray(np.concatenate([volume.min(0), volume.max(0)]))
    lims = np.full((3, 2), np.nan)
    for k, lim in enumerate((vx_lims, vy_lims, vz_lims)):
        if lim is not None:
            lims[k] = [float(lim[0]), float(lim[1])]
            if np.isnan(lims[k]).any():
                raise ValueError("tracked_points_table: velocity limits must be numbers")
    h_min_dt = None if min_dt is None else np.array([int(min_dt)], np.int64)
    eng = default_engine(engine)
    dev = eng.device
    d_ids, d_xyz = to_device(np.concatenate(ids) if M else np.zeros(0, np.int64), dev), to_device(np.concatenate(xyz) if M else np.zeros((0, 3)), dev)
    d_img = to_device(img, dev) if cams else None
    d_offs, d_days = to_device(offs, dev), to_device(days, dev)
    sid, perm = torch.sort(d_ids, stable=True)             # rows are concatenated by epoch: stable by id = ordered by (id, epoch)
    n_f64 = len(F64_COLS) + 4 * len(cams)
    oi = torch.empty((len(INT_COLS), M), dtype=torch.int64, device=dev)
    od = torch.empty((n_f64, M), dtype=torch.float64, device=dev)
    member = torch.empty(M, dtype=torch.uint8, device=dev)
    n_rows = torch.zeros(1, dtype=torch.int64, device=dev)
    eng.ctx.call("im_tracked_points", ptr(sid), ptr(perm), M, ptr(d_offs), E, ptr(d_xyz), ptr(d_days), None if vol is None else vol.ctypes.data,
                 int(min_tracked_epoches), None if h_min_dt is None else h_min_dt.ctypes.data, lims.ctypes.data, ptr(d_img), len(cams), ptr(oi),
                 ptr(od), ptr(member), ptr(n_rows), eng.stream_ptr())
    R = int(n_rows.item())
    hi, hd, hm = oi[:, :R].cpu().numpy(), od[:, :R].cpu().numpy(), member.cpu().numpy().astype(bool)
    cols = {k: np.ascontiguousarray(hi[j]) for j, k in enumerate(INT_COLS)}
    cols.update({k: np.ascontiguousarray(hd[j]) for j, k in enumerate(F64_COLS)})
    image_cols = {}
    for c, cam in enumerate(cams):
        for j, k in enumerate((f"x_{cam}_ini", f"y_{cam}_ini", f"x_{cam}_fin", f"y_{cam}_fin")):
            image_cols[k] = np.ascontiguousarray(hd[len(F64_COLS) + 4 * c + j])
    # the series of the tracked ids from the member rows: ascending id, ascending epoch
    rows = np.flatnonzero(hm)
    all_ids = np.concatenate(ids) if M else np.zeros(0, np.int64)
    ep_of = np.searchsorted(offs, rows, side="right") - 1
    order = np.lexsort((ep_of, all_ids[rows]))
    series = {}
    for i, e in zip(all_ids[rows][order].tolist(), ep_of[order].tolist()):
        series.setdefault(i, []).append(e)
    return TrackedPoints(image_points=image_cols, series=series, **cols)


def _pack_containers(points, keep=None):
    """dict epoch -> container (`get_track_ids()`, `[id].coordinates`) -> per-epoch ids and [n, 3] coordinates; keep(ep, id) filters."""
    epoches = list(points.keys())
    ids, xyz = [], []
    for ep in epoches:
        tid = [t for t in points[ep].get_track_ids() if keep is None or keep(ep, t)]
        ids.append(np.asarray(tid, np.int64))
        xyz.append(np.asarray([np.asarray(points[ep][t].coordinates, np.float64).reshape(3) for t in tid], np.float64).reshape(-1, 3))
    return epoches, ids, xyz


def tracked_points_time_series(points, min_tracked_epoches=1, volume=None, engine=None) -> dict:
    """`tracked_points_time_series` of the reference (`:123-169`): {track id: the epochs in which the point was tracked (inside
    `volume`)}, for the ids tracked in at least `min_tracked_epoches` epochs, in ascending id."""
    epoches, ids, xyz = _pack_containers(points)
    t = tracked_points_table(ids, xyz, np.arange(len(epoches)), min_tracked_epoches=min_tracked_epoches, volume=volume, engine=engine)
    return {i: [epoches[e] for e in eps] for i, eps in t.series.items()}


def tracked_dict_to_df(features, points, epoch_dict, fts, min_dt=None, vx_lims=None, vy_lims=None, vz_lims=None, save_path=None, engine=None):
    """`tracked_dict_to_df` of the reference (`:219-300`): the DataFrame of the tracked ids `fts` ({id: epochs}, as
    `tracked_points_time_series` returns it) with the first / last position, the displacement, dt, the velocities and |V|, filtered by
    `min_dt` (days) and the velocity limits. `features` {epoch: {cam: container}} gives x / y of every id at ini and fin."""
    epoches = list(points.keys())
    cams = list(features[list(features.keys())[0]].keys())
    in_series = {(ep, i) for i, eps in fts.items() for ep in eps}
    _, ids, xyz = _pack_containers(points, keep=lambda ep, i: (ep, i) in in_series)
    img = {cam: [np.asarray([[features[ep][cam][i].x, features[ep][cam][i].y] for i in tid.tolist()], np.float64).reshape(-1, 2)
                 for ep, tid in zip(epoches, ids)] for cam in cams}
    days = [datetime.strptime(epoch_dict[ep], "%Y_%m_%d").toordinal() for ep in epoches]
    t = tracked_points_table(ids, xyz, days, min_dt=min_dt, vx_lims=vx_lims, vy_lims=vy_lims, vz_lims=vz_lims, image_points=img, engine=engine)
    df = t.to_dataframe(epoch_dict, epochs=epoches)
    order = list(fts.keys())
    if order != sorted(order):                                   # the reference keeps the order of `fts`
        pos = {i: k for k, i in enumerate(order)}
        df = df.iloc[np.argsort([pos[i] for i in df["fid"]], kind="stable")]
        df.index = [pos[i] for i in df["fid"]]
    if save_path is not None:
        df.to_csv(save_path)
    return df
