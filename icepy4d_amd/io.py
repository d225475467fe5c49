"""The two CSV writers of the reference's `io/export2textfile.py` that report an adjusted epoch, under its names, headers and formats:
`write_cameras_to_file` (date, f, omega, phi, kappa per camera) and `write_reprojection_error_to_file` (pandas' `describe()` of the
reprojection residuals per camera), and `reprojection_table` for a whole sequence. The reference takes an `Epoch` object; here the pieces
are passed as they are: a timestamp, the cameras (a dict name -> camera, or a list named p1, p2, ...) and the residuals that
`sfm.bundle_adjust` returns (`BundleResult.residuals`, computed by `im_ba_residuals`)."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from .utils.homography import euler_from_matrix

CAMERA_ITEMS = ["date", "f1", "omega1", "phi1", "kappa1", "f2", "omega2", "phi2", "kappa2"]


def _named(cameras) -> dict:
    return dict(cameras) if isinstance(cameras, dict) else {f"p{i + 1}": c for i, c in enumerate(cameras)}


def write_cameras_to_file(output_path, timestamp, cameras, sep: str = ",") -> None:
    """One row per call, appended; the header is written where the file does not exist yet. Per camera: f = K[1, 1] with two decimals and
    the static x-y-z Euler angles of the POSE's rotation (camera -> world) in degrees with four."""
    output_path = Path(output_path)
    if not output_path.exists():
        with open(output_path, "w") as file:
            file.write(f"{sep.join(CAMERA_ITEMS)}\n")
    with open(output_path, "a") as file:
        file.write(f"{str(timestamp)}")
        for cam in _named(cameras).values():
            f = cam.K[1, 1]
            o, p, k = (np.rad2deg(a) for a in euler_from_matrix(cam.pose[:3, :3]))
            file.write(f"{sep}{f:.2f}{sep}{o:.4f}{sep}{p:.4f}{sep}{k:.4f}")
        file.write("\n")


def residual_frame(residuals, cam_names=("p1", "p2"), track_ids=None):
    """The reference's residual DataFrame: track_id, then x_, y_, norm_ per camera, then global_norm = the mean of the cameras' norms.
    residuals: [n, 2, 3] (x, y, norm per camera, NaN where a camera does not see the point)."""
    import pandas as pd
    res = np.asarray(residuals, np.float64)
    if res.ndim != 3 or res.shape[1:] != (len(cam_names), 3):
        raise ValueError(f"residuals of shape [n, {len(cam_names)}, 3] are expected (got {res.shape})")
    ids = np.arange(len(res)) if track_ids is None else np.asarray(track_ids)
    if len(ids) != len(res):
        raise ValueError("one track id per point is expected")
    frame = pd.DataFrame()
    frame["track_id"] = ids
    for c, key in enumerate(cam_names):
        frame[f"x_{key}"], frame[f"y_{key}"], frame[f"norm_{key}"] = res[:, c, 0], res[:, c, 1], res[:, c, 2]
    frame["global_norm"] = np.mean(frame[[f"norm_{x}" for x in cam_names]].to_numpy(), axis=1) if len(res) else np.zeros(0)
    return frame


def write_reprojection_error_to_file(output_path, timestamp, residuals, cam_names=("p1", "p2"), track_ids=None, sep: str = ",") -> None:
    """One row per call, appended: `describe()` of the residual frame, stacked (statistic by statistic, column by column), every number by
    `str`; the header "ep" and "<statistic>-<column>" is written where the file does not exist yet."""
    stats = residual_frame(residuals, cam_names, track_ids).describe().stack()
    output_path = Path(output_path)
    if not output_path.exists():
        with open(output_path, "w") as f:
            f.write("ep" + sep + f"{sep}".join([f"{x[0]}-{x[1]}" for x in stats.index.to_list()]) + "\n")
    with open(output_path, "a") as f:
        f.write(str(timestamp) + sep + f"{sep}".join([str(x) for x in stats.to_list()]) + "\n")


def reprojection_table(results, timestamps, cam_names=("p1", "p2"), out_path=None, sep: str = ","):
    """The rows of `write_reprojection_error_to_file` for a whole sequence as one DataFrame (index = the timestamps, columns
    "<statistic>-<column>"); `results` are `BundleResult`s or residual arrays. With `out_path` the file is written anew."""
    import pandas as pd
    if len(results) != len(timestamps):
        raise ValueError("one timestamp per result is expected")
    rows = {}
    for r, ts in zip(results, timestamps):
        stats = residual_frame(getattr(r, "residuals", r), cam_names).describe().stack()
        rows[str(ts)] = {f"{x[0]}-{x[1]}": v for x, v in zip(stats.index.to_list(), stats.to_list())}
    table = pd.DataFrame.from_dict(rows, orient="index")
    if out_path is not None:
        out_path = Path(out_path)
        out_path.parent.mkdir(parents=True, exist_ok=True)
        if out_path.exists():
            out_path.unlink()
        for r, ts in zip(results, timestamps):
            write_reprojection_error_to_file(out_path, ts, getattr(r, "residuals", r), cam_names, sep=sep)
    return table
