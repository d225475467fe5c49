"""Change detection between the clouds of a series, on the device: M3C2 (`post_processing/cloud_distance.py`) for every pair of epochs, in
the shape of `volume_variations.py`. `m3c2_series` uploads and bins every cloud once and serves all pairs; `m3c2_table` condenses the
per-point results into one row per pair. The reference has no counterpart (its scripts stop at the DEM of difference); the definitions
are this library's own and parity with CloudCompare's M3C2 plugin is unpinned (see that module). No CPU fallback: without a HIP device
`m3c2_series` raises.

M3C2 assumes both epochs in one frame. `coregister_series` brings them there first: an ICP (`post_processing/registration.py`) of every epoch
onto a reference epoch over the points inside a stable-ground polygon, and `coregistration_table` reports it, one row per epoch."""
import math

import numpy as np
import torch

from .engine import default_engine
from .post_processing.cloud_distance import M3C2Result, check_m3c2, m3c2
from .post_processing.registration import ICPConvergenceCriteria, check_registration, registration_icp
from .utils.point_cloud_filters import bin_cloud
from .volume_variations import cloud_points

CSV_COLUMNS = ["pcd0", "pcd1", "n_core", "n_distance", "n_significant", "mean", "median", "std", "lod_mean"]
HEADER = ",".join(CSV_COLUMNS)


def m3c2_series(clouds, pairs, engine=None, **m3c2_kwargs):
    """M3C2 of every pair (first, second) of indices into `clouds` (paths, `PointCloud`s, [n, 3] arrays or tensors), e.g. the indices behind
    `post_processing.make_pairs`: a list of `M3C2Result`, one per pair, equal to the per-pair call `m3c2(clouds[first], clouds[second],
    **m3c2_kwargs)`. Every cloud a pair names is uploaded and binned once. The core points of a pair are the first cloud's own points
    unless `core_points` is given. numpy results unless the first cloud of a pair is a tensor. The clouds are taken as they are, in one
    frame: `registration_error` wants the `inlier_rmse` of their co-registration (`coregister_series`, `registration_icp`)."""
    check_m3c2(m3c2_kwargs.get("normal_scale"), m3c2_kwargs.get("search_scale"), m3c2_kwargs.get("search_depth"),
               m3c2_kwargs.get("registration_error", 0.0), m3c2_kwargs.get("min_points", 5))
    pairs = np.asarray(list(pairs), np.int64).reshape(-1, 2)
    if len(pairs) and (pairs.min() < 0 or pairs.max() >= len(clouds)):
        raise ValueError(f"a pair names a cloud outside 0..{len(clouds) - 1}")
    eng = default_engine(engine)
    binned = {}
    for i in sorted(set(pairs.ravel().tolist())):
        c = clouds[i]
        binned[i] = bin_cloud(c if isinstance(c, torch.Tensor) else cloud_points(c), float(m3c2_kwargs["search_scale"]) / 2.0, engine=eng)
    explicit = m3c2_kwargs.get("core_points") is not None
    return [m3c2(binned[a], binned[b], engine=eng, **({} if explicit else {"as_numpy": not isinstance(clouds[a], torch.Tensor)}), **m3c2_kwargs)
            for a, b in pairs.tolist()]


def pair_statistics(result: M3C2Result) -> dict:
    """The figures of one pair: the number of core points, of those with a distance, of those significant; mean, median and sample standard
    deviation (NaN below two) of the distance over the significant ones (NaN when there is none); the mean level of detection over the
    core points that have one."""
    dist, lod, sig = (np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for v in (result.distance, result.lod, result.significant))
    sig = sig.astype(bool)
    d = dist[sig].astype(np.float64)
    has_lod = ~np.isnan(lod)
    return {"n_core": int(len(dist)), "n_distance": int((~np.isnan(dist)).sum()), "n_significant": int(sig.sum()),
            "mean": float(np.mean(d)) if len(d) else np.nan, "median": float(np.median(d)) if len(d) else np.nan,
            "std": float(np.std(d, ddof=1)) if len(d) > 1 else np.nan, "lod_mean": float(np.mean(lod[has_lod])) if has_lod.any() else np.nan}


def format_row(name0, name1, stats) -> str:
    """One CSV row: the two names, three counts, four figures with 4 decimals (NaN as "NaN")."""
    figures = [f"{stats[k]:.4f}" if np.isfinite(stats[k]) else "NaN" for k in CSV_COLUMNS[5:]]
    return ",".join([str(name0), str(name1)] + [str(stats[k]) for k in CSV_COLUMNS[2:5]] + figures) + "\n"


def m3c2_table(results, names=None, dates=None, out_path=None):
    """A DataFrame with one row per pair: CSV_COLUMNS, plus date_in and date_fin when `dates` = (date_in, date_fin) per pair is given.
    `names` = the (pcd0, pcd1) names of every pair (default: the pair's position). `out_path` also writes the rows as CSV under HEADER."""
    import pandas as pd
    results = list(results)
    names = [(str(k), str(k)) for k in range(len(results))] if names is None else [tuple(n) for n in names]
    if len(names) != len(results):
        raise ValueError(f"{len(results)} results but {len(names)} names")
    stats = [pair_statistics(r) for r in results]
    table = pd.DataFrame([[n[0], n[1]] + [s[k] for k in CSV_COLUMNS[2:]] for n, s in zip(names, stats)], columns=CSV_COLUMNS)
    if dates is not None:
        table = table.assign(date_in=pd.to_datetime([a for a, _ in dates]), date_fin=pd.to_datetime([b for _, b in dates]))
    if out_path is not None:
        from pathlib import Path
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        with open(out_path, "w") as f:
            f.write(HEADER + "\n")
            for n, s in zip(names, stats):
                f.write(format_row(n[0], n[1], s))
    return table


# ---- co-registration of a series ------------------------------------------------------------------------------------------------------------
REGISTRATION_COLUMNS = ["epoch", "reference", "iterations", "converged", "fitness", "inlier_rmse", "tx", "ty", "tz", "angle_deg"]


def _stable(points, stable, eng):
    """The points (device tensor or array) inside the polygon `stable` [nv, 2] of (x, y), or all of them without one."""
    if stable is None:
        return points
    from .post_processing.open3d_fun import crop_indices
    idx = crop_indices(points, stable, 0, 1, engine=eng)
    return points[torch.as_tensor(idx, device=points.device)] if isinstance(points, torch.Tensor) else points[idx]


def coregister_series(clouds, max_correspondence_distance, reference=0, stable=None, return_clouds=False, engine=None, **icp_kwargs):
    """`registration_icp` of every epoch of `clouds` (paths, `PointCloud`s, [n, 3] arrays or tensors) onto its reference epoch: the index
    `reference` for all (whose own entry is None), or "previous" for epoch i - 1 as it came in (epoch 0 has None). Both clouds are cut to
    the points whose (x, y) lie inside the polygon `stable` [nv, 2] (the existing polygon crop), so that only stable ground outside the
    glacier drives the fit; `target_normals` is not accepted (give `normal_radius`): the cut target has points of its own. Each entry
    equals the per-pair call on the cut clouds. Returns the list of `RegistrationResult`, and with `return_clouds` also every whole cloud
    under its transform as [n, 3] float64 device tensors (the reference as it is). `m3c2`'s `registration_error` wants `inlier_rmse`."""
    n = len(clouds)
    if reference != "previous" and (int(reference) != reference or not 0 <= int(reference) < n):
        raise ValueError(f"reference must be \"previous\" or an epoch index in 0..{n - 1} (got {reference!r})")
    if "target_normals" in icp_kwargs:
        raise ValueError("coregister_series estimates the normals of each cut reference: give normal_radius, not target_normals")
    probe = np.zeros((0, 3))
    check_registration(probe, probe, max_correspondence_distance, icp_kwargs.get("init"), icp_kwargs.get("estimation_method", "point_to_plane"),
                       icp_kwargs.get("criteria", ICPConvergenceCriteria()), None, icp_kwargs.get("normal_radius"), icp_kwargs.get("centre"))
    if stable is not None:
        stable = np.ascontiguousarray(stable, np.float64)
        if stable.ndim != 2 or stable.shape[1] != 2 or len(stable) < 3 or not np.isfinite(stable).all():
            raise ValueError("stable must be a finite polygon [nv >= 3, 2] of (x, y)")
    eng = default_engine(engine)
    from .utils.point_cloud_filters import _device_queries
    from .utils.transformations import transform_points
    whole = [_device_queries(c if isinstance(c, torch.Tensor) else cloud_points(c), eng.device, "cloud") for c in clouds]
    cut = [_stable(w, stable, eng) for w in whole]
    results = []
    for i in range(n):
        ref = i - 1 if reference == "previous" else int(reference)
        if ref < 0 or ref == i:
            results.append(None)
            continue
        r = registration_icp(cut[i], cut[ref], max_correspondence_distance, engine=eng, **icp_kwargs)
        if not isinstance(clouds[i], torch.Tensor):
            r = r._replace(transformation=r.transformation.cpu().numpy(), correspondence_set=r.correspondence_set.cpu().numpy())
        results.append(r)
    if not return_clouds:
        return results
    moved = [w if r is None else transform_points(np.asarray(r.transformation.cpu() if isinstance(r.transformation, torch.Tensor) else r.transformation),
                                                  w, engine=eng) for w, r in zip(whole, results)]
    return results, moved


def rotation_angle_deg(T) -> float:
    """The angle of the rotation block of a 4x4, in degrees, from its trace and its skew part (atan2: sound at small angles). A report
    computed on the host, not pinned to the bit."""
    R = np.asarray(T.cpu() if isinstance(T, torch.Tensor) else T, np.float64)[:3, :3]
    skew = 0.5 * math.sqrt((R[2, 1] - R[1, 2]) ** 2 + (R[0, 2] - R[2, 0]) ** 2 + (R[1, 0] - R[0, 1]) ** 2)
    return math.degrees(math.atan2(skew, 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)))


def coregistration_table(results, reference=0, names=None, out_path=None):
    """A DataFrame with one row per epoch of a `coregister_series` result: REGISTRATION_COLUMNS (the translation column of the transform
    as tx, ty, tz; the rotation angle in degrees). A reference epoch (None) has the identity: 0 iterations, converged, fitness 1, rmse 0.
    `names` = the epochs' names (default: their positions); `out_path` also writes the table as CSV."""
    import pandas as pd
    results = list(results)
    names = [str(k) for k in range(len(results))] if names is None else [str(n) for n in names]
    if len(names) != len(results):
        raise ValueError(f"{len(results)} results but {len(names)} names")
    rows = []
    for i, r in enumerate(results):
        ref = names[i - 1 if reference == "previous" and i > 0 else (i if reference == "previous" else int(reference))]
        if r is None:
            rows.append([names[i], names[i], 0, True, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
            continue
        T = np.asarray(r.transformation.cpu() if isinstance(r.transformation, torch.Tensor) else r.transformation, np.float64)
        rows.append([names[i], ref, int(r.iterations), bool(r.converged), float(r.fitness), float(r.inlier_rmse), T[0, 3], T[1, 3], T[2, 3],
                     rotation_angle_deg(T)])
    table = pd.DataFrame(rows, columns=REGISTRATION_COLUMNS)
    if out_path is not None:
        from pathlib import Path
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        table.to_csv(out_path, index=False)
    return table
