"""Change detection between the clouds of a series, on the device: M3C2 (`post_processing/cloud_distance.py`) for every pair of epochs, in
the shape of `volume_variations.py`. `m3c2_series` uploads and bins every cloud once and serves all pairs; `m3c2_table` condenses the
per-point results into one row per pair. The reference has no counterpart (its scripts stop at the DEM of difference); the definitions
are this library's own and parity with CloudCompare's M3C2 plugin is unpinned (see that module). No CPU fallback: without a HIP device
`m3c2_series` raises."""
import numpy as np
import torch

from .engine import default_engine
from .post_processing.cloud_distance import M3C2Result, check_m3c2, m3c2
from .utils.point_cloud_filters import bin_cloud
from .volume_variations import cloud_points

CSV_COLUMNS = ["pcd0", "pcd1", "n_core", "n_distance", "n_significant", "mean", "median", "std", "lod_mean"]
HEADER = ",".join(CSV_COLUMNS)


def m3c2_series(clouds, pairs, engine=None, **m3c2_kwargs):
    """M3C2 of every pair (first, second) of indices into `clouds` (paths, `PointCloud`s, [n, 3] arrays or tensors), e.g. the indices behind
    `post_processing.make_pairs`: a list of `M3C2Result`, one per pair, equal to the per-pair call `m3c2(clouds[first], clouds[second],
    **m3c2_kwargs)`. Every cloud a pair names is uploaded and binned once. The core points of a pair are the first cloud's own points
    unless `core_points` is given. numpy results unless the first cloud of a pair is a tensor."""
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
