"""Writes tests/golden/g14_velocity.npz: the reference's own binned statistics and tracked-point tables (`utils/binned_stats.py`:
`bins_from_nodes`, `bins_from_nodes3D`, `compute_binned_stats2D`, `compute_binned_stats3D`; `utils/tracking_features_utils.py`:
`tracked_points_time_series`, `tracked_dict_to_df`; `utils/geospatial.py`: `point_in_volume`) on the procedural inputs of
tests/binned_oracle.py.

    python tools/gen_golden_binned.py REFERENCE_ROOT

The reference modules are loaded from their files, unchanged, on the installed numpy / scipy / pandas. `cv2` is an empty stub (never
called), matplotlib uses Agg, and `icepy4d.*` are stand-in packages: `icepy4d.core` carries the four type names the annotations need,
`icepy4d.utils.timer.timeit` is the identity. The stand-in containers offer only `get_track_ids()`, `[id].coordinates`, `.X / .Y / .Z`
and `.x / .y`. The fixture stores a SHA-256 of every input array and the outputs only. Fixed zip timestamps: the file regenerates byte
for byte."""
import importlib.util
import io
import os
import sys
import types
import zipfile

import matplotlib
import numpy as np

matplotlib.use("Agg")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import binned_oracle as B  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g14_velocity.npz")


def _load(ref_root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _save(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def _stubs():
    mods = {"cv2": types.ModuleType("cv2")}
    for name in ("icepy4d", "icepy4d.core", "icepy4d.utils", "icepy4d.core.features", "icepy4d.core.points", "icepy4d.utils.timer"):
        mods[name] = types.ModuleType(name)
        mods[name].__path__ = []
    for t in ("Features", "FeaturesDict", "PointsDict", "EpochDataMap"):
        setattr(mods["icepy4d.core"], t, type(t, (), {}))
    mods["icepy4d.core.features"].Features = mods["icepy4d.core"].Features
    mods["icepy4d.core.features"].Feature = type("Feature", (), {})
    mods["icepy4d.core.points"].Point = type("Point", (), {})
    mods["icepy4d.utils.timer"].timeit = lambda f: f
    return mods


def main(ref_root):
    stubs = _stubs()
    loaded = ["icepy4d.utils.geospatial", "icepy4d.utils.binned_stats", "icepy4d.utils.tracking_features_utils"]
    saved = {k: sys.modules.get(k) for k in list(stubs) + loaded}
    sys.modules.update(stubs)
    g = {}
    try:
        src = "src/icepy4d/utils/"
        _load(ref_root, src + "geospatial.py", loaded[0])
        bs = _load(ref_root, src + "binned_stats.py", loaded[1])
        tf = _load(ref_root, src + "tracking_features_utils.py", loaded[2])

        for name in list(B.CASES) + ["trk"]:
            for k, h in B.input_hashes(name).items():
                g[f"{name}_hash_{k}"] = np.array(h)

        for name in ("a2d", "nan", "big"):
            c = B.CASES[name]()
            bx, by = bs.bins_from_nodes(c["x_nodes"], c["y_nodes"])
            g[f"{name}_binx"], g[f"{name}_biny"] = np.array(bx), np.array(by)
            for s in B.STATS:
                xx, yy, st = bs.compute_binned_stats2D(c["points"], c["values"], s, c["x_nodes"], c["y_nodes"])
                assert st.shape == xx.shape == (len(c["y_nodes"]), len(c["x_nodes"]))
                g[f"{name}_{s}"] = st
        cnt = g["a2d_count"]
        print(f"a2d: {int(cnt.sum())} of 6000 points inside, cells of up to {int(cnt.max())}; big: a cell of {int(g['big_count'].max())}")
        assert g["big_count"].max() >= 20000
        assert np.signbit(g["nan_median"][0, 5]) and g["nan_median"][0, 5] == 0, "the median of {0.0, -0.0, 5} is -0.0"
        assert np.isnan(g["nan_max"][2, 5]) and g["nan_min"][2, 5] == 1.0

        c = B.case_auto()
        for s in B.STATS:
            xx, yy, st = bs.compute_binned_stats2D(c["points"], c["values"], s, step=c["step"])
            g[f"auto_{s}"] = st
        g["auto_xx"], g["auto_yy"] = xx, yy

        c = B.case_a3d()
        for k, e in zip("xyz", bs.bins_from_nodes3D(c["x_nodes"], c["y_nodes"], c["z_nodes"])):
            g[f"a3d_bin{k}"] = np.array(e)
        for s in B.STATS:
            xx, yy, zz, st = bs.compute_binned_stats3D(c["points"], c["values"], s, c["x_nodes"], c["y_nodes"], c["z_nodes"])
            g[f"a3d_{s}"] = st
        g["a3d_grid_shape"], g["a3d_xx0"] = np.array(xx.shape, np.int64), xx[:, :, 0]

        c = B.case_sets()
        E, V = len(c["offsets"]) - 1, len(c["values"])
        for s in B.SETS_STATS:
            out = np.empty((E, V, len(c["x_nodes"]), len(c["y_nodes"])))
            for e in range(E):
                lo, hi = c["offsets"][e], c["offsets"][e + 1]
                if lo == hi:         # scipy raises on an empty sample: an empty set is all fill values (0 for count, NaN otherwise)
                    out[e] = 0.0 if s == "count" else np.nan
                    continue
                for k in range(V):
                    out[e, k] = bs.compute_binned_stats2D(c["points"][lo:hi], c["values"][k, lo:hi], s, c["x_nodes"], c["y_nodes"])[2].T
            g[f"sets_{s}"] = out

        c = B.case_trk()
        points, features = B.trk_containers(c)
        epoch_dict = B.trk_epoch_dict(c["days"])
        n_zero = 0
        for run, with_volume, min_eps in B.TRK_RUNS:
            fts = tf.tracked_points_time_series(points, min_tracked_epoches=min_eps, volume=B.TRK_VOLUME if with_volume else None)
            g[f"trk_{run}_series_ids"] = np.array(list(fts), np.int64)
            g[f"trk_{run}_series_mask"] = np.array([[ep in eps for ep in points] for eps in fts.values()], bool).reshape(len(fts), len(points))
            frames = [("f", tf.tracked_dict_to_df(features, points, epoch_dict, fts, **B.TRK_FILTER))]
            if run in B.TRK_UNFILTERED:
                frames.append(("u", tf.tracked_dict_to_df(features, points, epoch_dict, fts)))
            for tag, df in frames:
                g["trk_columns"], g["trk_dtypes"] = np.array(list(df.columns)), np.array([str(t) for t in df.dtypes])
                g[f"trk_{run}_{tag}_index"] = np.asarray(df.index, np.int64)
                for col in df.columns:
                    a = df[col].to_numpy()
                    g[f"trk_{run}_{tag}_{col}"] = a.view(np.int64) if a.dtype.kind in "mM" else a
                if tag == "u":
                    n_zero += int((df["dt"].dt.days == 0).sum())
                    assert np.isinf(df["vX"]).any() and np.isnan(df["vX"]).any() if min_eps == 1 else True
                print(f"trk {run} {tag}: {len(df)} rows of {len(fts)} tracked ids")
        assert n_zero > 0
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    _save(OUT, g)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.0f} kB)")
    assert os.path.getsize(OUT) < 500e3


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/gen_golden_binned.py REFERENCE_ROOT  (a checkout of franioli/icepy4d)")
    main(sys.argv[1])
