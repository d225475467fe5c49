"""Writes tests/golden/g16_pointcloud.npz: the reference's statistical outlier removal of one synthetic cloud
(`core/point_cloud.py`: `PointCloud.from_numpy`, `sor_filter`, `get_points`, `get_colors`; `post_processing/open3d_fun.py`:
`MeshingPoisson.SOR`).

    python tools/gen_golden_pointcloud.py REFERENCE_ROOT

The reference modules are loaded from their files, unchanged; Open3D is not installed, so `open3d` is a stub and THE STUB IS NOT OPEN3D:
  - o3d.geometry.PointCloud.remove_statistical_outlier(nb_neighbors, std_ratio): `tests/knn_oracle.py:remove_statistical_outlier`, the
    brute-force numpy restatement of the published algorithm. The arguments it is called with are recorded.
  - select_by_index(ind): rows of points and colours; o3d.utility.Vector3dVector: a float64 copy.
The filtered clouds of this fixture are therefore the restatement's, not Open3D's. What the fixture pins is the reference's own part: the
arguments of its two call sites (10 / 3.0 and 50 / 1.5), that it filters colours along with the points, and its colour conversion
((colors * 255.0).astype(int)).
Input: a seeded noisy height field of 3000 points with random colours plus 30 planted outliers well off the surface (stored).
Fixed zip timestamps: the file regenerates byte for byte."""
import importlib.util
import io
import logging
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_oracle as O  # noqa: E402

OUT = O.GOLDEN
N_SURFACE, N_OUTLIERS = 3000, 30


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


def cloud():
    rng = np.random.default_rng(16)
    xy = rng.uniform(0.0, 40.0, (N_SURFACE, 2))
    z = 3.0 * np.sin(xy[:, 0] / 6.0) + 2.0 * np.cos(xy[:, 1] / 9.0) + 0.1 * xy[:, 0] + rng.normal(0.0, 0.05, N_SURFACE)
    surface = np.column_stack([xy, z])
    out_xy = rng.uniform(0.0, 40.0, (N_OUTLIERS, 2))
    outliers = np.column_stack([out_xy, rng.uniform(15.0, 40.0, N_OUTLIERS) * rng.choice([-1.0, 1.0], N_OUTLIERS)])
    points = np.concatenate([surface, outliers])
    order = rng.permutation(len(points))
    planted = np.sort(np.nonzero(order >= N_SURFACE)[0])
    return points[order], rng.uniform(0.0, 1.0, (len(points), 3)), planted


def _stubs(calls):
    o3d = types.ModuleType("open3d")

    class StubCloud:                                      # the restatement, not Open3D
        def __init__(self):
            self.points, self.colors = np.zeros((0, 3)), None

        def remove_statistical_outlier(self, nb_neighbors, std_ratio):
            calls.append((int(nb_neighbors), float(std_ratio)))
            _, ind = O.remove_statistical_outlier(self.points, nb_neighbors, std_ratio)
            return self.select_by_index(ind), ind

        def select_by_index(self, ind):
            out = StubCloud()
            out.points = self.points[ind]
            out.colors = None if self.colors is None else self.colors[ind]
            return out

    o3d.geometry = types.SimpleNamespace(PointCloud=StubCloud)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.array(a, dtype=np.float64))
    o3d.io = types.SimpleNamespace()
    mods = {"open3d": o3d, "laspy": types.ModuleType("laspy")}
    for name in ("icepy4d", "icepy4d.utils", "matplotlib"):
        mods[name] = types.ModuleType(name)
        mods[name].__path__ = []
    easydict = types.ModuleType("easydict")
    easydict.EasyDict = dict
    geo = types.ModuleType("icepy4d.utils.geospatial")
    geo.ccw_sort_points = geo.point_in_hull = None
    timer = types.ModuleType("icepy4d.utils.timer")
    timer.AverageTimer = type("AverageTimer", (), {"__init__": lambda self, **kw: None, "update": lambda self, name: None})
    mpl_path = types.ModuleType("matplotlib.path")
    mods["matplotlib"].path = mpl_path
    mods.update({"easydict": easydict, "icepy4d.utils.geospatial": geo, "icepy4d.utils.timer": timer, "matplotlib.path": mpl_path})
    return mods


def main(ref_root):
    calls = []
    stubs = _stubs(calls)
    loaded = ["icepy4d.core.point_cloud", "icepy4d.post_processing.open3d_fun"]
    saved = {k: sys.modules.get(k) for k in list(stubs) + loaded}
    sys.modules.update(stubs)
    g = {}
    try:
        pcmod = _load(ref_root, "src/icepy4d/core/point_cloud.py", loaded[0])
        o3dfun = _load(ref_root, "src/icepy4d/post_processing/open3d_fun.py", loaded[1])
        points, colors, planted = cloud()
        g["points"], g["colors"], g["planted"] = points, colors, planted

        pc = pcmod.PointCloud(points3d=points.copy(), points_col=colors.copy())
        assert len(pc) == len(points) and np.array_equal(pc.get_points(), points)
        g["colors_int"] = pc.get_colors()
        pc.sor_filter()                                                   # the defaults of the reference: 10, 3.0
        g["sor10_points"], g["sor10_colors_int"] = pc.get_points(), pc.get_colors()
        _, g["sor10_ind"] = O.remove_statistical_outlier(points, *calls[-1])
        assert np.array_equal(g["sor10_points"], points[g["sor10_ind"]])

        mesher = object.__new__(o3dfun.MeshingPoisson)                    # SOR() reads only .pcd, .logger and .timer
        mesher.pcd = pcmod.PointCloud(points3d=points.copy()).get_pcd()
        mesher.logger, mesher.timer = logging.getLogger("g16"), stubs["icepy4d.utils.timer"].AverageTimer()
        mesher.SOR()
        g["sor50_points"] = np.asarray(mesher.pcd.points)
        _, g["sor50_ind"] = O.remove_statistical_outlier(points, *calls[-1])
        assert np.array_equal(g["sor50_points"], points[g["sor50_ind"]])
        g["args"] = np.array(calls, np.float64)
        assert calls == [(10, 3.0), (50, 1.5)], calls
        for tag in ("sor10", "sor50"):
            kept = set(g[f"{tag}_ind"].tolist())
            assert not kept & set(planted.tolist()), "a planted outlier survives"
            print(f"{tag}: {len(kept)} of {len(points)} points kept")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    _save(OUT, g)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e6:.2f} MB)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/gen_golden_pointcloud.py REFERENCE_ROOT  (a checkout of franioli/icepy4d)")
    main(sys.argv[1])
