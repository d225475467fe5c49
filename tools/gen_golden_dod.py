"""Writes tests/golden/g17_dod.npz: what the reference's own volume-variation code does around the two libraries it calls
(`post_processing/utils.py`: `make_pairs`; `post_processing/cloudcompare_fun.py`: `DemOfDifference`; `post_processing/open3d_fun.py`:
`filter_pcd_by_polyline`; `utils/geospatial.py`: `ccw_sort_points`).

    python tools/gen_golden_dod.py REFERENCE_ROOT

The reference modules are loaded from their files, unchanged. CloudComPy and Open3D are not installed, so both are stubs and THE STUBS
ARE NOT THOSE LIBRARIES:
  - cloudComPy: loadPointCloud reads a .ply with this project's reader (None for a file that cannot be read), ReportInfoVol is an empty
    object, ComputeVolume25D IS tests/dod_oracle.py (the restatement of DESIGN §4) and records the arguments it is called with.
  - open3d: a point cloud with .points, .colors and select_by_index. matplotlib is the real one: the polygon masks are matplotlib's own.
What the fixture pins is the reference's own part: the pairs and dates of `make_pairs` (the "202" index of the first stem, the range
len - step, the closest date with the first index on ties), the arguments of `ComputeVolume25D`, the CSV bytes and the header rule of
`write_result_to_file`, the IOError of an unreadable cloud, the polygon (`ccw_sort_points` of the polyline's y, z columns) and which points
matplotlib finds inside it. Fixed zip timestamps: the file regenerates byte for byte."""
import importlib.util
import io
import os
import sys
import tempfile
import types
import zipfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import dod_oracle as O  # noqa: E402

OUT = O.GOLDEN


def _load(ref_root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _save(path, arrays):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def front(seed, n, shift):
    """a synthetic glacier front seen along x: x = the height over the (y, z) plane"""
    rng = np.random.default_rng(seed)
    y, z = rng.uniform(0.0, 30.0, n), rng.uniform(0.0, 20.0, n)
    x = 100.0 + 4.0 * np.sin(y / 5.0) + 0.3 * z - shift * (1.0 + 0.5 * np.cos(z / 4.0)) + rng.normal(0.0, 0.05, n)
    return np.column_stack([x, y + 0.7 * shift, z])


def outline(kind):
    """the polyline file's rows x y z"""
    rng = np.random.default_rng(len(kind))
    if kind == "hexagon":
        a = np.linspace(0.0, 2 * np.pi, 7)[:-1] + 0.2
        r = np.array([9.0, 11.0, 8.5, 10.0, 12.0, 9.5])
    else:                                   # star-shaped around its centre, 64 vertices
        a = np.sort(rng.uniform(0.0, 2 * np.pi, 64))
        r = rng.uniform(4.0, 12.0, 64)
    poly = np.column_stack([np.full(len(a), 100.0), 15.0 + r * np.cos(a), 10.0 + 0.8 * r * np.sin(a)])
    return poly[rng.permutation(len(poly))]                                    # the file lists the vertices in no order


def _stubs(calls):
    from icepy4d_amd.core.point_cloud import read_ply
    cc = types.ModuleType("cloudComPy")

    def load(path):
        try:
            return read_ply(path)[0]
        except (OSError, ValueError, KeyError):
            return None

    def compute(report, ground, ceil, vertDim, gridStep, groundHeight, ceilHeight):
        calls.append((int(vertDim), float(gridStep), float(groundHeight), float(ceilHeight)))
        for k, v in O.dod(ground, ceil, vertDim, gridStep)["report"].items():
            setattr(report, k, float(v))
        return True

    cc.ccPointCloud = np.ndarray
    cc.loadPointCloud, cc.ReportInfoVol, cc.ComputeVolume25D = load, type("ReportInfoVol", (), {}), compute
    cc.deleteEntity = lambda e: None
    o3d = types.ModuleType("open3d")

    class StubCloud:
        def __init__(self, points=None, colors=None):
            self.points, self.colors = points, colors

        def select_by_index(self, idx):
            return StubCloud(self.points[idx], None if self.colors is None else self.colors[idx])

    o3d.geometry = types.SimpleNamespace(PointCloud=StubCloud)
    o3d.utility, o3d.io = types.SimpleNamespace(), types.SimpleNamespace()
    mods = {"cloudComPy": cc, "open3d": o3d}
    for name in ("icepy4d", "icepy4d.utils", "icepy4d.core"):
        mods[name] = types.ModuleType(name)
        mods[name].__path__ = []
    easydict = types.ModuleType("easydict")
    easydict.EasyDict = dict
    feats, points = types.ModuleType("icepy4d.core.features"), types.ModuleType("icepy4d.core.points")
    feats.Features = feats.Feature = points.Point = None
    timer = types.ModuleType("icepy4d.utils.timer")
    timer.AverageTimer = None
    mods.update({"easydict": easydict, "icepy4d.core.features": feats, "icepy4d.core.points": points, "icepy4d.utils.timer": timer})
    return mods, StubCloud


def main(ref_root):
    from icepy4d_amd.core.point_cloud import PointCloud
    calls = []
    stubs, StubCloud = _stubs(calls)
    loaded = ["icepy4d.utils.geospatial", "icepy4d.post_processing.utils", "icepy4d.post_processing.cloudcompare_fun", "icepy4d.post_processing.open3d_fun"]
    saved = {k: sys.modules.get(k) for k in list(stubs) + loaded}
    sys.modules.update(stubs)
    g = {}
    try:
        geo = _load(ref_root, "src/icepy4d/utils/geospatial.py", loaded[0])
        putils = _load(ref_root, "src/icepy4d/post_processing/utils.py", loaded[1])
        ccfun = _load(ref_root, "src/icepy4d/post_processing/cloudcompare_fun.py", loaded[2])
        o3dfun = _load(ref_root, "src/icepy4d/post_processing/open3d_fun.py", loaded[3])

        # make_pairs: a series with gaps, ties between two equally close dates, and steps that reach past its end
        stems = ["sampled_2022_05_01", "sampled_2022_05_02", "sampled_2022_05_04", "sampled_2022_05_08", "sampled_2022_05_09", "sampled_2022_05_15",
                 "sampled_2022_05_16"]
        g["stems"] = np.array(stems)
        for step in (1, 2, 5):
            pairs, dates = putils.make_pairs([Path("clouds") / (s + ".ply") for s in stems], step)
            g[f"pairs_step{step}"] = np.array([[stems.index(Path(a).stem), stems.index(Path(b).stem)] for a, b in pairs.values()], np.int64).reshape(-1, 2)
            g[f"pair_keys_step{step}"] = np.array(list(pairs.keys()), np.int64)
            g[f"pair_paths_step{step}"] = np.array([[a, b] for a, b in pairs.values()]).reshape(-1, 2)
        g["dates"] = np.array([d.strftime("%Y-%m-%d") for d in dates])

        # DemOfDifference over a series of three fronts
        clouds = [front(70 + t, 2500, 0.4 * t) for t in range(3)]
        clouds[1][5] = np.nan                                                   # one point the restatement ignores
        g["clouds"] = np.stack(clouds)
        with tempfile.TemporaryDirectory() as tmp:
            paths = []
            for t, c in enumerate(clouds):
                paths.append(os.path.join(tmp, f"sampled_2022_05_0{t + 1}.ply"))
                PointCloud(points3d=c).write_ply(paths[-1])
            csv = os.path.join(tmp, "out.csv")
            reports = []
            for k, (pair, kw) in enumerate([((paths[0], paths[1]), {}), ((paths[1], paths[2]), {"direction": "x", "grid_step": 0.3}),
                                            ((paths[0], paths[2]), {"direction": "z", "grid_step": 0.5})]):
                dod = ccfun.DemOfDifference(pair)
                assert dod.compute_volume(**kw) is True
                reports.append([getattr(dod.report, f) for f in O.FIELDS])
                dod.write_result_to_file(csv, mode="a+", header=(k != 0))          # first row: no file, header=False; then the file exists
                dod.clear()
            g["csv_append"] = np.frombuffer(Path(csv).read_bytes(), np.uint8)
            dod = ccfun.DemOfDifference((paths[0], paths[1]))
            dod.compute_volume()
            for name, mode, header in (("csv_new_header", "w", True), ("csv_new_noheader", "w", False)):
                dod.write_result_to_file(csv, mode=mode, header=header)
                g[name] = np.frombuffer(Path(csv).read_bytes(), np.uint8)
            os.remove(csv)
            dod.write_result_to_file(csv)                                          # the defaults on a file that does not exist: header
            dod.write_result_to_file(csv)                                          # and on one that does: none
            g["csv_defaults_twice"] = np.frombuffer(Path(csv).read_bytes(), np.uint8)
            try:
                ccfun.DemOfDifference((paths[0], os.path.join(tmp, "missing.ply")))
                raise AssertionError("no IOError")
            except IOError as e:
                g["ioerror_mentions_path"] = np.array("missing.ply" in str(e))
            try:
                dod.compute_volume(direction="w")
                raise AssertionError("no AssertionError")
            except AssertionError as e:
                g["bad_direction_message"] = np.array(str(e))
        g["volume_args"] = np.array(calls, np.float64)
        g["volume_pairs"] = np.array([[0, 1], [1, 2], [0, 2]], np.int64)
        g["volume_reports"] = np.array(reports, np.float64)
        assert calls[:3] == [(0, 1.0, 0.0, 0.0), (0, 0.3, 0.0, 0.0), (2, 0.5, 0.0, 0.0)], calls

        # filter_pcd_by_polyline: matplotlib's masks
        rng = np.random.default_rng(171)
        pts = np.column_stack([rng.uniform(95.0, 105.0, 6000), rng.uniform(0.0, 30.0, 6000), rng.uniform(-2.0, 22.0, 6000)])
        col = rng.uniform(0.0, 1.0, (6000, 3))
        g["crop_points"], g["crop_colors"] = pts, col
        with tempfile.TemporaryDirectory() as tmp:
            for kind in ("hexagon", "star64"):
                poly = outline(kind)
                path = os.path.join(tmp, kind + ".txt")
                np.savetxt(path, poly, delimiter=" ", fmt="%.17g")
                kept = o3dfun.filter_pcd_by_polyline(StubCloud(pts, col), path)
                mask = np.zeros(len(pts), bool)
                order = {tuple(p): i for i, p in enumerate(pts)}
                mask[[order[tuple(p)] for p in kept.points]] = True
                assert mask.sum() == len(kept.points) and np.array_equal(kept.points, pts[mask]) and np.array_equal(kept.colors, col[mask])
                g[f"polyline_{kind}"] = poly
                g[f"polygon_{kind}"] = geo.ccw_sort_points(poly[:, 1:])
                g[f"mask_{kind}"] = mask
                print(f"{kind}: {int(mask.sum())} of {len(pts)} points inside")
            try:
                o3dfun.filter_pcd_by_polyline(StubCloud(pts, col), path, dir="y")
                raise AssertionError("no ValueError")
            except ValueError as e:
                g["bad_dir_message"] = np.array(str(e))
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
        sys.exit("usage: python tools/gen_golden_dod.py REFERENCE_ROOT  (a checkout of franioli/icepy4d)")
    main(sys.argv[1])
