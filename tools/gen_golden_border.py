"""Writes tests/golden/g18_top_border.npz: the reference's top-border detection (`scripts/pcd_postprocessing/top_border.py`:
`detect_border_by_geometry`, `extract_glacier_border`) of two small synthetic epochs.

    python tools/gen_golden_border.py REFERENCE_ROOT

The reference script is loaded from its file, unchanged, with its module constants (PCD_DIR, OUT_DIR) pointed at a temporary directory.
CloudComPy is not installed, so `cloudComPy` is a stub and THE STUB IS NOT CLOUDCOMPARE:
  - cc.computeFeature(feature, radius, [cloud]): `tests/ball_oracle.py:ball_features`, the brute-force numpy restatement of this project's
    own definition of the features, stored as a scalar field. The arguments it is called with are recorded.
  - cc.filterBySFValue(lo, hi, cloud): the points (and every scalar field) with lo <= v <= hi of the current scalar field, NaN dropped.
  - loadPointCloud / SavePointCloud: the cloud travels through a table keyed by its path; the file written next to it holds only the
    header line the script's glob needs to find it. Scalar fields keep their order of creation, which the script relies on.
The feature values of this fixture are therefore the restatement's, not CloudCompare's. What the fixture pins is the reference's own
part: the features and radii it asks for (Linearity at 2.0, Verticality at 0.15), both on the full cloud, the order of its filters
(95-100 of Linearity, 95-100 of Verticality over the survivors, 60-95 of z over those), its y window and median(x) +- 10, and the text of
its CSV rows. The two scalar fields of every epoch are stored as well (`linearity<k>`, `verticality<k>`), so that the chain of filters
can be checked without computing 6000 balls by brute force again.
Input: two seeded synthetic fronts of 6000 points each, a steep wall under a plateau, in a local frame whose y spans the script's window.
Fixed zip timestamps: the file regenerates byte for byte."""
import importlib.util
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ball_cases as BC  # noqa: E402
import ball_oracle as B  # noqa: E402

OUT = B.GOLDEN
EPOCHS = (("20220726", 41, 0.0), ("20220801", 42, -0.35))         # date, seed, shift of the front along x between the epochs
N_POINTS = 6000


def _save(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def cloud(seed, shift):
    pts = BC.front(N_POINTS, seed, size=(4.0, 6.0), origin=(50.0 + shift, 223.0, 100.0))
    return np.round(pts * 1024.0) / 1024.0                           # multiples of 2^-10: the stored cloud is short and exact


class StubField:
    def __init__(self, values):
        self.values = np.array(values, np.float64)

    def toNpArray(self):
        return self.values

    def fromNpArrayCopy(self, a):
        self.values = np.array(a, np.float64)


class StubCloud:                                          # the restatement, not CloudCompare
    def __init__(self, points, index=None):
        self.points = np.array(points, np.float64).reshape(-1, 3)
        self.index = np.arange(len(self.points)) if index is None else np.asarray(index)
        self.names, self.fields, self.current = [], [], -1

    def toNpArrayCopy(self):
        return self.points.copy()

    def addScalarField(self, name):
        self.names.append(name)
        self.fields.append(StubField(np.full(len(self.points), np.nan)))
        return len(self.fields) - 1

    def getScalarFieldDic(self):
        return {name: k for k, name in enumerate(self.names)}

    def getScalarField(self, k):
        return self.fields[k]

    def setCurrentOutScalarField(self, k):
        self.current = k

    def select(self, keep):
        out = StubCloud(self.points[keep], self.index[keep])
        out.names = list(self.names)
        out.fields = [StubField(f.values[keep]) for f in self.fields]
        return out


def _stubs(calls, table):
    cc = types.ModuleType("cloudComPy")
    cc.GeomFeature = types.SimpleNamespace(Linearity="Linearity", Verticality="Verticality")

    def computeFeature(feature, radius, clouds):
        for c in clouds:
            calls.append((str(feature), float(radius), len(c.points)))
            k = c.addScalarField(f"{feature} ({radius})")
            c.getScalarField(k).fromNpArrayCopy(B.ball_features(c.points, radius)[str(feature)])
        return True

    def filterBySFValue(lo, hi, c):
        return c.select(B.filter_by_value(c.getScalarField(c.current).toNpArray(), lo, hi))

    def SavePointCloud(c, path):
        table[os.path.abspath(path)] = c
        with open(path, "w") as f:
            f.write("ply\n")
        return True

    cc.computeFeature, cc.filterBySFValue, cc.SavePointCloud = computeFeature, filterBySFValue, SavePointCloud
    cc.loadPointCloud = lambda path: table.get(os.path.abspath(path))
    cc.deleteEntity = lambda c: None
    mods = {"cloudComPy": cc, "open3d": types.ModuleType("open3d")}
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda it, *a, **k: it
    mods["tqdm"] = tq
    for name in ("icepy4d", "icepy4d.post_processing"):
        mods[name] = types.ModuleType(name)
        mods[name].__path__ = []
    fun = types.ModuleType("icepy4d.post_processing.open3d_fun")
    fun.filter_pcd_by_polyline = fun.read_and_merge_point_clouds = None
    mods["icepy4d.post_processing.open3d_fun"] = fun
    return mods


def main(ref_root):
    calls, table = [], {}
    stubs = _stubs(calls, table)
    name = "reference_top_border"
    saved = {k: sys.modules.get(k) for k in list(stubs) + [name]}
    sys.modules.update(stubs)
    g = {}
    try:
        with tempfile.TemporaryDirectory() as tmp:
            spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, "scripts/pcd_postprocessing/top_border.py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[name] = mod
            spec.loader.exec_module(mod)
            mod.PCD_DIR = mod.OUT_DIR = tmp + os.sep
            for k, (date, seed, shift) in enumerate(EPOCHS):
                pts = cloud(seed, shift)
                g[f"points{k}"] = pts
                stubs["cloudComPy"].SavePointCloud(StubCloud(pts), os.path.join(tmp, f"merged_{date}.ply"))
            mod.detect_border_by_geometry()
            assert [c[:2] for c in calls] == [("Linearity", 2.0), ("Verticality", 0.15)] * len(EPOCHS), calls
            assert all(c[2] == N_POINTS for c in calls), "a feature was computed on a filtered cloud"
            for k, (date, _, _) in enumerate(EPOCHS):
                border = table[os.path.abspath(os.path.join(tmp, f"border_{date}.ply"))]
                g[f"border{k}"] = border.index.astype(np.int64)
                full = table[os.path.abspath(os.path.join(tmp, f"merged_{date}.ply"))]
                g[f"linearity{k}"], g[f"verticality{k}"] = full.getScalarField(0).toNpArray(), full.getScalarField(1).toNpArray()
                assert np.array_equal(border.points, g[f"points{k}"][border.index]) and len(border.index) >= 2
                assert list(border.getScalarFieldDic()) == ["Linearity (2.0)", "Verticality (0.15)", "Coord. X", "Coord. Y", "Coord. Z"]
                print(f"epoch {date}: {len(border.index)} border points of {N_POINTS}")
            mod.extract_glacier_border()
            with open(os.path.join(tmp, mod.FOUT_NAME)) as f:
                text = f.read()
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    print(text)
    assert len(text.splitlines()) == 1 + len(EPOCHS) and "NaN" not in text and "nan" not in text
    g["csv"] = np.frombuffer(text.encode("ascii"), np.uint8)
    g["dates"] = np.array([int(e[0]) for e in EPOCHS], np.int64)
    g["args"] = np.array([c[1] for c in calls[:2]], np.float64)
    _save(OUT, g)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e6:.2f} MB)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/gen_golden_border.py REFERENCE_ROOT  (a checkout of franioli/icepy4d)")
    main(sys.argv[1])
