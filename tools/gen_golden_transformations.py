"""Writes tests/golden/g21_transformations.npz: the reference's own `Rotrotranslation` (`src/icepy4d/utils/transformations.py`) run on a
few dozen points.

    python tools/gen_golden_transformations.py REFERENCE_ROOT

The reference module is loaded from its file, unchanged. Open3D is not installed, so `open3d` is an empty stub: nothing recorded here goes
through it (the point-cloud file helpers are not exercised). Only data goes into the fixture:
  T_local / T_inv_local      a rigid transform about the origin (a rotation of 25 degrees about (0.2, -0.4, 0.9), a shift), its `T` and `T_inv`
  T_world / T_inv_world      the matrix of `belvedere_loc2utm()`, as data, and its `T_inv`
  pts_local / pts_world      48 points each (a local frame; the same points spread over 400 m)
  fwd_* / inv_*              `transform` and `transform_inverse` of those points under both transforms
  refused_last_row, refused_rotation      1 where the constructor refused a matrix whose last row / whose 3x3 block is wrong
  bad_last_row, bad_rotation              those two matrices
  file_text, file_T          the bytes `write_T_mat_to_csv` wrote and the `T` `read_T_from_file` read back from them
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
OUT = os.path.join(ROOT, "tests", "golden", "g21_transformations.npz")


def _save(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def load_reference(ref_root):
    o3d = types.ModuleType("open3d")
    o3d.geometry = types.SimpleNamespace(PointCloud=object)
    sys.modules["open3d"] = o3d
    spec = importlib.util.spec_from_file_location("ref_transformations", os.path.join(ref_root, "src", "icepy4d", "utils", "transformations.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def local_transform():
    a = np.array([0.2, -0.4, 0.9])
    a /= np.linalg.norm(a)
    t = np.deg2rad(25.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    T[:3, 3] = (12.5, -3.25, 101.0)
    return T


def main(ref_root):
    ref = load_reference(ref_root)
    rng = np.random.default_rng(21)
    pts_local = np.round(rng.uniform(-20.0, 20.0, (48, 3)) * 1024.0) / 1024.0
    pts_world = pts_local * 10.0
    out = {"pts_local": pts_local, "pts_world": pts_world}
    for name, rt in (("local", ref.Rotrotranslation(local_transform())), ("world", ref.Rotrotranslation.belvedere_loc2utm())):
        out[f"T_{name}"], out[f"T_inv_{name}"] = np.array(rt.T, np.float64), np.array(rt.T_inv, np.float64)
        for pn, pts in (("local", pts_local), ("world", pts_world)):
            fwd = rt.transform(pts)
            out[f"fwd_{name}_{pn}"] = np.array(fwd, np.float64)
            out[f"inv_{name}_{pn}"] = np.array(rt.transform_inverse(np.array(fwd, np.float64)), np.float64)
    bad_row, bad_rot = local_transform(), local_transform()
    bad_row[3] = (0.0, 0.0, 0.1, 1.0)
    bad_rot[:3, :3] *= 1.2
    for key, M in (("last_row", bad_row), ("rotation", bad_rot)):
        try:
            ref.Rotrotranslation(M)
            refused = 0
        except ValueError:
            refused = 1
        out[f"refused_{key}"], out[f"bad_{key}"] = np.array(refused, np.int32), M
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "T.txt")
        ref.Rotrotranslation(local_transform()).write_T_mat_to_csv(path)
        with open(path, "rb") as f:
            out["file_text"] = np.frombuffer(f.read(), np.uint8)
        out["file_T"] = np.array(ref.Rotrotranslation.read_T_from_file(path).T, np.float64)
    _save(OUT, out)
    print(f"wrote {OUT}: {sorted(out)}")


if __name__ == "__main__":
    main(sys.argv[1])
