"""Writes tests/golden/g12_dsm_orthophoto.npz: the reference's own DSM and orthophoto outputs (`src/icepy4d/utils/dsm_orthophoto.py`:
`build_dsm`, `generate_ortophoto`; `sfm/interpolate_colors.py`: `interpolate_point_colors`; `sfm/geometry.py`: `project_points`).

    python tools/gen_golden_dsm.py REFERENCE_ROOT

The three reference modules are loaded from their files, unchanged, with three un-vendored dependencies stubbed:
  - rasterio: imported for `save_path` only, which is never passed here (`rasterio.transform.Affine` is a placeholder)
  - cv2.cvtColor(image, COLOR_BGR2RGB): an exact channel reversal
  - cv2.Rodrigues / cv2.projectPoints: NOT OpenCV. `Rodrigues(R)` hands R itself on as the "rotation vector" (no round trip through
    the axis-angle form) and `projectPoints` is the float64 restatement of `tests/dsm_oracle.py:project_points_f64`. The projection in
    this fixture is therefore that restatement; everything after it (bilinear sampling, casts, uint8) is the reference's own code.
`LinearNDInterpolator` in the loaded `dsm_orthophoto` module is wrapped by a spy that records the binned points and values the
reference hands it, so the fixture pins the binning too. The colour image is a crop of `assets/img/cam1/IMG_2637.jpg` decoded with
PIL and stored in BGR order, as cv2.imread would give it. The x / y grids are not stored: tests rebuild them with np.arange /
np.meshgrid from the stored limits and step. The file is written with fixed zip timestamps: it regenerates byte for byte."""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dsm_oracle import project_points_f64  # noqa: E402  (the stand-in for cv2.projectPoints, see above)

OUT = os.path.join(ROOT, "tests", "golden", "g12_dsm_orthophoto.npz")
IMAGE = "assets/img/cam1/IMG_2637.jpg"
CROP = (slice(300, 460), slice(500, 740))     # 160 x 240 of the 800 x 1200 frame
FILL_KIND = {"nan": 0, "mean": 1, "number": 2}


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
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_BGR2RGB = 4

    def cvtColor(image, code):
        assert code == cv2.COLOR_BGR2RGB and image.ndim == 3 and image.shape[2] == 3
        return np.ascontiguousarray(image[:, :, ::-1])

    def Rodrigues(R):                       # no round trip: the "rotation vector" is R itself
        return np.asarray(R, np.float64), None

    def projectPoints(obj, rvec, tvec, K, dist):   # float64 restatement (dsm_oracle.project_points_f64), not OpenCV
        m = project_points_f64(np.asarray(obj, np.float64).reshape(-1, 3), K, dist, rvec, tvec)
        return m[:, None, :], None

    cv2.cvtColor, cv2.Rodrigues, cv2.projectPoints = cvtColor, Rodrigues, projectPoints
    rio = types.ModuleType("rasterio")
    rio.transform = types.ModuleType("rasterio.transform")
    rio.transform.Affine = object
    pkgs = {}
    for name in ("icepy4d", "icepy4d.core", "icepy4d.sfm", "icepy4d.utils"):
        pkgs[name] = types.ModuleType(name)
        pkgs[name].__path__ = []
    cam = types.ModuleType("icepy4d.core.camera")
    cam.Camera = object
    return {"cv2": cv2, "rasterio": rio, "rasterio.transform": rio.transform, "icepy4d.core.camera": cam, **pkgs}


class Camera:
    """The four attributes the reference reads."""

    def __init__(self, K, dist, R, t):
        self.K, self.dist, self.R, self.t = K, dist, R, t


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def cloud(rng, n, x0, x1, y0, y1):
    """A seeded cloud with a smooth surface plus noise."""
    x = rng.uniform(x0, x1, n)
    y = rng.uniform(y0, y1, n)
    z = 10 + 2 * np.sin(x / 5) + 1.5 * np.cos(y / 4) + 0.05 * rng.normal(size=n)
    return np.stack([x, y, z], 1)


def main(ref_root):
    from PIL import Image as PILImage

    stubs = _stubs()
    names = list(stubs) + ["icepy4d.sfm.geometry", "icepy4d.sfm.interpolate_colors", "icepy4d.utils.dsm_orthophoto"]
    saved = {k: sys.modules.get(k) for k in names}
    sys.modules.update(stubs)
    g = {}
    try:
        geom = _load(ref_root, "src/icepy4d/sfm/geometry.py", "icepy4d.sfm.geometry")
        ic = _load(ref_root, "src/icepy4d/sfm/interpolate_colors.py", "icepy4d.sfm.interpolate_colors")
        do = _load(ref_root, "src/icepy4d/utils/dsm_orthophoto.py", "icepy4d.utils.dsm_orthophoto")
        seen = {}
        real = do.LinearNDInterpolator

        def spy(points, values, fill_value=np.nan):
            p = np.asarray(points)
            seen["bx"], seen["by"], seen["bz"] = p[:, 0].copy(), p[:, 1].copy(), np.asarray(values).copy()
            return real(points, values, fill_value=fill_value)
        do.LinearNDInterpolator = spy

        rng = np.random.default_rng(12)
        base = cloud(rng, 5000, 2.3, 31.7, 1.2, 21.9)
        neg = cloud(rng, 1200, -4.9, 5.1, -3.2, 3.9)
        # rounding ties (half to even) and keys that round to -0.0 / +0.0
        neg[:60, 0] = rng.choice([-0.25, -0.2, -0.1, 0.1, 0.25, 0.75, -0.75, 1.25], 60)
        neg[60:120, 1] = rng.choice([-0.25, -0.1, 0.1, 0.25, -1.25], 60)
        nanz = cloud(rng, 1500, 0.0, 12.0, 0.0, 9.0)
        nanz[rng.random(len(nanz)) < 0.2, 2] = np.nan
        nanz[(nanz[:, 0] > 5.5) & (nanz[:, 0] < 6.5) & (nanz[:, 1] > 3.5) & (nanz[:, 1] < 4.5), 2] = np.nan   # an all-NaN cell
        cases = {
            # name: points, step, xlim, ylim, fill
            "s05": ("base", 0.5, None, None, np.nan),
            "s1": ("base", 1.0, None, None, "mean"),
            "narrow": ("base", 0.5, [8.0, 20.0], [5.0, 15.5], np.nan),
            "wide": ("base", 1.0, [-3.0, 36.0], [-2.5, 26.0], -9999.0),
            "neg": ("neg", 0.5, None, None, np.nan),
            "nanz": ("nanz", 0.5, None, None, np.nan),
            "nanz_mean": ("nanz", 1.0, None, None, "mean"),
        }
        g["pts_base"], g["pts_neg"], g["pts_nanz"] = base, neg, nanz
        dsms = {}
        for name, (pts, step, xlim, ylim, fill) in cases.items():
            seen.clear()
            d = do.build_dsm(g["pts_" + pts], dsm_step=step, xlim=xlim, ylim=ylim, fill_value=fill)
            dsms[name] = d
            p = g["pts_" + pts]
            lim = [np.floor(p[:, 0].min()), np.ceil(p[:, 0].max()), np.floor(p[:, 1].min()), np.ceil(p[:, 1].max())]
            g[name + "_src"] = np.frombuffer(pts.encode(), np.uint8)
            g[name + "_step"] = np.float64(step)
            g[name + "_lim"] = np.array((xlim or lim[:2]) + (ylim or lim[2:]), np.float64)
            g[name + "_lim_given"] = np.array([xlim is not None, ylim is not None])
            kind = "mean" if isinstance(fill, str) else ("nan" if np.isnan(fill) else "number")
            g[name + "_fill"] = np.array([FILL_KIND[kind], 0.0 if kind != "number" else fill], np.float64)
            g[name + "_z"] = d.z
            g[name + "_bx"], g[name + "_by"], g[name + "_bz"] = seen["bx"], seen["by"], seen["bz"]
            assert d.z.shape == (len(np.arange(*g[name + "_lim"][2:], step)), len(np.arange(*g[name + "_lim"][:2], step)))
        assert np.isnan(g["nanz_bz"]).any() and np.isnan(g["nanz_mean_bz"]).any() and np.isnan(g["nanz_mean_z"]).any()
        assert np.signbit(g["neg_bx"][g["neg_bx"] == 0]).any() or np.signbit(g["neg_by"][g["neg_by"] == 0]).any()

        # the orthophoto: a colour crop (BGR, as cv2.imread gives it) and a distorted camera looking down on the s05 DSM; the
        # footprint leaves the image on two sides
        rgb = np.asarray(PILImage.open(os.path.join(ref_root, IMAGE)).convert("RGB"))[CROP]
        img = np.ascontiguousarray(rgb[:, :, ::-1])
        g["image"] = img
        K = np.array([[190.0, 0.0, 121.5], [0.0, 188.0, 79.25], [0.0, 0.0, 1.0]])
        R = rot(np.pi + 0.08, -0.05, 0.3)
        C = np.array([16.0, 11.0, 30.0])
        t = (-R @ C).reshape(3, 1)
        dists = {"d0": np.zeros(0), "d4": np.array([-0.11, 0.03, 0.002, -0.001]),
                 "d5": np.array([-0.12, 0.04, 0.0015, -0.0007, -0.01]),
                 "d8": np.array([-0.1, 0.02, 0.001, -0.0005, 0.004, 0.05, -0.01, 0.002])}
        g["cam_K"], g["cam_R"], g["cam_t"] = K, R, t
        for k, v in dists.items():
            g["dist_" + k] = v
        cam = Camera(K, dists["d5"], R, t)
        d = dsms["s05"]
        g["ortho"] = do.generate_ortophoto(img, d, cam)
        uv = geom.project_points(np.stack([d.x.ravel(), d.y.ravel(), np.nan_to_num(d.z.ravel(), nan=10.0)], 1), cam)
        inside = (uv[:, 0] >= 0) & (uv[:, 0] < img.shape[1]) & (uv[:, 1] >= 0) & (uv[:, 1] < img.shape[0])
        assert 0.2 < inside.mean() < 0.9 and np.isnan(d.z).any() and g["ortho"].dtype == np.uint8
        # interpolate_point_colors / project_points on scattered points, some off the image, for each distortion length
        pts = np.stack([rng.uniform(-5, 40, 400), rng.uniform(-5, 30, 400), rng.uniform(5, 15, 400)], 1)
        g["pc_points"] = pts
        for k, v in dists.items():
            c = Camera(K, v, R, t)
            g["pc_proj_" + k] = geom.project_points(pts, c)
            g["pc_cols_" + k] = ic.interpolate_point_colors(pts, img, c)
        g["pc_cols_d5_bgr"] = ic.interpolate_point_colors(pts, img, cam, convert_BRG2RGB=False)
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
        sys.exit("usage: python tools/gen_golden_dsm.py REFERENCE_ROOT  (a checkout of franioli/icepy4d)")
    main(sys.argv[1])
