"""Writes tests/golden/g15_stabilise.npz: the reference's image stabilisation of seven synthetic epochs of one camera
(`utils/homography.py`: `homography_warping`; `sfm/geometry.py`: `undistort_image`; `core/camera.py`: `Camera`;
`thirdparty/transformations.py`: `euler_from_matrix`, `euler_matrix`; the rotation smoothing of `main_dev.py:453-481`).

    python tools/gen_golden_stabilise.py REFERENCE_ROOT

The reference modules are loaded from their files, unchanged; OpenCV is not installed, so `cv2` is a stub and THE STUBS ARE NOT OPENCV:
  - cv2.undistort(src, K, dist, None, K): `tests/warp_oracle.py:undistort`, the numpy restatement of the documented 8-bit bilinear path.
  - cv2.warpPerspective(src, H, (w, h)): `tests/warp_oracle.py:warp_perspective`, likewise. The matrix it is called with is recorded.
  - cv2.cvtColor(image, COLOR_RGB2BGR / COLOR_BGR2RGB): the channel axis reversed.
The resampled images of this fixture are therefore the restatement's, not OpenCV's. What the fixture pins is the reference's own part:
its camera algebra (H = K0 R K1^-1 through the pose / extrinsics updates), the order of its calls (undistort, then warp, at the input's
size), its channel handling (the two flips around the calls, which cancel because the channels are independent), and its Euler functions.
The driver's smoothing is a script, not a function: what it does (`main_dev.py:453-481`) is done here with the reference's own
`euler_from_matrix` / `euler_matrix` and `deepcopy` / `update_extrinsics`, with the window of the driver's `match` statement written for
n epochs (two at each end use the first / last five; for 160 epochs those are the driver's hard-coded cases).
Inputs: the two calibrations of the reference's `assets/calib` (numbers, read with np.loadtxt; stored unscaled, used scaled to a
144 x 96 frame), a reference camera, seven epoch cameras whose rotations differ from it by up to 0.5 degrees (epochs 0-3 with the first
calibration, 4-6 with the second), and procedural RGB images (`warp_oracle.image_pattern(96, 144, 3, seed=epoch)`: not stored).
Fixed zip timestamps: the file regenerates byte for byte."""
import importlib.util
import io
import os
import sys
import types
import zipfile
from copy import deepcopy

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import warp_oracle as W  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g15_stabilise.npz")
FRAME = (96, 144)
N_EPOCHS = 7


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


def read_calib(path):
    d = np.loadtxt(path).ravel()
    return d[0], d[1], d[2:11].reshape(3, 3).copy(), d[11:].copy()


def _stubs(h_log):
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_RGB2BGR, cv2.COLOR_BGR2RGB = 4, 4

    def cvtColor(image, code):
        assert code == 4 and image.ndim == 3 and image.shape[2] == 3
        return np.ascontiguousarray(image[:, :, ::-1])

    def undistort(src, K, dist, R, P):               # the restatement, not OpenCV
        assert R is None and P is K
        return W.undistort(src, K, dist)

    def warpPerspective(src, H, dsize):              # the restatement, not OpenCV
        h_log.append(np.array(H, np.float64))
        return W.warp_perspective(src, H, dsize)

    cv2.cvtColor, cv2.undistort, cv2.warpPerspective = cvtColor, undistort, warpPerspective
    mods = {"cv2": cv2}
    for name in ("icepy4d", "icepy4d.core", "icepy4d.sfm", "icepy4d.utils", "icepy4d.thirdparty"):
        mods[name] = types.ModuleType(name)
        mods[name].__path__ = []
    calib = types.ModuleType("icepy4d.core.calibration")
    calib.read_opencv_calibration = read_calib
    mods["icepy4d.core.calibration"] = calib
    return mods


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def main(ref_root):
    h_log = []
    stubs = _stubs(h_log)
    loaded = ["icepy4d.core.camera", "icepy4d.sfm.geometry", "icepy4d.utils.homography", "icepy4d.thirdparty.transformations"]
    saved = {k: sys.modules.get(k) for k in list(stubs) + loaded}
    sys.modules.update(stubs)
    g = {}
    try:
        src = "src/icepy4d/"
        cammod = _load(ref_root, src + "core/camera.py", loaded[0])
        geom = _load(ref_root, src + "sfm/geometry.py", loaded[1])
        hom = _load(ref_root, src + "utils/homography.py", loaded[2])
        tf = _load(ref_root, src + "thirdparty/transformations.py", loaded[3])
        Camera = cammod.Camera

        h, w = FRAME
        calib = {}
        for cam in ("cam1", "cam2"):
            fw, fh, K, d = read_calib(os.path.join(ref_root, f"assets/calib/{cam}.txt"))
            assert (fw, fh) == (W.FULL_WIDTH, 4008) and fw * h == fh * w
            g[f"calib_{cam}_K"], g[f"calib_{cam}_dist"] = K, d
            calib[cam] = (W.scale_K(K, w), d)

        rng = np.random.default_rng(15)
        R_ref, C_ref = rot(0.31, -0.12, 0.05), np.array([[120.0], [-45.0], [12.5]])
        cam_ref = Camera(w, h, calib["cam1"][0], calib["cam1"][1], R=R_ref, t=(-R_ref @ C_ref)[:, 0])
        g["ref_K"], g["ref_dist"], g["ref_extrinsics"] = cam_ref.K, cam_ref.dist, cam_ref.extrinsics.copy()
        half_degree = np.deg2rad(0.5)
        cams = []
        for e in range(N_EPOCHS):
            axis = rng.normal(size=3)
            d_ang = axis / np.linalg.norm(axis) * rng.uniform(0.2, 0.99) * half_degree
            R = rot(*d_ang) @ R_ref
            C = C_ref + rng.normal(scale=0.05, size=(3, 1))          # the centre moves a little too; H ignores it
            K, d = calib["cam1" if e < 4 else "cam2"]
            cams.append(Camera(w, h, K, d, R=R, t=(-R @ C)[:, 0]))
            g[f"ep{e}_K"], g[f"ep{e}_dist"], g[f"ep{e}_extrinsics"] = K, d, cams[-1].extrinsics.copy()

        und, warped, warped_und, Hs = [], [], [], []
        for e, cam in enumerate(cams):
            image = W.image_pattern(h, w, 3, seed=e)
            ext0, extr = cam.extrinsics.copy(), cam_ref.extrinsics.copy()
            und.append(geom.undistort_image(image, cam))
            del h_log[:]
            warped.append(hom.homography_warping(cam_ref, cam, image, undistort=False))
            warped_und.append(hom.homography_warping(cam_ref, cam, image, undistort=True))
            assert len(h_log) == 2 and np.array_equal(h_log[0], h_log[1])
            Hs.append(h_log[0])
            assert np.array_equal(cam.extrinsics, ext0) and np.array_equal(cam_ref.extrinsics, extr)     # the reference works on copies
            for a in (und[-1], warped[-1], warped_und[-1]):
                assert a.dtype == np.uint8 and a.shape == image.shape
        g["H"], g["undistorted"], g["warped"], g["warped_undistorted"] = np.stack(Hs), np.stack(und), np.stack(warped), np.stack(warped_und)
        assert all((a != 0).mean() > 0.5 for a in g["warped_undistorted"]), "the warps leave the frame"
        assert not np.array_equal(g["warped"], g["warped_undistorted"])

        # ---- the driver's smoothing (`main_dev.py:453-481`), median and mean
        g["angles"] = np.array([tf.euler_from_matrix(c.R) for c in cams])
        for name, reduce in (("median", np.median), ("mean", np.mean)):
            sm_ang, sm_ext = [], []
            for ep in range(N_EPOCHS):
                first = min(max(ep - 2, 0), N_EPOCHS - 5)                      # five epochs, centred where the sequence allows it
                per_axis = np.stack([tf.euler_from_matrix(cams[e].R) for e in range(first, first + 5)], axis=1)
                ang = reduce(per_axis, axis=1)
                smoothed = deepcopy(cams[ep])
                ext = deepcopy(smoothed.extrinsics)
                ext[:3, :3] = tf.euler_matrix(*ang)[:3, :3]
                smoothed.update_extrinsics(ext)
                sm_ang.append(ang)
                sm_ext.append(smoothed.extrinsics.copy())
            sm_ext = np.array(sm_ext)
            g[f"smooth_{name}_angles"], g[f"smooth_{name}_R"], g[f"smooth_{name}_extrinsics"] = np.array(sm_ang), sm_ext[:, :3, :3].copy(), sm_ext
        assert not np.array_equal(g["smooth_median_angles"], g["smooth_mean_angles"])
        print(f"{N_EPOCHS} epochs of {h} x {w}; rotation to the reference camera up to "
              f"{np.rad2deg(max(np.arccos(min(1.0, (np.trace(c.R @ R_ref.T) - 1) / 2)) for c in cams)):.3f} degrees; "
              f"non-zero share of the warped frames {np.mean(g['warped_undistorted'] != 0):.3f}")
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
        sys.exit("usage: python tools/gen_golden_stabilise.py REFERENCE_ROOT  (a checkout of franioli/icepy4d)")
    main(sys.argv[1])
