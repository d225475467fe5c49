"""Writes tests/golden/g13_sfm.npz: the reference's own two-view reconstruction of one synthetic epoch (`sfm/two_view_geometry.py`:
`RelativeOrientation.estimate_pose`; `sfm/triangulation.py`: `Triangulate.triangulate_two_views`; `thirdparty/triangulation.py`:
`iterative_LS_triangulation`, `linear_LS_triangulation`; `core/camera.py`: `Camera`).

    python tools/gen_golden_sfm.py REFERENCE_ROOT

The reference modules are loaded from their files, unchanged; OpenCV is not installed, so `cv2` is a stub and THE STUBS ARE NOT OPENCV:
  - cv2.solve(A, b, dst, DECOMP_SVD): numpy's SVD, x = V S^+ U^T b with singular values <= 2 DBL_EPSILON * sum(S) treated as zero (what
    OpenCV documents for DECOMP_SVD), written INTO dst (the reference passes a view of its output array). For a full-rank 4 x 3 system the
    least-squares solution is unique, so the triangulation in this fixture is pinned by the reference's own control flow (cumulative
    re-weighting, absolute tolerance, status arithmetic) whatever computes the SVD; the rank-deficient branch is pinned against the
    restatement only.
  - cv2.undistortPoints(pts, K, dist, None, K): `tests/sfm_oracle.py:undistort_points_f64`, the five-iteration restatement. The
    undistorted points of this fixture are that restatement's, not OpenCV's.
  - cv2.Rodrigues / cv2.projectPoints / cv2.cvtColor: as in tools/gen_golden_dsm.py (`tests/dsm_oracle.py:project_points_f64`).
  - `estimate_pose` inside `two_view_geometry` is replaced by a fixed (R, t, valid): the fixture pins the camera algebra of
    `RelativeOrientation.estimate_pose` (`two_view_geometry.py:99-105`), not an essential-matrix estimate.
The calibrations are the two of the reference's `assets/calib` (numbers, read with np.loadtxt). The scene: a rig with a 140 m baseline,
5000 points at 250-900 m seen by both cameras with 0.5 px noise, 60 points behind both cameras, 60 behind the second only, 80 on
near-parallel rays (2e4-2e6 m). The colour image is procedural (`sfm_oracle.image_pattern`), so it is not stored. Per point the fixture
keeps the number of solves, cond(A) of the first system and the smallest relative distance of max(|d1_new - d1|, |d2_new - d2|) to the
tolerance over the point's iterations (from the restatement, whose solve counts are checked against the calls the reference made); the
seed leaves no point within 1e-6 of the tolerance (asserted). Fixed zip timestamps: the file regenerates byte for byte."""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sfm_oracle as S  # noqa: E402
from dsm_oracle import project_points_f64  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g13_sfm.npz")
TOL = 3.0e-5
FRAME = (4008, 6012)


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


def _stubs(solve_log):
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_BGR2RGB, cv2.DECOMP_SVD = 4, 1

    def solve(A, b, dst, flags):                  # numpy SVD, not OpenCV; in place
        assert flags == cv2.DECOMP_SVD and A.shape == (4, 3) and dst.shape == (3, 1)
        U, s, Vt = np.linalg.svd(A, full_matrices=False)
        keep = s > 2.0 * np.finfo(np.float64).eps * s.sum()
        c = U.T @ b[:, 0]
        dst[:, 0] = Vt.T @ np.where(keep, c / np.where(keep, s, 1.0), 0.0)
        solve_log.append(1)
        return True, dst

    def undistortPoints(pts, K, dist, R, P):      # the restatement, not OpenCV
        assert R is None and P is K
        return S.undistort_points_f64(pts, K, dist)[:, None, :]

    def cvtColor(image, code):
        assert code == cv2.COLOR_BGR2RGB and image.ndim == 3 and image.shape[2] == 3
        return np.ascontiguousarray(image[:, :, ::-1])

    def Rodrigues(R):
        return np.asarray(R, np.float64), None

    def projectPoints(obj, rvec, tvec, K, dist):
        m = project_points_f64(np.asarray(obj, np.float64).reshape(-1, 3), K, dist, rvec, tvec)
        return m[:, None, :], None

    cv2.solve, cv2.undistortPoints, cv2.cvtColor, cv2.Rodrigues, cv2.projectPoints = solve, undistortPoints, cvtColor, Rodrigues, projectPoints
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


def camera_states(g, Camera, K0, d0, K1, d1):
    """A sequence of updates on the reference's Camera; the inputs and every property after each step go into the fixture."""
    R, C = rot(0.3, -0.2, 1.1), np.array([[12.5], [-3.25], [40.0]])
    t = -R @ C
    g["cam_in_R"], g["cam_in_C"], g["cam_in_t"] = R, C, t
    ext2 = np.eye(4)
    ext2[:3, :3], ext2[:3, 3] = rot(-0.15, 0.4, -0.6), [1.5, -2.0, 7.0]
    g["cam_in_ext2"] = ext2
    cam = Camera(6012, 4008, K0, d0, R=R, t=t[:, 0])
    steps = []

    def snap():
        i = len(steps)
        steps.append(i)
        for name in ("K", "dist", "extrinsics", "pose", "C", "t", "R", "P"):
            g[f"cam_s{i}_{name}"] = np.array(getattr(cam, name), np.float64)
        Kf, Rf, tf = cam.factor_P()
        g[f"cam_s{i}_factor_K"], g[f"cam_s{i}_factor_R"], g[f"cam_s{i}_factor_t"] = Kf, Rf, tf
        g[f"cam_s{i}_C_from_P"] = cam.C_from_P(cam.P)
    snap()                                                                   # 0: constructed from R, t
    cam.update_extrinsics(cam.pose_to_extrinsics(cam.build_pose_matrix(R.T, C)))
    snap()                                                                   # 1: the same orientation through the pose
    cam.update_K(K1)
    cam.update_dist(d1)
    snap()                                                                   # 2: other intrinsics
    cam.update_extrinsics(ext2)
    snap()                                                                   # 3: other extrinsics
    g["cam_s3_pose_of_ext0"] = cam.extrinsics_to_pose(g["cam_s0_extrinsics"])
    g["cam_s3_Rt_to_extrinsics"] = cam.Rt_to_extrinsics(R, t)
    cam.reset_EO()
    snap()                                                                   # 4: reset
    g["cam_n_states"] = np.int64(len(steps))


def main(ref_root):
    solve_log = []
    stubs = _stubs(solve_log)
    loaded = ["icepy4d.core.camera", "icepy4d.utils.math", "icepy4d.sfm.geometry", "icepy4d.sfm.interpolate_colors",
              "icepy4d.thirdparty.triangulation", "icepy4d.sfm.triangulation", "icepy4d.sfm.two_view_geometry"]
    saved = {k: sys.modules.get(k) for k in list(stubs) + loaded}
    sys.modules.update(stubs)
    g = {}
    try:
        src = "src/icepy4d/"
        cammod = _load(ref_root, src + "core/camera.py", loaded[0])
        _load(ref_root, src + "utils/math.py", loaded[1])
        geom = _load(ref_root, src + "sfm/geometry.py", loaded[2])
        _load(ref_root, src + "sfm/interpolate_colors.py", loaded[3])
        tp = _load(ref_root, src + "thirdparty/triangulation.py", loaded[4])
        tri = _load(ref_root, src + "sfm/triangulation.py", loaded[5])
        tvg = _load(ref_root, src + "sfm/two_view_geometry.py", loaded[6])
        Camera = cammod.Camera

        w0, h0, K0, d0 = read_calib(os.path.join(ref_root, "assets/calib/cam1.txt"))
        w1, h1, K1, d1 = read_calib(os.path.join(ref_root, "assets/calib/cam2.txt"))
        assert (h0, w0) == FRAME and (h1, w1) == FRAME
        g["K0"], g["dist0"], g["K1"], g["dist1"] = K0, d0, K1, d1
        camera_states(g, Camera, K0, d0, K1, d1)

        # ---- relative orientation with a fixed estimate: camera 0 oriented in the world, camera 1 from (R, t) and the baseline
        rng = np.random.default_rng(13)
        R0, C0 = rot(0.02, -0.03, 0.01), np.array([[10.0], [-5.0], [2.0]])
        cam0 = Camera(w0, h0, K0, d0, R=R0, t=(-R0 @ C0)[:, 0])
        cam1 = Camera(w1, h1, K1, d1)
        Rrel = rot(0.05, -0.35, 0.02)
        crel = np.array([60.0, 5.0, 126.0])
        trel = -Rrel @ (crel / np.linalg.norm(crel))          # unit translation: the baseline comes from scale_factor
        n_feat = 64
        valid = rng.random(n_feat) < 0.8
        g["ro_R"], g["ro_t"], g["ro_valid"], g["ro_scale"] = Rrel, trel, valid, np.float64(140.0)
        g["ro_cam0_extrinsics"] = cam0.extrinsics.copy()
        tvg.estimate_pose = lambda *a, **k: (Rrel, trel, valid)
        feats = [rng.uniform(0, 4000, (n_feat, 2)), rng.uniform(0, 4000, (n_feat, 2))]
        ro = tvg.RelativeOrientation([cam0, cam1], feats)
        out_valid = ro.estimate_pose(threshold=1.5, confidence=0.999999, scale_factor=140.0)
        assert out_valid is valid
        g["ro_cam1_extrinsics"], g["ro_cam1_P"], g["ro_cam1_C"] = cam1.extrinsics.copy(), cam1.P, cam1.C
        g["ro_scale_from_baseline_280"] = np.float64(ro.get_scale_factor_from_baseline(280.0))
        assert abs(np.linalg.norm(cam0.C - cam1.C) - 140.0) < 1e-9

        # ---- the scene, in camera-0 coordinates first
        def to_world(Xc):
            return (cam0.R.T @ (Xc.T - cam0.t)).T

        def in_cam(cam, Xw):
            return (cam.R @ Xw.T + cam.t).T

        def sample(n, zlo, zhi, keep):
            out = np.zeros((0, 3))
            for _ in range(400):
                if len(out) >= n:
                    break
                z = rng.uniform(zlo, zhi, 20000)
                Xc = np.stack([rng.uniform(-0.45, 0.45, 20000) * z, rng.uniform(-0.3, 0.3, 20000) * z, z], 1)
                Xw = to_world(Xc)
                out = np.concatenate([out, Xw[keep(Xw)]])
            assert len(out) >= n, f"the scene has no such points ({len(out)} of {n})"
            return out[:n]

        def inside(cam, Xw):
            uv = project_points_f64(Xw, cam.K, cam.dist, cam.R, cam.t)
            return (uv[:, 0] > 0) & (uv[:, 0] < FRAME[1]) & (uv[:, 1] > 0) & (uv[:, 1] < FRAME[0])

        def cone(cam, Xw, sign, half=0.45):
            c = in_cam(cam, Xw)
            return (sign * c[:, 2] > 1.0) & (np.abs(c[:, 0] / c[:, 2]) < half) & (np.abs(c[:, 1] / c[:, 2]) < half)

        sets = [
            ("both", sample(5000, 250.0, 900.0, lambda X: inside(cam0, X) & inside(cam1, X) & cone(cam1, X, 1)), 0.5),
            ("behind_both", sample(60, -400.0, -50.0, lambda X: cone(cam0, X, -1) & cone(cam1, X, -1, 0.2)), 0.0),
            ("behind_second", sample(60, 5.0, 120.0, lambda X: cone(cam0, X, 1) & cone(cam1, X, -1, 0.2)), 0.0),
            ("far", sample(80, 2.0e4, 2.0e6, lambda X: inside(cam0, X) & inside(cam1, X) & cone(cam1, X, 1)), 0.05),
        ]
        Xw = np.concatenate([s[1] for s in sets])
        noise = np.concatenate([np.full(len(s[1]), s[2]) for s in sets])[:, None]
        g["set_sizes"] = np.array([len(s[1]) for s in sets], np.int64)
        g["world_points"] = Xw
        kp = []
        for cam in (cam0, cam1):
            uv = project_points_f64(Xw, cam.K, cam.dist, cam.R, cam.t)
            kp.append((uv + noise * rng.normal(size=uv.shape)).astype(np.float32))
        g["kpts0"], g["kpts1"] = kp

        # ---- the reference's reconstruction
        und0, und1 = geom.undistort_points(kp[0], cam0), geom.undistort_points(kp[1], cam1)
        assert und0.dtype == np.float32 and und0.shape == kp[0].shape
        g["und0"], g["und1"], g["P0"], g["P1"] = und0, und1, cam0.P, cam1.P
        del solve_log[:]
        X, status = tp.iterative_LS_triangulation(und0, cam0.P, und1, cam1.P)
        n_calls = len(solve_log)
        Xl, sl = tp.linear_LS_triangulation(und0, cam0.P, und1, cam1.P)
        assert sl.all() and sl.dtype == bool
        image = S.image_pattern(*FRAME)
        t2 = tri.Triangulate([cam0, cam1], kp)
        X2 = t2.triangulate_two_views(compute_colors=True, image=image, cam_id=1)
        assert np.array_equal(X2, X) and t2.colors.shape == (len(X), 3)
        g["X"], g["status"], g["X_linear"], g["colors"] = X, status.astype(np.int8), Xl, t2.colors

        # ---- per-point diagnostics from the restatement; its control flow must be the reference's
        Xo, so, solves, margin = S.triangulate_iterative(und0, cam0.P, und1, cam1.P, TOL, 10, details=True)
        assert int(solves.sum()) == n_calls, (int(solves.sum()), n_calls)
        assert np.array_equal(so, status)
        A0, _ = S.system(und0, cam0.P, und1, cam1.P)
        cond = np.linalg.cond(A0)
        g["solves"], g["cond"], g["margin"] = solves.astype(np.int8), cond, margin
        assert margin.min() >= 1e-6, margin.min()
        seen = set(status.tolist())
        assert {1, -3} <= seen and (-1 in seen or -2 in seen), seen
        a, b = np.cumsum(g["set_sizes"])[[0, 1]]
        assert (status[a:b] == -3).all(), "the points behind both cameras"
        assert cond[-80:].min() > 1e3 > np.median(cond[:5000]), (cond[-80:].min(), np.median(cond[:5000]))
        err = np.linalg.norm(Xo - X, axis=1) / np.maximum(1.0, np.linalg.norm(X, axis=1)) / np.maximum(1.0, cond / 1e3)
        print(f"{len(X)} points, statuses {sorted(seen)}, {int((solves == 10).sum())} with ten solves, {n_calls} solves in all; "
              f"cond median {np.median(cond):.3g} max {cond.max():.3g}; smallest tolerance margin {margin.min():.3g}; "
              f"restatement vs reference, scaled: {err.max():.3g}")
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
        sys.exit("usage: python tools/gen_golden_sfm.py REFERENCE_ROOT  (a checkout of franioli/icepy4d)")
    main(sys.argv[1])
