"""The host side of the reconstruction (`icepy4d_amd/core/camera.py`, `icepy4d_amd/sfm.py`: `RelativeOrientation`, `Triangulate`) and the
numpy restatement of its kernels (tests/sfm_oracle.py) against the reference's outputs in tests/golden/g13_sfm.npz
(tools/gen_golden_sfm.py: the reference's modules with a stub cv2). No GPU.

Bounds: the restatement reproduces the fixture's undistorted points bit for bit (they were made by it) and the reference's triangulated
points within 1e-9 * max(1, |X|) * max(1, cond / 1e3) with identical status and solve counts: for a full-rank system the solution of each
solve is unique, so two SVDs differ by rounding amplified by the condition number, and 1e-9 is the project's bound for g10. The camera
algebra is products of 4 x 4 matrices in the reference's order: 1e-12.
The kernels' own text (csrc/sfm_point.h, csrc/lstsq_jacobi.h) compiled for the host equals the restatement bit for bit on every case of
tests/sfm_cases.py: the same IEEE float64 operations in the same order, contraction off on both sides, division and square root
correctly rounded. Whoever edits the solver without a device at hand is held to the restatement by that test. It pins the order of the
operations, the thresholds and the statuses, not the contraction: the host build is for plain x86-64, which has no fused multiply-add, so
a lost `#pragma clang fp contract(off)` does not show here. That is seen on the device only (tests/test_gpu_sfm_edges.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sfm_cases as C  # noqa: E402
import sfm_oracle as S  # noqa: E402
import toolchain  # noqa: E402


@pytest.fixture(scope="module")
def g13():
    return S.load_g13(os.path.join(ROOT, "tests", "golden", "g13_sfm.npz"))


def bound(g):
    return 1e-9 * np.maximum(1.0, np.linalg.norm(g["X"], axis=1)) * np.maximum(1.0, g["cond"] / 1e3)


def test_oracle_reproduces_g13(g13):
    g = g13
    for k, K, d in (("0", g["K0"], g["dist0"]), ("1", g["K1"], g["dist1"])):
        und = S.undistort_points_f64(g["kpts" + k], K, d)
        assert und.dtype == np.float32 and np.array_equal(und.view(np.int32), g["und" + k].view(np.int32))
    X, status, solves, margin = S.triangulate_iterative(g["und0"], g["P0"], g["und1"], g["P1"], 3e-5, 10, details=True)
    assert np.array_equal(status, g["status"].astype(np.int64)) and np.array_equal(solves, g["solves"].astype(np.int64))
    assert np.all(np.linalg.norm(X - g["X"], axis=1) <= bound(g))
    Xl, sl = S.triangulate_iterative(g["und0"], g["P0"], g["und1"], g["P1"], 3e-5, 1)
    assert (sl == 1).all() and np.all(np.linalg.norm(Xl - g["X_linear"], axis=1) <= bound(g))
    # what the fixture promises about itself
    assert set(np.unique(g["status"]).tolist()) >= {1, -3} and ((g["status"] == -1) | (g["status"] == -2)).any()
    assert g["margin"].min() >= 1e-6 and (g["solves"] == 10).mean() > 0.1 and (g["cond"] > 1e3).sum() >= 80
    assert (g["status"][g["solves"] == 10] == 1).any()          # ten solves without convergence still give status 1: no 0 anywhere
    assert not (g["status"] == 0).any()


def test_oracle_rank_deficient_solve_is_minimum_norm():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(50, 4, 3))
    A[:25, :, 2] = 2.0 * A[:25, :, 0] - A[:25, :, 1]            # rank 2
    A[:5] = 0.0                                                  # rank 0
    b = rng.normal(size=(50, 4))
    x = S.lstsq43_svd(A, b)
    for i in range(50):
        ref = np.linalg.lstsq(A[i], b[i], rcond=1e-13)[0]
        assert np.allclose(x[i], ref, rtol=1e-9, atol=1e-11), i


def test_undistort_guard_and_distortion_lengths():
    K = np.array([[1000.0, 0, 500.0], [0, 1000.0, 400.0], [0, 0, 1]])
    pts = np.array([[400.0, 350.0], [500.0, 400.0], [4000.0, -3000.0]], np.float32)
    assert np.array_equal(S.undistort_points_f64(pts, K, None), S.undistort_points_f64(pts, K, np.zeros(5)))
    assert np.allclose(S.undistort_points_f64(pts, K, np.zeros(4)), pts, atol=1e-3)
    # a strongly negative k1 drives icdist below zero far from the centre: the guard returns the distorted point
    out = S.undistort_points_f64(pts, K, np.array([-0.9, 0.0, 0.0, 0.0]))
    assert np.array_equal(out[2], pts[2]) and not np.array_equal(out[0], pts[0])
    with pytest.raises(AssertionError):
        S.undistort_points_f64(pts, K, np.zeros(3))


def replay_camera(g, Camera):
    """The update sequence of tools/gen_golden_sfm.py:camera_states on `Camera`; yields (state index, camera)."""
    R, C, t = g["cam_in_R"], g["cam_in_C"], g["cam_in_t"]
    cam = Camera(6012, 4008, g["K0"], g["dist0"], R=R, t=t[:, 0])
    yield 0, cam
    cam.update_extrinsics(cam.pose_to_extrinsics(cam.build_pose_matrix(R.T, C)))
    yield 1, cam
    cam.update_K(g["K1"])
    cam.update_dist(g["dist1"])
    yield 2, cam
    cam.update_extrinsics(g["cam_in_ext2"].copy())
    yield 3, cam
    cam.reset_EO()
    yield 4, cam


def test_camera_matches_reference_states(g13):
    from icepy4d_amd.core import Camera
    g = g13
    assert g["cam_n_states"].item() == 5
    for i, cam in replay_camera(g, Camera):
        for name in ("K", "dist", "extrinsics", "pose", "C", "t", "R", "P"):
            got, ref = np.asarray(getattr(cam, name), np.float64), g[f"cam_s{i}_{name}"]
            assert got.shape == ref.shape and np.max(np.abs(got - ref), initial=0.0) <= 1e-12 * max(1.0, np.abs(ref).max()), (i, name)
        Kf, Rf, tf = cam.factor_P()
        for got, key in ((Kf, "factor_K"), (Rf, "factor_R"), (tf, "factor_t"), (cam.C_from_P(cam.P), "C_from_P")):
            ref = g[f"cam_s{i}_{key}"]
            assert got.shape == ref.shape and np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.abs(ref).max()), (i, key)
        if i == 3:
            assert np.max(np.abs(cam.extrinsics_to_pose(g["cam_s0_extrinsics"]) - g["cam_s3_pose_of_ext0"])) <= 1e-12
            assert np.max(np.abs(cam.Rt_to_extrinsics(g["cam_in_R"], g["cam_in_t"]) - g["cam_s3_Rt_to_extrinsics"])) <= 1e-12
    assert cam.width == 6012 and cam.height == 4008 and np.array_equal(cam.extrinsics, np.eye(4))


def test_camera_argument_errors(g13, tmp_path):
    from icepy4d_amd.core import Camera
    cam = Camera(100, 80, g13["K0"], g13["dist0"])
    assert np.array_equal(cam.extrinsics, np.eye(4)) and np.array_equal(cam.C, np.zeros((3, 1)))
    with pytest.raises(AssertionError):
        cam.update_extrinsics(np.eye(3))
    with pytest.raises(AssertionError):
        cam.update_extrinsics(np.eye(4, dtype=np.float32))
    bad = np.eye(4)
    bad[3, 0] = 1.0
    with pytest.raises(AssertionError):
        cam.update_extrinsics(bad)
    with pytest.raises(ValueError):
        cam.build_pose_matrix(np.eye(4), np.zeros(3))
    with pytest.raises(ValueError):
        cam.build_pose_matrix(np.eye(3), np.zeros(4))
    with pytest.raises(AssertionError):
        cam.Rt_to_extrinsics(np.eye(3), np.zeros(4))
    assert cam.build_pose_matrix(np.eye(3), np.array([1.0, 2.0, 3.0]))[:3, 3].tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(FileNotFoundError):
        Camera(1, 1, calib_path=tmp_path / "missing.txt")
    f = tmp_path / "cam.txt"
    f.write_text("6012 4008 6.6e+03 0. 3.0e+03 0. 6.6e+03 1.9e+03 0. 0. 1. -9.4e-02 8.5e-02 1.7e-04 -8.7e-04 0.\n")
    c2 = Camera(1, 1, calib_path=f)
    assert c2.width == 6012 and c2.K[0, 0] == 6600.0 and len(c2.dist) == 5


def test_relative_orientation_camera_algebra(g13, monkeypatch):
    from icepy4d_amd import sfm
    from icepy4d_amd.core import Camera
    g = g13
    seen = {}

    def fixed(kpts0, kpts1, K0, K1, thresh, conf=0.9999, **kw):
        seen.update(thresh=thresh, conf=conf, n=len(kpts0), engine=kw.get("engine"))
        return g["ro_R"], g["ro_t"], g["ro_valid"]
    monkeypatch.setattr(sfm, "estimate_pose", fixed)
    engine = object()                                   # never touched: the estimate is the fixture's
    cam0 = Camera(6012, 4008, g["K0"], g["dist0"], extrinsics=g["ro_cam0_extrinsics"].copy())
    cam1 = Camera(6012, 4008, g["K1"], g["dist1"])
    feats = [np.zeros((len(g["ro_valid"]), 2)), np.zeros((len(g["ro_valid"]), 2))]
    ro = sfm.RelativeOrientation([cam0, cam1], feats, engine=engine)
    valid = ro.estimate_pose(threshold=1.5, confidence=0.999999, scale_factor=g["ro_scale"].item())
    assert np.array_equal(valid, g["ro_valid"]) and seen == dict(thresh=1.5, conf=0.999999, n=len(feats[0]), engine=engine)
    for got, key in ((cam1.extrinsics, "ro_cam1_extrinsics"), (cam1.P, "ro_cam1_P"), (cam1.C, "ro_cam1_C")):
        assert np.max(np.abs(got - g[key])) <= 1e-12 * max(1.0, np.abs(g[key]).max()), key
    assert abs(ro.get_scale_factor_from_baseline(280.0) - g["ro_scale_from_baseline_280"].item()) <= 1e-12
    monkeypatch.setattr(sfm, "estimate_pose", lambda *a, **k: None)
    with pytest.raises(ValueError):
        ro.estimate_pose()


def test_argument_errors_before_any_device_work(g13):
    """Shapes, distortion lengths and camera tables are checked on the host, before an engine is asked for."""
    import types
    from icepy4d_amd import sfm
    g = g13
    cam = types.SimpleNamespace(K=g["K0"], dist=np.zeros(3), R=np.eye(3), t=np.zeros(3))
    with pytest.raises(ValueError):
        sfm.undistort_points(np.zeros((4, 2), np.float32), cam)
    cam.dist = g["dist0"]
    with pytest.raises(ValueError):
        sfm.undistort_points(np.zeros((4, 3), np.float32), cam)
    with pytest.raises(ValueError):
        sfm._projection(np.eye(3))
    assert np.array_equal(sfm._projection(np.vstack([g["P0"], [0, 0, 0, 1]])), g["P0"].ravel())
    assert np.allclose(sfm._projection(cam).reshape(3, 4), g["K0"] @ np.eye(3, 4))
    with pytest.raises(ValueError):
        sfm._camera_table([[cam, cam], [cam, cam]], 3)
    tab = sfm._camera_table([cam, cam], 7)
    assert tab.shape == (1, 2, 24) and tab[0, 1, 12] == g["K0"][0, 0] and np.array_equal(tab[0, 0, 16:21], g["dist0"])
    t = sfm.Triangulate([cam, cam], [np.zeros((2, 2)), np.zeros((2, 2))])
    assert t.points3d is None and t.colors is None
    with pytest.raises(AssertionError):
        t.interpolate_colors_from_image(np.zeros((4, 4, 3), np.uint8), cam)
    with pytest.raises(AssertionError):
        t.triangulate_two_views(compute_colors=True, image=None)
    X = sfm.Triangulate([types.SimpleNamespace(P=g["P0"]), types.SimpleNamespace(P=g["P1"])],
                        [np.r_[g["und0"][0], 1.0], np.r_[g["und1"][0], 1.0]]).triangulate_nviews()
    assert X.shape == (4,) and X[3] == 1.0 and np.linalg.norm(X[:3] - g["X"][0]) < 1e-2 * np.linalg.norm(g["X"][0])


def test_pack_table_layout():
    from icepy4d_amd.sequence import HEADER, record_words
    rng = np.random.default_rng(0)
    k0, k1, m0 = S.scatter_matches(rng, rng.uniform(0, 9, (5, 2)).astype(np.float32), rng.uniform(0, 9, (5, 2)).astype(np.float32), 16)
    t = S.pack_table([(k0, k1, m0), None], 16)
    assert t.shape == (2, record_words(16, True)) and S.HEADER == HEADER and t[0, 3] == 5 and t[1, 3] == -1
    assert (t[1, HEADER:HEADER + 16] == -1).all() and np.array_equal(k0[m0 > -1], k0[np.flatnonzero(m0 > -1)])
    assert np.array_equal(t[0, HEADER + 32:HEADER + 32 + 2 * len(k0)].view(np.float32).reshape(-1, 2), k0)


def test_sfm_kernels_stay_in_registers(tmp_path):
    """csrc/sfm.hip compiled to assembly for gfx950: every kernel without spills and without a private segment (the small matrices of the
    Jacobi solver are indexed with compile-time constants only, so none of them lands in scratch)."""
    seen = {k: (f["vgpr_spill_count"], f["sgpr_spill_count"], f["private_segment_fixed_size"])
            for k, f in toolchain.kernel_resources(toolchain.device_listing("sfm.hip", str(tmp_path))).items()}
    names = " ".join(seen)
    for k in ("undistort_points_kernel", "triangulate_iterative_kernelIf", "triangulate_iterative_kernelId", "table_offsets_kernel",
              "triangulate_table_kernel"):
        assert k in names, (k, list(seen))
    assert all(v == (0, 0, 0) for v in seen.values()), {k: v for k, v in seen.items() if v != (0, 0, 0)}


# ---- the kernels' text on the host ---------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """tests/sfm_host_harness.cpp + csrc/sfm_point.h as a shared library, behind a stub <hip/hip_runtime.h>."""
    lib = toolchain.host_library(str(tmp_path_factory.mktemp("sfm_host")), "sfm_host_harness.cpp")
    P, L = ctypes.c_void_p, ctypes.c_longlong
    lib.sfm_host_undistort.argtypes, lib.sfm_host_undistort.restype = [P, L, P, P], None
    lib.sfm_host_triangulate.argtypes, lib.sfm_host_triangulate.restype = [P, P, L, P, P, ctypes.c_double, ctypes.c_int, P, P], None
    return lib


def host_triangulate(lib, u1, P1, u2, P2, tolerance, max_solves):
    a, b = np.ascontiguousarray(u1, np.float64), np.ascontiguousarray(u2, np.float64)
    p1, p2 = np.ascontiguousarray(P1, np.float64), np.ascontiguousarray(P2, np.float64)
    X, status = np.empty((len(a), 3)), np.empty(len(a), np.int32)
    lib.sfm_host_triangulate(a.ctypes.data, b.ctypes.data, len(a), p1.ctypes.data, p2.ctypes.data, tolerance, max_solves, X.ctypes.data,
                             status.ctypes.data)
    return X, status


def host_undistort(lib, pts, K, dist):
    p = np.ascontiguousarray(pts, np.float32)
    cam = np.ascontiguousarray(S.camera_row(np.zeros((3, 4)), K, dist)[12:])
    out = np.empty_like(p)
    lib.sfm_host_undistort(p.ctypes.data, len(p), cam.ctypes.data, out.ctypes.data)
    return out


def test_cases_reach_every_status_and_branch(g13):
    """What tests/sfm_cases.py promises, from the restatement alone: every status value, every solve count, the early exit at every limit,
    no float64 point on the convergence edge, rank-deficient systems with finite minimum-norm points."""
    g = g13
    rows = C.value_rows(g)
    _, st, solves, _ = S.triangulate_iterative(g["und0"][rows], g["P0"], g["und1"][rows], g["P1"], 3e-5, 10, details=True)
    assert len(rows) == 237 and len(np.unique(rows)) == 237 and np.array_equal(solves, g["solves"][rows])
    assert set(np.unique(solves).tolist()) == set(range(2, 11)) and set(np.unique(st).tolist()) == {1, -2, -3}
    cases = {c[0]: c for c in C.value_cases(g) + C.degenerate_cases(g)}
    assert len(cases) == len(C.value_cases(g)) + len(C.degenerate_cases(g))
    Xs = [C.expected(cases[f"max_solves={k}"])[0] for k in range(1, 11)]
    assert all(not np.array_equal(Xs[k], Xs[k + 1]) for k in range(9))            # each further solve moves some point
    assert all(not np.array_equal(C.expected(cases[f"tolerance={t}"])[0], Xs[9]) for t in ("0", "1e-09", "0.01"))
    sw = C.expected(cases["views swapped"])[1]
    assert (sw == -1).sum() == 60 and (st == -2).sum() == 60 and np.array_equal(sw == -1, st == -2)
    a, b = C.perturbed64(g)
    X64, _, _, margin = S.triangulate_iterative(a, g["P0"], b, g["P1"], 3e-5, 10, details=True)
    assert margin.min() > 5e-5                                                      # 1e-4: far from the edge for any rounding
    X32 = S.triangulate_iterative(g["und0"], g["P0"], g["und1"], g["P1"], 3e-5, 10)[0]
    assert (X64 != X32).any(1).all() and np.array_equal(C.expected(cases["float64 points"])[0], X64[rows])
    X, st2 = C.expected(cases["rank 2: one camera, one image point twice"])
    assert np.isfinite(X).all() and (X != 0).all() and set(np.unique(st2).tolist()) == {1, -3}
    X, st0 = C.expected(cases["rank 0: zero projection matrices"])
    assert (bits(X) == 0).all() and (st0 == -3).all()
    for name, want in (("NaN in P1[0, 0]", -3), ("NaN in P1[2, 3]", -2), ("NaN in P2[2, 3]", -1), ("NaN in P[2, 3] of both cameras", 0),
                       ("inf in P1[2, 3], -inf in P2[2, 3]", -2), ("-inf in P1[2, 3], inf in P2[2, 3]", -1)):
        X, stp = C.expected(cases["non-finite projection: " + name])
        assert (bits(X) == 0).all() and (stp == want).all(), name                   # X = 0; the status follows P[2, 3] alone
    for name in ("float32", "float64"):
        X, stn = C.expected(cases[f"non-finite image points, {name}"])
        zero = (X == 0).all(1)
        assert zero.sum() == 48 and np.isfinite(X).all() and (stn[zero] == -3).all() and (stn[~zero] == 1).all()
    assert not any(np.isnan(C.expected(c)[0]).any() for c in cases.values())        # no NaN out: bit equality has no payload to argue about


def test_host_build_equals_the_restatement(g13, host_lib):
    g = g13
    for case in C.value_cases(g) + C.degenerate_cases(g):
        X, status = host_triangulate(host_lib, *case[1:])
        Xo, so = C.expected(case)
        bad_x, bad_s = int((bits(X) != bits(Xo)).any(1).sum()), int((status != so).sum())
        assert bad_x == 0 and bad_s == 0, f"{case[0]}: {bad_x} points and {bad_s} statuses of {len(so)} differ"
    X, status = host_triangulate(host_lib, g["und0"], g["P0"], g["und1"], g["P1"], 3e-5, 10)
    Xo, so = S.triangulate_iterative(g["und0"], g["P0"], g["und1"], g["P1"], 3e-5, 10)
    assert np.array_equal(bits(X), bits(Xo)) and np.array_equal(status, so)
    for k in ("0", "1"):
        assert np.array_equal(bits(host_undistort(host_lib, g["kpts" + k], g["K" + k], g["dist" + k])), bits(g["und" + k]))
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(0, 6012, 5000), rng.uniform(0, 4008, 5000)], 1).astype(np.float32)
    pts[:6] = [[np.nan, 1.0], [np.inf, 2.0], [3.0, -np.inf], [3.0e38, 3.0e38], [0.0, 0.0], [-5000.0, 9000.0]]
    for dist in (g["dist0"], g["dist0"][:4], None, np.r_[g["dist1"], 0.01, -0.02, 0.005], np.array([-0.9, 0.0, 0.0, 0.0])):
        got, want = host_undistort(host_lib, pts, g["K0"], dist), S.undistort_points_f64(pts, g["K0"], dist)
        # The NaN rows are rows 0..2 (a NaN or infinite coordinate: r2 is NaN or inf, and inf / inf or 0 * inf makes both coordinates
        # NaN) and, with the eight-term model alone, row 3 (3e38: within the five iterations both polynomials of icdist overflow, inf / inf). Such a NaN comes out of
        # an invalid operation, whose sign IEEE 754 leaves open, so only there "NaN on both sides" stands in for equal bits.
        both_nan = np.isnan(got) & np.isnan(want)
        assert np.array_equal(bits(got)[~both_nan], bits(want)[~both_nan]), dist
        assert both_nan[:3].all() and not both_nan[4:].any() and both_nan[3].all() == both_nan[3].any() == (dist is not None and len(dist) == 8), dist


# ---- the table contract --------------------------------------------------------------------------------------------------------------
def test_table_restatement_is_the_flat_calls_per_record(g13):
    g = g13
    rng = np.random.default_rng(11)
    K = 96
    cuts = [(0, 60), (60, 60), (5040, 5100), (4990, 5053)]
    epochs = [S.scatter_matches(rng, g["kpts0"][a:b], g["kpts1"][a:b], K) for a, b in cuts]
    epochs.insert(2, None)
    cuts.insert(2, (0, 0))
    table = S.pack_table(epochs, K)
    pair = [S.camera_row(g["P0"], g["K0"], g["dist0"]), S.camera_row(g["P1"], g["K1"], g["dist1"])]
    total = int(np.maximum(table[:, 3], 0).sum())
    assert total == 60 + 60 + 63
    for undistort in (1, 0):
        off, X, st, u0, u1 = S.triangulate_table(table, K, [pair], undistort, 3e-5, 10, total)
        assert off.dtype == np.int64 and off.tolist() == [0, 60, 60, 60, 120, 183] and len(X) == len(st) == len(u0) == len(u1) == total
        for e, (a, b) in enumerate(cuts):
            p0, p1 = g["kpts0"][a:b], g["kpts1"][a:b]
            if undistort:
                p0, p1 = S.undistort_points_f64(p0, g["K0"], g["dist0"]), S.undistort_points_f64(p1, g["K1"], g["dist1"])
            Xf, sf = S.triangulate_iterative(p0, g["P0"], p1, g["P1"], 3e-5, 10)
            rows = slice(off[e], off[e + 1])
            assert np.array_equal(bits(X[rows]), bits(Xf)) and np.array_equal(st[rows], sf), (undistort, e)
            assert np.array_equal(bits(u0[rows]), bits(p0)) and np.array_equal(bits(u1[rows]), bits(p1))
    # the capacity cuts the rows and never the offsets; one pair per record: the record's own
    off2, X2, st2, _, _ = S.triangulate_table(table, K, [pair], 1, 3e-5, 10, 100)
    assert np.array_equal(off2, off) and len(X2) == 100 and np.array_equal(st2, S.triangulate_table(table, K, [pair], 1, 3e-5, 10, total)[2][:100])
    pairs = [pair, pair, pair, [pair[1], pair[0]], pair]
    _, X3, st3, _, _ = S.triangulate_table(table, K, pairs, 1, 3e-5, 10, total)
    Xa = S.triangulate_table(table, K, [pair], 1, 3e-5, 10, total)[1]
    assert np.array_equal(bits(X3[:60]), bits(Xa[:60])) and np.array_equal(bits(X3[120:]), bits(Xa[120:])) and (X3[60:120] != Xa[60:120]).any(1).all()
    # a header that promises more: NaN rows with status 0; one that promises fewer: the first ones in slot order; a negative one: nothing
    t2 = table.copy()
    t2[0, 3], t2[3, 3], t2[4, 3] = 65, 10, -7
    off4, X4, st4, u04, _ = S.triangulate_table(t2, K, [pair], 1, 3e-5, 10, 10 ** 6)
    assert off4.tolist() == [0, 65, 65, 65, 75, 75] and len(X4) == 75
    assert np.isnan(X4[60:65]).all() and (st4[60:65] == 0).all() and np.isnan(u04[60:65]).all()
    assert np.array_equal(bits(X4[:60]), bits(Xa[:60])) and np.array_equal(bits(X4[65:75]), bits(Xa[60:70]))
    # entries of matches0 outside [0, K) are no matches
    t3 = table.copy()
    slots = np.flatnonzero(t3[0, S.HEADER:S.HEADER + K] >= 0)
    t3[0, S.HEADER + slots[[1, 5, 7]]] = [K, -2, np.iinfo(np.int32).max]
    _, X5, _, _, _ = S.triangulate_table(t3, K, [pair], 1, 3e-5, 10, total)
    keep = np.delete(np.arange(60), [1, 5, 7])
    assert np.array_equal(bits(X5[:57]), bits(Xa[keep])) and np.isnan(X5[57:60]).all() and np.array_equal(bits(X5[60:]), bits(Xa[60:]))
