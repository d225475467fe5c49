"""Image stabilisation without a device: the numpy restatement of the kernels (tests/warp_oracle.py) against the reference's outputs in
tests/golden/g15_stabilise.npz (tools/gen_golden_stabilise.py: the reference's modules with a stub cv2 whose resampling IS the
restatement), the host side of `icepy4d_amd/utils/homography.py`, and the kernels' own text compiled for the host.

Bounds: everything is exact. The fixture's images were made by the restatement, so it reproduces them bit for bit; H and the Euler
angles are the same numpy / libm calls in the same order as the reference's, so `np.array_equal`. `inv3` against LAPACK: 1e-12 relative,
the bound of the project's other 3 x 3 and 4 x 4 algebra (cond(K) of the scaled calibrations is about 1e4, cond(H) the same: 1e4 eps is
1e-12). The host build of csrc/warp_pixel.h equals the restatement on every case the device tests use: the same IEEE float64 operations
in the same order, division correctly rounded, rint to even, integers behind. That pins the operation order, the clamps and the
thresholds, not the contraction: the host build is for plain x86-64, which has no fused multiply-add, so a lost
`#pragma clang fp contract(off)` shows on the device only (tests/test_gpu_stabilise.py)."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import toolchain  # noqa: E402
import warp_oracle as W  # noqa: E402

N = 7
FRAME = (96, 144)


@pytest.fixture(scope="module")
def g15():
    with np.load(W.GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def cameras(g):
    from icepy4d_amd.core import Camera
    ref = Camera(FRAME[1], FRAME[0], g["ref_K"], g["ref_dist"], extrinsics=g["ref_extrinsics"].copy())
    return ref, [Camera(FRAME[1], FRAME[0], g[f"ep{e}_K"], g[f"ep{e}_dist"], extrinsics=g[f"ep{e}_extrinsics"].copy()) for e in range(N)]


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_oracle_and_camera_algebra_reproduce_g15(g15):
    from icepy4d_amd.utils import homography as hom
    g = g15
    ref, cams = cameras(g)
    assert g["H"].shape == (N, 3, 3) and g["warped"].shape == (N,) + FRAME + (3,)
    for e, cam in enumerate(cams):
        ext = cam.extrinsics.copy()
        H = hom.homography(ref, cam)
        assert np.array_equal(H, g["H"][e]), e
        assert np.array_equal(cam.extrinsics, ext)                                   # works on copies
        img = W.image_pattern(*FRAME, 3, seed=e)
        und = W.undistort(img, cam.K, cam.dist)
        assert np.array_equal(und, g["undistorted"][e]), e
        assert np.array_equal(W.warp_perspective(img, H, (FRAME[1], FRAME[0])), g["warped"][e]), e
        assert np.array_equal(W.warp_perspective(und, H, (FRAME[1], FRAME[0])), g["warped_undistorted"][e]), e
        assert np.array_equal(hom.inverse_homography(H).reshape(3, 3), W.inv3(H))
        assert np.array_equal(hom.undistort_params(cam), W.cam_row(cam.K, cam.dist))
    # what the fixture promises about itself: both calibrations, real motion, frames that stay mostly inside
    assert np.array_equal(g["ep0_K"], g["ref_K"]) and not np.array_equal(g["ep6_K"], g["ref_K"])
    assert all((g["warped"][e] != W.image_pattern(*FRAME, 3, seed=e)).mean() > 0.2 for e in range(N))
    assert (g["warped_undistorted"] != 0).mean() > 0.5 and (g["undistorted"] != g["warped"]).any()


def test_smoothing_reproduces_the_reference(g15):
    from icepy4d_amd.utils import homography as hom
    g = g15
    _, cams = cameras(g)
    for e, cam in enumerate(cams):
        assert np.array_equal(np.array(hom.euler_from_matrix(cam.R)), g["angles"][e])
        assert np.array_equal(np.array(W.euler_from_matrix(cam.R)), g["angles"][e])
    for name, use_median in (("median", True), ("mean", False)):
        ext = [c.extrinsics.copy() for c in cams]
        out = hom.smooth_camera_rotations(cams, window=5, use_median=use_median)
        assert all(np.array_equal(c.extrinsics, x) for c, x in zip(cams, ext))      # copies
        for e, cam in enumerate(out):
            assert np.array_equal(cam.R, g[f"smooth_{name}_R"][e]) and np.array_equal(cam.extrinsics, g[f"smooth_{name}_extrinsics"][e]), (name, e)
            ang = g[f"smooth_{name}_angles"][e]
            assert np.array_equal(hom.euler_matrix(*ang), g[f"smooth_{name}_R"][e]) and np.array_equal(W.euler_matrix(*ang), g[f"smooth_{name}_R"][e])
            assert np.array_equal(cam.t, cams[e].t) and cam.K is not None
    # the angles round-trip; gimbal lock takes the other branch and still reproduces the matrix
    R = hom.euler_matrix(0.3, -0.2, 1.1)
    assert np.allclose(hom.euler_from_matrix(R), (0.3, -0.2, 1.1), atol=1e-15)
    lock = hom.euler_matrix(0.4, np.pi / 2, 0.0)
    a = hom.euler_from_matrix(lock)
    assert a[2] == 0.0 and np.allclose(hom.euler_matrix(*a), lock, atol=1e-15)
    with pytest.raises(ValueError):
        hom.smooth_camera_rotations(cams[:4])


def test_window_rule():
    from icepy4d_amd.utils.homography import smoothing_window
    assert [list(smoothing_window(e, 5)) for e in range(5)] == [[0, 1, 2, 3, 4]] * 5
    assert [smoothing_window(e, 6)[0] for e in range(6)] == [0, 0, 0, 1, 1, 1]
    for ep in range(160):               # the driver's `match`: 0, 1, 158 and 159 are its hard-coded cases
        want = {0: range(0, 5), 1: range(0, 5), 158: range(155, 160), 159: range(155, 160)}.get(ep, range(ep - 2, ep + 3))
        assert smoothing_window(ep, 160) == want == W.window(ep, 160), ep
    assert list(smoothing_window(4, 9, window=3)) == [3, 4, 5] and list(smoothing_window(0, 1, window=1)) == [0]
    with pytest.raises(ValueError):
        smoothing_window(0, 4)


def test_inv3_against_lapack(g15):
    from icepy4d_amd.utils.homography import inv3
    g = g15
    mats = [g["ref_K"], g["calib_cam1_K"], g["calib_cam2_K"]] + [g[f"ep{e}_K"] for e in range(N)] + list(g["H"])
    for M in mats:
        got, ref = inv3(M), np.linalg.inv(M)
        assert np.array_equal(got, W.inv3(M))
        assert (np.abs(got - ref)[ref != 0] <= 1e-12 * np.abs(ref)[ref != 0]).all()           # entry by entry
        assert (np.abs(got[ref == 0]) <= 1e-12 * np.abs(ref).max()).all()
    # the order of the cofactors, on a matrix without any symmetry
    M = np.array([[2.0, -1.0, 3.0], [0.5, 4.0, -2.0], [1.5, 0.25, 5.0]])
    assert np.allclose(inv3(M) @ M, np.eye(3), atol=1e-14)


# ---- the properties of the restatement -------------------------------------------------------------------------------------------------
def test_identity_and_integer_translation():
    img = W.image_pattern(37, 70, 3, seed=2)
    assert np.array_equal(W.warp_perspective(img, np.eye(3), (70, 37)), img)
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1), (5, -3), (-64, 2)):
        H = np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])
        want = np.zeros_like(img)
        ys, xs = slice(max(dy, 0), 37 + min(dy, 0)), slice(max(dx, 0), 70 + min(dx, 0))
        yo, xo = slice(max(-dy, 0), 37 + min(-dy, 0)), slice(max(-dx, 0), 70 + min(-dx, 0))
        want[ys, xs] = img[yo, xo]
        assert np.array_equal(W.warp_perspective(img, H, (70, 37)), want), (dx, dy)


def test_constant_image_stays_constant_inside():
    img = np.full((40, 90, 3), 201, np.uint8)
    M = W.all_inverses(40, 90)["rotation 10 deg"]
    sx, sy = W.warp_coords(M, 40, 90)
    _, xi, _ = W.fix(sx)
    _, yi, _ = W.fix(sy)
    inside = (xi >= 0) & (xi + 1 < 90) & (yi >= 0) & (yi + 1 < 40)
    out = W.warp_perspective_inv(img, M, 40, 90)
    assert inside.mean() > 0.5 and (out[inside] == 201).all() and (out[~inside] < 201).any()
    K, d = W.scaled_calib("cam1", 90)
    und = W.undistort(img, K, d)
    assert (und[5:-5, 5:-5] == 201).all()


def test_zero_distortion_is_the_identity_on_full_width_rows():
    for cam in ("cam1", "cam2"):
        K, _ = W.scaled_calib(cam, W.FULL_WIDTH)
        img = W.image_pattern(3, W.FULL_WIDTH, 1, seed=1)
        for dist in (np.zeros(4), np.zeros(5), np.zeros(8)):
            assert np.array_equal(W.undistort(img, K, dist), img), cam
        # and on the rows at the bottom of the frame: the rows of a 4008-row image are addressed through i alone
        sx, sy = W.undistort_coords(W.inv3(K), [K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.zeros(8), 4008, 16)
        assert np.array_equal(W.fix(sx)[1], np.broadcast_to(np.arange(16), (4008, 16))) and (W.fix(sx)[2] == 0).all()
        assert np.array_equal(W.fix(sy)[1], np.broadcast_to(np.arange(4008)[:, None], (4008, 16))) and (W.fix(sy)[2] == 0).all()


def test_fix_rounds_to_even_and_saturates():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 31.5, 32.5, -33.0, 1e30, -1e30, 2147483647.0, np.nan, np.inf, -np.inf, 32767 * 32.0 + 31, 32768 * 32.0])
    ok, xi, f = W.fix(v)
    assert ok.tolist() == [True] * 11 + [False] * 3 + [True] * 2
    assert xi[:8].tolist() == [0, 0, 0, 0, -1, 1, 1, -2] and f[:8].tolist() == [0, 2, 2, 0, 30, 0, 0, 31]
    assert xi[8:11].tolist() == [32767, -32768, 32767] and f[8:11].tolist() == [31, 0, 31]
    assert xi[14:].tolist() == [32767, 32767] and f[14:].tolist() == [31, 0]


def test_the_cases_reach_every_path():
    """What tests/warp_oracle.py's case lists promise, from the restatement alone."""
    img = W.image_pattern(5, 65, 3, seed=0)
    inv = W.all_inverses(5, 65)
    sx, _ = W.warp_coords(inv["W crosses zero"], 5, 65)
    assert (sx[:, 3] == 0).all() and np.array_equal(W.warp_perspective_inv(img, inv["W crosses zero"], 5, 65)[:, 3], np.broadcast_to(img[0, 0], (5, 3)))
    assert (sx[:, :3] < 0).all()                                                       # W < 0 to the left
    assert not W.warp_perspective_inv(img, inv["outside"], 5, 65).any()
    big = W.warp_perspective_inv(img, inv["scale 1e12"], 5, 65)
    assert np.array_equal(big[0, 0], img[0, 0]) and not big[1:, 1:].any()
    ok, xi, _ = W.fix(W.warp_coords(inv["scale 1e12"], 5, 65)[0])
    assert ok.all() and xi.max() == 32767                                            # the int clamp, then the short clamp
    half = W.warp_perspective_inv(img, inv["half pixel"], 5, 65).astype(int)
    q = img.astype(int)
    assert np.array_equal(half[1:, 1:], (q[:-1, :-1] + q[:-1, 1:] + q[1:, :-1] + q[1:, 1:] + 2) >> 2)
    for name, M in inv.items():
        if name.startswith("shift"):
            out = W.warp_perspective_inv(img, M, 5, 65)
            assert (out == 0).all(axis=2).sum() in (5, 65) and out.any(), name       # one border row or column of zeros
    names = [c[0] for c in W.undistort_cases()]
    assert len(set(names)) == len(names)
    for case in W.undistort_cases():
        name, h, w, K, dist = case
        src, row = W.undistort_inputs(case)
        out = W.undistort_row(src[0], row)
        if name.startswith("zero distortion"):
            assert np.array_equal(out, src[0]), name
        else:
            assert not np.array_equal(out, src[0]), name
        if name.startswith("strong barrel"):
            assert not out[0, 0].any() and not out[-1, -1].any() and out[h // 2, w // 2].any()
        if name.startswith("one non-finite"):
            sx, sy = W.undistort_coords(row[:9], row[9:13], row[13:], h, w)
            # kr = 1 / 0 on the unit circle: v = 0 * inf = NaN at (0, 1); by symmetry u is NaN and v infinite at (1, 0)
            assert np.isnan(sy[0, 1]) and np.isnan(sx[1, 0]) and np.isinf(sy[1, 0]) and np.isfinite(sy).sum() == sy.size - 2
            assert not out[0, 1].any() and not out[1, 0].any() and np.array_equal(out[0, 0], src[0][0, 0])
    lens = {len(np.atleast_1d(c[4])) for c in W.undistort_cases()}
    assert lens >= {4, 5, 8}


# ---- the host side of the package ------------------------------------------------------------------------------------------------------
def test_argument_errors_before_any_device_work(g15):
    """Matrices, distortion lengths and image types are checked on the host, before an engine is asked for: `engine` is an object
    that has nothing, so any use of it would raise AttributeError, not ValueError."""
    from icepy4d_amd import sfm
    from icepy4d_amd.core import Camera
    from icepy4d_amd.utils import homography as hom
    ref, cams = cameras(g15)
    img = W.image_pattern(*FRAME, 3)
    engine = object()
    cam = types.SimpleNamespace(K=cams[0].K.copy(), dist=cams[0].dist.copy())
    for bad in (np.zeros(3), np.zeros(6), np.zeros(0), None, np.array([0.0, np.nan, 0.0, 0.0])):
        cam.dist = bad
        with pytest.raises(ValueError):
            sfm.undistort_image(img, cam, engine=engine)
    cam.dist = cams[0].dist.copy()
    for K in (np.zeros((3, 3)), np.diag([1.0, np.inf, 1.0]), np.diag([1.0, np.nan, 1.0]), np.eye(4), np.array([[1.0, 2.0, 3.0]] * 3)):
        cam.K = K
        with pytest.raises(ValueError):
            sfm.undistort_image(img, cam, engine=engine)
        if K.shape == (3, 3):
            full = Camera(FRAME[1], FRAME[0], K, cams[0].dist, extrinsics=cams[0].extrinsics.copy())
            for undistort in (True, False):
                with pytest.raises(ValueError):
                    hom.stabilise_sequence(ref, [full], [img], undistort=undistort, engine=engine)
                with pytest.raises(ValueError):
                    hom.homography_warping(ref, full, img, undistort=undistort, engine=engine)
    cam.K = cams[0].K.copy()
    for image in (img.astype(np.float32), img.astype(np.int8), img[0, 0], np.zeros((4, 4, 5), np.uint8), np.zeros((0, 4, 3), np.uint8),
                  np.zeros((2, 2, 2, 2), np.uint8), img.tolist()):
        with pytest.raises(ValueError):
            sfm.undistort_image(image, cam, engine=engine)
        with pytest.raises(ValueError):
            hom.homography_warping(ref, cams[0], image, engine=engine)
    # a singular H: a reference camera whose K has no focal length
    flat = types.SimpleNamespace(K=np.diag([0.0, 1.0, 1.0]), dist=ref.dist, pose=ref.pose, R=ref.R, extrinsics=ref.extrinsics,
                                 pose_to_extrinsics=ref.pose_to_extrinsics, update_extrinsics=lambda e: None)
    with pytest.raises(ValueError):
        hom.homography_warping(flat, cams[0], img, engine=engine)
    with pytest.raises(ValueError):
        hom.inverse_homography(np.diag([1.0, np.nan, 1.0]))
    with pytest.raises(ValueError):
        hom.inv3(np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 1.0, 1.0]]))
    with pytest.raises(ValueError):
        hom.stabilise_sequence(ref, cams[:2], [img], engine=engine)                  # counts differ
    with pytest.raises(ValueError):
        hom.stabilise_sequence(ref, cams[:2], [img, img[:50]], engine=engine)        # shapes differ
    with pytest.raises(ValueError):
        hom.stabilise_sequence(ref, [], [], engine=engine)


def test_symbols_declared_in_header_and_binding():
    from icepy4d_amd import _lib
    header = open(os.path.join(ROOT, "include", "icematch.h")).read()
    for name, nargs in (("im_undistort_image", 9), ("im_warp_perspective", 11)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert "-74" in header


# ---- the kernels' text on the host -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """tests/warp_host_harness.cpp + csrc/warp_pixel.h as a shared library, behind a stub <hip/hip_runtime.h>."""
    lib = toolchain.host_library(str(tmp_path_factory.mktemp("warp_host")), "warp_host_harness.cpp")
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.warp_host_perspective.argtypes, lib.warp_host_perspective.restype = [P, I, I, I, I, P, I, I, P], None
    lib.warp_host_undistort.argtypes, lib.warp_host_undistort.restype = [P, I, I, I, I, P, P], None
    return lib


def host_warp(lib, src, minv, oh, ow):
    src, minv = np.ascontiguousarray(src), np.ascontiguousarray(minv, np.float64)
    n, h, w, c = src.shape
    out = np.full((n, oh, ow, c), 0xA5, np.uint8)
    lib.warp_host_perspective(src.ctypes.data, n, h, w, c, minv.ctypes.data, oh, ow, out.ctypes.data)
    return out


def host_undistort(lib, src, row):
    src, row = np.ascontiguousarray(src), np.ascontiguousarray(row, np.float64)
    n, h, w, c = src.shape
    out = np.full(src.shape, 0xA5, np.uint8)
    lib.warp_host_undistort(src.ctypes.data, n, h, w, c, row.ctypes.data, out.ctypes.data)
    return out


def test_host_build_equals_the_restatement(g15, host_lib):
    for case in W.warp_cases():
        got, want = host_warp(host_lib, *case[1:]), W.warp_expected(case)
        assert got.shape == want.shape and np.array_equal(got, want), f"{case[0]}: {int((got != want).sum())} of {want.size} bytes differ"
    for case in W.undistort_cases():
        for c, n in ((3, 1), (1, 2), (4, 1)):
            src, row = W.undistort_inputs(case, c, n)
            got, want = host_undistort(host_lib, src, row), np.stack([W.undistort_row(s, row) for s in src])
            assert np.array_equal(got, want), f"{case[0]} (c = {c}): {int((got != want).sum())} of {want.size} bytes differ"
    # the fixture's epochs through the host build
    ref, cams = cameras(g15)
    imgs = np.stack([W.image_pattern(*FRAME, 3, seed=e) for e in range(N)])
    minv = np.stack([W.inv3(H).ravel() for H in g15["H"]])
    assert np.array_equal(host_warp(host_lib, imgs, minv, *FRAME), g15["warped"])
    for e, cam in enumerate(cams):
        assert np.array_equal(host_undistort(host_lib, imgs[e:e + 1], W.cam_row(cam.K, cam.dist))[0], g15["undistorted"][e]), e
