"""The host plumbing around the geometry stages, on the device: RANSAC, linear triangulation and the two stabilisation launches are
timed by `im_profile_begin / end` under their own names and compute the same bits with profiling on; linear triangulation takes its
projection matrices by value (re-pinned at the 64-thread block boundary); a refused call leaves its context usable."""
import ctypes
import json

import numpy as np
import pytest
import torch

import geometry_oracle as go
from test_gpu_geometry import _cameras, _project, _triangulate, ransac, two_view

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _small_cameras():
    from icepy4d_amd.core import Camera
    K = np.array([[9.0, 0, 3.4], [0, 9.5, 2.6], [0, 0, 1]])
    dist = np.array([0.08, -0.02, 0.001, -0.002, 0.003])
    a = 0.03
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    return Camera(7, 5, K, dist, R=np.eye(3), t=np.zeros(3)), Camera(7, 5, K, dist, R=R, t=np.zeros(3))


def _stage_calls(e):
    """One call of every launch this file is about; every output as bytes."""
    from icepy4d_amd.utils import homography as hom
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    cam0, cam1 = _small_cameras()
    und = hom.undistort_image(frames[0], cam1, engine=e)
    warped = hom.homography_warping(cam0, cam1, frames[1], undistort=False, engine=e)
    assert und.shape == warped.shape == (5, 7, 3) and und.any() and warped.any()
    p0, p1 = two_view(5, 8, 0.5, 0.0)
    F, mask, info = ransac(e, p0, p1, 65, 1.0, 11)
    assert info[0] >= 0 and 0 <= info[1] < 65, info             # written: ransac() starts the outputs as sentinels
    P0, P1, x0, x1 = _tri_case(65)
    X = _triangulate(e, P0, P1, x0, x1)
    return [a.tobytes() for a in (und, warped, F, mask, info, X)]


def _tri_case(n):
    rng = np.random.default_rng(100 + n)
    P0, P1, _, _ = _cameras(4000.0, 1.0)
    depth = 10.0 * rng.uniform(0.8, 1.25, n)
    X = np.c_[rng.uniform(-0.5, 0.5, n) * depth, rng.uniform(-0.3, 0.3, n) * depth, depth]
    x0 = _project(P0, X) + np.c_[rng.normal(0, 0.5, (n, 2)), np.zeros(n)]
    x1 = _project(P1, X) + np.c_[rng.normal(0, 0.5, (n, 2)), np.zeros(n)]
    return P0, P1, x0, x1


def test_stage_launches_are_profiled_and_profiling_changes_no_bit(eng):
    plain = _stage_calls(eng)
    eng.ctx.call("im_profile_begin")
    timed = _stage_calls(eng)
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    eng.ctx.call("im_profile_end", buf, len(buf))
    prof = json.loads(buf.value.decode())
    prof.pop("_empty_event_pair", None)
    assert {k: v["count"] for k, v in prof.items()} == {"undistort_image": 1, "warp_perspective": 1, "ransac_hypotheses": 1,
                                                        "ransac_select": 1, "triangulate_linear": 1}, prof
    assert timed == plain
    assert _stage_calls(eng) == plain                           # and off again


@pytest.mark.parametrize("n", [1, 64, 65])
def test_triangulation_by_value_equals_itself_and_the_oracle(eng, n):
    """The bound of `test_gpu_geometry.test_triangulation_equals_oracle`: 8 x the oracle's conditioning bound of every point."""
    P0, P1, x0, x1 = _tri_case(n)
    Xd = _triangulate(eng, P0, P1, x0, x1)
    assert Xd.shape == (n, 4) and np.array_equal(Xd.view(np.int64), _triangulate(eng, P0, P1, x0, x1).view(np.int64))
    Xo, bound = go.triangulate(P0, P1, x0, x1)
    assert (Xd[:, 3] == 1.0).all()
    err = np.abs(Xd - Xo).max(1) / np.abs(Xo).max(1)
    assert (err <= 8 * bound).all(), (err.max(), (err / bound).max())


def test_triangulation_of_no_points_takes_null_pointers(eng):
    P0, P1, _, _ = _cameras(4000.0, 1.0)
    p0, p1 = np.ascontiguousarray(P0.reshape(12)), np.ascontiguousarray(P1.reshape(12))
    rc = eng.ctx.lib.im_triangulate_linear(eng.ctx.h, p0.ctypes.data, p1.ctypes.data, None, None, 0, None, eng.stream_ptr())
    assert rc == 0
    assert _triangulate(eng, P0, P1, np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 4)


def test_a_refused_call_leaves_the_context_usable(eng):
    """Each refusal returns its code; the valid call right after it gives the bits it gave before."""
    from icepy4d_amd._lib import IcematchError, ptr
    from icepy4d_amd.utils import point_cloud_filters as pcf
    st = eng.stream_ptr()
    # RANSAC with seven correspondences
    p0, p1 = two_view(5, 8, 0.5, 0.0)
    before = [a.tobytes() for a in ransac(eng, p0, p1, 65, 1.0, 11)]
    with pytest.raises(IcematchError) as ei:
        ransac(eng, p0[:7], p1[:7], 65, 1.0, 11)
    assert ei.value.rc == -70
    assert [a.tobytes() for a in ransac(eng, p0, p1, 65, 1.0, 11)] == before
    # a warp whose destination overlaps its source
    src = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (1, 5, 7, 3), dtype=np.uint8)).to(eng.device)
    minv = torch.from_numpy(np.array([1.0, 0.02, 0.3, -0.01, 1.0, 0.2, 0, 0, 1])).to(eng.device)
    dst = torch.zeros_like(src)

    def warp(d_dst):
        return eng.ctx.lib.im_warp_perspective(eng.ctx.h, ptr(src), 1, 5, 7, 3, ptr(minv), 5, 7, d_dst, st)
    assert warp(ptr(dst)) == 0
    before = dst.cpu().numpy().tobytes()
    assert warp(ptr(src) + 8) == -74
    dst.zero_()
    assert warp(ptr(dst)) == 0 and dst.cpu().numpy().tobytes() == before
    # k-NN with k = 65
    pts = np.random.default_rng(6).uniform(0, 1, (100, 3))
    before = {k: v.cpu().numpy().tobytes() for k, v in pcf.knn_self(pts, 5, engine=eng).items() if torch.is_tensor(v)}
    d_pts = torch.from_numpy(pts).to(eng.device)
    perm = torch.arange(100, dtype=torch.int64, device=eng.device)
    start = torch.tensor([0, 100], dtype=torch.int32, device=eng.device)
    grid = np.array([0.0, 0.0, 0.0, 1.0])
    rc = eng.ctx.lib.im_knn_self(eng.ctx.h, ptr(d_pts), ptr(perm), ptr(start), 100, grid.ctypes.data, 1, 1, 1, 65, float("inf"),
                                 None, None, None, None, None, None, st)
    assert rc == -75
    after = {k: v.cpu().numpy().tobytes() for k, v in pcf.knn_self(pts, 5, engine=eng).items() if torch.is_tensor(v)}
    assert after == before and before
