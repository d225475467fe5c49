"""Undistortion, least-squares triangulation and the match-table reconstruction on the device (csrc/sfm.hip) against the reference's
outputs (tests/golden/g13_sfm.npz, tools/gen_golden_sfm.py) and the numpy restatement (tests/sfm_oracle.py).

Bounds:
  undistortion   float32 output identical to the fixture and to the restatement (same float64 operations in the same order; on the
                 24 MP frame no float32 result sits within 1e-6 ulp of a rounding boundary, so the identity does not hang on the last
                 float64 bits). Five iterations leave ~1e-6 px of round-trip error: the algorithm's own, not tested here.
  triangulation  status and points identical to the restatement; against the fixture status identical and
                 |X - X_ref| <= 1e-9 * max(1, |X_ref|) where the stored cond(A) <= 1e3 (the project's bound for g10), scaled by
                 cond / 1e3 above. Points whose stored margin to the convergence tolerance is below 1e-6 may be left out, on at
                 most 1 % of the points (the fixture has none).
  fused / table  bit-identical to the separate calls; colours bit-identical to `interpolate_point_colors`, within 1e-12 of the fixture."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sfm_oracle as S  # noqa: E402

pytestmark = pytest.mark.gpu
FRAME = (4008, 6012)


@pytest.fixture(scope="module")
def g13():
    return S.load_g13(os.path.join(ROOT, "tests", "golden", "g13_sfm.npz"))


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


@pytest.fixture(scope="module")
def image():
    return S.image_pattern(*FRAME)


def cameras(g):
    """The fixture's two cameras as plain objects: K, dist, R, t of P = K [R | t] (and P itself)."""
    out = []
    for k in ("0", "1"):
        K, P = g["K" + k], g["P" + k]
        Rt = np.linalg.solve(K, P)
        ext = g["ro_cam0_extrinsics"] if k == "0" else g["ro_cam1_extrinsics"]
        assert np.allclose(Rt, ext[:3], atol=1e-9)
        out.append(types.SimpleNamespace(K=K, dist=g["dist" + k], R=ext[:3, :3], t=ext[:3, 3:4], P=P))
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def check_points(X, status, g, sel=slice(None), ref="X"):
    """The triangulation bounds of the module docstring."""
    Xr, cond, margin = g[ref][sel], g["cond"][sel], g["margin"][sel]
    if status is not None:
        assert np.array_equal(status, g["status"][sel].astype(np.int64))
    skip = margin < 1e-6 if ref == "X" else np.zeros(len(Xr), bool)
    assert skip.sum() <= 1e-2 * len(Xr)
    err = np.linalg.norm(X - Xr, axis=1)
    lim = 1e-9 * np.maximum(1.0, np.linalg.norm(Xr, axis=1)) * np.maximum(1.0, cond / 1e3)
    worst = float(np.max((err / lim)[~skip]))
    print(f"triangulation vs {ref}: worst error / bound {worst:.3g} on {int((~skip).sum())} points")
    assert np.all(err[~skip] <= lim[~skip]), worst


def test_undistort_points_identical(g13, eng):
    from icepy4d_amd import sfm
    c0, c1 = cameras(g13)
    for k, cam in (("0", c0), ("1", c1)):
        und = sfm.undistort_points(g13["kpts" + k], cam, engine=eng)
        assert und.dtype == np.float32 and und.shape == g13["kpts" + k].shape
        assert np.array_equal(bits(und), bits(g13["und" + k]))
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(0, FRAME[1], 200000), rng.uniform(0, FRAME[0], 200000)], 1).astype(np.float32)
    for dist in (g13["dist0"], g13["dist0"][:4], None, np.r_[g13["dist1"], 0.01, -0.02, 0.005]):
        cam = types.SimpleNamespace(K=g13["K0"], dist=dist)
        assert np.array_equal(bits(sfm.undistort_points(pts, cam, engine=eng)), bits(S.undistort_points_f64(pts, cam.K, dist)))
    # the icdist < 0 guard
    cam = types.SimpleNamespace(K=g13["K0"], dist=np.array([-0.9, 0.0, 0.0, 0.0]))
    far = np.array([[0.0, 0.0], [6000.0, 4000.0], [3000.0, 1900.0]], np.float32)
    out = sfm.undistort_points(far, cam, engine=eng)
    assert np.array_equal(bits(out), bits(S.undistort_points_f64(far, cam.K, cam.dist))) and np.array_equal(out[0], far[0])
    assert sfm.undistort_points(np.zeros((0, 2), np.float32), cam, engine=eng).shape == (0, 2)


def test_iterative_triangulation_matches_reference(g13, eng):
    from icepy4d_amd import sfm
    X, status = sfm.iterative_LS_triangulation(g13["und0"], g13["P0"], g13["und1"], g13["P1"], engine=eng)
    assert X.dtype == np.float64 and X.shape == (len(g13["X"]), 3) and status.dtype == np.int64
    check_points(X, status, g13)
    assert set(np.unique(status).tolist()) >= {1, -2, -3}
    # the restatement follows the same operations in the same order: the same bits
    Xo, so = S.triangulate_iterative(g13["und0"], g13["P0"], g13["und1"], g13["P1"])
    assert np.array_equal(so, status) and np.array_equal(bits(X), bits(Xo))
    # float64 points take the float64 kernel: the same values here, since float32 converts exactly
    X64, s64 = sfm.iterative_LS_triangulation(g13["und0"].astype(np.float64), g13["P0"], g13["und1"].astype(np.float64), g13["P1"], engine=eng)
    assert np.array_equal(bits(X64), bits(X)) and np.array_equal(s64, status)
    Xe, se = sfm.iterative_LS_triangulation(np.zeros((0, 2), np.float32), g13["P0"], np.zeros((0, 2), np.float32), g13["P1"], engine=eng)
    assert Xe.shape == (0, 3) and se.shape == (0,)


def test_linear_ls_triangulation_is_one_solve(g13, eng):
    from icepy4d_amd import sfm
    X, status = sfm.linear_LS_triangulation(g13["und0"], g13["P0"], g13["und1"], g13["P1"], engine=eng)
    assert status.dtype == bool and status.all() and len(status) == len(X)
    check_points(X, None, g13, ref="X_linear")


def test_fused_undistortion_is_the_two_calls(g13, eng):
    from icepy4d_amd import sfm
    c0, c1 = cameras(g13)
    dX, dst, u0, u1 = sfm._triangulate_device(eng, g13["kpts0"], g13["kpts1"], sfm._projection(c0), sfm._projection(c1),
                                              sfm._intrinsics(c0), sfm._intrinsics(c1), want_und=True)
    X, status = sfm.iterative_LS_triangulation(sfm.undistort_points(g13["kpts0"], c0, engine=eng), c0.P,
                                               sfm.undistort_points(g13["kpts1"], c1, engine=eng), c1.P, engine=eng)
    assert np.array_equal(bits(dX.cpu().numpy()), bits(X)) and np.array_equal(dst.cpu().numpy(), status)
    assert np.array_equal(bits(u0.cpu().numpy()), bits(g13["und0"])) and np.array_equal(bits(u1.cpu().numpy()), bits(g13["und1"]))


def test_triangulate_class_with_colours(g13, eng, image):
    from icepy4d_amd import sfm
    cams = cameras(g13)
    t = sfm.Triangulate(cams, [g13["kpts0"], g13["kpts1"]], engine=eng)
    X = t.triangulate_two_views(compute_colors=True, image=image, cam_id=1)
    assert X is t.points3d and t.colors.shape == (len(X), 3) and t.colors.dtype == np.float64
    check_points(X, t.status, g13)
    assert np.array_equal(bits(t.colors), bits(sfm.interpolate_point_colors(X, image, cams[1], engine=eng)))
    # the colours of the reference's own points, then ours against the fixture (identical wherever the projections agree)
    ref_cols = sfm.interpolate_point_colors(g13["X"], image, cams[1], engine=eng)
    assert np.max(np.abs(ref_cols - g13["colors"])) <= 1e-12
    same = np.all(sfm.project_points(X, cams[1], engine=eng) == sfm.project_points(g13["X"], cams[1], engine=eng), axis=1)
    print(f"colours: {int(same.sum())} of {len(same)} points project to the same float32 pixel position as the reference's")
    assert same.mean() > 0.9 and np.max(np.abs(t.colors[same] - g13["colors"][same])) <= 1e-12
    again = t.interpolate_colors_from_image(image, cams[1])
    assert np.array_equal(bits(again), bits(t.colors))


def test_linear_triangulation_approach(g13, eng):
    from icepy4d_amd import sfm
    cams = cameras(g13)
    n = 800
    t = sfm.Triangulate(cams, [g13["kpts0"][:n], g13["kpts1"][:n]], engine=eng)
    X = t.triangulate_two_views(approach="linear_triangulation")
    h0, h1 = np.c_[g13["und0"][:n].astype(np.float64), np.ones(n)], np.c_[g13["und1"][:n].astype(np.float64), np.ones(n)]
    ref = sfm.triangulate_points_linear(cams[0].P, cams[1].P, h0, h1, engine=eng)
    assert np.array_equal(bits(X), bits(ref[:, :3] / ref[:, 3:4])) and t.colors is None
    assert t.triangulate_two_views(approach="something else") is X


def test_table_mode(g13, eng, image):
    import torch
    from icepy4d_amd import sfm
    from icepy4d_amd.sequence import record_words
    cams = cameras(g13)
    rng = np.random.default_rng(7)
    K = 1024
    cuts = [0, 700, 700, 1500, 2100, 5200]               # epoch 1 is empty; a failed record sits between 2 and 3
    epochs, sel = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        b = min(b, a + 650)
        epochs.append(S.scatter_matches(rng, g13["kpts0"][a:b], g13["kpts1"][a:b], K))
        sel.append((a, b))
    epochs.insert(3, None)
    sel.insert(3, (0, 0))
    table = S.pack_table(epochs, K)
    assert table.shape == (6, record_words(K, True))
    want = np.r_[0, np.cumsum(np.maximum(table[:, 3], 0))]
    rec = sfm.triangulate_table(torch.from_numpy(table).to(eng.device), K, cams, engine=eng, image=image, cam_id=1)
    assert rec.offsets.dtype == np.int64 and np.array_equal(rec.offsets, want) and len(rec.points3d) == 6
    assert len(rec.points3d[1]) == 0 and len(rec.points3d[3]) == 0 and len(rec.status[3]) == 0 and rec.colors[3].shape == (0, 3)
    for e, (a, b) in enumerate(sel):
        t = sfm.Triangulate(cams, [g13["kpts0"][a:b], g13["kpts1"][a:b]], engine=eng)
        X = t.triangulate_two_views(compute_colors=b > a, image=image, cam_id=1)
        assert np.array_equal(bits(rec.points3d[e]), bits(X)) and np.array_equal(rec.status[e], t.status), e
        if b > a:
            assert np.array_equal(bits(rec.colors[e]), bits(t.colors)), e
            check_points(rec.points3d[e], rec.status[e], g13, slice(a, b))
    # one camera pair per record, no undistortion, host table: the flat call on the raw keypoints
    rec2 = sfm.triangulate_table(table, K, [cams] * 6, engine=eng, undistort=False)
    a, b = sel[4]
    X, status = sfm.iterative_LS_triangulation(g13["kpts0"][a:b], cams[0].P, g13["kpts1"][a:b], cams[1].P, engine=eng)
    assert rec2.colors is None and np.array_equal(bits(rec2.points3d[4]), bits(X)) and np.array_equal(rec2.status[4], status)
    # a header that promises more matches than matches0 holds: the surplus rows are NaN with status 0, nothing else moves
    broken = table.copy()
    broken[0, 3] += 5
    rec3 = sfm.triangulate_table(broken, K, cams, engine=eng)
    n0 = int(table[0, 3])
    assert len(rec3.points3d[0]) == n0 + 5 and np.isnan(rec3.points3d[0][n0:]).all() and (rec3.status[0][n0:] == 0).all()
    assert np.array_equal(bits(rec3.points3d[0][:n0]), bits(rec.points3d[0])) and np.array_equal(bits(rec3.points3d[2]), bits(rec.points3d[2]))
    with pytest.raises(ValueError):
        sfm.triangulate_table(table[:, :-2], K, cams, engine=eng)
    empty = sfm.triangulate_table(table[:0], K, cams, engine=eng)
    assert empty.offsets.tolist() == [0] and empty.points3d == [] and empty.status == []
