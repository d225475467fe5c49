"""Two-view dense stereo without a device: (a) the numpy restatement (tests/dense_oracle.py) against independent arithmetic and against the
truth of rendered scenes, (b) a host build of the kernels' own arithmetic (csrc/dense_pixel.h behind the stub <hip/hip_runtime.h>, in
tests/dense_host_harness.cpp, a stand-alone program built plain and with the address and undefined-behaviour sanitizers) against the
restatement bit for bit on every case of tests/dense_cases.py, (c) the host side of `icepy4d_amd.dense`: schedule, depth range, grey and
downscaling, refusals, the ABI, the scratch layout and the compiled resources of the kernels. The device run is tests/test_gpu_dense.py."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import toolchain  # noqa: E402
import dense_cases as DC  # noqa: E402
import dense_oracle as O  # noqa: E402

from icepy4d_amd import dense as D  # noqa: E402  (the feature under test: without it nothing here can pass)
from icepy4d_amd.core.camera import Camera  # noqa: E402

NAMES = ["im_dense_tile_w", "im_dense_tile_h", "im_dense_sweep", "im_dense_consistency", "im_dense_cloud"]


# ---- (a) the restatement against independent arithmetic --------------------------------------------------------------------------------------
def test_box_sums_equal_a_direct_49_term_loop():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 1 << 36, (13, 17), dtype=np.int64)
    got = O.box(img, 3)
    assert got.shape == (7, 11)
    for y in range(7):
        for x in range(11):
            s = 0
            for dy in range(7):
                for dx in range(7):
                    s += int(img[y + dy, x + dx])
            assert got[y, x] == s
    assert O.box(img, 7).shape == (0, 3) and O.box(img[:5], 3).shape == (0, 11)


def test_score_equals_corrcoef_of_the_integer_patches():
    """s = C / sqrt(VA VB) with C, VA, VB exact integers below 2^52: the product, the root and the quotient round once each, so s is
    within 3 * 2^-53 (relative) of the exact correlation, which is at most 1 in magnitude. np.corrcoef subtracts a rounded mean (relative
    error n u, u = 2^-53) from values up to M = max |x| and accumulates n products: its deviations carry an absolute error of about
    (n + 1) u M, i.e. (n + 1) u M / sigma relative to their scale sigma, once for either patch and again through either variance, and the
    n-term sums add n u. Bound: 4 u (n + 1) (1 + M_a / sigma_a + M_b / sigma_b), evaluated per patch."""
    c = DC.sweeps()["radius_3"]
    r, n = 3, 49
    a = c["ref"].astype(np.int64)
    b, ok = O.sample(c["src"], O.plane_h(c["A"], c["B"], c["w_first"], c["w_step"], 1), *a.shape)
    valid, s = O.score(n, O.box(a, r), O.box(a * a, r), O.box(b, r), O.box(b * b, r), O.box(a * b, r), 4)
    assert ok.all() and valid.sum() > 1000
    u, worst = 2.0 ** -53, 0.0
    for y, x in zip(*np.nonzero(valid)):
        pa, pb = a[y:y + 7, x:x + 7].ravel().astype(np.float64), b[y:y + 7, x:x + 7].ravel().astype(np.float64)
        bound = 4 * u * (n + 1) * (1 + pa.max() / pa.std() + pb.max() / pb.std())
        err = abs(s[y, x] - np.corrcoef(pa, pb)[0, 1])
        worst = max(worst, err / bound)
        assert err <= bound, (y, x, err, bound)
    print("largest error / bound:", worst)


def recovered(c):
    plane, w, score = O.sweep(c["ref"], c["src"], c["A"], c["B"], c["w_first"], c["w_step"], c["D"], c["r"], c["min_var"], c["min_score"])
    kept = plane >= 0
    err = np.abs((w - c["w_first"]) / c["w_step"] - c["k_true"])[kept]           # every kept pixel counts
    return plane, kept, err


def test_a_fronto_parallel_plane_on_a_hypothesis_is_found():
    """48 x 80, f = 120 px, 13 planes one pixel of disparity apart, r = 3, min_score = 0.9, the surface on plane 6. Tolerances cannot be
    derived; measured with this restatement: 80.9 % of the pixels kept (the window's border alone drops 19.1 %), the plane index exact
    at every kept pixel, the sub-plane offset off by at most 0.2004 plane steps (the parabola through three scores of an asymmetric
    correlation peak). Asserted: the kept share the issue sets (>= 0.7), the exact index, and 0.25, the next power of two above 0.2004."""
    c = DC.pair(1, 48, 80, 13, 3, min_score=0.9, k_true=6)
    plane, kept, err = recovered(c)
    print("kept", kept.mean(), "worst", err.max())
    assert kept.mean() >= 0.7
    assert (plane[kept] == 6).all()
    assert err.max() <= 0.25


def test_a_slanted_plane_is_found():
    """The same scene with the surface tilted by 0.06 planes per pixel along u and 0.05 along v (4.8 and 2.4 planes across the image).
    Measured with this restatement: 75.6 % kept, worst error 0.316 plane steps, 99th percentile 0.196. Asserted: the kept share the issue
    sets (>= 0.45), and the next powers of two above the measured errors, 0.5 and 0.25."""
    c = DC.pair(1, 48, 80, 13, 3, min_score=0.9, slant=(0.06, 0.05))
    plane, kept, err = recovered(c)
    print("kept", kept.mean(), "worst", err.max(), "p99", np.percentile(err, 99))
    assert kept.mean() >= 0.45
    assert err.max() <= 0.5 and np.percentile(err, 99) <= 0.25


def test_the_cases_reach_what_they_are_named_for():
    S = DC.sweeps()
    vol = lambda c: O.scores(c["ref"], c["src"], c["A"], c["B"], c["w_first"], c["w_step"], c["D"], c["r"], c["min_var"])  # noqa: E731
    # a best plane inside the schedule whose neighbour is invalid: no offset
    c = S["window_leaves_src"]
    valid, s = vol(c)
    plane, w, _ = DC.sweep_oracle("window_leaves_src")
    ii, jj = np.nonzero((plane >= 1) & (plane <= c["D"] - 2))
    lonely = ~(valid[plane[ii, jj] - 1, ii, jj] & valid[plane[ii, jj] + 1, ii, jj])
    assert lonely.any() and (w[ii, jj][lonely] == c["w_first"] + plane[ii, jj][lonely].astype(np.float64) * c["w_step"]).all()
    assert not valid.all(0)[c["r"]:-c["r"], c["r"]:-c["r"]].all()                 # part of a window leaves src
    # z <= 0 for some pixels, > 0 for others
    c = S["z_not_positive"]
    z = [(H[6] * np.arange(70.0) + H[8]) for H in [O.plane_h(c["A"], c["B"], c["w_first"], c["w_step"], 0)]][0]
    assert (z <= 0).any() and (z > 0).any()
    assert (DC.sweep_oracle("nan_in_A")[0] == -1).all() and (DC.sweep_oracle("ref_smaller_than_window")[0] == -1).all()
    # texture thresholds: the flat patches drop pixels that min_var = 0 drops too (a zero variance never scores), and VA is what drops them
    for name in ("constant_patch_in_ref", "constant_patch_in_src"):
        p4, p0 = DC.sweep_oracle(name)[0], DC.sweep_oracle(name + "_min_var_0")[0]
        full = DC.sweep_oracle("planes_3")[0]
        assert (p4 >= 0).sum() < (full >= 0).sum() and ((p0 >= 0) | (p4 < 0)).all()
    assert (DC.sweep_oracle("constant_patch_in_ref")[0][8:12, 14:26] == -1).all()
    # ties: index 0 and no offset
    plane, w, _ = DC.sweep_oracle("all_planes_tie")
    assert set(np.unique(plane)) == {-1, 0} and (w[plane == 0] == S["all_planes_tie"]["w_first"]).all()
    for name, k in (("best_at_first_plane", 0), ("best_at_last_plane", 4)):
        plane, w, _ = DC.sweep_oracle(name)
        c = S[name]
        assert (plane[plane >= 0] == k).all() and (w[plane >= 0] == c["w_first"] + float(k) * c["w_step"]).all()
    assert (DC.sweep_oracle("slanted")[1][DC.sweep_oracle("slanted")[0] >= 0] % S["slanted"]["w_step"] != 0).any()      # offsets in use
    # consistency: a pixel that projects outside view 1, and one that lands on a dropped pixel
    c0, c1, m0, m1 = DC.two_maps("crafted")
    kept = m0[0] >= 0
    X0 = O.backproject(O.W.inv3(c0["K0"]), *kept.shape, np.where(kept, m0[1], 1.0))
    p = (X0 @ c0["R"].T + c0["t"]) @ c0["K1"].T
    u1, v1 = np.rint(p[..., 0] / p[..., 2]), np.rint(p[..., 1] / p[..., 2])
    h1, w1 = m1[0].shape
    inside = kept & (p[..., 2] > 0) & (u1 >= 0) & (u1 < w1) & (v1 >= 0) & (v1 < h1)
    assert (kept & (p[..., 2] <= 0)).any() and (kept & (p[..., 2] > 0) & ((u1 < 0) | (u1 >= w1))).any()
    assert (m1[0][v1[inside].astype(np.int64), u1[inside].astype(np.int64)] < 0).any()
    assert 0 < DC.consistency_oracle("crafted", "MildFiltering").sum() < inside.sum()
    _, _, m0, _ = DC.two_maps("same_size")
    kept = m0[0] >= 0
    counts =[int(DC.consistency_oracle("same_size", f).sum()) for f in ("NoFiltering", "MildFiltering", "ModerateFiltering", "AggressiveFiltering")]
    assert counts[0] == kept.sum() and counts[0] > counts[1] >= counts[2] > counts[3] > 0
    # normals with zero, one and two kept neighbours per direction
    case, out = DC.cloud_case("half_kept")
    k = case["keep"] != 0
    left, right = np.zeros_like(k), np.zeros_like(k)
    left[:, 1:], right[:, :-1] = k[:, :-1], k[:, 1:]
    assert all((k & (left.astype(int) + right == m)).any() for m in (0, 1, 2))
    zero = (out[2] == 0).all(1)
    assert zero.any() and not zero.all() and np.allclose(np.linalg.norm(out[2][~zero], axis=1), 1.0, atol=1e-12)
    C0 = O.to_world(case["cam"], np.zeros(3))
    assert (((C0 - out[0][~zero]) * out[2][~zero]).sum(1) >= 0).all()            # towards the camera
    assert [len(DC.cloud_case(n)[1][0]) for n in ("empty", "one_point", "count_255", "count_256", "count_257", "count_65537")] == [0, 1, 255, 256, 257, 65537]


# ---- (b) the host build of the kernels' arithmetic ---------------------------------------------------------------------------------------------
def record(f, kind, name, ints, doubles, arrays):
    f.write(struct.pack("<qq", kind, len(name)) + name.encode())
    f.write(np.asarray(ints, np.int64).tobytes() + np.asarray(doubles, np.float64).tobytes())
    for a, t in arrays:
        f.write(np.ascontiguousarray(a, t).tobytes())


def write_records(path):
    n = 0
    with open(path, "wb") as f:
        for name, c in DC.sweeps().items():
            plane, w, score = DC.sweep_oracle(name)
            record(f, 1, "sweep " + name, [*c["ref"].shape, *c["src"].shape, c["D"], c["r"], c["min_var"]],
                   [*c["A"], *c["B"], c["w_first"], c["w_step"], c["min_score"]],
                   [(c["ref"], np.uint8), (c["src"], np.uint8), (plane, np.int16), (w, np.float64), (score, np.float32)])
            n += 1
        for pname, flt in DC.CONSISTENCY:
            c0, c1, m0, m1 = DC.two_maps(pname)
            tau = O.filter_tau(flt)
            record(f, 2, f"consistency {pname} {flt}", [*m0[0].shape, *m1[0].shape, int(tau is not None)],
                   [*DC.pose(c0), 0.0 if tau is None else tau * abs(c1["w_step"])],
                   [(m0[0], np.int16), (m0[1], np.float64), (m1[0], np.int16), (m1[1], np.float64), (DC.consistency_oracle(pname, flt), np.uint8)])
            n += 1
        for name in DC.CLOUDS:
            case, out = DC.cloud_case(name)
            record(f, 3, "cloud " + name, [case["h"], case["w_"], case["channels"], len(out[0])], case["cam"],
                   [(case["keep"], np.uint8), (case["w"], np.float64), (case["score"], np.float32), (case["img"], np.uint8),
                    (out[0], np.float64), (out[1], np.uint8), (out[2], np.float64), (out[3], np.float32)])
            n += 1
    return n


@pytest.fixture(scope="module")
def harness_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dense_host"))
    n = write_records(os.path.join(d, "records.bin"))
    return d, n


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_build_equals_the_restatement_bit_for_bit(harness_dir, sanitize):
    d, n = harness_dir
    exe = toolchain.host_program(d, "dense_host_harness.cpp", sanitize)
    r = subprocess.run([exe, os.path.join(d, "records.bin")], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout[-3000:] + r.stderr[-3000:]
    assert n == len(DC.sweeps()) + len(DC.CONSISTENCY) + len(DC.CLOUDS)
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") == n and "DIFFERENT" not in r.stdout and "MISSING" not in r.stdout


def test_dense_cloud_scratch_is_as_carved(harness_dir):
    exe = toolchain.host_program(harness_dir[0], "dense_host_harness.cpp", False)
    up256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for n in (1, 255, 256, 257, 8192, 8193, 16384 * 16384):
        r = subprocess.run([exe, "--scratch", str(n)], capture_output=True, text=True)
        assert r.returncode == 0 and int(r.stdout) == up256((n + 255) // 256 * 8), (n, r.stdout)


# ---- (c) the host side of the stage ---------------------------------------------------------------------------------------------------------------
def cameras(rot=0.01, tz=0.05):
    K = np.array([[1200.0, 0.0, 400.0], [0.0, 1200.0, 300.0], [0.0, 0.0, 1.0]])
    c, s = np.cos(rot), np.sin(rot)
    R1 = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    return [Camera(800, 600, K=K, R=np.eye(3), t=np.zeros(3)), Camera(800, 600, K=K, R=R1, t=np.array([-1.0, 0.02, tz]))]


@pytest.mark.parametrize("d_min,d_max,step", [(20.0, 60.0, 1.0), (20.0, 60.0, 0.5), (5.0, 500.0, 1.0), (30.0, 30.0, 1.0)])
def test_plane_schedule_moves_no_corner_by_more_than_the_step(d_min, d_max, step):
    c0, c1 = cameras()
    w_first, w_step, n = D.plane_schedule(c0, c1, d_min, d_max, step)
    assert w_first == 1.0 / d_max and 1 <= n <= D.MAX_PLANES
    if d_min == d_max:
        assert (w_step, n) == (0.0, 1)
        return
    assert abs(w_first + (n - 1) * w_step - 1.0 / d_min) <= 1e-15
    R, t = O.relative_pose(c0.R, c0.t, c1.R, c1.t)
    A, B = O.sweep_matrices(c0.K, c1.K, R, t)
    worst = 0.0
    for corner in ((0, 0), (799, 0), (0, 599), (799, 599)):
        p = np.array([(A + (w_first + k * w_step) * B).reshape(3, 3) @ [*corner, 1.0] for k in range(n)])
        xy = p[:, :2] / p[:, 2:]
        worst = max(worst, np.linalg.norm(np.diff(xy, axis=0), axis=1).max())
    assert worst <= step and worst > 0.4 * step                                  # and not needlessly fine


def test_plane_schedule_refuses():
    c0, c1 = cameras()
    for bad in ((0.0, 10.0, 1.0), (10.0, 5.0, 1.0), (10.0, np.inf, 1.0), (5.0, 10.0, 0.0), (np.nan, 10.0, 1.0)):
        with pytest.raises(ValueError):
            D.plane_schedule(c0, c1, *bad)
    with pytest.raises(ValueError, match="more than 4096 planes"):
        D.plane_schedule(c0, c1, 0.5, 1000.0, 0.25)


def test_depth_range_from_points():
    c0, c1 = cameras()
    rng = np.random.default_rng(3)
    X = np.stack([rng.normal(size=1000), rng.normal(size=1000), np.linspace(10.0, 50.0, 1000)], 1)
    X[:5, 2] = -3.0                                                               # behind the camera: ignored
    z = X[5:, 2]
    lo, hi = np.percentile(z, [1, 99])
    assert D.depth_range_from_points(X, c0) == (lo / 1.25, hi * 1.25)
    assert D.depth_range_from_points(X, c0, percentiles=(0, 100), margin=0.0) == (z.min(), z.max())
    z1 = (X @ c1.R.T + np.asarray(c1.t).reshape(3))[:, 2]
    z1 = z1[z1 > 0]
    assert D.depth_range_from_points(X, c1, (5, 95), 0.5) == (np.percentile(z1, 5) / 1.5, np.percentile(z1, 95) * 1.5)
    for bad in (dict(points3d=-X[5:]), dict(points3d=np.zeros((0, 3))), dict(percentiles=(60, 40)), dict(margin=-0.1)):
        with pytest.raises(ValueError):
            D.depth_range_from_points(**{"points3d": X, "cam": c0, **bad})


@pytest.mark.parametrize("f", [1, 2, 3, 4])
def test_grey_and_downscaling_equal_plain_numpy(f):
    rng = np.random.default_rng(f)
    rgb = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    rgb[0, 0], rgb[0, 1] = 255, 0
    g = D.to_grey(rgb)
    i = rgb.astype(np.int64)
    assert g.dtype == np.uint8 and np.array_equal(g, (77 * i[..., 0] + 150 * i[..., 1] + 29 * i[..., 2] + 128) // 256)
    assert g[0, 0] == 255 and g[0, 1] == 0 and D.to_grey(g) is g
    for img in (rgb, g):
        small = D.downscale_image(img, f)
        h, w = 37 // f, 53 // f
        want = np.zeros((h, w) + img.shape[2:], np.int64)
        for dy in range(f):
            for dx in range(f):
                want += img[dy:h * f:f, dx:w * f:f].astype(np.int64)
        assert small.dtype == np.uint8 and np.array_equal(small, (want + f * f // 2) // (f * f))
        assert np.array_equal(small, O.downscale(img, f))
    K = np.array([[1000.0, 0.0, 26.0], [0.0, 1010.0, 18.0], [0.0, 0.0, 1.0]])
    Kf = D.downscale_K(K, f)
    # the centre of small pixel (1, 2) is the mean of the large pixel centres of its block
    big = np.array([f * 1 + (f - 1) / 2.0, f * 2 + (f - 1) / 2.0])
    ray = np.linalg.solve(K, [*big, 1.0])
    assert np.allclose((Kf @ ray)[:2], [1.0, 2.0], atol=1e-12) and np.array_equal(Kf, O.downscale_K(K, f))


REFUSALS = [
    ("an unknown filter", dict(depth_filter="Moderate"), "invalid choise of depth filtering"),
    ("radius 0", dict(radius=0), "radius"),
    ("radius 8", dict(radius=8), "radius"),
    ("a negative min_var", dict(min_var=-1), "min_var"),
    ("downscale 0", dict(downscale=0), "downscale"),
    ("downscale 1.5", dict(downscale=1.5), "downscale"),
    ("view 2", dict(views=(2,)), "views"),
    ("no views", dict(views=()), "views"),
    ("no depth range", dict(depth_range=None), "depth_range"),
    ("an inverted depth range", dict(depth_range=(50.0, 20.0)), "d_min"),
    ("too many planes", dict(depth_range=(0.5, 1000.0), max_step_px=0.25), "planes"),
    ("a float image", dict(images=[np.zeros((600, 800)), np.zeros((600, 800))]), "uint8"),
    ("three images", dict(images=[np.zeros((6, 8), np.uint8)] * 3), "two images"),
]


@pytest.mark.parametrize("what,change,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_python_layer_refuses_before_any_device_work(what, change, text, monkeypatch):
    from icepy4d_amd import engine
    monkeypatch.setattr(engine, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    monkeypatch.setattr(D, "default_engine", lambda e: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    args = dict(images=[np.zeros((600, 800), np.uint8), np.zeros((600, 800), np.uint8)], cameras=cameras(), depth_range=(20.0, 60.0))
    args.update(change)
    with pytest.raises(ValueError, match=text):
        D.build_dense_cloud(**args)


def test_dense_series_takes_bundle_results_as_they_are(monkeypatch, tmp_path):
    from icepy4d_amd.sfm import BundleResult
    calls = []
    monkeypatch.setattr(D, "build_dense_cloud", lambda images, cameras, **kw: calls.append((images, cameras, kw)) or len(calls))
    pairs = [cameras(), cameras(rot=0.02)]
    pts = [np.ones((4, 3)), 2 * np.ones((5, 3))]
    results = [BundleResult(pairs[e], pts[e], "OK", 0.0, 0.0, 1, None, None, None) for e in range(2)]
    out = D.dense_series([["a0", "a1"], ["b0", "b1"]], results, out_dir=tmp_path, dates=["2022_05_01", "2022_05_02"], downscale=2)
    assert out == [1, 2]
    for e, (images, cams, kw) in enumerate(calls):
        assert images == [["a0", "a1"], ["b0", "b1"]][e] and cams is pairs[e] and kw["sparse_points"] is pts[e] and kw["downscale"] == 2
        assert kw["save_path"] == tmp_path / f"dense_2022_05_0{e + 1}.ply"
    calls.clear()
    D.dense_series([["a0", "a1"], ["b0", "b1"]], pairs[0], sparse_points=pts[0])                 # one pair and one cloud for all epochs
    assert [c[1] is pairs[0] and c[2]["sparse_points"] is pts[0] and c[2]["save_path"] is None for c in calls] == [True, True]
    with pytest.raises(ValueError, match="one camera pair or one per epoch"):
        D.dense_series([["a0", "a1"], ["b0", "b1"]], [pairs[0], pairs[1], pairs[0]])
    with pytest.raises(ValueError, match="one entry per epoch"):
        D.dense_series([["a0", "a1"], ["b0", "b1"]], pairs[0], sparse_points=[pts[0]])


def test_filter_names_are_the_references_four():
    assert D.DEPTH_FILTERS == O.FILTERS == {"NoFiltering": None, "MildFiltering": 2.0, "ModerateFiltering": 1.0, "AggressiveFiltering": 0.5}
    for f in (D.filter_tolerance, O.filter_tau):
        with pytest.raises(ValueError, match=r"Error: invalid choise of depth filtering. Choose one in \[NoFiltering, MildFiltering, ModerateFiltering, AggressiveFiltering\]"):
            f("moderate")


def test_abi_is_declared_bound_and_exported():
    from icepy4d_amd import _lib
    with open(os.path.join(ROOT, "include", "icematch.h")) as f:
        header = f.read()
    for n in NAMES:
        m = re.search(r"\nint " + n + r"\(([^;]*)\);", header)
        assert m and n in _lib.SIGNATURES, n
        args = [a for a in m.group(1).split(",") if a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES[n]), (n, len(args), len(_lib.SIGNATURES[n]))
    assert "-83" in header and "metashape.py:198-240" in header
    lib = _lib.load()
    assert (lib.im_dense_tile_w(), lib.im_dense_tile_h()) == (DC.TILE_W, DC.TILE_H)
    assert (D.MAX_SIDE, D.MAX_PLANES, D.MAX_RADIUS) == (O.MAX_SIDE, O.MAX_PLANES, O.MAX_RADIUS) == (16384, 4096, 7)
    with open(os.path.join(toolchain.CSRC, "dense_pixel.h")) as f:
        assert "DENSE_MAX_SIDE = 16384, DENSE_MAX_PLANES = 4096, DENSE_MAX_RADIUS = 7" in f.read()


def test_what_the_dense_stages_share_is_defined_once():
    """The tile, its staging and the scoring of a plane are csrc/dense_tile.h's, the arithmetic csrc/dense_pixel.h's, the host checks
    csrc/dense_host.h's: no kernel file restates them."""
    text = {}
    for name in os.listdir(toolchain.CSRC):
        if name.endswith((".h", ".hip")):
            with open(os.path.join(toolchain.CSRC, name)) as f:
                text[name] = f.read()
    calls = sorted(n for n, s in text.items() if re.search(r"(?<!bool )dense_sample\(", s))
    assert calls == ["dense_tile.h", "refine_pixel.h"], calls                     # the sweep's plane scoring and the slanted window; no .hip file
    assert not any("flow_score" in s for s in text.values())                      # dense_score with the scale 1 of bytes
    parabola = sorted(n for n, s in text.items() if re.search(r"- 2\.0 \* [\w.]*s0\) \+", s))
    assert parabola == ["dense_pixel.h"] and text["dense_pixel.h"].count("(sm - 2.0 * s0) + sp") == 1, parabola
    assert sum(len(re.findall(r"bool bad_side\(", s)) for s in text.values()) == 1 and "bool bad_side(" in text["dense_host.h"]
    for name in ("dense.hip", "dense_sgm.hip", "dense_refine.hip", "dense_flow.hip", "depth_clean.hip"):
        assert '#include "dense_tile.h"' in text[name] and "blockIdx.x * TW" not in text[name] and "= -83" not in text[name], name
    assert text["dense_tile.h"].count("static_assert(TW == 64") == 1 and not any("static_assert(TW == 64" in s for n, s in text.items() if n != "dense_tile.h")
    with open(os.path.join(ROOT, "tests", "dense_host_harness.cpp")) as f:
        assert "dense_tile.h" not in f.read()                                     # kernel text: threadIdx, __shared__, barriers


def test_the_kernels_spill_nothing_and_two_blocks_fit_a_cu(tmp_path):
    """The sweep's block is 256 threads, one wave per SIMD: two blocks on a CU need at most 256 VGPRs per lane (512 per SIMD lane) and
    80 KiB of LDS each (160 KiB per CU). Compiled: 42 576 B of LDS and 136 VGPRs, so three blocks fit by either."""
    res = toolchain.kernel_resources(toolchain.device_listing("dense.hip", str(tmp_path)))
    mine = {k: v for k, v in res.items() if "dense_" in k or "DenseCloudScan" in k}
    assert len(mine) == 2 + 2, sorted(res)                                    # two kernels and the scan's two templates
    for k, f in mine.items():
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (k, dict(f))
    sweep = [f for k, f in mine.items() if "dense_sweep" in k]
    assert len(sweep) == 1
    lds = 30 * 78 * (1 + 4) + 30 * 64 * (8 + 8) + 18 * 8                      # a, b, the two rows of partials, A and B; plus alignment
    assert lds <= sweep[0]["group_segment_fixed_size"] <= lds + 64 and 2 * (lds + 64) <= 160 * 1024
    print("dense_sweep_kernel: vgpr", sweep[0]["vgpr_count"], "sgpr", sweep[0]["sgpr_count"], "lds", lds)
    assert sweep[0]["vgpr_count"] <= 168                                       # 136 as compiled: three waves per SIMD of 512; two blocks need <= 256
    assert sweep[0]["max_flat_workgroup_size"] == 256


def test_module_imports_as_the_first_import():
    r = subprocess.run([sys.executable, "-c", "import icepy4d_amd.dense as d; print(d.MAX_PLANES)"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "4096", r.stderr[-2000:]
