"""The geometry kernels after the matcher, against the fp64 restatement in tests/geometry_oracle.py: fundamental / essential
RANSAC hypothesis by hypothesis and in batches (`im_ransac_fundamental`, `im_ransac_essential`), linear triangulation
(`im_triangulate_linear`), the tile merge (`im_merge_tile_matches`) and the row gather (`im_gather_rows`)."""
import numpy as np
import pytest
import torch

import geometry_oracle as go

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def dev(a, e):
    return torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


def ransac(e, p0, p1, n_hyp, threshold, seed, essential=False):
    """One launch pair; returns (F [3, 3], mask [n] uint8, info [2]). The outputs start as sentinels, so an unwritten one shows."""
    from icepy4d_amd._lib import ptr
    n = len(p0)
    d0, d1 = dev(np.asarray(p0, np.float32), e), dev(np.asarray(p1, np.float32), e)
    dF = torch.full((9,), float("nan"), dtype=torch.float64, device=e.device)
    dmask = torch.full((n,), 7, dtype=torch.uint8, device=e.device)
    dinfo = torch.full((2,), -5, dtype=torch.int32, device=e.device)
    e.ctx.call("im_ransac_essential" if essential else "im_ransac_fundamental", ptr(d0), ptr(d1), n, int(n_hyp), float(threshold),
               int(seed) & 0xFFFFFFFF, ptr(dF), ptr(dmask), ptr(dinfo), e.stream_ptr())
    return dF.cpu().numpy().reshape(3, 3), dmask.cpu().numpy(), dinfo.cpu().numpy()


def two_view(seed, n, noise=0.5, outliers=0.0, f=800.0, normalised=False):
    """A pixel-scale two-view scene (640 x 480, focal f) with Gaussian noise in image 1 and a fraction of gross outliers, as float32;
    `normalised` returns K^-1 coordinates instead (the essential path)."""
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(4, 8, n)]
    K = np.array([[f, 0, 320], [0, f, 240], [0, 0, 1.0]])
    a = 0.1
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    p0 = (K @ X.T).T
    p1 = (K @ (X @ R.T + np.array([0.5, 0.05, 0.1])).T).T
    p0, p1 = p0[:, :2] / p0[:, 2:], p1[:, :2] / p1[:, 2:] + rng.normal(0, noise, (n, 2))
    m = int(round(outliers * n))
    p1[:m] += rng.uniform(20, 60, (m, 2)) * rng.choice([-1, 1], (m, 2))
    if normalised:
        p0, p1 = (p0 - K[[0, 1], [2, 2]]) / f, (p1 - K[[0, 1], [2, 2]]) / f
    return p0.astype(np.float32), p1.astype(np.float32)


WELL_POSED = 1e-8      # sigma8 / sigma1 of the normalised sample above which the device must find the 8-point solution


def check_result(F, mask, info, p0, p1, threshold, Fo, kappa, where):
    """A valid winner: F equals the oracle's up to sign within its conditioning bound; the mask is the Sampson test of the device's own
    F point by point (the kernel's arithmetic), and the oracle's decision wherever the point is not ambiguous; info[0] is the mask's
    count."""
    ok, d = go.f_close(F, Fo, kappa, k=8.0)
    assert ok, (where, d, kappa)
    thr2 = float(threshold) ** 2
    r_dev = go.sampson_ratio(F, p0, p1, thr2)
    r_orc = go.sampson_ratio(Fo, p0, p1, thr2)
    m = mask.astype(bool)
    assert set(np.unique(mask).tolist()) <= {0, 1}, where
    sure = np.abs(r_dev - 1) > 1e-8
    assert np.array_equal(m[sure], (r_dev < 1)[sure]), (where, np.nonzero(m[sure] != (r_dev < 1)[sure])[0][:10])
    amb = (np.abs(r_orc - 1) <= 1e-6) | ((r_orc < 1) != (r_dev < 1))
    assert amb.sum() <= max(2, len(p0) // 200), (where, int(amb.sum()))
    assert np.array_equal(m[~amb], (r_orc < 1)[~amb]), where
    assert info[0] == int(m.sum()), (where, info)


def check_empty(F, mask, info, where, hyp=0):
    """No valid hypothesis (or none with an inlier): count 0, F = 0 and an all-false mask."""
    assert info[0] == 0 and info[1] == hyp, (where, info)
    assert np.array_equal(F, np.zeros((3, 3))), (where, F)
    assert not mask.any(), (where, int(mask.sum()))


# ------------------------------------------------------------------------------------------------ one hypothesis per launch
HYP_CASES = {
    # name: (points, threshold, essential, seeds)
    "px_noise_20pct": (lambda: two_view(1, 300, 0.5, 0.2), 1.0, False, 200),
    "px_noise_50pct": (lambda: two_view(2, 300, 0.5, 0.5), 1.0, False, 200),
    "px_f4000": (lambda: two_view(3, 400, 0.5, 0.2, f=4000.0), 0.7, False, 100),
    "norm_fundamental": (lambda: two_view(4, 300, 0.3, 0.2, normalised=True), 1e-4, False, 100),
    "norm_essential": (lambda: two_view(4, 300, 0.3, 0.2, normalised=True), 1e-4, True, 200),
    "n8": (lambda: two_view(5, 8, 0.5, 0.0), 1.0, False, 64),
    "n9": (lambda: two_view(6, 9, 0.5, 0.2), 1.0, False, 64),
    "n13": (lambda: two_view(7, 13, 0.5, 0.2), 1.0, False, 64),
    "n8_essential": (lambda: two_view(8, 8, 0.3, 0.0, normalised=True), 1e-4, True, 64),
    "n13_essential": (lambda: two_view(9, 13, 0.3, 0.1, normalised=True), 2e-3, True, 64),
}


def _with_duplicates(p):
    """40 points of which 15 repeat earlier ones: a mix of exactly degenerate and well-posed samples."""
    p0, p1 = p
    src = np.random.default_rng(10).integers(0, 25, 15)
    p0[25:], p1[25:] = p0[src], p1[src]
    return p0, p1


HYP_CASES["duplicates"] = (lambda: _with_duplicates(two_view(11, 40, 0.5, 0.1)), 1.0, False, 200)
HYP_CASES["duplicates_essential"] = (lambda: _with_duplicates(two_view(12, 40, 0.3, 0.1, normalised=True)), 1e-3, True, 200)


@pytest.mark.parametrize("case", list(HYP_CASES))
def test_ransac_single_hypothesis_equals_oracle(eng, case):
    """n_hyp = 1 exposes hypothesis (seed, 0) alone: its sample, 8-point F (rank 2, projected onto the essential manifold on the essential
    path), its Sampson count and mask must be the oracle's; a sample holding a duplicated correspondence gives count 0, F = 0 and no
    inlier, and so does a valid hypothesis without a single inlier."""
    make, thr, essential, seeds = HYP_CASES[case]
    p0, p1 = make()
    checked = degenerate = empty = 0
    for seed in range(seeds):
        F, mask, info = ransac(eng, p0, p1, 1, thr, seed, essential)
        hy = go.hypotheses(p0, p1, seed, [0], thr, essential)
        where = (case, seed, hy["idx"][0].tolist())
        if hy["dup"][0] or not hy["valid"][0]:
            check_empty(F, mask, info, where)
            degenerate += 1
        elif hy["cond"][0] > WELL_POSED and hy["count"][0] + hy["amb"][0] == 0:
            check_empty(F, mask, info, where)                  # a valid F without a single inlier is no better than none
            empty += 1
        elif hy["cond"][0] > WELL_POSED and hy["count"][0] > 0:
            assert info[1] == 0, where
            check_result(F, mask, info, p0, p1, thr, hy["F"][0], hy["kappa"][0], where)
            assert hy["count"][0] <= info[0] <= hy["count"][0] + hy["amb"][0], (where, info, hy["count"][0], hy["amb"][0])
            if essential:
                s = np.linalg.svd(F)[1]
                assert abs(s[0] - s[1]) < 1e-12 and s[2] < 1e-12, (where, s)
            checked += 1
    assert checked >= seeds // 5, (checked, degenerate, empty)
    if case.startswith("duplicates"):
        assert degenerate >= 10 and checked >= 10, (checked, degenerate)


# ------------------------------------------------------------------------------------------------ batches: selection
@pytest.mark.parametrize("n_hyp,n", [(1, 2000), (63, 2000), (64, 2000), (65, 2000), (1024, 2000), (1025, 2000), (4097, 2000),
                                     (65, 100000)])
def test_ransac_batch_selects_the_oracle_winner(eng, n_hyp, n):
    """The winner of n_hyp hypotheses is the oracle's arg-max of the inlier counts (ties: the lowest index), across the select kernel's
    1024 stride and partial blocks, and its mask across the n / 1024 stride; F is the winner's oracle matrix, info[0] the mask's count."""
    thr = 1.0
    p0, p1 = two_view(20 + n_hyp, n, 0.5, 0.3)
    seed = 1000 + n_hyp
    F, mask, info = ransac(eng, p0, p1, n_hyp, thr, seed)
    hy = go.hypotheses(p0, p1, seed, np.arange(n_hyp), thr)
    unsure = ~hy["valid"] | (hy["cond"] <= WELL_POSED)
    lo = np.where(unsure, 0, hy["count"])
    hi = hy["count"] + hy["amb"]
    h = int(info[1])
    assert 0 <= h < n_hyp, info
    assert lo[h] <= info[0] <= hi[h], (h, info, lo[h], hi[h])
    assert (lo[:h] < info[0]).all(), "an earlier hypothesis has at least as many inliers"
    assert (lo[h + 1:] <= info[0]).all(), "a later hypothesis has more inliers"
    if (lo == hi).all():
        assert (int(info[0]), h) == go.select(hy["count"])
    assert not unsure[h]
    check_result(F, mask, info, p0, p1, thr, hy["F"][h], hy["kappa"][h], (n_hyp, n, h))


@pytest.mark.parametrize("n_hyp", [64, 1025])
@pytest.mark.parametrize("essential", [False, True])
def test_ransac_ties_go_to_the_first_valid_hypothesis(eng, n_hyp, essential):
    """Noise-free, outlier-free data: every valid hypothesis counts every point, so the winner must be the first valid index. With
    heavy duplication the leading hypotheses are degenerate and the first valid one lies further in."""
    thr = 1e-4 if essential else 1.0
    for dupl in (False, True):
        p0, p1 = two_view(30, 200, 0.0, 0.0, normalised=essential)
        if dupl:
            src = np.random.default_rng(31).integers(0, 12, 188)
            p0[12:], p1[12:] = p0[src], p1[src]
        seed = 77
        F, mask, info = ransac(eng, p0, p1, n_hyp, thr, seed, essential)
        hy = go.hypotheses(p0, p1, seed, np.arange(n_hyp), thr, essential)
        ok = hy["valid"] & (hy["cond"] > WELL_POSED)
        assert ok.any() and (hy["count"][ok] == len(p0)).all() and (hy["amb"] == 0).all()
        first = int(np.argmax(hy["valid"]))
        assert ok[first]
        if dupl:
            assert first > 0, "the case must start with degenerate hypotheses"
        assert info[1] == first and info[0] == len(p0), (dupl, info, first)
        check_result(F, mask, info, p0, p1, thr, hy["F"][first], hy["kappa"][first], (essential, dupl))


# ------------------------------------------------------------------------------------------------ no valid hypothesis
def _all_degenerate_inputs():
    rng = np.random.default_rng(40)
    same0 = np.tile(np.float32([[100.5, 200.25]]), (50, 1))
    same1 = np.tile(np.float32([[300.75, 50.5]]), (50, 1))
    q0, q1 = two_view(41, 8, 0.5, 0.0)
    q0[3], q1[3] = q0[5], q1[5]
    t = rng.permutation(400)[:60].astype(np.float32)
    u = rng.permutation(400)[:60].astype(np.float32)
    diag0 = np.c_[t, t]                                   # exactly on y = x: equal columns in the 8 x 9 system
    const1 = np.c_[u, np.full(60, 7.0, np.float32)]      # exactly on y = 7: zero columns
    diag1 = np.c_[u, u]
    return {"identical": (same0, same1), "n8_duplicate": (q0, q1), "y_eq_x_and_y_const": (diag0, const1),
            "y_eq_x_both": (diag0, diag1)}


@pytest.mark.parametrize("essential", [False, True])
@pytest.mark.parametrize("case", list(_all_degenerate_inputs()))
def test_ransac_without_a_valid_hypothesis_returns_an_empty_result(eng, case, essential):
    """Every 8-point sample degenerate: the launch reports count 0, F = 0 and an all-false mask (it used to report every point an
    inlier of F = 0, whose Sampson test 0 < thr^2 * 1e-24 holds everywhere)."""
    p0, p1 = _all_degenerate_inputs()[case]
    hy = go.hypotheses(p0, p1, 5, np.arange(64), 1.0, essential)
    assert (hy["dup"] | (hy["cond"] < 1e-14)).all()
    for n_hyp in (1, 65, 1025):
        F, mask, info = ransac(eng, p0, p1, n_hyp, 1.0, 5, essential)
        check_empty(F, mask, info, (case, essential, n_hyp))


def test_geometric_verification_fails_like_the_reference_without_a_valid_hypothesis(eng):
    """Host level: `geometric_verification` on all-degenerate input takes the reference's failure path, (None, all matches kept), and
    `estimate_pose` still raises that it cannot estimate an essential matrix."""
    from icepy4d_amd import sfm
    from icepy4d_amd.matching import GeometricVerification, geometric_verification
    for case, (p0, p1) in _all_degenerate_inputs().items():
        F, mask = geometric_verification(p0, p1, GeometricVerification.PYDEGENSAC, threshold=1.0, engine=eng)
        assert F is None and mask.dtype == bool and mask.all() and len(mask) == len(p0), case
        # K = I keeps the normalised coordinates exactly degenerate (a principal point would move y = x onto a line float32 rounds)
        with pytest.raises(AssertionError, match="Unable to estimate Essential matrix"):
            sfm.estimate_pose(p0, p1, np.eye(3), np.eye(3), 1.0, 0.9999, engine=eng)


# ------------------------------------------------------------------------------------------------ triangulation
def _cameras(f, baseline, yaw=0.05):
    K = np.array([[f, 0, 3000.0], [0, f, 2000.0], [0, 0, 1]])
    R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    t = np.array([-baseline, 0.02 * baseline, 0.01 * baseline])
    return K @ np.eye(3, 4), K @ np.c_[R, t], R, t


def _project(P, X):
    x = (P @ np.c_[X, np.ones(len(X))].T).T
    return x / x[:, 2:]


def _triangulate(e, P0, P1, x0, x1):
    from icepy4d_amd import sfm
    return sfm.triangulate_points_linear(P0, P1, x0, x1, engine=e)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("f", [1000.0, 8000.0])
@pytest.mark.parametrize("ratio", [1.0, 10.0, 100.0, 1000.0])
def test_triangulation_equals_oracle(eng, n, f, ratio):
    """Pixel-scale cameras (6000 x 4000 images), depth-to-baseline ratios 1 to 1e3: every point within its conditioning bound of the
    oracle on 0.5 px noise, and within max(1e-9, its bound) of the true point on exact correspondences (the bounds hold the oracle
    itself with a margin of ~30 on these cases)."""
    rng = np.random.default_rng(int(f) + n + int(ratio))
    b = 1.0
    P0, P1, _, _ = _cameras(f, b)
    depth = ratio * b * rng.uniform(0.8, 1.25, n)
    half = 0.4 * 6000 / f                                   # keeps the points inside the first image
    X = np.c_[rng.uniform(-half, half, n) * depth, rng.uniform(-half, half, n) * depth * 2 / 3, depth]
    x0, x1 = _project(P0, X), _project(P1, X)
    Xd = _triangulate(eng, P0, P1, x0, x1)
    Xo, bound = go.triangulate(P0, P1, x0, x1)
    scale = np.abs(X).max(1)
    err_true = np.abs(Xd[:, :3] - X).max(1) / scale
    assert (err_true <= np.maximum(1e-9, 8 * bound)).all(), (err_true.max(), bound[np.argmax(err_true)])
    noisy0 = x0 + np.c_[rng.normal(0, 0.5, (n, 2)), np.zeros(n)]
    noisy1 = x1 + np.c_[rng.normal(0, 0.5, (n, 2)), np.zeros(n)]
    Xd = _triangulate(eng, P0, P1, noisy0, noisy1)
    Xo, bound = go.triangulate(P0, P1, noisy0, noisy1)
    assert (Xd[:, 3] == 1.0).all()
    err = np.abs(Xd - Xo).max(1) / np.abs(Xo).max(1)
    assert (err <= 8 * bound).all(), (err.max(), bound[np.argmax(err / bound)], (err / bound).max())


def test_triangulation_near_the_epipole(eng):
    """Forward motion (camera 1 one unit ahead along the optical axis, 1 degree of yaw) puts both epipoles inside the 6000 x 4000 images;
    points within 0.01 - 0.1 degrees of the baseline image within 20 px of them. Their two rays are nearly parallel, so the system is
    badly conditioned: the median bound is above 1e-9, where the cases of `test_triangulation_equals_oracle` at depth-to-baseline
    ratios 1 and 10 stay below 1e-10, and the device must still stay within it, of the oracle and of the true point."""
    rng = np.random.default_rng(50)
    n, f = 257, 8000.0
    K = np.array([[f, 0, 3000.0], [0, f, 2000.0], [0, 0, 1]])
    a = np.deg2rad(1.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    c1 = np.array([0.06, -0.03, 1.0])                      # camera centre 1 (camera 0 at the origin)
    P0, P1 = K @ np.eye(3, 4), K @ np.c_[R, -R @ c1]
    e0, e1 = _project(P0, c1[None])[0, :2], _project(P1, np.zeros((1, 3)))[0, :2]
    assert (np.abs(e0 - [3000, 2000]) < [3000, 2000]).all() and (np.abs(e1 - [3000, 2000]) < [3000, 2000]).all()
    d = c1 / np.linalg.norm(c1)
    u = rng.normal(size=(n, 3))
    u -= (u @ d)[:, None] * d
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    th = np.deg2rad(rng.uniform(0.01, 0.1, n))
    X = rng.uniform(5, 60, n)[:, None] * (np.cos(th)[:, None] * d + np.sin(th)[:, None] * u)
    x0, x1 = _project(P0, X), _project(P1, X)
    assert np.linalg.norm(x0[:, :2] - e0, axis=1).max() < 20 and np.linalg.norm(x1[:, :2] - e1, axis=1).max() < 20
    Xd = _triangulate(eng, P0, P1, x0, x1)
    Xo, bound = go.triangulate(P0, P1, x0, x1)
    assert np.median(bound) > 1e-9
    err = np.abs(Xd - Xo).max(1) / np.abs(Xo).max(1)
    assert (err <= 8 * bound).all(), (err.max(), (err / bound).max())
    err_true = np.abs(Xd[:, :3] - X).max(1) / np.abs(X).max(1)
    assert (err_true <= 8 * bound).all(), (err_true.max(), (err_true / bound).max())
    # 0.2 px of noise in image 0: the rays no longer meet, the device still solves the oracle's least-squares problem
    x0[:, :2] += rng.normal(0, 0.2, (n, 2))
    Xd = _triangulate(eng, P0, P1, x0, x1)
    Xo, bound = go.triangulate(P0, P1, x0, x1)
    err = np.abs(Xd - Xo).max(1) / np.abs(Xo).max(1)
    assert (err <= 8 * bound).all(), (err.max(), (err / bound).max())


def test_triangulation_of_zero_points_launches_nothing(eng):
    """n = 0 returns 0 and writes nothing, also with the null pointers of empty tensors (the host path returns a [0, 4] array)."""
    from icepy4d_amd._lib import ptr
    P0, P1, _, _ = _cameras(1000.0, 1.0)
    x = torch.zeros((1, 3), dtype=torch.float64, device=eng.device)
    dX = torch.full((1, 4), 3.5, dtype=torch.float64, device=eng.device)
    p0, p1 = np.ascontiguousarray(P0.reshape(12)), np.ascontiguousarray(P1.reshape(12))
    rc = eng.ctx.lib.im_triangulate_linear(eng.ctx.h, p0.ctypes.data, p1.ctypes.data, ptr(x), ptr(x), 0, ptr(dX), eng.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and (dX.cpu().numpy() == 3.5).all()
    assert _triangulate(eng, P0, P1, np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 4)


# ------------------------------------------------------------------------------------------------ tile merge, row gather
def _merge_case(seed, P, K, density):
    """Synthetic banks for P tile pairs: x drawn from a small pool of float32 values with arbitrary fractions (many equal x with
    different y), large tile offsets and image origins (the two orders of the additions round differently); half of tile 1 repeats
    tile 0 shifted by 512 at an offset 512 further (overlapping tiles landing on the same image points); the last pair shares the bank
    slot and offset of the first (exact duplicates); partly filled banks whose stale match entries past the count are >= 0."""
    rng = np.random.default_rng(seed)
    T0 = max(2, P // 3 + 1)
    T = T0 + max(1, P // 3 + 1)
    pool = (rng.integers(0, 40, 64) * 8 + rng.random(64)).astype(np.float32)
    kp = np.stack([rng.choice(pool, (T, K)), (rng.integers(0, 4000, (T, K)) * 0.37)], -1).astype(np.float32)
    h = K // 2
    kp[0, :h] = 512 + rng.integers(0, 1280, (h, 2)) * 0.25          # quarter steps: the shifted copies are exact
    kp[1, :h] = kp[0, :h] - np.float32(512)
    nb = np.where(rng.random(T) < 0.5, K, rng.integers(1, K + 1, T)).astype(np.int32)
    nb[:2] = np.maximum(nb[:2], h)
    slots = np.stack([rng.integers(0, T0, P), rng.integers(T0, T, P)], 1).astype(np.int32)
    off = (2048 + rng.random((P, 4)) * 1500).astype(np.float32)        # + 512 stays in [2048, 4096): exact
    slots[0, 0] = 0
    if P >= 2:
        slots[1, 0] = 1
    off[slots[:, 0] == 1, 0:2] = off[0, 0:2] + np.float32(512)
    if P >= 3:
        slots[-1, 0], off[-1, 0:2] = slots[0, 0], off[0, 0:2]
    matches = np.where(rng.random((P, K)) < density, rng.integers(0, K, (P, K)), -1).astype(np.int32)
    org = np.float32([31234.567, 20111.3, 17.77, 40000.9])
    return matches, slots, off, org, kp, nb


def _merge_on_device(e, matches, slots, off, org, kp, nb):
    from icepy4d_amd._lib import ptr
    P, K = matches.shape
    cap = P * K
    count = torch.full((1,), -1, dtype=torch.int32, device=e.device)
    idx0 = torch.full((cap,), -9, dtype=torch.int32, device=e.device)
    idx1 = torch.full((cap,), -9, dtype=torch.int32, device=e.device)
    kp0 = torch.full((cap, 2), -9.0, device=e.device)
    kp1 = torch.full((cap, 2), -9.0, device=e.device)
    dM, dS, dO, dK, dN = (dev(a, e) for a in (matches, slots, off, kp, nb))
    e.ctx.call("im_merge_tile_matches", P, K, ptr(dM), ptr(dS), ptr(dO), np.ascontiguousarray(org).ctypes.data, ptr(dK), ptr(dN),
               ptr(count), ptr(idx0), ptr(idx1), ptr(kp0), ptr(kp1), e.stream_ptr())
    S = int(count.item())
    return S, idx0.cpu().numpy(), idx1.cpu().numpy(), kp0.cpu().numpy(), kp1.cpu().numpy()


# (P, K, density): from a few matched rows to more than 3 x 1024, several blocks of the first / rank kernels. Run in this order on one
# context, five calls grow the scratch (capacity P * K above every earlier one) and three reuse it (4000 after 4000, 8192 after 16000,
# 131072 after 131072)
MERGE_CASES = [(1, 64, 0.1), (1, 1000, 0.5), (4, 1000, 0.3), (4, 1000, 0.9), (16, 1000, 0.25), (1, 8192, 0.45), (4, 8192, 0.12),
               (16, 8192, 0.03), (16, 8192, 0.1)]


def test_tile_merge_equals_the_header_contract():
    """count, idx0, idx1, kp0, kp1 exactly as the contract states them (tests/geometry_oracle.py merge_tile_matches), on one context
    whose scratch grows on some calls and is reused on others."""
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    try:
        sizes = []
        for seed, (P, K, density) in enumerate(MERGE_CASES):
            case = _merge_case(seed, P, K, density)
            matches, slots, off, org, kp, nb = case
            mk0, _, _, _ = go.merge_rows(*case)
            o0, o1, ok0, ok1 = go.merge_tile_matches(*case)
            S, i0, i1, k0, k1 = _merge_on_device(e, *case)
            where = (P, K, density, len(mk0), len(o0))
            assert S == len(o0), where
            assert np.array_equal(i0[:S], o0) and np.array_equal(i1[:S], o1), where
            assert np.array_equal(k0[:S].view(np.int32), ok0.view(np.int32)), where
            assert np.array_equal(k1[:S].view(np.int32), ok1.view(np.int32)), where
            assert (i0[S:] == -9).all() and (i1[S:] == -9).all(), where
            # the case can tell the reference's order of the two additions from the other one
            t0 = slots[:, 0]
            alt = kp[t0][..., 0] + (off[:, 0] + org[0])[:, None]
            ref = (kp[t0][..., 0] + off[:, 0][:, None]) + org[0]
            assert (alt != ref).any(), where
            sizes.append((len(mk0), len(o0)))
        assert max(r for r, _ in sizes) > 3 * 1024 and min(r for r, _ in sizes) < 16
        assert any(u < r for r, u in sizes[2:]), sizes                         # duplicates were removed
    finally:
        e.close()


@pytest.mark.parametrize("row_floats", [1, 2, 3, 4, 5, 8, 12, 64, 255, 256, 257, 1024])
def test_gather_rows_is_numpy_fancy_indexing(eng, row_floats):
    """dst[r] = src[idx[r]] bit for bit, over both the 16-byte and the scalar path; rows past n stay untouched."""
    from icepy4d_amd._lib import ptr
    rng = np.random.default_rng(row_floats)
    R = 300
    src = rng.normal(size=(R, row_floats)).astype(np.float32)
    src.view(np.int32)[:, 0] ^= rng.integers(0, 1 << 20, R).astype(np.int32)        # arbitrary low mantissa bits
    dsrc = dev(src, eng)
    for n in (1, 63, 64, 65, 1000):
        for kind in ("random", "reversed", "repeated"):
            if kind == "random":
                idx = rng.integers(0, R, n)
            elif kind == "reversed":
                idx = (R - 1 - np.arange(n)) % R
            else:
                idx = np.repeat(rng.integers(0, R, (n + 7) // 8), 8)[:n]
            idx = idx.astype(np.int32)
            dst = torch.full((n + 3, row_floats), float("nan"), device=eng.device)
            dst.view(torch.int32).fill_(0x7F00DEAD)
            didx = dev(idx, eng)
            eng.ctx.call("im_gather_rows", ptr(dsrc), row_floats, ptr(didx), n, ptr(dst), eng.stream_ptr())
            out = dst.cpu().numpy().view(np.int32)
            assert np.array_equal(out[:n], src[idx].view(np.int32)), (row_floats, n, kind)
            assert (out[n:] == 0x7F00DEAD).all(), (row_floats, n, kind)
