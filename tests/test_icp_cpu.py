"""ICP co-registration and rigid transforms without a device: the arithmetic compiled for the host (csrc/icp_point.h through
tests/icp_host_harness.cpp) against the restatement (tests/icp_oracle.py) on the shared cases (tests/icp_cases.py), the restatement
against independent arithmetic, the whole loop with scipy's cKDTree as the search, the reference's `Rotrotranslation` as recorded in
tests/golden/g21_transformations.npz, the host logic of the Python layers, the declarations and what the compiler made of the kernels.

Bounds, with u = 2^-53 and gamma_k = k u / (1 - k u).
 (1) Host build against the restatement: equality of bits (per-point terms, per-chunk partials, the 30 sums, pivots, x, R, M_next, status,
     fitness, rmse): the same IEEE float64 operations in the same order. A NaN equals a NaN whatever its payload.
 (2) The sums against extended-precision sums of the same products: each product is rounded once, fl(a b) = a b (1 + d), |d| <= u;
     adding m numbers in ANY order (a tree of at most m - 1 additions on the path of each leaf) gives sum x_i (1 + t_i) with
     |t_i| <= gamma_(m-1) (Higham 2002, §4.2); together |S - sum| <= gamma_m sum |a_i b_i|, m the number of rows added. The extended sums'
     own error (2^-64 relative per operation) is below 2^-10 of that.
 (3) The solve by its residual. For Cholesky of a symmetric positive definite n x n system the computed x satisfies (A + dA) x = b with
     |dA| <= gamma_(3n+1) |R^T| |R| (Higham 2002, Theorem 10.4) and || |R^T| |R| ||_2 <= n (1 - n gamma_(n+1))^-1 ||A||_2 (eq. 10.7);
     L D L^T without pivoting is the same factorisation with the diagonal kept apart (R = D^(1/2) L^T), so the residual obeys
     ||A x + b||_2 <= c n u ||A||_2 ||x||_2 with c = 3 n + 1 = 19 for n = 6 (asserted with 1.01 for the denominators).
 (4) The Cayley map. With a = w / 2, s = 1 + a.a, every entry of R is (p + q) / s with |p| + |q| <= 2 s: |1 - a.a| + 2 a_i^2 <= s and
     2 |a_i a_j| + 2 |a_k| <= (a_i^2 + a_j^2) + (1 + a_k^2) <= 2 s. a.a carries gamma_3 (three products, two additions of positive
     terms), 1 -+ a.a, the product, the sum of the entry and the division one rounding each: every computed entry is within
     E = 2 gamma_8 of the exact one. R + dR has (R + dR)^T (R + dR) - I = R^T dR + dR^T R + dR^T dR, so in the Frobenius norm
     <= 2 ||dR||_F + ||dR||_F^2 <= 2 * 3 E + (3 E)^2 < 100 u.
 (5) The end-to-end case: the exact conditions (identity correspondences at every iteration, fitness 1, convergence) and a final
     coordinate error of at most 4 ulp of the largest coordinate. Measured with the restatement: 2 ulp for both methods at the origin;
     2 ulp (point to point) and 3 ulp (point to plane) in the world frame; asserted at the next power of two above 3.
 (6) g21: `transform` against the reference's BLAS product of homogeneous columns: two 4-term dot products in different orders, each
     within gamma_4 sum_j |M_aj| |x_j| of the exact value (the division by the last row, 1.0, is exact): 2 gamma_4 sum_j |M_aj| |x_j| per
     component. `T_inv`: both sides are LU inverses; each is within c_n u kappa_inf(A) ||A^-1||_inf of the exact inverse with
     c_n = 8 n gamma_(3n) / u <= 8 * 4 * 12.1 for partial pivoting of a 4 x 4 with growth factor at most 2^(n-1) = 8 (Higham 2002, §14.3,
     §9.3): twice that between them."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_cases as IC  # noqa: E402
import icp_oracle as O  # noqa: E402
import toolchain  # noqa: E402

NEW_SYMBOLS = ("im_transform_points", "im_icp_accumulate", "im_icp_finish")
U = 2.0 ** -53
GOLDEN = os.path.join(ROOT, "tests", "golden", "g21_transformations.npz")


def gamma(k):
    return k * U / (1.0 - k * U)


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """tests/icp_host_harness.cpp + csrc/icp_point.h as a shared library, behind a stub <hip/hip_runtime.h>."""
    lib = toolchain.host_library(str(tmp_path_factory.mktemp("icp_host")), "icp_host_harness.cpp")
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.icp_host_apply.argtypes = [P, P, P, L, I]
    lib.icp_host_terms.argtypes = [P, L, P, P, L, P, P, P, I, P]
    lib.icp_host_partials.argtypes = [P, L, P, P, L, P, P, P, I, P]
    lib.icp_host_total.argtypes = [P, L, P]
    lib.icp_host_finish.argtypes = [P, P, P, L, I, P]
    lib.icp_host_cayley.argtypes = [P, P]
    lib.icp_host_scratch.argtypes = [L]
    lib.icp_host_scratch.restype = ctypes.c_ulonglong
    for f in (lib.icp_host_apply, lib.icp_host_terms, lib.icp_host_partials, lib.icp_host_total, lib.icp_host_finish, lib.icp_host_cayley):
        f.restype = None
    return lib


def same(a, b):
    """Equality of bits, a NaN equal to a NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def _args(case):
    return [np.ascontiguousarray(case[k]) for k in ("source", "target", "normals", "idx", "d2", "centre")]


# ---- (1) the host build of icp_point.h ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", IC.METHODS)
@pytest.mark.parametrize("name", IC.names(big=True))
def test_host_build_equals_the_restatement_bit_for_bit(host_lib, name, method):
    case = IC.by_name(name)
    src, tgt, nrm, idx, d2, c = _args(case)
    n, nt, chunks = len(src), len(tgt), O.n_chunks(len(src))
    want_parts, want_S, want_rec, want_eval = IC.expected(name, method)
    head = (src.ctypes.data, n, tgt.ctypes.data, nrm.ctypes.data, nt, idx.ctypes.data, d2.ctypes.data, c.ctypes.data, method)
    if name != "big":                                                   # the rows of every point: what it alone adds to sums of +0.0
        terms = np.full((n, O.TERMS), -7.0)
        host_lib.icp_host_terms(*head, terms.ctypes.data)
        row_list, ok = O.rows(src, tgt, nrm, idx, c, method)
        want = np.zeros((n, O.TERMS))
        for T in O.terms(row_list, ok, d2) if n else []:
            want = want + T
        assert same(terms, want), name
        assert (terms[~ok] == 0.0).all() and not np.signbit(terms[~ok]).any()                     # an unusable point: rows of +0.0
    parts = np.full((chunks, O.TERMS), -7.0)
    host_lib.icp_host_partials(*head, parts.ctypes.data)
    assert same(parts, want_parts), name
    S = np.full(O.TERMS, -7.0)
    host_lib.icp_host_total(parts.ctypes.data, chunks, S.ctypes.data)
    assert same(S, want_S) and not np.signbit(S[S == 0.0]).any(), name
    M = np.ascontiguousarray(case["M"])
    for solve, want in ((1, want_rec), (0, want_eval)):
        rec = np.full(O.RECORD, -7.0)
        host_lib.icp_host_finish(S.ctypes.data, M.ctypes.data, c.ctypes.data, n, solve, rec.ctypes.data)
        assert same(rec, want), (name, solve, rec, want)
    if want_rec[O.REC_STATUS] != O.OK:
        assert same(want_rec[:16], M.reshape(16))                          # the transform stays as it was
    assert same(want_eval[:16], M.reshape(16)) and (want_eval[O.REC_X:O.REC_SUMS] == 0.0).all()


def test_host_apply_and_cayley_equal_the_restatement(host_lib):
    rng = np.random.default_rng(1)
    M = np.ascontiguousarray(IC.motion(7.0, (0.3, 0.2, -0.9), (4.0e5, 5.0e6, 2.0e3)))
    pts = rng.normal(0, 50.0, (300, 3))
    pts[3], pts[4], pts[5, 1] = np.nan, np.inf, -np.inf
    for as_vectors in (0, 1):
        out = np.full_like(pts, -7.0)
        host_lib.icp_host_apply(M.ctypes.data, pts.ctypes.data, out.ctypes.data, len(pts), as_vectors)
        assert same(out, O.apply(M, pts, bool(as_vectors)))
    inplace = pts.copy()
    host_lib.icp_host_apply(M.ctypes.data, inplace.ctypes.data, inplace.ctypes.data, len(pts), 0)
    assert same(inplace, O.apply(M, pts))
    for w in list(rng.normal(0, 0.05, (20, 3))) + [np.zeros(3), np.array([2.0, 0.0, 0.0]), np.array([1e-170, 3.0, -1e200])]:
        w = np.ascontiguousarray(w)
        R = np.full(9, -7.0)
        host_lib.icp_host_cayley(w.ctypes.data, R.ctypes.data)
        assert same(R.reshape(3, 3), O.cayley(w)), w


def test_the_cases_are_what_they_claim():
    e = IC.expected
    assert O.ICP_CHUNK == 1024 and IC.BIG == 256 * 1024 + 1 and len(e("big", 1)[0]) == 257
    for m in IC.METHODS:
        assert e("n0", m)[2][O.REC_STATUS] == O.EMPTY == e("all_minus", m)[2][O.REC_STATUS]
        assert e("n0", m)[2][O.REC_FITNESS] == 0.0 and e("n0", m)[2][O.REC_RMSE] == 0.0
        assert e("n5", m)[2][O.REC_STATUS] == O.DEGENERATE == e("five_usable", m)[2][O.REC_STATUS] and e("five_usable", m)[1][O.I_COUNT] == 5.0
        assert e("n1025", m)[2][O.REC_STATUS] == O.OK == e("world", m)[2][O.REC_STATUS]
        assert same(e("flipped", m)[2], e("n1025", m)[2])                  # n -> -n leaves every bit
        assert 0.0 < e("partial_overlap", m)[2][O.REC_FITNESS] <= 0.75
    assert not same(IC.by_name("flipped")["normals"], IC.by_name("n1025")["normals"])
    planar = e("planar", O.POINT_TO_PLANE)
    A_diag = planar[1][[0, 6, 11, 15, 18, 20]]
    assert (A_diag[[2, 3, 4]] == 0.0).all() and (A_diag[[0, 1, 5]] > 0.0).all() and planar[2][O.REC_STATUS] == O.DEGENERATE
    ok, bad = e("near_singular_ok", 1), e("near_singular_degenerate", 1)
    assert ok[2][O.REC_STATUS] == O.OK and bad[2][O.REC_STATUS] == O.DEGENERATE
    ratio_ok = ok[2][O.REC_PIVOT + 5] / ok[1][20]
    ratio_bad = bad[2][O.REC_PIVOT + 5] / bad[1][20]
    assert O.PIVOT < ratio_ok < 1e-6 and ratio_bad < O.PIVOT               # the rule, exercised on both sides
    assert e("nan_normals", 1)[1][O.I_COUNT] < e("nan_normals", 0)[1][O.I_COUNT] == 900.0
    assert e("nonfinite_source", 0)[1][O.I_COUNT] == 696.0 and np.isfinite(e("nonfinite_source", 0)[1]).all()
    assert e("scattered_minus", 0)[1][O.I_COUNT] < 1500 - 1500 // 7
    assert IC.by_name("world")["target"][:, 1].min() >= 4.9e6 and np.abs(IC.by_name("far_centre")["centre"]).min() >= 1e5


# ---- (2) the restatement against independent arithmetic ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", IC.METHODS)
@pytest.mark.parametrize("name", ["n257", "n2049", "world", "far_centre", "scattered_minus", "moved_M"])
def test_sums_against_extended_precision(name, method):
    case = IC.by_name(name)
    row_list, ok = O.rows(case["source"], case["target"], case["normals"], case["idx"], case["centre"], method)
    J = np.concatenate([j for j, _ in row_list]).astype(np.longdouble)
    r = np.concatenate([rr for _, rr in row_list]).astype(np.longdouble)
    m = len(r)
    S = IC.expected(name, method)[1]
    JtJ, Jtr = J.T @ J, J.T @ r                                          # extended precision: numpy has no BLAS for it
    worst = 0.0
    for k, (a, b) in enumerate(O.UPPER):
        bound = gamma(m) * float(np.sum(np.abs(J[:, a] * J[:, b])))
        err = abs(float(np.longdouble(S[k]) - JtJ[a, b]))
        assert err <= bound, (name, a, b, err, bound)
        worst = max(worst, err / bound if bound else 0.0)
    for a in range(6):
        bound = gamma(m) * float(np.sum(np.abs(J[:, a] * r)))
        assert abs(float(np.longdouble(S[O.I_B + a]) - Jtr[a])) <= bound, (name, a)
    assert abs(float(np.longdouble(S[O.I_RR]) - r @ r)) <= gamma(m) * float(r @ r)
    d2 = np.where(ok, case["d2"], 0.0).astype(np.longdouble)
    assert abs(float(np.longdouble(S[O.I_D2]) - d2.sum())) <= gamma(len(d2)) * float(d2.sum())
    assert S[O.I_COUNT] == ok.sum()
    print(f"{name} method {method}: worst |S - J^T J| = {worst:.4f} of its bound over {m} rows")


@pytest.mark.parametrize("method", IC.METHODS)
@pytest.mark.parametrize("name", ["n6", "n257", "n2049", "world", "moved_M", "near_singular_ok"])
def test_solve_by_its_residual(name, method):
    _, S, rec, _ = IC.expected(name, method)
    if rec[O.REC_STATUS] != O.OK:
        pytest.fail(f"{name} must be a well-posed system")
    A = np.zeros((6, 6), np.longdouble)
    for k, (a, b) in enumerate(O.UPPER):
        A[a, b] = A[b, a] = S[k]
    x, b = rec[O.REC_X:O.REC_X + 6].astype(np.longdouble), S[O.I_B:O.I_B + 6].astype(np.longdouble)
    res = float(np.sqrt(((A @ x + b) ** 2).sum()))
    bound = 1.01 * 19 * 6 * U * float(np.linalg.norm(A.astype(np.float64), 2)) * float(np.sqrt((x * x).sum()))
    print(f"{name} method {method}: residual {res:.3e}, bound {bound:.3e}")
    assert res <= bound


def test_cayley_map_is_orthogonal_within_its_bound():
    rng = np.random.default_rng(2)
    worst = 0.0
    for w in list(rng.normal(0, 0.02, (200, 3))) + list(rng.normal(0, 2.0, (200, 3))) + [np.zeros(3)]:
        R = O.cayley(w).astype(np.longdouble)
        dev = float(np.sqrt(((R.T @ R - np.eye(3)) ** 2).sum()))
        worst = max(worst, dev)
        assert dev <= 100 * U, (w, dev)
    assert same(O.cayley(np.zeros(3)), np.eye(3))
    small = np.array([1e-3, -2e-3, 5e-4])                                # second-order agreement with the exponential map
    K = np.array([[0, -small[2], small[1]], [small[2], 0, -small[0]], [-small[1], small[0], 0]])
    t = np.linalg.norm(small)
    expm = np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / t ** 2 * (K @ K)
    assert np.abs(O.cayley(small) - expm).max() <= t ** 3
    print(f"worst ||R^T R - I||_F = {worst / U:.2f} u")


# ---- (3) end to end on the CPU, scipy's cKDTree as the search ------------------------------------------------------------------------------------
def kdtree_search(p, target, radius2):
    from scipy.spatial import cKDTree
    idx, d2o = np.full(len(p), -1, np.int32), np.full(len(p), np.inf)
    fin = np.isfinite(p).all(1)
    if len(target) == 0 or not fin.any():
        return idx, d2o
    j = cKDTree(target).query(p[fin], k=1)[1]
    d = p[fin] - target[j]
    d2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])                       # the kernel's own d2 of the pair found
    keep = ~(d2 > radius2)
    sel = np.nonzero(fin)[0][keep]
    idx[sel], d2o[sel] = j[keep], d2[keep]
    return idx, d2o


@pytest.mark.parametrize("world", [False, True])
@pytest.mark.parametrize("method", IC.METHODS)
def test_end_to_end_recovers_the_motion(world, method):
    src, tgt, nrm, _ = IC.end_to_end(world)
    M, records, corr, converged = O.icp(src, tgt, nrm, IC.D_MAX, method=method, search=kdtree_search)
    identity = np.arange(len(src))
    assert all(np.array_equal(idx, identity) for idx, _ in corr)          # identity correspondences at every iteration
    assert (records[:, O.REC_FITNESS] == 1.0).all() and (records[:, O.REC_STATUS] == O.OK).all()
    assert converged and len(records) - 1 <= 30
    err = np.abs(O.apply(M, src) - tgt).max()
    ulp = np.spacing(np.abs(tgt).max())
    print(f"world {world} method {method}: {len(records) - 1} iterations, rmse {records[:, O.REC_RMSE]}, final error {err:.3e} = {err / ulp:.1f} ulp")
    assert err <= 4 * ulp
    M2, records2, _, _ = IC.end_to_end_expected(world, method)             # the brute-force search finds the same pairs: the same bits
    assert same(M, M2) and same(records, records2)
    assert records[0, O.REC_RMSE] > 5e-2 and records[-1, O.REC_RMSE] < 1e-8


def test_a_source_equal_to_the_target_stays():
    tgt, nrm = IC.surface(12)
    for method in IC.METHODS:
        init = IC.motion(0.0, shift=(0.0, 0.0, 0.0))
        M, records, _, converged = O.icp(tgt, tgt, nrm, IC.D_MAX, init=init, method=method)
        assert same(M, init) and converged and records[-1, O.REC_RMSE] == 0.0 and records[-1, O.REC_FITNESS] == 1.0
        assert (records[0, O.REC_X:O.REC_X + 6] == 0.0).all()             # b = 0: the step is exactly zero
        for s, t, n in ((np.zeros((0, 3)), tgt, nrm), (tgt, np.zeros((0, 3)), np.zeros((0, 3)))):        # nothing to register, nothing to register to
            M, records, corr, converged = O.icp(s, t, n, IC.D_MAX, method=method)
            assert same(M, np.eye(4)) and len(records) == 1 and records[0, O.REC_STATUS] == O.EMPTY and not converged
            assert records[0, O.REC_FITNESS] == 0.0 and (corr[0][0] == -1).all()


# ---- (4) the reference's Rotrotranslation as recorded ------------------------------------------------------------------------------------------
def test_host_algebra_against_the_recorded_reference(tmp_path):
    from icepy4d_amd.utils import transformations as T
    g = np.load(GOLDEN)
    for frame in ("local", "world"):
        rt = T.Rotrotranslation(np.array(g[f"T_{frame}"]))
        A = rt.T
        assert same(A, g[f"T_{frame}"])
        Ainv = np.linalg.inv(A)
        kappa = np.abs(A).sum(1).max() * np.abs(Ainv).sum(1).max()
        bound = 2 * 8 * 4 * gamma(12) * kappa * np.abs(Ainv).sum(1).max()
        assert np.abs(rt.T_inv - g[f"T_inv_{frame}"]).max() <= bound
        for pn in ("local", "world"):
            x = g[f"pts_{pn}"]
            for M, want, src in ((A, g[f"fwd_{frame}_{pn}"], x), (g[f"T_inv_{frame}"], g[f"inv_{frame}_{pn}"], g[f"fwd_{frame}_{pn}"])):
                got = O.apply(rt._matrix(M), src)
                bound = 2 * gamma(4) * (np.abs(src) @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3])[None, :])
                assert (np.abs(got - want) <= bound).all(), (frame, pn, np.abs(got - want).max(), bound.min())
    for key in ("last_row", "rotation"):
        assert int(g[f"refused_{key}"].reshape(-1)[0]) == 1
        with pytest.raises(ValueError):
            T.Rotrotranslation(np.array(g[f"bad_{key}"]))
    with pytest.raises(AssertionError):
        T.Rotrotranslation(np.eye(3))
    path = tmp_path / "T.txt"
    T.Rotrotranslation(np.array(g["T_local"])).write_T_mat_to_csv(str(path))
    assert path.read_bytes() == g["file_text"].tobytes()
    assert same(T.Rotrotranslation.read_T_from_file(path).T, g["file_T"])
    (tmp_path / "bad.txt").write_text("1 2 3\n4 5 6\n")
    with pytest.raises(ValueError):
        T.Rotrotranslation.read_T_from_file(tmp_path / "bad.txt")
    with pytest.raises(ValueError):
        T.Rotrotranslation.read_T_from_file(tmp_path / "absent.txt")
    h = T.convert_to_homogeneous(np.arange(6.0).reshape(3, 2))
    assert h.shape == (4, 2) and (h[3] == 1.0).all() and same(T.convert_from_homogeneous(h * 2.0), np.arange(6.0).reshape(3, 2))
    assert T.convert_to_homogeneous(np.zeros((4, 2))) is None and T.convert_from_homogeneous(np.zeros((2, 2))) is None
    assert not hasattr(T.Rotrotranslation, "belvedere_loc2utm")


# ---- (5) host-side checks ------------------------------------------------------------------------------------------------------------------------
def test_python_layers_refuse_before_any_device_work(tmp_path):
    from icepy4d_amd import change_detection as C
    from icepy4d_amd.core.point_cloud import PointCloud
    from icepy4d_amd.post_processing import registration as R
    from icepy4d_amd.utils import transformations as T
    pts, nrm = np.zeros((5, 3)), np.tile([0.0, 0.0, 1.0], (5, 1))
    good = dict(target_normals=nrm)
    for bad in (np.zeros((5, 2)), np.zeros(5), np.zeros((5, 4))):
        with pytest.raises(ValueError, match="source"):
            R.registration_icp(bad, pts, 1.0, **good)
        with pytest.raises(ValueError, match="target"):
            R.registration_icp(pts, bad, 1.0, **good)
        with pytest.raises(ValueError, match="source"):
            R.evaluate_registration(bad, pts, 1.0)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            R.registration_icp(pts, pts, bad, **good)
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            R.evaluate_registration(pts, pts, bad)
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            C.coregister_series([pts, pts], bad, normal_radius=1.0)
    bad_row, bad_nan = np.eye(4), np.eye(4)
    bad_row[3, 0], bad_nan[0, 3] = 1e-9, np.nan
    for bad in (bad_row, bad_nan, np.eye(3), np.zeros((4, 5))):
        with pytest.raises(ValueError, match="init"):
            R.registration_icp(pts, pts, 1.0, init=bad, **good)
        with pytest.raises(ValueError, match="init"):
            R.evaluate_registration(pts, pts, 1.0, transformation=bad)
        with pytest.raises(ValueError, match="transformation"):
            PointCloud(points3d=pts).transform(bad)
    with pytest.raises(ValueError, match="estimation_method"):
        R.registration_icp(pts, pts, 1.0, estimation_method="kabsch", **good)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="max_iteration"):
            R.registration_icp(pts, pts, 1.0, criteria=R.ICPConvergenceCriteria(max_iteration=bad), **good)
    with pytest.raises(ValueError, match="normal_radius"):
        R.registration_icp(pts, pts, 1.0)                                 # point to plane with neither normals nor a radius
    with pytest.raises(ValueError, match="normal_radius"):
        R.registration_icp(pts, pts, 1.0, normal_radius=-1.0)
    with pytest.raises(ValueError, match="target_normals"):
        R.registration_icp(pts, pts, 1.0, target_normals=nrm[:4])
    for bad in ((0.0, np.nan, 0.0), (0.0, 0.0)):
        with pytest.raises(ValueError, match="centre"):
            R.registration_icp(pts, pts, 1.0, centre=bad, **good)
    with pytest.raises(ValueError, match="reference"):
        C.coregister_series([pts, pts], 1.0, reference=2, normal_radius=1.0)
    with pytest.raises(ValueError, match="target_normals"):
        C.coregister_series([pts, pts], 1.0, target_normals=nrm)
    with pytest.raises(ValueError, match="stable"):
        C.coregister_series([pts, pts], 1.0, stable=np.zeros((2, 2)), normal_radius=1.0)
    rt = T.Rotrotranslation(np.eye(4))
    for bad in (np.zeros((5, 4)), np.zeros((5, 2))):
        with pytest.raises(ValueError, match="n, 3"):
            rt.transform(bad)
        with pytest.raises(ValueError, match="n, 3"):
            rt.transform_inverse(bad)
    with pytest.raises(ValueError, match="points"):
        T.transform_points(np.eye(4), np.zeros((3, 2)))
    assert R.ICPConvergenceCriteria() == (1e-6, 1e-6, 30)
    assert R.RegistrationResult._fields == ("transformation", "fitness", "inlier_rmse", "correspondence_set", "iterations", "converged", "status",
                                            "history")
    assert (R.REC_M, R.REC_FITNESS, R.REC_RMSE, R.REC_COUNT, R.REC_STATUS, R.REC_X, R.REC_PIVOT, R.REC_SUMS, R.RECORD) == \
        (O.REC_M, O.REC_FITNESS, O.REC_RMSE, O.REC_COUNT, O.REC_STATUS, O.REC_X, O.REC_PIVOT, O.REC_SUMS, O.RECORD)
    assert "KABSCH" in R.__doc__ and "Cayley" in R.__doc__ and "inlier_rmse" in C.m3c2_series.__doc__


def test_coregistration_table_equals_plain_numpy(tmp_path):
    from icepy4d_amd import change_detection as C
    from icepy4d_amd.post_processing.registration import RegistrationResult
    M = IC.motion(0.6, (0.3, -0.5, 0.8), (0.04, -0.03, 0.05))
    r = RegistrationResult(M, 0.75, 0.0123, np.zeros((0, 2), np.int64), 4, True, "OK", np.zeros((5, 64)))
    table = C.coregistration_table([None, r, r._replace(converged=False, iterations=30)], reference=0, names=["e0", "e1", "e2"],
                                   out_path=tmp_path / "o" / "reg.csv")
    assert list(table.columns) == C.REGISTRATION_COLUMNS and len(table) == 3
    assert table.iloc[0].tolist() == ["e0", "e0", 0, True, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    row = table.iloc[1]
    assert (row["epoch"], row["reference"], row["iterations"], row["converged"], row["fitness"], row["inlier_rmse"]) == ("e1", "e0", 4, True, 0.75, 0.0123)
    assert (row["tx"], row["ty"], row["tz"]) == (M[0, 3], M[1, 3], M[2, 3]) and abs(row["angle_deg"] - 0.6) < 1e-9
    assert not table.iloc[2]["converged"] and table.iloc[2]["iterations"] == 30
    assert C.coregistration_table([None, r], reference="previous").iloc[1]["reference"] == "0"
    assert (tmp_path / "o" / "reg.csv").read_text().splitlines()[0] == ",".join(C.REGISTRATION_COLUMNS)
    assert C.rotation_angle_deg(np.eye(4)) == 0.0 and abs(C.rotation_angle_deg(IC.motion(179.0)) - 179.0) < 1e-9
    with pytest.raises(ValueError, match="names"):
        C.coregistration_table([None, r], names=["a"])


def test_the_new_symbols_are_declared_and_bound(host_lib):
    from icepy4d_amd import _lib
    header = open(os.path.join(ROOT, "include", "icematch.h")).read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and name in _lib.SIGNATURES, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), (name, len(m.group(1).split(",")), len(_lib.SIGNATURES[name]))
    assert re.search(r"\bint im_icp_chunk\(void\);", header) and _lib.SIGNATURES["im_icp_chunk"] == []
    assert "-81" in header
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW_SYMBOLS)
    assert lib.im_icp_chunk() == O.ICP_CHUNK == host_lib.icp_host_chunk() == 1024


def test_the_scratch_carve_is_pinned(host_lib):
    # one piece: 32 doubles per chunk (at least one chunk), rounded up to 256 bytes
    for chunks, want in ((0, 256), (1, 256), (2, 512), (3, 768), (257, 257 * 256), (65536, 65536 * 256)):
        assert host_lib.icp_host_scratch(chunks) == want == -(-max(chunks, 1) * O.TERMS * 8 // 256) * 256, chunks


@pytest.mark.parametrize("module", ["icepy4d_amd.post_processing.registration", "icepy4d_amd.utils.transformations"])
def test_new_modules_import_first_in_a_fresh_interpreter(module):
    r = subprocess.run([sys.executable, "-c", f"import {module} as m; print(m.__name__)"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == module, r.stderr[-2000:]


def test_the_icp_kernels_keep_their_sums_in_registers(tmp_path):
    res = toolchain.kernel_resources(toolchain.device_listing("icp.hip", str(tmp_path)))
    for kernel, lds in (("transform_points_kernel", 0), ("icp_accumulate_kernel", 4 * 32 * 8), ("icp_finish_kernel", 5 * 32 * 8)):
        r = res[next(k for k in res if kernel in k)]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, kernel   # no spills, no scratch memory
        assert r["group_segment_fixed_size"] == lds, kernel
