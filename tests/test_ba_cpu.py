"""Two-view bundle adjustment without a device: the arithmetic compiled for the host (csrc/ba_point.h through tests/ba_host_harness.cpp)
against the restatement (tests/ba_oracle.py) on the shared cases (tests/ba_cases.py), the restatement against independent arithmetic, the
whole loop against the truth of a synthetic scene and against scipy, the host logic of the Python layers, the two CSV writers, the
declarations and what the compiler made of the kernels.

Bounds, with u = 2^-53 and gamma_k = k u / (1 - k u).
 (1) Host build against the restatement: equality of bits (per-point factors, chunk partials, the 448 sums, pivots, steps, candidate
     cameras and points, cost partials, decisions, records, the whole loop): the same IEEE float64 operations in the same order. A NaN
     equals a NaN whatever its payload.
 (2) The analytic Jacobians against central differences of the restated projection in extended precision (numpy longdouble, 64-bit
     significand, u_x = 2^-64) with a step h per parameter: the difference quotient carries a truncation error h^2 |f'''| / 6 and a
     rounding error 2 u_x |f| / (2 h) (the restated residual is O(10) operations, so a few u_x |f|). With residuals |f| <= 2.4e4 (12000 px
     over sigma 0.5) and h = 2^-20 of the parameter's scale the rounding part is below 2.4e4 * 2^-64 * 2^20 * 8 = 1.1e-8 absolute; the third
     derivative can only be measured. Both are small against the entries of J (1e0 .. 1e5), so the check is relative to the largest entry
     of a column: |J - J_fd|_max / |J|_max per column. Measured with the restatement over all 14 + 3 columns of both cameras: 3.61e-11;
     asserted at the next power of two above, 2^-34 = 5.8e-11. (The analytic J itself is float64: its own rounding, a few u, is far below.)
 (3) The reduced solve by its residual: ||A x + b||_2 <= c n u ||A||_2 ||x||_2 with c = 3 n + 1 = 85 for n = 28, as derived in
     tests/test_icp_cpu.py (Higham 2002, Theorem 10.4 and eq. 10.7), asserted with 1.01 for the denominators.
 (4) The Schur elimination against the dense (28 + 3 N)-dimensional normal equations, N = 16, assembled from the restated rows and solved
     by Gaussian elimination with partial pivoting in extended precision, damped as the definition damps (the points' blocks by
     lambda diag(V), then the diagonal of the reduced system by lambda times itself). Both solve the same system H d = -g; the float64 route
     forms H with relative error gamma_m per entry (m <= 2 N + 2 products per sum) and solves by LDL^T, which is backward stable and
     invariant under a diagonal scaling of the unknowns (van der Sluis), so both are judged in the scaling s = sqrt(diag H) that makes
     the diagonal 1: ||s (d - d_dense)||_2 <= 4 n kappa_2(S^-1 H S^-1) u ||s d_dense||_2 with n = 28 + 3 N. The scaled condition numbers
     are 4.6e3 (default mask), 5.6e4 (all free) and 6.4e3 (default mask, a 5 cm prior on every point), so the bound is 1.5e-10 to 2e-8
     relative and a damping or prior error of that size fails it; measured 1.7e-14, 1.8e-13, 2.7e-14 relative.
 (5) End to end without noise (restatement, world frame): status OK through ctol = 2^-56 (a cost at rounding level: residuals of 12000 px
     / sigma carry about 20 u each, squared and summed over 4 * 300 rows: 1200 * (20 * 2^-53 * 2.4e4)^2 / 2 = 1.7e-18 = 2^-59, so
     ctol = 2^-56 leaves a factor 8), final cost below it, and the recovered f, rotations, centres and control points against the truth.
     Measured with the restatement: 7 iterations, cost 1.8e-21, |df| 2.73e-12 px, rotation entries 4.44e-16, worst residual 9.1e-12 px,
     asserted at the next power of two above each (2^-38, 2^-51, 2^-36); the centres and the control points came back to the very bits
     of the truth (measured 0), which cannot be asserted tighter than one spacing of the largest coordinate, 2^-30 m at 5e6 m.
 (6) End to end with 0.5 px noise against scipy.optimize.least_squares (method "trf", x_scale "jac", tolerances 1e-15) on the same cost
     from the same start: both are local minimisers of one function. Near a minimum the cost is flat to second order, so two minimisers
     that stopped within a relative step of 1e-6 agree in cost to 1e-12 relative; measured gap |cost - cost_scipy| / cost = 2.6e-11
     (ours the lower: 95.35017711670 against 95.35017711917), so scipy's own stopping rule, relative to its scaled variables, decides the
     gap, not ours. Asserted: ours is not above scipy's by more than 1e-10 relative (4 x the measured gap on the side that would show a
     defect of ours), and the two agree within 1e-9 (40 x, the side scipy's rule decides). The parameters (f, centres, rotations of both
     cameras) agree within 1e-3 of their a-posteriori standard deviation, which follows from the cost gap (derived at the assertion);
     measured 6.6e-5."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ba_cases as BC  # noqa: E402
import ba_oracle as O  # noqa: E402
import toolchain  # noqa: E402

NEW_SYMBOLS = ("im_ba_accumulate", "im_ba_solve", "im_ba_step_points", "im_ba_decide", "im_ba_residuals")
U = 2.0 ** -53
LD = np.longdouble


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """tests/ba_host_harness.cpp + csrc/ba_point.h as a shared library, behind a stub <hip/hip_runtime.h>."""
    lib = toolchain.host_library(str(tmp_path_factory.mktemp("ba_host")), "ba_host_harness.cpp")
    P, L, D, UI = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_double, ctypes.c_uint
    lib.ba_host_project.argtypes = [P, P, P]
    lib.ba_host_factors.argtypes = [P, P, P, P, P, L, D, P]
    lib.ba_host_partials.argtypes = [P, L, P]
    lib.ba_host_total.argtypes = [P, L, P]
    lib.ba_host_solve.argtypes = [P, P, P, D, UI, P, P]
    lib.ba_host_step_points.argtypes = [P, P, P, P, P, P, P, L, P, P, P]
    lib.ba_host_centre_cost.argtypes, lib.ba_host_centre_cost.restype = [P, P], D
    lib.ba_host_decide.argtypes = [P, D, P, P, P]
    lib.ba_host_residuals.argtypes = [P, P, P, L, P]
    lib.ba_host_run.argtypes = [P, P, P, P, P, L, P, UI, P, P, P, L]
    lib.ba_host_scratch.argtypes, lib.ba_host_scratch.restype = [L, L], ctypes.c_ulonglong
    lib.ba_host_default_mask.restype = UI
    for f in (lib.ba_host_project, lib.ba_host_factors, lib.ba_host_partials, lib.ba_host_total, lib.ba_host_solve, lib.ba_host_step_points,
              lib.ba_host_decide, lib.ba_host_residuals, lib.ba_host_run):
        f.restype = None
    return lib


def same(a, b):
    """Equality of bits, a NaN equal to a NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def _arrays(c):
    return [np.ascontiguousarray(c[k], np.float64) for k in ("cams", "X", "obs", "sig", "prior", "cprior")]


def host_run(lib, c, max_iter=30, extra=None):
    """ba_host_run on a case (or on `extra` = (X, obs, sig, prior) in its place): cams, X, state, history"""
    cams, X, obs, sig, prior, cprior = _arrays(c)
    if extra is not None:
        X, obs, sig, prior = (np.ascontiguousarray(v, np.float64) for v in extra)
    n = len(X)
    cams, Xw = cams.copy(), (X.copy() if n else np.zeros((1, 3)))
    opts = np.array(c["opts"])
    opts[3] = max_iter
    st, hist = O.initial_state(c["lam"]), np.zeros((max_iter, O.RECORD))
    lib.ba_host_run(cams.ctypes.data, Xw.ctypes.data, obs.ctypes.data, sig.ctypes.data, prior.ctypes.data, n, cprior.ctypes.data, int(c["mask"]),
                    opts.ctypes.data, st.ctypes.data, hist.ctypes.data, max_iter)
    return cams, Xw[:n], st, hist[:int(st[O.ST_ITER])]


# ---- (1) the host build of ba_point.h ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.names())
def test_host_build_equals_the_restatement_bit_for_bit(host_lib, name):
    c, w = BC.by_name(name), BC.first_iteration(name)
    cams, X, obs, sig, prior, cprior = _arrays(c)
    n, chunks = len(X), O.n_chunks(len(X))
    fac = np.full((max(n, 1), O.FAC), -7.0)
    host_lib.ba_host_factors(cams.ctypes.data, X.ctypes.data, obs.ctypes.data, sig.ctypes.data, prior.ctypes.data, n, c["lam"], fac.ctypes.data)
    assert same(fac[:n], w["fac"]), name
    bad = w["fac"][:, O.F_OK] == 0.0
    assert (fac[:n][bad] == 0.0).all() and not np.signbit(fac[:n][bad]).any()                      # an unusable point: +0.0 everywhere
    parts = np.full((max(chunks, 1), O.TERMS), -7.0)
    host_lib.ba_host_partials(fac.ctypes.data, n, parts.ctypes.data)
    assert same(parts[:chunks], w["parts"]), name
    S = np.full(O.TERMS, -7.0)
    host_lib.ba_host_total(parts.ctypes.data, chunks, S.ctypes.data)
    assert same(S, w["sums"]) and not np.signbit(S[S == 0.0]).any() and (S[O.SUMS:] == 0.0).all(), name
    draft, cand = np.full(O.RECORD, -7.0), np.full(O.EPOCH, -7.0)
    host_lib.ba_host_solve(S.ctypes.data, cams.ctypes.data, cprior.ctypes.data, c["lam"], int(c["mask"]), draft.ctypes.data, cand.ctypes.data)
    assert same(draft, w["draft"]) and same(cand, w["cand"]), (name, "pivots, steps, candidate cameras")
    out, terms, cparts = np.full((max(n, 1), 3), -7.0), np.full(max(n, 1), -7.0), np.full(max(chunks, 1), -7.0)
    host_lib.ba_host_step_points(fac.ctypes.data, draft[O.REC_X:].ctypes.data, X.ctypes.data, cand.ctypes.data, obs.ctypes.data, sig.ctypes.data,
                                 prior.ctypes.data, n, out.ctypes.data, terms.ctypes.data, cparts.ctypes.data)
    assert same(out[:n], w["cand_pts"]) and same(cparts[:chunks], w["cparts"]), (name, "candidate points")
    assert same(out[:n][bad], X[bad])                                                            # an unusable point does not move
    cost1 = O.total(w["cparts"][:, None])[0] + host_lib.ba_host_centre_cost(cand.ctypes.data, cprior.ctypes.data)
    st, rec = O.initial_state(c["lam"]), np.full(O.RECORD, -7.0)
    host_lib.ba_host_decide(draft.ctypes.data, cost1, np.ascontiguousarray(c["opts"]).ctypes.data, st.ctypes.data, rec.ctypes.data)
    assert same(rec, w["rec"]) and same(st, w["state"]), (name, "decision")
    res = np.full((max(n, 1), 2, 3), -7.0)
    host_lib.ba_host_residuals(cams.ctypes.data, X.ctypes.data, obs.ctypes.data, n, res.ctypes.data)
    assert same(res[:n], O.residuals(cams, X, obs)), name
    got, want = host_run(host_lib, c), BC.whole_run(name)
    assert all(same(a, b) for a, b in zip(got, want)), (name, "the whole loop")


def test_the_cases_are_what_they_claim(host_lib):
    f, run = BC.first_iteration, BC.whole_run
    assert O.BA_CHUNK == 256 == host_lib.ba_host_chunk() and O.BA_TILE == 32 == host_lib.ba_host_tile() and host_lib.ba_host_fac() == O.FAC
    assert host_lib.ba_host_default_mask() == O.MASK_DEFAULT and len(f("n513")["parts"]) == 3
    assert run("n0")[2][O.ST_STATUS] == O.EMPTY and len(run("n0")[3]) == 1
    assert run("singular")[2][O.ST_STATUS] == O.DEGENERATE and len(run("singular")[3]) == 1
    assert same(run("singular")[0], BC.by_name("singular")["cams"]) and same(run("singular")[1], BC.by_name("singular")["X"])    # the state stays
    acc = run("accept_reject")[3][:, O.REC_ACCEPTED]
    assert (acc[:8] == 1.0).any() and (acc[:8] == 0.0).any() and run("accept_reject")[2][O.ST_STATUS] == O.OK
    assert run("noisy", 3)[2][O.ST_STATUS] == O.MAX_ITER and run("noisy")[2][O.ST_STATUS] == O.OK
    h, c = run("ctol")[3], BC.by_name("ctol")                            # ended by ctol, not by ftol: the last step still halves the cost and more
    assert run("ctol")[2][O.ST_STATUS] == O.OK and 0.0 < h[-1, O.REC_COST1] <= c["opts"][4] and h[-1, O.REC_COST0] - h[-1, O.REC_COST1] > 0.5 * h[-1, O.REC_COST0]
    zero = np.array(c["opts"])
    zero[4] = 0.0
    assert O.run(c["cams"], c["X"], c["obs"], c["sig"], c["prior"], c["cprior"], c["mask"], zero, O.initial_state(c["lam"]))[2][O.ST_STATUS] != O.OK
    h, c = run("stalled")[3], BC.by_name("stalled")                      # the first rejected step takes lambda past its ceiling
    assert run("stalled")[2][O.ST_STATUS] == O.STALLED and h[-1, O.REC_ACCEPTED] == 0.0 and h[:-1, O.REC_ACCEPTED].all() and h[-1, O.REC_LAMBDA] * 10.0 > c["opts"][1]
    assert f("absent")["sums"][O.I_COUNT] == 97.0 and f("absent")["fac"][[5, 6, 7], O.F_OK].sum() == 0.0 and f("absent")["fac"][[96, 97], O.F_OK].sum() == 2.0
    assert f("nonfinite")["sums"][O.I_COUNT] == 90.0 and np.isfinite(f("nonfinite")["sums"]).all()
    assert f("behind")["fac"][8, O.F_OK] == 0.0 and f("behind")["fac"][9, O.F_OK] == 0.0 and f("behind")["sums"][O.I_COUNT] == 98.0
    x = f("mask_fixed")["draft"][O.REC_X:O.REC_X + O.DIM]
    assert (x == 0.0).all() and same(f("mask_fixed")["cand"], BC.by_name("mask_fixed")["cams"])
    x = f("mask_odd")["draft"][O.REC_X:O.REC_X + O.DIM]
    assert (x[1::2] == 0.0).all() and (x[0::2] != 0.0).all() and (f("mask_all")["draft"][O.REC_X:O.REC_X + O.DIM] != 0.0).all()
    assert np.abs(BC.by_name("world")["X"]).max() > 4.9e6 and run("world")[3][-1, O.REC_COST1] < 1e-9
    part = BC.by_name("partial_priors")["prior"]
    assert (part[10, 3:] > 0).sum() == 1 and (part[11, 3:] > 0).sum() == 2 and (part[66, 3:] > 0).sum() == 2
    assert [len(BC.by_name(n)["X"]) for n in BC.TABLE] == [0, 65, O.BA_CHUNK + 1]


# ---- (2) the analytic Jacobians ---------------------------------------------------------------------------------------------------------------
def _residual_ld(cam, X, uo, vo, i_s):
    p = O.project(cam, X)
    return np.stack([(p["u"] - uo) * i_s, (p["v"] - vo) * i_s], 1)


def _stepped_ld(cam, k, h):
    """The camera with parameter k of 14 stepped by h, in extended precision (O.step_camera's text without its float64 copy)."""
    x = np.zeros(O.CAM, LD)
    x[k] = h
    out = np.array(cam, LD)
    Q = O.cayley(x[:3])
    for a in range(3):
        for j in range(3):
            out[3 * a + j] = ((Q[3 * a] * cam[j]) + (Q[3 * a + 1] * cam[3 + j])) + (Q[3 * a + 2] * cam[6 + j])
    out[9:12] = cam[9:12] + x[3:6]
    out[12], out[13], out[14], out[15] = cam[12] + x[6], cam[13] + x[6], cam[14] + x[7], cam[15] + x[8]
    out[16:21] = cam[16:21] + x[9:14]
    return out


def test_analytic_jacobians_against_extended_central_differences():
    c = BC.by_name("n257")
    X, obs, i_s = np.array(c["X"]), np.array(c["obs"]), 1.0 / np.array(c["sig"])
    scale = [1.0] * 3 + [1.0] * 3 + [1000.0, 1000.0, 1000.0] + [1e-2] * 5                         # the size of a parameter's natural step
    worst = 0.0
    for cam_id in range(2):
        cam = np.array(c["cams"][24 * cam_id:24 * cam_id + 24])
        J, Jp, _ = O.rows(cam, O.project(cam, X), obs[:, 2 * cam_id], obs[:, 2 * cam_id + 1], i_s)
        cam_x, X_x, uo, vo, is_x = cam.astype(LD), X.astype(LD), obs[:, 2 * cam_id].astype(LD), obs[:, 2 * cam_id + 1].astype(LD), i_s.astype(LD)
        for k in range(O.CAM):
            h = LD(scale[k]) * LD(2.0) ** -20
            fd = (_residual_ld(_stepped_ld(cam_x, k, h), X_x, uo, vo, is_x) - _residual_ld(_stepped_ld(cam_x, k, -h), X_x, uo, vo, is_x)) / (2 * h)
            err = float(np.abs(J[:, :, k] - fd).max() / np.abs(J[:, :, k]).max())
            worst = max(worst, err)
            assert err <= 2.0 ** -34, (cam_id, k, err)
        for k in range(3):
            h = LD(2.0) ** -20
            d = np.zeros(3, LD)
            d[k] = h
            fd = (_residual_ld(cam_x, X_x + d, uo, vo, is_x) - _residual_ld(cam_x, X_x - d, uo, vo, is_x)) / (2 * h)
            err = float(np.abs(Jp[:, :, k] - fd).max() / np.abs(Jp[:, :, k]).max())
            worst = max(worst, err)
            assert err <= 2.0 ** -34, (cam_id, "X", k, err)
    print(f"worst relative deviation of a Jacobian column from its central difference: {worst:.3e}")


def test_projection_inverts_the_undistortion_model(host_lib):
    """Without distortion and with R = I the projection is the pinhole's; with it, the radial factor is the reciprocal of undistort_one's."""
    cam = O.camera_state(np.eye(3), [0.0, 0.0, 0.0], np.array([[1000.0, 0, 500.0], [0, 1100.0, 400.0], [0, 0, 1.0]]))
    X = np.array([[1.0, -2.0, 10.0]])
    p = O.project(cam, X)
    assert p["u"][0] == 1000.0 * 0.1 + 500.0 and p["v"][0] == 1100.0 * -0.2 + 400.0
    cam[16:24] = [-0.05, 0.02, 0.0, 0.0, 0.01, 1e-3, -5e-4, 2e-4]
    p = O.project(cam, X)
    r2 = 0.1 * 0.1 + 0.2 * 0.2
    icdist = (1.0 + ((2e-4 * r2 - 5e-4) * r2 + 1e-3) * r2) / (1.0 + ((0.01 * r2 + 0.02) * r2 - 0.05) * r2)
    assert abs(p["radial"][0] * icdist - 1.0) <= 4 * U
    out = np.zeros(3)
    host_lib.ba_host_project(cam.ctypes.data, X.ctypes.data, out.ctypes.data)
    assert same(out, [p["u"][0], p["v"][0], 10.0])


# ---- (3) the reduced solve -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n65", "n257", "world", "mask_all", "mask_odd", "partial_priors", "noisy"])
def test_reduced_solve_by_its_residual(name):
    c, w = BC.by_name(name), BC.first_iteration(name)
    A, b = O.reduced(w["sums"], c["cams"], c["cprior"], c["lam"], c["mask"])
    x, d, ok = O.solve(A, b)
    assert ok and (d > 0).all()
    res = float(np.sqrt((((A.astype(LD) @ x.astype(LD)) + b.astype(LD)) ** 2).sum()))
    bound = 1.01 * 85 * 28 * U * float(np.linalg.norm(A, 2)) * float(np.linalg.norm(x))
    print(f"{name}: residual {res:.3e}, bound {bound:.3e}")
    assert res <= bound


# ---- (4) the Schur elimination against the dense system -------------------------------------------------------------------------------------
def _solve_ld(H, g):
    """Gaussian elimination with partial pivoting in extended precision: H d = g"""
    H, g = H.copy(), g.copy()
    n = len(g)
    for k in range(n):
        piv = k + int(np.argmax(np.abs(H[k:, k])))
        H[[k, piv]], g[[k, piv]] = H[[piv, k]], g[[piv, k]]
        for i in range(k + 1, n):
            m = H[i, k] / H[k, k]
            H[i, k:] -= m * H[k, k:]
            g[i] -= m * g[k]
    d = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        d[i] = (g[i] - H[i, i + 1:] @ d[i + 1:]) / H[i, i]
    return d


@pytest.mark.parametrize("mask,all_priors", [(O.MASK_DEFAULT, False), (O.MASK_ALL, False), (O.MASK_DEFAULT, True)])
def test_schur_elimination_equals_the_dense_normal_equations(mask, all_priors):
    N, lam = 16, 1e-3
    c = BC.scene(N, seed=77, noise=0.3)
    cams, X, obs, sig, prior, cprior = _arrays(c)
    if all_priors:                                                      # every point a control point of 5 cm: a well-conditioned system, a bound that bites
        prior = np.concatenate([c["X_true"], np.full((N, 3), 0.05)], 1)
    dim = O.DIM + 3 * N
    rows_J, rows_r = [], []
    for cam_id in range(2):
        cam = cams[24 * cam_id:24 * cam_id + 24]
        J, Jp, r = O.rows(cam, O.project(cam, X), obs[:, 2 * cam_id], obs[:, 2 * cam_id + 1], 1.0 / sig)
        for i in range(N):
            for k in range(2):
                row = np.zeros(dim, LD)
                row[O.CAM * cam_id:O.CAM * (cam_id + 1)] = J[i, k]
                row[O.DIM + 3 * i:O.DIM + 3 * i + 3] = Jp[i, k]
                rows_J.append(row)
                rows_r.append(LD(r[i, k]))
    for i in range(N):
        for k in range(3):
            if prior[i, 3 + k] > 0:
                row = np.zeros(dim, LD)
                row[O.DIM + 3 * i + k] = LD(1.0) / LD(prior[i, 3 + k])
                rows_J.append(row)
                rows_r.append((LD(X[i, k]) - LD(prior[i, k])) / LD(prior[i, 3 + k]))
    for cam_id in range(2):
        for k in range(3):
            sc = cprior[6 * cam_id + 3 + k]
            if sc > 0:
                row = np.zeros(dim, LD)
                row[O.CAM * cam_id + 3 + k] = LD(1.0) / LD(sc)
                rows_J.append(row)
                rows_r.append((LD(cams[24 * cam_id + 9 + k]) - LD(cprior[6 * cam_id + k])) / LD(sc))
    Jm, r = np.array(rows_J), np.array(rows_r)
    H, g = Jm.T @ Jm, Jm.T @ r
    # the definition's damping: the points' blocks by lambda diag(V), then the REDUCED system's diagonal by lambda times itself
    pp = np.arange(O.DIM, dim)
    H[pp, pp] *= (LD(1.0) + LD(lam))
    schur_diag = np.array([H[a, a] - H[a, O.DIM:] @ _solve_ld(H[O.DIM:, O.DIM:], H[O.DIM:, a]) for a in range(O.DIM)])
    H[np.arange(O.DIM), np.arange(O.DIM)] += LD(lam) * schur_diag
    for p in range(O.DIM):
        if not (mask >> p) & 1:
            H[p, :], H[:, p], H[p, p], g[p] = 0.0, 0.0, 1.0, 0.0
    dense = _solve_ld(H, -g)
    st = O.initial_state(lam)
    it = O.iteration(cams, X, obs, sig, prior, cprior, mask, O.options(), st)
    ours = np.concatenate([it["draft"][O.REC_X:O.REC_X + O.DIM], (it["cand_pts"] - X).reshape(-1)])
    scale = np.sqrt(np.diag(H))                                         # LDL^T is invariant under a diagonal scaling (van der Sluis): judge both in it
    kappa = float(np.linalg.cond((H / np.outer(scale, scale)).astype(np.float64)))
    err = float(np.sqrt(((scale * (ours.astype(LD) - dense)) ** 2).sum()))
    bound = 4 * dim * kappa * U * float(np.sqrt(((scale * dense) ** 2).sum()))
    print(f"mask {mask:#x} all_priors {all_priors}: |d - d_dense| = {err:.3e}, bound {bound:.3e} (kappa {kappa:.2e}), relative {err / float(np.sqrt(((scale * dense) ** 2).sum())):.3e}")
    assert err <= bound + float(scale[O.DIM:].max()) * 3 * N * 2 * U * float(np.abs(X).max())   # forming X' - X in float64 costs an ulp of X per coordinate


# ---- (5), (6) end to end -------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_without_noise_returns_to_the_truth():
    c = BC.by_name("world")
    cams, X, st, hist = O.run(c["cams"], c["X"], c["obs"], c["sig"], c["prior"], c["cprior"], c["mask"], O.options(ctol=2.0 ** -56), O.initial_state(c["lam"]))
    truth = c["truth"]
    assert st[O.ST_STATUS] == O.OK and hist[0, O.REC_COST0] > 1e5 and hist[-1, O.REC_COST1] <= 2.0 ** -56
    df = max(abs(cams[24 * k + 12] - truth[24 * k + 12]) for k in range(2))
    dC = max(np.abs(cams[24 * k + 9:24 * k + 12] - truth[24 * k + 9:24 * k + 12]).max() for k in range(2))
    dR = max(np.abs(cams[24 * k:24 * k + 9] - truth[24 * k:24 * k + 9]).max() for k in range(2))
    dX = np.abs(X[-BC.N_CONTROL:] - c["X_true"][-BC.N_CONTROL:]).max()
    res = O.residuals(cams, X, c["obs"])
    print(f"noise-free: {len(hist)} iterations, cost {hist[-1, O.REC_COST1]:.3e}, |df| {df:.3e}, |dC| {dC:.3e}, |dR| {dR:.3e}, control {dX:.3e}, "
          f"worst residual {np.nanmax(res[:, :, 2]):.3e} px")
    ulp = float(np.spacing(np.abs(c["X_true"]).max()))
    assert ulp == 2.0 ** -30 and df <= 2.0 ** -38 and dC <= ulp and dR <= 2.0 ** -51 and dX <= ulp and np.nanmax(res[:, :, 2]) <= 2.0 ** -36


def test_end_to_end_with_noise_reaches_scipys_cost():
    optimize = pytest.importorskip("scipy.optimize")
    c = BC.by_name("noisy")
    cams0, X0, obs, sig, prior, cprior = _arrays(c)
    free = [p for p in range(O.DIM) if (c["mask"] >> p) & 1]
    n = len(X0)

    def unpack(v):
        x = np.zeros(O.DIM)
        x[free] = v[:len(free)]
        cams = np.concatenate([O.step_camera(cams0[24 * k:24 * k + 24], x[14 * k:14 * k + 14]) for k in range(2)])
        return cams, X0 + v[len(free):].reshape(n, 3)

    def fun(v):
        cams, X = unpack(v)
        out = []
        for k in range(2):
            p = O.project(cams[24 * k:24 * k + 24], X)
            out += [(p["u"] - obs[:, 2 * k]) / sig, (p["v"] - obs[:, 2 * k + 1]) / sig]
        has = prior[:, 3:] > 0
        out.append(((X - prior[:, :3]) / np.where(has, prior[:, 3:], 1.0))[has])
        for k in range(2):
            out.append((cams[24 * k + 9:24 * k + 12] - cprior[6 * k:6 * k + 3]) / cprior[6 * k + 3:6 * k + 6])
        return np.concatenate(out)

    sol = optimize.least_squares(fun, np.zeros(len(free) + 3 * n), method="trf", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=200)
    _, _, st, hist = BC.whole_run("noisy")
    ours = hist[-1, O.REC_COST1]
    start = 0.5 * float((fun(np.zeros(len(free) + 3 * n)) ** 2).sum())
    assert abs(start - hist[0, O.REC_COST0]) <= 1e-12 * start                                      # one function, one start
    gap = abs(ours - sol.cost) / sol.cost
    print(f"with noise: ours {ours!r} in {len(hist)} iterations, scipy {sol.cost!r} in {sol.nfev} evaluations, relative gap {gap:.3e}")
    assert st[O.ST_STATUS] == O.OK and ours <= sol.cost * (1.0 + 1e-10) and gap <= 1e-9
    # the parameters: near the minimum cost(x) - cost(x*) = 0.5 (x - x*)^T H (x - x*) with H = J^T J of the whitened residuals, so a point
    # whose cost is within g of the minimum lies within sqrt(2 g) in the metric of H, i.e. within sqrt(2 g) sigma_i in parameter i, sigma_i^2
    # = (H^-1)_ii. With g <= 1e-9 * cost = 1e-7 for each of the two that is 2 * sqrt(2e-7) = 9e-4 sigma_i between them: asserted at 1e-3
    # sigma_i for f, the centres (both additive in either parametrisation) and, to first order, the rotation entries (sigma of w).
    Jm = np.asarray(sol.jac.todense() if hasattr(sol.jac, "todense") else sol.jac)
    sigma = np.sqrt(np.diag(np.linalg.inv(Jm.T @ Jm)))[:len(free)]
    theirs, _ = unpack(sol.x)
    mine = BC.whole_run("noisy")[0]
    worst = 0.0
    for j, p in enumerate(free):
        k, q = divmod(p, O.CAM)
        if q < 3:
            d = np.abs(mine[24 * k:24 * k + 9] - theirs[24 * k:24 * k + 9]).max() / max(sigma[[free.index(14 * k + a) for a in range(3)]])
        elif q < 6:
            d = abs(mine[24 * k + 9 + q - 3] - theirs[24 * k + 9 + q - 3]) / sigma[j]
        else:
            d = abs(mine[24 * k + 12] - theirs[24 * k + 12]) / sigma[j]
        worst = max(worst, d)
        assert d <= 1e-3, (p, d)
    print(f"parameters: worst difference {worst:.3e} of a standard deviation; sigma_f {sigma[free.index(6)]:.3f} px, sigma_C {sigma[free.index(3)]:.4f} m")


# ---- (7) symmetries that hold in bits ---------------------------------------------------------------------------------------------------------
def test_unusable_points_appended_to_the_last_chunk_change_nothing(host_lib):
    c = BC.by_name("n65")
    base = host_run(host_lib, c)
    X, obs, sig, prior = (np.array(c[k]) for k in ("X", "obs", "sig", "prior"))
    junk = 40
    Xj = np.concatenate([X, np.full((junk, 3), np.nan)])
    Xj[70], Xj[80] = [1.0, 2.0, 3.0], X[3]
    obsj = np.concatenate([obs, np.tile(obs[:1], (junk, 1))])
    obsj[80] = np.nan                                                     # finite coordinates, seen by no camera
    sigj = np.concatenate([sig, np.full(junk, 0.5)])
    sigj[70] = 0.0                                                        # finite coordinates, no weight
    more = host_run(host_lib, c, extra=(Xj, obsj, sigj, np.concatenate([prior, np.zeros((junk, 6))])))
    assert same(more[0], base[0]) and same(more[1][:65], base[1]) and same(more[1][65:], Xj[65:]) and same(more[2], base[2]) and same(more[3], base[3])


def test_the_slot_rule_of_a_table_never_collides():
    """Arithmetic only: the rule csrc/ba.hip places an epoch's chunks by, slot = off[e] / 256 + e, leaves room for every epoch's chunks and
    stays inside M / 256 + E + 1 slots. That a table equals its epochs in any order is a statement about the kernels and is tested on the
    device (tests/test_gpu_ba.py); the host harness has no table."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        sizes = rng.integers(0, 4 * O.BA_CHUNK, rng.integers(1, 9))
        off = np.concatenate([[0], np.cumsum(sizes)])
        slots = [int(off[e]) // O.BA_CHUNK + e for e in range(len(sizes))]
        ends = [s + O.n_chunks(int(n)) for s, n in zip(slots, sizes)]
        assert all(ends[e] <= slots[e + 1] for e in range(len(sizes) - 1)) and ends[-1] <= int(off[-1]) // O.BA_CHUNK + len(sizes) + 1


# ---- (8) the Python layers -------------------------------------------------------------------------------------------------------------------------
def oracle_run(problems, mask, lambda0, opts, states):
    """`sfm.ba_run_device`'s contract on the restatement."""
    out = []
    for e, pr in enumerate(problems):
        st = O.initial_state(lambda0) if states is None else np.array(states[e])
        first = int(st[O.ST_ITER])
        st[O.ST_PARITY] = st[O.ST_DONE] = 0.0
        st[O.ST_STATUS] = O.RUNNING
        cams, X, st, hist = O.run(pr["cams"], pr["X"], pr["obs"], pr["sig"], pr["prior"], pr["cprior"], mask, opts, st)
        out.append((cams, X, st, hist, O.residuals(cams, X, np.asarray(pr["obs"]))))
        assert len(hist) == int(st[O.ST_ITER]) - first
    return out


def _cameras(c):
    from icepy4d_amd.core.camera import Camera
    cams = []
    for k in range(2):
        s = c["cams"][24 * k:24 * k + 24]
        K = np.array([[s[12], 0, s[14]], [0, s[13], s[15]], [0, 0, 1.0]])
        R, C = s[:9].reshape(3, 3), s[9:12].reshape(3, 1)
        cams.append(Camera(6000, 4000, K=K, dist=np.array(s[16:24]), R=R, t=-(R @ C)))
    return cams


def _call(c, **kw):
    n = len(c["X"]) - BC.N_CONTROL
    args = dict(targets=([c["obs"][n:, :2], c["obs"][n:, 2:]], c["prior"][n:, :3]), camera_centers_world=(c["cprior"][0:3], c["cprior"][6:9]),
                image_sigma=0.5, ftol=1e-12, _run=oracle_run)
    args.update(kw)
    return [c["obs"][:n, :2], c["obs"][:n, 2:]], c["X"][:n], args


def test_bundle_adjust_on_the_restatement_leaves_the_originals_untouched():
    from icepy4d_amd import sfm
    c = BC.by_name("noisy")
    cams = _cameras(c)
    before = [(np.array(cam.K), np.array(cam.extrinsics), np.array(cam.dist)) for cam in cams]
    uv, X, args = _call(c)
    X_before = np.array(X)
    pr = sfm.ba_problem(cams, uv, X, args["targets"], args["camera_centers_world"], 0.5)
    n = len(X)
    assert same(pr["X"][:n], c["X"][:n]) and same(pr["X"][n:], c["prior"][n:, :3]) and same(pr["obs"], c["obs"])           # a target starts at its object coordinates
    assert True and same(pr["sig"], c["sig"]) and same(pr["prior"], c["prior"]) and same(pr["cprior"], c["cprior"])
    assert np.abs(pr["cams"] - c["cams"]).max() <= 1e-9 and same(pr["cams"][12:24], c["cams"][12:24])       # C = -R^T (R C) by BLAS
    r = sfm.bundle_adjust(cams, uv, X, **args)
    for cam, (K, ext, dist) in zip(cams, before):
        assert np.array_equal(cam.K, K) and np.array_equal(cam.extrinsics, ext) and np.array_equal(cam.dist, dist)
    assert np.array_equal(X, X_before) and r.cameras[0] is not cams[0]
    assert r.status == "OK" and r.iterations == len(r.history) and r.history[-1, sfm.BA_REC_ACCEPTED] == 1.0
    assert r.cost == r.history[-1, sfm.BA_REC_COST1] and r.points3d.shape == (len(c["X"]), 3) and r.residuals.shape == (len(c["X"]), 2, 3)
    rows, unknowns = 4 * len(c["X"]) + 3 * BC.N_CONTROL + 6, 14 + 3 * len(c["X"])
    assert r.sigma0 == float(np.sqrt(2.0 * r.cost / (rows - unknowns))) and 0.7 < r.sigma0 < 1.3       # unit weight: the noise is the sigma
    for k in range(2):
        new = sfm._ba_camera_state(r.cameras[k])
        assert np.abs(new[:12] - O.run(pr["cams"], pr["X"], pr["obs"], pr["sig"], pr["prior"], pr["cprior"], c["mask"],
                                       sfm._ba_options(1e-3, 1e-12, 1e8, 1e-12, 30, 0.0))[0][24 * k:24 * k + 12]).max() <= 1e-9
        assert r.cameras[k].K[0, 0] == r.cameras[k].K[1, 1] - (before[k][0][1, 1] - before[k][0][0, 0]) and r.cameras[k].dist.shape == (8,)
    split = sfm.bundle_adjust(cams, uv, X, **dict(args, max_iter=2))
    assert split.status == "MAX_ITER" and split.iterations == 2
    rest = sfm.bundle_adjust(split.cameras, [c["obs"][:, :2], c["obs"][:, 2:]], split.points3d, image_sigma=0.5, ftol=1e-12, state=split.state,
                             _run=oracle_run)
    assert rest.history[0, sfm.BA_REC_ITER] == 2.0 and rest.history[0, sfm.BA_REC_LAMBDA] == split.state[0]
    many = sfm.bundle_adjust_epochs(cams, [uv, uv], [X, X], targets=args["targets"], camera_centers_world=args["camera_centers_world"],
                                    image_sigma=0.5, ftol=1e-12, _run=oracle_run)
    assert len(many) == 2 and all(same(m.history, r.history) and same(m.points3d, r.points3d) for m in many)


def test_python_layers_refuse_before_any_device_work():
    from icepy4d_amd import sfm
    c = BC.by_name("n65")
    cams = _cameras(c)
    uv, X, args = _call(c)

    def bad(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            sfm.bundle_adjust(*a, **dict(args, **kw))

    bad("two cameras", cams[:1], uv, X)
    bad("one row per tie point", cams, [uv[0][:-1], uv[1]], X)
    bad("one row per tie point", cams, uv, X[:-1])
    for m in (-1, 1 << 28, 2.5):
        bad("mask", cams, uv, X, mask=m)
    for s in (0.0, -1.0, np.nan, np.inf):
        bad("image_sigma", cams, uv, X, image_sigma=s)
        bad("target_image_sigma", cams, uv, X, target_image_sigma=s)
    bad("targets", cams, uv, X, targets=([uv[0][:3], uv[1][:3]], X[:4]))
    bad("target_accuracy", cams, uv, X, target_accuracy=-0.01)
    bad("cam_accuracy", cams, uv, X, cam_accuracy=np.nan)
    bad("camera centre", cams, uv, X, camera_centers_world=([0.0, np.nan, 0.0], None))
    bad("one centre", cams, uv, X, camera_centers_world=([0.0, 0.0, 0.0],))
    bad("lambda0", cams, uv, X, lambda0=-1.0)
    bad("lambda_min", cams, uv, X, lambda_min=0.0)
    bad("lambda_min", cams, uv, X, lambda_min=1.0, lambda_max=0.5)
    bad("ftol", cams, uv, X, ftol=-1.0)
    for m in (0, 2.5, 10001):
        bad("max_iter", cams, uv, X, max_iter=m)
    with pytest.raises(ValueError, match="one entry per epoch"):
        sfm.bundle_adjust_epochs(cams, [uv], [X, X], _run=oracle_run)
    with pytest.raises(ValueError, match="one entry per epoch"):
        sfm.bundle_adjust_epochs(cams, [uv, uv], [X, X], targets=[args["targets"]], _run=oracle_run)
    with pytest.raises(ValueError, match="unknown parameter"):
        sfm.ba_mask(("pose", "b1"))
    assert sfm.ba_mask() == O.MASK_DEFAULT == sfm.BA_MASK_DEFAULT and sfm.ba_mask(("all",)) == O.MASK_ALL
    assert sfm.ba_mask(("f", "k1"), cameras=(1,)) == (1 << 20) | (1 << 23) and sfm.ba_mask(("rotation",), (0,)) == 7
    assert (sfm.BA_REC_COST0, sfm.BA_REC_COST1, sfm.BA_REC_LAMBDA, sfm.BA_REC_ACCEPTED, sfm.BA_REC_COUNT, sfm.BA_REC_STATUS, sfm.BA_REC_X, sfm.BA_REC_PIVOT,
            sfm.BA_REC_ITER, sfm.BA_RECORD, sfm.BA_STATE, sfm.BA_SOL) == (O.REC_COST0, O.REC_COST1, O.REC_LAMBDA, O.REC_ACCEPTED, O.REC_COUNT, O.REC_STATUS,
                                                                     O.REC_X, O.REC_PIVOT, O.REC_ITER, O.RECORD, O.STATE, O.SOL)
    assert sfm.BA_STATUS == O.STATUS_NAMES and "Metashape" in sfm.bundle_adjust.__doc__


def test_the_csv_writers_character_for_character(tmp_path):
    import pandas as pd
    from icepy4d_amd import io as IO
    from icepy4d_amd.utils.homography import euler_from_matrix
    c = BC.by_name("absent")
    cams = _cameras(c)
    path = tmp_path / "cameras.csv"
    IO.write_cameras_to_file(path, "2022-07-28", {"p1": cams[0], "p2": cams[1]})
    IO.write_cameras_to_file(path, "2022-07-29", cams, sep=",")
    want = "date,f1,omega1,phi1,kappa1,f2,omega2,phi2,kappa2\n"
    row = ""
    for cam in cams:
        o, p, k = (np.degrees(a) for a in euler_from_matrix(np.asarray(cam.R).T))
        row += ",%.2f,%.4f,%.4f,%.4f" % (cam.K[1, 1], o, p, k)
    assert path.read_text() == want + "2022-07-28" + row + "\n" + "2022-07-29" + row + "\n"
    res = O.residuals(c["cams"], c["X"], c["obs"])
    path = tmp_path / "res.csv"
    IO.write_reprojection_error_to_file(path, 3, res)
    IO.write_reprojection_error_to_file(path, 4, res)
    frame = pd.DataFrame({"track_id": np.arange(len(res)), "x_p1": res[:, 0, 0], "y_p1": res[:, 0, 1], "norm_p1": res[:, 0, 2],
                          "x_p2": res[:, 1, 0], "y_p2": res[:, 1, 1], "norm_p2": res[:, 1, 2]})
    frame["global_norm"] = (res[:, 0, 2] + res[:, 1, 2]) / 2
    d = frame.describe()
    stats = ["count", "mean", "std", "min", "25%", "50%", "75%", "max"]
    header = "ep," + ",".join(f"{s}-{col}" for s in stats for col in frame.columns)
    line = ",".join(str(d.loc[s, col]) for s in stats for col in frame.columns)
    assert path.read_text() == header + "\n3," + line + "\n4," + line + "\n"
    assert d.loc["count", "x_p1"] == 97.0 and d.loc["count", "global_norm"] < 97.0                   # a NaN norm in either camera: no global norm
    table = IO.reprojection_table([res, res], ["a", "b"], out_path=tmp_path / "o" / "table.csv")
    assert list(table.index) == ["a", "b"] and list(table.columns) == header.split(",")[1:] and table.loc["b", "mean-norm_p2"] == d.loc["mean", "norm_p2"]
    assert (tmp_path / "o" / "table.csv").read_text() == header + "\na," + line + "\nb," + line + "\n"
    with pytest.raises(ValueError, match="residuals"):
        IO.residual_frame(np.zeros((5, 3, 3)))


# ---- (9) housekeeping ------------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_and_bound(host_lib):
    from icepy4d_amd import _lib
    header = open(os.path.join(ROOT, "include", "icematch.h")).read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and name in _lib.SIGNATURES, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), (name, len(m.group(1).split(",")), len(_lib.SIGNATURES[name]))
    assert re.search(r"\bint im_ba_chunk\(void\);", header) and _lib.SIGNATURES["im_ba_chunk"] == []
    assert "-82" in header and "-82" in open(os.path.join(ROOT, "icepy4d_amd", "csrc", "ba.hip")).read()
    assert not re.search(r"= -82\b", "".join(open(os.path.join(ROOT, "icepy4d_amd", "csrc", f)).read() for f in os.listdir(os.path.join(ROOT, "icepy4d_amd", "csrc"))
                                             if f.endswith(".hip") and f != "ba.hip"))          # a refusal code of its own
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW_SYMBOLS)
    assert lib.im_ba_chunk() == O.BA_CHUNK == host_lib.ba_host_chunk() == 256


def test_the_scratch_carve_is_pinned(host_lib):
    up = lambda b: -(-b // 256) * 256
    for E, M in ((1, 0), (1, 1), (1, 255), (1, 256), (3, 322), (1000, 10_000_000), (65535, 1 << 26)):
        slots = M // 256 + E + 1
        assert host_lib.ba_host_scratch(E, M) == up(8 * O.TERMS * slots) + up(8 * slots) + up(8 * O.KEEP * max(M, 1)), (E, M)


@pytest.mark.parametrize("module", ["icepy4d_amd.io", "icepy4d_amd.sfm"])
def test_new_modules_import_first_in_a_fresh_interpreter(module):
    r = subprocess.run([sys.executable, "-c", f"import {module} as m; print(m.__name__)"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == module, r.stderr[-2000:]


def test_the_ba_kernels_stay_out_of_scratch_memory(tmp_path):
    res = toolchain.kernel_resources(toolchain.device_listing("ba.hip", str(tmp_path)))
    lds = {"ba_accumulate_kernel": O.BA_TILE * O.FAC * 8, "ba_solve_kernel": (O.TERMS + O.DIM * O.DIM + 5 * O.DIM + O.RECORD) * 8,
           "ba_step_points_kernel": O.BA_CHUNK * 8, "ba_decide_kernel": O.RECORD * 8, "ba_residuals_kernel": 0}
    for kernel, want in lds.items():
        r = res[next(k for k in res if kernel in k)]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, kernel   # no spills, no scratch memory
        assert r["group_segment_fixed_size"] == want, (kernel, r["group_segment_fixed_size"], want)


def test_bundle_adjust_table_on_the_restatement():
    """A gathered match table with the keypoint payload: the matched keypoints in ascending keypoint-0 index, a failed record, the
    reconstruction given (no device): every record equals `bundle_adjust` on its own points."""
    from icepy4d_amd import sfm
    from icepy4d_amd.sequence import HEADER, record_words
    c = BC.by_name("noisy")
    cams = _cameras(c)
    n, K = 40, 64
    rng = np.random.default_rng(3)
    table = np.full((3, record_words(K, True)), -1, np.int32)
    points, uvs = [], []
    for e in range(3):
        if e == 1:
            table[e, :4] = [e, -1, -1, -1]                               # a failed record
            points.append(np.zeros((0, 3)))
            uvs.append([np.zeros((0, 2)), np.zeros((0, 2))])
            continue
        sel = np.sort(rng.choice(len(c["X"]) - BC.N_CONTROL, n, replace=False))
        slots0 = np.sort(rng.choice(K, n, replace=False))                # keypoint-0 indices of the matches, ascending with the points
        perm1 = rng.permutation(K)[:n]                                   # their partners in image 1
        k0, k1 = np.zeros((K, 2), np.float32), np.zeros((K, 2), np.float32)
        k0[slots0], k1[perm1] = c["obs"][sel, :2], c["obs"][sel, 2:]
        m0 = np.full(K, -1, np.int32)
        m0[slots0] = perm1
        table[e, :5] = [e, K, K, n, 0]
        table[e, HEADER:HEADER + K] = m0
        table[e, HEADER + 2 * K:] = np.concatenate([k0, k1]).reshape(-1).view(np.int32)
        points.append(np.array(c["X"][sel]))
        uvs.append([k0[slots0].astype(np.float64), k1[perm1].astype(np.float64)])
    got = sfm.table_image_points(table, K)
    assert all(same(g[0], w[0]) and same(g[1], w[1]) for g, w in zip(got, uvs))
    rec = sfm.TableReconstruction(points, [np.ones(len(p), np.int64) for p in points], None, np.array([0, n, n, 2 * n]))
    nc = len(c["X"]) - BC.N_CONTROL
    kw = dict(targets=([c["obs"][nc:, :2], c["obs"][nc:, 2:]], c["prior"][nc:, :3]), camera_centers_world=(c["cprior"][0:3], c["cprior"][6:9]),
              image_sigma=0.5, _run=oracle_run)
    out = sfm.bundle_adjust_table(table, K, cams, reconstruction=rec, **kw)
    assert len(out) == 3 and out[0].status == "OK" == out[2].status and out[1].points3d.shape == (BC.N_CONTROL, 3)
    for e in (0, 2):
        alone = sfm.bundle_adjust(cams, uvs[e], points[e], **kw)
        assert same(out[e].history, alone.history) and same(out[e].points3d, alone.points3d)
    with pytest.raises(ValueError, match="does not belong"):
        sfm.bundle_adjust_table(table, K, cams, reconstruction=rec._replace(points3d=points[::-1][:2] + [points[0][:5]]), **kw)
    with pytest.raises(ValueError, match="int32 table"):
        sfm.table_image_points(table[:, :-1], K)
