"""The inputs on which the per-point arithmetic of csrc/sfm.hip is compared with the numpy restatement (tests/sfm_oracle.py) bit for bit:
by the host build of the kernels' text (tests/test_sfm_cpu.py) and on the device (tests/test_gpu_sfm_edges.py). One list, so both see the
same cases, and the restatement's result of a case is computed once per process (`expected`).

A case is (name, u1, P1, u2, P2, tolerance, max_solves); float32 points take the float32 kernel, float64 points the float64 one."""
import numpy as np

import sfm_oracle as S

N_DEGENERATE = 64


def value_rows(g):
    """Rows 4990 .. 5199 of g13 (status 1 up to row 4999, -3 from row 5000, -2 from row 5060; these stop after 2, 5, 7, 8 or 10 solves)
    and in front of them the first three rows of every solve count 2 .. 10 the fixture stores: 237 points."""
    first = [np.flatnonzero(g["solves"][:4990] == k)[:3] for k in range(2, 11)]
    return np.concatenate(first + [np.arange(4990, 5200)])

def perturbed64(g):
    """The fixture's undistorted points as true float64 values: float32 widened plus uniform(-1e-3, 1e-3) px, `default_rng(1)`, image 0
    first. No float32 holds these values, so the float64 kernel cannot be replaced by the float32 one unnoticed."""
    rng = np.random.default_rng(1)
    a = g["und0"].astype(np.float64) + rng.uniform(-1e-3, 1e-3, g["und0"].shape)
    b = g["und1"].astype(np.float64) + rng.uniform(-1e-3, 1e-3, g["und1"].shape)
    return a, b


def value_cases(g):
    """Every solve limit, tolerances on both sides of the usual one, both orders of the views, true float64 points."""
    rows = value_rows(g)
    u1, u2, P1, P2 = g["und0"][rows], g["und1"][rows], g["P0"], g["P1"]
    out = [(f"max_solves={k}", u1, P1, u2, P2, 3e-5, k) for k in range(1, 11)]
    out += [(f"tolerance={t:g}", u1, P1, u2, P2, t, 10) for t in (0.0, 1e-9, 1e-2)]
    out.append(("views swapped", u2, P2, u1, P1, 3e-5, 10))
    a, b = perturbed64(g)
    out.append(("float64 points", a[rows], P1, b[rows], P2, 3e-5, 10))
    return out


def _with(P, entries):
    P = np.array(P, np.float64)
    for (i, j), v in entries.items():
        P[i, j] = v
    return P


def degenerate_cases(g):
    """Systems without full rank and inputs that are not finite, 64 points each: the minimum-norm branch of the solver, and the
    comparisons a NaN fails (the rotation test of the Jacobi sweep, the singular-value threshold, the depth tests of the status)."""
    n = N_DEGENERATE
    u1, u2, P1, P2 = g["und0"][:n], g["und1"][:n], g["P0"], g["P1"]
    nan, inf = np.nan, np.inf
    ur = g["und0"][4990:4990 + n]                              # the minimum-norm point lies in front of the camera for one of these
    out = [("rank 2: one camera, one image point twice", ur, P1, ur, P1, 3e-5, 10),
           ("rank 2, one solve", ur, P1, ur, P1, 3e-5, 1),
           ("rank 0: zero projection matrices", u1, np.zeros((3, 4)), u2, np.zeros((3, 4)), 3e-5, 10)]
    # non-finite image points: every fourth point keeps its values; the others get one bad coordinate, then two, then all four
    bad32 = np.array([nan, inf, -inf, 3.0e38], np.float32)
    bad64 = np.array([nan, inf, -inf, 1e300, -1e300, 1e160])
    for name, bad, dt in (("float32", bad32, np.float32), ("float64", bad64, np.float64)):
        a, b = u1.astype(dt), u2.astype(dt)
        flat = np.concatenate([a, b], 1)                       # [n, 4]: u1x u1y u2x u2y
        for i in range(n):
            v = bad[i % len(bad)]
            if i % 4 == 1:
                flat[i, (i // 4) % 4] = v
            elif i % 4 == 2:
                flat[i, (i // 4) % 4] = v
                flat[i, (i // 4 + 2) % 4] = bad[(i + 1) % len(bad)]
            elif i % 4 == 3:
                flat[i, :] = v
        out.append((f"non-finite image points, {name}", np.ascontiguousarray(flat[:, :2]), P1, np.ascontiguousarray(flat[:, 2:]), P2, 3e-5, 10))
    for name, e1, e2 in (("NaN in P1[0, 0]", {(0, 0): nan}, {}),
                         ("inf in P2[1, 3]", {}, {(1, 3): inf}),
                         ("NaN in P1[2, 3]", {(2, 3): nan}, {}),
                         ("NaN in P2[2, 3]", {}, {(2, 3): nan}),
                         ("NaN in P[2, 3] of both cameras", {(2, 3): nan}, {(2, 3): nan}),
                         ("inf in P1[2, 3], -inf in P2[2, 3]", {(2, 3): inf}, {(2, 3): -inf}),
                         ("-inf in P1[2, 3], inf in P2[2, 3]", {(2, 3): -inf}, {(2, 3): inf}),
                         ("1e300 in P1[2, 0 .. 2]", {(2, 0): 1e300, (2, 1): 1e300, (2, 2): -1e300}, {})):
        out.append((f"non-finite projection: {name}", u1, _with(P1, e1), u2, _with(P2, e2), 3e-5, 10))
    return out


_CACHE = {}


def expected(case):
    """(X [n, 3] float64, status [n] int32) of the restatement, computed once per case name."""
    name, u1, P1, u2, P2, tol, ms = case
    if name not in _CACHE:
        X, st = S.triangulate_iterative(u1, P1, u2, P2, tol, ms)
        X.setflags(write=False)
        st = st.astype(np.int32)
        st.setflags(write=False)
        _CACHE[name] = (X, st)
    return _CACHE[name]
