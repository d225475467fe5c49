"""The reconstruction kernels (csrc/sfm.hip, csrc/sfm_point.h, csrc/lstsq_jacobi.h) on the device at every boundary between two code paths:
every solve limit and status value, rank-deficient and non-finite systems, the thread grid of the flat kernels, the compaction of the
table kernel across wave and chunk edges, the capacity cut, the second chunk of the offsets scan, one camera pair per record, K = 16384
(65536 bytes of dynamic LDS next to 16 static ones: the launch needs the per-kernel opt-in), and the refusals of the C entry points.

Bound: equality of bits with the numpy restatement (tests/sfm_oracle.py), for every value and every row; no row is left out. Derived, not
measured: the kernels and the restatement perform the same IEEE float64 operations in the same order, contraction is off in every
function involved, float64 division and square root are correctly rounded on the device, and the library is built without a fast-math
flag. The host build of the same text agrees with the restatement on every case used here (tests/test_sfm_cpu.py), and no case produces a
NaN coordinate from arithmetic (the NaN rows of the table kernel are a constant it writes), so no NaN payload enters the comparison.

Every output buffer is at least one row longer than the call may write and is filled with a sentinel first (a NaN with a payload, -77 in
the integer buffers): the tail, and every row the contract leaves alone, must hold the sentinel afterwards, bit for bit. The calls go
through the C ABI wherever `icepy4d_amd.sfm` cannot reach the path (the `und` outputs of the table call, a capacity below the total,
max_solves other than 1 and 10)."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sfm_cases as C  # noqa: E402
import sfm_oracle as S  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = {np.dtype(np.float64): np.int64(0x7FF85E4700C0FFEE), np.dtype(np.float32): np.int32(0x7FC5E477), np.dtype(np.int32): np.int32(-77),
        np.dtype(np.int64): np.int64(-77)}
INT_MIN, INT_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
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


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def sentinel(eng, shape, dtype):
    """A device buffer of `shape` whose every element is the sentinel of `dtype`."""
    import torch
    dt = np.dtype(dtype)
    host = np.full(shape, SENT[dt], bits(np.zeros(1, dt)).dtype).view(dt)
    return torch.from_numpy(host).to(eng.device)


def check(buf, want, what):
    """The first len(want) rows of the device buffer are `want` bit for bit; every row behind them still holds the sentinel."""
    got = buf.cpu().numpy()
    want = np.asarray(want)
    n = len(want)
    assert got.dtype == want.dtype and n < len(got) and got.shape[1:] == want.shape[1:], (what, got.dtype, want.dtype, got.shape, want.shape)
    same = bits(got[:n]) == bits(want)
    assert same.all(), (what, f"{int((~same).sum())} of {same.size} values differ, first at row {int(np.argwhere(~same)[0][0])}")
    assert (bits(got[n:]) == SENT[got.dtype]).all(), (what, "a row behind the output was written")


def untouched(*bufs):
    hosts = [b.cpu().numpy() for b in bufs if b is not None]
    return all((bits(h) == SENT[h.dtype]).all() for h in hosts)


def dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def p(t):
    from icepy4d_amd._lib import ptr
    return ptr(t)


def intrinsics(K, dist):
    return np.ascontiguousarray(S.camera_row(np.zeros((3, 4)), K, dist)[12:])


# ---- the flat calls through the C ABI -------------------------------------------------------------------------------------------------
def call_undistort(eng, pts, cam, n=None, pad=1):
    n = len(pts) if n is None else n
    d, out = dev(eng, pts), sentinel(eng, (len(pts) + pad, 2), np.float32)
    eng.ctx.call("im_undistort_points", p(d), n, cam.ctypes.data, p(out), eng.stream_ptr())
    return out


def call_triangulate(eng, u1, P1, u2, P2, tolerance=3e-5, max_solves=10, cam1=None, cam2=None, want_und=False, n=None, pad=1):
    """-> the device buffers X [n + pad, 3], status [n + pad], und1, und2 [n + pad, 2] (or None)."""
    u1, u2 = np.ascontiguousarray(u1), np.ascontiguousarray(u2)
    assert u1.dtype == u2.dtype and u1.dtype in (np.float32, np.float64)
    f64 = int(u1.dtype == np.float64)
    rows = len(u1) + pad
    n = len(u1) if n is None else n
    d1, d2 = dev(eng, u1), dev(eng, u2)
    X, st = sentinel(eng, (rows, 3), np.float64), sentinel(eng, (rows,), np.int32)
    und1 = sentinel(eng, (rows, 2), np.float32) if want_und else None
    und2 = sentinel(eng, (rows, 2), np.float32) if want_und else None
    P1, P2 = np.ascontiguousarray(P1, np.float64), np.ascontiguousarray(P2, np.float64)
    out = (X, st, und1, und2)
    try:
        eng.ctx.call("im_triangulate_iterative", p(d1), p(d2), f64, n, P1.ctypes.data, P2.ctypes.data,
                     None if cam1 is None else cam1.ctypes.data, None if cam2 is None else cam2.ctypes.data, float(tolerance), int(max_solves),
                     p(X), p(st), p(und1), p(und2), eng.stream_ptr())
    except Exception as e:
        e.outputs = out
        raise
    return out


def run_case(eng, case):
    name, u1, P1, u2, P2, tol, ms = case
    X, st, _, _ = call_triangulate(eng, u1, P1, u2, P2, tol, ms)
    Xo, so = C.expected(case)
    check(X, Xo, name)
    check(st, so, name)
    return X.cpu().numpy()[:len(Xo)]


# ---- a. values ------------------------------------------------------------------------------------------------------------------------
def test_flat_triangulation_values(g13, eng):
    """Solve limits 1 .. 10, tolerances 0, 1e-9, 1e-2, the views swapped (status -1), true float64 points."""
    got = {case[0]: run_case(eng, case) for case in C.value_cases(g13)}
    assert len(got) == 15
    # the float64 kernel ran on values no float32 holds: its points are not those of the float32 path
    assert (got["float64 points"] != got["max_solves=10"]).any(1).all()
    assert all(not np.array_equal(got[f"max_solves={k}"], got[f"max_solves={k + 1}"]) for k in range(1, 10))


# ---- b. degenerate and non-finite inputs ----------------------------------------------------------------------------------------------
def test_rank_deficient_and_non_finite_systems(g13, eng):
    """Rank 2 (minimum-norm points, statuses 1 and -3), rank 0, NaN / inf / huge image points, NaN / inf projection entries: X = 0
    wherever a NaN reaches the system, the status from P[2, 3] alone, status 0 where both depths are NaN."""
    cases = C.degenerate_cases(g13)
    for case in cases:
        run_case(eng, case)
    seen = set(np.concatenate([C.expected(c)[1] for c in cases]).tolist())
    assert seen == {1, 0, -1, -2, -3}


# ---- c. the thread grid ---------------------------------------------------------------------------------------------------------------
GRID = (1, 255, 256, 257, 513)


def test_grid_boundaries_of_the_flat_kernels(g13, eng):
    g = g13
    idx = np.arange(5199, 5199 - 513, -1)              # -2 first, -3 from position 140, 1 from position 200
    k0, k1, u0, u1 = g["kpts0"][idx], g["kpts1"][idx], g["und0"][idx], g["und1"][idx]
    dist8 = np.r_[g["dist1"], 0.01, -0.02, 0.005]
    assert len(g["dist0"]) == 5 and len(dist8) == 8
    a64, b64 = (x[idx] for x in C.perturbed64(g))
    Xp, sp = S.triangulate_iterative(u0, g["P0"], u1, g["P1"], 3e-5, 10)
    X64, s64 = S.triangulate_iterative(a64, g["P0"], b64, g["P1"], 3e-5, 10)
    assert {1, -2, -3} <= set(sp[:255].tolist())
    fused = {}
    for key, d0, d1 in (((5, 8), g["dist0"], dist8), ((0, 4), None, g["dist0"][:4])):
        f0, f1 = S.undistort_points_f64(k0, g["K0"], d0), S.undistort_points_f64(k1, g["K1"], d1)
        fused[key] = (intrinsics(g["K0"], d0), intrinsics(g["K1"], d1), f0, f1, S.triangulate_iterative(f0, g["P0"], f1, g["P1"], 3e-5, 10))
    assert not np.array_equal(S.undistort_points_f64(k1, g["K1"], g["dist0"]), S.undistort_points_f64(k1, g["K1"], dist8))
    for n in GRID:
        for dist, K, pts in ((g["dist0"], g["K0"], k0), (dist8, g["K1"], k1)):
            check(call_undistort(eng, pts[:n], intrinsics(K, dist)), S.undistort_points_f64(pts[:n], K, dist), ("undistort", n))
        X, st, _, _ = call_triangulate(eng, u0[:n], g["P0"], u1[:n], g["P1"])
        check(X, Xp[:n], ("plain", n))
        check(st, sp[:n].astype(np.int32), ("plain", n))
        X, st, _, _ = call_triangulate(eng, a64[:n], g["P0"], b64[:n], g["P1"])
        check(X, X64[:n], ("float64", n))
        check(st, s64[:n].astype(np.int32), ("float64", n))
        for key, (c0, c1, f0, f1, (Xf, sf)) in fused.items():
            X, st, w0, w1 = call_triangulate(eng, k0[:n], g["P0"], k1[:n], g["P1"], cam1=c0, cam2=c1, want_und=True)
            check(X, Xf[:n], ("fused", key, n))
            check(st, sf[:n].astype(np.int32), ("fused", key, n))
            check(w0, f0[:n], ("fused und1", key, n))
            check(w1, f1[:n], ("fused und2", key, n))
    # n below the buffers' length: the rows behind n stay as they were, whatever the inputs hold there
    X, st, w0, w1 = call_triangulate(eng, k0[:300], g["P0"], k1[:300], g["P1"], cam1=fused[(5, 8)][0], cam2=fused[(5, 8)][1], want_und=True, n=256)
    Xf, sf = fused[(5, 8)][4]
    check(X, Xf[:256], "n = 256 of 300")
    check(st, sf[:256].astype(np.int32), "n = 256 of 300")
    check(w0, fused[(5, 8)][2][:256], "n = 256 of 300")
    check(w1, fused[(5, 8)][3][:256], "n = 256 of 300")


# ---- d. the table kernel --------------------------------------------------------------------------------------------------------------
def fixture_pair(g):
    return [S.camera_row(g["P0"], g["K0"], g["dist0"]), S.camera_row(g["P1"], g["K1"], g["dist1"])]


def source_rows(K, shift=0):
    """Fixture rows for the K keypoint slots of a record: the rows of every status first (4990 ..), then on through the fixture."""
    return (4990 + shift + np.arange(K)) % 5200


def record(g, K, m0, shift=0):
    """(kpts0, kpts1, matches0) of a record with the given matches0 [K]: slot i holds fixture point src[i] of image 0, and the slot of
    image 1 that a valid entry names holds the same fixture point of image 1 (the last writer wins where targets repeat)."""
    src = source_rows(K, shift)
    m0 = np.asarray(m0, np.int64)
    k0, k1 = g["kpts0"][src].copy(), g["kpts1"][src].copy()
    ok = np.flatnonzero((m0 >= 0) & (m0 < K))
    k1[m0[ok]] = g["kpts1"][src[ok]]
    return k0, k1, m0


def sparse_matches(rng, K, density=0.35):
    m0 = np.full(K, -1, np.int64)
    on = rng.random(K) < density
    on[K - 1] = True
    m0[on] = rng.permutation(K)[:int(on.sum())]
    return m0


def call_table(eng, table, K, cams, undistort, tolerance, max_solves, m_cap, rows, null_outputs=False, n_records=None, n_cams=None,
               null_offsets=False):
    """`im_triangulate_table` on sentinel-filled buffers of `rows` rows (offsets: E + 2 entries) -> the device buffers."""
    cams = np.ascontiguousarray(np.asarray(cams, np.float64).reshape(-1, 2, 24))
    E = len(table)
    dt, dc = dev(eng, table), dev(eng, cams)
    off = sentinel(eng, (E + 2,), np.int64)
    X, st = sentinel(eng, (rows, 3), np.float64), sentinel(eng, (rows,), np.int32)
    w0, w1 = sentinel(eng, (rows, 2), np.float32), sentinel(eng, (rows, 2), np.float32)
    out = (off, X, st, w0, w1)
    args = (None, None, None, None) if null_outputs else (p(X), p(st), p(w0), p(w1))
    try:
        eng.ctx.call("im_triangulate_table", p(dt), E if n_records is None else n_records, int(K), p(dc), len(cams) if n_cams is None else n_cams,
                     int(undistort), float(tolerance), int(max_solves), int(m_cap), None if null_offsets else p(off), *args, eng.stream_ptr())
    except Exception as e:
        e.outputs = out
        raise
    return out


def check_table(eng, table, K, cams, undistort=1, tolerance=3e-5, max_solves=10, m_cap=None, what=""):
    """The call against `S.triangulate_table`: offsets, points, statuses and both `und` outputs, the rows at and behind the capacity and
    behind the total untouched. -> the restatement's (offsets, X, status, und0, und1)."""
    total = int(np.maximum(table[:, 3], 0).sum())
    m_cap = total if m_cap is None else m_cap
    want = S.triangulate_table(table, K, cams, undistort, tolerance, max_solves, m_cap)
    assert len(want[1]) == min(total, m_cap) and want[0][-1] == total
    got = call_table(eng, table, K, cams, undistort, tolerance, max_solves, m_cap, rows=total + 1)
    for name, a, b in zip(("offsets", "X", "status", "und0", "und1"), got, want):
        check(a, b, (what, K, name, f"m_cap {m_cap} of {total}"))
    return want


K_LADDER = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 16384)


@pytest.mark.parametrize("K", K_LADDER)
def test_table_at_every_record_size(g13, eng, K):
    """Three records per size: every slot matched in reversed order, a sparse one, a failed one. K = 16384 takes 65536 bytes of dynamic
    LDS and 16 static ones: more than 64 KB in all."""
    rng = np.random.default_rng(K)
    epochs = [record(g13, K, np.arange(K)[::-1]), record(g13, K, sparse_matches(rng, K), shift=100), None]
    table = S.pack_table(epochs, K)
    assert table[0, 3] == K and 1 <= table[1, 3] <= K and table[2, 3] == -1
    off, X, st, _, _ = check_table(eng, table, K, [fixture_pair(g13)], undistort=1, max_solves=10 if K <= 1000 else 3, what="ladder")
    assert off.tolist() == [0, K, K + table[1, 3], K + table[1, 3]] and np.isfinite(X).all()
    if K >= 255:
        assert {1, -2, -3} <= set(st.tolist())


def test_table_compaction_edges(g13, eng):
    """K = 1000 (four chunks of 256 slots, the last one short): matches in the last chunk alone, on the wave and chunk edges, entries
    of matches0 outside [0, K), repeated targets, headers that promise more and fewer matches than there are, n_matches = -7."""
    g, K = g13, 1000
    none = np.full(K, -1, np.int64)

    def only(slots, targets=None):
        m = none.copy()
        m[np.asarray(slots)] = np.asarray(slots if targets is None else targets)
        return m
    invalid = only(np.arange(0, K, 3))
    bad_slots = [0, 63, 66, 255, 258, 513, 768, 999]
    invalid[bad_slots] = [K, K + 5, -2, INT_MIN, INT_MAX, K, -2, INT_MAX]
    epochs = [record(g, K, only([768, 769, 831, 832, 998, 999])),
              record(g, K, only([62, 63, 64, 65, 254, 255, 256, 257], [257, 256, 255, 254, 65, 64, 63, 62])),
              record(g, K, invalid),
              record(g, K, np.arange(K) // 2),                                    # every target twice
              record(g, K, only(np.arange(100, 400))),                            # the header will promise 9 more
              record(g, K, np.arange(K)),                                         # the header will promise 257 of the 1000
              record(g, K, only(np.arange(0, K, 2))),                             # n_matches = -7
              record(g, K, only([999], [0]))]
    table = S.pack_table(epochs, K)
    n_valid = len(np.arange(0, K, 3)) - len(bad_slots)                            # every bad slot replaces a valid entry
    assert all(s % 3 == 0 for s in bad_slots) and table[2, 3] == n_valid + 5      # the packer counts what is > -1: five more than the kernel takes
    table[4, 3] += 9
    table[5, 3] = 257
    table[6, 3] = -7
    for undistort, max_solves in ((1, 3), (0, 1), (0, 3), (1, 1)):
        off, X, st, w0, _ = check_table(eng, table, K, [fixture_pair(g)], undistort, 3e-5, max_solves, what="edges")
        assert off.tolist() == np.r_[0, np.cumsum([6, 8, n_valid + 5, K, 309, 257, 0, 1])].tolist()
        nan_rows = np.isnan(X).all(1)
        want_nan = np.zeros(len(X), bool)
        want_nan[off[2] + n_valid:off[3]] = True
        want_nan[off[4] + 300:off[5]] = True
        assert np.array_equal(nan_rows, want_nan) and (st[nan_rows] == 0).all() and np.isnan(w0[nan_rows]).all()
    # the order of the kept entries: record 2 without its bad slots is the same points in the same rows
    clean = invalid.copy()
    clean[bad_slots] = -1
    t2 = S.pack_table([record(g, K, clean)], K)
    Xc = S.triangulate_table(t2, K, [fixture_pair(g)], 1, 3e-5, 3, 10 ** 6)[1]
    Xi = S.triangulate_table(table[2:3], K, [fixture_pair(g)], 1, 3e-5, 3, 10 ** 6)[1]
    assert len(Xc) == n_valid and np.array_equal(bits(Xi[:n_valid]), bits(Xc))


@pytest.mark.parametrize("E", (1, 255, 256, 257, 513))
def test_offsets_scan_across_its_chunks(g13, eng, E):
    """K = 8; empty, failed, full and partly matched records in turn (the first record full, so that E = 1 has points)."""
    K = 8
    kinds = [np.arange(K)[::-1], np.full(K, -1), None, np.array([3, -1, -1, 0, -1, 7, -1, -1])]
    epochs = [None if kinds[e % 4] is None else record(g13, K, kinds[e % 4], shift=7 * e) for e in range(E)]
    table = S.pack_table(epochs, K)
    off = check_table(eng, table, K, [fixture_pair(g13)], undistort=1, max_solves=1, what=("scan", E))[0]
    assert off[-1] == sum((8, 0, 0, 3)[e % 4] for e in range(E))


def test_table_capacity_cut(g13, eng):
    """m_cap at the total, inside a record (inside a stride of the block and inside the NaN rows), at a record boundary, 1 and 0: the
    rows at and behind it are never written and the offsets are the full scan every time."""
    g, K = g13, 600
    rng = np.random.default_rng(3)
    epochs = [record(g, K, np.arange(K)[::-1]), record(g, K, sparse_matches(rng, K), shift=50), None, record(g, K, np.arange(K), shift=9)]
    table = S.pack_table(epochs, K)
    n1 = int(table[1, 3])
    table[1, 3] = n1 + 300                                                        # 300 NaN rows behind the sparse record's points
    total = 600 + n1 + 300 + 600
    cams = [fixture_pair(g)]
    full = S.triangulate_table(table, K, cams, 1, 3e-5, 3, total)
    for m_cap in (total, total + 5, 300, 600, 617, 600 + n1 + 150, 600 + n1 + 300, total - 1, 1, 0):
        off, X, st, _, _ = check_table(eng, table, K, cams, 1, 3e-5, 3, m_cap, what="capacity")
        assert np.array_equal(off, full[0]) and np.array_equal(bits(X), bits(full[1][:m_cap])) and np.array_equal(st, full[2][:m_cap])
    # no capacity and no outputs: the offsets alone
    off, X, st, w0, w1 = call_table(eng, table, K, cams, 1, 3e-5, 3, 0, rows=4, null_outputs=True)
    check(off, full[0], "offsets with m_cap = 0")
    assert untouched(X, st, w0, w1)


def perturbed_pair(g, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in ("0", "1"):
        P = g["P" + k] * (1.0 + 1e-3 * rng.uniform(-1, 1, (3, 4)))
        Km = g["K" + k].copy()
        Km[0, 0] *= 1.01
        Km[1, 2] += 3.0
        out.append(S.camera_row(P, Km, g["dist" + k] * rng.uniform(0.5, 1.5, len(g["dist" + k]))))
    return out


def test_table_with_one_camera_pair_per_record(g13, eng):
    g, K = g13, 64
    rng = np.random.default_rng(8)
    m = [np.arange(K)[::-1], sparse_matches(rng, K), np.arange(K), sparse_matches(rng, K, 0.7)]
    table = S.pack_table([record(g, K, m[e]) for e in range(4)], K)                # the same keypoints in every record: only the cameras differ
    a, b = fixture_pair(g)
    pairs = [[a, b], [b, a], perturbed_pair(g, 1), perturbed_pair(g, 2)]
    for undistort in (1, 0):
        per = check_table(eng, table, K, pairs, undistort, 3e-5, 3, what="camera pairs")
        one = check_table(eng, table, K, pairs[:1], undistort, 3e-5, 3, what="one pair")
        e0 = slice(0, per[0][1])
        assert np.array_equal(bits(per[1][e0]), bits(one[1][e0])) and (per[1][per[0][1]:] != one[1][one[0][1]:]).any(1).all()
        assert undistort == 0 or ((per[3][per[0][1]:] != one[3][per[0][1]:]).any(1).all() and (per[4][per[0][1]:] != one[4][per[0][1]:]).any(1).all())


# ---- e. refusals ----------------------------------------------------------------------------------------------------------------------
def refused(fn, *a, **k):
    """The call returns -73 and leaves every sentinel-filled output as it was."""
    from icepy4d_amd._lib import IcematchError
    with pytest.raises(IcematchError) as ei:
        fn(*a, **k)
    assert ei.value.rc == -73, (ei.value.rc, str(ei.value))
    assert untouched(*ei.value.outputs), str(ei.value)


def test_refusals(g13, eng):
    g = g13
    n = 70
    k0, k1, P0, P1 = g["kpts0"][:n], g["kpts1"][:n], g["P0"], g["P1"]
    c0, c1 = intrinsics(g["K0"], g["dist0"]), intrinsics(g["K1"], g["dist1"])
    nan, inf = np.nan, np.inf

    def focal(c, i, v):
        c = c.copy()
        c[i] = v
        return c

    def undistort(cam, n_arg):
        out = sentinel(eng, (n + 1, 2), np.float32)
        try:
            eng.ctx.call("im_undistort_points", p(dev(eng, k0)), n_arg, cam.ctypes.data, p(out), eng.stream_ptr())
        except Exception as e:
            e.outputs = (out,)
            raise
    refused(undistort, c0, -1)
    for i in (0, 1):
        for v in (0.0, nan, inf, -inf):
            refused(undistort, focal(c0, i, v), n)
    tri = lambda **kw: call_triangulate(eng, kw.pop("u1", k0), P0, kw.pop("u2", k1), P1, **kw)      # noqa: E731
    for ms in (0, 11, -1):
        refused(tri, max_solves=ms)
        refused(tri, max_solves=ms, cam1=c0, cam2=c1, want_und=True)
    for tol in (-1.0, nan, -1e-300):
        refused(tri, tolerance=tol)
        refused(tri, tolerance=tol, u1=k0.astype(np.float64), u2=k1.astype(np.float64))
    for i in (0, 1):
        for v in (0.0, nan, inf):
            refused(tri, cam1=focal(c0, i, v), cam2=c1, want_und=True)
            refused(tri, cam1=c0, cam2=focal(c1, i, v), want_und=True)
    refused(tri, u1=k0.astype(np.float64), u2=k1.astype(np.float64), cam1=c0, cam2=c1)      # fused undistortion of float64 points
    refused(tri, cam1=c0, want_und=True)                                                    # one camera only
    refused(tri, cam2=c1, want_und=True)
    refused(tri, u1=k0.astype(np.float64), u2=k1.astype(np.float64), want_und=True)         # float64 points with an `und` output
    refused(tri, n=-1)
    refused(tri, n=-1, cam1=c0, cam2=c1, want_und=True)
    # the table call
    K = 16
    table = S.pack_table([record(g, K, np.arange(K)), record(g, K, np.arange(K)[::-1]), record(g, K, np.arange(K))], K)
    pair = fixture_pair(g)
    tab = lambda **kw: call_table(eng, table, kw.pop("K", K), kw.pop("cams", [pair]), 1, kw.pop("tolerance", 3e-5),   # noqa: E731
                                  kw.pop("max_solves", 10), kw.pop("m_cap", 48), rows=49, **kw)
    for ms in (0, 11):
        refused(tab, max_solves=ms)
    for tol in (-1.0, nan):
        refused(tab, tolerance=tol)
    for bad_k in (0, 16385, -1):
        refused(tab, K=bad_k)
    refused(tab, cams=[pair, pair])                                                         # neither 1 nor n_records
    refused(tab, n_cams=0)
    refused(tab, cams=[pair] * 4)
    refused(tab, m_cap=-1)
    refused(tab, null_offsets=True)
    refused(tab, n_records=-1)
    refused(tab, null_outputs=True)                                                         # a capacity without outputs
    # the context is as good as before
    off, X, st, w0, w1 = tab()
    want = S.triangulate_table(table, K, [pair], 1, 3e-5, 10, 48)
    for a, b in zip((off, X, st, w0, w1), want):
        check(a, b, "after the refusals")


# ---- f. the Python level --------------------------------------------------------------------------------------------------------------
def test_python_table_with_a_camera_pair_and_an_image_per_record(g13, eng):
    from icepy4d_amd import sfm
    from test_gpu_sfm import cameras
    g = g13
    c0, c1 = cameras(g)

    def variant(c, fx, shift):
        K = c.K.copy()
        K[0, 0] *= fx
        K[0, 2] += shift
        t = c.t + 0.01 * shift
        return types.SimpleNamespace(K=K, dist=c.dist * (1.0 - 0.1 * shift), R=c.R, t=t, P=K @ np.c_[c.R, t])
    pairs = [[c0, c1], [c1, c0], [variant(c0, 1.01, 1.0), variant(c1, 0.99, 2.0)]]
    base = S.image_pattern(*FRAME)
    images = [base, np.ascontiguousarray(base[::-1]), np.ascontiguousarray(base[:, ::-1])]
    rng = np.random.default_rng(4)
    K = 256
    sel = [(4990, 5200), (0, 180), (5000, 5190)]
    table = S.pack_table([S.scatter_matches(rng, g["kpts0"][a:b], g["kpts1"][a:b], K) for a, b in sel], K)
    rec = sfm.triangulate_table(table, K, pairs, engine=eng, image=images, cam_id=1)
    assert rec.offsets.tolist() == [0, 210, 390, 580]
    flat = []
    for e, (a, b) in enumerate(sel):
        t = sfm.Triangulate(pairs[e], [g["kpts0"][a:b], g["kpts1"][a:b]], engine=eng)
        X = t.triangulate_two_views(compute_colors=True, image=images[e], cam_id=1)
        assert np.array_equal(bits(rec.points3d[e]), bits(X)) and np.array_equal(rec.status[e], t.status), e
        assert np.array_equal(bits(rec.colors[e]), bits(t.colors)) and t.colors.shape == (b - a, 3), e
        flat.append((X, t.colors))
    # the pairs and the images matter: record 0 with record 2's cameras, or with record 1's image, is another result
    t = sfm.Triangulate(pairs[2], [g["kpts0"][4990:5200], g["kpts1"][4990:5200]], engine=eng)
    assert (t.triangulate_two_views(compute_colors=True, image=images[1], cam_id=1) != flat[0][0]).any(1).all()
    assert (t.colors != flat[0][1]).any()
