"""Velocity fields on the device (csrc/binned.hip, csrc/scan.h) at every boundary between two code paths: the four median paths by
cell size (0-8 points: eight lanes, 9-64: one wave, 65-4096: a block over LDS, more: a block over global memory), the grid stride of
each median kernel, the second level of the scans (more than 256 blocks of 256 items), the three modes of scipy's rightmost-edge
rounding, empty point sets at every position, and one dimension at the C entry points.

Bound: the rule of tests/test_gpu_velocity.py, unchanged. count, sum, mean, std, median and every table column bit for bit (any NaN equals
any NaN), min and max with == plus an equal NaN mask. The expectation is `scipy.stats.binned_statistic_dd` wherever scipy accepts the
input, else the sequential restatement (tests/binned_oracle.py). Every test prints the sizes / item counts that show which path ran and
asserts them from the reference's count."""
import os
import sys

import numpy as np
import pytest
from scipy.stats import binned_statistic_dd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import binned_oracle as B  # noqa: E402
from test_gpu_velocity import check, check_table  # noqa: E402

pytestmark = pytest.mark.gpu

GROUP, WAVE, SCAN = 8, 64, 256      # binned.hip: BIN_GROUP, IM_WAVE; scan.h: SCAN_THREADS


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


@pytest.fixture(scope="module")
def M():
    from icepy4d_amd.utils import binned_stats
    return binned_stats


@pytest.fixture(scope="module")
def T():
    from icepy4d_amd.utils import tracking_features_utils
    return tracking_features_utils


@pytest.fixture(scope="module")
def cus(eng):
    import torch
    return int(torch.cuda.get_device_properties(eng.device).multi_processor_count)


def scipy_stats(points, values, stats, edges):
    with np.errstate(all="ignore"):
        return {s: binned_statistic_dd(points, list(values), s, bins=edges).statistic for s in stats}


def blocks_of(n, t):
    return (n + t - 1) // t


# ---- value columns whose median is decided by a tie rule ------------------------------------------------------------------------
def col_distinct(rng, n):
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)


def col_ties(rng, n):
    return rng.integers(-1, 2, n).astype(np.float64)


def col_zero_run(rng, n):
    """Two thirds signed zeros of random sign, the rest -2 or 3: both middle ranks lie inside the zero run."""
    nz = -(-2 * n // 3)
    v = np.concatenate([np.where(rng.random(nz) < 0.5, 0.0, -0.0), rng.choice([-2.0, 3.0], n - nz)])
    return v[rng.permutation(n)]


def col_nan(rng, n, k):
    """k NaNs among distinct finite values."""
    v = col_distinct(rng, n)
    v[rng.choice(n, min(k, n), replace=False)] = np.nan
    return v


def col_inf(rng, n, both_halves):
    if both_halves:                                   # n // 2 times -inf, the rest +inf: (-inf + inf) / 2 for an even n
        v = np.concatenate([np.full(n // 2, -np.inf), np.full(n - n // 2, np.inf)])
        return v[rng.permutation(n)]
    v = col_distinct(rng, n)
    k = n // 2
    v[rng.choice(n, k, replace=False)] = rng.choice([-np.inf, np.inf], k)
    return v


def cell_columns(rng, n, kinds, row=0):
    f = {"distinct": lambda: col_distinct(rng, n), "ties": lambda: col_ties(rng, n), "zeros": lambda: col_zero_run(rng, n),
         "nan_half": lambda: col_nan(rng, n, n // 2), "nan_most": lambda: col_nan(rng, n, n // 2 + 1),
         "inf": lambda: col_inf(rng, n, row == 1)}
    return np.stack([f[k]() for k in kinds]) if n else np.zeros((len(kinds), 0))


def cells_in_a_row(rng, sizes, kinds, rows=1):
    """A grid of len(sizes) x rows cells; cell (c, row) holds exactly sizes[c] points, all points shuffled together."""
    p, v = [], []
    for row in range(rows):
        for c, n in enumerate(sizes):
            p.append(np.stack([c + rng.uniform(0.1, 0.9, n), row + rng.uniform(0.1, 0.9, n)], 1))
            v.append(cell_columns(rng, n, kinds, row))
    p, v = np.concatenate(p), np.concatenate(v, 1)
    order = rng.permutation(len(p))
    return p[order], v[:, order], [np.arange(len(sizes) + 1.0), np.arange(rows + 1.0)]


# ---- 1. the cell-size ladder ----------------------------------------------------------------------------------------------------
LADDER = list(range(12)) + [15, 16, 17, 31, 32, 33] + list(range(62, 68)) + [127, 128, 129, 255, 256, 257, 258, 511, 512, 513]
LADDER_KINDS = ("distinct", "ties", "zeros", "nan_half", "nan_most", "inf")


def ladder_case():
    return cells_in_a_row(np.random.default_rng(101), LADDER, LADDER_KINDS, rows=2)


def test_cell_size_ladder(eng, M):
    p, v, edges = ladder_case()
    assert len(p) == 7086 and len(v) == 6
    ref = scipy_stats(p, v, B.STATS, edges)
    out = M.binned_statistics(p, v, B.STATS, edges, engine=eng)
    sizes = np.array(LADDER, np.float64)
    print(f"ladder: {len(p)} points, V = {len(v)}, cell sizes {LADDER}")
    for row in range(2):
        assert np.array_equal(ref["count"][0, :, row], sizes) and np.array_equal(out["count"][0, 0, :, row], sizes)
    for s in B.STATS:
        check(s, out[s][0], ref[s], "ladder")
    med = ref["median"]                               # the reference itself reaches the cases the columns were built for
    big = sizes >= 3
    assert (med[2][big] == 0).all() and np.signbit(med[2][big]).any() and not np.signbit(med[2][big]).all()
    assert np.isnan(med[4][sizes >= 1]).all() and np.isfinite(med[3][(sizes % 2 == 1), :]).all()
    assert np.isnan(ref["std"][5][sizes >= 2]).all() and np.isinf(ref["sum"][5]).any()


# ---- 2. the grid stride of the three median kernels -------------------------------------------------------------------------------
def lanes_case(cus):
    rng = np.random.default_rng(102)
    V, n1 = 3, 60
    n0 = max(3000, blocks_of(cus * 64 * 32 + 1, V * n1) + 1)
    n = 400_000
    p = np.stack([rng.uniform(-1.0, n0 - 1.0, n), rng.uniform(-0.5, n1 + 0.5, n)], 1)      # the last column of cells is planted below
    planted = [(8, 9, 0, 1, 7, 9, 8, 10, 2, 64, 65, 3)[j % 12] for j in range(n1)]
    hp = [np.stack([n0 - 1 + rng.uniform(0.1, 0.9, k), j + rng.uniform(0.1, 0.9, k)], 1) for j, k in enumerate(planted)]
    p = np.concatenate([p] + hp)
    order = rng.permutation(len(p))
    p = p[order]
    v = np.stack([col_distinct(rng, len(p)), col_ties(rng, len(p)), np.where(rng.random(len(p)) < 0.5, 0.0, -0.0)])
    return p, v, [np.arange(n0 + 1.0), np.arange(n1 + 1.0)], planted


def test_eight_lane_kernel_strides_over_the_grid(eng, M, cus):
    p, v, edges, planted = lanes_case(cus)
    stats = ("median", "count")
    ref = scipy_stats(p, v, stats, edges)
    out = M.binned_statistics(p, v, stats, edges, engine=eng)
    items = ref["count"][0].size * len(v)
    groups = min(blocks_of(items, 256 // GROUP), cus * 64) * (256 // GROUP)
    print(f"8 lanes: {cus} CUs, {items} items over {groups} groups of {GROUP} lanes ({groups // 32} blocks), last cells hold {planted[:12]}, "
          f"largest random cell {int(ref['count'][0][:-1].max())}")
    assert items > groups
    assert np.array_equal(ref["count"][0][-1], np.array(planted, np.float64))
    for s in stats:
        check(s, out[s][0], ref[s], "8 lanes")


def wave_case(cus):
    rng = np.random.default_rng(103)
    V = 16
    n_cells = blocks_of(cus * 32 * 4 + 1, V) + 59
    sizes = rng.integers(9, 13, n_cells)
    some = rng.choice(n_cells, n_cells // 8, replace=False)
    sizes[some] = rng.integers(13, 65, len(some))
    sizes[[0, 1, 2, 3, n_cells // 2, n_cells - 4, n_cells - 3, n_cells - 2, n_cells - 1]] = [9, 64, 63, 10, 64, 9, 64, 63, 9]
    kinds = ("distinct", "ties", "zeros", "nan_half") * 4
    return cells_in_a_row(rng, sizes.tolist(), kinds) + (sizes,)


def test_wave_kernel_strides_over_the_grid(eng, M, cus):
    p, v, edges, sizes = wave_case(cus)
    stats = ("median", "count")
    ref = scipy_stats(p, v, stats, edges)
    out = M.binned_statistics(p, v, stats, edges, engine=eng)
    items = len(sizes) * len(v)
    waves = min(blocks_of((len(p) // (GROUP + 1)) * len(v), 4), cus * 32) * 4
    print(f"wave: {cus} CUs, {len(p)} points, {len(sizes)} cells of {sizes.min()}..{sizes.max()} points x {len(v)} columns = {items} items over "
          f"{waves} waves ({waves // 4} blocks); cells of 9: {int((sizes == 9).sum())}, of 64: {int((sizes == 64).sum())}")
    assert items > waves and sizes.min() == GROUP + 1 and sizes.max() == WAVE
    assert np.array_equal(ref["count"][0][:, 0], sizes.astype(np.float64))
    for s in stats:
        check(s, out[s][0], ref[s], "wave")


def block_case(cus, cap):
    rng = np.random.default_rng(104)
    V = 64
    n_cells = blocks_of(2 * cus * 8 + 1, V) + 5                 # more than two items for some blocks
    sizes = rng.integers(65, 301, n_cells)
    sizes[:4] = [65, 66, 300, 67]
    sizes[rng.choice(np.arange(4, n_cells), 2, replace=False)] = [cap + 1, 5000]
    sizes = sizes[rng.permutation(n_cells)]
    kinds = ("zeros", "nan_half", "ties", "distinct", "distinct") * 13
    return cells_in_a_row(rng, sizes.tolist(), kinds[:V]) + (sizes,)


def test_block_kernel_takes_several_items_per_block(eng, M, cus):
    """Three items for some blocks, in every order of staged and unstaged: the second and third item reuse the keys, the histogram, `next`
    and `pos` in LDS. What this can and cannot show: a wrong reuse (a stale histogram or `next`, keys of the previous cell) changes the
    medians and fails here. The barrier at the top of the item loop only orders thread 0's reset of `next` for the new item behind the
    other waves' read of it for the old one, and only thread 0's copy reaches the output, so a run without that barrier gives the same
    medians unless the scheduler delays a wave by a whole staging loop: no test can rely on that."""
    cap = M.lds_cell_capacity()
    p, v, edges, sizes = block_case(cus, cap)
    stats = ("median", "count")
    ref = scipy_stats(p, v, stats, edges)
    out = M.binned_statistics(p, v, stats, edges, engine=eng)
    n_cells, V = len(sizes), len(v)
    items = n_cells * V
    blocks = min((len(p) // (WAVE + 1)) * V, cus * 8)
    staged = sizes <= cap                                        # item it is cell it % n_cells: every cell is listed, in cell order
    runs = ["".join("s" if staged[it % n_cells] else "u" for it in range(b, items, blocks)) for b in range(blocks)]
    print(f"block: {cus} CUs, {len(p)} points, {n_cells} cells of {sizes.min()}..{sizes.max()} points x {V} columns = {items} items over {blocks} "
          f"blocks, up to {max(map(len, runs))} items per block; staged (s) / unstaged (u) sequences met: {sorted(set(runs))}")
    assert items > 2 * blocks and sizes.min() == WAVE + 1 and (sizes > cap).sum() == 2
    assert any("sus" in r for r in runs) and any(r.startswith("us") for r in runs)
    assert np.array_equal(ref["count"][0][:, 0], sizes.astype(np.float64))
    even = sizes % 2 == 0
    assert np.isnan(ref["median"][1][even]).all() and (ref["median"][0] == 0).all()      # the NaN key as the upper middle; the zero run
    for s in stats:
        check(s, out[s][0], ref[s], "block")


# ---- 3. scans across their second level -------------------------------------------------------------------------------------------
def scan_cells_case(n0, n1=1, sets=1):
    """About 1.5 points per cell (12 for the small grids); by hand: 9 .. 70 points in the first and last cell of every set and in the
    cells either side of every multiple of 256 x 256 segments, so that listed cells lie on both sides of a carry."""
    rng = np.random.default_rng(1000 + n0 * n1 + sets)
    C = n0 * n1
    per_set = min(50_000, 12 * C) if sets > 1 else min(100_000, 12 * C)
    hand = {}
    for seg in sorted({0, C - 1, sets * C - 1} | {m + d for m in range(SCAN * SCAN, sets * C, SCAN * SCAN) for d in (-1, 0)}):
        hand[seg] = (9, 70, 33, 12, 65, 10, 64, 66)[len(hand) % 8]
    p, offs = [], [0]
    for e in range(sets):
        q = np.stack([rng.uniform(-0.01 * n0, 1.01 * n0, per_set), rng.uniform(-0.05, n1 + 0.05, per_set)], 1)
        for seg, k in hand.items():
            if seg // C == e:
                c = seg % C
                q = np.concatenate([q, np.stack([c // n1 + rng.uniform(0.1, 0.9, k), c % n1 + rng.uniform(0.1, 0.9, k)], 1)])
        p.append(q[rng.permutation(len(q))])
        offs.append(offs[-1] + len(q))
    p = np.concatenate(p)
    return p, col_distinct(rng, len(p)), [np.arange(n0 + 1.0), np.arange(n1 + 1.0)], np.array(offs, np.int64), hand


@pytest.mark.parametrize("n0,n1,sets", [(255, 1, 1), (256, 1, 1), (257, 1, 1), (65535, 1, 1), (65536, 1, 1), (65537, 1, 1), (65537, 2, 2)])
def test_cell_scans_across_their_second_level(eng, M, n0, n1, sets):
    """CountScan and LargeScan both scan one item per segment (sets x cells), whether or not the cell is listed: their block sums pass 256
    blocks, and need the carry of the top level, as soon as there are more than 65536 segments. With the carry ignored every segment past
    the first 65536 gets a start that is short by the points before it, so the hand-made cells behind each multiple of 65536 (which the
    wave and block kernels find through LargeScan's list) show it without 65536 listed cells being needed."""
    p, v, edges, offs, hand = scan_cells_case(n0, n1, sets)
    stats = ("median", "count", "sum")
    ref = B.binned_statistics_seq(p, v, stats, edges, offs)
    out = M.binned_statistics(p, v, stats, edges, offs, engine=eng)
    n_seg = sets * n0 * n1
    cnt = ref["count"].reshape(-1)
    listed = np.flatnonzero(cnt > GROUP)
    print(f"cell scans: {n_seg} segments = {blocks_of(n_seg, SCAN)} scan blocks ({blocks_of(blocks_of(n_seg, SCAN), SCAN)} rounds of the top level), "
          f"{len(p)} points, {len(listed)} listed cells, the first {listed[:3].tolist()} and the last {listed[-3:].tolist()}, by hand {hand}")
    for seg, k in hand.items():
        assert cnt[seg] >= k and cnt[seg] > GROUP
    assert (blocks_of(n_seg, SCAN) > SCAN) == (n_seg > SCAN * SCAN)
    for s in stats:
        assert out[s].shape == ref[s].shape
        check(s, out[s], ref[s], f"{n0}x{n1}x{sets}")


def tracked_case(M_rows, single_ids=False):
    """Four epochs (days 0, 3, 3, 7: dt = 0 between the two middle ones) with exactly M_rows rows in all. Otherwise M_rows (id, epoch)
    pairs drawn from twice as many; `single_ids`: every id in one epoch only, so that there are as many ids as rows."""
    rng = np.random.default_rng(2000 + M_rows + single_ids)
    days = np.array([0, 3, 3, 7], np.int64)
    n_ids = M_rows if single_ids else (M_rows + 1) // 2
    if single_ids:
        pid, pep = np.arange(n_ids), rng.integers(0, 4, n_ids)
    else:
        pick = rng.choice(n_ids * 4, M_rows, replace=False)
        pid, pep = pick // 4, pick % 4
    names = np.sort(rng.choice(8 * n_ids, n_ids, replace=False)).astype(np.int64)
    base = np.stack([rng.uniform(-60, 80, n_ids), rng.uniform(-50, 90, n_ids), rng.uniform(80, 140, n_ids)], 1)
    base[-3:] = base[:3] = [0.0, 0.0, 100.0]                      # the first and the last ids are inside the volume
    vel = np.stack([rng.normal(0.1, 0.08, n_ids), rng.normal(-0.05, 0.1, n_ids), rng.normal(0, 0.02, n_ids)], 1)
    ids, xyz = [], []
    for e, d in enumerate(days):
        here = np.flatnonzero(pep == e)
        here = pid[here][rng.permutation(len(here))]
        ids.append(names[here])
        xyz.append(base[here] + vel[here] * d + rng.normal(0, 0.01, (len(here), 3)))
    assert sum(len(i) for i in ids) == M_rows
    return ids, xyz, days, len(np.unique(pid))


TRACKED = [(255, False), (256, False), (257, False), (65535, False), (65536, False), (65537, False), (65536, True), (65537, True)]


@pytest.mark.parametrize("M_rows,single_ids", TRACKED)
def test_tracked_scans_across_their_second_level(eng, T, M_rows, single_ids):
    """IdScan scans the M rows; TrackedScan and KeptRowScan scan M items too but count only the ids, so their carry matters once there
    are more than 65536 ids: the single-epoch cases (every row an id of its own, min_tracked_epoches = 1, no dt filter)."""
    ids, xyz, days, n_ids = tracked_case(M_rows, single_ids)
    kw = dict(min_tracked_epoches=1, volume=B.TRK_VOLUME) if single_ids else \
        dict(min_tracked_epoches=2, volume=B.TRK_VOLUME, min_dt=1, vx_lims=[0, 0.2])
    t = T.tracked_points_table(ids, xyz, days, engine=eng, **kw)
    ref, series = B.tracked_table_seq(ids, xyz, days, **kw)
    dt0 = sum(1 for s in series.values() if days[s[0]] == days[s[-1]])
    print(f"tracked scans: {M_rows} rows = {blocks_of(M_rows, SCAN)} scan blocks, {n_ids} ids, {len(series)} tracked (with dt = 0: {dt0}), "
          f"{len(ref['fid'])} rows kept, fid {ref['fid'][:1].tolist()} .. {ref['fid'][-1:].tolist()}")
    assert len(np.unique(np.concatenate(ids))) == n_ids and len(ref["fid"]) > 0 and dt0 > 0 and (ref["dt"] == 0).any() == single_ids
    if single_ids:
        assert n_ids == M_rows and ref["fid"][-1] == max(i.max() for i in ids if len(i)) and ref["index"][-1] == len(series) - 1
    check_table(t, ref, series)


# ---- 4. the rightmost-edge rule in np.around's three modes ------------------------------------------------------------------------
@pytest.mark.parametrize("w,decimal", [(1e-5, 11), (2e6, 0), (5e7, -1), (3e9, -3)])
def test_rightmost_edge_in_every_rounding_mode(eng, M, w, decimal):
    e0 = (0.25 if w < 1 else 1e9) + np.arange(6) * w
    assert int(-np.log10(np.diff(e0).min())) + 6 == decimal       # scipy's `decimal`, np.around's mode by its sign
    edges = [e0, np.array([0.0, 1.0])]
    step, last = 10.0 ** -decimal, e0[-1]
    x = np.array([last, np.nextafter(last, np.inf), last + 0.3 * step, last + 0.49 * step, last + 0.51 * step, last + 2 * step,
                  np.nextafter(last, -np.inf), e0[0], np.nextafter(e0[0], -np.inf), e0[2]])
    cells = B.bin_numbers(np.stack([x, np.full(len(x), 0.5)], 1), edges)
    print(f"w = {w:g}: decimal {decimal}, step {step:g}, cells of the ten points {cells.tolist()}")
    assert cells.tolist() == [4, 4, 4, 4, -1, -1, 4, 0, -1, 2]
    # the ten points against scipy; then with NaN and +-inf coordinates in either dimension against the restatement
    extra = np.array([[np.nan, 0.5], [np.inf, 0.5], [-np.inf, 0.5], [e0[1], np.nan], [e0[1], np.inf], [last, -np.inf], [last, 1.0], [e0[3], 0.0]])
    p = np.concatenate([np.stack([x, np.full(len(x), 0.5)], 1), extra])
    v = 2.0 ** np.arange(len(p))                                  # any sum names its points
    stats = ("count", "sum")
    ref = scipy_stats(p[:len(x)], [v[:len(x)]], stats, edges)
    out = M.binned_statistics(p[:len(x)], v[:len(x)], stats, edges, engine=eng)
    for s in stats:
        check(s, out[s][0], ref[s], f"w={w:g}")
    assert out["count"][0, 0, :, 0].tolist() == [1, 0, 1, 0, 5] and out["sum"][0, 0, 4, 0] == 1 + 2 + 4 + 8 + 64
    ref = B.binned_statistics_seq(p, v, stats, edges)
    out = M.binned_statistics(p, v, stats, edges, engine=eng)
    for s in stats:
        check(s, out[s], ref[s], f"w={w:g} with NaN and inf")
    assert B.bin_numbers(extra, edges).tolist() == [-1, -1, -1, -1, -1, -1, 4, 3]
    assert out["count"][0, 0, :, 0].tolist() == [1, 0, 1, 1, 6]


# ---- 5. empty point sets at the front, at the back and in runs --------------------------------------------------------------------
def test_empty_point_sets_everywhere(eng, M):
    rng = np.random.default_rng(105)
    sizes = [0, 0, 300, 0, 1, 65, 0]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    edges = [np.array([0.0, 1.0, 2.0, 3.0, 4.0]), np.array([0.0, 1.5, 2.0, 3.0])]
    p = np.stack([rng.uniform(-0.2, 4.2, 366), rng.uniform(-0.2, 3.2, 366)], 1)
    p[300] = [3.5, 2.5]                                           # the set of one point: the last cell
    p[301:] = np.stack([rng.uniform(1.1, 1.9, 65), rng.uniform(1.6, 1.9, 65)], 1)      # the set of 65: one cell, the block kernel
    v = np.stack([col_distinct(rng, 366), col_ties(rng, 366), col_zero_run(rng, 366), col_nan(rng, 366, 30)])
    ref = B.binned_statistics_seq(p, v, B.STATS, edges, offs)
    out = M.binned_statistics(p, v, B.STATS, edges, offs, engine=eng)
    per_set = ref["count"][:, 0].sum(axis=(1, 2)).astype(int).tolist()
    print(f"sets of {sizes} points: inside {per_set}, cells of the 65-point set {ref['count'][5, 0].astype(int).tolist()}")
    assert per_set[4:6] == [1, 65] and ref["count"][5, 0, 1, 1] == 65 and ref["count"][4, 0, 3, 2] == 1 and 200 < per_set[2] < 300
    for s in B.STATS:
        assert out[s].shape == (7, 4, 4, 3)
        check(s, out[s], ref[s], "sets")
        for e in (0, 1, 3, 6):
            fill = out[s][e]
            assert (fill == 0).all() if s in ("count", "sum") else np.isnan(fill).all(), (s, e)


# ---- 6. one dimension, at the C entry points ----------------------------------------------------------------------------------------
def test_one_dimension_at_the_c_entry_points(eng, M):
    import torch
    from icepy4d_amd._lib import IcematchError, ptr
    rng = np.random.default_rng(106)
    e = np.cumsum(rng.uniform(0.5, 1.5, 12))
    N, V, C = 900, 2, len(e) - 1
    x = rng.uniform(e[0] - 0.5, e[-1] + 0.5, N)
    x[:6] = [e[-1], np.nextafter(e[-1], np.inf), e[-1] + 1e-9, e[0], np.nextafter(e[0], -np.inf), e[5]]
    x[6] = np.nan
    x[100:170] = rng.uniform(e[3] + 0.01, e[4] - 0.01, 70)       # a cell for the block kernel
    v = np.stack([col_distinct(rng, N), col_zero_run(rng, N)])
    decimal = int(-np.log10(np.diff(e).min())) + 6
    dev, st = eng.device, eng.stream_ptr()
    d_x, d_v, d_e = (torch.from_numpy(a).to(dev) for a in (x, v, e))
    d_offs = torch.tensor([0, N], dtype=torch.int64, device=dev)
    n_edges, scale, mode = np.array([len(e)] * 4, np.int32), np.full(4, 10.0 ** abs(decimal)), np.full(4, int(np.sign(decimal)), np.int32)
    slots = np.arange(len(B.STATS), dtype=np.int32)               # M.STATISTICS is B.STATS' order
    assert tuple(M.STATISTICS) == tuple(B.STATS)
    ref_cell = B.bin_numbers(x.reshape(-1, 1), [e])
    ref = B.binned_statistics_seq(x.reshape(-1, 1), v, B.STATS, [e])

    def cells(dims, ne=n_edges):
        key = torch.full((N,), -7, dtype=torch.int64, device=dev)
        eng.ctx.call("im_binned_cells", ptr(d_x), N, dims, ptr(d_e), ne.ctypes.data, scale.ctypes.data, mode.ctypes.data, ptr(d_offs), 1, ptr(key), st)
        return key

    def right_answer():
        key = cells(1)
        assert np.array_equal(key.cpu().numpy(), np.where(ref_cell < 0, C, ref_cell))
        skey, perm = torch.sort(key, stable=True)
        out = torch.empty((len(B.STATS), 1, V, C), dtype=torch.float64, device=dev)
        eng.ctx.call("im_binned_stats", ptr(skey), ptr(perm), N, 1, C, ptr(d_v), V, slots.ctypes.data, ptr(out), st)
        host = out.cpu().numpy()
        for k, s in enumerate(B.STATS):
            check(s, host[k], ref[s], "one dimension")

    cnt = ref["count"][0, 0].astype(int)
    print(f"one dimension: {N} points, {int((ref_cell >= 0).sum())} inside, cells of {cnt.tolist()} points")
    assert cnt[3] > WAVE and cnt.min() > GROUP and ref_cell[:7].tolist() == [C - 1, C - 1, C - 1, 0, -1, 5, -1]
    right_answer()
    for what, call in [("dims = 0", lambda: cells(0)), ("dims = 4", lambda: cells(4)),
                       ("one edge", lambda: cells(1, np.array([1], np.int32)))]:
        with pytest.raises(IcematchError) as err:
            call()
        print(f"{what}: {err.value}")
        assert err.value.rc == -72, what
    right_answer()
