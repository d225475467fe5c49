"""The shapes of the assignment stage's tests, shared by test_assign_cpu.py (no GPU) and test_gpu_assign.py: the smallest ones that
reach each kernel form and each internal boundary of `launch_assign` (csrc/lg_misc.hip), with NaN padding and planted exact ties.

Which form a case runs follows from `launch_assign`'s condition alone (through `im_assign_from_sim`, which sets m_max = m, n_max = n,
one pair):
    vec  = ld % 4 == 0 and the base pointer is 16-byte aligned
    pipe = vec and ceil(m / 16) <= 384         -> lse_stats_pipe_kernel, best_sweep_pipe_kernel<0>
    vec and not pipe (m > 6144)                -> lse_stats_kernel<true>, best_sweep_kernel<0, true>
    not vec                                    -> lse_stats_kernel<false>, best_sweep_kernel<0, false>
`pvec` (16-byte stores of the strip partials) is on when n is even. torch's device allocations are 256-byte aligned, so `off`
(the view's start inside its buffer, in floats) decides the alignment: off = 1 alone selects the scalar-load form.

| (m, n, ld), off          | form     | what it reaches                                                                      |
|--------------------------|----------|--------------------------------------------------------------------------------------|
| (1, 1, 4)                | pipe     | one entry: every other quad, row and strip masked                                    |
| (16, 4, 4)               | pipe     | one full strip, one full quad, no padding                                            |
| (17, 5, 8)               | pipe     | second strip of one row, second quad of one column, padding inside the last quad     |
| (15, 1023, 1024)         | pipe     | last column of the first chunk missing, strip one row short                          |
| (33, 1024, 1024)         | pipe     | the chunk exactly full; 32-column combine blocks exactly full                        |
| (16, 1025, 1028)         | pipe     | one live column in wave 1's chunk                                                    |
| (48, 4096, 4096)         | pipe     | all four waves' chunks exactly full; scales 3 and 30                                 |
| (20, 4097, 4100)         | pipe     | second 4096 pass of wave 0 with a single live column                                 |
| (1025, 40, 40)           | pipe     | 65 strips: second trip of both column combines; scales 3 and 30                      |
| (1026, 40, 40)           | pipe     | as above with a free last row: the 65th strip alone holds a column's winner          |
| (1040, 33, 36)           | pipe     | 65 full strips, second combine block of one column                                   |
| (300, 258, 260)          | pipe     | pvec on (even n) with a partial last quad                                            |
| (300, 257, 260)          | pipe     | pvec off beside it                                                                   |
| (300, 257, 257)          | scalar   | odd ld                                                                               |
| (17, 4097, 4097)         | scalar   | second pass                                                                          |
| (1025, 33, 33)           | scalar   | second combine trip                                                                  |
| (1026, 33, 33)           | scalar   | second combine trip, the 65th strip alone holds a column's winner                    |
| (33, 1024, 1024), off 1  | scalar   | alignment alone                                                                      |
| (6145, 8, 8)             | vec      | 385 strips                                                                           |
| (6160, 1028, 1028)       | vec      | 385 full strips, wave 1's chunk with one quad                                        |
"""
from collections import namedtuple

import numpy as np

import assign_oracle as ao

Case = namedtuple("Case", "m n ld off scale form")

CASES = [
    Case(1, 1, 4, 0, 3, "pipe"), Case(16, 4, 4, 0, 3, "pipe"), Case(17, 5, 8, 0, 3, "pipe"), Case(15, 1023, 1024, 0, 3, "pipe"),
    Case(33, 1024, 1024, 0, 3, "pipe"), Case(16, 1025, 1028, 0, 3, "pipe"), Case(48, 4096, 4096, 0, 3, "pipe"),
    Case(48, 4096, 4096, 0, 30, "pipe"), Case(20, 4097, 4100, 0, 3, "pipe"), Case(1025, 40, 40, 0, 3, "pipe"),
    Case(1025, 40, 40, 0, 30, "pipe"), Case(1026, 40, 40, 0, 3, "pipe"), Case(1040, 33, 36, 0, 3, "pipe"), Case(300, 258, 260, 0, 3, "pipe"),
    Case(300, 257, 260, 0, 3, "pipe"),
    Case(300, 257, 257, 0, 3, "scalar"), Case(17, 4097, 4097, 0, 3, "scalar"), Case(1025, 33, 33, 0, 3, "scalar"),
    Case(1026, 33, 33, 0, 3, "scalar"),
    Case(33, 1024, 1024, 1, 3, "scalar"),
    Case(6145, 8, 8, 0, 3, "vec"), Case(6160, 1028, 1028, 0, 3, "vec"),
]

MAX_KPTS = 6160          # the engine every case runs on
THRESHOLD = 0.1
# duplicated columns j | j': inside a quad (one lane's registers), one lane across two quads, then across a quad, a wave quarter, a
# chunk (two waves) and the 4096-column pass
COL_PAIRS = [(1, 2), (9, 265), (3, 4), (255, 256), (1023, 1024), (4095, 4096)]
# duplicated rows i | i': inside one two-row trip of the best sweep, inside a strip, across a strip, across the 64-strip combine trip
ROW_PAIRS = [(4, 5), (2, 9), (15, 16), (1023, 1024)]


def case_id(c):
    return f"{c.m}x{c.n}-ld{c.ld}-off{c.off}-s{c.scale}-{c.form}"


def selected_form(c, base_alignment=256):
    """`launch_assign`'s choice for case c, re-derived: (form, pvec)."""
    vec = c.ld % 4 == 0 and (base_alignment + 4 * c.off) % 16 == 0
    nstrips = (c.m + 15) // 16
    return ("pipe" if vec and nstrips <= 384 else "vec" if vec else "scalar"), c.n % 2 == 0


def _row_col_scores(x, z0, z1, i, j):
    """Restated float32 score of entry (i, j) with the normalisers of ITS row and column derived in float64 and rounded once
    (what normalisers_from_ref64 gives for the whole matrix)."""
    f = np.float32
    r, c = x[i].astype(np.float64), x[:, j].astype(np.float64)
    rm, cm = f(r.max()), f(c.max())
    rl = f(r.max() + np.log(np.exp(r - r.max()).sum()) - np.float64(rm))
    cl = f(c.max() + np.log(np.exp(c - c.max()).sum()) - np.float64(cm))
    l0, l1 = f(ao.logsigmoid64(z0[i])), f(ao.logsigmoid64(z1[j]))
    v = x[i, j]
    return f(f(f(f(v - rm) - rl) + f(f(v - cm) - cl)) + f(l0 + l1))


def _tune_one_ulp(x, z0, z1, fixed, moving, zarr, zi):
    """Makes the restated score of entry `moving` exactly one float32 step above that of entry `fixed` (two entries of one row or of
    one column): coarsely through x[moving] (one float32 step of a value near 12 x scale moves the score by tens of its own steps),
    then finely through the certainty logit zarr[zi], which enters the moving entry's score alone. False where no value gives that."""
    up, dn = np.float32(np.inf), np.float32(-np.inf)

    def scores():
        return _row_col_scores(x, z0, z1, *fixed), _row_col_scores(x, z0, z1, *moving)

    def bisect(put, lo, hi):       # largest value in [lo, hi) at which moving <= fixed (the score rises with the value)
        for _ in range(80):
            mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
            if mid == lo or mid == hi:
                break
            put(mid)
            a, b = scores()
            if b > a:
                hi = mid
            else:
                lo = mid
        put(lo)
        return lo

    def put_x(v):
        x[moving] = v

    def put_z(v):
        zarr[zi] = v
    xv = bisect(put_x, np.float32(x[fixed] - 4.0), np.float32(x[fixed] + 4.0))
    z_start = np.float32(zarr[zi])
    for _ in range(8):                  # where the float32 steps of the certainty sum skip the wanted value: one step of x further down
        v = bisect(put_z, z_start, np.float32(z_start + 1.0))
        for _ in range(32):
            v = np.nextafter(v, dn)
        for _ in range(256):
            put_z(v)
            a, b = scores()
            if b == np.nextafter(a, up):
                return True
            v = np.nextafter(v, up)
        put_z(z_start)
        xv = np.nextafter(xv, dn)
        put_x(xv)
    return False


def make_case(c):
    """Inputs of case c: `buf` (flat float32 allocation, NaN outside the live m x n block: before `off`, in the padding columns
    n .. ld and in two rows after row m), the live view `sim`, `z0` / `z1`, and `plants`:
        cols: [(j, j', rows)]  column j' duplicates column j (and z1), both carry a bonus in `rows`: those rows must choose j
        rows: [(i, i', cols)]  row i' duplicates row i (and z0), both carry a bonus in `cols`: those columns must choose i
        last_row: (m - 1, c)   the last row (where no duplicate) alone wins column c, and c wins it: the last strip, however short, counts
        last_col: (r, n - 1)   the last column (where no duplicate) alone wins row r, and r wins it: the last quad, however short, counts
        near_row: (r, a, b)    the restated scores of (r, a) and (r, b), a < b, are the row's two best and (r, b) is one float32 step above
        near_col: (c, p, q)    the same down column c, rows p < q, (q, c) one step above."""
    m, n, ld, off, scale = c.m, c.n, c.ld, c.off, c.scale
    rng = np.random.default_rng(1000 * m + n + 7 * scale + off)
    x = (rng.normal(0, 1, size=(m, n)) * scale).astype(np.float32)
    z0 = rng.normal(2, 2, size=m).astype(np.float32)
    z1 = rng.normal(2, 2, size=n).astype(np.float32)
    bonus = np.float32(12 * scale)
    col_pairs = [(a, b) for a, b in COL_PAIRS if b < n]
    row_pairs = [(a, b) for a, b in ROW_PAIRS if b < m]
    dup_rows = {i for p in row_pairs for i in p}
    dup_cols = {j for p in col_pairs for j in p}
    free_rows = [i for i in range(m) if i not in dup_rows]
    free_cols = [j for j in range(n) if j not in dup_cols]
    # spread over the matrix, deterministic: the bonus rows / columns are drawn from a seeded shuffle of the free ones
    rng.shuffle(free_rows)
    rng.shuffle(free_cols)
    per = 3 if m >= 40 else 1
    last_row, last_col = m >= 8 and m - 1 in free_rows, n >= 8 and n - 1 in free_cols
    if last_row:
        free_rows.remove(m - 1)
    if last_col:
        free_cols.remove(n - 1)

    def take(pool, k):
        got = pool[:k]
        del pool[:k]
        return sorted(got)
    plants = dict(cols=[], rows=[], last_row=None, last_col=None, near_row=None, near_col=None)
    for j, j2 in col_pairs:
        x[:, j2] = x[:, j]
        z1[j2] = z1[j]
        rows = take(free_rows, per)
        if not rows and not dup_rows:
            rows = [0]
        for i in rows:
            x[i, j] += bonus
            x[i, j2] = x[i, j]
        plants["cols"].append((j, j2, rows))
    perc = 3 if n >= 40 else 1
    for i, i2 in row_pairs:
        x[i2, :] = x[i, :]
        z0[i2] = z0[i]
        cols = take(free_cols, perc)
        for j in cols:
            x[i, j] += bonus
            x[i2, j] = x[i, j]
        plants["rows"].append((i, i2, cols))
    if last_row:                        # (reserved above, before the bonus rows / columns were drawn)
        cc = take(free_cols, 1)
        if cc:
            x[m - 1, cc[0]] += bonus
            plants["last_row"] = (m - 1, cc[0])
    if last_col:
        r = take(free_rows, 1)
        if r:
            x[r[0], n - 1] += bonus
            plants["last_col"] = (r[0], n - 1)
    # near ties: a row whose two best differ by one float32 step of the restated score, and a column likewise
    if len(free_rows) >= 3 and len(free_cols) >= 3:
        r, = take(free_rows, 1)
        a, b = take(free_cols, 2)
        x[r, a] += bonus
        x[r, b] = x[r, a]
        if _tune_one_ulp(x, z0, z1, (r, a), (r, b), z1, b):
            plants["near_row"] = (r, a, b)
        p, q = take(free_rows, 2)
        cc, = take(free_cols, 1)
        x[p, cc] += bonus
        x[q, cc] = x[p, cc]
        if _tune_one_ulp(x, z0, z1, (p, cc), (q, cc), z0, q):
            plants["near_col"] = (cc, p, q)
    total = off + (m + 2) * ld + 8
    buf = np.full(total, np.nan, dtype=np.float32)
    view = buf[off:off + (m + 2) * ld].reshape(m + 2, ld)
    view[:m, :n] = x
    return dict(case=c, buf=buf, sim=x, z0=z0, z1=z1, plants=plants)


def planted_tie(plants, kind, idx, pair):
    """True if the decision of row / column `idx` (kind "row" / "col") between the two candidates `pair` is one the plants put
    inside any tolerance on purpose: the two halves of a duplicated pair (an exact tie wherever either is the best), or the planted
    one-step tie."""
    pair = tuple(sorted(int(v) for v in pair))
    if kind == "row":
        near = plants["near_row"]
        return pair in [(j, j2) for j, j2, _ in plants["cols"]] or (near is not None and idx == near[0] and pair == (near[1], near[2]))
    near = plants["near_col"]
    return pair in [(i, i2) for i, i2, _ in plants["rows"]] or (near is not None and idx == near[0] and pair == (near[1], near[2]))


_MEMO = {}


def prepared(c):
    """(inputs, float64 reference, yardsticks) of case c: computed once, shared by the tests that need them, never modified. One case
    is kept at a time (the largest holds 150 MB); the tests are parametrised case by case."""
    if c not in _MEMO:
        d = make_case(c)
        r64 = ao.ref64(d["sim"], d["z0"], d["z1"])
        y = ao.yardsticks(d["sim"], d["z0"], d["z1"], r64)
        _MEMO.clear()
        _MEMO[c] = (d, r64, y)
    return _MEMO[c]
