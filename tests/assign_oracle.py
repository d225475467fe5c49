"""Oracles of the assignment stage (`sigmoid_log_double_softmax` + `filter_matches`): plain numpy / torch, no library import.

Two references, for two kinds of claim:

* `ref64`: the float64 log-assignment of the float32 inputs. It says what the stage SHOULD compute; the normalisers (which go through
  `fexp` / `logf` on the device) are held against it within a tolerance, and `explain` holds the final matches against it end to end.
* `restate`: once the normalisers are known, the score is adds and subtracts with a fixed association (`assign_score`,
  csrc/assign_sweep.h), which numpy's float32 reproduces bit for bit. Everything behind the normalisers - row arg-max (first column
  among equals), column arg-max (lowest row among equals), the 64-bit column keys, the mutual check and the scatter - is then a
  matter of identity, not of tolerance.
"""
import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ column keys (csrc/common.h)
def f2ord(x):
    """Order-preserving float32 -> uint32 (`f2ord`): negative floats have all bits flipped, the others their sign bit set."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ord2f(u):
    u = np.ascontiguousarray(u, dtype=np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)


def make_keys(val, row):
    """f2ord(score) << 32 | ~row: a larger key is a larger score or, at equal score bits, a lower row."""
    return (f2ord(val).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(row).astype(np.uint64))


def decode_keys(keys):
    keys = np.asarray(keys, dtype=np.uint64)
    val = ord2f((keys >> np.uint64(32)).astype(np.uint32))
    row = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    return val, row


# ------------------------------------------------------------------------------------------------ float64 reference
def _logsumexp64(x, axis):
    mx = x.max(axis=axis, keepdims=True)
    return np.squeeze(mx, axis) + np.log(np.exp(x - mx).sum(axis=axis))


def logsigmoid64(z):
    z = np.asarray(z, dtype=np.float64)
    return np.minimum(z, 0.0) - np.log1p(np.exp(-np.abs(z)))


def ref64(sim, z0, z1):
    """Float64 log-assignment of float32 inputs: row log_softmax + column log_softmax + logsigmoid certainties, with the row and
    column max and logsumexp it went through."""
    x = np.asarray(sim, dtype=np.float64)
    rlse, clse = _logsumexp64(x, 1), _logsumexp64(x, 0)
    l0, l1 = logsigmoid64(z0), logsigmoid64(z1)
    scores = ((x - rlse[:, None]) + (x - clse[None, :])) + (l0[:, None] + l1[None, :])
    return dict(scores=scores, rmax=x.max(1), rlse=rlse, cmax=x.max(0), clse=clse, lz0=l0, lz1=l1)


def normalisers_from_ref64(r):
    """The float32 normalisers a perfect device would hold: (max, lse - max) and the certainties, rounded once."""
    f = np.float32
    rmax, cmax = r["rmax"].astype(f), r["cmax"].astype(f)
    return dict(rmax=rmax, rlog=(r["rlse"] - rmax.astype(np.float64)).astype(f), cmax=cmax,
                clog=(r["clse"] - cmax.astype(np.float64)).astype(f), lz0=r["lz0"].astype(f), lz1=r["lz1"].astype(f))


# ------------------------------------------------------------------------------------------------ float32 restatement
def restate_scores(sim, nz, mode):
    """The score matrix exactly as `assign_score` associates it, in float32:
    mode 0: (((x - rm) - rl) + ((x - cm) - cl)) + (l0 + l1);  mode 1: ((x + u) + v) - norm."""
    x = np.ascontiguousarray(sim, dtype=np.float32)
    f = lambda a: np.asarray(a, dtype=np.float32)
    if mode == 0:
        rm, rl, cm, cl = f(nz["rmax"])[:, None], f(nz["rlog"])[:, None], f(nz["cmax"])[None, :], f(nz["clog"])[None, :]
        s = (x - rm) - rl
        s += (x - cm) - cl
        s += f(nz["lz0"])[:, None] + f(nz["lz1"])[None, :]
    else:
        s = (x + f(nz["u"])[:, None]) + f(nz["v"])[None, :]
        s -= np.float32(nz["norm"])
    assert s.dtype == np.float32
    return s


def restate(sim, nz, mode):
    """Scores, row arg-max (first column among equal values), column arg-max (lowest row among equal values) and the column keys."""
    s = restate_scores(sim, nz, mode)
    ridx = s.argmax(1)                       # numpy: first occurrence
    cidx = s.argmax(0)
    rval = s[np.arange(s.shape[0]), ridx]
    cval = s[cidx, np.arange(s.shape[1])]
    return dict(scores=s, ridx=ridx.astype(np.int64), rval=rval, cidx=cidx.astype(np.int64), cval=cval, keys=make_keys(cval, cidx))


def filter_matches(ridx, rval, cidx, th, ms_dev=None):
    """`filter_matches` as oracle/ref_cpu.mutual_nn_filter, on the arg-maxima. The matching score is exp(rval); with `ms_dev` (the
    device's own matching_scores0) the threshold decision `ms > th` is taken on that value."""
    ridx, cidx = np.asarray(ridx, dtype=np.int64), np.asarray(cidx, dtype=np.int64)
    m, n = len(ridx), len(cidx)
    mutual0 = cidx[ridx] == np.arange(m)
    mutual1 = ridx[cidx] == np.arange(n)
    ms0 = np.where(mutual0, np.exp(np.asarray(rval, dtype=np.float64)), 0.0)
    dec = ms0 if ms_dev is None else np.asarray(ms_dev)
    valid0 = mutual0 & (dec > (np.float32(th) if ms_dev is not None else th))
    valid1 = mutual1 & valid0[cidx]
    ms1 = np.where(mutual1, ms0[cidx], 0.0)
    return dict(m0=np.where(valid0, ridx, -1), m1=np.where(valid1, cidx, -1), ms0=ms0, ms1=ms1, mutual0=mutual0, mutual1=mutual1)


def ulp_distance(a, b):
    """Distance of two float32 arrays in units in the last place (same sign assumed: matching scores are >= 0)."""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


# ------------------------------------------------------------------------------------------------ end to end against float64
def explain(ridx, cidx, m0, m1, r64, th, tol):
    """Holds a result (arg-maxima `ridx` / `cidx` and final matches `m0` / `m1`) against the float64 reference `r64` end to end.

    Every difference is one of three decisions, and each is explained only by its own float64 margin:
      * a row whose arg-max differs: explained if score64[i, reference's best] - score64[i, chosen] <= tol;
      * a column whose arg-max differs: the same, down the column;
      * with the arg-maxima as chosen the mutual check is integer work, so a remaining difference of the matches is a threshold
        decision: explained if |exp(score64[i, chosen]) - th| <= tol.
    Anything else is unexplained. Returns the explained rows / columns / threshold rows and the unexplained items."""
    s = r64["scores"]
    m, n = s.shape
    ridx, cidx = np.asarray(ridx, dtype=np.int64), np.asarray(cidx, dtype=np.int64)
    ref_r, ref_c = s.argmax(1), s.argmax(0)
    ar, ac = np.arange(m), np.arange(n)
    unexplained, rows, cols, thr = [], [], [], []
    for i in np.nonzero(ridx != ref_r)[0]:
        gap = s[i, ref_r[i]] - s[i, ridx[i]]
        (rows if gap <= tol else unexplained).append(("row", int(i), int(ridx[i]), int(ref_r[i]), float(gap)))
    for j in np.nonzero(cidx != ref_c)[0]:
        gap = s[ref_c[j], j] - s[cidx[j], j]
        (cols if gap <= tol else unexplained).append(("col", int(j), int(cidx[j]), int(ref_c[j]), float(gap)))
    # the reference's filter on the result's own arg-maxima: only the threshold decisions are left to differ
    f = filter_matches(ridx, s[ar, ridx], cidx, th)
    for i in np.nonzero(np.asarray(m0) != f["m0"])[0]:
        d = abs(f["ms0"][i] - th)
        ok = f["mutual0"][i] and d <= tol and {int(m0[i]), int(f["m0"][i])} == {-1, int(ridx[i])}
        (thr if ok else unexplained).append(("m0", int(i), int(m0[i]), int(f["m0"][i]), float(d)))
    for j in np.nonzero(np.asarray(m1) != f["m1"])[0]:
        i = cidx[j]
        d = abs(f["ms0"][i] - th)
        ok = f["mutual1"][j] and d <= tol and {int(m1[j]), int(f["m1"][j])} == {-1, int(i)}
        if not ok:
            unexplained.append(("m1", int(j), int(m1[j]), int(f["m1"][j]), float(d)))
    # and the reference's own matches, for the caller that wants the plain comparison
    g = filter_matches(ref_r, s[ar, ref_r], ref_c, th)
    return dict(rows=rows, cols=cols, thr=thr, unexplained=unexplained, ref_m0=g["m0"], ref_m1=g["m1"])


def decisions_within(r64, th, tol):
    """How many decisions of the REFERENCE itself lie inside `tol`: rows / columns whose best and second-best float64 scores are closer
    than tol, and mutual rows with |ms - th| <= tol. (Indices, so that a caller can exempt what it planted.)"""
    s = r64["scores"]
    m, n = s.shape

    def close(a, axis):
        if a.shape[axis] < 2:
            return np.zeros(a.shape[1 - axis], dtype=bool)
        top = np.partition(a, a.shape[axis] - 2, axis=axis)
        top = np.take(top, [a.shape[axis] - 2, a.shape[axis] - 1], axis=axis)
        return (np.take(top, 1, axis=axis) - np.take(top, 0, axis=axis)) <= tol
    rows, cols = np.nonzero(close(s, 1))[0], np.nonzero(close(s, 0))[0]
    ref_r, ref_c = s.argmax(1), s.argmax(0)
    f = filter_matches(ref_r, s[np.arange(m), ref_r], ref_c, th)
    thr = np.nonzero(f["mutual0"] & (np.abs(f["ms0"] - th) <= tol))[0]
    return rows, cols, thr


# ------------------------------------------------------------------------------------------------ yardsticks
def yardsticks(sim, z0, z1, r64=None):
    """What plain float32 arithmetic loses on these inputs, measured against float64 (never against the kernel):
    tol = 4 x max |oracle float32 scores - ref64|, tol_lse = 4 x max |torch float32 logsumexp - float64 logsumexp|. The factor 4 is
    the margin the suite gives plain float32 arithmetic elsewhere (test_flash_attn_large_dynamic_range): the sweeps sum in another
    order, and `fexp` is good to 2^-22 rather than half an ulp."""
    from oracle import ref_cpu
    r64 = ref64(sim, z0, z1) if r64 is None else r64
    t = torch.from_numpy(np.ascontiguousarray(sim, dtype=np.float32))
    tz0 = torch.from_numpy(np.asarray(z0, dtype=np.float32)).reshape(1, -1, 1)
    tz1 = torch.from_numpy(np.asarray(z1, dtype=np.float32)).reshape(1, -1, 1)
    s32 = ref_cpu.double_softmax_scores(t[None], tz0, tz1)[0, :-1, :-1].numpy().astype(np.float64)
    err = float(np.abs(s32 - r64["scores"]).max())
    lr = torch.logsumexp(t, 1).numpy().astype(np.float64)
    lc = torch.logsumexp(t.t().contiguous(), 1).numpy().astype(np.float64)
    err_lse = float(max(np.abs(lr - r64["rlse"]).max(), np.abs(lc - r64["clse"]).max()))
    return dict(tol=4.0 * err, tol_lse=4.0 * err_lse, err32=err, err32_lse=err_lse)
