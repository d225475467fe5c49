"""Numpy restatement of csrc/tm_pair.h, the arithmetic of one template-matching pair: the plan of the correlation kernel, the window rule,
the block C as the order of its float32 fused multiply-adds, the wave's argmax and sum of |C| as lane 0 sees them, the peak tail, and the
rule for windows that hold a NaN or an infinity. Bit for bit what the host build of the header and the kernels give (tests/
test_templatematch_host_cpu.py, tests/test_gpu_templatematch_edges.py); `forient` is oc_oracle.forient, which is exact already.

The fused multiply-add. Python 3.10 has no math.fma, so fma32 emulates it: the product of two float32 values has at most 48 significant
bits and is exact in float64; the accumulator is added with TwoSum, which yields the rounded sum s and the exact error e; where e != 0
the sum is moved to the neighbour with an odd last bit (rounding to odd), and the result is rounded to float32. Rounding to odd at p = 53
bits followed by rounding to nearest at q = 24 bits equals one rounding to nearest of the exact value whenever p >= q + 2 (Boldo and
Melquiond, "Emulation of FMA and correctly rounded sums: proved algorithms using rounding to odd", 2008); a float32 subnormal result has
fewer than 24 bits, which only widens the margin, and nothing here leaves the range of float64.

Zero-padded terms. The kernel multiplies zeros beyond the template's T rows and columns (up to the chunk sizes kt and kx), and the
imaginary plane's zeros are isign * 0 = -0 when isign is -1. With finite inputs such a term is fma(+-0, b, acc) = acc + (+-0): that is acc
for every acc other than -0, and acc is never -0, because a chain starts from +0, the sum of +0 and -0 is +0 in rounding to nearest, and
an exact cancellation x + (-x) gives +0. So corr_block skips them when both windows are finite. When a window holds a NaN or an infinity
the padding matters (0 * NaN is NaN), and corr_block then multiplies every term the kernel multiplies, B beyond the S x S window being 0.
"""
import numpy as np

import oc_oracle

F32, F64 = np.float32, np.float64
TM_DX, TM_MAX_THREADS, TM_LDS_FLOATS, TM_WAVE = 16, 256, 16384, 64
PLAN_FIELDS = ("R", "gy", "gx", "ks", "ny", "nx", "kt", "kx", "pitch", "brows", "threads", "lds_floats")


def fma32(a, b, c):
    """round_to_float32(a * b + c) with one rounding, elementwise; a, b, c float32 (see the module docstring)."""
    a, b, c = np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(F64) * b.astype(F64)
        c64 = c.astype(F64)
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)
        s = np.array(s, F64, ndmin=1)
        bits = s.view(np.int64)
        # the exact sum lies between s and its neighbour on e's side; of two neighbours one has an odd last bit
        odd = (e != 0) & ((bits & 1) == 0) & np.isfinite(s)
        bits += np.where((e > 0) == (s > 0), 1, -1) * odd
        return s.astype(F32).reshape(np.broadcast(a, b, c).shape)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def _up(a, b):
    return (a + b - 1) // b * b


def stage_floats(p):
    return 2 * p["brows"] * p["pitch"] + 2 * p["kt"] * p["kx"]


def plan(T, S):
    p = {"R": S - T}
    R = p["R"]
    p["gy"] = R if R < 16 else (32 if _up(R, 32) <= _up(R, 16) else 16)
    mx = (R + TM_DX - 1) // TM_DX
    p["gx"] = min(mx, TM_MAX_THREADS // p["gy"])
    p["nx"] = (mx + p["gx"] - 1) // p["gx"]
    p["gx"] = (mx + p["nx"] - 1) // p["nx"]
    p["ny"] = (R + p["gy"] - 1) // p["gy"]
    p["ks"] = max(1, min(TM_MAX_THREADS // (p["gy"] * p["gx"]), T))
    p["kx"] = min(_up(T, 16), 128)

    def set_rows(kt):
        p["kt"], p["brows"], p["pitch"] = kt, p["gy"] + kt - 1, TM_DX * p["gx"] + p["kx"] + 4

    set_rows(p["ks"])
    p["ks_first"], p["kx_first"] = p["ks"], p["kx"]                   # before the two loops: what the case list asserts against
    while stage_floats(p) > TM_LDS_FLOATS and p["ks"] > 1:
        p["ks"] //= 2
        set_rows(p["ks"])
    while stage_floats(p) > TM_LDS_FLOATS and p["kx"] > 16:
        p["kx"] -= 16
        set_rows(p["ks"])
    kt_max = p["ks"]
    for kt in range(2 * p["ks"], _up(T, p["ks"]) + 1, p["ks"]):
        set_rows(kt)
        if stage_floats(p) > TM_LDS_FLOATS:
            break
        kt_max = kt
    nchunks = (T + kt_max - 1) // kt_max
    set_rows(_up((T + nchunks - 1) // nchunks, p["ks"]))
    p["threads"] = _up(p["gy"] * p["gx"] * p["ks"], TM_WAVE)
    p["stage"] = stage_floats(p)
    p["reduce"] = p["threads"] * TM_DX if p["ks"] > 1 else 0
    p["lds_floats"] = max(p["stage"], p["reduce"])
    return p


# ---- the window of a pair ---------------------------------------------------------------------------------------------------------------
def pair_window(pair, bidx, n_b, T, S, ha, wa, hb, wb):
    """dict valid, arow, acol, brow, bcol, pu, pv, initdu, initdv of one row (u, v, initdu, initdv) of the pair table."""
    u, v, idu, idv = (F64(x) for x in pair)
    w = dict(valid=False, arow=0, acol=0, brow=0, bcol=0, pu=u, pv=v, initdu=F64(np.nan), initdv=F64(np.nan))
    if np.isnan(u):
        return w
    with np.errstate(invalid="ignore", over="ignore"):
        th, sh = (0.5 if T & 1 else 0.0), (0.5 if S & 1 else 0.0)
        acx, acy = np.rint(u) - th, np.rint(v) - th
        bcx, bcy = np.rint(u + idu) - sh, np.rint(v + idv) - sh
        w.update(pu=acx, pv=acy, initdu=bcx - acx, initdv=bcy - acy)
        if np.isnan(u + v):
            return w
        b0, b1, c0, c1 = np.trunc(bcy - S / 2.0), np.trunc(bcy + S / 2.0), np.trunc(bcx - S / 2.0), np.trunc(bcx + S / 2.0)
        a0, a1, d0, d1 = np.trunc(acy - T / 2.0), np.trunc(acy + T / 2.0), np.trunc(acx - T / 2.0), np.trunc(acx + T / 2.0)
        if not (b0 >= 0) or not (a0 >= 0) or not (c0 >= 0) or not (d0 >= 0):
            return w
        if not (b1 < hb) or not (a1 < ha) or not (c1 < wb) or not (d1 < wa):
            return w
    w.update(valid=bool(0 <= int(bidx) < n_b), brow=int(b0), bcol=int(c0), arow=int(a0), acol=int(d0))
    return w


# ---- C ----------------------------------------------------------------------------------------------------------------------------------
def term_order(p, T):
    """(group k, ty, tx, channel) of every multiply-add of one element of C, padding included, in the order of the header's definition."""
    for k in range(p["ks"]):
        for cy in range(0, T, p["kt"]):
            for cx in range(0, T, p["kx"]):
                for r in range(k, p["kt"], p["ks"]):
                    for ch in (0, 1):
                        for t in range(p["kx"]):
                            yield k, cy + r, cx + t, ch


def _fma_rows(av, b64, acc64):
    """fma32(av, b, acc) for whole arrays held as float64 (every value a float32), for operands whose non-zero magnitudes lie in
    [2^-30, 2^30]: every exact sum is then a multiple of 2^-106 below 2^128, so the float32 result is normal or zero. Rounding the
    float64 sum s to float32 differs from rounding the exact sum only when s lies exactly half way between two float32 values (any
    float32 midpoint is a float64, and rounding is monotonic, so a midpoint between the exact sum and s is s itself): the low 29 bits of s
    are then 1 followed by zeros. Only those elements take the slow path."""
    prod = av * b64
    s = prod + acc64
    tie = (s.view(np.int64) & 0x1FFFFFFF) == 0x10000000
    r = s.astype(F32)
    if tie.any():
        r[tie] = fma32(F32(av), b64[tie].astype(F32), acc64[tie].astype(F32))
    return r.astype(F64)


def corr_block(Aw, Bw, isign, p=None):
    """C [R, R] float32 of a template Aw [T, T] and a search window Bw [S, S] (complex64), all R^2 elements at once: they share one order."""
    T, S = Aw.shape[0], Bw.shape[0]
    p = p or plan(T, S)
    R = p["R"]
    a = np.stack([Aw.real, Aw.imag], -1).astype(F32)
    b = np.stack([Bw.real, Bw.imag], -1).astype(F32)
    finite = bool(np.isfinite(a).all() and np.isfinite(b).all())
    mags = np.abs(np.concatenate([a.ravel(), b.ravel()]))
    fast = finite and (mags[mags > 0].size == 0 or (mags[mags > 0].min() >= 2.0 ** -30 and mags.max() <= 2.0 ** 30))
    reach = max(_up(T, p["kt"]), _up(T, p["kx"]))
    bp = np.zeros((2, R + reach, R + reach), F64 if fast else F32)     # zero beyond the window, as staged
    bp[:, :S, :S] = np.moveaxis(b, -1, 0)
    sgn = (F32(1.0), F32(isign))
    parts = []
    acc, group = None, -1
    for k, ty, tx, ch in term_order(p, T):
        if k != group:
            if acc is not None:
                parts.append(acc.astype(F32))
            acc, group = np.zeros((R, R), F64 if fast else F32), k
        inside = ty < T and tx < T
        if finite and not inside:
            continue
        av = sgn[ch] * (a[ty, tx, ch] if inside else F32(0.0))
        if fast:
            acc = _fma_rows(F64(av), bp[ch, ty:ty + R, tx:tx + R], acc)
        else:
            acc = fma32(av, bp[ch, ty:ty + R, tx:tx + R], acc)
    parts.append(acc.astype(F32))
    with np.errstate(invalid="ignore", over="ignore"):
        s = parts[0]
        for q in parts[1:]:
            s = s + q
    return s


# ---- the wave's reduction and the peak tail ---------------------------------------------------------------------------------------------
def wave_reduce(C):
    """(best, bi, sabs) of lane 0 after the per-lane scans and the xor butterfly with strides 32 ... 1. C finite."""
    c = np.asarray(C, F32).ravel()
    n = c.size
    best, bi, sabs = np.full(TM_WAVE, -np.inf, F32), np.full(TM_WAVE, n, np.int64), np.zeros(TM_WAVE, F64)
    for lane in range(TM_WAVE):
        for e in range(lane, n, TM_WAVE):
            if c[e] > best[lane] or bi[lane] == n:
                best[lane], bi[lane] = c[e], e
            sabs[lane] = sabs[lane] + abs(F64(c[e]))
    lanes = np.arange(TM_WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        ob, oi = best[lanes ^ o], bi[lanes ^ o]
        take = (ob > best) | ((ob == best) & (oi < bi))
        best, bi = np.where(take, ob, best), np.where(take, oi, bi)
        sabs = sabs + sabs[lanes ^ o]
    return F32(best[0]), int(bi[0]), F64(sabs[0])


def np_sum_small(vals, dtype):
    """The header's np_sum_small over the values in order: numpy's pairwise summation of fewer than 129 values."""
    v = [dtype(x) for x in vals]
    n = len(v)
    zero = dtype(0)
    if n < 8:
        r = zero
        for x in v:
            r = dtype(r + x)
        return dtype(zero + r)
    r = v[:8]
    i = 8
    while i < n - n % 8:
        r = [dtype(r[j] + v[i + j]) for j in range(8)]
        i += 8
    res = dtype(dtype(dtype(r[0] + r[1]) + dtype(r[2] + r[3])) + dtype(dtype(r[4] + r[5]) + dtype(r[6] + r[7])))
    for x in v[i:]:
        res = dtype(res + x)
    return dtype(zero + res)


def peak_tail(C, bi, best, sabs, initdu, initdv):
    """[du, dv, peakCorr, meanAbsCorr] (float64) as lane 0 writes them."""
    C = np.asarray(C, F32)
    R = C.shape[0]
    out = np.full(4, np.nan)
    out[3] = F64(F32(F64(sabs) / (R * R)))
    mi, mj = divmod(int(bi), R)
    edge = min(mi, mj, R - 1 - mi, R - 1 - mj)
    if edge == 0:
        return out
    ww = min(edge, 4)
    side = 2 * ww + 1
    m = side * side
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cw = [C[mi - ww + e // side, mj - ww + e % side] for e in range(m)]
        mean_abs = F32(np_sum_small([abs(c) for c in cw], F32) / F32(m))
        cpos = [F32(0.0) if F32(c - mean_abs) < 0 else F32(c - mean_abs) for c in cw]
        tot = np_sum_small(cpos, F32)
        wkeep = R / 2.0
        cv = np_sum_small([F64(-wkeep + (mi - ww + e // side)) * F64(F32(cpos[e] / tot)) for e in range(m)], F64)
        cu = np_sum_small([F64(-wkeep + (mj - ww + e % side)) * F64(F32(cpos[e] / tot)) for e in range(m)], F64)
        out[0], out[1], out[2] = cu + F64(initdu), cv + F64(initdv), F64(best)
    return out


# ---- the whole stage --------------------------------------------------------------------------------------------------------------------
def windows(case):
    return [pair_window(case["pairs"][i], case["bidx"][i], len(case["B"]), case["T"], case["S"], *case["A"].shape, *case["B"].shape[1:])
            for i in range(len(case["pairs"]))]


def corr(case):
    """{pair index: C} of the valid pairs of a case: what im_template_match_corr writes."""
    T, S = case["T"], case["S"]
    p = plan(T, S)
    out = {}
    for i, w in enumerate(windows(case)):
        if not w["valid"]:
            continue
        Aw = case["A"][w["arow"]:w["arow"] + T, w["acol"]:w["acol"] + T]
        Bw = case["B"][int(case["bidx"][i])][w["brow"]:w["brow"] + S, w["bcol"]:w["bcol"] + S]
        out[i] = corr_block(Aw, Bw, 1.0 if case["conj_b"] else -1.0, p)
    return out


def window_finite(case, i, w):
    T, S = case["T"], case["S"]
    Aw = case["A"][w["arow"]:w["arow"] + T, w["acol"]:w["acol"] + T]
    Bw = case["B"][int(case["bidx"][i])][w["brow"]:w["brow"] + S, w["bcol"]:w["bcol"] + S]
    return bool(np.isfinite(Aw.real).all() and np.isfinite(Aw.imag).all() and np.isfinite(Bw.real).all() and np.isfinite(Bw.imag).all())


def oc(case, Cs=None):
    """[6, n_pairs] float64: pu, pv, du, dv, peakCorr, meanAbsCorr, as im_template_match_oc writes them."""
    Cs = corr(case) if Cs is None else Cs
    n = len(case["pairs"])
    out = np.full((6, n), np.nan)
    for i, w in enumerate(windows(case)):
        out[0, i], out[1, i] = w["pu"], w["pv"]
        if not w["valid"] or not window_finite(case, i, w):
            continue
        best, bi, sabs = wave_reduce(Cs[i])
        out[2:, i] = peak_tail(Cs[i], bi, best, sabs, w["initdu"], w["initdv"])
    return out


forient = oc_oracle.forient
