"""Numpy fp64 restatement of csrc/geometry.hip (fundamental / essential RANSAC hypotheses and selection, linear triangulation) and of
the tile-merge contract of csrc/tile_merge.hip (`im_merge_tile_matches`), for tests only.

The device solves each 8 x 9 system by Gauss-Jordan with full pivoting and takes singular directions from Jacobi sweeps; this oracle
uses `np.linalg.svd` throughout, so the two agree within a bound set by each problem's conditioning, which is returned next to the
result. The sampler, the Sampson test, the selection and the merge are restated exactly."""
import numpy as np

M32 = 0xFFFFFFFF
EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------ sampler
def _u32(x):
    return np.asarray(x, np.uint64) & M32


def rng_hash(seed, hyp, draw):
    """`rng_hash(seed, hyp, draw)` in wrapping uint32 arithmetic (held in uint64 and masked); broadcasts over arrays."""
    seed, hyp, draw = _u32(seed), _u32(hyp), _u32(draw)
    x = ((seed * 0x9E3779B9) & M32) ^ ((((hyp + 0x7F4A7C15) & M32) * 0x85EBCA6B) & M32) ^ ((((draw + 1) & M32) * 0xC2B2AE35) & M32)
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def sample_indices(seed, hyps, n):
    """The 8 distinct indices of each hypothesis in `hyps` under `seed`: draw k = 0, 1, ... is `rng_hash(seed, h, k) % n`, a draw equal
    to an index already taken is rejected. Vectorised over hypotheses; returns int64 [len(hyps), 8]."""
    hyps = np.atleast_1d(np.asarray(hyps, np.int64))
    H = len(hyps)
    idx = np.full((H, 8), -1, np.int64)
    filled = np.zeros(H, np.int64)
    draw = 0
    while (filled < 8).any():
        live = np.nonzero(filled < 8)[0]
        cand = (rng_hash(seed, hyps[live], draw) % np.uint64(n)).astype(np.int64)
        draw += 1
        fresh = ~(idx[live] == cand[:, None]).any(1)
        take = live[fresh]
        idx[take, filled[take]] = cand[fresh]
        filled[take] += 1
    return idx


# ------------------------------------------------------------------------------------------------ 8-point, essential projection
def _normalise(x, y):
    """Hartley normalisation of a stack of samples [H, 8] as the device forms it: centroid, mean distance, scale sqrt(2) / d."""
    cx, cy = x.mean(1, keepdims=True), y.mean(1, keepdims=True)
    d = np.sqrt((x - cx) ** 2 + (y - cy) ** 2).mean(1, keepdims=True)
    s = np.sqrt(2.0) / np.maximum(d, 1e-12)
    T = np.zeros((len(x), 3, 3))
    T[:, 0, 0] = T[:, 1, 1] = s[:, 0]
    T[:, 0, 2], T[:, 1, 2], T[:, 2, 2] = -s[:, 0] * cx[:, 0], -s[:, 0] * cy[:, 0], 1.0
    return s * (x - cx), s * (y - cy), T


def eight_point(p0, p1, idx):
    """Normalised 8-point on samples idx [H, 8] of float32 points p0, p1 [n, 2] (widened to fp64, as the device reads them).
    Returns a dict of stacks over H:
      F      [H, 3, 3] rank 2 (smallest singular value dropped), denormalised, unit Frobenius norm (sign arbitrary);
      cond   sigma8 / sigma1 of the normalised 8 x 9 system (0 for an exactly rank-deficient one);
      kappa  a first-order bound on the relative error of F from rounding: the null vector's and the rank-2 direction's sensitivity,
             amplified by the two normalising transforms;
      dup    the sample holds two identical correspondences (an exactly degenerate system);
      G      [H, 3, 3] the normalised null-vector matrix before the rank-2 step, with its singular values `sv`."""
    q0, q1 = np.asarray(p0, np.float32).astype(np.float64), np.asarray(p1, np.float32).astype(np.float64)
    a = np.concatenate([q0[idx], q1[idx]], -1)                                    # [H, 8, 4]
    dup = np.zeros(len(idx), bool)
    for i in range(8):
        for j in range(i + 1, 8):
            dup |= (a[:, i] == a[:, j]).all(-1)
    a0, b0, T0 = _normalise(a[..., 0], a[..., 1])
    a1, b1, T1 = _normalise(a[..., 2], a[..., 3])
    one = np.ones_like(a0)
    A = np.stack([a1 * a0, a1 * b0, a1, b1 * a0, b1 * b0, b1, a0, b0, one], -1)   # [H, 8, 9]
    _, sA, vt = np.linalg.svd(A, full_matrices=True)
    G = vt[:, -1].reshape(-1, 3, 3)
    u, sv, wt = np.linalg.svd(G)
    F2 = u @ (sv[:, :, None] * np.array([1.0, 1.0, 0.0])[None, :, None] * wt)
    F = np.swapaxes(T1, 1, 2) @ F2 @ T0
    nF = np.maximum(np.linalg.norm(F, axis=(1, 2)), 1e-300)
    F /= nF[:, None, None]
    cond = sA[:, 7] / sA[:, 0]
    gap2 = np.maximum(sv[:, 1] ** 2 - sv[:, 2] ** 2, 1e-300)            # the device finds the rank-2 direction from G^T G
    amp = np.linalg.norm(T0, 2, axis=(1, 2)) * np.linalg.norm(T1, 2, axis=(1, 2)) / nF    # |dF| / |F| <= amp |dG| (|G| = 1)
    kappa = (1.0 / np.maximum(cond, 1e-300) + sv[:, 0] ** 2 / gap2) * amp
    return {"F": F, "cond": cond, "kappa": kappa, "dup": dup, "G": G, "sv": sv}


def project_essential(F):
    """U diag(1, 1, 0) V^T / sqrt(2) for a stack F [H, 3, 3] (the device's E = U diag(m, m, 0) V^T once normalised); `ok` is False where
    the device gives up, s2 <= 1e-12 s1; `gap` = (s2 - s3) / s1 sets the sensitivity of the projection."""
    u, s, vt = np.linalg.svd(F)
    E = u @ (np.array([1.0, 1.0, 0.0])[None, :, None] * vt) / np.sqrt(2.0)
    ok = (s[:, 1] > 1e-12 * s[:, 0]) & (s[:, 0] > 0)
    return E, ok, (s[:, 1] - s[:, 2]) / np.maximum(s[:, 0], 1e-300)


# ------------------------------------------------------------------------------------------------ scoring and selection
def sampson_ratio(F, p0, p1, thr2):
    """num^2 / (thr2 * max(den, 1e-24)) per point for a matrix or a stack of them ([n] or [H, n]): the device counts a point as an inlier
    iff num^2 < thr2 * max(den, 1e-24), i.e. iff this ratio is below 1. Points with a ratio within ~1e-6 of 1 are ambiguous."""
    q0, q1 = np.asarray(p0, np.float32).astype(np.float64), np.asarray(p1, np.float32).astype(np.float64)
    Fs = np.asarray(F, np.float64).reshape(-1, 9)
    x0, y0, x1, y1 = q0[:, 0], q0[:, 1], q1[:, 0], q1[:, 1]
    f = [Fs[:, k, None] for k in range(9)]
    fx0 = f[0] * x0 + f[1] * y0 + f[2]
    fx1 = f[3] * x0 + f[4] * y0 + f[5]
    fx2 = f[6] * x0 + f[7] * y0 + f[8]
    ft0 = f[0] * x1 + f[3] * y1 + f[6]
    ft1 = f[1] * x1 + f[4] * y1 + f[7]
    num = x1 * fx0 + y1 * fx1 + fx2
    den = fx0 * fx0 + fx1 * fx1 + ft0 * ft0 + ft1 * ft1
    r = num * num / (thr2 * np.maximum(den, 1e-24))
    return r[0] if np.ndim(F) == 2 else r


def hypotheses(p0, p1, seed, hyps, threshold, essential=False, chunk=256):
    """Every hypothesis h in `hyps` as the device's hypothesis kernel forms it: sample, 8-point, optional essential projection, Sampson
    count. Returns a dict of stacks: idx, F (0 where invalid), valid, dup, kappa (bound on F's relative error), count (points with ratio
    < 1 - amb_tol), amb (points with |ratio - 1| <= amb_tol); the device's count lies in [count, count + amb]."""
    n = len(p0)
    hyps = np.atleast_1d(np.asarray(hyps, np.int64))
    idx = sample_indices(seed, hyps, n)
    ep = eight_point(p0, p1, idx)
    F, valid, kappa = ep["F"], ~ep["dup"], ep["kappa"].copy()
    if essential:
        E, ok, gap = project_essential(F)
        F, valid = E, valid & ok
        kappa = kappa + 1.0 / np.maximum(gap, 1e-300)
    F = np.where(valid[:, None, None], F, 0.0)
    thr2 = float(threshold) ** 2
    amb_tol = 1e-6
    count = np.zeros(len(hyps), np.int64)
    amb = np.zeros(len(hyps), np.int64)
    for c in range(0, len(hyps), chunk):
        r = sampson_ratio(F[c:c + chunk], p0, p1, thr2)
        count[c:c + chunk] = (r < 1 - amb_tol).sum(1)
        amb[c:c + chunk] = (np.abs(r - 1) <= amb_tol).sum(1)
    count[~valid] = amb[~valid] = 0
    return {"idx": idx, "F": F, "valid": valid, "dup": ep["dup"], "cond": ep["cond"], "kappa": kappa, "count": count, "amb": amb}


def select(count):
    """The select kernel: the most inliers wins, ties go to the lowest index. Returns (count, index); with count 0 the device writes
    F = 0 and an all-false mask."""
    count = np.asarray(count)
    h = int(np.argmax(count))               # first of the maxima
    return int(count[h]), h


def f_close(Fd, Fo, kappa, k=64.0):
    """|Fd -/+ Fo|_max <= k eps kappa (+ a floor of 1e-14): F agrees up to sign within its conditioning bound."""
    Fd, Fo = np.asarray(Fd).reshape(3, 3), np.asarray(Fo).reshape(3, 3)
    d = min(np.abs(Fd - Fo).max(), np.abs(Fd + Fo).max())
    return d <= k * EPS * kappa + 1e-14, d


# ------------------------------------------------------------------------------------------------ triangulation
def triangulate(P0, P1, x0, x1):
    """The reference's two-view system per point, [P_i | -x_i e_i] [X; lambda] = 0 (6 x 6), its SVD null vector normalised to X[3] = 1.
    Returns (X [n, 4], bound [n]): `bound` is a first-order bound on |X - X_true|_max / |X|_max from rounding in a backward-stable solver,
    eps * sigma1 / (sigma5 - sigma6) / |v3| with v the unit null vector."""
    x0, x1 = np.asarray(x0, np.float64), np.asarray(x1, np.float64)
    n = len(x0)
    M = np.zeros((n, 6, 6))
    M[:, 0:3, 0:4] = np.asarray(P0, np.float64).reshape(3, 4)
    M[:, 3:6, 0:4] = np.asarray(P1, np.float64).reshape(3, 4)
    M[:, 0:3, 4] = -x0
    M[:, 3:6, 5] = -x1
    if n == 0:
        return np.zeros((0, 4)), np.zeros(0)
    _, s, vt = np.linalg.svd(M)
    v = vt[:, -1]
    X = v[:, :4] / v[:, 3:4]
    bound = EPS * s[:, 0] / np.maximum(s[:, 4] - s[:, 5], 1e-300) / np.abs(v[:, 3])
    return X, bound


# ------------------------------------------------------------------------------------------------ tile merge, row gather
def merge_rows(matches, slots, off, origin, kp_bank, n_bank):
    """Rows of the merge before the unique step, concatenated in tile-pair order: for pair p and keypoint i < n_bank[t0] with
    matches[p, i] > -1, mkpts0 = (kp + off) + origin in float32 (the reference's order), mkpts1 likewise. Returns (mk0, mk1, idx0, idx1)."""
    matches, slots, n_bank = np.asarray(matches), np.asarray(slots), np.asarray(n_bank)
    off, origin, kp_bank = np.asarray(off, np.float32), np.asarray(origin, np.float32), np.asarray(kp_bank, np.float32)
    P, K = matches.shape
    mk0, mk1, i0, i1 = [], [], [], []
    for p in range(P):
        t0, t1 = int(slots[p, 0]), int(slots[p, 1])
        rows = np.nonzero((np.arange(K) < n_bank[t0]) & (matches[p] > -1))[0]
        j = matches[p, rows]
        mk0.append((kp_bank[t0, rows] + off[p, 0:2]) + origin[0:2])
        mk1.append((kp_bank[t1, j] + off[p, 2:4]) + origin[2:4])
        i0.append(t0 * K + rows)
        i1.append(t1 * K + j)
    return (np.concatenate(mk0).astype(np.float32), np.concatenate(mk1).astype(np.float32), np.concatenate(i0).astype(np.int32),
            np.concatenate(i1).astype(np.int32))


def merge_tile_matches(matches, slots, off, origin, kp_bank, n_bank):
    """The header contract of `im_merge_tile_matches`: the rows of `merge_rows`, then the unique image-0 points in lexicographic (x, y)
    order, each with the first row that holds it. Returns (idx0, idx1, kp0, kp1)."""
    mk0, mk1, i0, i1 = merge_rows(matches, slots, off, origin, kp_bank, n_bank)
    order = np.lexsort((np.arange(len(mk0)), mk0[:, 1], mk0[:, 0]))     # x, then y, then row: the first occurrence leads its group
    s = mk0[order]
    first = np.ones(len(s), bool)
    first[1:] = (s[1:] != s[:-1]).any(1)
    keep = order[first]
    return i0[keep], i1[keep], mk0[keep], mk1[keep]
