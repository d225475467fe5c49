"""The numpy restatement of the semi-global regularisation of a dense-stereo depth map (csrc/sgm_pixel.h): the sweep's scores
(`dense_oracle.scores`) as an 8-bit cost volume, min-plus path costs summed over four or eight directions, and the choice of the plane of
least sum with its sub-plane offset. A definition of this project's own; it is not Metashape's depth filter. Costs, path costs and sums
are integers, so the kernels equal this bit for bit whatever order they walk the paths in; the two float64 expressions (the cost out of
the score, the offset and the inverse depth) are written element by element in the association of the header."""
import numpy as np

import dense_oracle as O

MAX_PLANES, MAX_PENALTY, INVALID = 256, 4095, 255
DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))       # (dy, dx); `paths` = 4 takes the first four
FAR = 1 << 20


def quantise(valid, s):
    """cost [h0, w0, D] uint8 from the sweep's (valid, s) [D, h0, w0]: 255 where invalid, else min(254, max(0, floor((1 - s) 127)))."""
    with np.errstate(all="ignore"):
        q = np.floor((1.0 - np.where(valid, s, 0.0)) * 127.0)
    c = np.minimum(254, np.maximum(0, q.astype(np.int64)))
    return np.ascontiguousarray(np.moveaxis(np.where(valid, c, INVALID), 0, -1).astype(np.uint8))


def cost_volume(ref, src, A, B, w_first, w_step, D, r, min_var=4):
    return quantise(*O.scores(ref, src, A, B, w_first, w_step, D, r, min_var))


def check_penalties(P1, P2, paths):
    if not (int(P1) == P1 and int(P2) == P2 and 0 <= P1 <= P2 <= MAX_PENALTY):
        raise ValueError(f"0 <= P1 <= P2 <= {MAX_PENALTY} is expected (got {P1}, {P2})")
    if paths not in (4, 8):
        raise ValueError(f"paths is 4 or 8 (got {paths})")


def path_costs(cost, P1, P2, dy, dx):
    """L [h0, w0, D] int64 along one direction: a whole row (dy != 0) or column (dy == 0) of pixels at a time, each from the row or column
    before it; pixels whose predecessor lies outside the image take their plain cost."""
    c = np.asarray(cost).astype(np.int64)
    h0, w0, D = c.shape
    L = np.empty_like(c)

    def step(cp, Lq, has_q):
        """cp [n, D] costs, Lq [n, D] the predecessors' path costs (any value where has_q [n] is False)."""
        m = Lq.min(1, keepdims=True)
        below = np.full_like(Lq, FAR)
        above = np.full_like(Lq, FAR)
        below[:, 1:] = Lq[:, :-1] + P1
        above[:, :-1] = Lq[:, 1:] + P1
        best = np.minimum(np.minimum(Lq, m + P2), np.minimum(below, above))
        return np.where(has_q[:, None], cp + best - m, cp)

    if dy == 0:
        xs = range(w0) if dx > 0 else range(w0 - 1, -1, -1)
        for x in xs:
            q = x - dx
            inside = 0 <= q < w0
            L[:, x] = step(c[:, x], L[:, q] if inside else c[:, x], np.full(h0, inside))
        return L
    ys = range(h0) if dy > 0 else range(h0 - 1, -1, -1)
    for y in ys:
        qy = y - dy
        if not 0 <= qy < h0:
            L[y] = c[y]
            continue
        qx = np.arange(w0) - dx
        has = (qx >= 0) & (qx < w0)
        L[y] = step(c[y], L[qy][np.clip(qx, 0, w0 - 1)], has)
    return L


def aggregate(cost, P1, P2, paths=8):
    """sum [h0, w0, D] uint16 of the path costs over the first `paths` directions."""
    check_penalties(P1, P2, paths)
    cost = np.asarray(cost)
    assert cost.dtype == np.uint8 and cost.ndim == 3 and 1 <= cost.shape[2] <= MAX_PLANES
    S = np.zeros(cost.shape, np.int64)
    for dy, dx in DIRECTIONS[:paths]:
        S += path_costs(cost, int(P1), int(P2), dy, dx)
    assert S.max() <= paths * (255 + P2) <= 65535
    return S.astype(np.uint16)


def choose(cost, S, w_first, w_step, min_score):
    """(plane int16, w float64, score float32) [h0, w0]: the least sum among the planes valid at the pixel, ties to the lower plane."""
    cost, S = np.asarray(cost), np.asarray(S)
    assert cost.dtype == np.uint8 and S.dtype == np.uint16 and cost.shape == S.shape
    h0, w0, D = cost.shape
    c, Si = cost.astype(np.int64), S.astype(np.int64)
    ok = c != INVALID
    key = np.where(ok, Si * 65536 + np.arange(D), 1 << 40)
    k = key.argmin(2)                                            # unique keys: the lower plane carries the lower key
    some = ok.any(2)
    ii, jj = np.indices((h0, w0))
    c0, S0 = c[ii, jj, k], Si[ii, jj, k]
    km, kp = np.clip(k - 1, 0, D - 1), np.clip(k + 1, 0, D - 1)
    inner = (k >= 1) & (k <= D - 2) & ok[ii, jj, km] & ok[ii, jj, kp]
    Sm, Sp = Si[ii, jj, km], Si[ii, jj, kp]
    den = (Sm - 2 * S0) + Sp
    use = inner & (den > 0)
    with np.errstate(all="ignore"):
        off = np.where(use, (0.5 * (Sm - Sp).astype(np.float64)) / np.where(use, den, 1).astype(np.float64), 0.0)
        w = np.float64(w_first) + (k.astype(np.float64) + off) * np.float64(w_step)
        sc = 1.0 - c0.astype(np.float64) / 127.0
    kept = some & ~(sc < min_score)
    return np.where(kept, k, -1).astype(np.int16), np.where(kept, w, 0.0), np.where(kept, sc, 0.0).astype(np.float32)


def sweep(ref, src, A, B, w_first, w_step, D, r, min_var=4, min_score=0.8, P1=16, P2=128, paths=8):
    """The regularised counterpart of `dense_oracle.sweep`: cost, aggregate, choose."""
    cost = cost_volume(ref, src, A, B, w_first, w_step, D, r, min_var)
    return choose(cost, aggregate(cost, P1, P2, paths), w_first, w_step, min_score)
