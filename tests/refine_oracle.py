"""The numpy restatement of the slanted-window refinement of a depth map (csrc/refine_pixel.h): the slant of a pixel, a
least-squares plane through the inverse depths of its neighbourhood out of exact integer sums, and the refined inverse depth, the best of
a few sub-plane candidates whose window samples follow that slant. A definition of this project's own: Metashape's matcher is closed and is
not reproduced. The sample and the score are `dense_oracle`'s; float64 element by element in the association of the header (numpy never
contracts), integers everywhere else, so the kernels equal this bit for bit whatever order they sum in. Slants are in plane steps per pixel."""
import numpy as np

import dense_oracle as O

MAX_FIT_RADIUS, MIN_COUNT, MAX_COUNT, MAX_SPAN, MAX_SUB, MAX_DIFF, Q = 7, 3, 225, 4, 8, 64.0, 1024


# ---- (1) the slant ---------------------------------------------------------------------------------------------------------------------------
def slant_sums(plane, w, w_step, R, max_diff):
    """The nine int64 sums [9, h, w] (n, Sx, Sy, Sxx, Syy, Sxy, Sq, Sqx, Sqy) of every pixel over its counting neighbours; zero where the
    pixel is dropped."""
    plane, w = np.asarray(plane), np.asarray(w, np.float64)
    h, wd = plane.shape
    kept = plane >= 0
    s = np.zeros((9, h, wd), np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            # pixel i = (y, x) of [ys, xs] has its neighbour j = (y + dy, x + dx) inside the map
            ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(wd, wd - dx))
            yj, xj = slice(max(0, -dy) + dy, min(h, h - dy) + dy), slice(max(0, -dx) + dx, min(wd, wd - dx) + dx)
            if ys.start >= ys.stop or xs.start >= xs.stop:
                continue
            with np.errstate(all="ignore"):
                d = (w[yj, xj] - w[ys, xs]) / np.float64(w_step)
                counts = kept[ys, xs] & kept[yj, xj] & (np.abs(d) <= max_diff)           # a NaN fails
                q = np.rint(np.where(counts, d, 0.0) * 1024.0).astype(np.int64)            # ties to even, as llrint
            c = counts.astype(np.int64)
            for k, term in enumerate((c, c * dx, c * dy, c * dx * dx, c * dy * dy, c * dx * dy, q, q * dx, q * dy)):
                s[k][ys, xs] += term
    return s


def slant_fit(s, min_count):
    """(slant [h, w, 2] float64, fitted [h, w] uint8) out of the nine sums."""
    n, sx, sy, sxx, syy, sxy, sq, sqx, sqy = s
    a11, a22, a12 = n * sxx - sx * sx, n * syy - sy * sy, n * sxy - sx * sy
    b1, b2 = n * sqx - sx * sq, n * sqy - sy * sq
    det = a11 * a22 - a12 * a12
    fitted = (n >= min_count) & (det > 0)
    safe = np.where(fitted, det, 1).astype(np.float64)
    gu = ((a22 * b1 - a12 * b2).astype(np.float64) / safe) / 1024.0
    gv = ((a11 * b2 - a12 * b1).astype(np.float64) / safe) / 1024.0
    return np.stack([np.where(fitted, gu, 0.0), np.where(fitted, gv, 0.0)], -1), fitted.astype(np.uint8)


def slant(plane, w, w_step, R=4, max_diff=2.0, min_count=6):
    return slant_fit(slant_sums(plane, w, w_step, R, max_diff), min_count)


# ---- (2) the refined depth -------------------------------------------------------------------------------------------------------------------
def candidate_scores(ref, src, A, B, w, sl, w_step, r, min_var, span, sub):
    """(valid [N, h0, w0] bool, s [N, h0, w0] float64) of the N = 2 span sub + 1 candidates c = -span sub .. span sub of every pixel whose
    window lies inside ref (nothing is valid elsewhere). The sample of (dx, dy) is `dense_oracle.sample` at ref pixel (u + dx, v + dy) under
    the centre's own H: the H of every centre is moved by (dy, dx), so that the grid of `sample` is the grid of the sample positions."""
    ref = np.asarray(ref)
    assert ref.dtype == np.uint8 and ref.ndim == 2
    h0, w0 = ref.shape
    half = span * sub
    N = 2 * half + 1
    valid, s = np.zeros((N, h0, w0), bool), np.zeros((N, h0, w0))
    if h0 < 2 * r + 1 or w0 < 2 * r + 1:
        return valid, s
    a = ref.astype(np.int64)
    n = (2 * r + 1) ** 2
    sa, saa = O.box(a, r), O.box(a * a, r)
    A, B = np.asarray(A, np.float64).reshape(9), np.asarray(B, np.float64).reshape(9)
    w = np.asarray(w, np.float64)
    gu, gv = np.asarray(sl, np.float64)[..., 0], np.asarray(sl, np.float64)[..., 1]
    inner = (slice(r, h0 - r), slice(r, w0 - r))
    for c in range(-half, half + 1):
        sb, sbb, sab = (np.zeros((h0, w0), np.int64) for _ in range(3))
        inv = np.zeros((h0, w0), np.int64)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                with np.errstate(all="ignore"):
                    t = np.float64(c) / np.float64(sub) + (gu * np.float64(dx) + gv * np.float64(dy))
                    ws = w + t * np.float64(w_step)
                    H = A[:, None, None] + ws[None] * B[:, None, None]
                b, ok = O.sample(src, np.roll(H, (dy, dx), (1, 2)), h0, w0)
                b, ok = np.roll(b, (-dy, -dx), (0, 1)), np.roll(ok, (-dy, -dx), (0, 1))      # back onto the centres
                av = np.roll(a, (-dy, -dx), (0, 1))
                sb += b
                sbb += b * b
                sab += av * b
                inv += ~ok
        v, sc = O.score(n, sa, saa, sb[inner], sbb[inner], sab[inner], min_var)
        v = v & (inv[inner] == 0)
        valid[c + half][inner] = v
        s[c + half][inner] = np.where(v, sc, 0.0)
    return valid, s


def choose(valid, s, plane, w, score, w_step, span, sub, r):
    """(w' float64, score' float32, taken uint8): the candidates visited in the order 0, -1, +1, -2, +2, ..., a later one replacing the
    best only on a strictly greater score."""
    plane, w, score = np.asarray(plane), np.asarray(w, np.float64), np.asarray(score, np.float32)
    h0, w0 = plane.shape
    half = span * sub
    N = 2 * half + 1
    k = np.full((h0, w0), -1, np.int64)
    s0 = np.zeros((h0, w0))
    order = [0] + [c for m in range(1, half + 1) for c in (-m, m)]
    for c in order:
        d = c + half
        rep = valid[d] & ((k < 0) | (s[d] > s0))
        k, s0 = np.where(rep, d, k), np.where(rep, s[d], s0)
    kc = np.clip(k, 1, N - 2)
    ii, jj = np.indices((h0, w0))
    sm, sp, vm, vp = s[kc - 1, ii, jj], s[kc + 1, ii, jj], valid[kc - 1, ii, jj], valid[kc + 1, ii, jj]
    inside = np.zeros((h0, w0), bool)
    if h0 >= 2 * r + 1 and w0 >= 2 * r + 1:
        inside[r:h0 - r, r:w0 - r] = True
    with np.errstate(all="ignore"):
        den = (sm - 2.0 * s0) + sp
        use = (k >= 1) & (k <= N - 2) & vm & vp & (den < 0.0)
        off = np.where(use, (0.5 * (sm - sp)) / np.where(use, den, 1.0), 0.0)
        taken = (plane >= 0) & inside & (k >= 0) & (s0 > score.astype(np.float64))          # a NaN score takes nothing
        w_new = w + (((k - half).astype(np.float64) + off) / np.float64(sub)) * np.float64(w_step)
    return np.where(taken, w_new, w), np.where(taken, s0.astype(np.float32), score), taken.astype(np.uint8)


def refine(ref, src, A, B, plane, w, score, sl, w_step, r=3, min_var=4, span=1, sub=4):
    valid, s = candidate_scores(ref, src, A, B, w, sl, w_step, r, min_var, span, sub)
    return choose(valid, s, plane, w, score, w_step, span, sub, r)


def refine_slanted(ref, src, A, B, plane, w, score, w_step, passes=2, fit_radius=4, max_diff=2.0, min_count=6, span=1, sub=4, r=3, min_var=4):
    """`passes` times slant, then refine: (w, score, taken of the last pass, slant of the last pass)."""
    taken = sl = None
    for _ in range(passes):
        sl, _ = slant(plane, w, w_step, fit_radius, max_diff, min_count)
        w, score, taken = refine(ref, src, A, B, plane, w, score, sl, w_step, r, min_var, span, sub)
    return w, score, taken, sl
