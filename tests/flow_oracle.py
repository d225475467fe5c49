"""The numpy restatement of the dense surface displacement between two epochs (csrc/flow_pixel.h): the match of every pixel of
image a in image b by the zero-mean normalised cross-correlation of exact integer window sums over an integer search range, with a
parabola between the best candidate's neighbours; the forward-backward check of two fields; the lift of both ends of a match to world
points through each epoch's own depth map and pose. A definition of this project's own: the reference has no such step. The definition and
nothing cleverer: every candidate of every pixel is scored, and they are visited in the order the definition names. float64 element by
element in the association of the header (numpy never contracts), integers everywhere else, so the kernels equal this bit for bit
whatever order they sum in."""
import numpy as np

import dense_oracle as O

MAX_RADIUS, MAX_SEARCH, MAX_PRIOR, MAX_MIN_VAR = 15, 16, 4096, 1 << 26


# ---- match ------------------------------------------------------------------------------------------------------------------------------------
def score(n, sa, saa, sb, sbb, sab, min_var):
    """(valid, s) of windows from their integer sums (int64 arrays): `dense_oracle.score` without the 2^20 scale of warped samples."""
    VA, VB, C = n * saa - sa * sa, n * sbb - sb * sb, n * sab - sa * sb
    valid = ~((VA < n * n * min_var) | (VB < n * n * min_var) | (VA <= 0) | (VB <= 0))
    with np.errstate(all="ignore"):
        s = C.astype(np.float64) / np.sqrt(VA.astype(np.float64) * VB.astype(np.float64))
    return valid, np.where(valid, s, 0.0)


def order(S):
    """The candidates (dx, dy) in ascending (dx^2 + dy^2, dy, dx)."""
    return sorted(((dx, dy) for dy in range(-S, S + 1) for dx in range(-S, S + 1)), key=lambda c: (c[0] * c[0] + c[1] * c[1], c[1], c[0]))


def candidate_scores(a, b, r, S, prior=(0, 0), min_var=4):
    """(valid [2 S + 1, 2 S + 1, h, w] bool, s likewise float64), indexed [dy + S, dx + S]: the score of every candidate of every pixel;
    invalid where either window leaves its image."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.ndim == 2 and a.shape == b.shape
    h, w = a.shape
    side, n = 2 * S + 1, (2 * r + 1) ** 2
    valid, s = np.zeros((side, side, h, w), bool), np.zeros((side, side, h, w))
    if h < 2 * r + 1 or w < 2 * r + 1:
        return valid, s
    ai, bi = a.astype(np.int64), b.astype(np.int64)
    sa, saa, sb, sbb = O.box(ai, r), O.box(ai * ai, r), O.box(bi, r), O.box(bi * bi, r)      # [h - 2 r, w - 2 r], of the centre (y - r, x - r)
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            ex, ey = prior[0] + dx, prior[1] + dy
            # the pixels (y, x) of a whose partner (y + ey, x + ex) lies in b; a window inside this overlap lies inside a and its partner inside b
            y0, y1, x0, x1 = max(0, -ey), min(h, h - ey), max(0, -ex), min(w, w - ex)
            if y1 - y0 < 2 * r + 1 or x1 - x0 < 2 * r + 1:
                continue
            sab = O.box(ai[y0:y1, x0:x1] * bi[y0 + ey:y1 + ey, x0 + ex:x1 + ex], r)           # centres y0 + r .. y1 - r - 1 of a
            ca = (slice(y0, y1 - 2 * r), slice(x0, x1 - 2 * r))                                # those centres in the box arrays of a
            cb = (slice(y0 + ey, y1 + ey - 2 * r), slice(x0 + ex, x1 + ex - 2 * r))            # and their partners in those of b
            v, sc = score(n, sa[ca], saa[ca], sb[cb], sbb[cb], sab, min_var)
            at = (slice(y0 + r, y1 - r), slice(x0 + r, x1 - r))
            valid[dy + S, dx + S][at] = v
            s[dy + S, dx + S][at] = sc
    return valid, s


def choose(valid, s, S, prior=(0, 0), min_score=0.8, ask=None):
    """(du, dv float64, score float32, valid uint8) [h, w] from the scores of every candidate."""
    _, _, h, w = s.shape
    have = np.zeros((h, w), bool)
    s0 = np.zeros((h, w))
    bx, by = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    for dx, dy in order(S):
        rep = valid[dy + S, dx + S] & (~have | (s[dy + S, dx + S] > s0))
        have, s0 = have | rep, np.where(rep, s[dy + S, dx + S], s0)
        bx, by = np.where(rep, dx, bx), np.where(rep, dy, by)
    ii, jj = np.indices((h, w))

    def offset(ax, ay):
        inside = (bx - ax >= -S) & (bx + ax <= S) & (by - ay >= -S) & (by + ay <= S)
        my, mx = np.clip(by - ay + S, 0, 2 * S), np.clip(bx - ax + S, 0, 2 * S)
        py, px = np.clip(by + ay + S, 0, 2 * S), np.clip(bx + ax + S, 0, 2 * S)
        sm, sp = s[my, mx, ii, jj], s[py, px, ii, jj]
        both = inside & valid[my, mx, ii, jj] & valid[py, px, ii, jj]
        with np.errstate(all="ignore"):
            den = (sm - 2.0 * s0) + sp
            use = both & (den < 0.0)
            return np.where(use, (0.5 * (sm - sp)) / np.where(use, den, 1.0), 0.0)

    ok = have & ~(s0 < min_score)
    if ask is not None:
        ok &= np.asarray(ask) != 0
    du = (np.float64(prior[0]) + bx.astype(np.float64)) + offset(1, 0)
    dv = (np.float64(prior[1]) + by.astype(np.float64)) + offset(0, 1)
    return np.where(ok, du, 0.0), np.where(ok, dv, 0.0), np.where(ok, s0, 0.0).astype(np.float32), ok.astype(np.uint8)


def match(a, b, ask=None, r=7, S=8, prior=(0, 0), min_var=4, min_score=0.8):
    valid, s = candidate_scores(a, b, r, S, prior, min_var)
    return choose(valid, s, S, prior, min_score, ask)


# ---- check ------------------------------------------------------------------------------------------------------------------------------------
def check(du, dv, valid, du_b, dv_b, valid_b, tol):
    """keep [h, w] uint8."""
    h, w = du.shape
    u = np.arange(w, dtype=np.float64)[None, :]
    v = np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        ju, jv = np.rint(u + du), np.rint(v + dv)
        inside = (ju >= 0.0) & (ju <= float(w - 1)) & (jv >= 0.0) & (jv <= float(h - 1))      # a NaN fails
        iu, iv = np.where(inside, ju, 0.0).astype(np.int64), np.where(inside, jv, 0.0).astype(np.int64)
        ex, ey = du + du_b[iv, iu], dv + dv_b[iv, iu]
        ok = inside & (valid_b[iv, iu] != 0) & (ex * ex + ey * ey <= np.float64(tol) * np.float64(tol))
    return ((np.asarray(valid) != 0) & ok).astype(np.uint8)


# ---- lift -------------------------------------------------------------------------------------------------------------------------------------
def depth_at(plane_b, w_b, keep_b, x, y, span):
    """(ok, w) of map b at the float positions (x, y)."""
    hb, wb = plane_b.shape
    with np.errstate(all="ignore"):
        fx, fy = np.floor(x), np.floor(y)
        inside = (fx >= 0.0) & (fx + 1.0 <= float(wb - 1)) & (fy >= 0.0) & (fy + 1.0 <= float(hb - 1))      # a NaN fails
        x0 = np.clip(np.where(inside, fx, 0.0).astype(np.int64), 0, max(wb - 2, 0))
        y0 = np.clip(np.where(inside, fy, 0.0).astype(np.int64), 0, max(hb - 2, 0))
        x1, y1 = np.minimum(x0 + 1, wb - 1), np.minimum(y0 + 1, hb - 1)
        taps = ((y0, x0), (y0, x1), (y1, x0), (y1, x1))
        ok = inside.copy()
        for t in taps:
            ok &= (plane_b[t] >= 0) & (keep_b[t] != 0)
        w00, w01, w10, w11 = (w_b[t] for t in taps)
        lo, hi = w00, w00
        for t in (w01, w10, w11):                                                     # in the header's order, by its comparisons
            lo, hi = np.where(t < lo, t, lo), np.where(t > hi, t, hi)
        ok &= (hi - lo) <= span
        tx, ty = x - fx, y - fy
        top, bot = w00 + tx * (w01 - w00), w10 + tx * (w11 - w10)
        w = top + ty * (bot - top)
    return ok, np.where(ok, w, 0.0)


def lift(du, dv, valid, keep, plane_a, w_a, cam_a, plane_b, w_b, keep_b, cam_b, w_step_b, max_diff):
    """(P [h, w, 3], D [h, w, 3] float64, ok [h, w] uint8). cam = inv(K), R, t [21]."""
    h, w = du.shape
    cam_a, cam_b = np.asarray(cam_a, np.float64).reshape(21), np.asarray(cam_b, np.float64).reshape(21)
    u = np.arange(w, dtype=np.float64)[None, :]
    v = np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        x, y = u + du, v + dv
        span = np.float64(max_diff) * np.abs(np.float64(w_step_b))
        found, wq = depth_at(plane_b, w_b, keep_b, x, y, span)
        ok = (np.asarray(keep) != 0) & (plane_a >= 0) & (np.asarray(valid) != 0) & found
        P = O.to_world(cam_a, O.backproject(cam_a[:9], h, w, np.where(ok, w_a, 1.0)))
        Ki = cam_b[:9]
        wq = np.where(ok, wq, 1.0)
        X = np.stack([((Ki[3 * i] * x + Ki[3 * i + 1] * y) + Ki[3 * i + 2]) / wq for i in range(3)], -1)
        Q = O.to_world(cam_b, X)
        D = Q - P
    return np.where(ok[..., None], P, 0.0), np.where(ok[..., None], D, 0.0), ok.astype(np.uint8)


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------------
def camera(K, R, t):
    return np.concatenate([O.W.inv3(K).reshape(9), np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def surface_displacement(map_a, keep_a, map_b, keep_b, dt_days, do_check=True, radius=7, search=8, prior=(0, 0), min_var=4, min_score=0.8, tol=1.0,
                         max_diff=2.0):
    """A map is a dict of grey, plane, w, K, R, t, w_step. Returns (points, displacement, velocity, score, pixels) of the lifted pixels in
    row-major order, and the forward field, the keep mask and (P, D, ok) for those who want to look."""
    fwd = match(map_a["grey"], map_b["grey"], keep_a, radius, search, prior, min_var, min_score)
    keep = fwd[3]
    if do_check:
        bwd = match(map_b["grey"], map_a["grey"], None, radius, search, (-prior[0], -prior[1]), min_var, min_score)
        keep = check(fwd[0], fwd[1], fwd[3], bwd[0], bwd[1], bwd[3], tol)
    P, D, ok = lift(fwd[0], fwd[1], fwd[3], keep, map_a["plane"], map_a["w"], camera(map_a["K"], map_a["R"], map_a["t"]), map_b["plane"], map_b["w"], keep_b,
                    camera(map_b["K"], map_b["R"], map_b["t"]), map_b["w_step"], max_diff)
    sel = ok != 0
    vu = np.argwhere(sel)
    Dn = D[sel]
    return (P[sel], Dn, Dn / np.float64(dt_days), fwd[2][sel], np.stack([vu[:, 1], vu[:, 0]], 1).astype(np.int64)), fwd, keep, (P, D, ok)
