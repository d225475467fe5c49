"""The numpy restatement of the coarse-to-fine dense displacement (csrc/flow_field_pixel.h, csrc/dense_flow_field.hip): the
levels of the pyramid through `oracle.pyramid_cpu.pyr_down`, the prior of a fine pixel from the field of the level above (twice the lower
median of the valid, finite displacements around its parent), the match of every pixel around its own prior (`flow_oracle.match` once per
distinct prior, selected per pixel: the definition and nothing cleverer), the rule that names the path a tile of the kernel takes, and the
chain down the pyramid and on through `flow_oracle.check` and `flow_oracle.lift`. float64 element by element, integers everywhere else."""
import numpy as np

import flow_oracle as FO
from oracle.pyramid_cpu import pyr_down

MAX_LEVELS, MAX_MEDIAN_RADIUS, MAX_SPREAD, LDS_BUDGET = 6, 2, 8, 64 * 1024 - 1024
TILE_W, TILE_H = 64, 16


# ---- levels -------------------------------------------------------------------------------------------------------------------------------------
def levels_of(img, levels):
    out = [np.ascontiguousarray(img)]
    for _ in range(levels - 1):
        out.append(pyr_down(out[-1]))
    return out


def coarse_prior(p, levels):
    """rint(p / 2^(levels - 1)), ties to even, in integers."""
    d = 1 << (levels - 1)
    q, rest = divmod(int(p), d)
    return q + (1 if 2 * rest > d or (2 * rest == d and q % 2 == 1) else 0)


def reach(levels, search, fine_search):
    return 2 ** (levels - 1) * search + (2 ** (levels - 1) - 1) * fine_search


# ---- the prior of a level from the field above -----------------------------------------------------------------------------------------------------
def prior_up(du_c, dv_c, valid_c, shape, m=1, min_count=1):
    """(pu, pv int16, have uint8) [h, w]."""
    h, w = shape
    hc, wc = du_c.shape
    assert (hc, wc) == ((h + 1) // 2, (w + 1) // 2)
    with np.errstate(all="ignore"):
        use_c = (np.asarray(valid_c) != 0) & np.isfinite(du_c) & np.isfinite(dv_c)
    # the neighbourhood of every coarse pixel, padded: [(2 m + 1)^2, hc, wc]; an unused place holds +inf and sorts behind every used one
    pad = lambda a, fill: np.pad(a, m, constant_values=fill)      # noqa: E731
    U, xs, ys = pad(use_c, False), pad(np.where(use_c, du_c, np.inf), np.inf), pad(np.where(use_c, dv_c, np.inf), np.inf)
    cut = lambda a: np.stack([a[dy:dy + hc, dx:dx + wc] for dy in range(2 * m + 1) for dx in range(2 * m + 1)])      # noqa: E731
    n = cut(U).sum(0)
    k = np.maximum(n - 1, 0) // 2
    med = [np.take_along_axis(np.sort(cut(a), 0), k[None], 0)[0] for a in (xs, ys)]
    with np.errstate(all="ignore"):
        p = [np.rint(2.0 * np.where(n > 0, a, 0.0)) for a in med]
    have = (n >= min_count) & (n > 0) & (np.abs(p[0]) <= 4096.0) & (np.abs(p[1]) <= 4096.0)
    pu_c, pv_c = (np.where(have, a, 0.0).astype(np.int16) for a in p)
    iy, ix = np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1
    return np.ascontiguousarray(pu_c[iy, ix]), np.ascontiguousarray(pv_c[iy, ix]), np.ascontiguousarray(have.astype(np.uint8)[iy, ix])


# ---- the match around a prior per pixel --------------------------------------------------------------------------------------------------------------
def wanted(pu, pv, have, ask=None):
    """The pixels that are matched: have set, asked for, both components in -4096..4096."""
    pu, pv = np.asarray(pu).astype(np.int64), np.asarray(pv).astype(np.int64)
    m = (np.asarray(have) != 0) & (np.abs(pu) <= FO.MAX_PRIOR) & (np.abs(pv) <= FO.MAX_PRIOR)
    return m if ask is None else m & (np.asarray(ask) != 0)


def match_field(a, b, pu, pv, have, ask=None, r=7, S=2, min_var=4, min_score=0.8):
    """(du, dv float64, score float32, valid uint8) [h, w]: `flow_oracle.match` with each distinct prior, selected per pixel."""
    h, w = a.shape
    m = wanted(pu, pv, have, ask)
    out = (np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w), np.float32), np.zeros((h, w), np.uint8))
    key = np.asarray(pu).astype(np.int64) * 65536 + np.asarray(pv).astype(np.int64)
    for k in np.unique(key[m]):
        sel = m & (key == k)
        prior = (int(np.asarray(pu)[sel][0]), int(np.asarray(pv)[sel][0]))
        one = FO.match(a, b, None, r, S, prior, min_var, min_score)
        for o, f in zip(out, one):
            o[sel] = f[sel]
    return out


# ---- the path of a tile ------------------------------------------------------------------------------------------------------------------------------
def lds_bytes(r, S, ex, ey):
    up8 = lambda v: (v + 7) & ~7      # noqa: E731
    return (up8((TILE_W + 2 * r) * (TILE_H + 2 * r)) + up8((TILE_W + ex + 2 * (r + S)) * (TILE_H + ey + 2 * (r + S)))
            + (TILE_W + ex + 2 * S) * (TILE_H + ey + 2 * S) * 8 + (TILE_H + 2 * r) * TILE_W * 4)


def spread(r, S):
    """The widest box of priors, per axis, that a tile may span on the tiled path at (r, S)."""
    E = MAX_SPREAD
    while E > 0 and lds_bytes(r, S, E, E) > LDS_BUDGET:
        E -= 1
    return E


def tile_paths(shape, pu, pv, have, ask, r, S):
    """uint8 [blocks_y, blocks_x]: 0 no pixel of the tile is wanted with its window inside a; else 1 where the box of those pixels' priors
    spans at most spread(r, S) on either axis, 2 otherwise."""
    h, w = shape
    uu, vv = np.meshgrid(np.arange(w), np.arange(h))
    m = wanted(pu, pv, have, ask) & (uu >= r) & (uu < w - r) & (vv >= r) & (vv < h - r)
    E = spread(r, S)
    out = np.zeros(((h + TILE_H - 1) // TILE_H, (w + TILE_W - 1) // TILE_W), np.uint8)
    for by in range(out.shape[0]):
        for bx in range(out.shape[1]):
            t = (slice(by * TILE_H, (by + 1) * TILE_H), slice(bx * TILE_W, (bx + 1) * TILE_W))
            if m[t].any():
                x, y = np.asarray(pu)[t][m[t]].astype(np.int64), np.asarray(pv)[t][m[t]].astype(np.int64)
                out[by, bx] = 1 if x.max() - x.min() <= E and y.max() - y.min() <= E else 2
    return out


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------------------
def match_pyramid(a, b, ask=None, levels=3, r=7, S=8, fine=2, prior=(0, 0), min_var=4, min_score=0.8, m=1, min_count=1, trace=None):
    """Level 0's field. `trace`: a list that receives, per finer level and coarsest first, (level, prior field, tile paths)."""
    if levels == 1:
        return FO.match(a, b, ask, r, S, prior, min_var, min_score)
    la, lb = levels_of(a, levels), levels_of(b, levels)
    field = FO.match(la[-1], lb[-1], None, r, S, (coarse_prior(prior[0], levels), coarse_prior(prior[1], levels)), min_var, min_score)
    for level in range(levels - 2, -1, -1):
        pf = prior_up(field[0], field[1], field[3], la[level].shape, m, min_count)
        mask = ask if level == 0 else None
        if trace is not None:
            trace.append((level, pf, tile_paths(la[level].shape, *pf, mask, r, fine)))
        field = match_field(la[level], lb[level], *pf, mask, r, fine, min_var, min_score)
    return field


def surface_displacement(map_a, keep_a, map_b, keep_b, dt_days, do_check=True, radius=7, search=8, prior=(0, 0), min_var=4, min_score=0.8, tol=1.0,
                         max_diff=2.0, levels=1, fine_search=2, median_radius=1, min_count=1):
    """`flow_oracle.surface_displacement` with the pyramid in place of both matches."""
    pyr = dict(levels=levels, r=radius, S=search, fine=fine_search, min_var=min_var, min_score=min_score, m=median_radius, min_count=min_count)
    fwd = match_pyramid(map_a["grey"], map_b["grey"], keep_a, prior=prior, **pyr)
    keep = fwd[3]
    if do_check:
        bwd = match_pyramid(map_b["grey"], map_a["grey"], None, prior=(-prior[0], -prior[1]), **pyr)
        keep = FO.check(fwd[0], fwd[1], fwd[3], bwd[0], bwd[1], bwd[3], tol)
    P, D, ok = FO.lift(fwd[0], fwd[1], fwd[3], keep, map_a["plane"], map_a["w"], FO.camera(map_a["K"], map_a["R"], map_a["t"]), map_b["plane"], map_b["w"],
                       keep_b, FO.camera(map_b["K"], map_b["R"], map_b["t"]), map_b["w_step"], max_diff)
    sel = ok != 0
    vu = np.argwhere(sel)
    Dn = D[sel]
    return (P[sel], Dn, Dn / np.float64(dt_days), fwd[2][sel], np.stack([vu[:, 1], vu[:, 0]], 1).astype(np.int64)), fwd, keep, (P, D, ok)
