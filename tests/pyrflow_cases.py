"""The shared cases of the coarse-to-fine displacement tests (tests/test_pyrflow_cpu.py, tests/test_gpu_pyrflow.py): coarse fields for the
prior rule, images with a prior field for the match, pairs for the pyramid and the scenes whose truth is known. A case is everything an
entry point takes. Expected outputs are computed once per process by the restatement (tests/pyrflow_oracle.py) and shared; nobody may
write into them.

`dense_cases.texture` has structure at a few pixels only and is flat after two `pyr_down` steps, so nothing matches on it above level 1:
the pyramid cases use `octaves`, a sum of noise at block sizes 1 to 16. The match kernel's block owns a 64 x 16 tile."""
import functools

import numpy as np

import dense_cases as DC
import flow_cases as FC
import pyrflow_oracle as PO

M = 32            # the margin of the texture around image a


def octaves(seed, h, w):
    """A seeded 8-bit texture with structure at every scale from 1 to 16 pixels: seeded noise in blocks of 1, 2, 4, 8 and 16 pixels, summed
    and smoothed once by a 2 x 2 box."""
    rng = np.random.default_rng(seed)
    t = np.zeros((h + 1, w + 1))
    for s in (1, 2, 4, 8, 16):
        n = rng.random(((h + 1 + s - 1) // s + 1, (w + 1 + s - 1) // s + 1))
        t += np.kron(n, np.ones((s, s)))[:h + 1, :w + 1]
    t = (t[:-1, :-1] + t[1:, :-1] + t[:-1, 1:] + t[1:, 1:]) / 4.0
    t = (t - t.min()) / (t.max() - t.min())
    return np.round(t * 255.0).astype(np.uint8)


def noisy(b, seed, noise):
    if not noise:
        return np.ascontiguousarray(b)
    rng = np.random.default_rng(seed + 1000)
    return np.clip(np.rint(b.astype(np.float64) + rng.normal(0.0, noise, b.shape)), 0, 255).astype(np.uint8)


def shifted(seed, h, w, sx, sy, noise=2.0):
    """(a, b) [h, w] uint8 with b(x + sx, y + sy) = a(x, y), cut from one octave texture; Gaussian noise of sigma `noise` on b."""
    t = octaves(seed, h + 2 * M, w + 2 * M)
    return np.ascontiguousarray(t[M:M + h, M:M + w]), noisy(t[M - sy:M - sy + h, M - sx:M - sx + w], seed, noise)


def sheared(seed, h, w, left, right, noise=2.0, seam=None):
    """(a, b): the pixels of a left of the seam (the middle) move by `left` px along x, the others by `right` (left > right >= 0: the
    left side overruns the right one where they meet)."""
    t = octaves(seed, h + 2 * M, w + 2 * M)
    xb = np.arange(w)
    src = np.where(xb - left < (w // 2 if seam is None else seam), xb - left, xb - right)
    return np.ascontiguousarray(t[M:M + h, M:M + w]), noisy(t[M:M + h, M + src], seed, noise)


def stretched(seed, h, w, far, noise=2.0):
    """(a, b, d): pixel x of a moves by d(x) = far x / (w - 1) px along x, linearly from 0 to `far`; b by linear interpolation of the texture."""
    t = octaves(seed, h + 2 * M, w + 2 * M).astype(np.float64)
    g = far / (w - 1.0)
    xa = np.arange(w) / (1.0 + g)                        # the place in a that lands on column x of b
    x0 = np.floor(xa).astype(np.int64)
    f = xa - x0
    b = (1.0 - f)[None, :] * t[M:M + h, M + x0] + f[None, :] * t[M:M + h, M + x0 + 1]
    return np.ascontiguousarray(t[M:M + h, M:M + w].astype(np.uint8)), noisy(np.rint(b), seed, noise), g * np.arange(w)


frozen = FC.frozen


# ---- coarse fields for the prior rule ---------------------------------------------------------------------------------------------------------------
def coarse_field(seed, hc, wc, p_valid=0.7, spread=30.0):
    """Displacements on a grid of quarter pixels, so that twice a median often ends on .5: the tie of rint."""
    rng = np.random.default_rng(seed)
    valid = (rng.random((hc, wc)) < p_valid).astype(np.uint8)
    q = lambda: np.rint(rng.uniform(-spread, spread, (hc, wc)) * 4.0) / 4.0      # noqa: E731
    return q(), q(), valid                               # values under valid = 0 too: they must not count


def up_case(field, shape, m, min_count):
    return frozen(dict(du=field[0], dv=field[1], valid=field[2], shape=tuple(shape), m=m, min_count=min_count))


SHAPES_UP = (((8, 32), (16, 64)), ((8, 32), (15, 63)), ((9, 33), (17, 65)), ((17, 49), (33, 97)), ((1, 35), (1, 70)), ((35, 1), (70, 1)), ((1, 1), (2, 2)),
             ((1, 1), (1, 1)))


def _ups():
    c = {}
    for i, (coarse, fine) in enumerate(SHAPES_UP):
        for m in (0, 1, 2):
            for mc in (1, (2 * m + 1) ** 2):
                if coarse == (17, 49) or (i + m) % 3 == 0 or mc == 1 and m == 1:
                    c[f"up_{coarse[0]}x{coarse[1]}_to_{fine[0]}x{fine[1]}_m{m}_count{mc}"] = up_case(coarse_field(700 + i, *coarse, p_valid=0.85), fine, m, mc)
    hc, wc, fine = 9, 33, (17, 65)
    zero, full = np.zeros((hc, wc)), np.ones((hc, wc), np.uint8)
    c["no_valid_pixel"] = up_case((zero + 3.0, zero - 2.0, np.zeros((hc, wc), np.uint8)), fine, 1, 1)
    one = np.zeros((hc, wc), np.uint8)
    one[4, 20] = 1
    for m in (0, 1, 2):
        c[f"one_valid_pixel_m{m}"] = up_case((zero + 3.25, zero - 2.75, one), fine, m, 1)
    bad = coarse_field(720, hc, wc, p_valid=1.0)
    du, dv = bad[0].copy(), bad[1].copy()
    du[::3, ::4] = np.nan
    dv[1::3, 1::4] = np.inf
    du[2::3, 2::4] = -np.inf
    dv[::4, 3::5] = np.nan
    c["nan_and_infinity_under_valid"] = up_case((du, dv, full), fine, 1, 1)
    c["nan_and_infinity_under_valid_m0"] = up_case((du, dv, full), fine, 0, 1)
    c["nan_and_infinity_under_valid_m2_count20"] = up_case((du, dv, full), fine, 2, 20)
    # twice the median ends on .5: rint goes to the even neighbour. 1.25 -> 2.5 -> 2, 1.75 -> 3.5 -> 4, -0.25 -> -0.5 -> -0, -2.75 -> -5.5 -> -6
    halves = np.array([1.25, 1.75, -0.25, -2.75, 0.25, 2.25])[np.arange(wc) % 6][None, :] + zero
    c["medians_at_half"] = up_case((halves, -halves, full), fine, 0, 1)
    # 2 x median at the limit and beyond: 2048 -> 4096 (kept), 2048.25 -> 4096.5 -> 4096 (kept), 2048.5 -> 4097 (no prior), the other sign, and
    # numbers far beyond an int
    edge = np.array([2048.0, 2048.25, 2048.5, -2048.0, -2048.25, -2048.5, 1e300, -1e300, 3e9, 5.0])[np.arange(wc) % 10][None, :] + zero
    c["twice_the_median_at_4096_and_beyond_along_u"] = up_case((edge, zero + 1.0, full), fine, 0, 1)
    c["twice_the_median_at_4096_and_beyond_along_v"] = up_case((zero - 1.0, edge, full), fine, 0, 1)
    # an even count: two valid neighbours of different values; the lower one is the median
    two = np.zeros((hc, wc), np.uint8)
    two[4, 10], two[4, 11], two[2, 25], two[3, 25] = 1, 1, 1, 1
    du = zero.copy()
    du[4, 10], du[4, 11], du[2, 25], du[3, 25] = 7.0, 3.0, -5.0, -9.0
    c["an_even_count_takes_the_lower_median"] = up_case((du, -du, two), fine, 1, 2)
    return c


@functools.lru_cache(maxsize=None)
def ups():
    return _ups()


@functools.lru_cache(maxsize=None)
def up_expected(name):
    c = ups()[name]
    out = PO.prior_up(c["du"], c["dv"], c["valid"], c["shape"], c["m"], c["min_count"])
    for a in out:
        a.setflags(write=False)
    return out


# ---- images with a prior field -----------------------------------------------------------------------------------------------------------------------
def field_case(a, b, r, S, pu, pv, have=None, ask=None, min_var=4, min_score=0.5):
    h, w = a.shape
    grid = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int16), (h, w)))      # noqa: E731
    return frozen(dict(a=a, b=b, r=r, S=S, pu=grid(pu), pv=grid(pv), have=np.ones((h, w), np.uint8) if have is None else have, ask=ask, min_var=min_var,
                       min_score=min_score))


def _fields():
    c = {}
    # a constant field: im_flow_match with that prior. Shapes on, beside and beyond the tile's edges; r in {1, 3, 7, 15}, S in {0, 1, 2, 16}
    for (h, w), r, S, (sx, sy), prior in (((15, 63), 1, 0, (3, -2), (3, -2)), ((16, 64), 3, 1, (5, 4), (4, 4)), ((17, 65), 7, 2, (-6, 3), (-5, 1)),
                                          ((33, 97), 3, 2, (9, -7), (8, -6)), ((33, 97), 15, 1, (1, 1), (1, 0)), ((17, 65), 1, 16, (-11, 5), (-3, 2)),
                                          ((16, 64), 7, 0, (2, 0), (2, 0))):
        c[f"constant_{h}x{w}_r{r}_S{S}"] = field_case(*shifted(h * 100 + w + r + S, h, w, sx, sy), r, S, prior[0], prior[1])
    c["constant_largest_r15_S16_40x80"] = field_case(*shifted(800, 40, 80, 19, -16), 15, 16, 10, -10)
    for h, w in ((1, 70), (70, 1)):
        c[f"constant_{h}x{w}"] = field_case(*shifted(810 + h, h, w, 1, 0), 1, 1, 1, 0)
    c["constant_5x9_smaller_than_the_window"] = field_case(*shifted(812, 5, 9, 0, 0), 3, 2, 0, 0)
    # two priors inside one tile
    h, w = 33, 97
    uu, vv = np.meshgrid(np.arange(w), np.arange(h))
    a, b = sheared(820, h, w, 6, 2, seam=30)
    c["two_priors_split_along_x"] = field_case(a, b, 3, 2, np.where(uu < 30, 5, 2), 0)
    t = octaves(821, h + 2 * M, w + 2 * M)
    yb = np.arange(h)
    rows = np.where(yb - 3 < 8, yb - 3, yb + 1)                                      # rows above 8 move down by 3, the others up by 1
    a, b = np.ascontiguousarray(t[M:M + h, M:M + w]), noisy(t[M + rows][:, M:M + w], 821, 2.0)
    c["two_priors_split_along_y"] = field_case(a, b, 3, 2, 0, np.where(vv < 8, 3, -1))
    # the spread of a tile exactly at the tiled path's limit and one beyond it: r = 3, S = 2 has E = 8
    E = PO.spread(3, 2)
    a, b = shifted(822, h, w, 4, 0)
    for name, far in (("spread_at_the_limit", E), ("spread_one_beyond_the_limit", E + 1)):
        c[name + "_along_x"] = field_case(a, b, 3, 2, np.where((uu + vv) % 7 == 0, 4 - far, 4), 0)
        c[name + "_along_y"] = field_case(a, b, 3, 2, 4, np.where((uu + 2 * vv) % 5 == 0, far, 0))
    E15 = PO.spread(15, 8)
    a15, b15 = shifted(823, 48, 80, 2, 1)
    u15, v15 = np.meshgrid(np.arange(80), np.arange(48))
    c[f"spread_at_the_limit_{E15}_of_r15_S8"] = field_case(a15, b15, 15, 8, np.where(u15 % 2 == 0, 2, 2 - E15), 1)
    c[f"spread_one_beyond_the_limit_{E15}_of_r15_S8"] = field_case(a15, b15, 15, 8, np.where(u15 % 2 == 0, 2, 1 - E15), 1)
    # a random field of wide spread out of a dozen priors: direct everywhere
    rng = np.random.default_rng(824)
    a, b = shifted(824, h, w, 3, -2)
    menu = np.array([(3, -2), (-20, 4), (17, 9), (2, -3), (4, -1), (30, -30), (-9, 0), (3, 12), (0, 0), (5, -4), (-1, -2), (12, -14)], np.int16)
    pick = rng.integers(0, len(menu), (h, w))
    c["random_field_of_wide_spread"] = field_case(a, b, 3, 2, menu[pick, 0], menu[pick, 1])
    c["random_field_of_wide_spread_r1_S16"] = field_case(a, b, 1, 16, menu[pick, 0] // 4, menu[pick, 1] // 4)      # E = 8 all the same: spreads above it
    # have and ask
    c["have_all_zero"] = field_case(a, b, 3, 2, 3, -2, have=np.zeros((h, w), np.uint8))
    one = np.zeros((h, w), np.uint8)
    for y0 in range(0, h, DC.TILE_H):
        for x0 in range(0, w, DC.TILE_W):
            one[min(y0 + 5, h - 1), min(x0 + 10, w - 1)] = 1
    c["have_one_pixel_per_tile"] = field_case(a, b, 3, 2, menu[pick, 0], menu[pick, 1], have=one)
    have = (rng.random((h, w)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)      # any non-zero byte counts
    ask = np.where(uu < 64, (rng.random((h, w)) < 0.5) * rng.integers(1, 256, (h, w)), 0).astype(np.uint8)  # and one tile column asks for nothing
    c["ask_crossed_with_have"] = field_case(a, b, 3, 2, np.where(vv < 16, 3, 2), np.where(uu < 40, -2, -3), have=have, ask=ask)
    # priors at the limit, beyond it through int16 values, and priors that push every window out of b
    a, b = shifted(825, 20, 70, 0, 0)
    u2 = np.arange(70)[None, :] + np.zeros((20, 1), np.int64)
    edge = np.array([4096, -4096, 4097, -4097, 32767, -32768, 0], np.int16)
    v2 = np.arange(20)[:, None] + np.zeros((1, 70), np.int64)
    c["priors_at_4096_and_beyond"] = field_case(a, b, 2, 2, edge[u2 % 7], edge[(u2 + v2) % 7])
    c["priors_beyond_4096_only_and_zero"] = field_case(a, b, 2, 2, np.where(u2 % 2 == 0, 0, 4097), np.where(u2 % 3 == 0, 0, -32768))
    c["priors_push_every_window_out"] = field_case(a, b, 2, 4, 4096, np.where(u2 % 2 == 0, -4096, -4090))
    c["priors_leave_a_strip"] = field_case(a, b, 2, 2, np.where(u2 % 2 == 0, 60, 58), 0, min_score=-1.0)
    # the periodic texture under priors -3, 0 and 3: all of dx = -3, 0, 3 (absolute) tie; each pixel takes the one nearest its own prior
    t = DC.texture(826, 20, 70)
    t = np.ascontiguousarray(t[:, np.arange(70) % 3])
    c["periodic_tie_under_priors_-3_0_3"] = field_case(t, t.copy(), 2, 4, np.array([-3, 0, 3], np.int16)[(u2 // 5) % 3], 0, min_score=0.8)
    # the best on the rim of a pixel's own range: the shift is (4, 1); priors (2, 0) have it at dx = +2, priors (6, 3) at dx = -2, dy = -2
    a, b = shifted(827, 20, 70, 4, 1, noise=0.0)
    alt = (u2 // 9) % 2 == 0
    c["best_on_the_rim_of_the_own_range"] = field_case(a, b, 2, 2, np.where(alt, 2, 6), np.where(alt, 0, 3), min_score=0.8)
    return c


@functools.lru_cache(maxsize=None)
def fields():
    return _fields()


@functools.lru_cache(maxsize=None)
def field_expected(name):
    """(du, dv, score, valid) of the case."""
    c = fields()[name]
    out = PO.match_field(c["a"], c["b"], c["pu"], c["pv"], c["have"], c["ask"], c["r"], c["S"], c["min_var"], c["min_score"])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def field_paths(name):
    c = fields()[name]
    out = PO.tile_paths(c["a"].shape, c["pu"], c["pv"], c["have"], c["ask"], c["r"], c["S"])
    out.setflags(write=False)
    return out


def is_constant(c):
    return c["ask"] is None and c["have"].all() and (c["pu"] == c["pu"][0, 0]).all() and (c["pv"] == c["pv"][0, 0]).all()


# ---- pairs for the pyramid ---------------------------------------------------------------------------------------------------------------------------
def pyramid_case(a, b, levels, r, S, fine, ask=None, prior=(0, 0), min_var=4, min_score=0.5, m=1, min_count=1):
    return frozen(dict(a=a, b=b, levels=levels, r=r, S=S, fine=fine, ask=ask, prior=tuple(prior), min_var=min_var, min_score=min_score, m=m, min_count=min_count))


# whole-image shifts on 65 x 193, every one beyond the single level's reach at the same search
SHIFTS = {"shift_21_-11_3_levels": ((21, -11), 3, 3, 4, 2), "shift_13_-9_3_levels": ((13, -9), 3, 2, 3, 1), "shift_6_-5_2_levels": ((6, -5), 2, 3, 4, 1),
          "shift_19_-11_at_the_reach": ((19, -11), 3, 3, 4, 1), "shift_20_-11_beyond_the_reach": ((20, -11), 3, 3, 4, 1)}


def _pyramids():
    c = {}
    for i, (name, (shift, levels, r, S, fine)) in enumerate(SHIFTS.items()):
        c[name] = pyramid_case(*shifted(900 + i, 65, 193, *shift), levels, r, S, fine)
    rng = np.random.default_rng(910)
    ask = np.where(np.arange(193)[None, :] < 128, rng.random((65, 193)) < 0.5, False).astype(np.uint8)
    for name in ("shift_13_-9_3_levels", "shift_6_-5_2_levels"):
        c[name + "_asked"] = frozen(dict(c[name], ask=ask))
    c["shift_6_-5_2_levels_prior_3_-2_m2_count3"] = frozen(dict(c["shift_6_-5_2_levels"], prior=(3, -2), m=2, min_count=3))
    c["shear_20_against_2"] = pyramid_case(*sheared(911, 64, 256, 20, 2), 3, 3, 4, 2)
    c["shear_16_against_2"] = pyramid_case(*sheared(911, 64, 256, 16, 2), 3, 3, 4, 2)
    a, b, _ = stretched(912, 64, 256, 24.0)
    c["gradient_0_to_24"] = pyramid_case(a, b, 3, 3, 4, 2)
    return c


@functools.lru_cache(maxsize=None)
def pyramids():
    return _pyramids()


@functools.lru_cache(maxsize=None)
def pyramid_expected(name):
    """((du, dv, score, valid) of level 0, the trace of `pyrflow_oracle.match_pyramid`)."""
    c = pyramids()[name]
    trace = []
    out = PO.match_pyramid(c["a"], c["b"], c["ask"], c["levels"], c["r"], c["S"], c["fine"], c["prior"], c["min_var"], c["min_score"], c["m"], c["min_count"], trace)
    for a in out:
        a.setflags(write=False)
    return out, trace


DEVICE_PYRAMIDS = ("shift_13_-9_3_levels", "shift_6_-5_2_levels", "shift_13_-9_3_levels_asked", "shift_6_-5_2_levels_asked", "shift_6_-5_2_levels_prior_3_-2_m2_count3")
