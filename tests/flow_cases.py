"""The shared cases of the dense-displacement tests (tests/test_flow_cpu.py, tests/test_gpu_flow.py): matches, checks and lifts, built from
`dense_cases.texture` and small crafted maps. A case is everything an entry point takes. Expected outputs are computed once per process by
the restatement (tests/flow_oracle.py) and shared; nobody may write into them.

The match kernel's block owns a 64 x 16 tile: 15 x 63, 16 x 64, 17 x 65 and 33 x 97 lie on, beside and beyond its edges; 1 x 70, 70 x 1 and
5 x 9 hold no window at all."""
import functools

import numpy as np

import dense_cases as DC
import flow_oracle as FO

M = 24            # the margin of the texture around image a: shifts up to 24 px show texture everywhere


def shifted(seed, h, w, sx, sy, noise=0.0):
    """(a, b) [h, w] uint8 with b(x + sx, y + sy) = a(x, y): two cuts of one seeded texture; `noise`: Gaussian noise added to b."""
    t = DC.texture(seed, h + 2 * M, w + 2 * M)
    a, b = t[M:M + h, M:M + w], t[M - sy:M - sy + h, M - sx:M - sx + w]
    if noise:
        rng = np.random.default_rng(seed + 1000)
        b = np.clip(np.rint(b.astype(np.float64) + rng.normal(0.0, noise, b.shape)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def frozen(d):
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            d[k] = np.ascontiguousarray(v)
            d[k].setflags(write=False)
    return d


def match_case(a, b, r, S, prior=(0, 0), min_var=4, min_score=0.8, ask=None):
    return frozen(dict(a=a, b=b, r=r, S=S, prior=tuple(prior), min_var=min_var, min_score=min_score, ask=ask))


def _matches():
    c = {}
    # shapes on, beside and beyond the tile's edges; r in {1, 3, 7, 15}; S in {0, 1, 4, 16}, the largest of both together once
    for (h, w), r, S, (sx, sy) in (((15, 63), 1, 0, (0, 0)), ((16, 64), 3, 1, (1, -1)), ((17, 65), 7, 4, (-3, 1)), ((33, 97), 3, 4, (2, 3)),
                                   ((33, 97), 15, 1, (1, 0)), ((17, 65), 1, 16, (-11, 5)), ((16, 64), 1, 4, (4, -4)), ((15, 63), 3, 0, (0, 0))):
        c[f"shape_{h}x{w}_r{r}_S{S}"] = match_case(*shifted(h * 100 + w + r + S, h, w, sx, sy, noise=2.0), r, S, min_score=0.5)
    c["largest_r15_S16_40x80"] = match_case(*shifted(300, 40, 80, 9, -6, noise=2.0), 15, 16, min_score=0.5)
    for h, w in ((1, 70), (70, 1)):
        c[f"shape_{h}x{w}"] = match_case(*shifted(310 + h, h, w, 0, 0), 1, 1)
    c["image_smaller_than_window"] = match_case(*shifted(312, 5, 9, 0, 0), 3, 2)
    c["prior_4_-2_shift_5_-3"] = match_case(*shifted(313, 33, 97, 5, -3, noise=2.0), 3, 2, prior=(4, -2), min_score=0.5)
    c["prior_-12_9_shift_-13_10"] = match_case(*shifted(314, 20, 70, -13, 10), 2, 1, prior=(-12, 9))
    c["prior_pushes_every_window_out"] = match_case(*shifted(315, 20, 70, 0, 0), 2, 4, prior=(4096, -4096))
    c["prior_leaves_a_strip"] = match_case(*shifted(316, 20, 70, 0, 0), 2, 2, prior=(60, 0), min_score=-1.0)      # only the left columns find b
    for name, which in (("constant_patch_in_a", 0), ("constant_patch_in_b", 1)):
        pair = [x.copy() for x in shifted(317 + which, 20, 70, 1, 1)]
        pair[which][4:16, 10:40] = 128 if which == 0 else 77
        c[name] = match_case(*pair, 2, 2)
        c[name + "_min_var_0"] = match_case(*pair, 2, 2, min_var=0)
    a, b = shifted(319, 33, 97, 2, -1, noise=2.0)
    c["mask_asks_for_nothing"] = match_case(a, b, 3, 4, ask=np.zeros((33, 97), np.uint8), min_score=0.5)
    one = np.zeros((33, 97), np.uint8)
    for y0 in range(0, 33, DC.TILE_H):
        for x0 in range(0, 97, DC.TILE_W):
            one[min(y0 + 5, 32), min(x0 + 10, 96)] = 1
    c["mask_one_pixel_per_tile"] = match_case(a, b, 3, 4, ask=one, min_score=0.5)
    rng = np.random.default_rng(320)
    c["mask_random_and_one_empty_tile"] = match_case(a, b, 3, 4, ask=np.where(np.arange(97)[None, :] < 64, rng.integers(0, 2, (33, 97)), 0).astype(np.uint8),
                                                     min_score=0.5)
    # a texture with a period of 3 px along x under a zero shift: dx = 0, -3, +3 tie exactly and the tie must go to the smallest displacement
    t = DC.texture(321, 20, 70)
    t = np.ascontiguousarray(t[:, np.arange(70) % 3])
    c["periodic_tie"] = match_case(t, t.copy(), 2, 4)
    # the best candidate on the rim of the search range: no offset is taken along that axis
    c["best_on_the_rim_along_x"] = match_case(*shifted(322, 20, 70, 4, 1), 2, 4)
    c["best_on_the_rim_along_y"] = match_case(*shifted(323, 20, 70, -1, -4), 2, 4)
    c["every_score_kept"] = match_case(*shifted(324, 17, 65, 2, 2, noise=30.0), 1, 2, min_score=-2.0)
    return c


@functools.lru_cache(maxsize=None)
def matches():
    return _matches()


@functools.lru_cache(maxsize=None)
def candidates(name):
    c = matches()[name]
    return FO.candidate_scores(c["a"], c["b"], c["r"], c["S"], c["prior"], c["min_var"])


@functools.lru_cache(maxsize=None)
def match_expected(name):
    """(du, dv, score, valid) of the case."""
    c = matches()[name]
    out = FO.match(c["a"], c["b"], c["ask"], c["r"], c["S"], c["prior"], c["min_var"], c["min_score"])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def backward_expected(name):
    """The backward field of a match case: b into a with the negated prior, every pixel asked."""
    c = matches()[name]
    out = FO.match(c["b"], c["a"], None, c["r"], c["S"], (-c["prior"][0], -c["prior"][1]), c["min_var"], c["min_score"])
    for a in out:
        a.setflags(write=False)
    return out


# ---- checks ---------------------------------------------------------------------------------------------------------------------------------------
FROM_MATCH = ("shape_33x97_r3_S4", "prior_4_-2_shift_5_-3", "shape_17x65_r1_S16", "constant_patch_in_b", "mask_one_pixel_per_tile", "shape_1x70")


def check_case(fwd, bwd, tol):
    return frozen(dict(du=fwd[0], dv=fwd[1], valid=fwd[3], du_b=bwd[0], dv_b=bwd[1], valid_b=bwd[3], tol=tol))


def crafted_field(seed, h, w, spread=3.0, p_valid=0.8):
    rng = np.random.default_rng(seed)
    valid = (rng.random((h, w)) < p_valid).astype(np.uint8)
    return (np.where(valid, rng.uniform(-spread, spread, (h, w)), 0.0), np.where(valid, rng.uniform(-spread, spread, (h, w)), 0.0),
            np.where(valid, rng.random((h, w)), 0.0).astype(np.float32), valid)


def _checks():
    c = {}
    for name in FROM_MATCH:
        c["from_match_" + name] = check_case(match_expected(name), backward_expected(name), 1.0)
    for (h, w), tol in (((15, 63), 1.0), ((33, 97), 2.5), ((1, 70), 4.0), ((70, 1), 0.5)):
        c[f"crafted_{h}x{w}"] = check_case(crafted_field(400 + h, h, w), crafted_field(401 + h, h, w), tol)
    h, w = 17, 65
    full = np.ones((h, w), np.uint8)
    zero = np.zeros((h, w))
    # the backward field is invalid wherever the forward one lands (two columns to the right), valid elsewhere
    vb = full.copy()
    vb[:, 20:40] = 0
    c["backward_hit_on_an_invalid_pixel"] = check_case((zero + 2.0, zero, None, full), (zero - 2.0, zero, None, vb), 1.0)
    # hits outside the image on every side; rint(u + du) = -1 and = w are outside, -0.5 rounds to -0 and is inside
    du = np.where(np.arange(w)[None, :] < 8, -8.5, np.where(np.arange(w)[None, :] >= w - 8, 8.5, 0.0)) + zero
    dv = np.where(np.arange(h)[:, None] < 3, -3.5, np.where(np.arange(h)[:, None] >= h - 3, 3.5, 0.0)) + zero
    c["hit_outside_the_image"] = check_case((du, dv, None, full), (-du, -dv, None, full), 1.0)
    # the sum exactly at tol on the even columns (kept) and one unit in the last place above on the odd ones (dropped)
    du_b = np.where(np.arange(w)[None, :] % 2 == 0, -2.0, np.nextafter(-2.0, 0.0)) + zero
    c["sum_exactly_at_tol"] = check_case((zero + 3.0, zero, None, full), (du_b, zero, None, full), 1.0)
    c["sum_exactly_at_tol_3_4_5"] = check_case((zero + 3.0, zero + 4.0, None, full), (zero, zero, None, full), 5.0)
    nan = crafted_field(410, h, w)
    du = nan[0].copy()
    du[::3, ::5] = np.nan
    dvb = crafted_field(411, h, w)
    dub = dvb[0].copy()
    dub[1::3, 1::5] = np.nan
    c["nan_fails"] = check_case((du, nan[1], None, nan[3]), (dub, dvb[1], None, dvb[3]), 100.0)
    return c


@functools.lru_cache(maxsize=None)
def checks():
    return _checks()


@functools.lru_cache(maxsize=None)
def check_expected(name):
    c = checks()[name]
    out = FO.check(c["du"], c["dv"], c["valid"], c["du_b"], c["dv_b"], c["valid_b"], c["tol"])
    out.setflags(write=False)
    return out


# ---- lifts ----------------------------------------------------------------------------------------------------------------------------------------
def cameras(h, w):
    """Epoch A's camera and epoch B's, which stands somewhere else: [21] = inv(K), R, t each."""
    K = np.array([[DC.F, 0.0, w / 2.0], [0.0, DC.F, h / 2.0], [0.0, 0.0, 1.0]])
    c, s = np.cos(0.01), np.sin(0.01)
    Rb = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]) @ DC.R_WORLD
    return FO.camera(K, DC.R_WORLD, DC.T_WORLD), FO.camera(K + np.array([[0.5, 0.0, 0.25], [0.0, 0.5, -0.25], [0.0, 0.0, 0.0]]), Rb, DC.T_WORLD + np.array([0.02, -0.01, 0.03]))


def lift_case(seed, h, w, w_step=0.001, max_diff=2.0, hb=None, wb=None, rough=0.0004, **change):
    rng = np.random.default_rng(seed)
    hb, wb = hb or h, wb or w
    du, dv, _, valid = crafted_field(seed + 1, h, w)
    plane_a = rng.integers(-1, 6, (h, w)).astype(np.int16)
    plane_b = np.where(rng.random((hb, wb)) < 0.05, -1, rng.integers(0, 6, (hb, wb))).astype(np.int16)
    uu, vv = np.meshgrid(np.arange(wb), np.arange(hb))
    d = dict(du=du, dv=dv, valid=valid, keep=(rng.random((h, w)) < 0.8).astype(np.uint8), plane_a=plane_a,
             w_a=np.where(plane_a >= 0, 0.1 + 0.004 * rng.random((h, w)), 0.0), plane_b=plane_b,
             w_b=np.where(plane_b >= 0, 0.1 + 0.0002 * uu - 0.0001 * vv + rough * rng.random((hb, wb)), 0.0),
             keep_b=(rng.random((hb, wb)) < 0.95).astype(np.uint8), w_step_b=w_step, max_diff=max_diff)
    d["cam_a"], d["cam_b"] = cameras(h, w)
    d.update(change)
    return frozen(d)


def _lifts():
    c = {}
    for h, w in ((15, 63), (16, 64), (17, 65), (33, 97), (1, 70), (70, 1)):
        c[f"shape_{h}x{w}"] = lift_case(500 + h, h, w)
    c["map_b_of_another_shape"] = lift_case(510, 17, 65, hb=20, wb=50)
    c["negative_w_step_b"] = lift_case(511, 17, 65, w_step=-0.001)
    c["rough_map_b_gated_by_max_diff"] = lift_case(512, 33, 97, rough=0.004, max_diff=1.5)
    h, w = 17, 65
    full, zero = np.ones((h, w), np.uint8), np.zeros((h, w))
    flat = dict(valid=full, keep=full, plane_a=np.zeros((h, w), np.int16), w_a=zero + 0.25, plane_b=np.zeros((h, w), np.int16), w_b=zero + 0.25, keep_b=full,
                dv=zero + 0.25)
    # taps outside: the last columns are pushed beyond the map; an integer x in the last column has its right tap (of weight zero) outside
    du = zero + 0.5
    du[:, -3:] = 10.0
    du[:, -6] = 5.0                      # x = w - 1 exactly: not lifted
    du[:, -7] = 5.0                      # x = w - 2 exactly: lifted
    du[:, :2] = -2.5                     # x < 0
    c["a_tap_outside_and_an_integer_x_in_the_last_column"] = lift_case(513, h, w, **dict(flat, du=du))
    plane_b = np.zeros((h, w), np.int16)
    plane_b[5:8, 20:30] = -1
    keep_b = full.copy()
    keep_b[10:13, 40:50] = 0
    c["a_tap_dropped_and_a_tap_not_kept"] = lift_case(514, h, w, **dict(flat, du=zero + 0.5, plane_b=plane_b, keep_b=keep_b))
    # the span exactly at max_diff |w_step| (lifted) and one unit in the last place above (not lifted): w_step = 2^-10, max_diff = 2
    w_b = zero + 0.25
    w_b[4, 10:30:4] = 0.25 + 2.0 ** -9
    w_b[12, 10:30:4] = np.nextafter(0.25 + 2.0 ** -9, 1.0)
    for name, step in (("span_exactly_at_and_just_above_max_diff", 2.0 ** -10), ("span_exactly_at_and_just_above_max_diff_negative_step", -(2.0 ** -10))):
        c[name] = lift_case(515, h, w, w_step=step, max_diff=2.0, **dict(flat, du=zero + 0.5, w_b=w_b))
    return c


@functools.lru_cache(maxsize=None)
def lifts():
    return _lifts()


LIFT_ARGS = ("du", "dv", "valid", "keep", "plane_a", "w_a", "cam_a", "plane_b", "w_b", "keep_b", "cam_b", "w_step_b", "max_diff")


@functools.lru_cache(maxsize=None)
def lift_expected(name):
    c = lifts()[name]
    out = FO.lift(*(c[k] for k in LIFT_ARGS))
    for a in out:
        a.setflags(write=False)
    return out
