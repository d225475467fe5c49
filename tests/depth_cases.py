"""The shared cases of the depth-map clean-up tests (tests/test_depth_clean_cpu.py, tests/test_gpu_depth_clean.py): plane maps for the
labelling, maps with speckles, maps with holes, and the chain on the three noisy scenes of tests/sgm_cases.py. Expected outputs are computed
once per process by the restatement (tests/depth_oracle.py) and shared; nobody may write into them.

The labelling block owns a 64 x 16 tile (`im_depth_tile_w/h`): the shapes lie on, beside and beyond its edges, 3 x 3 tiles and more."""
import functools

import numpy as np

import depth_oracle as DO
import sgm_cases as SC

TILE_W, TILE_H = 64, 16
H3, W3 = 3 * TILE_H, 3 * TILE_W


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def random_planes(h, w, density, seed, planes=4):
    """int16 [h, w]: a pixel holds a plane of 0..planes-1 with probability `density`, else -1."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, planes, (h, w)).astype(np.int16)
    p[rng.random((h, w)) >= density] = -1
    return p


def serpentine(h, w):
    """A path one pixel wide: every even row, joined to the next at alternating ends. It crosses every vertical tile edge in every even row."""
    p = np.full((h, w), -1, np.int16)
    p[0::2] = 2
    for k, y in enumerate(range(1, h - 1, 2)):
        p[y, w - 1 if k % 2 == 0 else 0] = 2
    return p


def spiral(h, w):
    """A path one pixel wide that winds inwards from (0, 0), one pixel apart from its earlier turns."""
    g = np.full((h, w), -1, np.int16)
    y = x = d = turns = 0
    g[0, 0] = 1
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    inside = lambda v, u: 0 <= v < h and 0 <= u < w  # noqa: E731
    while turns < 2:
        dy, dx = dirs[d]
        ok = inside(y + dy, x + dx) and g[y + dy, x + dx] < 0 and (not inside(y + 2 * dy, x + 2 * dx) or g[y + 2 * dy, x + 2 * dx] < 0)
        if ok:
            y, x, turns = y + dy, x + dx, 0
            g[y, x] = 1
        else:
            d, turns = (d + 1) % 4, turns + 1
    return g


# ---- labelling: name -> (plane, mode, max_diff) ---------------------------------------------------------------------------------------------
def _labellings():
    c = {}
    shapes = ((1, 1), (1, 70), (70, 1), (2, 2), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (3 * TILE_H + 5, 3 * TILE_W + 7))
    for h, w in shapes:
        for mode in (0, 1):
            c[f"shape_{h}x{w}_mode{mode}"] = (random_planes(h, w, 0.7, 100 * h + w), mode, 1)
    c["one_component_3x3_tiles"] = (np.full((H3, W3), 3, np.int16), 0, 0)
    c["one_hole_3x3_tiles"] = (np.full((H3, W3), -1, np.int16), 1, 0)
    yy, xx = np.indices((H3, W3))
    c["checkerboard"] = (np.where((yy + xx) % 2 == 0, 0, 100).astype(np.int16), 0, 1)
    c["checkerboard_joined_at_100"] = (c["checkerboard"][0], 0, 100)
    for mode in (0, 1):
        c[f"serpentine_mode{mode}"] = (serpentine(H3, W3), mode, 0)
        c[f"serpentine_transposed_mode{mode}"] = (np.ascontiguousarray(serpentine(W3, H3).T), mode, 0)
        c[f"spiral_mode{mode}"] = (spiral(H3, W3), mode, 0)
    corner = np.full((2 * TILE_H, 2 * TILE_W), -1, np.int16)
    corner[:TILE_H, :TILE_W] = 1
    corner[TILE_H:, TILE_W:] = 1
    c["tiles_meet_at_a_corner"] = (corner, 0, 1)
    c["holes_meet_at_a_corner"] = (np.where(corner < 0, 1, -1).astype(np.int16), 1, 0)
    h, w = TILE_H + 3, TILE_W + 2                                    # partial tiles on the right and below
    bridge = np.full((h, w), 1, np.int16)
    bridge[TILE_H, :w - 1] = -1                                      # a wall but for the last column, in the first row of the lower tiles
    c["joined_through_the_last_column"] = (bridge, 0, 1)
    bridge = np.full((h, w), 1, np.int16)
    bridge[:h - 1, TILE_W] = -1                                      # a wall but for the last row, in the first column of the right tiles
    c["joined_through_the_last_row"] = (bridge, 0, 1)
    chain = np.full((3, 9), -1, np.int16)
    chain[1, :3] = (3, 4, 5)                                         # one component at max_diff = 1: joining is transitive
    chain[1, 4:6] = (3, 5)                                           # two
    c["chain_345_against_pair_35"] = (chain, 0, 1)
    exact = np.full((3, 9), -1, np.int16)
    exact[1, :2] = (10, 17)                                          # a difference of exactly max_diff
    exact[1, 3:5] = (10, 18)                                         # and of max_diff + 1
    exact[0, 7], exact[1, 7] = 4095, 0                               # the largest difference there is
    c["difference_of_exactly_max_diff"] = (exact, 0, 7)
    c["difference_of_4095"] = (exact, 0, 4095)
    for density in (0.3, 0.6, 0.9):
        for mode in (0, 1):
            c[f"random_65x130_density_{density}_mode{mode}"] = (random_planes(65, 130, density, int(density * 10)), mode, 1)
    for mode in (0, 1):
        c[f"all_invalid_mode{mode}"] = (np.full((20, 70), -1, np.int16), mode, 1)
        c[f"all_valid_mode{mode}"] = (np.full((20, 70), 5, np.int16), mode, 1)
    for v in c.values():
        frozen(v[0])
    return c


@functools.lru_cache(maxsize=None)
def labellings():
    return _labellings()


@functools.lru_cache(maxsize=None)
def label_oracle(name):
    plane, mode, max_diff = labellings()[name]
    return frozen(*DO.components(plane, mode, max_diff))


# ---- maps: a surface with its w and score ----------------------------------------------------------------------------------------------------
W_FIRST, W_STEP = 0.08, 0.01


def surface(h, w, seed, slant=(0.02, 0.03), D=12, w_first=W_FIRST, w_step=W_STEP):
    """(plane, w, score) of a slanted surface: w = w_first + k w_step with k affine in (x, y) plus a little noise, plane = the nearest."""
    rng = np.random.default_rng(seed)
    yy, xx = np.indices((h, w))
    k = np.clip(D / 2.0 + slant[0] * (xx - w / 2.0) + slant[1] * (yy - h / 2.0) + 0.2 * rng.normal(size=(h, w)), 0.0, D - 1.0)
    return np.rint(k).astype(np.int16), w_first + k * w_step, (0.5 + 0.5 * rng.random((h, w))).astype(np.float32)


def punch(maps, mask):
    """The maps with the pixels of `mask` dropped as the sweep drops them."""
    plane, w, score = maps
    return np.where(mask, -1, plane).astype(np.int16), np.where(mask, 0.0, w), np.where(mask, 0.0, score).astype(np.float32)


# ---- speckles: name -> dict(plane, w, score, min_size, max_diff) -------------------------------------------------------------------------------
def _speckles():
    c = {}

    def case(maps, min_size, max_diff):
        return dict(plane=maps[0], w=maps[1], score=maps[2], min_size=min_size, max_diff=max_diff)

    m = surface(20, 70, 1, slant=(0.0, 0.0))
    keep = np.zeros((20, 70), bool)
    keep[2, 3:8] = True                                              # five pixels: exactly min_size, kept
    keep[5, 3:7] = True                                              # four: min_size - 1, dropped
    keep[8:10, 20:23] = True                                         # six
    keep[12, 40] = True                                              # one
    flat = (np.full((20, 70), 4, np.int16), m[1], m[2])
    c["sizes_min_size_and_one_less"] = case(punch(flat, ~keep), 5, 1)
    c["min_size_1_drops_nothing"] = case(punch(surface(33, 97, 2), random_planes(33, 97, 0.5, 3) < 0), 1, 1)
    c["random_65x130"] = case(punch(surface(65, 130, 4, slant=(0.05, 0.08)), random_planes(65, 130, 0.6, 5) < 0), 4, 1)
    c["random_3x3_tiles_plus"] = case(punch(surface(H3 + 5, W3 + 7, 6, slant=(0.03, 0.1)), random_planes(H3 + 5, W3 + 7, 0.62, 7) < 0), 16, 0)
    c["all_invalid"] = case(punch(surface(20, 70, 8), np.ones((20, 70), bool)), 16, 1)
    c["all_valid_one_component"] = case(flat, 16, 1)
    c["all_valid_dropped_whole"] = case(flat, 20 * 70 + 1, 1)
    c["largest_min_size"] = case(flat, 2 ** 31 - 1, 1)
    for v in c.values():
        frozen(v["plane"], v["w"], v["score"])
    return c


@functools.lru_cache(maxsize=None)
def speckles():
    return _speckles()


@functools.lru_cache(maxsize=None)
def speckle_oracle(name):
    """(size of mode 0, plane, w, score, count)."""
    c = speckles()[name]
    _, size = DO.components(c["plane"], 0, c["max_diff"])
    plane, w, score, count = DO.drop_small(c["plane"], c["w"], c["score"], size, c["min_size"])
    return frozen(size, plane, w, score) + (count,)


# ---- holes: name -> dict(plane, w, score, max_hole, max_diff, w_first, w_step, D[, speckle]) ---------------------------------------------------
def _holes():
    c = {}

    def case(maps, max_hole=64, max_diff=2, w_first=W_FIRST, w_step=W_STEP, D=12, speckle=None):
        return dict(plane=maps[0], w=np.ascontiguousarray(maps[1], np.float64), score=maps[2], max_hole=max_hole, max_diff=max_diff, w_first=w_first,
                    w_step=w_step, D=D, speckle=speckle)

    h, w = 40, 150
    mask = np.zeros((h, w), bool)
    mask[0:3, 20:23] = True                                          # touches the first row
    mask[h - 2:h, 50:52] = True                                      # the last row
    mask[10:12, 0:2] = True                                          # the first column
    mask[20:23, w - 1] = True                                        # the last column
    mask[25:28, 100:104] = True                                      # none: filled
    c["holes_at_the_four_borders"] = case(punch(surface(h, w, 10), mask))
    mask = np.zeros((h, w), bool)
    mask[TILE_H - 2:TILE_H + 2, TILE_W - 2:TILE_W + 2] = True        # over the corner of four tiles
    mask[2 * TILE_H - 1:2 * TILE_H + 1, 100:103] = True              # over a row edge
    c["hole_over_tile_edges"] = case(punch(surface(h, w, 11), mask))
    mask = np.zeros((h, w), bool)
    mask[5:8, 10:14] = True                                          # twelve pixels: exactly max_hole, filled
    mask[5:8, 30:34] = True
    mask[8, 30] = True                                               # thirteen: not
    c["sizes_max_hole_and_one_more"] = case(punch(surface(h, w, 12), mask), max_hole=12)
    steps = np.full((h, w), 3, np.int16)
    steps[:, 40:80] = 5
    steps[:, 80:] = 6
    steps[:, 120:] = 3
    flat = (steps, W_FIRST + steps * W_STEP, surface(h, w, 13)[2])
    mask = np.zeros((h, w), bool)
    mask[10:13, 38:42] = True                                        # rim 3 and 5: exactly max_diff
    mask[10:13, 118:122] = True                                      # rim 6 and 3: max_diff + 1
    mask[20:22, 78:82] = True                                        # rim 5 and 6
    c["rim_spread_max_diff_and_one_more"] = case(punch(flat, mask))
    mask = np.zeros((h, w), bool)
    mask[10:16, 60] = True                                           # an L over a tile edge: every pixel has anchors of its own
    mask[15, 60:70] = True
    c["l_shaped_hole"] = case(punch(surface(h, w, 14, slant=(0.04, 0.06)), mask))
    mask = np.zeros((h, w), bool)
    mask[10:15, 20:26] = True
    mask[12, 22:24] = False                                          # an island of two pixels inside the hole: the speckle step removes it first
    c["hole_with_an_island"] = case(punch(surface(h, w, 15, slant=(0.0, 0.0)), mask), speckle=(3, 1))
    c["hole_with_an_island_kept"] = case(punch(surface(h, w, 15, slant=(0.0, 0.0)), mask))
    mask = np.zeros((h, w), bool)
    mask[7, 7] = mask[20, 64] = mask[16, 100] = mask[1, 1] = mask[h - 2, w - 2] = True
    c["one_pixel_holes"] = case(punch(surface(h, w, 16), mask), max_hole=1)
    mask = np.zeros((h, w), bool)
    mask[10:12, 10:13] = mask[25:27, 130:133] = True
    far = surface(h, w, 17, slant=(0.1, 0.0), D=16)                  # planes up to 15 on the right, but the schedule handed in has six: the plane is cut at 5
    c["plane_beyond_the_schedule"] = case(punch(far, mask), D=6, max_diff=4095)
    c["plane_before_the_schedule"] = case(punch(far, mask), w_first=W_FIRST + 9 * W_STEP, D=6)       # on the left w < w_first: the plane is cut at 0
    neg = surface(h, w, 18, w_first=0.5, w_step=-0.01)
    c["negative_w_step"] = case(punch(neg, mask), w_first=0.5, w_step=-0.01)
    ties = np.full((5, 9), 2, np.int16)
    ties[:, 3:] = 3
    ties[:, 6:] = 4
    tw = ties.astype(np.float64)                                     # w_first = 0, w_step = 1: w is the plane, halves are exact
    mask = np.zeros((5, 9), bool)
    mask[1, 2] = mask[3, 5] = True
    tw[1, 1], tw[1, 3], tw[0, 2], tw[2, 2] = 2.0, 3.0, 2.0, 3.0      # (1, 2): a = b = 2.5 -> plane 2
    tw[3, 4], tw[3, 6], tw[2, 5], tw[4, 5] = 3.0, 4.0, 3.0, 4.0      # (3, 5): a = b = 3.5 -> plane 4
    c["ties_round_to_even"] = case(punch((ties, tw, np.ones((5, 9), np.float32)), mask), w_first=0.0, w_step=1.0, D=8)
    c["all_invalid"] = case(punch(surface(20, 70, 19), np.ones((20, 70), bool)))
    c["all_valid"] = case(surface(20, 70, 20))
    c["random_65x130"] = case(punch(surface(65, 130, 21, slant=(0.03, 0.05)), random_planes(65, 130, 0.85, 22) < 0))
    c["random_3x3_tiles_plus"] = case(punch(surface(H3 + 5, W3 + 7, 23, slant=(0.02, 0.08)), random_planes(H3 + 5, W3 + 7, 0.7, 24) < 0), max_hole=9, max_diff=1)
    c["largest_limits"] = case(punch(surface(65, 130, 25), random_planes(65, 130, 0.6, 26) < 0), max_hole=4096, max_diff=4095)
    for v in c.values():
        frozen(v["plane"], v["w"], v["score"])
    return c


@functools.lru_cache(maxsize=None)
def holes():
    return _holes()


@functools.lru_cache(maxsize=None)
def hole_input(name):
    """The maps `fill_holes` sees: the case's own, after its speckle step where it has one."""
    c = holes()[name]
    if c["speckle"] is None:
        return c["plane"], c["w"], c["score"]
    return frozen(*DO.remove_speckles(c["plane"], c["w"], c["score"], *c["speckle"])[:3])


@functools.lru_cache(maxsize=None)
def hole_oracle(name):
    """(label of mode 1, size of mode 1, plane, w, score, filled, count) on `hole_input`."""
    c = holes()[name]
    plane, w, score = hole_input(name)
    label, size = DO.components(plane, 1, 0)
    out = DO.fill_holes(plane, w, score, c["max_hole"], c["max_diff"], c["w_first"], c["w_step"], c["D"], label, size)
    return frozen(label, size, *out[:4]) + (out[4],)


# ---- the noisy scenes: the chain on the winner-take-all maps -----------------------------------------------------------------------------------
SPECKLE, HOLES = (16, 1), (64, 2)


@functools.lru_cache(maxsize=None)
def noisy_chain(seed):
    """(maps without speckles, maps with the holes filled, filled) of the winner-take-all maps of `sgm_cases.noisy(seed)`."""
    c = SC.noisy(seed)
    wta, _ = SC.noisy_oracle(seed)
    clean = DO.remove_speckles(*wta, *SPECKLE)[:3]
    out = DO.fill_holes(*clean, *HOLES, c["w_first"], c["w_step"], c["D"])
    return frozen(*clean), frozen(*out[:3]), frozen(out[3])


def right_and_wrong(plane, c):
    """The interior pixels (window inside ref) that hold a plane within one of the true one, and those that hold one farther off."""
    r = c["r"]
    p, t = plane[r:-r, r:-r].astype(np.float64), c["k_true"][r:-r, r:-r]
    held = p >= 0
    return held & (np.abs(p - t) <= 1.0), held & (np.abs(p - t) > 1.0)
