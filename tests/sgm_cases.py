"""The shared cases of the semi-global regularisation tests (tests/test_sgm_cpu.py, tests/test_gpu_sgm.py): cost volumes out of the pairs of
tests/dense_cases.py, seeded random volumes, the crafted volumes of the choice, and the three noisy scenes of the quality condition.
Expected outputs are computed once per process by the restatement (tests/sgm_oracle.py) and shared; nobody may write into them."""
import functools

import numpy as np

import dense_cases as DC
import dense_oracle as O
import sgm_oracle as S

PENALTIES = ((0, 0), (16, 128), (7, 7), (0, 4095), (4095, 4095))


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- costs ----------------------------------------------------------------------------------------------------------------------------------
def _costs():
    c = {}
    for h, w in ((15, 63), (16, 64), (17, 65), (33, 97)):
        c[f"shape_{h}x{w}"] = DC.pair(h * 100 + w, h, w, 3, 1)
    for r in (1, 3, 7):
        c[f"radius_{r}"] = DC.pair(50 + r, 33, 97, 3, r)
    for D in (1, 2, 3, 4, 5, 63, 64, 65):
        c[f"planes_{D}"] = DC.pair(40 + D, 20, 70, D, 1, step_px=1.0 if D <= 5 else 0.25)
    for D in (255, 256):
        c[f"planes_{D}"] = DC.pair(40 + D, 9, 20, D, 1, step_px=0.05)
    sweeps = DC.sweeps()
    for name in ("ref_smaller_than_window", "window_leaves_src", "nan_in_A", "constant_patch_in_ref", "constant_patch_in_src",
                 "constant_patch_in_ref_min_var_0", "constant_patch_in_src_min_var_0"):
        c[name] = sweeps[name]
    return c


@functools.lru_cache(maxsize=None)
def costs():
    return _costs()


def volume_of(c):
    return S.cost_volume(c["ref"], c["src"], c["A"], c["B"], c["w_first"], c["w_step"], c["D"], c["r"], c["min_var"])


@functools.lru_cache(maxsize=None)
def cost_oracle(name):
    return frozen(volume_of(costs()[name]))


# ---- aggregation: volumes of the restatement and seeded random ones -------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 70), (70, 1), (2, 2), (17, 65), (65, 17), (33, 33))
PLANES = (1, 3, 4, 5, 64, 255, 256)


@functools.lru_cache(maxsize=None)
def random_volume(h, w, D, seed=0):
    """uint8 [h, w, D] with a fifth of the entries 255 and some pixels all 255."""
    rng = np.random.default_rng(1000 * h + 10 * w + D + seed)
    c = rng.integers(0, 255, (h, w, D), dtype=np.uint8)
    c[rng.random((h, w, D)) < 0.2] = 255
    c[rng.random((h, w)) < 0.05] = 255
    return frozen(c)


def _aggregations():
    """name -> (volume, P1, P2, paths). Every shape at D = 5 and every D on 17 x 65 with (16, 128) and both path counts; every pair of
    penalties on 33 x 33 x 5 and on 2 x 2 x 256; two volumes of the restatement."""
    a = {}
    for h, w in SHAPES:
        for paths in (4, 8):
            a[f"random_{h}x{w}x5_p{paths}"] = (random_volume(h, w, 5), 16, 128, paths)
    for D in PLANES:
        for paths in (4, 8):
            a[f"random_17x65x{D}_p{paths}"] = (random_volume(17, 65, D), 16, 128, paths)
        a[f"random_65x17x{D}_p8"] = (random_volume(65, 17, D), 7, 7, 8)
    for P1, P2 in PENALTIES:
        a[f"random_33x33x5_P{P1}_{P2}"] = (random_volume(33, 33, 5, 1), P1, P2, 8)
        a[f"random_2x2x256_P{P1}_{P2}"] = (random_volume(2, 2, 256), P1, P2, 8)
        a[f"random_1x70x64_P{P1}_{P2}"] = (random_volume(1, 70, 64), P1, P2, 4)
    for name in ("shape_33x97", "planes_65", "window_leaves_src"):
        for paths in (4, 8):
            a[f"{name}_p{paths}"] = (cost_oracle(name), 16, 128, paths)
    return a


@functools.lru_cache(maxsize=None)
def aggregations():
    return _aggregations()


@functools.lru_cache(maxsize=None)
def aggregate_oracle(name):
    c, P1, P2, paths = aggregations()[name]
    return frozen(S.aggregate(c, P1, P2, paths))


# ---- the choice: crafted volumes ---------------------------------------------------------------------------------------------------------------
def _choices():
    """name -> dict(cost, sum, w_first, w_step, min_score)."""
    c = {}

    def case(cost, total, w_first=0.08, w_step=0.01, min_score=-2.0):
        return dict(cost=np.ascontiguousarray(cost, np.uint8), sum=np.ascontiguousarray(total, np.uint16), w_first=w_first, w_step=w_step, min_score=min_score)

    for name in ("all_planes_tie", "best_at_first_plane", "best_at_last_plane", "every_score_kept"):
        p = DC.sweeps()[name]
        vol = volume_of(p)
        c[name] = case(vol, S.aggregate(vol, 16, 128, 8), p["w_first"], p["w_step"], p["min_score"])
    rng = np.random.default_rng(11)
    h, w, D = 9, 37, 7
    cost = rng.integers(0, 200, (h, w, D), dtype=np.uint8)
    total = rng.integers(100, 30000, (h, w, D)).astype(np.uint16)
    k = rng.integers(1, D - 1, (h, w))
    ii, jj = np.indices((h, w))
    total[ii, jj, k] = 50                                         # the least sum at an inner plane
    lonely = cost.copy()
    lonely[ii, jj, np.where(rng.random((h, w)) < 0.5, k - 1, k + 1)] = 255
    c["invalid_neighbour"] = case(lonely, total)
    flat = total.copy()
    flat[...] = 777                                               # den = 0 everywhere, and every plane ties
    c["flat_sum"] = case(cost, flat)
    concave = total.copy()
    concave[ii, jj, k - 1] = 50
    concave[ii, jj, k + 1] = 50                                   # ties at k - 1, k, k + 1: the lower wins, its den may be <= 0
    c["ties_between_neighbours"] = case(cost, concave)
    c["min_score_drops"] = case(cost, total, min_score=0.3)       # 1 - c / 127 < 0.3 for c >= 89
    dead = cost.copy()
    dead[rng.random((h, w)) < 0.3] = 255
    dead[0, 0] = 255
    c["all_invalid_pixels"] = case(dead, total)
    valid_is_not_least = cost.copy()
    valid_is_not_least[ii, jj, k] = 255                           # the least sum belongs to an invalid plane: the next one wins
    c["least_sum_is_invalid"] = case(valid_is_not_least, total)
    big = rng.integers(0, 255, (5, 19, 256), dtype=np.uint8)
    c["planes_256"] = case(big, rng.integers(0, 34801, (5, 19, 256)).astype(np.uint16))
    c["one_plane"] = case(rng.integers(0, 256, (6, 21, 1), dtype=np.uint8), rng.integers(0, 2041, (6, 21, 1)).astype(np.uint16))
    c["one_pixel"] = case(cost[:1, :1], total[:1, :1])
    for v in c.values():
        frozen(v["cost"], v["sum"])
    return c


@functools.lru_cache(maxsize=None)
def choices():
    return _choices()


@functools.lru_cache(maxsize=None)
def choose_oracle(name):
    c = choices()[name]
    return frozen(*S.choose(c["cost"], c["sum"], c["w_first"], c["w_step"], c["min_score"]))


# ---- the noisy scenes of the quality condition --------------------------------------------------------------------------------------------------
NOISY = {200: dict(h0=33, w0=97, D=17, r=1, slant=(0.0, 0.0), sigma=12.0), 201: dict(h0=33, w0=97, D=17, r=1, slant=(0.03, 0.05), sigma=12.0),
         202: dict(h0=40, w0=70, D=33, r=2, slant=(0.05, -0.08), sigma=16.0)}
CONTRAST = 0.25
P1, P2, PATHS = 16, 128, 8


def low_contrast(img):
    """The image at a quarter of its contrast about grey level 128."""
    return np.clip(np.rint(128.0 + CONTRAST * (img.astype(np.float64) - 128.0)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def noisy(seed):
    """`dense_cases.pair(seed, ...)` with both images at contrast 0.25 and Gaussian noise of `sigma` grey levels added to ref only."""
    n = NOISY[seed]
    c = DC.pair(seed, n["h0"], n["w0"], n["D"], n["r"], slant=n["slant"], min_var=0, min_score=-2.0)
    rng = np.random.default_rng(seed + 1)
    ref = low_contrast(c["ref"]).astype(np.float64) + rng.normal(0.0, n["sigma"], c["ref"].shape)
    c["ref"] = np.clip(np.rint(ref), 0, 255).astype(np.uint8)
    c["src"] = low_contrast(c["src"])
    frozen(c["ref"], c["src"])
    return c


@functools.lru_cache(maxsize=None)
def noisy_oracle(seed):
    """(winner-take-all maps, regularised maps) of a noisy scene."""
    c = noisy(seed)
    valid, s = O.scores(c["ref"], c["src"], c["A"], c["B"], c["w_first"], c["w_step"], c["D"], c["r"], c["min_var"])
    wta = O.choose(valid, s, c["w_first"], c["w_step"], c["min_score"])
    cost = S.quantise(valid, s)
    sgm = S.choose(cost, S.aggregate(cost, P1, P2, PATHS), c["w_first"], c["w_step"], c["min_score"])
    return frozen(*wta), frozen(*sgm)


def share_within_one_plane(plane, c):
    """The share of the interior pixels (window inside ref) whose plane lies within one of the true one; a dropped pixel counts as wrong."""
    r = c["r"]
    p, t = plane[r:-r, r:-r].astype(np.float64), c["k_true"][r:-r, r:-r]
    return float(((p >= 0) & (np.abs(p - t) <= 1.0)).mean())
