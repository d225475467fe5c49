"""The shared cases of the slanted-window refinement tests (tests/test_refine_cpu.py, tests/test_gpu_refine.py), built from
`dense_cases.pair` / `render` / `two_maps` and swept with the restatement. A case is everything both entry points take: the pair (ref,
src, A, B), a map (plane, w, score) with its step, and the options of the slant (R, max_diff, min_count) and of the refinement (r,
min_var, span, sub). Expected outputs are computed once per process and shared; nobody may write into them.

The kernels' block owns a 64 x 16 tile: 15 x 63, 16 x 64, 17 x 65 and 33 x 97 lie on, beside and beyond its edges; 1 x 70 and 70 x 1 have
neighbourhoods on one line (det = 0)."""
import functools

import numpy as np

import dense_cases as DC
import dense_oracle as O
import refine_oracle as RO


def swept(c):
    return O.sweep(c["ref"], c["src"], c["A"], c["B"], c["w_first"], c["w_step"], c["D"], c["r"], c["min_var"], c["min_score"])


def crafted_map(c, seed, dropped=True):
    """A map no sweep made: random planes (some dropped), inverse depths within 0.4 steps of them."""
    rng = np.random.default_rng(seed)
    shape = c["ref"].shape
    plane = rng.integers(-1 if dropped else 0, c["D"], shape).astype(np.int16)
    w = c["w_first"] + (plane + rng.uniform(-0.4, 0.4, shape)) * c["w_step"]
    return plane, np.where(plane >= 0, w, 0.0), np.where(plane >= 0, rng.random(shape), 0.0).astype(np.float32)


def case(c, m, R=4, max_diff=2.0, min_count=6, span=1, sub=4, **change):
    d = dict(ref=c["ref"], src=c["src"], A=c["A"], B=c["B"], plane=m[0], w=m[1], score=m[2], w_step=c["w_step"], w_first=c["w_first"], D=c["D"],
             r=c["r"], min_var=c["min_var"], R=R, max_diff=max_diff, min_count=min_count, span=span, sub=sub)
    d.update(change)
    for k in ("ref", "src", "plane", "w", "score"):
        d[k] = np.ascontiguousarray(d[k])
        d[k].setflags(write=False)
    return d


def _cases():
    c = {}
    # shapes on, beside and beyond the tile's edges; r and R in {1, 3 or 4, 7}; (span, sub) in {(1, 1), (1, 4), (4, 8)}, the last with r = 7 once
    for (h, w), r, R, (span, sub) in (((15, 63), 1, 1, (1, 1)), ((16, 64), 3, 4, (1, 4)), ((17, 65), 7, 7, (4, 8)), ((33, 97), 3, 4, (1, 4)),
                                      ((33, 97), 7, 1, (1, 1)), ((16, 64), 1, 7, (4, 8)), ((17, 65), 3, 3, (1, 1))):
        p = DC.pair(h * 100 + w + r, h, w, 5, r, slant=(0.04, -0.03), min_score=0.5)
        c[f"shape_{h}x{w}_r{r}_R{R}_span{span}_sub{sub}"] = case(p, swept(p), R=R, span=span, sub=sub, min_count=3 if R == 1 else 6)
    for h, w in ((1, 70), (70, 1)):
        p = DC.pair(200 + h, h, w, 5, 1)
        c[f"shape_{h}x{w}"] = case(p, crafted_map(p, 201 + h), R=3, min_count=3)
    p = DC.sweeps()["ref_smaller_than_window"]                                          # 5 x 9, r = 3: nothing is refined, the slant still fits
    c["ref_smaller_than_window"] = case(p, crafted_map(p, 210, dropped=False), R=1, min_count=3)
    for name in ("window_leaves_src", "z_not_positive", "constant_patch_in_ref", "constant_patch_in_src", "constant_patch_in_ref_min_var_0",
                 "constant_patch_in_src_min_var_0"):
        c[name] = case(DC.sweeps()[name], DC.sweep_oracle(name), R=3)
    p = DC.sweeps()["window_leaves_src"]
    c["samples_leave_src_crafted"] = case(p, crafted_map(p, 211), R=3, span=4, sub=1)    # four steps either way: candidates beyond src's edge
    p = DC.sweeps()["nan_in_A"]
    c["nan_in_A"] = case(p, crafted_map(p, 212), R=3)
    p = DC.pair(213, 20, 70, 7, 2, slant=(0.05, 0.04), min_score=0.5)
    back = dict(p, w_first=p["w_first"] + (p["D"] - 1) * p["w_step"], w_step=-p["w_step"])      # the same planes, counted from the far end
    c["negative_w_step"] = case(back, swept(back), R=4)
    m = swept(p)
    c["every_pixel_dropped"] = case(p, (np.full_like(m[0], -1), np.zeros_like(m[1]), np.zeros_like(m[2])), R=4)
    c["every_score_is_one"] = case(p, (m[0], m[1], np.where(m[0] >= 0, np.float32(1.0), np.float32(0.0))), R=4)
    # a filled block: the clean-up's score 0 on inverse depths half a step off
    w, score = m[1].copy(), m[2].copy()
    w[6:12, 20:40] += 0.5 * p["w_step"]
    score[6:12, 20:40] = 0.0
    c["filled_pixels_with_score_0"] = case(p, (m[0], np.where(m[0] >= 0, w, 0.0), score), R=4)
    # every neighbour gated out, and fewer than min_count of them
    c["max_diff_gates_every_neighbour"] = case(p, crafted_map(p, 214, dropped=False), R=2, max_diff=2.0 ** -20, min_count=3)
    c["fewer_than_min_count"] = case(p, m, R=1, min_count=10)
    c["max_diff_64_min_count_225"] = case(p, crafted_map(p, 215, dropped=False), R=7, max_diff=64.0, min_count=225)
    # exact ties between candidates that are no mirrored pair: src has a period of 3 px along x and a plane step is 1 px, so with the map
    # one plane below the truth the candidates -2, +1 and +4 sample the same bytes and score the same; the order 0, -1, +1, -2, ... keeps +1
    p = DC.pair(216, 20, 70, 9, 2)
    src = np.ascontiguousarray(p["src"][:, np.arange(p["src"].shape[1]) % 3])
    p = dict(p, src=src, ref=DC.render(src, p["A"], p["B"], np.full((20, 70), p["w_first"] + 4.0 * p["w_step"])))
    plane = np.full((20, 70), 3, np.int16)
    c["periodic_tie"] = case(p, (plane, p["w_first"] + plane.astype(np.float64) * p["w_step"], np.full((20, 70), 0.5, np.float32)), R=2, span=4, sub=1)
    for v, name in ((2, "crafted_view0"), (3, "crafted_view1")):
        t = DC.two_maps("crafted")
        c[name] = case(t[v - 2], t[v], R=3, max_diff=8.0)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    return _cases()


@functools.lru_cache(maxsize=None)
def expected(name):
    """(slant, fitted, w', score', taken) of the case: the refinement runs on the case's own slant."""
    c = cases()[name]
    sl, fitted = RO.slant(c["plane"], c["w"], c["w_step"], c["R"], c["max_diff"], c["min_count"])
    out = (sl, fitted) + RO.refine(c["ref"], c["src"], c["A"], c["B"], c["plane"], c["w"], c["score"], sl, c["w_step"], c["r"], c["min_var"], c["span"], c["sub"])
    for a in out:
        a.setflags(write=False)
    return out


# ---- rendered scenes: the error against the truth -----------------------------------------------------------------------------------------------
SCENES = {
    "slant_0.06_0.05": dict(seed=1, D=13, r=3, slant=(0.06, 0.05)),
    "slant_0.15_0.10": dict(seed=2, D=21, r=3, slant=(0.15, 0.10)),
    "slant_0.15_0.10_radius_5": dict(seed=4, D=21, r=5, slant=(0.15, 0.10)),
    "slant_0.15_0.10_noise_4": dict(seed=2, D=21, r=3, slant=(0.15, 0.10), noise=4.0),
    "slant_0.15_0.10_noise_10": dict(seed=2, D=21, r=3, slant=(0.15, 0.10), noise=10.0),
    "fronto_parallel": dict(seed=1, D=13, r=3, k_true=6),
    "fronto_parallel_noise_10": dict(seed=1, D=13, r=3, k_true=6, noise=10.0),
}
ASSERTED = ("slant_0.06_0.05", "slant_0.15_0.10", "slant_0.15_0.10_radius_5", "slant_0.15_0.10_noise_4")      # the first four of the issue's table
H, W, PASSES = 48, 80, 2


def noisy(img, sigma, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(img.astype(np.float64) + rng.normal(0.0, sigma, img.shape)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(pair, [(w, score, taken) before and after each pass]) of a rendered 48 x 80 scene with the defaults: two passes, fit_radius 4, span 1,
    sub 4. Gaussian noise, where named, is added to both images behind the rendering."""
    o = dict(SCENES[name])
    noise = o.pop("noise", None)
    p = DC.pair(o.pop("seed"), H, W, o.pop("D"), o.pop("r"), **o)
    if noise is not None:
        p = dict(p, ref=noisy(p["ref"], noise, 1000), src=noisy(p["src"], noise, 1001))
    plane, w, score = swept(p)
    states = [(w, score, np.zeros(w.shape, np.uint8))]
    for _ in range(PASSES):
        w, score, taken, _ = RO.refine_slanted(p["ref"], p["src"], p["A"], p["B"], plane, w, score, p["w_step"], passes=1, r=p["r"], min_var=p["min_var"])
        states.append((w, score, taken))
    return p, plane, states


def errors(name):
    """Per state: (RMS, worst, 99th percentile) of |w - truth| / w_step over the kept pixels, and their mean score."""
    p, plane, states = scene(name)
    kept = plane >= 0
    truth = p["w_first"] + p["k_true"] * p["w_step"]
    out = []
    for w, score, _ in states:
        e = np.abs(w - truth)[kept] / abs(p["w_step"])
        out.append((float(np.sqrt((e * e).mean())), float(e.max()), float(np.percentile(e, 99)), float(score[kept].astype(np.float64).mean())))
    return out
