"""The shared cases of the depth-map fusion tests (tests/test_fuse_cpu.py, tests/test_gpu_fuse.py). A case is a dict: keep_a, w_a, score_a of
the base view, keep_b, w_b, score_b of the other one, pose_ab and pose_ba [30], tol_b and tol_a (inverse depths of the view linked into).
Expected outputs are computed once per process by the restatement (tests/fuse_oracle.py) and shared; nobody may write into them.

The kernels run one thread per pixel in blocks of 256: the shapes lie on, beside and beyond one block, and view b never has view a's size."""
import functools

import numpy as np

import dense_cases as DC
import dense_oracle as O
import fuse_oracle as FO

F = DC.F
BLOCK = 256
SHAPES = ((1, 1), (1, 255), (1, 256), (1, 257), (15, 63), (16, 64), (17, 65), (33, 97))
SWEPT = ("padded", "same_size", "rotated")
TOL = 1.0                                                    # plane steps, the default of `dense.fuse`
W_STEP = 1.0 / F


def frozen(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def geometry(ha, wa, rot=0.0, tz=0.0, scale_b=1.0, mx=16, my=3):
    """(Ka, Kb, R, t, hb, wb): a baseline of 1 along x and f = 120 px; view b is larger by (2 my, mx + 4) pixels with its principal point moved
    (then scaled by scale_b), rotated by `rot` about y and moved by `tz` along its axis."""
    Ka = np.array([[F, 0.0, wa / 2.0], [0.0, F, ha / 2.0], [0.0, 0.0, 1.0]])
    hb, wb = ha + 2 * my, wa + mx + 4
    Kb = np.array([[F, 0.0, wa / 2.0 + mx], [0.0, F, ha / 2.0 + my], [0.0, 0.0, 1.0]])
    if scale_b != 1.0:
        Kb = np.diag([scale_b, scale_b, 1.0]) @ Kb
        hb, wb = max(int(hb * scale_b), 1), max(int(wb * scale_b), 1)
    c, s = np.cos(rot), np.sin(rot)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    return Ka, Kb, R, np.array([-1.0, 0.0, tz]), hb, wb


def surface(seed, ha, wa, noise=0.3, density=0.9, normal=(0.02, -0.03, 1.0), depth=10.0, tol=TOL, **geo):
    """Two maps of one plane normal . X = depth (frame of view a), each with its own noise (in plane steps of 1 / f) and its own random
    keep mask; scores uniform in 0..1."""
    Ka, Kb, R, t, hb, wb = geometry(ha, wa, **geo)
    rng = np.random.default_rng(seed)
    n = np.asarray(normal, np.float64)

    def rays(K, h, w):
        Ki = O.W.inv3(K)
        uu, vv = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        return np.stack([Ki[i, 0] * uu + Ki[i, 1] * vv + Ki[i, 2] for i in range(3)], -1)

    za = depth / (rays(Ka, ha, wa) @ n)                                    # X = z ray
    rb = rays(Kb, hb, wb) @ R                                              # R^T ray, row by row
    zb = (depth + n @ (R.T @ t)) / (rb @ n)                                # X = R^T (z ray - t)
    pose_ab, pose_ba = FO.invert_pose(Ka, Kb, R, t)
    c = dict(keep_a=(rng.random((ha, wa)) < density).astype(np.uint8), w_a=1.0 / za + noise * W_STEP * rng.normal(size=(ha, wa)),
             score_a=rng.random((ha, wa)).astype(np.float32), keep_b=(rng.random((hb, wb)) < density).astype(np.uint8),
             w_b=1.0 / zb + noise * W_STEP * rng.normal(size=(hb, wb)), score_b=rng.random((hb, wb)).astype(np.float32),
             pose_ab=pose_ab, pose_ba=pose_ba, tol_b=tol * W_STEP, tol_a=tol * W_STEP)
    return c


def swapped(c):
    """The same case with view b as the base."""
    return dict(keep_a=c["keep_b"], w_a=c["w_b"], score_a=c["score_b"], keep_b=c["keep_a"], w_b=c["w_a"], score_b=c["score_a"], pose_ab=c["pose_ba"],
                pose_ba=c["pose_ab"], tol_b=c["tol_a"], tol_a=c["tol_b"])


# ---- the swept pairs of tests/dense_cases.py under every depth_filter ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def keep_masks(name, depth_filter):
    """(keep of view 0, keep of view 1) of a swept pair, as `im_dense_consistency` writes them."""
    c0, c1, m0, m1 = DC.two_maps(name)
    tau = O.filter_tau(depth_filter)
    k0 = DC.consistency_oracle(name, depth_filter)
    k1 = O.consistency(m1[0], m1[1], m0[0], m0[1], DC.pose(c1), 0.0 if tau is None else tau * abs(c0["w_step"]), tau is not None)
    k1.setflags(write=False)
    return k0, k1


def swept(name, depth_filter, base=0):
    c0, c1, m0, m1 = DC.two_maps(name)
    k0, k1 = keep_masks(name, depth_filter)
    c = dict(keep_a=k0, w_a=m0[1], score_a=m0[2], keep_b=k1, w_b=m1[1], score_b=m1[2], pose_ab=DC.pose(c0), pose_ba=DC.pose(c1),
             tol_b=TOL * abs(c1["w_step"]), tol_a=TOL * abs(c0["w_step"]))
    return c if base == 0 else swapped(c)


def truth(name):
    """(true inverse depth [h0, w0] of view 0, w_step) of a swept pair."""
    c0 = DC.two_maps(name)[0]
    return c0["w_first"] + c0["k_true"] * c0["w_step"], c0["w_step"]


# ---- crafted and planted maps ---------------------------------------------------------------------------------------------------------------------
def crafted():
    """Maps no sweep made, under a pose with t_z != 0 and a rotation: inverse depths far beyond the surface (negative, zero and NaN ones too),
    keep masks that drop pixels which hold a value, and a tolerance wide enough for a wrong target to link."""
    c = surface(83, 33, 97, noise=0.8, density=0.8, rot=0.05, tz=0.4, tol=32.0)
    rng = np.random.default_rng(84)
    for k in ("w_a", "w_b"):
        w = c[k]
        w[rng.random(w.shape) < 0.1] *= -1.0                # behind the camera; as a target within the tolerance, and 1 / w_b - t_z < 0
        w[rng.random(w.shape) < 0.1] *= 8.0
        w[rng.random(w.shape) < 0.03] = 0.0                 # as a target within the tolerance too: 1 / w_b is infinite, w' = 0
        w[rng.random(w.shape) < 0.03] = np.nan
    return c


def base_case(seed=7, **kw):
    a = dict(noise=0.2, density=1.0)
    a.update(kw)
    return surface(seed, 12, 20, **a)


def plant(c, p):
    """Pixel p = (v, u) of view a of case c: (j as (row, column) of view b, the inverse depth its point has there). Both masks must let it link."""
    hb, wb = c["keep_b"].shape
    inside, iu, iv, wz = FO.target(c["w_a"], c["pose_ab"], hb, wb)
    assert inside[p], p
    return (int(iv[p]), int(iu[p])), float(wz[p])


def _planted():
    out = {}
    # the tolerance met to the bit, and missed by one ulp: the difference is taken in the restatement's own arithmetic
    c = base_case(noise=0.0)
    p = (5, 9)
    j, wz = plant(c, p)
    c["w_b"][j] = wz + 0.37 * W_STEP
    diff = float(np.abs(np.float64(c["w_b"][j]) - np.float64(wz)))
    exact, above = dict(c), dict(c)
    exact.update(tol_b=diff)
    above.update(tol_b=float(np.nextafter(diff, 0.0)))                     # the difference lies one ulp above this tolerance
    out["tolerance_met_to_the_bit"], out["difference_one_ulp_above_the_tolerance"] = exact, above
    # tol = 0: only targets that hold the projected inverse depth itself link
    c = base_case(seed=8)
    for p in ((2, 3), (6, 11), (11, 19)):
        j, wz = plant(c, p)
        c["w_b"][j] = wz
    c.update(tol_b=0.0, tol_a=0.0)
    out["tolerance_zero"] = c
    # scores: both 0 (two filled pixels), one negative, both negative
    c = base_case(seed=9)
    hb, wb = c["keep_b"].shape
    _, iu, iv, _ = FO.target(c["w_a"], c["pose_ab"], hb, wb)
    c["score_a"][3, :] = 0.0
    c["score_b"][iv[3, :], iu[3, :]] = 0.0
    c["score_a"][5, :] = -0.5
    c["score_a"][7, :] = -0.25
    c["score_b"][iv[7, :], iu[7, :]] = -0.75
    out["scores_zero_and_negative"] = c
    # view b at half the resolution: neighbouring pixels of view a claim the same target
    out["many_claim_one_target"] = surface(10, 12, 20, noise=0.1, density=1.0, scale_b=0.5)
    # keep masks that drop pixels which hold a plane: `dense_consistent` would pass them
    c = base_case(seed=11)
    c["keep_b"][::2, ::3] = 0
    c["keep_a"][1::3, ::2] = 0
    out["masks_drop_pixels_that_hold_a_plane"] = c
    for name, (ka, kb) in (("mask_a_all_zero", (0, 1)), ("mask_b_all_zero", (1, 0)), ("masks_all_zero", (0, 0)), ("masks_all_one", (1, 1))):
        c = base_case(seed=12)
        c["keep_a"][:], c["keep_b"][:] = ka, kb
        out[name] = c
    # 1 / w_b - t_z <= 0 at a linked pixel: the second measurement is unusable, the pixel keeps its own
    c = base_case(seed=13, tz=0.4, tol=1e6)
    c["w_b"][:, ::2] = 2.5                                                  # 1 / 2.5 - 0.4 = 0 (or an ulp off it), 1 / 3 - 0.4 < 0
    c["w_b"][::2, ::2] = 3.0
    out["second_measurement_unusable"] = c
    return out


def _cases():
    c = {}
    for h, w in SHAPES:
        c[f"shape_{h}x{w}"] = surface(h * 1000 + w, h, w, rot=0.01)
    for name in SWEPT:
        for f in O.FILTERS:
            for base in (0, 1):
                c[f"swept_{name}_{f}_base{base}"] = swept(name, f, base)
    c["crafted"] = crafted()
    c["crafted_swapped"] = swapped(crafted())
    c.update(_planted())
    return {k: frozen(v) for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def cases():
    return _cases()


@functools.lru_cache(maxsize=None)
def expected(name):
    """(link, w_out, score_out, views, claimed, rest) of a case."""
    c = cases()[name]
    out = FO.fuse(c["keep_a"], c["w_a"], c["score_a"], c["keep_b"], c["w_b"], c["score_b"], c["pose_ab"], c["tol_b"])
    out = out + (FO.rest(c["keep_b"], c["w_b"], c["keep_a"], c["w_a"], c["pose_ba"], c["tol_a"], out[4]),)
    for a in out:
        a.setflags(write=False)
    return out
