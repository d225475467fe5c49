"""The shared cases of the dense-stereo tests (tests/test_dense_cpu.py, tests/test_gpu_dense.py), rendered with the restatement's own
bilinear (tests/dense_oracle.py) from a seeded texture: view 1 IS the texture, view 0 is view 1 seen through the homography of the true
surface. Expected outputs are computed once per process and shared; nobody may write into them.

The sweep's block owns a 64 x 16 tile (`im_dense_tile_w/h`): widths 63, 64, 65, 97 and heights 15, 16, 17, 33 lie on, beside and beyond
its edges, 97 x 33 takes 2 x 3 blocks."""
import functools

import numpy as np

import dense_oracle as O

TILE_W, TILE_H = 64, 16
F = 120.0


def texture(seed, h, w):
    """A seeded 8-bit texture with structure at the scale of a few pixels."""
    rng = np.random.default_rng(seed)
    t = rng.random((h + 4, w + 4))
    t = (t[:-1, :-1] + t[1:, :-1] + t[:-1, 1:] + t[1:, 1:]) / 4.0
    t = (t[:-1, :-1] + t[1:, :-1] + t[:-1, 1:] + t[1:, 1:]) / 4.0
    t = t[:h, :w]
    t = (t - t.min()) / (t.max() - t.min())
    return np.round(t * 255.0).astype(np.uint8)


def render(src, A, B, wmap):
    """The ref view of a surface of inverse depth wmap [h0, w0] (a plane: affine in (u, v)): per pixel the restatement's sample under
    A + w B, rounded to 8 bits. Pixels that see nothing of src are 0."""
    h0, w0 = wmap.shape
    out = np.zeros((h0, w0), np.uint8)
    A, B = np.asarray(A).reshape(9), np.asarray(B).reshape(9)
    u = np.arange(w0, dtype=np.float64)[None, :] + np.zeros((h0, 1))
    v = np.arange(h0, dtype=np.float64)[:, None] + np.zeros((1, w0))
    H = A[:, None, None] + wmap[None] * B[:, None, None]
    x, y, z = (H[0] * u + H[1] * v) + H[2], (H[3] * u + H[4] * v) + H[5], (H[6] * u + H[7] * v) + H[8]
    okx, xi, fx = O.W.fix((x / z) * 32.0)
    oky, yi, fy = O.W.fix((y / z) * 32.0)
    h1, w1 = src.shape
    ok = okx & oky & (z > 0) & (xi >= 0) & (xi + 1 < w1) & (yi >= 0) & (yi + 1 < h1)
    xc, yc = np.clip(xi, 0, w1 - 2), np.clip(yi, 0, h1 - 2)
    s = src.astype(np.int64)
    b = ((32 - fx) * (32 - fy)) * s[yc, xc] + (fx * (32 - fy)) * s[yc, xc + 1] + ((32 - fx) * fy) * s[yc + 1, xc] + (fx * fy) * s[yc + 1, xc + 1]
    out[ok] = ((b[ok] + 512) >> 10).astype(np.uint8)
    return out


def pair(seed, h0, w0, D, r, k_true=None, slant=(0.0, 0.0), step_px=1.0, first_px=10.0, pad=True, min_var=4, min_score=0.8, rot=0.0):
    """A stereo pair with a baseline of 1 along x and f = 120 px: plane k has a disparity of first_px + k step_px pixels. pad: view 1 is
    large enough (and its principal point moved) for every hypothesis of every ref pixel to fall inside it; otherwise it has ref's size
    and K, so that hypotheses leave it on the left. The true surface is plane k_true (default the middle one), tilted by `slant` planes
    per pixel along (u, v). rot: a rotation of view 1 about its y axis, radians."""
    k_true = (D - 1) / 2.0 if k_true is None else k_true
    w_step, w_first = step_px / F, first_px / F
    d_max = first_px + (D - 1) * max(step_px, 0.0)
    K0 = np.array([[F, 0.0, w0 / 2.0], [0.0, F, h0 / 2.0], [0.0, 0.0, 1.0]])
    if pad:
        mx, my = int(np.ceil(d_max)) + 2, 4
        h1, w1 = h0 + 2 * my, w0 + mx + 4
        K1 = np.array([[F, 0.0, w0 / 2.0 + mx], [0.0, F, h0 / 2.0 + my], [0.0, 0.0, 1.0]])
    else:
        h1, w1, K1 = h0, w0, K0.copy()
    c, s = np.cos(rot), np.sin(rot)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    t = np.array([-1.0, 0.0, 0.0])
    A, B = O.sweep_matrices(K0, K1, R, t)
    src = texture(seed, h1, w1)
    uu, vv = np.meshgrid(np.arange(w0, dtype=np.float64), np.arange(h0, dtype=np.float64))
    ktrue = k_true + slant[0] * (uu - w0 / 2.0) + slant[1] * (vv - h0 / 2.0)
    ref = render(src, A, B, w_first + ktrue * w_step)
    return dict(ref=ref, src=src, A=A, B=B, w_first=w_first, w_step=w_step, D=D, r=r, min_var=min_var, min_score=min_score,
                K0=K0, K1=K1, R=R, t=t, k_true=ktrue)


def _sweeps():
    c = {}
    for h, w in ((15, 63), (16, 64), (17, 65), (33, 97), (16, 97), (33, 63)):
        c[f"shape_{h}x{w}"] = pair(h * 100 + w, h, w, 3, 1)
    for D in (1, 2, 3, 64, 65):
        c[f"planes_{D}"] = pair(40 + D, 20, 70, D, 1, step_px=1.0 if D <= 3 else 0.25)
    for r in (1, 3, 7):
        c[f"radius_{r}"] = pair(50 + r, 33, 97, 3, r)
    c["ref_smaller_than_window"] = pair(60, 5, 9, 3, 3)
    c["ref_of_one_window"] = pair(61, 15, 15, 2, 7)
    c["window_leaves_src"] = pair(62, 20, 70, 6, 2, pad=False, first_px=2.0, step_px=3.0, k_true=1)
    z = pair(63, 20, 70, 4, 1)
    z["A"] = np.array([1.0, 0.0, 3.0, 0.0, 1.0, 2.0, -0.02, 0.0, 1.0])
    z["B"] = np.array([0.0, 0.0, -120.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    z["min_score"] = -1.0
    c["z_not_positive"] = z
    nan = pair(64, 17, 65, 3, 1)
    nan["A"] = nan["A"].copy()
    nan["A"][4] = np.nan
    c["nan_in_A"] = nan
    flat = pair(65, 20, 70, 3, 2)
    flat["ref"] = flat["ref"].copy()
    flat["ref"][4:16, 10:30] = 128
    c["constant_patch_in_ref"] = flat
    flat = pair(66, 20, 70, 3, 2)
    flat["src"] = flat["src"].copy()
    flat["src"][6:20, 30:60] = 77
    c["constant_patch_in_src"] = flat
    for name in ("constant_patch_in_ref", "constant_patch_in_src"):
        m = dict(c[name])
        m["min_var"] = 0
        c[name + "_min_var_0"] = m
    c["all_planes_tie"] = pair(67, 17, 65, 5, 1, step_px=0.0)
    c["best_at_first_plane"] = pair(68, 20, 70, 5, 1, k_true=0)
    c["best_at_last_plane"] = pair(69, 20, 70, 5, 1, k_true=4)
    c["slanted"] = pair(70, 33, 97, 9, 3, slant=(0.03, 0.05), min_score=0.5)
    c["every_score_kept"] = pair(71, 17, 65, 4, 1, min_score=-2.0)
    return c


@functools.lru_cache(maxsize=None)
def sweeps():
    return _sweeps()


@functools.lru_cache(maxsize=None)
def sweep_oracle(name):
    c = sweeps()[name]
    out = O.sweep(c["ref"], c["src"], c["A"], c["B"], c["w_first"], c["w_step"], c["D"], c["r"], c["min_var"], c["min_score"])
    for a in out:
        a.setflags(write=False)
    return out


# ---- two maps and their consistency -------------------------------------------------------------------------------------------------------
def inverse(c):
    """The same pair with the roles and the pose inverted: the sweep of view 1 over the same schedule."""
    Ri, ti = c["R"].T, -c["R"].T @ c["t"]
    A, B = O.sweep_matrices(c["K1"], c["K0"], Ri, ti)
    d = dict(c)
    d.update(ref=c["src"], src=c["ref"], A=A, B=B, K0=c["K1"], K1=c["K0"], R=Ri, t=ti)
    return d


def pose(c):
    return np.concatenate([O.W.inv3(c["K0"]).reshape(9), c["R"].reshape(9), c["t"], np.asarray(c["K1"], np.float64).reshape(9)])


def camera(c, R0=None, t0=None):
    R0 = np.eye(3) if R0 is None else R0
    t0 = np.zeros(3) if t0 is None else t0
    return np.concatenate([O.W.inv3(c["K0"]).reshape(9), np.asarray(R0, np.float64).reshape(9), np.asarray(t0, np.float64).reshape(3)])


PAIRS = {
    "padded": dict(seed=80, h0=33, w0=97, D=7, r=1, min_score=0.6),
    "same_size": dict(seed=81, h0=20, w0=70, D=7, r=1, pad=False, first_px=1.0, step_px=1.0, k_true=3, min_score=0.6),
    "rotated": dict(seed=82, h0=17, w0=65, D=9, r=2, rot=0.02, slant=(0.02, -0.04), min_score=0.5),
    "crafted": dict(seed=83, h0=33, w0=97, D=7, r=1, pad=False, first_px=4.0, rot=0.05),
}


@functools.lru_cache(maxsize=None)
def two_maps(name):
    """(case of view 0, case of view 1, map 0, map 1), maps = (plane, w, score)."""
    c0 = pair(**PAIRS[name])
    c1 = inverse(c0)
    maps = []
    if name == "crafted":
        # maps no sweep made: inverse depths far beyond the schedule (negative ones too), so that kept pixels of map 0 project outside
        # view 1, behind it, and onto dropped pixels of map 1
        rng = np.random.default_rng(83)
        for c in (c0, c1):
            shape = c["ref"].shape
            plane = rng.integers(-1, c["D"], shape).astype(np.int16)
            w = c["w_first"] + (plane + rng.normal(0.0, 0.8, shape)) * c["w_step"]
            w[rng.random(shape) < 0.1] *= -1.0
            w[rng.random(shape) < 0.1] *= 8.0
            m = (plane, np.where(plane >= 0, w, 0.0), np.where(plane >= 0, rng.random(shape), 0.0).astype(np.float32))
            for a in m:
                a.setflags(write=False)
            maps.append(m)
        return c0, c1, maps[0], maps[1]
    for c in (c0, c1):
        m = O.sweep(c["ref"], c["src"], c["A"], c["B"], c["w_first"], c["w_step"], c["D"], c["r"], c["min_var"], c["min_score"])
        for a in m:
            a.setflags(write=False)
        maps.append(m)
    return c0, c1, maps[0], maps[1]


CONSISTENCY = [(p, f) for p in PAIRS for f in O.FILTERS]


@functools.lru_cache(maxsize=None)
def consistency_oracle(name, depth_filter):
    c0, c1, m0, m1 = two_maps(name)
    tau = O.filter_tau(depth_filter)
    keep = O.consistency(m0[0], m0[1], m1[0], m1[1], pose(c0), 0.0 if tau is None else tau * abs(c1["w_step"]), tau is not None)
    keep.setflags(write=False)
    return keep


# ---- clouds: a keep mask over a random surface ----------------------------------------------------------------------------------------------
CLOUDS = {"empty": (12, 20, 0, 1), "one_point": (12, 20, 1, 3), "count_255": (20, 20, 255, 1), "count_256": (20, 20, 256, 3), "count_257": (20, 20, 257, 1),
          "count_65537": (260, 260, 65537, 3), "half_kept": (33, 97, 1600, 3), "all_kept": (17, 65, 17 * 65, 1), "one_row": (1, 300, 200, 3),
          "one_column": (300, 1, 200, 1)}
R_WORLD = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])
T_WORLD = np.array([0.5, -2.0, 3.0])


@functools.lru_cache(maxsize=None)
def cloud_case(name):
    h, w, count, channels = CLOUDS[name]
    rng = np.random.default_rng(len(name) * 1000 + count)
    keep = np.zeros(h * w, np.uint8)
    keep[rng.choice(h * w, count, replace=False)] = 1
    keep = keep.reshape(h, w)
    uu, vv = np.meshgrid(np.arange(w), np.arange(h))
    wmap = 0.1 + 0.0004 * uu + 0.0003 * vv + 0.002 * rng.random((h, w))
    wmap[rng.random((h, w)) < 0.02] = 0.1                   # repeated depths: some tangents are parallel, some normals degenerate
    score = rng.random((h, w)).astype(np.float32)
    img = rng.integers(0, 256, (h, w, 3) if channels == 3 else (h, w), dtype=np.uint8)
    K = np.array([[F, 0.0, w / 2.0], [0.0, F, h / 2.0], [0.0, 0.0, 1.0]])
    cam = camera(dict(K0=K), R_WORLD, T_WORLD)
    out = O.cloud(keep, wmap, score, img, cam)
    for a in (keep, wmap, score, img, cam) + tuple(out):
        a.setflags(write=False)
    return dict(keep=keep, w=wmap, score=score, img=img, cam=cam, channels=channels, h=h, w_=w, count=count), out
