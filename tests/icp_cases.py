"""The cases the ICP tests share (tests/test_icp_cpu.py on the host build, tests/test_gpu_icp.py on the device), and their expected values
from tests/icp_oracle.py, computed once per process.

A case of the accumulate / finish entry points is a dict: source [n, 3] (already transformed), target [nt, 3], normals [nt, 3], idx [n]
int32 and d2 [n] float64 (from the oracle's search at d_max, or synthetic), centre [3], M [4, 4] (the transform the sums belong to)."""
import functools

import numpy as np

import icp_oracle as O

CH = O.ICP_CHUNK
SIZES = (0, 1, 2, 5, 6, 63, 64, 65, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH + 1)
BIG = 256 * CH + 1                      # a finish thread takes a second chunk; synthetic idx, no search
WORLD = np.array([4.0e5, 5.0e6, 2.0e3])
D_MAX = 0.5
METHODS = (O.POINT_TO_POINT, O.POINT_TO_PLANE)


def surface(g, step=0.25, offset=(0.0, 0.0, 0.0)):
    """(points [g * g, 3], unit normals) of z = 0.8 sin(0.35 x) + 0.6 cos(0.27 y) + 0.05 x y / 10 over a g x g lattice."""
    i, j = np.meshgrid(np.arange(g, dtype=np.float64), np.arange(g, dtype=np.float64), indexing="ij")
    x, y = (i * step).ravel(), (j * step).ravel()
    z = 0.8 * np.sin(0.35 * x) + 0.6 * np.cos(0.27 * y) + 0.05 * x * y / 10.0
    fx = 0.8 * 0.35 * np.cos(0.35 * x) + 0.005 * y
    fy = -0.6 * 0.27 * np.sin(0.27 * y) + 0.005 * x
    n = np.stack([-fx, -fy, np.ones_like(x)], 1)
    n /= np.sqrt((n * n).sum(1))[:, None]
    return np.ascontiguousarray(np.stack([x, y, z], 1) + np.asarray(offset, np.float64)[None, :]), np.ascontiguousarray(n)


def motion(angle_deg=0.6, axis=(0.3, -0.5, 0.8), shift=(0.04, -0.03, 0.05), about=(0.0, 0.0, 0.0)):
    """The 4x4 of a rotation by angle_deg about `axis` through `about`, then `shift` (test data only: sin and cos are fine here)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(angle_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = np.asarray(about) - R @ np.asarray(about) + np.asarray(shift)
    return M


def moved_sample(n, seed, offset=(0.0, 0.0, 0.0), noise=0.02):
    """n source points: target points of a 30 x 30 surface moved by the inverse of a small motion, plus noise."""
    tgt, nrm = surface(30, offset=offset)
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(tgt), n)
    Minv = np.linalg.inv(motion(about=np.asarray(offset) + (3.5, 3.5, 0.5)))
    src = tgt[pick] @ Minv[:3, :3].T + Minv[:3, 3] + rng.normal(0, noise, (n, 3))
    return np.ascontiguousarray(src), tgt, nrm


def _searched(src, tgt, nrm, centre=None, d_max=D_MAX, M=None):
    idx, d2 = O.nearest(src, tgt, d_max * d_max)
    return dict(source=src, target=tgt, normals=nrm, idx=idx, d2=d2, centre=O.default_centre(tgt) if centre is None else np.asarray(centre, np.float64),
                M=np.eye(4) if M is None else M, d_max=d_max)


def planar(normal_fn=None, g=24, lift=0.01):
    """A lattice z = 0 with normals (0, 0, 1) (or normal_fn(i)); the source is the lattice lifted; identity correspondences; centre 0."""
    i, j = np.meshgrid(np.arange(g, dtype=np.float64), np.arange(g, dtype=np.float64), indexing="ij")
    tgt = np.ascontiguousarray(np.stack([i.ravel() - 11.0, j.ravel() - 12.0, np.zeros(g * g)], 1))
    nrm = np.tile([0.0, 0.0, 1.0], (g * g, 1)) if normal_fn is None else normal_fn(np.arange(g * g))
    src = tgt + np.array([0.0, 0.0, lift])
    return dict(source=src, target=tgt, normals=np.ascontiguousarray(nrm), idx=np.arange(g * g, dtype=np.int32), d2=np.full(g * g, lift * lift),
                centre=np.zeros(3), M=np.eye(4), d_max=D_MAX)


def _near_singular(ratio):
    """Normals (d + e s_i, 0.3 t_i, 1), s and t of +-1: the column of n_z is the column of n_x over d up to e / d = ratio, so its pivot is
    about ratio^2 of its diagonal entry: above 2^-40 for 1e-4, below for 1e-8."""
    d = 0.01
    def fn(i):
        s = np.where(i % 2 == 0, 1.0, -1.0)
        t = np.where((i // 3) % 2 == 0, 1.0, -1.0)
        return np.stack([d + d * ratio * s, 0.3 * t, np.ones(len(i))], 1)
    return planar(fn)


@functools.lru_cache(maxsize=None)
def by_name(name):
    if name.startswith("n") and name[1:].isdigit():
        n = int(name[1:])
        return _searched(*moved_sample(n, seed=n + 1))
    if name == "big":
        tgt, nrm = surface(30)
        rng = np.random.default_rng(9)
        idx = (np.arange(BIG) % len(tgt)).astype(np.int32)
        src = tgt[idx] + rng.normal(0, 0.02, (BIG, 3))
        idx[::11] = -1
        d = src - tgt[np.maximum(idx, 0)]
        d2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
        return dict(source=np.ascontiguousarray(src), target=tgt, normals=nrm, idx=idx, d2=np.where(idx >= 0, d2, np.inf), centre=O.default_centre(tgt),
                    M=np.eye(4), d_max=D_MAX)
    if name == "all_minus":
        c = dict(_searched(*moved_sample(300, seed=2)))
        c["idx"], c["d2"] = np.full(300, -1, np.int32), np.full(300, np.inf)
        return c
    if name == "scattered_minus":
        c = dict(_searched(*moved_sample(1500, seed=3)))
        idx, d2 = c["idx"].copy(), c["d2"].copy()
        idx[3::7], d2[3::7] = -1, np.inf
        idx[10], idx[20], idx[30] = len(c["target"]), len(c["target"]) + 5, -2      # outside the target: unusable, nothing is read
        c["idx"], c["d2"] = idx, d2
        return c
    if name == "nonfinite_source":
        c = dict(_searched(*moved_sample(700, seed=4)))
        src = c["source"].copy()
        src[5, 0], src[300, 1], src[301, 2], src[699] = np.nan, np.inf, -np.inf, (np.nan, np.inf, 0.0)
        c["source"] = src                          # idx and d2 stay as found for the finite points: the kernel's own test is what excludes them
        return c
    if name == "nan_normals":
        c = dict(_searched(*moved_sample(900, seed=5)))
        nrm = c["normals"].copy()
        nrm[::5, 0], nrm[1::17, 2], nrm[2::31] = np.nan, np.inf, np.nan
        c["normals"] = nrm
        return c
    if name == "flipped":
        c = dict(by_name("n1025"))
        c["normals"] = c["normals"] * np.where(np.arange(len(c["normals"])) % 3 == 0, -1.0, 1.0)[:, None]
        return c
    if name == "world":
        return _searched(*moved_sample(1300, seed=6, offset=WORLD))
    if name == "far_centre":
        src, tgt, nrm = moved_sample(600, seed=7)
        return _searched(src, tgt, nrm, centre=(1.0e6, -1.0e6, 1.0e5))
    if name == "moved_M":
        src, tgt, nrm = moved_sample(800, seed=8)
        return _searched(src, tgt, nrm, M=motion(1.5, (0.1, 0.9, -0.2), (0.5, -0.25, 0.125)))
    if name == "planar":
        return planar()
    if name == "five_usable":
        c = dict(_searched(*moved_sample(40, seed=10)))
        idx, d2 = c["idx"].copy(), c["d2"].copy()
        keep = np.nonzero(idx >= 0)[0][:5]
        gone = np.setdiff1d(np.arange(40), keep)
        idx[gone], d2[gone] = -1, np.inf
        c["idx"], c["d2"] = idx, d2
        return c
    if name == "near_singular_ok":
        return _near_singular(1.0e-4)
    if name == "near_singular_degenerate":
        return _near_singular(1.0e-8)
    if name == "partial_overlap":
        src, tgt, nrm = moved_sample(500, seed=11)
        src[::4] += (0.0, 0.0, 3.0)                # beyond d_max of every target point
        return _searched(src, tgt, nrm)
    raise KeyError(name)


SPECIAL = ("all_minus", "scattered_minus", "nonfinite_source", "nan_normals", "flipped", "world", "far_centre", "moved_M", "planar", "five_usable",
           "near_singular_ok", "near_singular_degenerate", "partial_overlap")


def names(big=False):
    return [f"n{n}" for n in SIZES] + list(SPECIAL) + (["big"] if big else [])


@functools.lru_cache(maxsize=None)
def expected(name, method):
    """(partials [chunks, 32], total [32], record with the solve [64], record of the evaluation only [64])"""
    c = by_name(name)
    parts = O.partials(c["source"], c["target"], c["normals"], c["idx"], c["d2"], c["centre"], method)
    S = O.total(parts)
    n = len(c["source"])
    return parts, S, O.finish(S, c["M"], c["centre"], n, True), O.finish(S, c["M"], c["centre"], n, False)


# ---- the end-to-end case -----------------------------------------------------------------------------------------------------------------------
def end_to_end(world):
    """(source, target, normals, the motion that takes the source onto the target): a 40 x 40 lattice at step 0.25 and the same points
    moved by the inverse of 0.6 degrees about (0.3, -0.5, 0.8) and a shift of (0.04, -0.03, 0.05)."""
    off = WORLD if world else np.zeros(3)
    tgt, nrm = surface(40, offset=off)
    M = motion(about=off)
    Minv = np.linalg.inv(M)
    src = np.ascontiguousarray(tgt @ Minv[:3, :3].T + Minv[:3, 3])
    return src, tgt, nrm, M


@functools.lru_cache(maxsize=None)
def end_to_end_expected(world, method):
    src, tgt, nrm, _ = end_to_end(world)
    return O.icp(src, tgt, nrm, D_MAX, method=method)
