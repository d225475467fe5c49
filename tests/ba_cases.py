"""The shared cases of the bundle-adjustment tests (tests/test_ba_cpu.py, tests/test_gpu_ba.py): a synthetic stereo scene in the layout of
csrc/ba_point.h, and what tests/ba_oracle.py makes of every case, computed once and handed out read-only.

A case is a dict: cams [48], X [n, 3], obs [n, 4], sig [n], prior [n, 6], cprior [12], mask, lam (the lambda of the first iteration), opts.
Unless a case says otherwise the last six points are control points with a full prior of 1 cm, both centres carry a prior of 10 cm, the
mask is the default (both poses and f), the scene sits at the origin and the start is the truth perturbed."""
import functools

import numpy as np

import ba_oracle as O

WORLD = np.array([4.0e5, 5.0e6, 2.0e3])
N_CONTROL = 6
SIZES = (0, 1, 63, 64, 65, O.BA_TILE - 1, O.BA_TILE, O.BA_TILE + 1, O.BA_CHUNK - 1, O.BA_CHUNK, O.BA_CHUNK + 1, 2 * O.BA_CHUNK + 1)


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def true_cameras(origin=np.zeros(3)):
    """Two cameras 30 m apart that converge on a front about 120 m away; 6000 px focal length, OpenCV distortion with all eight terms."""
    K = np.array([[6000.0, 0, 3000.0], [0, 6000.0, 2000.0], [0, 0, 1]])
    d0 = [-0.05, 0.02, 1e-4, -2e-4, 0.01, 1e-3, -5e-4, 2e-4]
    d1 = [-0.04, 0.015, -1.5e-4, 1e-4, 0.008, -8e-4, 3e-4, 1e-4]
    c0 = O.camera_state(_rot(0.01, 0.12, -0.005), origin + [-15.0, 0.0, 0.0], K, d0)
    K1 = K.copy()
    K1[0, 0] = K1[1, 1] = 6050.0
    K1[0, 2], K1[1, 2] = 2990.0, 2010.0
    c1 = O.camera_state(_rot(-0.008, -0.12, 0.004), origin + [15.0, 0.5, -0.3], K1, d1)
    return np.concatenate([c0, c1])


def scene(n, seed=0, origin=np.zeros(3), noise=0.0, perturb=1.0):
    """n points in all (the last min(n, 6) are control points): truth and a perturbed start."""
    rng = np.random.default_rng(1000 + seed)
    origin = np.asarray(origin, np.float64)
    truth = true_cameras(origin)
    Xt = origin + np.stack([rng.uniform(-40, 40, n), rng.uniform(-25, 25, n), rng.uniform(90, 150, n)], 1)
    obs = np.zeros((n, 4))
    for c in range(2):
        p = O.project(truth[24 * c:24 * c + 24], Xt) if n else dict(u=np.zeros(0), v=np.zeros(0))
        obs[:, 2 * c], obs[:, 2 * c + 1] = p["u"], p["v"]
    obs = obs + noise * rng.normal(0, 1.0, obs.shape)
    prior = np.zeros((n, 6))
    nc = min(n, N_CONTROL)
    if nc:
        prior[n - nc:, :3], prior[n - nc:, 3:] = Xt[n - nc:], 0.01
    cprior = np.concatenate([truth[9:12], [0.1] * 3, truth[33:36], [0.1] * 3])
    start = truth.copy()
    for c in range(2):
        w = perturb * rng.normal(0, 2e-3, 3)
        start[24 * c:24 * c + 9] = (_rot(*w) @ truth[24 * c:24 * c + 9].reshape(3, 3)).reshape(9)
        start[24 * c + 9:24 * c + 12] += perturb * rng.normal(0, 0.05, 3)
        start[24 * c + 12:24 * c + 14] += perturb * rng.normal(0, 20.0)
    X0 = Xt + perturb * rng.normal(0, 0.2, Xt.shape)
    return dict(cams=start, X=X0, obs=obs, sig=np.full(n, 0.5), prior=prior, cprior=cprior, mask=O.MASK_DEFAULT, lam=1e-3, opts=O.options(),
                truth=truth, X_true=Xt)


def _build():
    cases = {}
    for n in SIZES:
        cases[f"n{n}"] = scene(n, seed=n)
    c = scene(100, seed=1)                                       # absent observations: without a full prior such a point is unusable
    c["obs"][5, 0] = c["obs"][6, 3] = c["obs"][7, :] = np.nan
    c["obs"][96, 1] = c["obs"][97, 2] = np.nan                   # control points seen by one camera: usable
    cases["absent"] = c
    c = scene(100, seed=2)                                       # non-finite coordinates, observations, sigmas
    c["X"][3, 0], c["X"][4, 1], c["X"][5, 2] = np.nan, np.inf, -np.inf
    c["obs"][10, 0], c["obs"][11, 3] = np.inf, -np.inf
    c["sig"][12], c["sig"][13], c["sig"][14], c["sig"][15] = 0.0, -1.0, np.inf, np.nan
    c["prior"][95, 0] = np.nan
    cases["nonfinite"] = c
    c = scene(100, seed=3)                                       # a point behind camera 0, one in its plane
    c["X"][8] = c["cams"][9:12] - 50.0 * c["cams"][6:9]
    c["X"][9] = c["cams"][9:12] + 20.0 * c["cams"][0:3]
    cases["behind"] = c
    c = scene(70, seed=4)                                        # partial priors, on tie points too
    c["prior"][10, 3:] = [0.05, 0.0, 0.0]
    c["prior"][10, :3] = c["X_true"][10]
    c["prior"][11, 3:] = [0.0, 0.02, 0.03]
    c["prior"][11, :3] = c["X_true"][11]
    c["prior"][66, 5] = 0.0
    c["cprior"][3:6] = [0.05, 0.0, 0.2]                          # and on the centres
    cases["partial_priors"] = c
    for name, mask in (("mask_fixed", 0), ("mask_all", O.MASK_ALL), ("mask_odd", 0b0101010101010101010101010101)):
        c = scene(130, seed=5)
        c["mask"] = mask
        cases[name] = c
    cases["world"] = scene(300, seed=6, origin=WORLD)
    c = scene(80, seed=7)                                        # all free, no prior anywhere, lambda 0: the gauge is free
    c["prior"][:] = 0.0
    c["cprior"][:] = 0.0
    c["mask"], c["lam"] = O.MASK_ALL, 0.0
    cases["singular"] = c
    c = scene(90, seed=8, noise=0.5, perturb=40.0)               # a far start with every parameter free: some steps overshoot
    c["mask"] = O.MASK_ALL
    cases["accept_reject"] = c
    cases["noisy"] = scene(200, seed=9, noise=0.5)
    c = scene(40, seed=10)                                       # no noise: the cost reaches rounding level, and ctol > 0 ends the run OK
    c["opts"] = O.options(ctol=2.0 ** -56)
    cases["ctol"] = c
    c = scene(90, seed=8, noise=0.5, perturb=40.0)               # accept_reject's scene under a low ceiling: its first rejected step stalls
    c["mask"], c["opts"] = O.MASK_ALL, O.options(lambda_max=1e-6)
    cases["stalled"] = c
    for c in cases.values():
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return cases


_CASES = None


def by_name(name):
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES[name]


def names():
    by_name("n0")
    return list(_CASES)


TABLE = ("n0", "n65", f"n{O.BA_CHUNK + 1}")                     # the three-epoch table


@functools.lru_cache(maxsize=None)
def first_iteration(name):
    """What the restatement makes of the first iteration of a case, and the state after it."""
    c = by_name(name)
    st = O.initial_state(c["lam"])
    it = O.iteration(c["cams"], c["X"], c["obs"], c["sig"], c["prior"], c["cprior"], c["mask"], c["opts"], st)
    it["state"] = st
    for v in it.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return it


@functools.lru_cache(maxsize=None)
def whole_run(name, max_iter=30):
    """cams, X, state, history of the restatement's whole loop."""
    c = by_name(name)
    opts = np.array(c["opts"])
    opts[3] = max_iter
    out = O.run(c["cams"], c["X"], c["obs"], c["sig"], c["prior"], c["cprior"], c["mask"], opts, O.initial_state(c["lam"]))
    for v in out:
        v.setflags(write=False)
    return out


def table(names_=TABLE):
    """The cases one behind the other: off [E + 1], cams [E, 48], X, obs, sig, prior, cprior [E, 12]"""
    cs = [by_name(n) for n in names_]
    off = np.concatenate([[0], np.cumsum([len(c["X"]) for c in cs])]).astype(np.int64)
    cat = lambda k, w: np.concatenate([np.asarray(c[k], np.float64).reshape(-1, w) for c in cs]) if w else np.concatenate([c[k] for c in cs])
    return dict(off=off, cams=np.stack([c["cams"] for c in cs]), X=cat("X", 3), obs=cat("obs", 4), sig=cat("sig", 0), prior=cat("prior", 6),
                cprior=np.stack([c["cprior"] for c in cs]))
