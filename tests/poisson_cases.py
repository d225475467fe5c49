"""The clouds the Poisson tests share (tests/test_poisson_cpu.py, tests/test_gpu_poisson.py), small enough that the numpy restatement
(tests/poisson_oracle.py) of each takes well under a second, and `oracle(name)`: every stage of the restatement, computed once."""
import functools

import numpy as np

import poisson_oracle as O


def sphere(n, seed, noise=0.0, upper_only=False, dense_upper=False):
    """n unit-sphere samples with outward normals; `noise` moves every sample along its normal by a normal deviate of that size."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1)[:, None]
    if upper_only:
        p[:, 2] = np.abs(p[:, 2])
    if dense_upper:              # two thirds of the samples on the upper half: twice the density of the lower one
        p[:, 2] = np.where(rng.random(n) < 2.0 / 3.0, np.abs(p[:, 2]), -np.abs(p[:, 2]))
    nrm = p.copy()
    if noise:
        p = p * (1.0 + noise * rng.normal(size=(n, 1)))
    return p, nrm


def front(n, seed):
    """A sloped, undulating glacier front z(x, y) over 100 m x 60 m with its upward normals, not normalised."""
    rng = np.random.default_rng(seed)
    x, y = rng.random(n) * 100.0, rng.random(n) * 60.0
    z = 0.3 * x + 5.0 * np.sin(x / 10.0) * np.cos(y / 8.0)
    zx = 0.3 + 0.5 * np.cos(x / 10.0) * np.cos(y / 8.0)
    zy = -0.625 * np.sin(x / 10.0) * np.sin(y / 8.0)
    return np.stack([x, y, z], 1), np.stack([-zx, -zy, np.ones(n)], 1) * 3.0


def lattice_shell():
    """The 98 integer points on the faces of [0, 4]^3 with normals away from its centre: with scale = 1 and depth 2 every sample lies on
    a node (h = 1), and those on the upper faces in the last cell with fraction 1, where the cell index clamps."""
    g = np.stack(np.meshgrid(*[np.arange(5.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    p = g[((g == 0) | (g == 4)).any(1)]
    return p, p - 2.0


def _case(points, normals, depth, scale=1.1, cycles=8, grid=None):
    return dict(points=np.ascontiguousarray(points), normals=np.ascontiguousarray(normals), depth=depth, scale=scale, cycles=cycles, grid=grid)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "sphere_d4":
        return _case(*sphere(2000, 1), 4)
    if name == "sphere_d4_one_cycle":
        return _case(*sphere(2000, 1), 4, cycles=1)
    if name == "sphere_d5":
        return _case(*sphere(4000, 2), 5)
    if name == "sphere_d5_noise":
        return _case(*sphere(4000, 2, noise=0.01), 5)
    if name == "half_sphere_d5":
        return _case(*sphere(4000, 3, upper_only=True), 5)
    if name == "sphere_d2":
        return _case(*sphere(500, 4), 2)
    if name == "front_d6":
        return _case(*front(20000, 5), 6)
    if name == "single":
        return _case(np.array([[0.4, 0.6, 0.3]]), np.array([[0.0, 0.0, 2.0]]), 2, grid=(np.zeros(3), 0.25, 2))
    if name == "lattice_d2":
        return _case(*lattice_shell(), 2, scale=1.0)
    if name == "two_densities_d4":
        return _case(*sphere(6000, 6, dense_upper=True), 4)
    raise KeyError(name)


SPHERES = ["sphere_d4", "sphere_d5", "sphere_d5_noise"]
OTHERS = ["sphere_d4_one_cycle", "half_sphere_d5", "sphere_d2", "front_d6", "single", "lattice_d2", "two_densities_d4"]
ALL = SPHERES + OTHERS


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The restatement's stages of a case (see `poisson_oracle.field`) with its mesh: vertices, triangles, weights, keys, density."""
    c = case(name)
    f = O.field(c["points"], c["normals"], depth=c["depth"], scale=c["scale"], cycles=c["cycles"], grid=c["grid"])
    f["vertices"], f["triangles"], f["weights"], f["keys"] = O.extract(f["chi"], f["W"], f["iso"], f["origin"], f["h"], f["depth"])
    f["density"] = O.density(f["weights"], f["depth"])
    return f


def edge_census(triangles):
    """(every directed edge occurs once, every directed edge has its reverse, number of undirected edges)."""
    t = triangles.astype(np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    n = int(t.max()) + 1 if len(t) else 1
    fwd, back = e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]
    once = len(np.unique(fwd)) == len(fwd)
    paired = np.array_equal(np.sort(fwd), np.sort(back))
    return once, paired, len(fwd) // 2
