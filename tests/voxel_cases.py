"""The cases the voxel tests share (tests/test_voxel_cpu.py, tests/test_gpu_voxel.py): the smallest shapes at which a path of
csrc/voxel.hip can go wrong. A case is a dict: `clouds` (a list of [n, 3] float64), `colors` and `normals` (lists of [n, 3] or None),
`grids` [G, 7] (min_bound, max_bound, voxel_size; G = 1, or one per cloud when `per_cloud`). `full(name)` is the restatement's result per
cloud, computed once. Mesh cases are (grid, grid_index [V, 3], colors [V, 3]).

Sizes: 1 / 63 / 64 / 65 / 1025 points in one voxel (a wave, and more than a block, of points in one segment); 255 / 256 / 257 voxels
(the scan block, SCAN_THREADS = 256) and 65537 (the second level of the scan, 256 blocks); grids of one voxel, one row along either
outer axis, 2^20 voxels per axis, and the largest the cap of 2^62 allows, alone and in a batch of three."""
import functools

import numpy as np

import voxel_oracle as O

S20 = 2 ** 20


def _case(name, clouds, grids, colors=None, normals=None, per_cloud=False):
    clouds = [np.ascontiguousarray(c, np.float64).reshape(-1, 3) for c in clouds]
    case = {"name": name, "clouds": clouds, "grids": np.ascontiguousarray(np.asarray(grids, np.float64).reshape(-1, 7)), "per_cloud": per_cloud,
            "colors": None if colors is None else [np.ascontiguousarray(c, np.float64).reshape(-1, 3) for c in colors],
            "normals": None if normals is None else [np.ascontiguousarray(c, np.float64).reshape(-1, 3) for c in normals]}
    for group in (case["clouds"], case["colors"] or [], case["normals"] or [], [case["grids"]]):
        for a in group:
            a.setflags(write=False)
    return case


def _attrs(rng, n):
    col = np.round(rng.uniform(0, 1, (n, 3)) * 255) / 255
    nrm = rng.normal(0, 1, (n, 3))
    return col, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def _in_voxels(rng, grid, idx):
    """one point strictly inside each of the voxels idx [m, 3]"""
    return grid[:3] + (idx + rng.uniform(0.05, 0.95, idx.shape)) * grid[6]


def _filled(name, rng, dims, V, per_voxel, s=0.25, origin=(-3.0, 10.0, 100.0)):
    """V distinct voxels of a grid of `dims`, `per_voxel` points in each on average, in random order, with colours and normals"""
    dims = np.array(dims)
    grid = O.make_grid(origin, np.array(origin) + dims * s - 0.01 * s, s)
    assert O.grid_dims(grid) == tuple(dims)
    cells = rng.choice(int(dims.prod()), V, replace=False)
    idx = np.stack([cells // (dims[1] * dims[2]), cells // dims[2] % dims[1], cells % dims[2]], 1)
    which = np.concatenate([np.arange(V), rng.integers(0, V, int(V * (per_voxel - 1)))])
    rng.shuffle(which)
    pts = _in_voxels(rng, grid, idx[which])
    col, nrm = _attrs(rng, len(pts))
    return _case(name, [pts], grid, [col], [nrm])


def _one_voxel(rng, n):
    grid = O.make_grid((1.0, 2.0, 3.0), (1.99, 2.99, 3.99), 0.5)          # 2 x 2 x 2 voxels, all points in voxel (1, 0, 1)
    pts = _in_voxels(rng, grid, np.tile([1, 0, 1], (n, 1)))
    col, nrm = _attrs(rng, n)
    return _case(f"one_voxel_{n}", [pts], grid, [col], [nrm])


def _batch(rng, sizes, name, per_cloud=False, colors=True):
    shared = O.make_grid((0.0, 0.0, 0.0), (3.0, 2.0, 1.0), 0.3)
    clouds, cols, nrms, grids = [], [], [], []
    for k, n in enumerate(sizes):
        pts = rng.uniform(-0.2, 3.2, (n, 3)) * (1.0, 0.7, 0.35)              # some fall outside the shared grid
        if n > 5:
            pts[3] = (np.nan, 1.0, 0.5)
        c, m = _attrs(rng, n)
        clouds.append(pts); cols.append(c); nrms.append(m)
        g = O.auto_grid(pts, 0.3 + 0.1 * k)
        grids.append(g if g is not None else shared)
    return _case(name, clouds, grids if per_cloud else shared, cols if colors else None, nrms if colors else None, per_cloud)


@functools.lru_cache(maxsize=None)
def _all():
    rng = np.random.default_rng(19)
    unit = O.make_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.25)
    cases = [_case("n0", [np.zeros((0, 3))], unit, [np.zeros((0, 3))], [np.zeros((0, 3))]),
             _case("n1", [[0.3, 0.3, 0.3]], unit, [[0.5, 0.25, 1.0]], [[0.0, 0.0, 1.0]]),
             _case("n2", [[[0.3, 0.3, 0.3], [0.9, 0.1, 0.6]]], unit, [[[0.5, 0.25, 1.0], [0.1, 0.2, 0.3]]], [[[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]])]
    cases += [_one_voxel(rng, n) for n in (1, 63, 64, 65, 1025)]
    cases += [_filled(f"voxels_{V}", rng, (16, 8, 4), V, 3) for V in (255, 256, 257)]
    cases.append(_filled("voxels_65537", rng, (64, 64, 32), 65537, 1.1))
    cases.append(_case("grid_1x1x1", [rng.uniform(0, 1, (9, 3))], O.make_grid((0, 0, 0), (1, 1, 1), 2.0), [rng.uniform(0, 1, (9, 3))]))
    g = O.make_grid((5.0, 5.0, 5.0), (5.2, 5.2, 9.9), 0.7)                         # 1 x 1 x 8
    cases.append(_case("grid_1x1xN", [rng.uniform(5.0, 5.2, (40, 3)) + (0, 0, 1) * rng.uniform(0, 4.7, (40, 1))], g, [rng.uniform(0, 1, (40, 3))]))
    g = O.make_grid((5.0, 5.0, 5.0), (9.9, 5.2, 5.2), 0.7)                         # 8 x 1 x 1
    cases.append(_case("grid_Nx1x1", [rng.uniform(5.0, 5.2, (40, 3)) + (1, 0, 0) * rng.uniform(0, 4.7, (40, 1))], g, [rng.uniform(0, 1, (40, 3))]))
    # 2^20 voxels per axis, s = 1: the keys reach 2^60
    big = O.make_grid((0, 0, 0), (S20 - 0.5,) * 3, 1.0)
    far = np.array([[S20 - 0.75] * 3, [0.0, 0.0, 0.0], [S20 - 0.75, 0.25, 7.5], [0.5, S20 - 0.75, 0.5], [S20 - 0.75] * 3])
    cases.append(_case("grid_2p20", [far], big, [rng.uniform(0, 1, (5, 3))]))
    cases.append(_case("cap_exact", [far + (S20, S20, 0)], cap_grid(0)[0], [rng.uniform(0, 1, (5, 3))]))               # 2^21 x 2^21 x 2^20 = 2^62 voxels
    g3 = cap_grid_3(0)[0]                                                                                     # 3 x (2^20 x 2^20 x 1398101) = 2^62 - 2^40
    top = np.array([[S20 - 0.75, S20 - 0.75, 1398101 - 0.75], [0.0, 0.0, 0.0], [S20 - 0.75, S20 - 0.75, 1398101 - 0.75]])
    cases.append(_case("cap_under_3_clouds", [top, top[:2], top[::-1]], g3, [rng.uniform(0, 1, (len(c), 3)) for c in (top, top[:2], top)]))
    cases.append(_case("cap_per_cloud_3", [far + (S20, 0, 0), far, far[:3]], [O.make_grid((0, 0, 0), (2 * S20 - 0.5, S20 - 0.5, S20 - 0.5), 1.0), big, big],
                       per_cloud=True))                                                                       # 2^61 + 2^60 + 2^60 = 2^62
    # on the bounds and on the faces: min = 0, max = 2, s = 0.5 -> 5 voxels per axis, max itself in voxel 4
    g = O.make_grid((0, 0, 0), (2, 2, 2), 0.5)
    on = np.array([[0, 0, 0], [2, 2, 2], [0.5, 1.0, 1.5], [0, 2, 0], [2, 0, 1], [1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [1.5, 2.0, 0.0]])
    cases.append(_case("on_bounds_and_faces", [on], g, [rng.uniform(0, 1, (len(on), 3))]))
    # the division: at s = 0.1 the points 0.3, 0.6, 0.7 lie in voxels 2, 5, 6; a multiplication by 1 / s gives 3, 6, 7
    div = np.array([[0.3, 0.05, 0.05], [0.6, 0.05, 0.05], [0.7, 0.05, 0.05], [0.05, 0.3, 0.6], [0.05, 0.7, 0.3]])
    cases.append(_case("division_s01", [div], O.make_grid((0, 0, 0), (1, 1, 1), 0.1), [rng.uniform(0, 1, (5, 3))]))
    lo, hi = np.array([-1.5, 0.25, 3.0]), np.array([2.5, 4.25, 7.0])
    ulp = [lo, hi, (lo + hi) / 2]
    for a in range(3):
        for bound, toward in ((lo, -np.inf), (hi, np.inf)):
            p = ((lo + hi) / 2).copy()
            p[a] = np.nextafter(bound[a], toward)
            ulp.append(p)
            q = p.copy()
            q[a] = bound[a]
            ulp.append(q)
    cases.append(_case("one_ulp_outside", [np.array(ulp)], O.make_grid(lo, hi, 0.5), [rng.uniform(0, 1, (len(ulp), 3))]))
    bad = rng.uniform(0.1, 0.9, (20, 3))
    k = 1
    for a in range(3):
        for v in (np.nan, np.inf, -np.inf):
            bad[k, a] = v
            k += 2
    cases.append(_case("nonfinite_points", [bad], unit, [rng.uniform(0, 1, (20, 3))], [rng.uniform(0, 1, (20, 3))]))
    pts = rng.uniform(0.1, 0.9, (12, 3))
    col, nrm = rng.uniform(0, 1, (12, 3)), rng.uniform(0, 1, (12, 3))
    col[2, 0], col[5, 1], col[7, 2], nrm[1, 0], nrm[4, 1] = np.nan, np.inf, -np.inf, np.nan, np.inf
    cases.append(_case("nonfinite_attributes", [pts], unit, [col], [nrm]))
    z = np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.1], [-0.0, -0.0, -0.0], [0.3, -0.0, 0.0]])
    cases.append(_case("signed_zeros", [z], O.make_grid((0.0, -0.0, 0.0), (1, 1, 1), 0.25), [[[-0.0, 0.0, -0.0]] * 4], [[[-0.0, -0.0, -0.0]] * 4]))
    cases.append(_case("negative_zero_origin", [z], O.make_grid((-0.0, -0.0, -0.0), (1, 1, 1), 0.25), [rng.uniform(0, 1, (4, 3))]))
    same = np.tile([0.3, 0.3, 0.3], (4, 1))
    cases.append(_case("colour_sum_overflows", [same], unit, [np.tile([1e308, -1e308, 1.7e308], (4, 1))]))
    cases.append(_case("colour_sum_denormal", [same], unit, [np.tile([5e-324, 1e-310, 2.5e-308], (4, 1)) * np.arange(1, 5)[:, None]]))
    cases.append(_case("colours_absent", [rng.uniform(0, 1, (30, 3))], unit))
    cases.append(_batch(rng, (37, 0, 150), "batch_3_one_empty"))
    cases.append(_batch(rng, (37, 0, 150), "batch_3_per_cloud", per_cloud=True))
    cases.append(_batch(rng, (300, 70, 1), "batch_3_no_colours", colors=False))
    return {c["name"]: c for c in cases}


def cap_grid(extra):
    """2^21 x 2^21 x (2^20 + extra) voxels: at the cap of 2^62 with extra = 0, over it with 1; and the far corner"""
    return O.make_grid((0, 0, 0), (2 * S20 - 0.5, 2 * S20 - 0.5, S20 + extra - 0.5), 1.0), (2 * S20, 2 * S20, S20 + extra)


def cap_grid_3(extra):
    """a grid for three clouds: 3 x 2^20 x 2^20 x (1398101 + extra) = 2^62 - 2^40 voxels with extra = 0, 2^62 + 2^41 with 1"""
    return O.make_grid((0, 0, 0), (S20 - 0.5, S20 - 0.5, 1398101 + extra - 0.5), 1.0), (S20, S20, 1398101 + extra)


def names():
    return list(_all())


def by_name(name):
    return _all()[name]


def grid_of(case, e):
    return case["grids"][e if case["per_cloud"] else 0]


def attr(case, which, e):
    return None if case[which] is None else case[which][e]


@functools.lru_cache(maxsize=None)
def full(name):
    """the restatement's result for every cloud of the case (read-only)"""
    case = by_name(name)
    out = []
    for e, cloud in enumerate(case["clouds"]):
        r = O.voxelize(cloud, grid_of(case, e), attr(case, "colors", e), attr(case, "normals", e))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(r)
    return out


def packed(case):
    """(points [n, 3], colors or None, normals or None, offsets [E + 1] int64) of the case's clouds one behind the other"""
    cat = lambda group: None if group is None else np.ascontiguousarray(np.concatenate(list(group) + [np.zeros((0, 3))]))
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in case["clouds"]])]).astype(np.int64)
    return cat(case["clouds"]), cat(case["colors"]), cat(case["normals"]), offsets


# ---- mesh cases ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _meshes():
    rng = np.random.default_rng(91)
    grid = O.make_grid((-2.0, 3.0, 50.0), (0.9, 5.9, 52.9), 0.5)              # 6 x 6 x 6 voxels
    n = O.grid_dims(grid)

    def m(name, idx, g=grid, vertices=None):
        idx = np.array(sorted(map(tuple, idx)), np.int32).reshape(-1, 3)     # ascending voxel key
        col = np.round(rng.uniform(0, 1, (len(idx), 3)) * 255) / 255
        return name, {"grid": g, "grid_index": idx, "colors": col, "vertices": vertices}

    block = [(i, j, k) for i in (2, 3) for j in (1, 2) for k in (4, 5)]
    out = [m("one_voxel", [(1, 2, 3)], vertices=8), m("share_face", [(1, 2, 3), (2, 2, 3)], vertices=12), m("share_edge", [(1, 2, 3), (2, 3, 3)], vertices=14),
           m("share_corner", [(1, 2, 3), (2, 3, 4)], vertices=15), m("block_2x2x2", block, vertices=27),
           m("extremes", [(0, 0, 0), (n[0] - 1, n[1] - 1, n[2] - 1), (0, n[1] - 1, 0)], vertices=24)]
    for V in (31, 32, 33):                                                     # 8 V + 1 scanned items = 249, 257, 265: around the scan block
        cells = rng.choice(216, V, replace=False)
        out.append(m(f"voxels_{V}", [(c // 36, c // 6 % 6, c % 6) for c in cells]))
    huge = full("voxels_65537")[0]                                            # 524296 items: the second level of the scan
    out.append(m("voxels_65537", huge["grid_index"], by_name("voxels_65537")["grids"][0]))
    out.append(m("far_corner", full("grid_2p20")[0]["grid_index"], by_name("grid_2p20")["grids"][0]))
    return dict(out)


def mesh_names():
    return list(_meshes())


def mesh_by_name(name):
    return _meshes()[name]


@functools.lru_cache(maxsize=None)
def mesh_full(name):
    c = mesh_by_name(name)
    return O.box_mesh(c["grid"], c["grid_index"], c["colors"])
