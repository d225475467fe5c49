"""The shared case list of the DEM-of-difference tests (tests/test_dod_cpu.py: the host build of csrc/dod_cell.h; tests/test_gpu_dod.py: the
kernels): every size at which csrc/dod.hip takes another path - empty and tiny clouds, degenerate grids, widths and cell counts around the
wave, the block and the chunk B of the cell sums, cells around the sizes a heavy-cell path would start at, points exactly on a half-step
boundary, non-finite coordinates, signed zeros, every direction, no valid cell, identical clouds, the neighbour window at every corner and
edge, H of mixed sign over 600 orders of magnitude, a batch that shares clouds, a pair at the cell cap. A case is a dict: name, clouds
(list of [n, 3] float64), pairs (list of (ground, ceil) cloud indices), d (vertDim), s (step). Results of tests/dod_oracle.py are cached per
case and handed out read-only."""
import functools

import numpy as np

import dod_oracle as O

B = O.CHUNK
HALF = 0.5                        # a power of two: (x - min) / s + 0.5 is exact for the lattices below


def cloud(x, y, z, d):
    """[n, 3] with x along X = (d + 1) % 3, y along Y = (d + 2) % 3 and z along d"""
    x, y, z = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(z, np.float64))
    out = np.zeros((x.size, 3))
    out[:, (d + 1) % 3], out[:, (d + 2) % 3], out[:, d] = x.ravel(), y.ravel(), z.ravel()
    return out


def boxed(rng, n, w, h, s, d, z0=0.0):
    """n random points in the box of a w x h grid of step s, the two corners that pin the grid first"""
    x = np.concatenate([[0.0, (w - 1) * s], rng.uniform(0.0, (w - 1) * s, n)]) if w > 1 else np.zeros(n + 2)
    y = np.concatenate([[0.0, (h - 1) * s], rng.uniform(0.0, (h - 1) * s, n)]) if h > 1 else np.zeros(n + 2)
    return cloud(x, y, z0 + rng.normal(0.0, 1.0, n + 2), d)


def case(name, clouds, pairs=((0, 1),), d=2, s=HALF):
    return {"name": name, "clouds": [np.ascontiguousarray(c, np.float64).reshape(-1, 3) for c in clouds], "pairs": [tuple(p) for p in pairs],
            "d": d, "s": float(s)}


def grid_case(name, w, h, n=40, d=2, seed=0):
    rng = np.random.default_rng(seed + 1000 * w + h)
    return case(name, [boxed(rng, n, w, h, HALF, d), boxed(rng, n, w, h, HALF, d, 2.0)], d=d)


def cells_case(name, cells_ij, w, h, d=2):
    """both clouds fill exactly the listed cells (i, j) of a w x h grid, the ground also the two corners that pin it"""
    ij = np.array(cells_ij, np.float64).reshape(-1, 2)
    rng = np.random.default_rng(len(ij) + w)
    ceil = cloud(ij[:, 0] * HALF, ij[:, 1] * HALF, rng.normal(3.0, 1.0, len(ij)), d)
    pin = np.array([[0, 0], [w - 1, h - 1]], np.float64)
    gij = np.concatenate([ij, pin])
    ground = cloud(gij[:, 0] * HALF, gij[:, 1] * HALF, rng.normal(0.0, 1.0, len(gij)), d)
    return case(name, [ground, ceil], d=d)


@functools.lru_cache(maxsize=None)
def all_cases():
    rng = np.random.default_rng(17)
    out = []
    e = np.zeros((0, 3))
    one, two = np.array([[1.0, 2.0, 3.0]]), np.array([[1.0, 2.0, 3.0], [1.7, 2.1, 4.0]])
    out += [case("n0_n0", [e, e]), case("n0_n1", [e, one]), case("n1_n0", [one, e]), case("n1_n1", [one, one + [0.0, 0.0, 1.5]]),
            case("n2_n2", [two, two[::-1] + [0.0, 0.0, -2.0]]), case("n1_n2_y", [one, two], d=1)]
    out += [grid_case("grid_1x1", 1, 1), grid_case("grid_1x7", 1, 7), grid_case("grid_7x1", 7, 1)]
    for wdt in (63, 64, 65, 255, 256, 257, B - 1, B, B + 1):
        out.append(grid_case(f"width_{wdt}", wdt, 1, n=3 * wdt))
    for (w, h) in ((7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (1, 257), (33, 31), (32, 32), (25, 41), (64, 48), (3, B + 1)):
        out.append(grid_case(f"cells_{w * h}_{w}x{h}", w, h, n=2 * w * h))
    for n in (1, 63, 64, 65, 1025):                      # one cell of a 3 x 3 grid holds n points of the ground and n + 1 of the ceil
        g = np.concatenate([boxed(rng, 6, 3, 3, HALF, 2), cloud(rng.uniform(0.3, 0.7, n), rng.uniform(0.3, 0.7, n), rng.normal(0, 1e3, n), 2)])
        c = np.concatenate([cloud(rng.uniform(0.3, 0.7, n + 1), rng.uniform(0.3, 0.7, n + 1), rng.normal(5, 1e3, n + 1), 2), boxed(rng, 6, 3, 3, HALF, 2)])
        out.append(case(f"heavy_cell_{n}", [g, c]))
    k = np.arange(9, dtype=np.float64)                   # x = min + (k + 1/2) s exactly: the upper of the two cells
    on_edge = cloud(np.concatenate([[0.0], 0.25 + k * HALF]), np.concatenate([[0.0], 0.25 + k[::-1] * HALF]), np.arange(10.0), 2)
    out.append(case("half_step_boundary", [on_edge, on_edge[::-1] + [0.0, 0.0, 1.0]]))
    base_g, base_c = boxed(rng, 60, 6, 5, HALF, 2), boxed(rng, 60, 6, 5, HALF, 2, 1.0)
    for col in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            g, c = base_g.copy(), base_c.copy()
            g[5::7, col], c[3::11, col] = bad, bad
            out.append(case(f"nonfinite_{'xyz'[col]}_{str(bad).replace('-', 'm')}", [g, c]))
    g, c = base_g.copy(), base_c.copy()
    g[:, :] = np.nan
    out.append(case("ground_all_dropped", [g, c]))
    z = np.array([-0.0, -0.0, 0.0, -0.0])
    out.append(case("negative_zero_heights", [cloud([0, 0, 0.5, 1.0], [0, 0, 0, 0.5], z, 2), cloud([0, 0.5, 1.0, 0], [0, 0, 0.5, 0], -z, 2)]))
    out.append(case("negative_zero_origin", [cloud([-0.0, 0.0, 1.0], [0.0, -0.0, 1.0], [1, 2, 3], 2), cloud([0.0, 1.0], [0.0, 1.0], [1, 1], 2)]))
    for d in (0, 1, 2):
        r = np.random.default_rng(40 + d)
        out.append(case(f"direction_{'xyz'[d]}", [r.uniform(-20, 20, (500, 3)) * (1, 2, 3), r.uniform(-20, 20, (400, 3)) * (1, 2, 3)], d=d, s=0.3 * (d + 1)))
    out.append(case("world_frame", [rng.uniform(0, 30, (800, 3)) + (416000.0, 5090000.0, 1800.0), rng.uniform(0, 30, (800, 3)) + (416000.0, 5090000.0, 1800.0)],
                    d=0, s=0.3))
    out.append(case("disjoint", [boxed(rng, 50, 5, 5, HALF, 2), boxed(rng, 50, 5, 5, HALF, 2) + (100.0, 0.0, 0.0)]))
    same = boxed(rng, 300, 12, 9, HALF, 2)
    out.append(case("identical", [same, same.copy()]))
    w, h = 6, 5
    ring = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (2, 0), (3, h - 1), (0, 2), (w - 1, 2), (2, 2), (3, 2)]
    out.append(cells_case("corners_and_edges", ring, w, h))
    out.append(cells_case("all_valid_6x5", [(i, j) for j in range(h) for i in range(w)], w, h))
    out.append(cells_case("checkerboard", [(i, j) for j in range(9) for i in range(11) if (i + j) % 2 == 0], 11, 9))
    mags = 10.0 ** np.arange(-300, 301, 25)
    hh = np.concatenate([mags[::2], -mags[1::2], [1e300, -1e300, 5e-324, -5e-324]])[rng.permutation(len(mags) + 4)]
    n = len(hh)
    out.append(case("magnitudes", [cloud(np.arange(n) % 6 * HALF, np.arange(n) // 6 * HALF, np.zeros(n), 2), cloud(np.arange(n) % 6 * HALF, np.arange(n) // 6 * HALF, hh, 2)]))
    out.append(case("overflowing_cell", [cloud([0, 0, 0.5], [0, 0, 0], [1e308, 1e308, 1.0], 2), cloud([0, 0.5], [0, 0], [1.0, 2.0], 2)]))
    series = [boxed(rng, 900, 40, 30, 0.3, 0, z0=float(t)) + (0.0, 0.1 * t, -0.2 * t) for t in range(4)]
    out.append(case("batch_5_pairs_4_clouds", series, pairs=[(0, 1), (1, 2), (2, 3), (0, 3), (1, 1)], d=0, s=0.3))
    out.append(case("batch_with_empty", [series[0], e, series[1]], pairs=[(0, 1), (1, 1), (0, 2), (2, 0)], d=0, s=0.3))
    side = 4096                                          # side * side = im_dod_max_cells()
    g = cloud([0, (side - 1) * HALF, 3.0, 100.0], [0, (side - 1) * HALF, 7.5, 2000.0], [1.0, 2.0, 3.0, 4.0], 2)
    c = cloud([(side - 1) * HALF, 3.0, 100.25, 0], [(side - 1) * HALF, 7.5, 2000.0, 0], [5.0, 7.0, 11.0, -1.0], 2)
    out.append(case("cell_cap", [g, c]))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    for c in out:
        for a in c["clouds"]:
            a.setflags(write=False)
    return tuple(out)


def over_the_cap():
    """one column more than `cell_cap`: refused"""
    c = by_name("cell_cap")
    g = np.concatenate([c["clouds"][0], [[4096 * HALF, 0.0, 0.0]]])
    return case("over_the_cap", [g, c["clouds"][1]])


def names():
    return [c["name"] for c in all_cases()]


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


def packed(c):
    """(points [N, 3], offsets [E + 1] int64, pairs [P, 2] int32) as the C entry points take a case"""
    pts = np.ascontiguousarray(np.concatenate(c["clouds"] + [np.zeros((0, 3))]), np.float64)
    offsets = np.concatenate([[0], np.cumsum([len(a) for a in c["clouds"]])]).astype(np.int64)
    return pts, offsets, np.array(c["pairs"], np.int32).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def full(name, chunk=O.CHUNK):
    """tests/dod_oracle.py's result of every pair of the case, read-only"""
    c = by_name(name)
    res = [O.dod(c["clouds"][g], c["clouds"][k], c["d"], c["s"], chunk) for g, k in c["pairs"]]
    for r in res:
        for v in (r["H"], r["report_row"]) + r["cells"] + r["counts"] + r["means"]:
            v.setflags(write=False)
    return tuple(res)
