"""DSMs and orthophotos on the device (csrc/dsm.hip) against the reference's outputs (tests/golden/g12_dsm_orthophoto.npz) and against
the numpy + scipy oracle (tests/dsm_oracle.py) on random clouds.

Bounds: binned x / y / z bit-identical; z bit-identical, and the NaN mask identical, on every cell whose smallest barycentric
coordinate in scipy's simplex exceeds 1e-12 (a unique containing triangle) and on every cell outside the triangulation. A cell on a
shared edge or vertex takes the lowest simplex index that contains it where scipy's walk may stop in a neighbour; both contain the
cell to within scipy's own tolerance (eps = 100 DBL_EPSILON in barycentric units), so there z may differ by 4 ulp plus
eps * max |z of the vertices| * 4 (on at most 1 % of the cells by more than 4 ulp), and a NaN vertex value of the one triangle
reaches the cell through a zero weight (0 * NaN) only there. Orthophotos from the same DSM and projections bit-identical; colours
within 1e-12.

This file is the statement about the reference (scipy's `find_simplex`, g12). What the device itself computes, the lowest simplex index
that contains a cell, is pinned exactly and on every cell, shared edges and vertices included, against the brute-force restatement in
tests/test_gpu_dsm_edges.py, with the colours, the refusals and the code's own boundaries."""
import os
import sys
import types

import numpy as np
import pytest
from scipy.spatial import QhullError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dsm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g12():
    return O.load_g12(os.path.join(ROOT, "tests", "golden", "g12_dsm_orthophoto.npz"))


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


def camera(g, dist="d5"):
    return types.SimpleNamespace(K=g["cam_K"], dist=g["dist_" + dist], R=g["cam_R"], t=g["cam_t"])


def check_grid(z, ref, tri, bz, xq, yq, qx=None, qy=None):
    """The bounds of the module docstring for z (the device) against ref (the reference / oracle) on cells (qx, qy)."""
    if qx is None:
        gx, gy = np.meshgrid(xq, yq)
        qx, qy = gx.ravel(), gy.ravel()
    z, ref = np.asarray(z).ravel(), np.asarray(ref).ravel()
    s = tri.find_simplex(np.stack([qx, qy], 1)).astype(np.int64)
    unique = (O.min_barycentric(tri, s, qx, qy) > 1e-12) & (s >= 0)
    outside = s < 0
    mask = np.isnan(z) != np.isnan(ref)
    assert not mask[unique | outside].any(), f"NaN mask: {int(mask[unique | outside].sum())} cells differ"
    assert O.bits_equal(z[unique], ref[unique]), f"{int((z[unique] != ref[unique]).sum())} interior cells differ"
    assert O.bits_equal(z[outside], ref[outside])
    ok = ~np.isnan(ref) & ~np.isnan(z)
    d = np.abs(z[ok] - ref[ok])
    ulp = np.spacing(np.maximum(np.abs(z[ok]), np.abs(ref[ok])))
    vmax = np.nanmax(np.abs(np.asarray(bz, np.float64)), initial=0.0)
    assert np.all(d <= 4 * ulp + 4 * O.EPS * vmax), float(np.max((d - 4 * ulp) / (O.EPS * vmax)))
    assert (d > 4 * ulp).sum() <= 1e-2 * len(z), int((d > 4 * ulp).sum())
    return int(unique.sum()), int((~unique & ok).sum())


@pytest.mark.parametrize("case", O.G12_CASES)
def test_g12_build_dsm(g12, eng, case):
    from icepy4d_amd.utils.dsm_orthophoto import _bin_on_device, build_dsm
    pts, step, xlim, ylim, fill, xq, yq = O.g12_case(g12, case)
    _, (bx, by, bz) = _bin_on_device(eng, np.ascontiguousarray(pts, np.float64), step)
    for k, v in (("bx", bx), ("by", by), ("bz", bz)):
        assert O.bits_equal(v, g12[f"{case}_{k}"]), k
    d = build_dsm(pts, dsm_step=step, xlim=xlim, ylim=ylim, fill_value=fill, engine=eng)
    ref = g12[case + "_z"]
    assert d.z.dtype == np.float64 and d.z.shape == ref.shape == (len(yq), len(xq)) and d.res == step
    assert np.array_equal(d.x, np.meshgrid(xq, yq)[0]) and np.array_equal(d.y, np.meshgrid(xq, yq)[1])
    check_grid(d.z, ref, O.triangulate(bx, by), bz, xq, yq)


def test_g12_orthophoto_from_reference_dsm(g12, eng):
    from icepy4d_amd.utils.dsm_orthophoto import DSM, generate_ortophoto
    pts, step, xlim, ylim, fill, xq, yq = O.g12_case(g12, "s05")
    d = DSM(*np.meshgrid(xq, yq), g12["s05_z"], step)
    o = generate_ortophoto(g12["image"], d, camera(g12), engine=eng)
    assert O.bits_equal(o, g12["ortho"])


def test_g12_build_dsm_then_orthophoto(g12, eng):
    from icepy4d_amd.utils.dsm_orthophoto import build_dsm, generate_ortophoto
    pts, step, xlim, ylim, fill, xq, yq = O.g12_case(g12, "s05")
    d = build_dsm(pts, dsm_step=step, engine=eng)
    o = generate_ortophoto(g12["image"], d, camera(g12), engine=eng)
    ref = g12["ortho"]
    assert o.shape == ref.shape and o.dtype == np.uint8
    diff = np.abs(o.astype(np.int16) - ref.astype(np.int16)).max(axis=2)
    assert diff.max() <= 1 and (diff > 0).sum() <= 1e-4 * diff.size


@pytest.mark.parametrize("dist", O.G12_DISTS)
def test_g12_points(g12, eng, dist):
    from icepy4d_amd.sfm import interpolate_point_colors, project_points
    c = camera(g12, dist)
    assert O.bits_equal(project_points(g12["pc_points"], c, engine=eng), g12["pc_proj_" + dist])
    cols = interpolate_point_colors(g12["pc_points"], g12["image"], c, engine=eng)
    assert cols.dtype == np.float64 and cols.shape == g12["pc_cols_" + dist].shape
    assert np.abs(cols - g12["pc_cols_" + dist]).max() <= 1e-12
    if dist == "d5":
        bgr = interpolate_point_colors(g12["pc_points"], g12["image"], c, convert_BRG2RGB=False, engine=eng)
        assert np.abs(bgr - g12["pc_cols_d5_bgr"]).max() <= 1e-12


def random_cloud(n, step, seed, extent=40.0):
    """Half the points on integer coordinates (grid nodes for steps that divide 1; cocircular quadruples everywhere), z smooth + noise."""
    rng = np.random.default_rng(seed)
    if n == 3:
        return np.array([[1.3, 2.2, 5.0], [37.9, 5.1, 7.5], [12.4, 38.8, 6.0]])
    xy = rng.uniform(0, extent, (n, 2))
    k = n // 2
    xy[:k] = rng.integers(0, int(extent) + 1, (k, 2))
    z = 5 + np.sin(xy[:, 0] / 7) * 3 + np.cos(xy[:, 1] / 5) + rng.normal(0, 0.1, n)
    z[rng.random(n) < 0.01] = np.nan
    return np.c_[xy, z]


@pytest.mark.parametrize("n", [3, 100, 20_000, 300_000])
@pytest.mark.parametrize("step", [0.1, 0.25, 1.0, 2.5])
def test_random_against_oracle(eng, n, step):
    from icepy4d_amd.utils.dsm_orthophoto import _bin_on_device, build_dsm
    pts = random_cloud(n, step, seed=int(n + 1000 * step))
    r = O.build_dsm(pts, step)
    _, (bx, by, bz) = _bin_on_device(eng, pts, step)
    for k, v in (("bx", bx), ("by", by), ("bz", bz)):
        assert O.bits_equal(v, r[k]), k
    # a 3 x 3 input is read as three points in columns, as in the reference: hand it over transposed
    d = build_dsm(pts.T if n == 3 else pts, dsm_step=step, engine=eng)
    check_grid(d.z, r["z"], r["tri"], r["bz"], r["xq"], r["yq"])


def test_large_grid_sampled(eng):
    """A 4000 x 4000 grid (16 M cells) from 20 k points; 100 k cells checked against scipy's find_simplex + the oracle's evaluation."""
    from icepy4d_amd.utils.dsm_orthophoto import build_dsm
    rng = np.random.default_rng(7)
    pts = np.c_[rng.uniform(0, 400, (20_000, 2)), rng.normal(50, 5, 20_000)]
    step = 0.1
    d = build_dsm(pts, dsm_step=step, xlim=[0.0, 400.0], ylim=[0.0, 400.0], engine=eng)
    assert d.z.shape == (4000, 4000)
    bx, by, bz = O.bin_points(pts, step)
    tri = O.triangulate(bx, by)
    xq, yq = O.grid_axes([0.0, 400.0], [0.0, 400.0], step)
    cells = rng.choice(d.z.size, 100_000, replace=False)
    r, c = np.divmod(cells, 4000)
    qx, qy = xq[c], yq[r]
    s = tri.find_simplex(np.stack([qx, qy], 1)).astype(np.int64)
    ref = O.eval_cells(tri, bz, s, qx, qy, np.nan)
    check_grid(d.z.ravel()[cells], ref, tri, bz, xq, yq, qx, qy)


def test_repeatable(g12, eng):
    from icepy4d_amd.utils.dsm_orthophoto import build_dsm, generate_ortophoto
    pts = random_cloud(20_000, 0.25, seed=3)
    a = build_dsm(pts, dsm_step=0.25, engine=eng)
    b = build_dsm(pts, dsm_step=0.25, engine=eng)
    assert O.bits_equal(a.z, b.z)
    pts, step, xlim, ylim, fill, xq, yq = O.g12_case(g12, "s1")
    d = build_dsm(pts, dsm_step=step, fill_value=fill, engine=eng)
    o1 = generate_ortophoto(g12["image"], d, camera(g12), engine=eng)
    o2 = generate_ortophoto(g12["image"], d, camera(g12), engine=eng)
    assert O.bits_equal(o1, o2)


def test_qhull_errors_as_in_the_reference(eng):
    from icepy4d_amd.utils.dsm_orthophoto import build_dsm
    line = np.c_[np.arange(10.0), 2 * np.arange(10.0), np.ones(10)]
    with pytest.raises(QhullError):
        build_dsm(line, dsm_step=1.0, engine=eng)
    one_bin = np.array([[1.1, 1.1, 0.0], [1.2, 0.9, 1.0], [0.9, 1.0, 2.0], [1.0, 1.2, 3.0]])
    with pytest.raises(QhullError):
        build_dsm(one_bin, dsm_step=1.0, engine=eng)
