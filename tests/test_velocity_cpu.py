"""Velocity fields without a GPU: the sequential restatement (tests/binned_oracle.py) against the reference's outputs
(tests/golden/g14_velocity.npz, written by tools/gen_golden_binned.py), bit for bit; the host-side parts of
`icepy4d_amd.utils.binned_stats` / `tracking_features_utils` (edges, argument validation); the C ABI of csrc/binned.hip."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import binned_oracle as B  # noqa: E402

NEW_SYMBOLS = ("im_binned_lds_capacity", "im_binned_cells", "im_binned_stats", "im_tracked_points")


@pytest.fixture(scope="module")
def g14():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g14_velocity.npz"), allow_pickle=False))


@pytest.mark.parametrize("name", list(B.CASES) + ["trk"])
def test_input_hashes(g14, name):
    for k, h in B.input_hashes(name).items():
        assert str(g14[f"{name}_hash_{k}"].reshape(-1)[0]) == h, (name, k)


@pytest.mark.parametrize("name", ["a2d", "nan", "big"])
def test_restatement_2d(g14, name):
    c = B.CASES[name]()
    out = B.binned_statistics_seq(c["points"], c["values"], B.STATS, [g14[f"{name}_binx"], g14[f"{name}_biny"]])
    for s in B.STATS:
        assert B.same(s, out[s][0, 0].T, g14[f"{name}_{s}"]), (name, s)


def test_restatement_auto_nodes(g14):
    from icepy4d_amd.utils import binned_stats as M
    c = B.case_auto()
    xn, yn = g14["auto_xx"][0], g14["auto_yy"][:, 0]
    out = B.binned_statistics_seq(c["points"], c["values"], B.STATS, M.bins_from_nodes(xn, yn))
    for s in B.STATS:
        assert B.same(s, out[s][0, 0].T, g14[f"auto_{s}"]), s


def test_restatement_3d(g14):
    c = B.case_a3d()
    out = B.binned_statistics_seq(c["points"], c["values"], B.STATS, [g14["a3d_binx"], g14["a3d_biny"], g14["a3d_binz"]])
    for s in B.STATS:
        assert B.same(s, out[s][0, 0], g14[f"a3d_{s}"]), s
    assert g14["a3d_grid_shape"].tolist() == [len(c["y_nodes"]), len(c["x_nodes"]), len(c["z_nodes"])]


def test_restatement_sets(g14):
    from icepy4d_amd.utils import binned_stats as M
    c = B.case_sets()
    out = B.binned_statistics_seq(c["points"], c["values"], B.SETS_STATS, M.bins_from_nodes(c["x_nodes"], c["y_nodes"]), c["offsets"])
    for s in B.SETS_STATS:
        assert B.bits_equal(out[s], g14[f"sets_{s}"]), s


@pytest.mark.parametrize("run,with_volume,min_eps", B.TRK_RUNS)
def test_restatement_tracked_table(g14, run, with_volume, min_eps):
    c = B.case_trk()
    vol = B.TRK_VOLUME if with_volume else None
    frames = [("f", B.TRK_FILTER)] + ([("u", {})] if run in B.TRK_UNFILTERED else [])
    for tag, filt in frames:
        table, series = B.tracked_table_seq(c["ids"], c["xyz"], c["days"], min_eps, vol, image_points=B.trk_image_points(c), **filt)
        assert series == B.golden_series(g14, run)
        assert np.array_equal(table["index"], g14[f"trk_{run}_{tag}_index"])
        assert np.array_equal(table["dt"] * 86400 * 10 ** 9, g14[f"trk_{run}_{tag}_dt"])
        for col in g14["trk_columns"].tolist():
            if col in ("dt", "date_ini", "date_fin"):
                continue
            ref = g14[f"trk_{run}_{tag}_{col}"]
            ok = np.array_equal(table[col], ref) if ref.dtype.kind == "i" else B.bits_equal(table[col], ref)
            assert ok, (run, tag, col)
    if run == "all_1":
        u = g14["trk_all_1_u_vX"]
        assert np.isinf(u).any() and np.isnan(u).any(), "dt = 0 rows"


def test_edges_of_the_module(g14):
    from icepy4d_amd.utils import binned_stats as M
    for name in ("a2d", "nan", "big"):
        c = B.CASES[name]()
        bx, by = M.bins_from_nodes(c["x_nodes"], c["y_nodes"])
        assert np.array_equal(np.array(bx), g14[f"{name}_binx"]) and np.array_equal(np.array(by), g14[f"{name}_biny"])
    c = B.case_a3d()
    for k, e in zip("xyz", M.bins_from_nodes3D(c["x_nodes"], c["y_nodes"], c["z_nodes"])):
        assert np.array_equal(np.array(e), g14[f"a3d_bin{k}"])
    assert g14["a3d_binz"][-1] - g14["a3d_binz"][-2] == 1.0, "the z half-width is the x step's"


def test_argument_validation():
    from icepy4d_amd.utils import binned_stats as M
    from icepy4d_amd.utils import tracking_features_utils as T
    p, v, xn = np.zeros((4, 2)), np.zeros(4), np.arange(4.0)
    with pytest.raises(ValueError, match="invalid statistic 'var'"):
        M.compute_binned_stats2D(p, v, "var", xn, xn)
    with pytest.raises(ValueError):
        M.compute_binned_stats3D(np.zeros((4, 3)), v, "var", xn, xn, xn)
    with pytest.raises(NotImplementedError):
        M.compute_binned_stats2D(p, v, np.mean, xn, xn)
    with pytest.raises(NotImplementedError):
        M.binned_statistics(p, v, ("mean", np.median), [xn, xn])
    with pytest.raises(AssertionError):
        M.compute_binned_stats2D(p, v, "mean", xn, np.arange(4.0) * 2)
    with pytest.raises(AssertionError):
        M.bins_from_nodes3D(xn, xn * 2, xn)
    with pytest.raises(AssertionError):
        M.compute_binned_stats2D(p, v, "mean")                      # no nodes, no step
    with pytest.raises(ValueError, match="more than once"):
        T.tracked_points_table([np.array([3, 5, 3])], [np.zeros((3, 3))], [0])
    with pytest.raises(ValueError):
        T.tracked_points_table([np.array([3, 5])], [np.zeros((3, 3))], [0])


def test_new_symbols_are_declared_bound_and_built():
    from icepy4d_amd import _lib
    header = open(os.path.join(ROOT, "include", "icematch.h")).read()
    declared = set(re.findall(r"\b(im_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    from icepy4d_amd.utils import binned_stats as M
    assert M.lds_cell_capacity() == lib.im_binned_lds_capacity() > 64


@pytest.mark.parametrize("first", ["sfm", "utils.binned_stats", "utils.point_cloud_filters", "utils.homography", "utils.dsm_orthophoto",
                                   "matching.templatematch"])
def test_every_module_can_be_the_first_import(first):
    """`sfm` imports `matching`, which imports `utils`, which imports the velocity modules: these must not need `sfm` at import time, and
    the stage modules do not need it at all (the engine they default to comes from `engine`, not through `sfm`).
    A fresh interpreter, because the order of the imports in this process is the suite's."""
    import subprocess
    no_sfm = first in ("utils.point_cloud_filters", "utils.homography", "utils.dsm_orthophoto", "matching.templatematch")
    code = (f"import sys, icepy4d_amd.{first}; assert not {no_sfm} or 'icepy4d_amd.sfm' not in sys.modules, 'imports sfm'; "
            "from icepy4d_amd import sfm, utils; from icepy4d_amd.engine import default_engine; "
            "assert callable(utils.binned_stats.binned_statistics) and callable(utils.tracking_features_utils.tracked_points_table)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
