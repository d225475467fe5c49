"""Velocity fields on the device (csrc/binned.hip) against the reference's outputs (tests/golden/g14_velocity.npz), against
`scipy.stats.binned_statistic_dd` on fresh random inputs and against the sequential restatement (tests/binned_oracle.py).

Bound: bit identity. count, sum, mean, std, median and every column of the tracked-point table are compared bit for bit (any NaN equals
any NaN); min and max with == plus an equal NaN mask, because numpy's default argsort leaves the sign of a zero tie in scipy's min / max
undefined. scipy raises on an empty sample: there the expectation is the fill value (0 for count and sum, NaN otherwise)."""
import os
import sys
import types

import numpy as np
import pytest
from scipy.stats import binned_statistic_dd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import binned_oracle as B  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g14():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g14_velocity.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


@pytest.fixture(scope="module")
def M():
    from icepy4d_amd.utils import binned_stats
    return binned_stats


@pytest.fixture(scope="module")
def T():
    from icepy4d_amd.utils import tracking_features_utils
    return tracking_features_utils


def check(name, got, ref, what):
    bad = int((~((got == ref) | (np.isnan(got) & np.isnan(ref)))).sum()) if np.shape(got) == np.shape(ref) else -1
    print(f"{what} {name}: shape {np.shape(got)}, cells that differ as numbers: {bad}")
    assert B.same(name, got, ref), (what, name)


# ---- the fixture, through the public functions ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a2d", "nan", "big"])
def test_golden_2d(g14, eng, M, name):
    c = B.CASES[name]()
    for s in B.STATS:
        xx, yy, st = M.compute_binned_stats2D(c["points"], c["values"], s, c["x_nodes"], c["y_nodes"], engine=eng)
        check(s, st, g14[f"{name}_{s}"], name)
        assert xx.shape == yy.shape == st.shape and np.array_equal(xx[0], c["x_nodes"]) and np.array_equal(yy[:, 0], c["y_nodes"])
    if name == "nan":
        _, _, st = M.compute_binned_stats2D(c["points"], c["values"], "median", c["x_nodes"], c["y_nodes"], engine=eng)
        assert st[0, 5] == 0 and np.signbit(st[0, 5]), "the median of {0.0, -0.0, 5} is -0.0"


def test_golden_auto_nodes_and_display_warning(g14, eng, M):
    c = B.case_auto()
    for s in B.STATS:
        xx, yy, st = M.compute_binned_stats2D(c["points"], c["values"], s, step=c["step"], engine=eng)
        check(s, st, g14[f"auto_{s}"], "auto")
    assert np.array_equal(xx, g14["auto_xx"]) and np.array_equal(yy, g14["auto_yy"])
    with pytest.warns(UserWarning, match="display_results"):
        M.compute_binned_stats2D(c["points"], c["values"], "count", step=c["step"], display_results=True, engine=eng)


def test_golden_3d(g14, eng, M):
    c = B.case_a3d()
    for s in B.STATS:
        xx, yy, zz, st = M.compute_binned_stats3D(c["points"], c["values"], s, c["x_nodes"], c["y_nodes"], c["z_nodes"], engine=eng)
        check(s, st, g14[f"a3d_{s}"], "a3d")
    assert list(xx.shape) == g14["a3d_grid_shape"].tolist() and np.array_equal(xx[:, :, 0], g14["a3d_xx0"])
    assert st.shape == (len(c["x_nodes"]), len(c["y_nodes"]), len(c["z_nodes"]))


def test_golden_sets_in_one_call(g14, eng, M):
    c = B.case_sets()
    out = M.binned_statistics(c["points"], c["values"], B.SETS_STATS, M.bins_from_nodes(c["x_nodes"], c["y_nodes"]), c["offsets"], engine=eng)
    assert list(out) == list(B.SETS_STATS)
    for s in B.SETS_STATS:
        check(s, out[s], g14[f"sets_{s}"], "sets")


# ---- all seven statistics in one call against scipy ----------------------------------------------------------------------------
def random_values(rng, n):
    """Two columns: magnitudes over six decades; and one with a fifth of signed zeros, some NaN and integer ties."""
    a = rng.normal(0, 1, n) * 10.0 ** rng.uniform(-3, 3, n)
    b = np.round(rng.normal(0, 2, n))
    u = rng.random(n)
    b[u < 0.2] = np.where(rng.random(int((u < 0.2).sum())) < 0.5, 0.0, -0.0)
    b[u > 0.97] = np.nan
    return np.stack([a, b])


def scipy_all(points, values, edges):
    if len(points) == 0:
        shape = [len(values)] + [len(e) - 1 for e in edges]
        return {s: np.full(shape, 0.0 if s in ("count", "sum") else np.nan) for s in B.STATS}
    return {s: binned_statistic_dd(points, list(values), s, bins=edges).statistic for s in B.STATS}


def edges_case(name):
    rng = np.random.default_rng({"2d": 1, "3d": 2, "nz1": 3, "one_cell": 4, "n0": 5, "n1": 6, "outside": 7, "edges3000": 8}[name])
    n = {"n0": 0, "n1": 1}.get(name, 4096)
    if name in ("2d", "n0", "n1", "outside"):
        edges = [np.linspace(-3.0, 9.0, 13) + 0.05, np.cumsum(rng.uniform(0.3, 1.2, 10))]
    elif name == "3d":
        edges = [np.linspace(0.0, 6.0, 7), np.linspace(-1.0, 4.0, 6) * 1.1, np.cumsum(rng.uniform(0.5, 1.0, 5))]
    elif name == "nz1":
        edges = [np.linspace(0.0, 6.0, 7), np.linspace(-1.0, 4.0, 6), np.array([0.25, 2.5])]
    elif name == "one_cell":
        edges = [np.array([-1.0, 1.0]), np.array([0.0, 3.0])]
    else:
        edges = [np.cumsum(rng.uniform(1e-3, 2e-3, 3000)), np.array([0.0, 0.5, 1.0, 1.5])]
    lo, hi = np.array([e[0] for e in edges]), np.array([e[-1] for e in edges])
    span = hi - lo
    p = rng.uniform(lo - 0.05 * span, hi + 0.05 * span, (n, len(edges)))
    if name == "outside":
        p[:, 0] = hi[0] + 1.0 + rng.random(n)
    if n > 64:
        p[:16, 0] = edges[0][-1]                   # on the last edge, just beyond it, on an inner edge, on the first
        p[16:24, 0] = edges[0][-1] + 1e-9 * span[0] / 12
        p[24:32, 0] = edges[0][len(edges[0]) // 2]
        p[32:40, 0] = edges[0][0]
    return p, random_values(rng, n), edges


@pytest.mark.parametrize("name", ["2d", "3d", "nz1", "one_cell", "n0", "n1", "outside", "edges3000"])
def test_all_statistics_in_one_call_against_scipy(eng, M, name):
    p, v, edges = edges_case(name)
    ref = scipy_all(p, v, edges)
    out = M.binned_statistics(p, v, B.STATS, edges, engine=eng)
    print(f"{name}: {len(p)} points, {int(ref['count'][0].sum())} inside, largest cell {int(ref['count'].max())}")
    for s in B.STATS:
        assert out[s].shape == (1,) + ref[s].shape
        check(s, out[s][0], ref[s], name)
    one = M.binned_statistics(p, v[1], "median", edges, engine=eng)["median"]        # one statistic, one column: a string and [N] will do
    assert B.bits_equal(one[0, 0], ref["median"][1])


def around_capacity(n, seed):
    """A cell of n points whose two middle ranks fall into a run of signed zeros, next to 300 other points."""
    rng = np.random.default_rng(seed)
    zeros = np.where(rng.random(41) < 0.5, 0.0, -0.0)
    neg = -(10.0 ** rng.uniform(-3, 3, n // 2 - 20))
    pos = 10.0 ** rng.uniform(-3, 3, n - len(neg) - len(zeros))
    v = np.concatenate([neg, zeros, pos, rng.normal(0, 1, 300)])
    p = np.concatenate([np.stack([rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)], 1),
                        np.stack([rng.uniform(1.0, 3.0, 300), rng.uniform(0.0, 2.0, 300)], 1)])
    order = rng.permutation(len(v))
    return p[order], v[order], [np.array([0.0, 1.0, 2.0, 3.0]), np.array([0.0, 1.0, 2.0])]


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_cells_around_the_lds_capacity(eng, M, delta):
    cap = M.lds_cell_capacity()
    p, v, edges = around_capacity(cap + delta, 20 + delta)
    stats = ("median", "std", "sum", "count")
    out = M.binned_statistics(p, v, stats, edges, engine=eng)
    assert out["count"][0, 0, 0, 0] == cap + delta
    for s in stats:
        check(s, out[s][0, 0], binned_statistic_dd(p, v, s, bins=edges).statistic, f"capacity{delta:+d}")
    p2, v2, _ = around_capacity(cap + delta + 1, 30 + delta)      # an odd / even size next to it: the middle rank is one zero
    ref = binned_statistic_dd(p2, v2, "median", bins=edges).statistic
    got = M.binned_statistics(p2, v2, "median", edges, engine=eng)["median"][0, 0]
    assert ref[0, 0] == 0 and B.bits_equal(got, ref), (got[0, 0], ref[0, 0])


def test_device_inputs_and_determinism(eng, M):
    import torch
    p, v, edges = edges_case("2d")
    a = M.binned_statistics(p, v, B.STATS, edges, engine=eng)
    b = M.binned_statistics(p, v, B.STATS, edges, engine=eng)
    c = M.binned_statistics(torch.from_numpy(p).to(eng.device), torch.from_numpy(v).to(eng.device), B.STATS, edges, engine=eng)
    for s in B.STATS:
        assert a[s].tobytes() == b[s].tobytes() == c[s].tobytes(), s


# ---- tracked points ---------------------------------------------------------------------------------------------------------------
def check_table(t, ref, series):
    cols = t.columns()
    assert set(cols) == set(ref)
    for k, r in ref.items():
        ok = np.array_equal(cols[k], r) if r.dtype.kind == "i" else B.bits_equal(cols[k], r)
        assert ok and cols[k].dtype == r.dtype, k
    assert t.series == series and list(t.series) == sorted(t.series)


@pytest.mark.parametrize("run,with_volume,min_eps", B.TRK_RUNS)
def test_tracked_points_table_golden_case(g14, eng, T, run, with_volume, min_eps):
    c = B.case_trk()
    vol = B.TRK_VOLUME if with_volume else None
    img = B.trk_image_points(c)
    for tag, filt in [("f", B.TRK_FILTER), ("u", {})]:
        t = T.tracked_points_table(c["ids"], c["xyz"], c["days"], min_eps, vol, image_points=img, engine=eng, **filt)
        ref, series = B.tracked_table_seq(c["ids"], c["xyz"], c["days"], min_eps, vol, image_points=img, **filt)
        print(f"trk {run} {tag}: {len(t.fid)} rows of {len(series)} tracked ids, {int((t.dt == 0).sum())} with dt = 0")
        check_table(t, ref, series)
        assert series == B.golden_series(g14, run)
        if tag == "f" or run in B.TRK_UNFILTERED:
            import pandas as pd
            pd.testing.assert_frame_equal(t.to_dataframe(B.trk_epoch_dict(c["days"])), B.golden_frame(g14, run, tag), check_exact=True)


def test_dict_wrappers_equal_the_reference(g14, eng, T):
    import pandas as pd
    c = B.case_trk()
    points, features = B.trk_containers(c)
    epoch_dict = B.trk_epoch_dict(c["days"])
    for run, with_volume, min_eps in (B.TRK_RUNS[0], B.TRK_RUNS[3]):
        fts = T.tracked_points_time_series(points, min_tracked_epoches=min_eps, volume=B.TRK_VOLUME if with_volume else None, engine=eng)
        assert fts == B.golden_series(g14, run) and list(fts) == list(B.golden_series(g14, run))
        df = T.tracked_dict_to_df(features, points, epoch_dict, fts, engine=eng, **B.TRK_FILTER)
        pd.testing.assert_frame_equal(df, B.golden_frame(g14, run, "f"), check_exact=True)
        df = T.tracked_dict_to_df(features, points, epoch_dict, fts, engine=eng)
        pd.testing.assert_frame_equal(df, B.golden_frame(g14, run, "u"), check_exact=True)


@pytest.mark.parametrize("name", ["random", "one_epoch", "single_ids", "empty_epochs", "lists"])
def test_tracked_points_table_against_the_restatement(eng, T, name):
    kw = dict(min_tracked_epoches=2, volume=B.TRK_VOLUME, min_dt=2, vy_lims=[-0.2, 0.1], vz_lims=[-0.03, 0.03])
    if name == "random":
        c = B.case_trk(seed=77, n_ids=1500, days=[3, 3, 5, 8, 8, 13, 21, 40], p_present=0.4)
    elif name == "one_epoch":
        c, kw = B.case_trk(seed=78, n_ids=50, days=[7]), dict(min_tracked_epoches=1)
    elif name == "single_ids":                       # every id occurs in one epoch only: d = 0, dt = 0, v = NaN
        c, kw = B.case_trk(seed=79, n_ids=60, days=[0, 2, 5]), dict()
        c["ids"] = [i + 1000 * e for e, i in enumerate(c["ids"])]
    elif name == "empty_epochs":
        c, kw = B.case_trk(seed=80, n_ids=80, days=[0, 1, 2, 6, 9]), dict(min_dt=1)
        for e in (0, 2, 4):
            c["ids"][e], c["xyz"][e] = c["ids"][e][:0], c["xyz"][e][:0]
            c["img"][e] = {cam: a[:0] for cam, a in c["img"][e].items()}
    else:                                            # the per-epoch views of `triangulate_table`'s TableReconstruction.points3d
        c = B.case_trk(seed=81, n_ids=200, days=[0, 10, 20])
        whole = np.concatenate(c["xyz"])
        offs = np.concatenate([[0], np.cumsum([len(x) for x in c["xyz"]])])
        rec = types.SimpleNamespace(points3d=[whole[offs[e]:offs[e + 1]] for e in range(3)])
        c["xyz"] = rec.points3d
    img = B.trk_image_points(c)
    t = T.tracked_points_table(c["ids"], c["xyz"], c["days"], image_points=img, engine=eng, **kw)
    ref, series = B.tracked_table_seq(c["ids"], c["xyz"], c["days"], image_points=img, **kw)
    print(f"{name}: {len(t.fid)} rows of {len(series)} tracked ids")
    check_table(t, ref, series)
    if name == "single_ids":
        assert len(t.fid) == sum(len(i) for i in c["ids"]) and np.isnan(t.V).all() and (t.num_tracked_eps == 1).all()
    if name == "empty_epochs":
        all_empty = T.tracked_points_table([i[:0] for i in c["ids"]], [x[:0] for x in c["xyz"]], c["days"], engine=eng)
        assert len(all_empty.fid) == 0 and all_empty.series == {}
