"""Velocity fields: the procedural inputs of tests/golden/g14_velocity.npz (tools/gen_golden_binned.py) and a sequential numpy
restatement of what the reference computes from them (`utils/binned_stats.py` over `scipy.stats.binned_statistic_dd`,
`utils/tracking_features_utils.py`: `tracked_points_time_series`, `tracked_dict_to_df`).

The restatement walks every cell in input order with Python floats (IEEE double, one rounding per operation, no fused multiply-add):
sum = np.bincount's order, std from the same sums, the median from a stable sort of the cell (numbers compare as numbers: -0.0 == 0.0,
NaN last), min ignoring NaN, max NaN when the cell holds one. tests/test_velocity_cpu.py pins it to the fixture bit for bit; the
device code (csrc/binned.hip) is then compared with it on other inputs."""
import hashlib
import math
from datetime import date, timedelta

import numpy as np

STATS = ("count", "sum", "mean", "std", "min", "max", "median")
SEEDS = {"a2d": 1401, "nan": 1402, "auto": 1403, "a3d": 1404, "big": 1405, "sets": 1406, "trk": 1407}
NAN = float("nan")


def sha(a) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def bits_equal(a, b) -> bool:
    """Same shape and the same bits, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


def values_equal(a, b) -> bool:
    """== plus an equal NaN mask (min / max: numpy's default argsort leaves the sign of a zero tie undefined)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


def same(name, a, b) -> bool:
    return values_equal(a, b) if name in ("min", "max") else bits_equal(a, b)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def edges_of(nodes, step):
    return np.array([v - step / 2 for v in nodes] + [nodes[-1] + step / 2], np.float64)


def case_a2d():
    rng = np.random.default_rng(SEEDS["a2d"])
    step = 0.7
    xn, yn = np.arange(18) * step, np.arange(13) * step
    bx, by = edges_of(xn, xn[1] - xn[0]), edges_of(yn, xn[1] - xn[0])
    n = 6000
    p = np.stack([rng.uniform(bx[0] - 0.6, bx[-1] + 0.6, n), rng.uniform(by[0] - 0.6, by[-1] + 0.6, n)], 1)
    k = 0
    for d, e in ((0, bx), (1, by)):
        special = [e[3], e[7], e[0], np.nextafter(e[0], -np.inf), e[-1], np.nextafter(e[-1], np.inf)] + [e[-1] + 1e-9] * 10 + [e[-1] + 1e-5] * 4
        for s in special:
            p[k, d] = s
            p[k, 1 - d] = (by, bx)[d][2] + 0.3 + 0.01 * (k % 7)      # well inside in the other dimension
            k += 1
    v = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)
    ties = rng.choice(np.arange(k, n), 60, replace=False)
    v[ties] = rng.integers(0, 4, 60).astype(np.float64)
    return dict(points=p, values=v, x_nodes=xn, y_nodes=yn)


def case_nan():
    rng = np.random.default_rng(SEEDS["nan"])
    xn, yn = np.arange(6) * 1.0, np.arange(5) * 1.0
    n = 800
    p = np.stack([rng.uniform(-0.5, 4.5, n), rng.uniform(-0.5, 4.5, n)], 1)       # the column of x node 5 is hand-made below
    v = rng.normal(0, 3, n)
    p[rng.choice(n, 20, replace=False), rng.integers(0, 2, 20)] = np.nan
    v[rng.choice(n, 40, replace=False)] = np.nan
    z = rng.choice(n, 60, replace=False)
    v[z] = np.where(rng.random(60) < 0.5, 0.0, -0.0)
    cells = {0: [0.0, -0.0, 5.0], 1: [-0.0, 0.0], 2: [np.nan, 1.0, 2.0], 3: [np.nan, np.nan], 4: [-0.0, -0.0, 0.0, 0.0, -3.0, 7.0]}
    hp = [(5.0 + 0.1 * i, float(row)) for row, vals in cells.items() for i in range(len(vals))]
    hv = [x for vals in cells.values() for x in vals]
    return dict(points=np.concatenate([p, np.array(hp)]), values=np.concatenate([v, np.array(hv)]), x_nodes=xn, y_nodes=yn)


def case_auto():
    rng = np.random.default_rng(SEEDS["auto"])
    n = 1500
    p = np.stack([rng.uniform(-7.3, 21.9, n), rng.uniform(3.2, 17.8, n)], 1)
    return dict(points=p, values=rng.normal(1.0, 2.0, n), step=2.5)


def case_a3d():
    rng = np.random.default_rng(SEEDS["a3d"])
    xn, yn, zn = np.arange(6) * 1.0, np.arange(5) * 1.0, np.arange(8) * 0.5    # z spacing = step / 2: the z bins still use the x step
    n = 3000
    p = np.stack([rng.uniform(-0.9, 5.9, n), rng.uniform(-0.9, 4.9, n), rng.uniform(-0.9, 4.4, n)], 1)
    p[:6, 2] = [-0.5, 0.0, 3.0, 4.0, 4.0 + 1e-9, 4.0 + 1e-5]
    p[:6, :2] = 2.2
    return dict(points=p, values=rng.normal(0, 1, n) * 10.0 ** rng.uniform(-2, 2, n), x_nodes=xn, y_nodes=yn, z_nodes=zn)


def case_big():
    rng = np.random.default_rng(SEEDS["big"])
    xn, yn = np.arange(4) * 1.0, np.arange(4) * 1.0
    p = np.concatenate([np.stack([rng.uniform(1.5, 2.5, 20000), rng.uniform(0.5, 1.5, 20000)], 1),
                        np.stack([rng.uniform(-0.5, 3.5, 200), rng.uniform(-0.5, 3.5, 200)], 1)])
    p = p[rng.permutation(len(p))]
    v = rng.normal(0, 1, len(p)) * 10.0 ** rng.uniform(-3, 3, len(p))
    v[rng.choice(len(p), 300, replace=False)] = rng.integers(-2, 3, 300).astype(np.float64)
    return dict(points=p, values=v, x_nodes=xn, y_nodes=yn)


SETS_STATS = ("median", "mean", "count", "std")


def case_sets():
    rng = np.random.default_rng(SEEDS["sets"])
    xn, yn = np.arange(9) * 2.0, np.arange(7) * 2.0
    sizes = [700, 0, 500]
    n = sum(sizes)
    p = np.stack([rng.uniform(-1.5, 17.5, n), rng.uniform(-1.5, 13.5, n)], 1)
    v = rng.normal(0, 1, (4, n)) * 10.0 ** rng.uniform(-2, 2, (4, n))
    return dict(points=p, values=v, offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), x_nodes=xn, y_nodes=yn)


TRK_DAYS = [0, 1, 1, 4, 9, 30]
TRK_CAMS = ("cam0", "cam1")
TRK_VOLUME = np.array([[-40.0, -30.0, 90.0], [55.0, 60.0, 130.0]])
TRK_RUNS = [("all_1", False, 1), ("all_2", False, 2), ("vol_1", True, 1), ("vol_2", True, 2)]      # name, volume, min_tracked_epoches
TRK_FILTER = dict(min_dt=1, vx_lims=[0, 0.2])
TRK_UNFILTERED = ("all_1", "vol_2")


def case_trk(seed=SEEDS["trk"], n_ids=400, days=TRK_DAYS, p_present=0.6):
    """Per epoch: ids (shuffled), xyz [n, 3] and the image points [n, 2] of two cameras."""
    rng = np.random.default_rng(seed)
    base = np.stack([rng.uniform(-60, 80, n_ids), rng.uniform(-50, 90, n_ids), rng.uniform(80, 140, n_ids)], 1)
    vel = np.stack([rng.normal(0.1, 0.08, n_ids), rng.normal(-0.05, 0.1, n_ids), rng.normal(0, 0.02, n_ids)], 1)
    all_ids = rng.permutation(5 * n_ids)[:n_ids].astype(np.int64)
    ids, xyz, img = [], [], []
    for d in days:
        here = np.flatnonzero(rng.random(n_ids) < p_present)
        here = here[rng.permutation(len(here))]
        ids.append(all_ids[here])
        xyz.append(base[here] + vel[here] * d + rng.normal(0, 0.01, (len(here), 3)))
        img.append({cam: rng.uniform(0, 4000, (len(here), 2)) for cam in TRK_CAMS})
    return dict(ids=ids, xyz=xyz, img=img, days=np.asarray(days, np.int64))


def trk_epoch_dict(days):
    return {ep: (date(2022, 5, 1) + timedelta(days=int(d))).strftime("%Y_%m_%d") for ep, d in enumerate(days)}


CASES = {"a2d": case_a2d, "nan": case_nan, "auto": case_auto, "a3d": case_a3d, "big": case_big, "sets": case_sets}


def input_hashes(name):
    c = case_trk() if name == "trk" else CASES[name]()
    if name == "trk":
        arrs = {"ids": np.concatenate(c["ids"]), "xyz": np.concatenate(c["xyz"]), "days": c["days"]}
        for cam in TRK_CAMS:
            arrs["img_" + cam] = np.concatenate([e[cam] for e in c["img"]])
    else:
        arrs = {k: np.asarray(v) for k, v in c.items() if k != "step"}
    return {k: sha(v) for k, v in arrs.items()}


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def bin_numbers(sample, edges):
    """scipy's `_bin_numbers`: the row-major cell of every point, -1 outside."""
    sample = np.asarray(sample, np.float64).reshape(len(sample), len(edges))
    cell = np.zeros(len(sample), np.int64)
    inside = np.ones(len(sample), bool)
    for d, e in enumerate(edges):
        e = np.asarray(e, np.float64)
        x = sample[:, d]
        b = np.searchsorted(e, x, side="right")            # np.digitize for ascending edges; NaN sorts behind every edge
        decimal = int(-np.log10(np.diff(e).min())) + 6
        with np.errstate(invalid="ignore"):
            on_edge = (x >= e[-1]) & (np.around(x, decimal) == np.around(e[-1], decimal))
        b = b - on_edge
        inside &= (b >= 1) & (b <= len(e) - 1)
        cell = cell * (len(e) - 1) + (b - 1)
    return np.where(inside, cell, -1)


def cell_statistics(vals, statistics):
    """One cell's values in input order -> {name: float}."""
    n = len(vals)
    out = {}
    v = [float(x) for x in vals]
    s = 0.0
    for x in v:
        s += x
    if "count" in statistics:
        out["count"] = float(n)
    if "sum" in statistics:
        out["sum"] = s
    if "mean" in statistics:
        out["mean"] = s / n if n else NAN
    if "std" in statistics:
        if n:
            mu, q = s / n, 0.0
            for x in v:
                q += (x - mu) * (x - mu)
            out["std"] = math.sqrt(q / n)
        else:
            out["std"] = NAN
    if "min" in statistics:
        fin = [x for x in v if x == x]
        out["min"] = min(fin) if fin else NAN
    if "max" in statistics:
        out["max"] = NAN if (not n or any(x != x for x in v)) else max(v)
    if "median" in statistics:
        if n:
            a = np.asarray(v, np.float64)
            a = a[np.argsort(a, kind="stable")]
            out["median"] = float((a[(n - 1) // 2] + a[n // 2]) / 2)
        else:
            out["median"] = NAN
    return out


def binned_statistics_seq(points, values, statistics, edges, offsets=None):
    """{name: [E, V, n0, n1(, n2)]} as `icepy4d_amd.utils.binned_stats.binned_statistics` returns it."""
    values = np.atleast_2d(np.asarray(values, np.float64))
    n = values.shape[1]
    offsets = np.array([0, n]) if offsets is None else np.asarray(offsets)
    nb = [len(e) - 1 for e in edges]
    C = int(np.prod(nb))
    cell = bin_numbers(points, edges) if n else np.zeros(0, np.int64)
    E, V = len(offsets) - 1, len(values)
    out = {s: np.empty((E, V, C)) for s in statistics}
    for e in range(E):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        order = np.argsort(cell[lo:hi], kind="stable") + lo
        sc = cell[order]
        first = np.searchsorted(sc, np.arange(C + 1))
        for c in range(C):
            idx = order[first[c]:first[c + 1]]
            for k in range(V):
                for name, x in cell_statistics(values[k, idx], statistics).items():
                    out[name][e, k, c] = x
    return {s: a.reshape([E, V] + nb) for s, a in out.items()}


INT_COLS = ("fid", "num_tracked_eps", "ep_ini", "ep_fin", "dt", "index")
F64_COLS = ("X_ini", "Y_ini", "Z_ini", "X_fin", "Y_fin", "Z_fin", "dX", "dY", "dZ", "vX", "vY", "vZ", "V")


def tracked_table_seq(ids, xyz, days, min_tracked_epoches=1, volume=None, min_dt=None, vx_lims=None, vy_lims=None, vz_lims=None,
                      image_points=None):
    """The table as a dict of columns, and {id: [epoch indices]} of the tracked ids (ascending ids)."""
    lo = hi = None
    if volume is not None:
        volume = np.asarray(volume, np.float64)
        lo, hi = volume.min(0), volume.max(0)
    series = {}
    for ep, (ii, pp) in enumerate(zip(ids, xyz)):
        for row, (i, p) in enumerate(zip(np.asarray(ii).tolist(), np.asarray(pp, np.float64).reshape(-1, 3))):
            if lo is not None and not all(lo[k] <= p[k] <= hi[k] for k in range(3)):
                continue
            series.setdefault(i, []).append((ep, row))
    series = {i: s for i, s in sorted(series.items()) if len(s) >= min_tracked_epoches}
    cams = list(image_points) if image_points else []
    names = list(INT_COLS) + list(F64_COLS) + [f"{a}_{cam}_{s}" for cam in cams for s in ("ini", "fin") for a in ("x", "y")]
    cols = {k: [] for k in names}
    with np.errstate(divide="ignore", invalid="ignore"):
        for index, (i, s) in enumerate(series.items()):
            (e0, r0), (e1, r1) = s[0], s[-1]
            p0, p1 = np.asarray(xyz[e0], np.float64)[r0], np.asarray(xyz[e1], np.float64)[r1]
            dt = int(days[e1]) - int(days[e0])
            d = p1 - p0
            v = d / np.float64(dt)
            V = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            keep = min_dt is None or dt >= min_dt
            for k, lim in enumerate((vx_lims, vy_lims, vz_lims)):
                if lim is not None:
                    keep = keep and bool(v[k] >= lim[0]) and bool(v[k] < lim[1])
            if not keep:
                continue
            row = [i, len(s), e0, e1, dt, index] + list(p0) + list(p1) + list(d) + list(v) + [V]
            for cam in cams:
                row += list(np.asarray(image_points[cam][e0], np.float64)[r0]) + list(np.asarray(image_points[cam][e1], np.float64)[r1])
            for k, x in zip(names, row):
                cols[k].append(x)
    table = {k: np.asarray(c, np.int64 if k in INT_COLS else np.float64) for k, c in cols.items()}
    return table, {i: [ep for ep, _ in s] for i, s in series.items()}


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def golden_series(g, run):
    ids, mask = g[f"trk_{run}_series_ids"], g[f"trk_{run}_series_mask"]
    return {int(i): np.flatnonzero(m).tolist() for i, m in zip(ids, mask)}


def golden_frame(g, run, tag):
    """The reference's DataFrame of run ("all_1", ..) and tag ("f": filtered by TRK_FILTER, "u": unfiltered) from its stored columns."""
    import pandas as pd
    d = {}
    for col, dtype in zip(g["trk_columns"].tolist(), g["trk_dtypes"].tolist()):
        a = g[f"trk_{run}_{tag}_{col}"]
        d[col] = a.view(dtype) if dtype[0] in "dt" and "64[" in dtype else a.astype(dtype)
    return pd.DataFrame(d, index=pd.Index(g[f"trk_{run}_{tag}_index"], dtype="int64"))


def trk_image_points(c):
    return {cam: [e[cam] for e in c["img"]] for cam in TRK_CAMS}


class Item:
    """A stand-in point / feature: only the accessors the wrappers may use."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Container:
    def __init__(self, ids, items):
        self._d = dict(zip(ids, items))

    def get_track_ids(self):
        return tuple(self._d)

    def __getitem__(self, i):
        return self._d[i]


def trk_containers(c):
    """(points, features): {epoch: container}, {epoch: {cam: container}} as the reference's dict-like classes."""
    points, features = {}, {}
    for ep, (ids, xyz, img) in enumerate(zip(c["ids"], c["xyz"], c["img"])):
        ids = [int(i) for i in ids]
        points[ep] = Container(ids, [Item(coordinates=p, X=p[0], Y=p[1], Z=p[2]) for p in xyz])
        features[ep] = {cam: Container(ids, [Item(x=q[0], y=q[1]) for q in img[cam]]) for cam in TRK_CAMS}
    return points, features
