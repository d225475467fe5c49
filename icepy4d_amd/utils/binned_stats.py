"""Binned statistics of point values (reference `src/icepy4d/utils/binned_stats.py`): `bins_from_nodes`, `bins_from_nodes3D`,
`compute_binned_stats2D` and `compute_binned_stats3D` with the reference's names, signatures and outputs, and `binned_statistics`, one
binning pass for several value columns, statistics and point sets. The reference goes through `scipy.stats.binned_statistic_2d / _dd`;
here the cell of every point, the grouping and every statistic are computed on the device (csrc/binned.hip: `im_binned_cells`,
`im_binned_stats`; the one stable sort by (set, cell) is torch's). Every entry point takes an optional `engine=` (default: the shared
engine of device 0); there is no CPU fallback: without a HIP device the calls raise.

Numerics (tests/test_gpu_velocity.py, g14): count, sum, mean, std and median are bit-identical to scipy's; min and max are equal as
numbers (numpy's default argsort leaves the sign of a zero tie in scipy's min / max undefined)."""
import warnings

import numpy as np
import torch

from .._lib import ptr
from ..engine import default_engine, to_device

STATISTICS = ("count", "sum", "mean", "std", "min", "max", "median")      # the order of `im_binned_stats`' h_slots


def lds_cell_capacity() -> int:
    """The largest cell (in points) whose median is selected in LDS; larger cells are selected from global memory."""
    from .._lib import load
    return int(load().im_binned_lds_capacity())


def bins_from_nodes(x_nodes, y_nodes):
    """Divides a 2D space into bins based on the x and y coordinates of the nodes: (binx, biny), the boundaries of the bins."""
    step = x_nodes[1] - x_nodes[0]
    assert step == y_nodes[1] - y_nodes[0], "Invalid input. Different step for x and y is not yet supported."
    binx = [x - step / 2 for x in x_nodes]
    binx.append(x_nodes[-1] + step / 2)
    biny = [x - step / 2 for x in y_nodes]
    biny.append(y_nodes[-1] + step / 2)
    return (binx, biny)


def bins_from_nodes3D(x_nodes, y_nodes, z_nodes):
    """(binx, biny, binz). As in the reference, the z half-width is the x step's."""
    step = x_nodes[1] - x_nodes[0]
    assert step == y_nodes[1] - y_nodes[0], "Invalid input. Different step for x and y is not yet supported."
    binx = [v - step / 2 for v in x_nodes]
    binx.append(x_nodes[-1] + step / 2)
    biny = [v - step / 2 for v in y_nodes]
    biny.append(y_nodes[-1] + step / 2)
    binz = [v - step / 2 for v in z_nodes]
    binz.append(z_nodes[-1] + step / 2)
    return (binx, biny, binz)


def _check_statistic(statistic):
    if callable(statistic):
        raise NotImplementedError("binned statistics on the device: a callable statistic is not supported; use one of " + ", ".join(STATISTICS))
    if statistic not in STATISTICS:
        raise ValueError(f"invalid statistic {statistic!r}")      # scipy's message


def _device_f64(x, dev):
    return x.to(device=dev, dtype=torch.float64).contiguous() if isinstance(x, torch.Tensor) else to_device(x, dev, np.float64)


def binned_statistics(points, values, statistics, edges, offsets=None, engine=None):
    """One binning pass: `points` [N, D] (D = 2 or 3; or a sequence of D coordinate arrays), `values` [V, N] (or [N]), `statistics` a
    tuple of names out of count, sum, mean, std, min, max, median, `edges` the D ascending edge arrays, `offsets` [E + 1] the rows of E
    point sets that share the edges (default: one set). Returns {name: float64 [E, V, n0, n1(, n2)]}, n_d = len(edges[d]) - 1, in scipy's
    axis order. Inputs may be device tensors (they are then not copied to the host and back)."""
    statistics = (statistics,) if isinstance(statistics, str) or callable(statistics) else tuple(statistics)
    for s in statistics:
        _check_statistic(s)
    if len(set(statistics)) != len(statistics):
        raise ValueError("binned_statistics: a statistic is named twice")
    edges = [np.ascontiguousarray(e, dtype=np.float64).ravel() for e in edges]
    D = len(edges)
    if D not in (2, 3):
        raise ValueError(f"binned_statistics: 2 or 3 dimensions are supported (got {D})")
    scale, mode = [], []
    for e in edges:
        if len(e) < 2 or not np.isfinite(e).all() or not (np.diff(e) >= 0).all():
            raise ValueError("binned_statistics: every dimension needs two or more finite, ascending edges")
        dmin = np.diff(e).min()
        if dmin == 0:
            raise ValueError("The smallest edge difference is numerically 0.")      # scipy's message
        decimal = int(-np.log10(dmin)) + 6
        scale.append(10.0 ** abs(decimal))
        mode.append(int(np.sign(decimal)))
    eng = default_engine(engine)
    dev = eng.device
    if not isinstance(points, torch.Tensor) and not isinstance(points, np.ndarray):
        points = np.stack([np.asarray(c, np.float64).ravel() for c in points], 1)
    pts = _device_f64(points, dev)
    if pts.ndim != 2 or pts.shape[1] != D:
        raise ValueError(f"binned_statistics: points must be [N, {D}] (got {tuple(pts.shape)})")
    N = pts.shape[0]
    vals = _device_f64(values, dev)
    vals = vals.reshape(1, -1) if vals.ndim <= 1 else vals
    if vals.ndim != 2 or vals.shape[1] != N or vals.shape[0] < 1:
        raise AttributeError("The number of `values` elements must match the length of each `sample` dimension.")    # scipy's
    V = vals.shape[0]
    offs = np.array([0, N], np.int64) if offsets is None else np.ascontiguousarray(torch.as_tensor(offsets).cpu().numpy(), dtype=np.int64)
    if offs.ndim != 1 or len(offs) < 2 or offs[0] != 0 or offs[-1] != N or (np.diff(offs) < 0).any():
        raise ValueError("binned_statistics: offsets must ascend from 0 to the number of points")
    E = len(offs) - 1
    nb = [len(e) - 1 for e in edges]
    C = int(np.prod(nb))
    st = eng.stream_ptr()
    d_edges, d_offs = to_device(np.concatenate(edges), dev), to_device(offs, dev)
    key = torch.empty(N, dtype=torch.int64, device=dev)
    n_edges = np.array([len(e) for e in edges], np.int32)
    h_scale, h_mode = np.array(scale, np.float64), np.array(mode, np.int32)
    eng.ctx.call("im_binned_cells", ptr(pts), N, D, ptr(d_edges), n_edges.ctypes.data, h_scale.ctypes.data, h_mode.ctypes.data, ptr(d_offs), E,
                 ptr(key), st)
    skey, perm = torch.sort(key, stable=True)
    slots = np.full(len(STATISTICS), -1, np.int32)
    for k, s in enumerate(statistics):
        slots[STATISTICS.index(s)] = k
    out = torch.empty((len(statistics), E, V) + tuple(nb), dtype=torch.float64, device=dev)
    eng.ctx.call("im_binned_stats", ptr(skey), ptr(perm), N, E, C, ptr(vals), V, slots.ctypes.data, ptr(out), st)
    host = out.cpu().numpy()
    return {s: host[k] for k, s in enumerate(statistics)}


def _ignore_display(display_results):
    if display_results:
        warnings.warn("display_results=True is ignored: plots are not part of this library", stacklevel=3)


def compute_binned_stats2D(points_xy, points_values, statistic="count", x_nodes=None, y_nodes=None, step=None, display_results=False,
                           title=None, engine=None):
    """`compute_binned_stats2D` of the reference (`binned_stats.py:135-194`): (xx_nodes, yy_nodes, statistic), the meshgrids of the nodes
    and the statistic of `points_values` over the bins around the nodes, [len(y_nodes), len(x_nodes)]. Without nodes they are
    np.arange(floor(min), ceil(max) + step, step) per axis."""
    _check_statistic(statistic)
    _ignore_display(display_results)
    if x_nodes is None or y_nodes is None:
        assert step is not None, "Missing 'step' value. Unable to compute nodes grid"
        x_nodes = np.arange(np.floor(min(points_xy[:, 0])), np.ceil(max(points_xy[:, 0])) + step, step)
        y_nodes = np.arange(np.floor(min(points_xy[:, 1])), np.ceil(max(points_xy[:, 1])) + step, step)
    binx, biny = bins_from_nodes(x_nodes, y_nodes)
    pts = np.stack([np.asarray(points_xy[:, 0], np.float64).flatten(), np.asarray(points_xy[:, 1], np.float64).flatten()], 1)
    ret = binned_statistics(pts, np.asarray(points_values, np.float64).flatten(), (statistic,), [binx, biny], engine=engine)[statistic][0, 0]
    xx_nodes, yy_nodes = np.meshgrid(x_nodes, y_nodes)
    return (xx_nodes, yy_nodes, ret.T)


def compute_binned_stats3D(points_xyz, points_values, statistic="count", x_nodes=None, y_nodes=None, z_nodes=None, step=None, engine=None):
    """`compute_binned_stats3D` of the reference (`binned_stats.py:224-279`): (xx_nodes, yy_nodes, zz_nodes, statistic). As there, the
    meshgrids are numpy's default 'xy' ones, [ny, nx, nz], next to a statistic of shape [nx, ny, nz]."""
    _check_statistic(statistic)
    if x_nodes is None or y_nodes is None:
        assert step is not None, "Missing 'step' value. Unable to compute nodes grid"
        x_nodes = np.arange(np.floor(min(points_xyz[:, 0])), np.ceil(max(points_xyz[:, 0])) + step, step)
        y_nodes = np.arange(np.floor(min(points_xyz[:, 1])), np.ceil(max(points_xyz[:, 1])) + step, step)
        z_nodes = np.arange(np.floor(min(points_xyz[:, 2])), np.ceil(max(points_xyz[:, 2])) + step, step)
    binx, biny, binz = bins_from_nodes3D(x_nodes, y_nodes, z_nodes)
    ret = binned_statistics(np.asarray(points_xyz, np.float64), np.asarray(points_values, np.float64).flatten(), (statistic,),
                            [binx, biny, binz], engine=engine)[statistic][0, 0]
    xx_nodes, yy_nodes, zz_nodes = np.meshgrid(x_nodes, y_nodes, z_nodes)
    return (xx_nodes, yy_nodes, zz_nodes, ret)
