"""Co-registration of two epoch clouds on the device: the ICP between "clouds exist" and "clouds are compared" (Open3D's
`pipelines.registration.registration_icp` and `evaluate_registration`, CloudCompare's fine registration), run on stable terrain so that
`m3c2(..., registration_error=result.inlier_rmse)` has its number. Built on `knn_cross` (the correspondence search, k = 1 within
`max_correspondence_distance`, over a target binned once) and csrc/icp.hip (transform, normal equations, solve). No CPU fallback: without
a HIP device the calls raise.

The definitions are this library's own (csrc/icp_point.h; tests/icp_oracle.py, bit-identical at every iteration):
  - both estimation methods take the same 6-parameter Gauss-Newton step x = (w, t) of the linearised residuals about a centre c (default:
    the midpoint of the target's bounding box, which keeps the 6x6 system conditioned in a world frame): point to plane with the
    residual (p - q) . n and the target's normals used as given (the result does not depend on their orientation), point to point with
    the three residuals p - q. THE CLOSED-FORM KABSCH / HORN STEP IS NOT PROVIDED: it needs a 3x3 SVD or a 4x4 eigen-solve, and with the
    correspondences fixed the Gauss-Newton step has the same fixed point;
  - the rotation of a step is the Cayley map of w, not the exponential map: they agree to second order, which suffices for a
    Gauss-Newton step and needs neither sin nor cos; the rotation block is not re-orthonormalised;
  - the sums run in an order fixed by the source index alone (chunks of `im_icp_chunk()` points), float64 without fused operations: a
    result is a function of the input alone, whatever the cell size or the order of the queries;
  - no robust loss kernels, no multi-scale or coloured variants, no scale estimation.
The loop has Open3D's shape: evaluate at `init`; then at most `max_iteration` times take the step, evaluate again and stop when
|fitness - previous| < relative_fitness and |inlier_rmse - previous| < relative_rmse (absolute differences, as in Open3D, despite the
names), or on a status other than OK. One small record is read back per iteration; nothing else synchronises.
PARITY WITH AN OPEN3D OR CLOUDCOMPARE BINARY IS UNPINNED."""
import math
from typing import NamedTuple

import numpy as np
import torch

from .._lib import ptr
from ..engine import default_engine, to_device
from ..utils import point_cloud_filters as F
from ..utils.transformations import check_transform
from .cloud_distance import _is_numpy, _points

METHODS = {"point_to_point": 0, "point_to_plane": 1}
STATUS = ("OK", "EMPTY", "DEGENERATE")
# the record of im_icp_finish, in doubles (include/icematch.h)
REC_M, REC_FITNESS, REC_RMSE, REC_COUNT, REC_STATUS, REC_X, REC_PIVOT, REC_SUMS, RECORD = 0, 16, 17, 18, 19, 20, 26, 32, 64


class ICPConvergenceCriteria(NamedTuple):
    relative_fitness: float = 1e-6
    relative_rmse: float = 1e-6
    max_iteration: int = 30


class RegistrationResult(NamedTuple):
    transformation: object      # [4, 4] float64: takes the source onto the target
    fitness: float              # usable correspondences / source points, at `transformation`
    inlier_rmse: float          # sqrt(mean squared distance of the usable correspondences); what m3c2's registration_error wants
    correspondence_set: object  # [c, 2] int64 (source index, target index): the pairs the search found at `transformation`
    iterations: int             # steps taken
    converged: bool
    status: str                 # of the last evaluation: OK, EMPTY (no correspondence), DEGENERATE (fewer than six, or a singular system)
    history: np.ndarray         # [iterations + 1, 64] float64: the record of every evaluation (layout in include/icematch.h)


def icp_chunk() -> int:
    """The source points per partial sum (part of the definition of every sum)."""
    from .._lib import load
    return int(load().im_icp_chunk())


def _shape3(a, what):
    shape = tuple(a.pts.shape) if isinstance(a, F.BinnedCloud) else tuple(a.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{what} must be [n, 3] (got {shape})")
    if shape[0] > F.MAX_BALL_POINTS:
        raise ValueError(f"at most 2^26 {what} points")
    return shape[0]


def check_registration(source, target, max_correspondence_distance, init, estimation_method, criteria, target_normals, normal_radius, centre):
    """The exceptions of bad arguments, before any device work: (source, target, d_max, init [4, 4], method code, criteria, centre or None)."""
    source, target = _points(source), _points(target)
    _shape3(source, "source")
    nt = _shape3(target, "target")
    d = float(max_correspondence_distance)
    if not (d > 0.0 and math.isfinite(d)):
        raise ValueError(f"max_correspondence_distance must be finite and positive (got {max_correspondence_distance})")
    init = check_transform(np.eye(4) if init is None else init, "init")
    if estimation_method not in METHODS:
        raise ValueError(f"estimation_method must be one of {sorted(METHODS)} (got {estimation_method!r})")
    criteria = ICPConvergenceCriteria(*criteria)
    if int(criteria.max_iteration) != criteria.max_iteration or criteria.max_iteration < 0:
        raise ValueError(f"max_iteration must be an integer >= 0 (got {criteria.max_iteration})")
    if estimation_method == "point_to_plane":
        if target_normals is None and normal_radius is None:
            raise ValueError("point_to_plane needs target_normals or a normal_radius to estimate them")
        shape = None if target_normals is None else tuple(target_normals.shape if hasattr(target_normals, "shape") else np.shape(target_normals))
        if shape is not None and shape != (nt, 3):
            raise ValueError(f"target_normals must be [{nt}, 3] (got {shape})")
        if target_normals is None:
            F._check_radius(normal_radius, "normal_radius")
    if centre is not None:
        centre = np.ascontiguousarray(centre, np.float64)
        if centre.shape != (3,) or not np.isfinite(centre).all():
            raise ValueError("centre must be three finite numbers")
    return source, target, d, init, METHODS[estimation_method], criteria, centre


def _prepare(eng, target, d_max, method, target_normals, normal_radius, centre):
    """(binned target, device normals or None, centre [3] host)"""
    tb = target if isinstance(target, F.BinnedCloud) else F.bin_cloud(target, d_max, engine=eng)
    nrm = None
    if method == METHODS["point_to_plane"]:
        if target_normals is not None:
            nrm = F._device_queries(target_normals, eng.device, "target_normals")
        elif len(tb):
            nrm = F.ball_cross(tb.pts, None, float(normal_radius), want=("normal",), engine=eng, binned=tb)["normal"]
        if nrm is None or nrm.shape[0] == 0:
            nrm = torch.zeros((1, 3), dtype=torch.float64, device=eng.device)       # an empty target: never read
    if centre is None:
        if len(tb):
            lo, hi = F._bounds(tb.pts)
            centre = (lo + hi) / np.float64(2.0)
        else:
            centre = np.zeros(3)
    return tb, nrm, np.ascontiguousarray(centre, np.float64)


def _loop(eng, src, tb, nrm, d_max, init, method, criteria, centre, sort_queries, solve):
    """The passes: (M [4, 4] of the last evaluation, history [passes, 64], idx of the last search, converged)."""
    dev, st = eng.device, eng.stream_ptr()
    n, nt = src.shape[0], len(tb)
    chunks = -(-n // icp_chunk())
    max_it = int(criteria.max_iteration) if solve else 0
    d_M = to_device(init.reshape(16), dev, np.float64)
    recs = torch.zeros((max_it + 1, RECORD), dtype=torch.float64, device=dev)
    p = torch.empty_like(src)
    tgt = tb.pts if nt else torch.zeros((1, 3), dtype=torch.float64, device=dev)
    M, history, converged, idx = init, [], False, None
    for it in range(max_it + 1):
        m_ptr = ptr(d_M) if it == 0 else recs[it - 1].data_ptr()
        if n:
            eng.ctx.call("im_transform_points", m_ptr, ptr(src), ptr(p), n, 0, st)
        found = F.knn_cross(p, None, 1, radius=d_max, want=("idx", "d2"), engine=eng, binned=tb, sort_queries=sort_queries)
        idx = found["idx"].reshape(-1)
        if n:
            eng.ctx.call("im_icp_accumulate", ptr(p), n, ptr(tgt), ptr(nrm), nt, ptr(idx), ptr(found["d2"]), centre.ctypes.data, method, chunks,
                         None, st)
        eng.ctx.call("im_icp_finish", None, n, chunks, m_ptr, centre.ctypes.data, 1 if it < max_it else 0, recs[it].data_ptr(), st)
        rec = recs[it].cpu().numpy()                                   # the one read-back of the iteration
        history.append(rec)
        if it > 0 and abs(rec[REC_FITNESS] - history[-2][REC_FITNESS]) < criteria.relative_fitness \
                and abs(rec[REC_RMSE] - history[-2][REC_RMSE]) < criteria.relative_rmse:
            converged = True
            break
        if int(rec[REC_STATUS]) != 0 or it == max_it:
            break
        M = rec[REC_M:REC_M + 16].reshape(4, 4).copy()
    return M, np.array(history), idx, converged


def _result(M, history, idx, converged, as_numpy, dev):
    last = history[-1]
    src_i = torch.nonzero(idx >= 0).reshape(-1)
    pairs = torch.stack([src_i, idx[src_i].long()], 1)
    return RegistrationResult(M if as_numpy else torch.as_tensor(M, device=dev), float(last[REC_FITNESS]), float(last[REC_RMSE]),
                              pairs.cpu().numpy() if as_numpy else pairs, len(history) - 1, converged, STATUS[int(last[REC_STATUS])], history)


def registration_icp(source, target, max_correspondence_distance, init=None, estimation_method="point_to_plane",
                     criteria=ICPConvergenceCriteria(), target_normals=None, normal_radius=None, centre=None, engine=None,
                     sort_queries=True) -> RegistrationResult:
    """The rigid transform that takes `source` onto `target` (arrays, tensors, `PointCloud`s; the target also a `bin_cloud` result, else
    binned once with cell size `max_correspondence_distance`), from `init` (default: the identity), by the module's definition.
    Point to plane takes the target's normals from `target_normals` [nt, 3] or estimates them once with `ball_cross` at
    `normal_radius`; with neither it raises ValueError. Source points with a non-finite coordinate, without a target point within the
    distance, or (point to plane) with a non-finite normal do not count. With a status other than OK the transform stays as it was.
    `sort_queries` is a tunable: no result depends on it. numpy in, numpy out; a tensor source gives tensors."""
    source, target, d, init, method, criteria, centre = check_registration(source, target, max_correspondence_distance, init, estimation_method,
                                                                            criteria, target_normals, normal_radius, centre)
    eng = default_engine(engine)
    src = F._device_queries(source, eng.device, "source")
    tb, nrm, centre = _prepare(eng, target, d, method, target_normals, normal_radius, centre)
    M, history, idx, converged = _loop(eng, src, tb, nrm, d, init, method, criteria, centre, sort_queries, True)
    return _result(M, history, idx, converged, _is_numpy(source), eng.device)


def evaluate_registration(source, target, max_correspondence_distance, transformation=None, engine=None, sort_queries=True) -> RegistrationResult:
    """Fitness, inlier rmse and correspondences of `source` under `transformation` (default: the identity) against `target`: one
    evaluation, no step (`iterations` 0, `converged` False)."""
    source, target, d, init, method, criteria, centre = check_registration(source, target, max_correspondence_distance, transformation,
                                                                            "point_to_point", ICPConvergenceCriteria(), None, None, None)
    eng = default_engine(engine)
    src = F._device_queries(source, eng.device, "source")
    tb, nrm, centre = _prepare(eng, target, d, method, None, None, centre)
    M, history, idx, converged = _loop(eng, src, tb, nrm, d, init, method, criteria, centre, sort_queries, False)
    return _result(M, history, idx, converged, _is_numpy(source), eng.device)
