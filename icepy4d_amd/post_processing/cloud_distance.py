"""How far the surface moved between two epoch clouds, point by point, on the device: the cloud-to-cloud distance (CloudCompare's C2C,
Open3D's `compute_point_cloud_distance`) and M3C2 (Lague et al. 2013: the distance along the local normal with a level of detection;
CloudCompare's plugin of that name). Built on `utils/point_cloud_filters.py`: `knn_cross`, `ball_cross`, `cylinder_stats`
(csrc/cloud_distance.hip). No CPU fallback: without a HIP device the calls raise.

The definitions are this library's own (tests/cloud_distance_oracle.py, bit-identical):
  - C2C: the distance to the nearest point of the reference cloud, sqrt of the float64 d2 = ((dx*dx) + (dy*dy)) + (dz*dz), the lower index
    among equally near points. No local surface model.
  - M3C2: per core point a normal (the ball of diameter `normal_scale` in cloud 1 around it, the eigenvector of the smallest eigenvalue,
    oriented along `orientation` or towards `viewpoint`), then in each cloud the points inside the cylinder of diameter `search_scale` that
    reaches `search_depth` to either side along the normal; their projections on the normal are quantised to search_depth * 2^-18 and
    summed exactly; distance = mean2 - mean1, lod = 1.96 * (sqrt(std1^2 / n1 + std2^2 / n2) + registration_error) with the sample standard
    deviations, NaN where a cylinder holds fewer than `min_points` points; significant = |distance| > lod.
PARITY WITH A CLOUDCOMPARE OR OPEN3D BINARY IS UNPINNED: CloudCompare stores float32 coordinates after a global shift, offers sub-sampled
core points, a multi-scale normal search and median / IQR statistics, which are not provided, and may place a point that sits on a
cylinder's wall at the scale of rounding on the other side; the 2^-18 search_depth quantisation of projections (19 um at 5 m) is ours."""
import math
from typing import NamedTuple

import numpy as np
import torch

from .._lib import ptr
from ..engine import default_engine
from ..utils import point_cloud_filters as F


class CloudDistance(NamedTuple):
    distance: object      # [m] float64, +inf where the reference holds no point
    index: object         # [m] int32 into the reference, -1 where there is none
    split: object         # [m, 3] float64 = fl(reference[index] - compared), NaN where there is none


class M3C2Result(NamedTuple):
    core_points: object   # [m, 3] float64
    normals: object       # [m, 3] float64, oriented; NaN for a degenerate ball
    distance: object      # [m] float64, NaN where a cylinder is empty or the normal is NaN
    lod: object           # [m] float64, NaN where a cylinder holds fewer than min_points points
    significant: object   # [m] bool
    count1: object        # [m] int32
    count2: object        # [m] int32
    std1: object          # [m] float64, NaN below two points
    std2: object          # [m] float64


def _points(cloud):
    """A `BinnedCloud`, a tensor, or [n, 3] float64 numpy of a `core.PointCloud` or an array."""
    from ..core.point_cloud import PointCloud
    if isinstance(cloud, (F.BinnedCloud, torch.Tensor)):
        return cloud
    if isinstance(cloud, PointCloud):
        return np.ascontiguousarray(cloud.get_points(), np.float64).reshape(-1, 3)
    return np.ascontiguousarray(np.asarray(cloud, np.float64))


def _is_numpy(cloud):
    return not isinstance(cloud, (torch.Tensor, F.BinnedCloud))


def cloud_to_cloud_distance(compared, reference, engine=None) -> CloudDistance:
    """For every point of `compared` its nearest point of `reference` (arrays, tensors, `PointCloud`s, or a `bin_cloud` result as the
    reference): `CloudDistance(distance, index, split)`. numpy in, numpy out; a tensor `compared` gives tensors."""
    eng = default_engine(engine)
    compared, reference = _points(compared), _points(reference)
    ref = reference.pts if isinstance(reference, F.BinnedCloud) else F._device_points(reference, eng.device)
    q = F._device_queries(compared, eng.device)
    r = F.knn_cross(q, ref, 1, want=("idx", "d2"), engine=eng, binned=reference if isinstance(reference, F.BinnedCloud) else None)
    idx, d2 = r["idx"][:, 0].contiguous(), r["d2"][:, 0].contiguous()
    has = idx >= 0
    near = ref[idx.clamp(min=0).long()] if ref.shape[0] else torch.zeros_like(q)
    split = torch.where(has[:, None], near - q, torch.full_like(q, math.nan))
    out = CloudDistance(torch.sqrt(d2), idx, split)
    return CloudDistance(*[v.cpu().numpy() for v in out]) if _is_numpy(compared) else out


def unit_normals(normals):
    """Rows scaled to unit length by explicit float64 operations: len = sqrt(((x*x) + (y*y)) + (z*z)), each component divided by it (a
    zero row becomes NaN). numpy or tensor, the same kind out."""
    n = normals
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    sqrt = np.sqrt if isinstance(n, np.ndarray) else torch.sqrt
    with np.errstate(invalid="ignore", divide="ignore"):
        return n / sqrt(((x * x) + (y * y)) + (z * z))[:, None]


def orient_normals(normals, core_points, orientation=(0.0, 0.0, 1.0), viewpoint=None):
    """Flips a normal iff ((nx*ox) + (ny*oy)) + (nz*oz) < 0, o the fixed `orientation` or `viewpoint - core` when a viewpoint is given.
    Flipping is a change of sign, exact; a NaN normal stays. numpy or tensor, the same kind out."""
    lib = np if isinstance(normals, np.ndarray) else torch
    if viewpoint is not None:
        v = np.asarray(viewpoint, np.float64).reshape(3)
        o = (v if lib is np else torch.as_tensor(v, device=normals.device)) - core_points
        ox, oy, oz = o[:, 0], o[:, 1], o[:, 2]
    else:
        ox, oy, oz = (float(c) for c in np.asarray(orientation, np.float64).reshape(3))
    dot = ((normals[:, 0] * ox) + (normals[:, 1] * oy)) + (normals[:, 2] * oz)
    return lib.where((dot < 0)[:, None], -normals, normals)


def check_m3c2(normal_scale, search_scale, search_depth, registration_error, min_points):
    """The exceptions of bad arguments, before any device work; (normal_scale, search_scale, search_depth, registration_error, min_points)."""
    scales = []
    for name, v in (("normal_scale", normal_scale), ("search_scale", search_scale), ("search_depth", search_depth)):
        v = float(v)
        if not (v > 0.0 and math.isfinite(v)) or v * 2.0 ** -19 < 2.2250738585072014e-308:
            raise ValueError(f"{name} must be finite and positive (got {v})")
        scales.append(v)
    reg = float(registration_error)
    if not (reg >= 0.0 and math.isfinite(reg)):
        raise ValueError(f"registration_error must be finite and >= 0 (got {registration_error})")
    if int(min_points) != min_points or int(min_points) < 2:
        raise ValueError(f"min_points must be an integer >= 2 (got {min_points})")
    return scales[0], scales[1], scales[2], reg, int(min_points)


def m3c2(cloud1, cloud2, core_points=None, *, normal_scale, search_scale, search_depth, registration_error=0.0, min_points=5,
         orientation=(0.0, 0.0, 1.0), viewpoint=None, normals=None, engine=None, as_numpy=None) -> M3C2Result:
    """M3C2 between `cloud1` and `cloud2` (arrays, tensors, `PointCloud`s or `bin_cloud` results) at `core_points` (default: cloud1's own
    points), by the module's definition. The scales are diameters, as in CloudCompare's dialog: the normals come from the ball of radius
    normal_scale / 2 in cloud1 unless `normals` [m, 3] are supplied (scaled to unit length here), the cylinders have radius search_scale / 2
    and reach `search_depth` to either side. A degenerate ball (NaN normal) gives NaN distance and significant False. numpy in, numpy
    out; tensor core points (or cloud1, without core points) give tensors; `as_numpy` overrides."""
    normal_scale, search_scale, search_depth, reg, min_points = check_m3c2(normal_scale, search_scale, search_depth, registration_error, min_points)
    eng = default_engine(engine)
    dev = eng.device
    cloud1, cloud2 = _points(cloud1), _points(cloud2)
    b1 = cloud1 if isinstance(cloud1, F.BinnedCloud) else F.bin_cloud(cloud1, search_scale / 2.0, engine=eng)
    b2 = cloud2 if isinstance(cloud2, F.BinnedCloud) else F.bin_cloud(cloud2, search_scale / 2.0, engine=eng)
    if as_numpy is None:
        as_numpy = _is_numpy(cloud1) if core_points is None else not isinstance(core_points, torch.Tensor)
    core = b1.pts if core_points is None else F._device_queries(_points(core_points), dev, "core_points")
    m = core.shape[0]
    if normals is None:
        nrm = F.ball_cross(core, None, normal_scale / 2.0, want=("normal",), engine=eng, binned=b1)["normal"]
    else:
        nrm = unit_normals(F._device_queries(normals, dev, "normals"))
        if nrm.shape[0] != m:
            raise ValueError(f"{m} core points but {nrm.shape[0]} normals")
    nrm = orient_normals(nrm, core, orientation, viewpoint).contiguous()
    want = ("count", "sums", "std")
    s1 = F.cylinder_stats(core, nrm, None, search_scale / 2.0, search_depth, want=want, engine=eng, binned=b1)
    s2 = F.cylinder_stats(core, nrm, None, search_scale / 2.0, search_depth, want=want, engine=eng, binned=b2)
    dist = torch.empty(m, dtype=torch.float64, device=dev)
    lod = torch.empty(m, dtype=torch.float64, device=dev)
    sig = torch.empty(m, dtype=torch.uint8, device=dev)
    eng.ctx.call("im_m3c2_finish", ptr(s1["count"]), ptr(s1["sums"]), ptr(s2["count"]), ptr(s2["sums"]), m, search_depth, reg, min_points,
                 ptr(dist), ptr(lod), ptr(sig), eng.stream_ptr())
    out = M3C2Result(core, nrm, dist, lod, sig.bool(), s1["count"], s2["count"], s1["std"], s2["std"])
    return M3C2Result(*[v.cpu().numpy() for v in out]) if as_numpy else out
