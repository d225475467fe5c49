"""Two-view dense stereo: depth maps and the dense cloud of an epoch's stereo pair, on the device (csrc/dense.hip). In the reference this
step is Metashape's: `MetashapeProject.build_dense_cloud` calls `chunk.buildDepthMaps(downscale=..., filter_mode=...)` and
`chunk.buildDenseCloud(point_colors=True, point_confidence=True)` straight after the bundle adjustment (`metashape/metashape.py:198-240,
361-371`) and exports `dense_{date}.ply`, which every later stage reads. Metashape's matcher is closed and is NOT reproduced: the stage has
a definition of its own (csrc/dense_pixel.h, DESIGN §4, restated in tests/dense_oracle.py) - a plane sweep over fronto-parallel planes
of each view scored by the zero-mean normalised cross-correlation of exact integer window sums, a left-right consistency check whose
tolerance the reference's four `depth_filter` names select, and a cloud of the kept pixels with colours, camera-oriented normals and the
score as confidence. Parity with Metashape is unpinned by construction. No host fallback: `default_engine(engine)`.
`regularisation="sgm"` replaces the per-pixel choice of the sweep by a semi-global one (csrc/dense_sgm.hip, csrc/sgm_pixel.h, restated in
tests/sgm_oracle.py): the scores as an 8-bit cost volume, min-plus path costs summed over four or eight directions, the plane of least
sum. It is this project's own definition too, not Metashape's depth filter; the default None is the plain sweep.
`speckle=(min_size, max_diff)` and `holes=(max_hole, max_diff)` clean each view's map behind the sweep (csrc/depth_clean.hip,
csrc/depth_pixel.h, restated in tests/depth_oracle.py): connected components of the map labelled on the device, the small ones dropped,
the small holes filled by interpolation. Again a definition of this project's own: neither OpenCV's `filterSpeckles` nor Metashape's
filter; the default None makes no call.
`fuse=(tol, min_views)` on `build_dense_cloud` fuses the two views' maps into one cloud (csrc/dense_fuse.hip, csrc/fuse_pixel.h, restated
in tests/fuse_oracle.py): a kept pixel of the base view is linked to the kept pixel of the other view it falls on, a linked pixel gives one
point placed by both measurements, the other view adds only what the base does not represent, and every point carries the number of
views that agreed on it. Once more a definition of this project's own, not Metashape's merge of its depth maps: parity with Metashape
is unpinned by construction; the default None makes no call and concatenates the views' clouds as before.
`refine=(passes, fit_radius)` refines each view's map over slanted windows behind the clean-up (csrc/dense_refine.hip, csrc/refine_pixel.h,
restated in tests/refine_oracle.py): the sweep warps every sample of a window with the centre's inverse depth, which a surface seen
obliquely does not have; a pass fits the slant of every pixel to the map and searches a few sub-plane candidates whose window follows
it. A definition of this project's own as well, parity with Metashape unpinned by construction; the default None makes no call.

Cameras are objects with `.K .R .t` (X_cam = R X_world + t) and optionally `.dist`, as `core.Camera` and the cameras of a
`sfm.BundleResult`. Images are uint8 [h, w] or [h, w, 3] (RGB) numpy arrays or device tensors."""
import logging
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np
import torch

from ._lib import ptr
from .core.point_cloud import PointCloud
from .engine import default_engine, to_device
from .utils.homography import inv3

logger = logging.getLogger(__name__)

MAX_SIDE, MAX_PLANES, MAX_RADIUS = 16384, 4096, 7
MAX_SGM_PLANES, MAX_PENALTY, MAX_VOLUME = 256, 4095, 1 << 32
MAX_PLANE_DIFF, MAX_HOLE, MAX_MIN_SIZE = 4095, 4096, (1 << 31) - 1
MAX_FIT_RADIUS, MAX_SLANT_DIFF, MAX_SPAN, MAX_SUB, MAX_REFINE_PASSES = 7, 64.0, 4, 8, 16
REGULARISATIONS = (None, "sgm")
DEPTH_FILTERS = {"NoFiltering": None, "MildFiltering": 2.0, "ModerateFiltering": 1.0, "AggressiveFiltering": 0.5}


def filter_tolerance(depth_filter: str) -> Optional[float]:
    """tau of the consistency check, in plane steps of the other view, for one of the reference's four names; None skips the check.
    An unknown name raises the reference's ValueError (`metashape.py:217-220`)."""
    if depth_filter not in DEPTH_FILTERS:
        raise ValueError("Error: invalid choise of depth filtering. Choose one in [NoFiltering, MildFiltering, ModerateFiltering, AggressiveFiltering]")
    return DEPTH_FILTERS[depth_filter]


# ---- images: grey, downscaling ------------------------------------------------------------------------------------------------------------
def _tensor(image) -> torch.Tensor:
    t = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
    if t.dtype != torch.uint8 or not (t.ndim == 2 or (t.ndim == 3 and t.shape[2] == 3)):
        raise ValueError(f"dense: a uint8 [h, w] or [h, w, 3] image is expected (got {t.dtype}, shape {tuple(t.shape)})")
    return t


def to_grey(image):
    """(77 R + 150 G + 29 B + 128) >> 8 of an RGB image, in integers; a grey image is returned as it is. numpy in, numpy out; tensor in, tensor out."""
    t = _tensor(image)
    if t.ndim == 2:
        return image
    i = t.to(torch.int32)
    g = ((77 * i[..., 0] + 150 * i[..., 1] + 29 * i[..., 2] + 128) >> 8).to(torch.uint8)
    return g if torch.is_tensor(image) else g.numpy()


def downscale_image(image, f: int):
    """The exact integer mean (sum + f^2 // 2) // f^2 of f x f blocks, per channel; rows and columns beyond the last whole block are dropped."""
    f = _factor(f)
    t = _tensor(image)
    if f == 1:
        return image
    h, w = t.shape[0] // f, t.shape[1] // f
    if h < 1 or w < 1:
        raise ValueError(f"dense: the image is smaller than one {f} x {f} block")
    b = t[:h * f, :w * f].to(torch.int32).reshape((h, f, w, f) + tuple(t.shape[2:]))
    out = torch.div(b.sum((1, 3)) + (f * f) // 2, f * f, rounding_mode="floor").to(torch.uint8)
    return out if torch.is_tensor(image) else out.numpy()


def downscale_K(K, f: int) -> np.ndarray:
    """K of the downscaled image: the centre of pixel u of the small image lies at f u + (f - 1) / 2 of the large one."""
    f = _factor(f)
    K = np.array(K, np.float64).reshape(3, 3)
    if f == 1:
        return K
    S = np.array([[1.0 / f, 0.0, -(f - 1) / (2.0 * f)], [0.0, 1.0 / f, -(f - 1) / (2.0 * f)], [0.0, 0.0, 1.0]])
    return S @ K


def _factor(f) -> int:
    if int(f) != f or not 1 <= int(f) <= 64:
        raise ValueError(f"dense: downscale must be an integer in 1..64 (got {f})")
    return int(f)


# ---- geometry on the host: a few 3 x 3 products ---------------------------------------------------------------------------------------------
def _pose(cam):
    R, t = np.asarray(cam.R, np.float64).reshape(3, 3), np.asarray(cam.t, np.float64).reshape(3)
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        raise ValueError("dense: a camera pose is not finite")
    return R, t


def relative_pose(cam0, cam1):
    """(R, t) of X1 = R X0 + t."""
    R0, t0 = _pose(cam0)
    R1, t1 = _pose(cam1)
    R = R1 @ R0.T
    return R, t1 - R @ t0


def sweep_matrices(K0, K1, R, t):
    """A = K1 R inv(K0) and B = K1 t e3^T inv(K0), [9] float64 each: the homography of the plane of inverse depth w is A + w B."""
    Ki = inv3(np.asarray(K0, np.float64).reshape(3, 3))
    K1 = np.asarray(K1, np.float64).reshape(3, 3)
    A = K1 @ np.asarray(R, np.float64).reshape(3, 3) @ Ki
    B = np.outer(K1 @ np.asarray(t, np.float64).reshape(3), Ki[2])
    return np.ascontiguousarray(A.reshape(9)), np.ascontiguousarray(B.reshape(9))


def _corner_steps(A, B, shape, w_first, w_step, D) -> float:
    """The largest distance, in pixels of the other view, that two adjacent planes put between the images of a corner of `shape`."""
    h, w = shape
    corners = np.array([[0.0, 0.0, 1.0], [w - 1.0, 0.0, 1.0], [0.0, h - 1.0, 1.0], [w - 1.0, h - 1.0, 1.0]])
    ws = w_first + np.arange(D, dtype=np.float64) * w_step
    H = A.reshape(1, 3, 3) + ws[:, None, None] * B.reshape(1, 3, 3)
    p = np.einsum("dij,cj->dci", H, corners)
    with np.errstate(all="ignore"):
        xy = p[..., :2] / p[..., 2:3]
        step = np.linalg.norm(np.diff(xy, axis=0), axis=-1)
    step = step[np.isfinite(step)]
    return float(step.max()) if step.size else 0.0


def plane_schedule(cam0, cam1, d_min: float, d_max: float, max_step_px: float = 1.0, shape=None):
    """(w_first, w_step, D): D inverse depths from 1 / d_max to 1 / d_min of view `cam0`, evenly spaced, with D the smallest count found
    for which adjacent planes move no corner of cam0's image by more than `max_step_px` pixels in cam1's. `shape` = (h, w) of the image
    (default cam0's height and width)."""
    if not (0.0 < d_min <= d_max < np.inf) or not (max_step_px > 0.0):
        raise ValueError(f"plane_schedule: 0 < d_min <= d_max and max_step_px > 0 are expected (got {d_min}, {d_max}, {max_step_px})")
    shape = (int(cam0.height), int(cam0.width)) if shape is None else shape
    R, t = relative_pose(cam0, cam1)
    A, B = sweep_matrices(cam0.K, cam1.K, R, t)
    w_first, w_last = 1.0 / d_max, 1.0 / d_min
    if w_last == w_first:
        return w_first, 0.0, 1
    D = 2
    for _ in range(64):
        step = _corner_steps(A, B, shape, w_first, (w_last - w_first) / (D - 1), D)
        if step <= max_step_px:
            return w_first, (w_last - w_first) / (D - 1), D
        D = max(D + 1, int(np.ceil((D - 1) * step / max_step_px)) + 1)
        if D > MAX_PLANES:
            break
    raise ValueError(f"plane_schedule: the depth range {d_min}..{d_max} needs more than {MAX_PLANES} planes at {max_step_px} px per step; "
                     f"narrow the range, raise max_step_px or downscale")


def depth_range_from_points(points3d, cam, percentiles=(1, 99), margin: float = 0.25):
    """(d_min, d_max) for `cam` from a sparse cloud [n, 3] in world coordinates: the two percentiles of the depths of the points in front
    of the camera, widened to lo / (1 + margin) and hi (1 + margin)."""
    X = np.asarray(points3d, np.float64).reshape(-1, 3)
    lo_p, hi_p = percentiles
    if not (0.0 <= lo_p <= hi_p <= 100.0) or not (margin >= 0.0):
        raise ValueError(f"depth_range_from_points: 0 <= percentiles[0] <= percentiles[1] <= 100 and margin >= 0 are expected (got {percentiles}, {margin})")
    R, t = _pose(cam)
    z = (X @ R.T + t)[:, 2]
    z = z[np.isfinite(z) & (z > 0.0)]
    if z.size == 0:
        raise ValueError("depth_range_from_points: no point lies in front of the camera")
    lo, hi = np.percentile(z, [lo_p, hi_p])
    return float(lo / (1.0 + margin)), float(hi * (1.0 + margin))


# ---- the three launches ---------------------------------------------------------------------------------------------------------------------
class DepthMap(NamedTuple):
    """One view's map on the device: plane [h, w] int16 (-1: dropped), w [h, w] float64 inverse depths, score [h, w] float32; the
    (downscaled) image the colours come from, its grey form, K of that image, the pose and the schedule (w_first, w_step, D)."""
    plane: torch.Tensor
    w: torch.Tensor
    score: torch.Tensor
    image: torch.Tensor
    grey: torch.Tensor
    K: np.ndarray
    R: np.ndarray
    t: np.ndarray
    schedule: tuple


class _SmallCam(NamedTuple):
    """K of the downscaled image with the camera's pose."""
    K: np.ndarray
    R: np.ndarray
    t: np.ndarray


def _check_sweep(h0, w0, h1, w1, D, radius, min_var):
    for v in (h0, w0, h1, w1):
        if not 1 <= v <= MAX_SIDE:
            raise ValueError(f"dense: image sides must be 1..{MAX_SIDE} (got {v})")
    if int(D) != D or not 1 <= D <= MAX_PLANES:
        raise ValueError(f"dense: the number of planes must be 1..{MAX_PLANES} (got {D})")
    if int(radius) != radius or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"dense: the window radius must be 1..{MAX_RADIUS} (got {radius})")
    if int(min_var) != min_var or not 0 <= min_var <= 1 << 26:
        raise ValueError(f"dense: min_var must be an integer in 0..2^26 (got {min_var})")


def _check_regularisation(regularisation, p1, p2, paths):
    if regularisation not in REGULARISATIONS:
        raise ValueError(f"dense: regularisation is None or 'sgm' (got {regularisation!r})")
    if regularisation is None:
        return
    if int(p1) != p1 or int(p2) != p2 or not 0 <= p1 <= p2 <= MAX_PENALTY:
        raise ValueError(f"dense: the penalties must be integers with 0 <= p1 <= p2 <= {MAX_PENALTY} (got {p1}, {p2})")
    if paths not in (4, 8):
        raise ValueError(f"dense: paths must be 4 or 8 (got {paths})")


def _check_volume(h0, w0, D):
    if int(D) != D or not 1 <= D <= MAX_SGM_PLANES:
        raise ValueError(f"dense: semi-global aggregation holds at most {MAX_SGM_PLANES} planes (the schedule has {D}); raise downscale or max_step_px")
    for v in (h0, w0):
        if not 1 <= v <= MAX_SIDE:
            raise ValueError(f"dense: image sides must be 1..{MAX_SIDE} (got {v})")
    if h0 * w0 * int(D) > MAX_VOLUME:
        raise ValueError(f"dense: a cost volume of {h0} x {w0} x {D} entries exceeds 2^32; raise downscale or max_step_px")


def cost_volume(ref, src, A, B, w_first, w_step, D, radius=3, min_var=4, engine=None) -> torch.Tensor:
    """`im_dense_costs` on two grey device images: the sweep's scores as costs, uint8 [h0, w0, D] on the device (255: the plane did not score)."""
    h0, w0 = ref.shape
    h1, w1 = src.shape
    _check_sweep(h0, w0, h1, w1, D, radius, min_var)
    _check_volume(h0, w0, D)
    eng = default_engine(engine)
    dev = eng.device
    ref, src = ref.to(dev).contiguous(), src.to(dev).contiguous()
    A, B = np.ascontiguousarray(A, np.float64).reshape(9), np.ascontiguousarray(B, np.float64).reshape(9)
    cost = torch.empty((h0, w0, int(D)), dtype=torch.uint8, device=dev)
    eng.ctx.call("im_dense_costs", ptr(ref), h0, w0, ptr(src), h1, w1, A.ctypes.data, B.ctypes.data, float(w_first), float(w_step), int(D), int(radius),
                 int(min_var), ptr(cost), eng.stream_ptr())
    return cost


def _volume(cost, what):
    if not torch.is_tensor(cost) or cost.dtype != torch.uint8 or cost.ndim != 3:
        raise ValueError(f"{what}: a uint8 [h, w, D] cost volume is expected")
    _check_volume(*cost.shape)


def sgm_aggregate(cost, P1: int = 16, P2: int = 128, paths: int = 8, engine=None) -> torch.Tensor:
    """`im_dense_sgm`: the path costs of a cost volume summed over 4 or 8 directions, uint16 [h0, w0, D] on the device."""
    _volume(cost, "sgm_aggregate")
    _check_regularisation("sgm", P1, P2, paths)
    eng = default_engine(engine)
    cost = cost.to(eng.device).contiguous()
    h0, w0, D = cost.shape
    total = torch.empty((h0, w0, D), dtype=torch.uint16, device=eng.device)
    eng.ctx.call("im_dense_sgm", ptr(cost), h0, w0, D, int(P1), int(P2), int(paths), ptr(total), eng.stream_ptr())
    return total


def sgm_choose(cost, total, w_first, w_step, min_score=0.8, engine=None):
    """`im_dense_sgm_choose`: (plane, w, score) device tensors as `sweep` gives them, out of a cost volume and its summed path costs."""
    _volume(cost, "sgm_choose")
    if not torch.is_tensor(total) or total.dtype != torch.uint16 or total.shape != cost.shape:
        raise ValueError("sgm_choose: the sums are a uint16 tensor of the cost volume's shape")
    eng = default_engine(engine)
    dev = eng.device
    cost, total = cost.to(dev).contiguous(), total.to(dev).contiguous()
    h0, w0, D = cost.shape
    plane = torch.empty((h0, w0), dtype=torch.int16, device=dev)
    w = torch.empty((h0, w0), dtype=torch.float64, device=dev)
    score = torch.empty((h0, w0), dtype=torch.float32, device=dev)
    eng.ctx.call("im_dense_sgm_choose", ptr(cost), ptr(total), h0, w0, D, float(w_first), float(w_step), float(min_score), ptr(plane), ptr(w), ptr(score),
                 eng.stream_ptr())
    return plane, w, score


def sweep(ref, src, A, B, w_first, w_step, D, radius=3, min_var=4, min_score=0.8, engine=None, regularisation=None, p1=16, p2=128, paths=8):
    """`im_dense_sweep` on two grey device images: (plane, w, score) device tensors of ref's shape. `regularisation="sgm"` takes the cost
    volume, its semi-global aggregation with the penalties `p1 <= p2` over `paths` directions, and the choice instead; the volumes are
    freed once the maps are chosen."""
    h0, w0 = ref.shape
    h1, w1 = src.shape
    _check_sweep(h0, w0, h1, w1, D, radius, min_var)
    _check_regularisation(regularisation, p1, p2, paths)
    if regularisation == "sgm":
        _check_volume(h0, w0, D)
        eng = default_engine(engine)
        cost = cost_volume(ref, src, A, B, w_first, w_step, D, radius, min_var, engine=eng)
        total = sgm_aggregate(cost, p1, p2, paths, engine=eng)
        maps = sgm_choose(cost, total, w_first, w_step, min_score, engine=eng)
        del cost, total
        return maps
    eng = default_engine(engine)
    dev = eng.device
    ref, src = ref.to(dev).contiguous(), src.to(dev).contiguous()
    A, B = np.ascontiguousarray(A, np.float64).reshape(9), np.ascontiguousarray(B, np.float64).reshape(9)
    plane = torch.empty((h0, w0), dtype=torch.int16, device=dev)
    w = torch.empty((h0, w0), dtype=torch.float64, device=dev)
    score = torch.empty((h0, w0), dtype=torch.float32, device=dev)
    eng.ctx.call("im_dense_sweep", ptr(ref), h0, w0, ptr(src), h1, w1, A.ctypes.data, B.ctypes.data, float(w_first), float(w_step), int(D), int(radius),
                 int(min_var), float(min_score), ptr(plane), ptr(w), ptr(score), eng.stream_ptr())
    return plane, w, score


# ---- clean-up: components, speckles, holes -----------------------------------------------------------------------------------------------------
def _check_count(what, name, v, hi):
    if isinstance(v, bool) or int(v) != v or not 1 <= v <= hi:
        raise ValueError(f"{what}: {name} must be an integer in 1..{hi} (got {v})")


def _check_max_diff(what, max_diff):
    if isinstance(max_diff, bool) or int(max_diff) != max_diff or not 0 <= max_diff <= MAX_PLANE_DIFF:
        raise ValueError(f"{what}: max_diff must be an integer in 0..{MAX_PLANE_DIFF} (got {max_diff})")


def _check_clean_up(speckle, holes):
    """`speckle` = None | (min_size, max_diff) and `holes` = None | (max_hole, max_diff) of `build_depth_maps`, as pairs of ints."""
    out = []
    for name, value, first, hi in (("speckle", speckle, "min_size", MAX_MIN_SIZE), ("holes", holes, "max_hole", MAX_HOLE)):
        if value is None:
            out.append(None)
            continue
        try:
            a, b = value
        except (TypeError, ValueError):
            raise ValueError(f"dense: {name} is None or ({first}, max_diff) (got {value!r})") from None
        _check_count(f"dense: {name}", first, a, hi)
        _check_max_diff(f"dense: {name}", b)
        out.append((int(a), int(b)))
    return out


def _check_plane_map(plane, what):
    if not torch.is_tensor(plane) or plane.dtype != torch.int16 or plane.ndim != 2:
        raise ValueError(f"{what}: an int16 [h, w] plane map is expected")
    for v in plane.shape:
        if not 1 <= v <= MAX_SIDE:
            raise ValueError(f"{what}: image sides must be 1..{MAX_SIDE} (got {v})")


def _check_fill_schedule(schedule, what):
    w_first, w_step, D = schedule
    if not (np.isfinite(w_first) and np.isfinite(w_step)) or w_step == 0.0:
        raise ValueError(f"{what}: w_first must be finite and w_step finite and not zero (got {w_first}, {w_step}); a one-plane schedule has no step to round to")
    if int(D) != D or not 1 <= D <= MAX_PLANES:
        raise ValueError(f"{what}: the number of planes must be 1..{MAX_PLANES} (got {D})")


def depth_components(plane, max_diff: int = 1, holes: bool = False, engine=None):
    """`im_depth_components` on a plane map [h, w] int16: (label, size) int32 device tensors. Pixels are neighbours across an edge.
    `holes=False`: the members hold a plane (>= 0) and are joined when their planes differ by at most `max_diff`; `holes=True`: the members
    hold none and are all joined. label = the least linear index of the pixel's component (-1: no member), size = its pixel count (0)."""
    _check_plane_map(plane, "depth_components")
    _check_max_diff("depth_components", max_diff)
    eng = default_engine(engine)
    plane = plane.to(eng.device).contiguous()
    h, w = plane.shape
    label = torch.empty((h, w), dtype=torch.int32, device=eng.device)
    size = torch.empty((h, w), dtype=torch.int32, device=eng.device)
    eng.ctx.call("im_depth_components", ptr(plane), h, w, 1 if holes else 0, int(max_diff), ptr(label), ptr(size), eng.stream_ptr())
    return label, size


def remove_speckles(m: DepthMap, min_size: int = 16, max_diff: int = 1, engine=None, return_counts: bool = False):
    """The map without its speckles: pixels whose surface component (`depth_components`) has fewer than `min_size` pixels get plane -1,
    w 0, score 0, as the sweep writes a dropped pixel. The three tensors are cloned; `m` is not modified. `return_counts`: also the
    number of dropped pixels, an int64 [1] device tensor; nothing is read back."""
    _check_plane_map(m.plane, "remove_speckles")
    _check_count("remove_speckles", "min_size", min_size, MAX_MIN_SIZE)
    _check_max_diff("remove_speckles", max_diff)
    eng = default_engine(engine)
    dev = eng.device
    plane, w, score = m.plane.to(dev).clone().contiguous(), m.w.to(dev).clone().contiguous(), m.score.to(dev).clone().contiguous()
    h, wd = plane.shape
    _, size = depth_components(plane, max_diff, engine=eng)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    eng.ctx.call("im_depth_drop_small", ptr(size), h, wd, int(min_size), ptr(plane), ptr(w), ptr(score), ptr(count), eng.stream_ptr())
    out = m._replace(plane=plane, w=w, score=score)
    return (out, count) if return_counts else out


def fill_holes(m: DepthMap, max_hole: int = 64, max_diff: int = 2, engine=None, return_counts: bool = False):
    """The map with its small holes filled: a hole (a component of pixels without a plane) of at most `max_hole` pixels that does not
    touch the image border and whose rim spreads over at most `max_diff` planes takes, per pixel, the mean of the linear interpolations
    between its nearest plane-holding pixels along its row and along its column; the plane is the nearest of the schedule, the score 0.
    New tensors; `m` is not modified. `return_counts`: also the number of filled pixels, an int64 [1] device tensor."""
    _check_plane_map(m.plane, "fill_holes")
    _check_count("fill_holes", "max_hole", max_hole, MAX_HOLE)
    _check_max_diff("fill_holes", max_diff)
    _check_fill_schedule(m.schedule, "fill_holes")
    eng = default_engine(engine)
    dev = eng.device
    plane, w, score = m.plane.to(dev).contiguous(), m.w.to(dev).contiguous(), m.score.to(dev).contiguous()
    h, wd = plane.shape
    label, size = depth_components(plane, 0, holes=True, engine=eng)
    plane_out, w_out, score_out = torch.empty_like(plane), torch.empty_like(w), torch.empty_like(score)
    filled = torch.empty((h, wd), dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    w_first, w_step, D = m.schedule
    eng.ctx.call("im_depth_fill_holes", ptr(plane), ptr(w), ptr(score), ptr(label), ptr(size), h, wd, int(max_hole), int(max_diff), float(w_first),
                 float(w_step), int(D), ptr(plane_out), ptr(w_out), ptr(score_out), ptr(filled), ptr(count), eng.stream_ptr())
    out = m._replace(plane=plane_out, w=w_out, score=score_out)
    return (out, count) if return_counts else out


# ---- slanted-window refinement ----------------------------------------------------------------------------------------------------------------
REFINE_OPTIONS = ("passes", "fit_radius", "max_diff", "min_count", "span", "sub")


def _check_int(what, name, v, lo, hi):
    try:
        ok = not isinstance(v, (bool, str)) and int(v) == v and lo <= v <= hi
    except (TypeError, ValueError, OverflowError):                                # None, a NaN, an infinity
        ok = False
    if not ok:
        raise ValueError(f"{what}: {name} must be an integer in {lo}..{hi} (got {v!r})")


def _check_slant(what, fit_radius, max_diff, min_count):
    _check_int(what, "fit_radius", fit_radius, 1, MAX_FIT_RADIUS)
    if isinstance(max_diff, (bool, str)) or not isinstance(max_diff, (int, float, np.integer, np.floating)) or not 0.0 < max_diff <= MAX_SLANT_DIFF:
        raise ValueError(f"{what}: max_diff must be a number of plane steps in (0, {MAX_SLANT_DIFF:g}] (got {max_diff!r})")
    _check_int(what, "min_count", min_count, 3, 225)


def _check_refine_options(what, passes, fit_radius, max_diff, min_count, span, sub):
    _check_int(what, "passes", passes, 1, MAX_REFINE_PASSES)
    _check_slant(what, fit_radius, max_diff, min_count)
    _check_int(what, "span", span, 1, MAX_SPAN)
    _check_int(what, "sub", sub, 1, MAX_SUB)


def _check_refine(refine):
    """`refine` = None | (passes, fit_radius) | a dict of `refine_slanted`'s options but `radius` and `min_var`, which are the call's own:
    None, or the checked options as a dict."""
    if refine is None:
        return None
    if isinstance(refine, dict):
        unknown = sorted(set(refine) - set(REFINE_OPTIONS))
        if unknown:
            raise ValueError(f"dense: refine: unknown options {unknown}; a dict of {list(REFINE_OPTIONS)} is expected (radius and min_var are the call's own)")
        options = dict(refine)
    else:
        try:
            passes, fit_radius = refine
        except (TypeError, ValueError):
            raise ValueError(f"dense: refine is None, (passes, fit_radius) or a dict of {list(REFINE_OPTIONS)} (got {refine!r})") from None
        options = dict(passes=passes, fit_radius=fit_radius)
    full = dict(passes=2, fit_radius=4, max_diff=2.0, min_count=6, span=1, sub=4)
    full.update(options)
    _check_refine_options("dense: refine", **full)
    return full


def _check_map(m, what):
    _check_plane_map(m.plane, what)
    if not torch.is_tensor(m.w) or m.w.dtype != torch.float64 or m.w.shape != m.plane.shape:
        raise ValueError(f"{what}: w is a float64 tensor of the plane map's shape")
    if not torch.is_tensor(m.score) or m.score.dtype != torch.float32 or m.score.shape != m.plane.shape:
        raise ValueError(f"{what}: score is a float32 tensor of the plane map's shape")
    w_step = m.schedule[1]
    if not np.isfinite(w_step) or w_step == 0.0:
        raise ValueError(f"{what}: the schedule's w_step must be finite and not zero (got {w_step}); a one-plane schedule has no step to search along")


def slant_map(m: DepthMap, fit_radius: int = 4, max_diff: float = 2.0, min_count: int = 6, engine=None):
    """`im_dense_slant` (csrc/dense_refine.hip, csrc/refine_pixel.h, restated in tests/refine_oracle.py): (slant [h, w, 2] float64, fitted [h, w]
    uint8) on the device. The slant of a kept pixel, in plane steps per pixel along (u, v), is the least-squares plane through the inverse
    depths of the kept pixels of its (2 fit_radius + 1)^2 neighbourhood that lie within `max_diff` plane steps of its own, out of exact
    integer sums; fitted where at least `min_count` of them count and they do not lie on one line, zero elsewhere."""
    _check_map(m, "slant_map")
    _check_slant("slant_map", fit_radius, max_diff, min_count)
    eng = default_engine(engine)
    dev = eng.device
    plane, w = m.plane.to(dev).contiguous(), m.w.to(dev).contiguous()
    h, wd = plane.shape
    slant = torch.empty((h, wd, 2), dtype=torch.float64, device=dev)
    fitted = torch.empty((h, wd), dtype=torch.uint8, device=dev)
    eng.ctx.call("im_dense_slant", ptr(plane), ptr(w), h, wd, float(m.schedule[1]), int(fit_radius), float(max_diff), int(min_count), ptr(slant), ptr(fitted),
                 eng.stream_ptr())
    return slant, fitted


def refine_slanted(m: DepthMap, other: DepthMap, passes: int = 2, fit_radius: int = 4, max_diff: float = 2.0, min_count: int = 6, span: int = 1,
                   sub: int = 4, radius: int = 3, min_var: int = 4, engine=None, return_taken: bool = False):
    """The map `m` with its inverse depths refined over slanted windows against the view of `other` (of which only the grey image, K and the
    pose are read): `passes` times `slant_map`, then `im_dense_refine`. Every kept pixel whose window of `radius` lies inside the image
    searches the candidates -span .. span plane steps around its inverse depth, `sub` per step, each scored like the sweep but over a
    window whose samples follow the pixel's slant; the best one (with the sweep's parabola between its neighbours) is taken where it
    scores strictly more than the pixel does now, so no score falls. `plane` is left as it was: it stays the label that the clean-up
    segments, `w` carries the measurement. New tensors; `m` is not modified. `return_taken`: also the last pass's mask [h, w] uint8.
    A definition of this project's own, not Metashape's matcher; parity with Metashape is unpinned by construction."""
    _check_map(m, "refine_slanted")
    _check_refine_options("refine_slanted", passes, fit_radius, max_diff, min_count, span, sub)
    for g, name in ((m.grey, "the map's"), (other.grey, "the other view's")):
        if not torch.is_tensor(g) or g.dtype != torch.uint8 or g.ndim != 2:
            raise ValueError(f"refine_slanted: {name} grey image is a uint8 [h, w] tensor")
    if m.grey.shape != m.plane.shape:
        raise ValueError("refine_slanted: the map's grey image has the map's shape")
    (h0, w0), (h1, w1) = m.grey.shape, other.grey.shape
    _check_sweep(h0, w0, h1, w1, 1, radius, min_var)
    R = other.R @ m.R.T
    A, B = sweep_matrices(m.K, other.K, R, other.t - R @ m.t)
    eng = default_engine(engine)
    dev = eng.device
    ref, src = m.grey.to(dev).contiguous(), other.grey.to(dev).contiguous()
    plane, w, score = m.plane.to(dev).contiguous(), m.w.to(dev).contiguous(), m.score.to(dev).contiguous()
    out, taken = m._replace(plane=plane, w=w, score=score), None
    for _ in range(int(passes)):
        slant, _ = slant_map(out, fit_radius, max_diff, min_count, engine=eng)
        w_out, score_out = torch.empty_like(w), torch.empty_like(score)
        taken = torch.empty((h0, w0), dtype=torch.uint8, device=dev)
        eng.ctx.call("im_dense_refine", ptr(ref), h0, w0, ptr(src), h1, w1, A.ctypes.data, B.ctypes.data, ptr(plane), ptr(out.w), ptr(out.score), ptr(slant),
                     float(m.schedule[1]), int(radius), int(min_var), int(span), int(sub), ptr(w_out), ptr(score_out), ptr(taken), eng.stream_ptr())
        out = out._replace(w=w_out, score=score_out)
    return (out, taken) if return_taken else out


def consistency(map0: DepthMap, map1: DepthMap, depth_filter: str = "ModerateFiltering", engine=None) -> torch.Tensor:
    """`im_dense_consistency`: keep [h, w] uint8 on the device for the pixels of `map0` against `map1`."""
    tau = filter_tolerance(depth_filter)
    eng = default_engine(engine)
    h0, w0 = map0.plane.shape
    h1, w1 = map1.plane.shape
    keep = torch.empty((h0, w0), dtype=torch.uint8, device=eng.device)
    if tau is None:
        eng.ctx.call("im_dense_consistency", ptr(map0.plane), ptr(map0.w), h0, w0, None, None, h1, w1, None, 0.0, 0, ptr(keep), eng.stream_ptr())
        return keep
    R = map1.R @ map0.R.T
    t = map1.t - R @ map0.t
    pose = np.ascontiguousarray(np.concatenate([inv3(map0.K).reshape(9), R.reshape(9), t, map1.K.reshape(9)]))
    eng.ctx.call("im_dense_consistency", ptr(map0.plane), ptr(map0.w), h0, w0, ptr(map1.plane), ptr(map1.w), h1, w1, pose.ctypes.data,
                 float(tau * abs(map1.schedule[1])), 1, ptr(keep), eng.stream_ptr())
    return keep


def _check_fuse(fuse):
    """`fuse` = None | (tol, min_views) of `build_dense_cloud`, as (float, int)."""
    if fuse is None:
        return None
    try:
        tol, min_views = fuse
    except (TypeError, ValueError):
        raise ValueError(f"dense: fuse is None or (tol, min_views) (got {fuse!r})") from None
    _check_fuse_tol("dense: fuse", tol)
    if isinstance(min_views, bool) or min_views not in (1, 2):
        raise ValueError(f"dense: fuse: min_views must be 1 or 2 (got {min_views!r})")
    return float(tol), int(min_views)


def _check_fuse_tol(what, tol):
    if isinstance(tol, (bool, str)) or not isinstance(tol, (int, float, np.integer, np.floating)) or not tol >= 0.0:
        raise ValueError(f"{what}: tol must be a number of plane steps >= 0 (got {tol!r})")


def _pose_between(a: DepthMap, b: DepthMap) -> np.ndarray:
    """h_pose [30] = inv(Ka), R, t, Kb with Xb = R Xa + t, as `consistency` builds it."""
    R = b.R @ a.R.T
    t = b.t - R @ a.t
    return np.ascontiguousarray(np.concatenate([inv3(a.K).reshape(9), R.reshape(9), t, b.K.reshape(9)]))


def fuse(map_a: DepthMap, keep_a: torch.Tensor, map_b: DepthMap, keep_b: torch.Tensor, tol: float = 1.0, engine=None):
    """`im_dense_fuse_link` and `im_dense_fuse_rest` (csrc/dense_fuse.hip, csrc/fuse_pixel.h, restated in tests/fuse_oracle.py): the two maps of a
    pair as one. A kept pixel of the base view `map_a` links to the kept pixel of `map_b` its point falls on when that pixel's inverse depth
    agrees within `tol` plane steps of map_b's schedule; a linked pixel takes the mean of both measurements along its own ray, weighted by
    the scores, and the greater score. Returns (the fused DepthMap of view a, views [ha, wa] uint8 = 2 linked / 1 kept only / 0 not kept,
    link [ha, wa] int32 = the linear index of the target or -1, rest [hb, wb] uint8 = 1 on the kept pixels of view b that no pixel
    claimed and that do not link into view a themselves: what view a does not represent), all on the device. The plane of a fused pixel
    is left as it was. A definition of this project's own, not Metashape's merge; parity with Metashape is unpinned by construction."""
    _check_fuse_tol("fuse", tol)
    (ha, wa), (hb, wb) = map_a.plane.shape, map_b.plane.shape
    for v in (ha, wa, hb, wb):
        if not 1 <= v <= MAX_SIDE:
            raise ValueError(f"fuse: image sides must be 1..{MAX_SIDE} (got {v})")
    for keep, shape in ((keep_a, (ha, wa)), (keep_b, (hb, wb))):
        if not torch.is_tensor(keep) or keep.dtype != torch.uint8 or tuple(keep.shape) != shape:
            raise ValueError("fuse: a keep mask is a uint8 tensor of its map's shape")
    eng = default_engine(engine)
    dev = eng.device
    w_a, s_a, k_a = map_a.w.to(dev).contiguous(), map_a.score.to(dev).contiguous(), keep_a.to(dev).contiguous()
    w_b, s_b, k_b = map_b.w.to(dev).contiguous(), map_b.score.to(dev).contiguous(), keep_b.to(dev).contiguous()
    link = torch.empty((ha, wa), dtype=torch.int32, device=dev)
    w_out, score_out = torch.empty_like(w_a), torch.empty_like(s_a)
    views = torch.empty((ha, wa), dtype=torch.uint8, device=dev)
    claimed = torch.empty((hb, wb), dtype=torch.uint8, device=dev)
    rest = torch.empty((hb, wb), dtype=torch.uint8, device=dev)
    ab, ba = _pose_between(map_a, map_b), _pose_between(map_b, map_a)
    eng.ctx.call("im_dense_fuse_link", ptr(k_a), ptr(w_a), ptr(s_a), ha, wa, ptr(k_b), ptr(w_b), ptr(s_b), hb, wb, ab.ctypes.data,
                 float(tol * abs(map_b.schedule[1])), ptr(link), ptr(w_out), ptr(score_out), ptr(views), ptr(claimed), eng.stream_ptr())
    eng.ctx.call("im_dense_fuse_rest", ptr(k_b), ptr(w_b), hb, wb, ptr(k_a), ptr(w_a), ha, wa, ba.ctypes.data, float(tol * abs(map_a.schedule[1])),
                 ptr(claimed), ptr(rest), eng.stream_ptr())
    return map_a._replace(w=w_out, score=score_out), views, link, rest


_fuse_maps = fuse            # `build_dense_cloud` has a parameter of the same name


def cloud_of(m: DepthMap, keep: torch.Tensor, engine=None):
    """`im_dense_cloud`: (points [n, 3] float64, rgb [n, 3] uint8, normals [n, 3] float64, confidence [n] float32) device tensors of the kept
    pixels of one map in row-major order. One count is read back."""
    eng = default_engine(engine)
    dev = eng.device
    h, w = m.plane.shape
    cap = h * w
    xyz = torch.empty((cap, 3), dtype=torch.float64, device=dev)
    rgb = torch.empty((cap, 3), dtype=torch.uint8, device=dev)
    nrm = torch.empty((cap, 3), dtype=torch.float64, device=dev)
    conf = torch.empty(cap, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    cam = np.ascontiguousarray(np.concatenate([inv3(m.K).reshape(9), m.R.reshape(9), m.t]))
    img = m.image.contiguous()
    eng.ctx.call("im_dense_cloud", ptr(keep), ptr(m.w), ptr(m.score), ptr(img), 3 if img.ndim == 3 else 1, h, w, cam.ctypes.data, cap, ptr(xyz),
                 ptr(rgb), ptr(nrm), ptr(conf), ptr(count), eng.stream_ptr())
    n = int(count.item())
    return xyz[:n], rgb[:n], nrm[:n], conf[:n]


# ---- the stage --------------------------------------------------------------------------------------------------------------------------------
def _prepare(image, cam, downscale, eng):
    """The (undistorted, downscaled) image of one view on the device and its grey form."""
    t = _tensor(image)
    dist = getattr(cam, "dist", None)
    if dist is not None and np.any(np.asarray(dist, np.float64) != 0.0):
        from .sfm import undistort_image
        t = _tensor(undistort_image(t.to(eng.device), cam, engine=eng))
    t = downscale_image(t.to(eng.device), downscale).contiguous()
    return t, to_grey(t).contiguous()


def build_depth_maps(images, cameras, depth_range=None, sparse_points=None, downscale: int = 1, radius: int = 3, min_score: float = 0.8,
                     min_var: int = 4, max_step_px: float = 1.0, engine=None, regularisation=None, p1: int = 16, p2: int = 128, paths: int = 8,
                     speckle=None, holes=None, refine=None):
    """The depth maps of both views of a stereo pair, `chunk.buildDepthMaps` of the reference with a definition of this project's own
    (module docstring): [DepthMap of view 0, DepthMap of view 1], on the device. `depth_range` = (d_min, d_max) in view 0 (and, through the
    same points, view 1) or None: then `sparse_points` [n, 3] give it per view (`depth_range_from_points`). Images with a non-zero
    `dist` are undistorted first (`sfm.undistort_image`). `regularisation` = None: each pixel takes its best plane by itself;
    "sgm": semi-global aggregation of the costs with the penalties `p1 <= p2` over `paths` (4 or 8) directions decides (`sweep`), which
    holds at most 256 planes per view. `speckle` = (min_size, max_diff) drops the small components of each view's map (`remove_speckles`),
    `holes` = (max_hole, max_diff) then fills its small holes (`fill_holes`): after the sweep, under either regularisation. None: neither.
    `refine` = (passes, fit_radius) or a dict of `refine_slanted`'s options (passes, fit_radius, max_diff, min_count, span, sub) then refines
    each view's map over slanted windows (`refine_slanted`), with this call's `radius` and `min_var`; a filled pixel has score 0, so any
    valid candidate is taken there and the pixel gains a measured confidence. None: no call, and the maps are what they were."""
    if len(images) != 2 or len(cameras) != 2:
        raise ValueError("build_depth_maps: a stereo pair has two images and two cameras")
    downscale = _factor(downscale)
    _check_regularisation(regularisation, p1, p2, paths)
    speckle, holes = _check_clean_up(speckle, holes)
    refine = _check_refine(refine)
    if depth_range is None and sparse_points is None:
        raise ValueError("build_depth_maps: a depth_range or sparse_points to take it from are needed")
    # everything that can be refused is refused before the first launch
    shapes = [tuple(_tensor(im).shape[:2]) for im in images]
    small_shapes = [(s[0] // downscale, s[1] // downscale) for s in shapes]
    _check_sweep(*small_shapes[0], *small_shapes[1], 1, radius, min_var)
    ranges = [tuple(depth_range) if depth_range is not None else depth_range_from_points(sparse_points, c) for c in cameras]
    small = [_SmallCam(downscale_K(c.K, downscale), *_pose(c)) for c in cameras]
    plans = []
    for v in range(2):
        schedule = plane_schedule(small[v], small[1 - v], ranges[v][0], ranges[v][1], max_step_px, shape=small_shapes[v])
        if regularisation == "sgm":
            _check_volume(*small_shapes[v], schedule[2])
        if holes is not None:
            _check_fill_schedule(schedule, "dense: holes")
        if refine is not None:
            _check_fill_schedule(schedule, "dense: refine")
        plans.append((schedule, sweep_matrices(small[v].K, small[1 - v].K, *relative_pose(small[v], small[1 - v]))))
    chosen = {} if regularisation is None else dict(regularisation=regularisation, p1=p1, p2=p2, paths=paths)
    eng = default_engine(engine)
    prepared = [_prepare(im, c, downscale, eng) for im, c in zip(images, cameras)]
    maps = []
    for v in range(2):
        (w_first, w_step, D), (A, B) = plans[v]
        plane, w, score = sweep(prepared[v][1], prepared[1 - v][1], A, B, w_first, w_step, D, radius, min_var, min_score, engine=eng, **chosen)
        m = DepthMap(plane, w, score, prepared[v][0], prepared[v][1], small[v].K, small[v].R, small[v].t, (w_first, w_step, D))
        if speckle is not None:
            m = remove_speckles(m, *speckle, engine=eng)
        if holes is not None:
            m = fill_holes(m, *holes, engine=eng)
        maps.append(m)
    if refine is not None:                        # of the other view only the image and the camera are read: the order does not matter
        maps = [refine_slanted(maps[v], maps[1 - v], radius=radius, min_var=min_var, engine=eng, **refine) for v in range(2)]
    return maps


def build_dense_cloud(images, cameras, sparse_points=None, depth_filter: str = "ModerateFiltering", downscale: int = 1, views=(0,), save_path=None,
                      depth_range=None, radius: int = 3, min_score: float = 0.8, min_var: int = 4, max_step_px: float = 1.0, engine=None,
                      regularisation=None, p1: int = 16, p2: int = 128, paths: int = 8, speckle=None, holes=None, fuse=None,
                      ply_scalars=(), refine=None) -> PointCloud:
    """`MetashapeProject.build_dense_cloud` of the reference with a definition of this project's own: the depth maps of the pair, their
    consistency under `depth_filter`, and the cloud of the kept pixels of `views` (view 0's points first) as a `core.PointCloud` with
    colours, normals turned towards the camera and `confidence` (the score, float32). `save_path` writes it as PLY (`dense_{date}.ply`),
    with the per-point scalars named in `ply_scalars` ("confidence", "views") behind the other properties.
    `regularisation`, `p1`, `p2`, `paths`, `speckle`, `holes`, `refine`: as `build_depth_maps` takes them; the clean-up and the refinement
    come before the consistency check, and a filled pixel enters the cloud with confidence 0 unless the refinement measured it.
    `fuse` = None: the clouds of `views` one behind the other, a surface that both views see twice. `fuse` = (tol, min_views) fuses the two
    maps instead (the module-level `fuse`; `views` must name both views, the first is the base): `depth_filter` still decides both keep
    masks first, then the base view gives one point per kept pixel with at least `min_views` (1 or 2) views, from the fused map, and with
    min_views = 1 the pixels of the other view that the base does not represent follow. The cloud's `views` (uint8, 2 or 1) says how many
    depth maps agreed on a point, as Metashape's point confidence counts them; the rule is this project's own, not Metashape's."""
    filter_tolerance(depth_filter)
    _check_regularisation(regularisation, p1, p2, paths)
    _check_clean_up(speckle, holes)
    _check_refine(refine)
    fuse = _check_fuse(fuse)
    ply_scalars = PointCloud.check_scalars(ply_scalars)
    views = tuple(views)
    if not views or any(v not in (0, 1) for v in views):
        raise ValueError(f"build_dense_cloud: views are 0 and / or 1 (got {views})")
    if fuse is not None and views not in ((0, 1), (1, 0)):
        raise ValueError(f"build_dense_cloud: fuse needs both views, the base first: views=(0, 1) or (1, 0) (got {views})")
    if fuse is None and "views" in ply_scalars:
        raise ValueError("build_dense_cloud: ply_scalars names 'views', which only a fused cloud has (fuse=(tol, min_views))")
    chosen = {} if regularisation is None else dict(regularisation=regularisation, p1=p1, p2=p2, paths=paths)
    if speckle is not None:
        chosen["speckle"] = speckle
    if holes is not None:
        chosen["holes"] = holes
    if refine is not None:
        chosen["refine"] = refine
    maps = build_depth_maps(images, cameras, depth_range, sparse_points, downscale, radius, min_score, min_var, max_step_px, engine=engine, **chosen)
    eng = default_engine(engine)
    parts, seen = [], None
    if fuse is None:
        for v in views:
            keep = consistency(maps[v], maps[1 - v], depth_filter, engine=eng)
            parts.append(cloud_of(maps[v], keep, engine=eng))
    else:
        (tol, min_views), (a, b) = fuse, views
        keep_a = consistency(maps[a], maps[b], depth_filter, engine=eng)
        keep_b = consistency(maps[b], maps[a], depth_filter, engine=eng)
        fused, count, _, rest = _fuse_maps(maps[a], keep_a, maps[b], keep_b, tol, engine=eng)
        mask = (count >= min_views).to(torch.uint8)
        parts.append(cloud_of(fused, mask, engine=eng))
        seen = [count[mask != 0]]                             # row-major, the order of the scan
        if min_views == 1:
            parts.append(cloud_of(maps[b], rest, engine=eng))
            seen.append(torch.ones(len(parts[1][0]), dtype=torch.uint8, device=eng.device))
    xyz, rgb, nrm, conf = (torch.cat([p[i] for p in parts]).cpu().numpy() for i in range(4))
    pcd = PointCloud(points3d=xyz, points_col=rgb.astype(np.float64) / 255.0)
    pcd.normals = nrm
    pcd.confidence = conf
    if seen is not None:
        pcd.views = torch.cat(seen).cpu().numpy()
    if save_path is not None:
        if ply_scalars:
            pcd.write_ply(Path(save_path), scalars=ply_scalars)
        else:
            pcd.write_ply(Path(save_path))
    return pcd


def dense_series(images, cameras, sparse_points=None, out_dir=None, dates=None, fuse=None, refine=None, **options) -> list:
    """`build_dense_cloud` for every epoch of a sequence: `images` a list of E pairs, `cameras` one pair, a list of E pairs or a list of E
    `sfm.BundleResult` (as `bundle_adjust_epochs` returns them: their cameras and, unless `sparse_points` is given, their points are
    taken), `sparse_points` None, one array or a list of E. With `out_dir`, epoch e is written to `dense_{dates[e]}.ply` (default e).
    `fuse` = (tol, min_views) fuses every epoch's two maps into one cloud (`build_dense_cloud`; `views=(0, 1)` or `(1, 0)` must come with
    it); `refine` = (passes, fit_radius) or a dict refines every epoch's maps over slanted windows (`refine_slanted`); `options` are
    `build_dense_cloud`'s other ones, `ply_scalars` among them, handed down as they are."""
    if fuse is not None:
        options["fuse"] = fuse
    if refine is not None:
        options["refine"] = refine
    E = len(images)
    results = list(cameras) if len(cameras) == E and all(hasattr(c, "cameras") and hasattr(c, "points3d") for c in cameras) else None
    if results is not None:
        pairs = [r.cameras for r in results]
        if sparse_points is None:
            sparse_points = [r.points3d for r in results]
    else:
        pairs = [cameras] if len(cameras) == 2 and not isinstance(cameras[0], (list, tuple)) else list(cameras)
    if len(pairs) not in (1, E):
        raise ValueError(f"dense_series: one camera pair or one per epoch ({E}) is expected (got {len(pairs)})")
    if isinstance(sparse_points, list) and len(sparse_points) != E:
        raise ValueError(f"dense_series: a list of sparse_points holds one entry per epoch ({E})")
    out = []
    for e in range(E):
        path = None if out_dir is None else Path(out_dir) / f"dense_{dates[e] if dates is not None else e}.ply"
        sp = sparse_points[e] if isinstance(sparse_points, list) else sparse_points
        out.append(build_dense_cloud(images[e], pairs[e if len(pairs) > 1 else 0], sparse_points=sp, save_path=path, **options))
    return out
