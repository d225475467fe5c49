"""Dense surface displacement between epochs from depth maps, on the device (csrc/dense_flow.hip). After `dense.build_depth_maps` every
epoch holds, per camera, a `DepthMap`: the grey image, the inverse depths and the epoch's own adjusted K, R, t. This module joins two
epochs of one camera: every kept pixel of the map at epoch A gets the pixel of the same camera's image at epoch B that shows the same
piece of the surface (`match_flow`, optionally checked forwards and backwards by `flow_consistency`), both ends are lifted to world points
through each epoch's own map and pose (`lift_flow`), and the result is a point, a displacement vector and a velocity per pixel
(`surface_displacement`, `displacement_series`) in the table format that `utils.binned_stats` reads. Because each end is lifted with its
own epoch's camera, a camera that moved between the epochs does not leak into the displacement.

The reference has no such step: its velocities come from tracked keypoints alone (`scripts/tracking_experimental.py`). The stage has a
definition of this project's own (csrc/flow_pixel.h, DESIGN §4, restated in tests/flow_oracle.py): an integer-pixel search by the zero-mean
normalised cross-correlation of exact integer window sums with a parabola between the best candidate's neighbours; no rotation or scale
of the template. Parity with any image-correlation package is unpinned by construction.

One level (`match_flow`, and `levels=1` of the stage) searches `search` pixels around a single global prior. With `levels` > 1
(`match_flow_pyramid`, csrc/dense_flow_field.hip, restated in tests/pyrflow_oracle.py) the search is coarse to fine: `match_flow` runs on
the coarsest level of a Gaussian pyramid (`im_pyr_down`), every finer level takes a prior per pixel from the level above
(`prior_field_up`: twice the lower median of the valid displacements around the pixel's parent) and searches `fine_search` pixels around
it (`match_flow_field`). The reach is 2^(levels - 1) search + (2^(levels - 1) - 1) fine_search pixels around the global prior, rock at
0 px and ice at tens of pixels are found in one frame, and a fine pixel scores (2 fine_search + 1)^2 candidates.
No host fallback: `default_engine(engine)`."""
import datetime
from typing import NamedTuple

import numpy as np
import torch

from ._lib import ptr
from .dense import MAX_SIDE, DepthMap
from .engine import default_engine
from .utils.homography import inv3
from .utils.tracking_features_utils import F64_COLS

MAX_RADIUS, MAX_SEARCH, MAX_PRIOR, MAX_MIN_VAR = 15, 16, 4096, 1 << 26
MAX_LEVELS, MAX_MEDIAN_RADIUS = 6, 2
TABLE_COLS = F64_COLS + ("dt", "ep_ini", "ep_fin")


class FlowField(NamedTuple):
    """A dense match on the device: du, dv [h, w] float64 (pixels, the prior included), score [h, w] float32, valid [h, w] uint8; zeros
    where invalid or not asked for."""
    du: torch.Tensor
    dv: torch.Tensor
    score: torch.Tensor
    valid: torch.Tensor


class PriorField(NamedTuple):
    """A prior per pixel on the device: pu, pv [h, w] int16 (pixels), have [h, w] uint8; a pixel without a prior is not matched."""
    pu: torch.Tensor
    pv: torch.Tensor
    have: torch.Tensor


class DisplacementField(NamedTuple):
    """The lifted pixels of one epoch pair in row-major order, on the device: points [n, 3] float64 (the world point at epoch A),
    displacement [n, 3] float64 (world point at epoch B minus that), velocity = displacement / dt_days, score [n] float32 (the forward
    match's), pixels [n, 2] int64 (u, v of the pixel at epoch A)."""
    points: torch.Tensor
    displacement: torch.Tensor
    velocity: torch.Tensor
    score: torch.Tensor
    pixels: torch.Tensor


# ---- checks: everything is refused before any device work -------------------------------------------------------------------------------------
def _check_int(what, name, v, lo, hi):
    try:
        ok = not isinstance(v, (bool, str)) and int(v) == v and lo <= v <= hi
    except (TypeError, ValueError, OverflowError):                                # None, a NaN, an infinity
        ok = False
    if not ok:
        raise ValueError(f"{what}: {name} must be an integer in {lo}..{hi} (got {v!r})")


def _check_positive(what, name, v, unit):
    if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not v > 0.0:
        raise ValueError(f"{what}: {name} must be a finite number of {unit} > 0 (got {v!r})")


def _check_grey(what, name, g):
    if not torch.is_tensor(g) or g.dtype != torch.uint8 or g.ndim != 2:
        raise ValueError(f"{what}: {name} is a uint8 [h, w] tensor")
    for v in g.shape:
        if not 1 <= v <= MAX_SIDE:
            raise ValueError(f"{what}: image sides must be 1..{MAX_SIDE} (got {v})")


def _check_mask(what, name, m, shape):
    if not torch.is_tensor(m) or m.dtype != torch.uint8 or tuple(m.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} is a uint8 tensor of shape {tuple(shape)}")


def _check_match(what, radius, search, prior, min_var, min_score):
    _check_int(what, "radius", radius, 1, MAX_RADIUS)
    _check_int(what, "search", search, 0, MAX_SEARCH)
    try:
        pu, pv = prior
    except (TypeError, ValueError):
        raise ValueError(f"{what}: prior is a pair of integers (du, dv) (got {prior!r})") from None
    _check_int(what, "prior[0]", pu, -MAX_PRIOR, MAX_PRIOR)
    _check_int(what, "prior[1]", pv, -MAX_PRIOR, MAX_PRIOR)
    _check_int(what, "min_var", min_var, 0, MAX_MIN_VAR)
    if isinstance(min_score, (bool, str)) or not isinstance(min_score, (int, float, np.integer, np.floating)) or not np.isfinite(min_score):
        raise ValueError(f"{what}: min_score must be a finite number (got {min_score!r})")


def _check_pyramid(what, shape, levels, radius, fine_search, median_radius, min_count):
    _check_int(what, "levels", levels, 1, MAX_LEVELS)
    _check_int(what, "fine_search", fine_search, 0, MAX_SEARCH)
    _check_int(what, "median_radius", median_radius, 0, MAX_MEDIAN_RADIUS)
    _check_int(what, "min_count", min_count, 1, (2 * int(median_radius) + 1) ** 2)
    if shape is not None and levels > 1:                                          # one level takes any image, as ever: nothing matches in a small one
        h, w = level_shapes(shape, levels)[-1]
        if min(h, w) < 2 * radius + 1:
            raise ValueError(f"{what}: levels = {levels} leaves a coarsest level of {h} x {w}, smaller than the window of 2 radius + 1 = {2 * radius + 1}; "
                             f"take fewer levels or a smaller radius")


def _check_prior_field(what, name, f, shape):
    if not isinstance(f, PriorField):
        raise ValueError(f"{what}: {name} is a PriorField")
    for t, dtype, part in ((f.pu, torch.int16, "pu"), (f.pv, torch.int16, "pv"), (f.have, torch.uint8, "have")):
        if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {name}.{part} is a {str(dtype).replace('torch.', '')} tensor of the images' shape {tuple(shape)}")


def _check_field(what, name, f, shape=None):
    if not isinstance(f, FlowField):
        raise ValueError(f"{what}: {name} is a FlowField")
    shape = tuple(f.du.shape) if shape is None and torch.is_tensor(f.du) else shape
    for t, dtype, part in ((f.du, torch.float64, "du"), (f.dv, torch.float64, "dv"), (f.score, torch.float32, "score"), (f.valid, torch.uint8, "valid")):
        if not torch.is_tensor(t) or t.dtype != dtype or t.ndim != 2 or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {name}.{part} is a {str(dtype).replace('torch.', '')} [h, w] tensor of the field's shape")
    for v in shape:
        if not 1 <= v <= MAX_SIDE:
            raise ValueError(f"{what}: image sides must be 1..{MAX_SIDE} (got {v})")


def _check_depth_map(what, name, m):
    if not isinstance(m, DepthMap):
        raise ValueError(f"{what}: {name} is a dense.DepthMap")
    if not torch.is_tensor(m.plane) or m.plane.dtype != torch.int16 or m.plane.ndim != 2:
        raise ValueError(f"{what}: {name}.plane is an int16 [h, w] tensor")
    for v in m.plane.shape:
        if not 1 <= v <= MAX_SIDE:
            raise ValueError(f"{what}: image sides must be 1..{MAX_SIDE} (got {v})")
    if not torch.is_tensor(m.w) or m.w.dtype != torch.float64 or m.w.shape != m.plane.shape:
        raise ValueError(f"{what}: {name}.w is a float64 tensor of the plane map's shape")
    for a, n, part in ((m.K, 9, "K"), (m.R, 9, "R"), (m.t, 3, "t")):
        try:
            a = np.asarray(a, np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: {name}.{part} holds {n} finite numbers") from None
        if a.size != n or not np.isfinite(a).all():
            raise ValueError(f"{what}: {name}.{part} holds {n} finite numbers")
    try:
        w_first, w_step, D = m.schedule
        ok = all(not isinstance(v, (bool, str)) and isinstance(v, (int, float, np.integer, np.floating)) for v in (w_first, w_step, D))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: {name}.schedule is (w_first, w_step, D), three numbers (got {m.schedule!r})")


def _cam(m: DepthMap) -> np.ndarray:
    """h_cam [21] = inv(K), R, t, as `dense.cloud_of` builds it."""
    return np.ascontiguousarray(np.concatenate([inv3(np.asarray(m.K, np.float64).reshape(3, 3)).reshape(9), np.asarray(m.R, np.float64).reshape(9),
                                                np.asarray(m.t, np.float64).reshape(3)]))


# ---- the three launches ---------------------------------------------------------------------------------------------------------------------------
def match_flow(grey_a, grey_b, ask=None, radius: int = 7, search: int = 8, prior=(0, 0), min_var: int = 4, min_score: float = 0.8, engine=None) -> FlowField:
    """`im_flow_match` on two grey device images of one shape: for every pixel of `grey_a` (where `ask` [h, w] uint8 is not 0; None: every
    pixel) the displacement to the pixel of `grey_b` whose (2 radius + 1)^2 window correlates best with its own, over the integer
    candidates prior + (dx, dy), |dx|, |dy| <= search, with a parabola between the best candidate's neighbours along each axis. Exact ties
    go to the smallest displacement from the prior. A pixel is invalid where its window leaves the image, where no candidate has
    `min_var` of variance in both windows or where the best score is below `min_score`."""
    what = "match_flow"
    _check_grey(what, "grey_a", grey_a)
    _check_grey(what, "grey_b", grey_b)
    if grey_a.shape != grey_b.shape:
        raise ValueError(f"{what}: the two images have one shape (got {tuple(grey_a.shape)} and {tuple(grey_b.shape)})")
    if ask is not None:
        _check_mask(what, "ask", ask, grey_a.shape)
    _check_match(what, radius, search, prior, min_var, min_score)
    eng = default_engine(engine)
    dev = eng.device
    a, b = grey_a.to(dev).contiguous(), grey_b.to(dev).contiguous()
    ask = None if ask is None else ask.to(dev).contiguous()
    h, w = a.shape
    du = torch.empty((h, w), dtype=torch.float64, device=dev)
    dv = torch.empty((h, w), dtype=torch.float64, device=dev)
    score = torch.empty((h, w), dtype=torch.float32, device=dev)
    valid = torch.empty((h, w), dtype=torch.uint8, device=dev)
    eng.ctx.call("im_flow_match", ptr(a), ptr(b), h, w, int(radius), int(search), int(prior[0]), int(prior[1]), int(min_var), float(min_score), ptr(ask),
                 ptr(du), ptr(dv), ptr(score), ptr(valid), eng.stream_ptr())
    return FlowField(du, dv, score, valid)


# ---- coarse to fine ---------------------------------------------------------------------------------------------------------------------------------
def level_shapes(shape, levels):
    """The shapes of the `levels` levels of the pyramid of an image of `shape`: a level is ((h + 1) // 2, (w + 1) // 2) of the one below."""
    out = [(int(shape[0]), int(shape[1]))]
    for _ in range(int(levels) - 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def coarse_prior(p: int, levels: int) -> int:
    """rint(p / 2^(levels - 1)), ties to even, in integers."""
    d = 1 << (levels - 1)
    q, rest = divmod(int(p), d)
    return q + (1 if 2 * rest > d or (2 * rest == d and q % 2 == 1) else 0)


def prior_field_up(field: FlowField, shape, median_radius: int = 1, min_count: int = 1, engine=None) -> PriorField:
    """`im_flow_prior_up`: the prior of every pixel of a level of `shape` from the `FlowField` of the level above, whose shape is
    ((h + 1) // 2, (w + 1) // 2). A fine pixel (u, v) looks at the (2 median_radius + 1)^2 coarse pixels around (u >> 1, v >> 1) that are
    valid with finite displacements; with `min_count` or more of them its prior is twice the lower median of their du and of their dv,
    rounded, else it has none. The median keeps one wrong coarse match from steering four fine pixels and gives a prior to pixels whose
    own parent failed."""
    what = "prior_field_up"
    _check_field(what, "field", field)
    try:
        h, w = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: shape is (h, w) (got {shape!r})") from None
    for v in (h, w):
        if not 1 <= v <= MAX_SIDE:
            raise ValueError(f"{what}: image sides must be 1..{MAX_SIDE} (got {v})")
    hc, wc = field.du.shape
    if (hc, wc) != ((h + 1) // 2, (w + 1) // 2):
        raise ValueError(f"{what}: the field of the level above a {h} x {w} level is {(h + 1) // 2} x {(w + 1) // 2} (got {hc} x {wc})")
    _check_int(what, "median_radius", median_radius, 0, MAX_MEDIAN_RADIUS)
    _check_int(what, "min_count", min_count, 1, (2 * int(median_radius) + 1) ** 2)
    eng = default_engine(engine)
    dev = eng.device
    f = [t.to(dev).contiguous() for t in (field.du, field.dv, field.valid)]
    pu = torch.empty((h, w), dtype=torch.int16, device=dev)
    pv = torch.empty((h, w), dtype=torch.int16, device=dev)
    have = torch.empty((h, w), dtype=torch.uint8, device=dev)
    eng.ctx.call("im_flow_prior_up", *(ptr(t) for t in f), hc, wc, h, w, int(median_radius), int(min_count), ptr(pu), ptr(pv), ptr(have), eng.stream_ptr())
    return PriorField(pu, pv, have)


def match_flow_field(grey_a, grey_b, prior_field: PriorField, ask=None, radius: int = 7, search: int = 2, min_var: int = 4, min_score: float = 0.8,
                     engine=None, tile_path=None) -> FlowField:
    """`im_flow_match_field`: `match_flow` with a prior per pixel. A pixel is matched where `prior_field.have` is not 0, `ask` (None:
    every pixel) is not 0 and both components of its prior lie in -4096..4096; its candidates are its own prior + (dx, dy),
    |dx|, |dy| <= search. Everything else is `match_flow`'s; with a constant field the two give the same bits. `tile_path`: None, or a
    uint8 device tensor [ceil(h / 16), ceil(w / 64)] that receives the path each tile took (0 nothing to do, 1 tiled, 2 direct)."""
    what = "match_flow_field"
    _check_grey(what, "grey_a", grey_a)
    _check_grey(what, "grey_b", grey_b)
    if grey_a.shape != grey_b.shape:
        raise ValueError(f"{what}: the two images have one shape (got {tuple(grey_a.shape)} and {tuple(grey_b.shape)})")
    _check_prior_field(what, "prior_field", prior_field, grey_a.shape)
    if ask is not None:
        _check_mask(what, "ask", ask, grey_a.shape)
    _check_match(what, radius, search, (0, 0), min_var, min_score)
    h, w = grey_a.shape
    if tile_path is not None:
        _check_mask(what, "tile_path", tile_path, ((h + 15) // 16, (w + 63) // 64))
    eng = default_engine(engine)
    dev = eng.device
    if tile_path is not None and (tile_path.device != dev or not tile_path.is_contiguous()):
        raise ValueError(f"{what}: tile_path is a contiguous tensor on the engine's device")
    a, b = grey_a.to(dev).contiguous(), grey_b.to(dev).contiguous()
    pf = [t.to(dev).contiguous() for t in prior_field]
    ask = None if ask is None else ask.to(dev).contiguous()
    du = torch.empty((h, w), dtype=torch.float64, device=dev)
    dv = torch.empty((h, w), dtype=torch.float64, device=dev)
    score = torch.empty((h, w), dtype=torch.float32, device=dev)
    valid = torch.empty((h, w), dtype=torch.uint8, device=dev)
    eng.ctx.call("im_flow_match_field", ptr(a), ptr(b), h, w, int(radius), int(search), ptr(pf[0]), ptr(pf[1]), ptr(pf[2]), int(min_var), float(min_score),
                 ptr(ask), ptr(du), ptr(dv), ptr(score), ptr(valid), ptr(tile_path), eng.stream_ptr())
    return FlowField(du, dv, score, valid)


def _pyr_down(eng, img):
    h, w = img.shape
    out = torch.empty(((h + 1) // 2, (w + 1) // 2), dtype=torch.uint8, device=eng.device)
    eng.ctx.call("im_pyr_down", ptr(img), ptr(out), 1, h, w, 1, eng.stream_ptr())
    return out


def match_flow_pyramid(grey_a, grey_b, ask=None, levels: int = 3, radius: int = 7, search: int = 8, fine_search: int = 2, prior=(0, 0), min_var: int = 4,
                       min_score: float = 0.8, median_radius: int = 1, min_count: int = 1, engine=None, tile_paths=None) -> FlowField:
    """The coarse-to-fine match of `grey_a` in `grey_b`, on the device from end to end. Level l + 1 is `im_pyr_down` of level l. The
    coarsest level runs `match_flow` on every pixel with `search` and the prior rint(prior / 2^(levels - 1)) (ties to even); every
    finer level takes `prior_field_up` of the level above with `median_radius` and `min_count` and runs `match_flow_field` with
    `fine_search`; `ask` applies at level 0 only, so priors exist beside the mask. `radius`, `min_var` and `min_score` hold at every
    level. Returns level 0's field. The reach is 2^(levels - 1) search + (2^(levels - 1) - 1) fine_search pixels around `prior`.
    `levels=1` is `match_flow`. `tile_paths`: None, or a list that receives one uint8 tensor of tile paths per finer level, level 0 last."""
    what = "match_flow_pyramid"
    _check_grey(what, "grey_a", grey_a)
    _check_grey(what, "grey_b", grey_b)
    if grey_a.shape != grey_b.shape:
        raise ValueError(f"{what}: the two images have one shape (got {tuple(grey_a.shape)} and {tuple(grey_b.shape)})")
    if ask is not None:
        _check_mask(what, "ask", ask, grey_a.shape)
    _check_match(what, radius, search, prior, min_var, min_score)
    _check_pyramid(what, grey_a.shape, levels, radius, fine_search, median_radius, min_count)
    eng = default_engine(engine)
    match = dict(radius=radius, min_var=min_var, min_score=min_score, engine=eng)
    if levels == 1:
        return match_flow(grey_a, grey_b, ask=ask, search=search, prior=prior, **match)
    dev = eng.device
    pyr = [(grey_a.to(dev).contiguous(), grey_b.to(dev).contiguous())]
    for _ in range(levels - 1):
        pyr.append((_pyr_down(eng, pyr[-1][0]), _pyr_down(eng, pyr[-1][1])))
    field = match_flow(*pyr[-1], search=search, prior=(coarse_prior(prior[0], levels), coarse_prior(prior[1], levels)), **match)
    for level in range(levels - 2, -1, -1):
        a, b = pyr[level]
        pf = prior_field_up(field, a.shape, median_radius, min_count, engine=eng)
        path = None
        if tile_paths is not None:
            path = torch.empty(((a.shape[0] + 15) // 16, (a.shape[1] + 63) // 64), dtype=torch.uint8, device=dev)
            tile_paths.append(path)
        field = match_flow_field(a, b, pf, ask=ask if level == 0 else None, search=fine_search, tile_path=path, **match)
    return field


def flow_consistency(fwd: FlowField, bwd: FlowField, tol: float = 1.0, engine=None) -> torch.Tensor:
    """`im_flow_check`: keep [h, w] uint8 on the device. A valid pixel of the forward field (A to B) is kept when the backward field (B to A)
    is valid at the pixel it lands on (by rint) and brings it back to within `tol` pixels of where it started."""
    what = "flow_consistency"
    _check_field(what, "fwd", fwd)
    _check_field(what, "bwd", bwd, tuple(fwd.du.shape))
    _check_positive(what, "tol", tol, "pixels")
    eng = default_engine(engine)
    dev = eng.device
    f = [t.to(dev).contiguous() for t in (fwd.du, fwd.dv, fwd.valid, bwd.du, bwd.dv, bwd.valid)]
    h, w = f[0].shape
    keep = torch.empty((h, w), dtype=torch.uint8, device=dev)
    eng.ctx.call("im_flow_check", *(ptr(t) for t in f), h, w, float(tol), ptr(keep), eng.stream_ptr())
    return keep


def lift_flow(field: FlowField, keep, map_a: DepthMap, map_b: DepthMap, keep_b, max_diff: float = 2.0, engine=None):
    """`im_flow_lift`: (P [h, w, 3] float64, D [h, w, 3] float64, ok [h, w] uint8) on the device. A pixel with `keep` set, a plane in `map_a`
    and a valid match is lifted: P is its world point through map A and A's camera; the B end at (u + du, v + dv) takes the bilinear mean of
    the inverse depths of map B's four pixels around it - all four inside the map, holding a plane, set in `keep_b` and within `max_diff`
    plane steps of map B of one another - and Q is its world point through B's camera; D = Q - P. Zeros where not lifted. Inverse depth is
    interpolated and not depth: it is linear in the image for a plane."""
    what = "lift_flow"
    _check_depth_map(what, "map_a", map_a)
    _check_depth_map(what, "map_b", map_b)
    _check_field(what, "field", field, tuple(map_a.plane.shape))
    _check_mask(what, "keep", keep, map_a.plane.shape)
    _check_mask(what, "keep_b", keep_b, map_b.plane.shape)
    _check_positive(what, "max_diff", max_diff, "plane steps")
    w_step = map_b.schedule[1]
    if not np.isfinite(w_step) or w_step == 0.0:
        raise ValueError(f"{what}: map_b's schedule has a w_step that is finite and not zero (got {w_step}); a one-plane schedule has no step to measure by")
    cam_a, cam_b = _cam(map_a), _cam(map_b)
    eng = default_engine(engine)
    dev = eng.device
    f = [t.to(dev).contiguous() for t in (field.du, field.dv, field.valid, keep, map_a.plane, map_a.w)]
    g = [t.to(dev).contiguous() for t in (map_b.plane, map_b.w, keep_b)]
    (h, w), (hb, wb) = map_a.plane.shape, map_b.plane.shape
    P = torch.empty((h, w, 3), dtype=torch.float64, device=dev)
    D = torch.empty((h, w, 3), dtype=torch.float64, device=dev)
    ok = torch.empty((h, w), dtype=torch.uint8, device=dev)
    eng.ctx.call("im_flow_lift", *(ptr(t) for t in f), h, w, cam_a.ctypes.data, *(ptr(t) for t in g), hb, wb, cam_b.ctypes.data, float(w_step),
                 float(max_diff), ptr(P), ptr(D), ptr(ok), eng.stream_ptr())
    return P, D, ok


# ---- the stage ------------------------------------------------------------------------------------------------------------------------------------
OPTIONS = ("radius", "search", "prior", "min_var", "min_score", "tol", "max_diff", "levels", "fine_search", "median_radius", "min_count")


def _options(what, options, shape=None):
    unknown = sorted(set(options) - set(OPTIONS))
    if unknown:
        raise ValueError(f"{what}: unknown options {unknown}; {list(OPTIONS)} are known")
    full = dict(radius=7, search=8, prior=(0, 0), min_var=4, min_score=0.8, tol=1.0, max_diff=2.0, levels=1, fine_search=2, median_radius=1, min_count=1)
    full.update(options)
    _check_match(what, full["radius"], full["search"], full["prior"], full["min_var"], full["min_score"])
    _check_pyramid(what, shape, full["levels"], full["radius"], full["fine_search"], full["median_radius"], full["min_count"])
    _check_positive(what, "tol", full["tol"], "pixels")
    _check_positive(what, "max_diff", full["max_diff"], "plane steps")
    return full


def _check_pair(what, map_a, keep_a, map_b, keep_b):
    for name, m, keep in (("map_a", map_a, keep_a), ("map_b", map_b, keep_b)):
        _check_depth_map(what, name, m)
        _check_grey(what, f"{name}.grey", m.grey)
        if m.grey.shape != m.plane.shape:
            raise ValueError(f"{what}: {name}.grey has the map's shape")
        _check_mask(what, "keep" + name[3:], keep, m.plane.shape)
    if map_a.plane.shape != map_b.plane.shape:
        raise ValueError(f"{what}: the two maps are of one camera and have one shape (got {tuple(map_a.plane.shape)} and {tuple(map_b.plane.shape)})")
    w_step = map_b.schedule[1]
    if not np.isfinite(w_step) or w_step == 0.0:
        raise ValueError(f"{what}: map_b's schedule has a w_step that is finite and not zero (got {w_step})")


def _check_dt(what, dt_days):
    if isinstance(dt_days, (bool, str)) or not isinstance(dt_days, (int, float, np.integer, np.floating)) or not np.isfinite(dt_days) or dt_days == 0:
        raise ValueError(f"{what}: dt_days must be a finite number of days that is not zero (got {dt_days!r})")


def surface_displacement(map_a: DepthMap, keep_a, map_b: DepthMap, keep_b, dt_days, check: bool = True, engine=None, **options) -> DisplacementField:
    """The dense displacement of the surface between two epochs of one camera: `match_flow` of map A's grey image into map B's on the pixels
    of `keep_a`; with `check`, the backward match of every pixel of B with the negated prior and `flow_consistency` within `tol` pixels;
    `lift_flow` of what is left; and the lifted pixels compacted in row-major order, as `dense.cloud_of` compacts a cloud.
    `options`: radius, search, prior, min_var, min_score of `match_flow`, tol of `flow_consistency`, max_diff of `lift_flow`; and levels
    (1: the single-level match above and nothing else), fine_search, median_radius, min_count of `match_flow_pyramid`, which takes the
    place of both matches where levels > 1: the backward field is the same pyramid with the images swapped, the prior negated and no mask."""
    what = "surface_displacement"
    _check_pair(what, map_a, keep_a, map_b, keep_b)
    _check_dt(what, dt_days)
    o = _options(what, options, map_a.grey.shape)
    eng = default_engine(engine)
    match = dict(radius=o["radius"], search=o["search"], min_var=o["min_var"], min_score=o["min_score"], engine=eng)
    matcher = match_flow
    if o["levels"] > 1:
        matcher = match_flow_pyramid
        match.update(levels=o["levels"], fine_search=o["fine_search"], median_radius=o["median_radius"], min_count=o["min_count"])
    fwd = matcher(map_a.grey, map_b.grey, ask=keep_a, prior=tuple(o["prior"]), **match)
    keep = fwd.valid
    if check:
        bwd = matcher(map_b.grey, map_a.grey, prior=(-int(o["prior"][0]), -int(o["prior"][1])), **match)
        keep = flow_consistency(fwd, bwd, o["tol"], engine=eng)
    P, D, ok = lift_flow(fwd, keep, map_a, map_b, keep_b, o["max_diff"], engine=eng)
    sel = ok != 0                                                                 # row-major, the order of the scan
    vu = torch.nonzero(sel)
    D = D[sel]
    # element by element against a tensor: torch divides by a Python number as a product with its reciprocal, which is not the quotient
    return DisplacementField(P[sel], D, D / torch.full_like(D, float(dt_days)), fwd.score[sel], torch.stack([vu[:, 1], vu[:, 0]], 1))


def day_number(date) -> float:
    """The day number of a date: a number as it is, a `datetime.date` / `datetime` by its ordinal (with the fraction of the day), a
    string in the project's "%Y_%m_%d"."""
    if isinstance(date, str):
        date = datetime.datetime.strptime(date, "%Y_%m_%d")
    if isinstance(date, datetime.datetime):
        return date.toordinal() + (date - datetime.datetime.combine(date.date(), datetime.time())).total_seconds() / 86400.0
    if isinstance(date, datetime.date):
        return float(date.toordinal())
    if isinstance(date, (bool,)) or not isinstance(date, (int, float, np.integer, np.floating)) or not np.isfinite(date):
        raise ValueError(f"displacement_series: a date is a day number, a datetime.date or a '%Y_%m_%d' string (got {date!r})")
    return float(date)


def displacement_series(maps, keeps, dates, camera: int = 0, lag: int = 1, check: bool = True, engine=None, **options):
    """`surface_displacement` for every epoch pair (e, e + lag) of a sequence: `maps` a list of E pairs of `DepthMap` as `build_depth_maps`
    returns them, `keeps` the E pairs of their keep masks (`dense.consistency`), `dates` the E dates (`day_number`), `camera` the view.
    Returns (fields, table): one `DisplacementField` per pair, and all pairs' rows one behind the other as a dict of host arrays under the
    float64 column names of `utils.tracking_features_utils` (X_ini .. Z_fin, dX .. dZ, vX .. vZ, V = |v|) with dt (days, float64) and
    ep_ini, ep_fin (epoch indices, int64): `np.stack([table["X_ini"], table["Y_ini"]], 1)` and a column go into
    `utils.binned_stats.compute_binned_stats2D` as they are."""
    what = "displacement_series"
    E = len(maps)
    _check_int(what, "lag", lag, 1, max(E - 1, 1))
    if camera not in (0, 1) or isinstance(camera, bool):
        raise ValueError(f"{what}: camera is 0 or 1 (got {camera!r})")
    if E < 2 or len(keeps) != E or len(dates) != E:
        raise ValueError(f"{what}: two or more epochs with a pair of keep masks and a date each are expected (got {E} maps, {len(keeps)} keeps, {len(dates)} dates)")
    days = [day_number(d) for d in dates]
    o = _options(what, options)
    pairs = [(e, e + lag) for e in range(E - lag)]
    for a, b in pairs:
        _check_pair(what, maps[a][camera], keeps[a][camera], maps[b][camera], keeps[b][camera])
        _check_dt(what, days[b] - days[a])
        _options(what, options, maps[a][camera].grey.shape)
    eng = default_engine(engine)
    fields = [surface_displacement(maps[a][camera], keeps[a][camera], maps[b][camera], keeps[b][camera], days[b] - days[a], check, engine=eng, **o)
              for a, b in pairs]
    cols = []
    for f in fields:
        v = f.velocity
        speed = torch.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        cols.append(torch.cat([f.points, f.points + f.displacement, f.displacement, v, speed[:, None]], 1))
    host = torch.cat(cols).cpu().numpy()
    table = {k: np.ascontiguousarray(host[:, j]) for j, k in enumerate(F64_COLS)}
    counts = [len(f.points) for f in fields]
    table["dt"] = np.repeat(np.array([days[b] - days[a] for a, b in pairs], np.float64), counts)
    table["ep_ini"] = np.repeat(np.array([a for a, _ in pairs], np.int64), counts)
    table["ep_fin"] = np.repeat(np.array([b for _, b in pairs], np.int64), counts)
    return fields, table
