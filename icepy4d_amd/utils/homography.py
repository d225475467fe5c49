"""Image stabilisation for image correlation: `homography_warping` of the reference (`utils/homography.py`) and the rotation smoothing
of its driver (`main_dev.py:453-481`), with the resampling on the device (csrc/warp.hip: `im_undistort_image`, `im_warp_perspective`).

The reference resamples with cv2.undistort and cv2.warpPerspective. OpenCV is not a dependency of this project: the kernels restate its
documented 8-bit INTER_LINEAR path (float64 source coordinates rounded to 1/32 pixel, four integer-weighted taps, zero border) and are
bit-identical with the numpy restatement `tests/warp_oracle.py`; parity with a particular OpenCV binary is not pinned. Channels are
independent, so the reference's RGB <-> BGR flips around its calls cancel and are not performed: images stay in the order given.
There is no host fallback: without the library or a device every call raises."""
import math
from copy import deepcopy
from pathlib import Path

import numpy as np
import torch

from .._lib import ptr
from ..engine import default_engine, to_device

MAX_SIDE = 32766                 # the taps' coordinates are saturated to a short, as in OpenCV
WORK_BYTES = 1 << 30             # `stabilise_sequence`: bound on its two working buffers (uploaded chunk, undistorted chunk) together
_EULER_EPS = 4.0 * np.finfo(np.float64).eps


# ---- small host algebra -------------------------------------------------------------------------------------------------------------
def inv3(M) -> np.ndarray:
    """The inverse of a 3 x 3 matrix by cofactors, in Python floats: every entry is its cofactor times 1 / det. The kernels receive
    inverted matrices and never invert; this fixed formula (and not LAPACK's) is part of what the oracle pins. ValueError when the
    matrix or its inverse is not finite or the determinant is zero."""
    M = np.asarray(M, np.float64)
    if M.shape != (3, 3):
        raise ValueError(f"expected a 3x3 matrix (got shape {M.shape})")
    a, b, c, d, e, f, g, h, i = (float(v) for v in M.ravel())
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    if not math.isfinite(det) or det == 0.0:
        raise ValueError("the matrix is singular or not finite")
    s = 1.0 / det
    out = np.array([[(e * i - f * h) * s, (c * h - b * i) * s, (b * f - c * e) * s],
                    [(f * g - d * i) * s, (a * i - c * g) * s, (c * d - a * f) * s],
                    [(d * h - e * g) * s, (b * g - a * h) * s, (a * e - b * d) * s]])
    if not np.isfinite(out).all():
        raise ValueError("the inverse of the matrix is not finite")
    return out


def euler_from_matrix(R) -> tuple:
    """Static-frame x-y-z Euler angles ('sxyz') of a rotation matrix (the upper 3 x 3 of what is given): R = Rz(az) Ry(ay) Rx(ax).
    cos(ay) is the length of the first column's upper two entries; where it vanishes (gimbal lock) az is set to 0."""
    M = np.asarray(R, np.float64)[:3, :3]
    cy = math.sqrt(M[0, 0] * M[0, 0] + M[1, 0] * M[1, 0])
    if cy > _EULER_EPS:
        return math.atan2(M[2, 1], M[2, 2]), math.atan2(-M[2, 0], cy), math.atan2(M[1, 0], M[0, 0])
    return math.atan2(-M[1, 2], M[1, 1]), math.atan2(-M[2, 0], cy), 0.0


def euler_matrix(ax: float, ay: float, az: float) -> np.ndarray:
    """The 3 x 3 rotation Rz(az) Ry(ay) Rx(ax) of 'sxyz' angles, entry by entry."""
    sx, sy, sz = math.sin(ax), math.sin(ay), math.sin(az)
    cx, cy, cz = math.cos(ax), math.cos(ay), math.cos(az)
    cxcz, cxsz, sxcz, sxsz = cx * cz, cx * sz, sx * cz, sx * sz
    return np.array([[cy * cz, sy * sxcz - cxsz, sy * cxcz + sxsz],
                     [cy * sz, sy * sxsz + cxcz, sy * cxsz - sxcz],
                     [-sy, cy * sx, cy * cx]])


def smoothing_window(ep: int, n: int, window: int = 5) -> range:
    """The epochs whose rotations smooth epoch `ep` of n: `window` of them, centred where the sequence allows it."""
    if window < 1 or n < window:
        raise ValueError(f"a window of {window} epochs needs at least as many cameras (got {n})")
    s = min(max(ep - window // 2, 0), n - window)
    return range(s, s + window)


def smooth_camera_rotations(cameras, window: int = 5, use_median: bool = True) -> list:
    """The driver's pose smoothing (`main_dev.py:453-481`): per epoch the median (or mean) of each Euler angle over `smoothing_window`,
    the rotation rebuilt from the three angles. Returns copies of the cameras with that rotation; translation columns stay."""
    cameras = list(cameras)
    angles = np.array([euler_from_matrix(c.R) for c in cameras]).reshape(len(cameras), 3)
    out = []
    for ep, cam in enumerate(cameras):
        win = smoothing_window(ep, len(cameras), window)
        stack = np.stack([angles[e] for e in win], axis=1)
        ang = np.median(stack, axis=1) if use_median else np.mean(stack, axis=1)
        cam = deepcopy(cam)
        ext = deepcopy(cam.extrinsics)
        ext[:3, :3] = euler_matrix(*ang)
        cam.update_extrinsics(ext)
        out.append(cam)
    return out


def homography(cam_0, cam_1) -> np.ndarray:
    """H = K0 R K1^-1 that maps pixels of `cam_1` onto `cam_0` for a pure rotation, by the reference's camera algebra: copies of both
    cameras, T = inv(cam_0.pose), both extrinsics updated through pose_to_extrinsics(T @ pose)."""
    ref, cam = deepcopy(cam_0), deepcopy(cam_1)
    to_ref = np.linalg.inv(ref.pose)                     # the reference camera's frame becomes the world frame
    for c in (ref, cam):
        c.update_extrinsics(c.pose_to_extrinsics(to_ref @ c.pose))
    try:
        return (ref.K @ cam.R) @ np.linalg.inv(cam.K)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"homography_warping: the K of the camera to warp is singular ({e})") from None


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def undistort_params(camera) -> np.ndarray:
    """h_cam of `im_undistort_image`, [21] float64: inv3(K), fx fy cx cy, k1 k2 p1 p2 k3 k4 k5 k6. ValueError for a singular or
    non-finite K, a non-finite coefficient and a distortion vector of a length other than 4, 5 or 8."""
    K = np.asarray(camera.K, np.float64)
    if K.shape != (3, 3) or not np.isfinite(K).all():
        raise ValueError("undistort_image: K must be a finite 3x3 matrix")
    dist = np.asarray(camera.dist, np.float64).ravel() if camera.dist is not None else None
    if dist is None or len(dist) not in (4, 5, 8):
        raise ValueError(f"undistort_image: distortion vectors of length 4, 5 or 8 are supported (got {None if dist is None else len(dist)})")
    if not np.isfinite(dist).all():
        raise ValueError("undistort_image: the distortion coefficients must be finite")
    k = np.zeros(8)
    k[:len(dist)] = dist
    return np.ascontiguousarray(np.concatenate([inv3(K).ravel(), [K[0, 0], K[1, 1], K[0, 2], K[1, 2]], k]))


def inverse_homography(H) -> np.ndarray:
    """inv3(H) as the [9] float64 row of `im_warp_perspective`; ValueError for a singular or non-finite H."""
    H = np.asarray(H, np.float64)
    if H.shape != (3, 3) or not np.isfinite(H).all():
        raise ValueError("homography_warping: H must be a finite 3x3 matrix")
    return np.ascontiguousarray(inv3(H).ravel())


def _is_tensor(x) -> bool:
    return hasattr(x, "data_ptr")


def _check_image(image, batched: bool = False) -> tuple:
    """(h, w, c, had a channel axis) of a uint8 image H x W [x C] (with a leading n when `batched`), numpy or device tensor."""
    if _is_tensor(image):
        ok = image.dtype == torch.uint8
    else:
        ok = isinstance(image, np.ndarray) and image.dtype == np.uint8
    if not ok:
        raise ValueError("expected a uint8 image (numpy array or device tensor)")
    shape = tuple(image.shape[1:] if batched else image.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"expected an image of shape H x W or H x W x C (got {tuple(image.shape)})")
    h, w, c = shape[0], shape[1], shape[2] if len(shape) == 3 else 1
    if not (1 <= c <= 4 and 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"expected 1..4 channels and sides of 1..{MAX_SIDE} pixels (got {h} x {w} x {c})")
    return h, w, c, len(shape) == 3


def _on_engine(eng, image):
    """The image as a contiguous tensor on the engine's device; a tensor that lives elsewhere is refused, not moved."""
    if _is_tensor(image):
        if image.device != eng.device:
            raise ValueError(f"the image is on {image.device}, the engine on {eng.device}")
        return image.contiguous()
    return to_device(image, eng.device)


def _write(out_path, image) -> None:
    """Through PIL, channels as given (RGB in, RGB on disk); byte parity with OpenCV's encoders is not claimed."""
    from PIL import Image
    out_path = Path(out_path)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    a = image.cpu().numpy() if _is_tensor(image) else image
    Image.fromarray(a[:, :, 0] if a.ndim == 3 and a.shape[2] == 1 else a).save(str(out_path))


# ---- the two launches ----------------------------------------------------------------------------------------------------------------
def undistort_device(eng, d_src, h_cam: np.ndarray, d_dst=None):
    """`im_undistort_image` on a contiguous [n, h, w, c] uint8 device tensor: one camera for all images."""
    n, h, w, c = d_src.shape
    if d_dst is None:
        d_dst = torch.empty_like(d_src)
    eng.ctx.call("im_undistort_image", ptr(d_src), n, h, w, c, h_cam.ctypes.data, ptr(d_dst), eng.stream_ptr())
    return d_dst


def warp_device(eng, d_src, minv: np.ndarray, out_hw=None, d_dst=None):
    """`im_warp_perspective` on a contiguous [n, h, w, c] uint8 device tensor: minv [n, 9] float64 (host), one inverse per image."""
    n, h, w, c = d_src.shape
    oh, ow = (h, w) if out_hw is None else out_hw
    d_minv = to_device(np.asarray(minv, np.float64).reshape(n, 9), eng.device)
    if d_dst is None:
        d_dst = torch.empty((n, oh, ow, c), dtype=torch.uint8, device=eng.device)
    eng.ctx.call("im_warp_perspective", ptr(d_src), n, h, w, c, ptr(d_minv), oh, ow, ptr(d_dst), eng.stream_ptr())
    return d_dst


def _like_input(image, d_out, had_c: bool):
    """One image back in the kind it came in: device tensor or numpy, with or without the channel axis."""
    out = d_out[0] if had_c else d_out[0, :, :, 0]
    return out if _is_tensor(image) else out.cpu().numpy()


def undistort_image(image, camera, out_path=None, engine=None):
    """`undistort_image` of the reference (`sfm/geometry.py:121-143`: cv2.undistort(image, K, dist, None, K)) on the device. A uint8
    H x W [x C] numpy array or device tensor; returns the same kind."""
    h, w, c, had_c = _check_image(image)
    h_cam = undistort_params(camera)
    eng = default_engine(engine)
    d_out = undistort_device(eng, _on_engine(eng, image).reshape(1, h, w, c), h_cam)
    out = _like_input(image, d_out, had_c)
    if out_path is not None:
        _write(out_path, out)
    return out


def homography_warping(cam_0, cam_1, image, undistort: bool = False, out_path=None, engine=None):
    """`homography_warping` of the reference: `image` of `cam_1` resampled into the orientation and the K of `cam_0`, optionally
    undistorted first with `cam_1`'s K and dist, at the input's size. A uint8 H x W [x C] numpy array or device tensor in, the same kind
    out. Everything is validated before the first launch."""
    h, w, c, had_c = _check_image(image)
    minv = inverse_homography(homography(cam_0, cam_1))
    h_cam = undistort_params(cam_1) if undistort else None
    eng = default_engine(engine)
    d = _on_engine(eng, image).reshape(1, h, w, c)
    if undistort:
        d = undistort_device(eng, d, h_cam)
    out = _like_input(image, warp_device(eng, d, minv[None]), had_c)
    if out_path is not None:
        _write(out_path, out)
    return out


def stabilise_sequence(cam_ref, cameras, images, undistort: bool = True, engine=None, to_host: bool = False):
    """All epochs of one camera: image e of `cameras[e]` warped onto `cam_ref`, as `homography_warping` per image, in one undistort
    launch and one warp launch per chunk. `images`: a list of equal-shape uint8 arrays or an [n, h, w, c] device tensor. Returns an
    [n, h, w, c] uint8 device tensor (numpy with `to_host`). The images go through in chunks whose two working buffers (the uploaded
    chunk of a host list, the undistorted chunk) hold at most WORK_BYTES together, or one image each; the result itself is not counted.
    One undistort launch takes one camera: epochs of a chunk whose K or dist differ are undistorted in runs of equal intrinsics."""
    cameras = list(cameras)
    if _is_tensor(images):
        if images.ndim != 4:
            raise ValueError(f"expected an [n, h, w, c] tensor (got {tuple(images.shape)})")
        n = images.shape[0]
        h, w, c, _ = _check_image(images, batched=True)
    else:
        images = list(images)
        n = len(images)
        if n == 0:
            raise ValueError("no images")
        shapes = {_check_image(im)[:3] + (im.ndim,) for im in images}
        if len(shapes) != 1:
            raise ValueError("the images must have one shape")
        h, w, c, _ = shapes.pop()
    if n != len(cameras) or n == 0:
        raise ValueError(f"{n} images for {len(cameras)} cameras")
    minv = np.stack([inverse_homography(homography(cam_ref, cam)) for cam in cameras])
    cams = [undistort_params(cam) for cam in cameras] if undistort else None
    eng = default_engine(engine)
    if _is_tensor(images) and images.device != eng.device:
        raise ValueError(f"the images are on {images.device}, the engine on {eng.device}")
    out = torch.empty((n, h, w, c), dtype=torch.uint8, device=eng.device)
    chunk = max(1, WORK_BYTES // (2 * h * w * c))
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        if _is_tensor(images):
            d = images[a:b].contiguous()
        else:
            d = to_device(np.stack([np.asarray(im).reshape(h, w, c) for im in images[a:b]]), eng.device)
        if undistort:
            und = torch.empty_like(d)
            r = a
            while r < b:                                     # runs of equal intrinsics: one launch each, one in all for a fixed camera
                e = r + 1
                while e < b and np.array_equal(cams[e], cams[r]):
                    e += 1
                undistort_device(eng, d[r - a:e - a], cams[r], und[r - a:e - a])
                r = e
            d = und
        warp_device(eng, d, minv[a:b], d_dst=out[a:b])
    return out.cpu().numpy() if to_host else out
