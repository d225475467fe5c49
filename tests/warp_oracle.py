"""numpy restatement of the image stabilisation kernels (csrc/warp.hip, csrc/warp_pixel.h), operation for operation: the source
coordinates of cv2.warpPerspective(src, H, (w, h)) and cv2.undistort(src, K, dist, None, K) in float64, their rounding to 1/32 pixel,
and the four-tap integer sum of OpenCV's documented 8-bit INTER_LINEAR path with BORDER_CONSTANT 0. THIS IS NOT OPENCV: parity with an
OpenCV binary is not pinned anywhere in this project; what is pinned is that the kernels equal this file bit for bit. numpy's elementwise
float64 operations are single IEEE operations (no contraction), integers follow the rounding, so equality is exact.

Also here: the 'sxyz' Euler angle pair the driver's rotation smoothing uses, the cases of the host and device tests (one list for both),
and the procedural test image."""
import math
import os

import numpy as np


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------------
def inv3(M):
    """Cofactor inverse in Python floats; each entry = cofactor * (1 / det)."""
    a, b, c, d, e, f, g, h, i = (float(v) for v in np.asarray(M, np.float64).reshape(9))
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    s = 1.0 / det
    return np.array([[(e * i - f * h) * s, (c * h - b * i) * s, (b * f - c * e) * s],
                     [(f * g - d * i) * s, (a * i - c * g) * s, (c * d - a * f) * s],
                     [(d * h - e * g) * s, (b * g - a * h) * s, (a * e - b * d) * s]])


def fix(v):
    """v = coordinates times 32 -> (finite, integer pixel saturated to a short, 5-bit fraction)."""
    v = np.asarray(v, np.float64)
    finite = np.isfinite(v)
    c = np.clip(np.where(finite, v, 0.0), -2147483648.0, 2147483647.0)
    X = np.rint(c).astype(np.int64)                       # ties to even; the clamp keeps it inside int32
    return finite, np.clip(X >> 5, -32768, 32767), X & 31


def remap(src, sx, sy):
    """src [h, w] or [h, w, C] uint8; sx, sy [oh, ow] float64 coordinates times 32 -> [oh, ow(, C)] uint8."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3)
    s3 = src.reshape(src.shape[0], src.shape[1], -1).astype(np.int64)
    h, w = s3.shape[:2]
    okx, xi, fx = fix(sx)
    oky, yi, fy = fix(sy)
    ok = okx & oky

    def tap(y, x):
        inside = ok & (y >= 0) & (y < h) & (x >= 0) & (x < w)
        p = s3[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
        return np.where(inside[..., None], p, 0)

    w00, w01 = 32 * (32 - fx) * (32 - fy), 32 * fx * (32 - fy)
    w10, w11 = 32 * (32 - fx) * fy, 32 * fx * fy
    assert ((w00 + w01 + w10 + w11) == 32768).all()
    acc = (w00[..., None] * tap(yi, xi) + w01[..., None] * tap(yi, xi + 1) + w10[..., None] * tap(yi + 1, xi)
           + w11[..., None] * tap(yi + 1, xi + 1))
    out = ((acc + 16384) >> 15).astype(np.uint8)
    return out.reshape(sx.shape + src.shape[2:])


def warp_coords(M, oh, ow):
    """M = the INVERSE homography (output -> source). Coordinates times 32 of every output pixel, formed per 64-pixel block."""
    M = np.asarray(M, np.float64).reshape(3, 3)
    x = np.arange(ow, dtype=np.int64)[None, :]
    y = np.arange(oh, dtype=np.int64)[:, None].astype(np.float64)
    xb = (64 * (x // 64)).astype(np.float64)
    x1 = (x - 64 * (x // 64)).astype(np.float64)
    with np.errstate(all="ignore"):
        X0 = (M[0, 0] * xb + M[0, 1] * y) + M[0, 2]
        Y0 = (M[1, 0] * xb + M[1, 1] * y) + M[1, 2]
        W0 = (M[2, 0] * xb + M[2, 1] * y) + M[2, 2]
        W = W0 + M[2, 0] * x1
        Wi = np.where(W != 0.0, 32.0 / np.where(W != 0.0, W, 1.0), 0.0)
        return (X0 + M[0, 0] * x1) * Wi, (Y0 + M[1, 0] * x1) * Wi


def warp_perspective_inv(src, M, oh, ow):
    sx, sy = warp_coords(M, oh, ow)
    return remap(src, sx, sy)


def warp_perspective(src, H, dsize):
    """cv2.warpPerspective(src, H, (w, h)) restated."""
    return warp_perspective_inv(src, inv3(H), dsize[1], dsize[0])


def dist8(dist):
    d = np.zeros(0) if dist is None else np.asarray(dist, np.float64).ravel()
    assert len(d) in (0, 4, 5, 8), len(d)
    k = np.zeros(8)
    k[:len(d)] = d
    return k


def undistort_coords(ir, intr, k, h, w):
    """ir = inverse K (3 x 3); intr = fx fy cx cy; k = k1 k2 p1 p2 k3 k4 k5 k6. Coordinates times 32."""
    ir = np.asarray(ir, np.float64).reshape(9)
    fx, fy, cx, cy = (np.float64(v) for v in intr)
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(v) for v in k)
    j = np.arange(w, dtype=np.float64)[None, :]
    i = np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        _x = j * ir[0] + (i * ir[1] + ir[2])
        _y = j * ir[3] + (i * ir[4] + ir[5])
        _w = j * ir[6] + (i * ir[7] + ir[8])
        iw = 1.0 / _w
        x, y = _x * iw, _y * iw
        x2, y2 = x * x, y * y
        r2, _2xy = x2 + y2, 2.0 * x * y
        kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = (x * kr + p1 * _2xy) + p2 * (r2 + 2.0 * x2)
        yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * _2xy
        u = fx * xd + cx
        v = fy * yd + cy
        return u * 32.0, v * 32.0


def cam_row(K, dist):
    """The 21 doubles of `im_undistort_image`: inv3(K), fx fy cx cy, eight coefficients."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    return np.ascontiguousarray(np.concatenate([inv3(K).ravel(), [K[0, 0], K[1, 1], K[0, 2], K[1, 2]], dist8(dist)]))


def undistort_row(src, row):
    h, w = src.shape[:2]
    sx, sy = undistort_coords(row[:9], row[9:13], row[13:21], h, w)
    return remap(src, sx, sy)


def undistort(src, K, dist):
    """cv2.undistort(src, K, dist, None, K) restated."""
    return undistort_row(src, cam_row(K, dist))


# ---- 'sxyz' Euler angles -------------------------------------------------------------------------------------------------------------
def euler_from_matrix(R):
    M = np.asarray(R, np.float64)[:3, :3]
    cy = math.sqrt(M[0, 0] * M[0, 0] + M[1, 0] * M[1, 0])
    if cy > 4.0 * np.finfo(np.float64).eps:
        return math.atan2(M[2, 1], M[2, 2]), math.atan2(-M[2, 0], cy), math.atan2(M[1, 0], M[0, 0])
    return math.atan2(-M[1, 2], M[1, 1]), math.atan2(-M[2, 0], cy), 0.0


def euler_matrix(ax, ay, az):
    """Rz(az) Ry(ay) Rx(ax), entry by entry: each entry is one or two products of the six sines and cosines."""
    sx, sy, sz = math.sin(ax), math.sin(ay), math.sin(az)
    cx, cy, cz = math.cos(ax), math.cos(ay), math.cos(az)
    return np.array([[cy * cz, sy * (sx * cz) - cx * sz, sy * (cx * cz) + sx * sz],
                     [cy * sz, sy * (sx * sz) + cx * cz, sy * (cx * sz) - sx * cz],
                     [-sy, cy * sx, cy * cx]])


def window(ep, n, width=5):
    s = min(max(ep - width // 2, 0), n - width)
    return range(s, s + width)


# ---- test material -------------------------------------------------------------------------------------------------------------------
def image_pattern(h, w, c=3, seed=0):
    """A procedural uint8 image [h, w, c] from integer arithmetic alone (the same bytes on every machine): hashed levels on 6 x 4 blocks
    (an edge every few pixels in both directions, flat in between, so resampled copies still compress), different per channel and seed."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    out = np.empty((h, w, c), np.uint8)
    for ch in range(c):
        s = seed * 4 + ch
        bx, by = (x + s) // 6, (y + 2 * s) // 4
        out[:, :, ch] = (20 + ((bx * 73856093 + by * 19349663 + (s + 1) * 83492791) % 251) % 216).astype(np.uint8)
    return out


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_stabilise.npz")
FULL_WIDTH = 6012


def scale_K(K, width, full_width=FULL_WIDTH):
    """K of a calibration for a `full_width`-pixel frame, scaled to a frame `width` pixels wide."""
    s = width / full_width
    return np.array([[K[0, 0] * s, 0.0, K[0, 2] * s], [0.0, K[1, 1] * s, K[1, 2] * s], [0.0, 0.0, 1.0]])


_calib = {}


def scaled_calib(name, width):
    """(K, dist) of an asset calibration ("cam1", "cam2": the numbers are in the fixture) scaled to a frame `width` pixels wide."""
    if not _calib:
        with np.load(GOLDEN, allow_pickle=False) as g:
            for cam in ("cam1", "cam2"):
                _calib[cam] = (g[f"calib_{cam}_K"], g[f"calib_{cam}_dist"])
    K, dist = _calib[name]
    return scale_K(K, width), dist.copy()


WARP_SHAPES = [(1, 1), (1, 257), (3, 63), (2, 64), (2, 65), (5, 255), (5, 256), (5, 257), (97, 131)]


def warp_matrices(h, w):
    """name -> H (source -> output) for an h x w image; the kernels get inv3(H). `None` entries give the inverse directly."""
    a = math.radians(10.0)
    c, s = math.cos(a), math.sin(a)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    rot = np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0.0, 0.0, 1.0]])

    def shift(dx, dy):
        return np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])
    return {
        "identity": np.eye(3),
        "shift right": shift(1.0, 0.0), "shift left": shift(-1.0, 0.0), "shift down": shift(0.0, 1.0), "shift up": shift(0.0, -1.0),
        "half pixel": shift(0.5, 0.5),
        "rotation 10 deg": rot,
        "outside": shift(1.0e5, -1.0e5),
        "scale 1e12": np.diag([1.0e-12, 1.0e-12, 1.0]),          # inverse: source coordinates of 1e12 x: the int clamp, the short clamp
    }


def warp_inverse_cases(h, w):
    """Inverse matrices given directly: W = x - 3 is exactly 0 at column 3 and negative to its left."""
    return {"W crosses zero": np.array([[2.0, 0.0, 1.0], [0.0, 2.0, 1.0], [1.0, 0.0, -3.0]]),
            "W crosses zero, oblique": np.array([[1.0, 1.0, 0.0], [0.0, 3.0, 2.0], [1.0, 1.0, -4.0]])}


def all_inverses(h, w):
    out = {k: inv3(H) for k, H in warp_matrices(h, w).items()}
    out.update(warp_inverse_cases(h, w))
    return out


def undistort_cases():
    """(name, h, w, K, dist): every path of the undistortion."""
    cases = []
    for cam in ("cam1", "cam2"):
        K, d = scaled_calib(cam, 257)
        cases.append((f"zero distortion, {cam}", 4, 257, K, np.zeros(5)))
        for h, w in ((5, 65), (97, 131)):
            K, d = scaled_calib(cam, w)
            cases.append((f"asset coefficients, {cam}, {h}x{w}", h, w, K, d))
    K, d = scaled_calib("cam1", 131)
    cases.append(("4 coefficients", 97, 131, K, d[:4]))
    cases.append(("5 coefficients, k3", 97, 131, K, np.r_[d[:4], 0.35]))
    cases.append(("8 coefficients", 97, 131, K, np.r_[d[:4], 0.35, 0.02, -0.15, 0.07]))
    cases.append(("tangential only", 97, 131, K, np.array([0.0, 0.0, 0.03, -0.02])))
    cases.append(("strong barrel: corners sample outside", 97, 131, K, np.array([3.0, 0.0, 0.0, 0.0])))
    # fx = fy = 1, cx = cy = 0, k4 = -1: pixel (row 0, column 1) has r2 = 1, kr = 1 / 0 = inf, y = 0, so v = 0 * inf = NaN -> 0
    cases.append(("one non-finite coordinate", 3, 5, np.eye(3), np.array([0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0])))
    return cases


def warp_cases(shapes=None):
    """(name, src [n, h, w, c], minv [n, 9], oh, ow): every shape with 1, 3 and 4 channels, every matrix on one image, three images with
    three matrices in one call, and an output size other than the input's."""
    cases = []
    for h, w in (WARP_SHAPES if shapes is None else shapes):
        inv = all_inverses(h, w)
        for c in (1, 3, 4):
            imgs = np.stack([image_pattern(h, w, c, seed=s) for s in range(3)])
            for name, M in inv.items():
                cases.append((f"{h}x{w}x{c} {name}", imgs[:1], M.reshape(1, 9), h, w))
            three = np.stack([inv["rotation 10 deg"], inv["half pixel"], inv["W crosses zero"]]).reshape(3, 9)
            cases.append((f"{h}x{w}x{c} three images, three matrices", imgs, three, h, w))
    if shapes is None:
        inv = all_inverses(5, 65)
        for c in (1, 3, 4):
            imgs = np.stack([image_pattern(5, 65, c, seed=s) for s in range(3)])
            three = np.stack([inv["rotation 10 deg"], inv["shift left"], inv["W crosses zero, oblique"]]).reshape(3, 9)
            cases.append((f"5x65x{c} -> 7x200", imgs, three, 7, 200))
    return cases


def warp_expected(case):
    _, src, minv, oh, ow = case
    return np.stack([warp_perspective_inv(src[b], minv[b], oh, ow) for b in range(len(src))])


def undistort_inputs(case, c=3, n=1):
    """(src [n, h, w, c], the 21 doubles) of an undistortion case."""
    _, h, w, K, dist = case
    return np.stack([image_pattern(h, w, c, seed=s) for s in range(n)]), cam_row(K, dist)
