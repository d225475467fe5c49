"""The numpy restatement of two-view dense stereo (csrc/dense_pixel.h): a plane sweep over fronto-parallel planes of the
reference view scored by the zero-mean normalised cross-correlation of exact integer window sums, the consistency of the two maps, and the
cloud of the kept pixels with camera-oriented normals. A definition of this project's own: Metashape's matcher is closed and is not
reproduced. float64 element by element in the association of the header (numpy never contracts), integers behind the coordinate rounding
(`warp_oracle.fix`), so the kernels equal this bit for bit whatever order they sum in."""
import numpy as np

import warp_oracle as W

MAX_SIDE, MAX_PLANES, MAX_RADIUS = 16384, 4096, 7
FILTERS = {"NoFiltering": None, "MildFiltering": 2.0, "ModerateFiltering": 1.0, "AggressiveFiltering": 0.5}
DBL_MAX = 1.7976931348623157e308


def filter_tau(name):
    """tau of a `depth_filter` name; the reference's ValueError text for an unknown one (`metashape.py:209-222`)."""
    if name not in FILTERS:
        raise ValueError("Error: invalid choise of depth filtering. Choose one in [NoFiltering, MildFiltering, ModerateFiltering, AggressiveFiltering]")
    return FILTERS[name]


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------
def plane_h(A, B, w_first, w_step, k):
    A, B = np.asarray(A, np.float64).reshape(9), np.asarray(B, np.float64).reshape(9)
    with np.errstate(all="ignore"):
        wk = np.float64(w_first) + np.float64(k) * np.float64(w_step)
        return A + wk * B


def sample(src, H, h0, w0):
    """(b [h0, w0] int64, ok [h0, w0] bool): the warped value of every ref pixel under the plane's homography H [9]."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2
    h1, w1 = src.shape
    u = np.arange(w0, dtype=np.float64)[None, :]
    v = np.arange(h0, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        x = (H[0] * u + H[1] * v) + H[2]
        y = (H[3] * u + H[4] * v) + H[5]
        z = (H[6] * u + H[7] * v) + H[8]
        front = z > 0.0
        okx, xi, fx = W.fix((x / z) * 32.0)
        oky, yi, fy = W.fix((y / z) * 32.0)
    ok = front & okx & oky & (xi >= 0) & (xi + 1 < w1) & (yi >= 0) & (yi + 1 < h1)
    xc, yc = np.clip(xi, 0, max(w1 - 2, 0)), np.clip(yi, 0, max(h1 - 2, 0))
    s = src.astype(np.int64)
    if h1 < 2 or w1 < 2:
        return np.zeros((h0, w0), np.int64), np.zeros((h0, w0), bool)
    b = ((32 - fx) * (32 - fy)) * s[yc, xc] + (fx * (32 - fy)) * s[yc, xc + 1] + ((32 - fx) * fy) * s[yc + 1, xc] + (fx * fy) * s[yc + 1, xc + 1]
    return np.where(ok, b, 0), ok


def box(img, r):
    """Sums over the (2 r + 1)^2 window of every pixel whose window lies inside, int64 [h - 2 r, w - 2 r] (empty where none does)."""
    img = np.asarray(img, np.int64)
    h, w = img.shape
    if h < 2 * r + 1 or w < 2 * r + 1:
        return np.zeros((max(h - 2 * r, 0), max(w - 2 * r, 0)), np.int64)
    c = np.zeros((h + 1, w + 1), np.int64)
    c[1:, 1:] = img.cumsum(0).cumsum(1)
    s = 2 * r + 1
    return c[s:, s:] - c[:-s, s:] - c[s:, :-s] + c[:-s, :-s]


def score(n, sa, saa, sb, sbb, sab, min_var):
    """(valid, s) of windows from their integer sums (int64 arrays)."""
    VA, VB, C = n * saa - sa * sa, n * sbb - sb * sb, n * sab - sa * sb
    valid = ~((VA < n * n * min_var) | (VB < n * n * min_var * (1 << 20)) | (VA <= 0) | (VB <= 0))
    with np.errstate(all="ignore"):
        s = C.astype(np.float64) / np.sqrt(VA.astype(np.float64) * VB.astype(np.float64))
    return valid, np.where(valid, s, 0.0)


def scores(ref, src, A, B, w_first, w_step, D, r, min_var=4):
    """(valid [D, h0, w0] bool, s [D, h0, w0] float64): the whole cost volume (the kernel never stores it)."""
    ref = np.asarray(ref)
    assert ref.dtype == np.uint8 and ref.ndim == 2
    h0, w0 = ref.shape
    a = ref.astype(np.int64)
    n = (2 * r + 1) ** 2
    sa, saa = box(a, r), box(a * a, r)
    valid, s = np.zeros((D, h0, w0), bool), np.zeros((D, h0, w0))
    if sa.size == 0:
        return valid, s
    for k in range(D):
        b, ok = sample(src, plane_h(A, B, w_first, w_step, k), h0, w0)
        inv = box(~ok, r)
        v, sc = score(n, sa, saa, box(b, r), box(b * b, r), box(a * b, r), min_var)
        valid[k, r:h0 - r, r:w0 - r] = v & (inv == 0)
        s[k, r:h0 - r, r:w0 - r] = np.where(v & (inv == 0), sc, 0.0)
    return valid, s


def choose(valid, s, w_first, w_step, min_score):
    """(plane int16, w float64, score float32) [h0, w0] from the cost volume: the running best in ascending plane order."""
    D, h0, w0 = s.shape
    k = np.full((h0, w0), -1, np.int64)
    s0 = np.zeros((h0, w0))
    for d in range(D):
        rep = valid[d] & ((k < 0) | (s[d] > s0))
        k, s0 = np.where(rep, d, k), np.where(rep, s[d], s0)
    kc = np.clip(k, 1, max(D - 2, 1))
    ii, jj = np.indices((h0, w0))
    if D >= 3:
        sm, sp, vm, vp = s[kc - 1, ii, jj], s[kc + 1, ii, jj], valid[kc - 1, ii, jj], valid[kc + 1, ii, jj]
    else:
        sm = sp = np.zeros((h0, w0))
        vm = vp = np.zeros((h0, w0), bool)
    with np.errstate(all="ignore"):
        den = (sm - 2.0 * s0) + sp
        use = (k >= 1) & (k <= D - 2) & vm & vp & (den < 0.0)
        off = np.where(use, (0.5 * (sm - sp)) / np.where(use, den, 1.0), 0.0)
        w = np.float64(w_first) + (k.astype(np.float64) + off) * np.float64(w_step)
    kept = (k >= 0) & ~(s0 < min_score)
    return np.where(kept, k, -1).astype(np.int16), np.where(kept, w, 0.0), np.where(kept, s0, 0.0).astype(np.float32)


def sweep(ref, src, A, B, w_first, w_step, D, r, min_var=4, min_score=0.8):
    valid, s = scores(ref, src, A, B, w_first, w_step, D, r, min_var)
    return choose(valid, s, w_first, w_step, min_score)


# ---- consistency ------------------------------------------------------------------------------------------------------------------------
def backproject(Ki, h, w, wmap):
    """X0 [h, w, 3] = Ki (u, v, 1) / w of every pixel."""
    Ki = np.asarray(Ki, np.float64).reshape(9)
    u = np.arange(w, dtype=np.float64)[None, :]
    v = np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        return np.stack([((Ki[3 * i] * u + Ki[3 * i + 1] * v) + Ki[3 * i + 2]) / wmap for i in range(3)], -1)


def consistency(plane0, w0map, plane1, w1map, pose, tol, check=True):
    """keep [h0, w0] uint8. pose [30] = inv(K0), R, t, K1."""
    keep = np.asarray(plane0) >= 0
    if not check:
        return keep.astype(np.uint8)
    pose = np.asarray(pose, np.float64).reshape(30)
    Ki, R, t, K1 = pose[:9], pose[9:18], pose[18:21], pose[21:]
    h0, w0 = plane0.shape
    h1, w1 = plane1.shape
    with np.errstate(all="ignore"):
        X0 = backproject(Ki, h0, w0, np.where(keep, w0map, 1.0))
        X1 = [((R[3 * i] * X0[..., 0] + R[3 * i + 1] * X0[..., 1]) + R[3 * i + 2] * X0[..., 2]) + t[i] for i in range(3)]
        p = [(K1[3 * i] * X1[0] + K1[3 * i + 1] * X1[1]) + K1[3 * i + 2] * X1[2] for i in range(3)]
        ju, jv = np.rint(p[0] / p[2]), np.rint(p[1] / p[2])
        inside = (X1[2] > 0.0) & (ju >= 0.0) & (ju <= float(w1 - 1)) & (jv >= 0.0) & (jv <= float(h1 - 1))
        iu, iv = np.where(inside, ju, 0.0).astype(np.int64), np.where(inside, jv, 0.0).astype(np.int64)
        ok = inside & (plane1[iv, iu] >= 0) & (np.abs(w1map[iv, iu] - 1.0 / X1[2]) <= tol)
    return (keep & ok).astype(np.uint8)


# ---- the cloud --------------------------------------------------------------------------------------------------------------------------
def to_world(cam, X0):
    cam = np.asarray(cam, np.float64).reshape(21)
    R, t = cam[9:18], cam[18:21]
    with np.errstate(all="ignore"):
        d = [X0[..., i] - t[i] for i in range(3)]
        return np.stack([(R[i] * d[0] + R[3 + i] * d[1]) + R[6 + i] * d[2] for i in range(3)], -1)


def cloud(keep, wmap, scoremap, img, cam):
    """(xyz [n, 3] float64, rgb [n, 3] uint8, normals [n, 3] float64, confidence [n] float32) of the kept pixels in row-major order."""
    keep = np.asarray(keep) != 0
    h, w = keep.shape
    cam = np.asarray(cam, np.float64).reshape(21)
    with np.errstate(all="ignore"):
        P = to_world(cam, backproject(cam[:9], h, w, np.where(keep, wmap, 1.0)))
        C0 = to_world(cam, np.zeros(3))

        def tangent(axis):
            lo, hi = np.zeros((h, w), bool), np.zeros((h, w), bool)
            L, H = P.copy(), P.copy()
            if axis == 1:
                lo[:, 1:], hi[:, :-1] = keep[:, :-1], keep[:, 1:]
                L[:, 1:][lo[:, 1:]] = P[:, :-1][lo[:, 1:]]
                H[:, :-1][hi[:, :-1]] = P[:, 1:][hi[:, :-1]]
            else:
                lo[1:], hi[:-1] = keep[:-1], keep[1:]
                L[1:][lo[1:]] = P[:-1][lo[1:]]
                H[:-1][hi[:-1]] = P[1:][hi[:-1]]
            return H - L, lo | hi

        Tu, hu = tangent(1)
        Tv, hv = tangent(0)
        nx = Tu[..., 1] * Tv[..., 2] - Tu[..., 2] * Tv[..., 1]
        ny = Tu[..., 2] * Tv[..., 0] - Tu[..., 0] * Tv[..., 2]
        nz = Tu[..., 0] * Tv[..., 1] - Tu[..., 1] * Tv[..., 0]
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        good = hu & hv & (length > 0.0) & (length <= DBL_MAX)
        safe = np.where(good, length, 1.0)
        n = np.stack([nx / safe, ny / safe, nz / safe], -1)
        dot = (n[..., 0] * (C0[0] - P[..., 0]) + n[..., 1] * (C0[1] - P[..., 1])) + n[..., 2] * (C0[2] - P[..., 2])
        n = np.where((dot < 0.0)[..., None], -n, n)
        n = np.where(good[..., None], n, 0.0)
    img = np.asarray(img)
    rgb = img if img.ndim == 3 else np.repeat(img[..., None], 3, -1)
    return P[keep], np.ascontiguousarray(rgb[keep]), n[keep], np.asarray(scoremap, np.float32)[keep]


# ---- the host side of the stage: matrices, schedule, images -------------------------------------------------------------------------------
def relative_pose(R0, t0, R1, t1):
    """(R, t) of X1 = R X0 + t from the two world-to-camera poses."""
    R0, R1 = np.asarray(R0, np.float64).reshape(3, 3), np.asarray(R1, np.float64).reshape(3, 3)
    R = R1 @ R0.T
    return R, np.asarray(t1, np.float64).reshape(3) - R @ np.asarray(t0, np.float64).reshape(3)


def sweep_matrices(K0, K1, R, t):
    """A = K1 R inv(K0), B = K1 t e3^T inv(K0), [9] each."""
    Ki = W.inv3(K0)
    K1 = np.asarray(K1, np.float64).reshape(3, 3)
    A = K1 @ np.asarray(R, np.float64).reshape(3, 3) @ Ki
    B = np.outer(K1 @ np.asarray(t, np.float64).reshape(3), Ki[2])
    return np.ascontiguousarray(A.reshape(9)), np.ascontiguousarray(B.reshape(9))


def grey(img):
    """(77 R + 150 G + 29 B + 128) >> 8 of an [h, w, 3] uint8 image; a grey image is returned as it is."""
    img = np.asarray(img)
    if img.ndim == 2:
        return img
    i = img.astype(np.int64)
    return ((77 * i[..., 0] + 150 * i[..., 1] + 29 * i[..., 2] + 128) >> 8).astype(np.uint8)


def downscale(img, f):
    """The integer mean (sum + f^2 // 2) // f^2 of f x f blocks, per channel; rows and columns beyond the last whole block are dropped."""
    img = np.asarray(img)
    if f == 1:
        return img
    h, w = img.shape[0] // f, img.shape[1] // f
    b = img[:h * f, :w * f].astype(np.int64).reshape((h, f, w, f) + img.shape[2:])
    return ((b.sum((1, 3)) + f * f // 2) // (f * f)).astype(np.uint8)


def downscale_K(K, f):
    """K of the downscaled image: pixel centre u of the small image lies at f u + (f - 1) / 2 of the large one."""
    K = np.array(K, np.float64).reshape(3, 3)
    if f == 1:
        return K
    S = np.array([[1.0 / f, 0.0, -(f - 1) / (2.0 * f)], [0.0, 1.0 / f, -(f - 1) / (2.0 * f)], [0.0, 0.0, 1.0]])
    return S @ K
