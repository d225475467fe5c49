"""The numpy restatement of the fusion of the two depth maps (csrc/fuse_pixel.h): the link of a kept pixel of the base view a
to a kept pixel of view b, view b's measurement carried onto the pixel's own ray, the fused inverse depth and score with the number of
views, the pixels of view b the cloud still lacks, and the cloud of both. A definition of this project's own: Metashape's merge of its
depth maps is closed and is not reproduced; parity with Metashape is unpinned by construction. float64 element by element in the
association of the header (numpy never contracts); every pixel is decided from the inputs alone, and the claims are applied one after
another, so the kernels equal this bit for bit whatever order their threads run in."""
import numpy as np

import dense_oracle as O

MAX_SIDE = 16384
DBL_MAX = 1.7976931348623157e308


def split(pose):
    pose = np.asarray(pose, np.float64).reshape(30)
    return pose[:9], pose[9:18], pose[18:21], pose[21:]


def invert_pose(Ka, Kb, R, t):
    """(pose a -> b, pose b -> a) [30] each = inv(K of the source), R, t, K of the target, from Xb = R Xa + t."""
    Ka, Kb, R, t = (np.asarray(x, np.float64) for x in (Ka, Kb, R, t))
    R = R.reshape(3, 3)
    Ri = R.T
    ti = -(Ri @ t.reshape(3))
    ab = np.concatenate([O.W.inv3(Ka.reshape(3, 3)).reshape(9), R.reshape(9), t.reshape(3), Kb.reshape(9)])
    ba = np.concatenate([O.W.inv3(Kb.reshape(3, 3)).reshape(9), np.ascontiguousarray(Ri).reshape(9), ti, Ka.reshape(9)])
    return ab, ba


def target(w_a, pose, hb, wb):
    """Per pixel of view a (inverse depths w_a [ha, wa]): (inside bool, iu, iv int64, 1 / Xb.z): whether the pixel's point lies in front of
    view b and its nearest pixel inside it, that pixel (0 where not), and the inverse depth the point has there."""
    w_a = np.asarray(w_a, np.float64)
    Ki, R, t, K1 = split(pose)
    ha, wa = w_a.shape
    with np.errstate(all="ignore"):
        Xa = O.backproject(Ki, ha, wa, w_a)
        Xb = [((R[3 * i] * Xa[..., 0] + R[3 * i + 1] * Xa[..., 1]) + R[3 * i + 2] * Xa[..., 2]) + t[i] for i in range(3)]
        p = [(K1[3 * i] * Xb[0] + K1[3 * i + 1] * Xb[1]) + K1[3 * i + 2] * Xb[2] for i in range(3)]
        ju, jv = np.rint(p[0] / p[2]), np.rint(p[1] / p[2])
        inside = (Xb[2] > 0.0) & (ju >= 0.0) & (ju <= float(wb - 1)) & (jv >= 0.0) & (jv <= float(hb - 1))
        iu, iv = np.where(inside, ju, 0.0).astype(np.int64), np.where(inside, jv, 0.0).astype(np.int64)
        return inside, iu, iv, 1.0 / Xb[2]


def link(keep_a, w_a, keep_b, w_b, pose, tol):
    """int32 [ha, wa]: the linear index of the kept pixel of view b that each kept pixel of view a links to, -1 where there is none."""
    keep_a, keep_b = np.asarray(keep_a) != 0, np.asarray(keep_b) != 0
    w_b = np.asarray(w_b, np.float64)
    hb, wb = keep_b.shape
    inside, iu, iv, wz = target(w_a, pose, hb, wb)
    with np.errstate(all="ignore"):
        ok = keep_a & inside & keep_b[iv, iu] & (np.abs(w_b[iv, iu] - wz) <= tol)
    return np.where(ok, iv * wb + iu, -1).astype(np.int32)


def second(pose, ha, wa, wb_j):
    """(w' [ha, wa], usable [ha, wa]): view b's measurement wb_j (per pixel of view a, an inverse depth of view b) on the pixel's own ray."""
    Ki, R, t, _ = split(pose)
    u = np.arange(wa, dtype=np.float64)[None, :] + np.zeros((ha, 1))
    v = np.arange(ha, dtype=np.float64)[:, None] + np.zeros((1, wa))
    with np.errstate(all="ignore"):
        d = [(Ki[3 * i] * u + Ki[3 * i + 1] * v) + Ki[3 * i + 2] for i in range(3)]
        g = (R[6] * d[0] + R[7] * d[1]) + R[8] * d[2]
        w2 = g / (1.0 / np.asarray(wb_j, np.float64) - t[2])
        return w2, (w2 > 0.0) & (w2 <= DBL_MAX)


def fuse(keep_a, w_a, score_a, keep_b, w_b, score_b, pose, tol):
    """(link int32, w_out float64, score_out float32, views uint8) [ha, wa] and claimed uint8 [hb, wb]."""
    if not tol >= 0.0:
        raise ValueError("fuse: the tolerance must not be negative")
    keep = np.asarray(keep_a) != 0
    w_a, w_b = np.asarray(w_a, np.float64), np.asarray(w_b, np.float64)
    score_a, score_b = np.asarray(score_a, np.float32), np.asarray(score_b, np.float32)
    ha, wa = keep.shape
    lk = link(keep_a, w_a, keep_b, w_b, pose, tol)
    linked = lk >= 0
    j = np.where(linked, lk, 0)
    w2, usable = second(pose, ha, wa, np.where(linked, w_b.reshape(-1)[j], 1.0))
    sb = score_b.reshape(-1)[j]
    with np.errstate(all="ignore"):
        a = np.where(score_a.astype(np.float64) > 0.0, score_a.astype(np.float64), 0.0)
        b = np.where(sb.astype(np.float64) > 0.0, sb.astype(np.float64), 0.0)
        both = np.where(a + b > 0.0, (a * w_a + b * w2) / (a + b), 0.5 * (w_a + w2))
    use = linked & usable
    w_out = np.where(keep, np.where(use, both, w_a), 0.0)
    score_out = np.where(keep, np.where(use, np.where(sb > score_a, sb, score_a), score_a), np.float32(0.0)).astype(np.float32)
    views = np.where(keep, np.where(linked, 2, 1), 0).astype(np.uint8)
    claimed = np.zeros(np.asarray(keep_b).shape, np.uint8)
    flat = claimed.reshape(-1)
    for target in lk[linked]:                                  # one claim after another; a target claimed twice is claimed
        flat[target] = 1
    return lk, w_out, score_out, views, claimed


def rest(keep_b, w_b, keep_a, w_a, pose_ba, tol_a, claimed):
    """uint8 [hb, wb]: kept, unclaimed, and without a link of its own into view a."""
    if not tol_a >= 0.0:
        raise ValueError("rest: the tolerance must not be negative")
    back = link(keep_b, w_b, keep_a, w_a, pose_ba, tol_a)
    return ((np.asarray(keep_b) != 0) & (np.asarray(claimed) == 0) & (back < 0)).astype(np.uint8)


def fused_cloud(keep_a, map_a, img_a, cam_a, keep_b, map_b, img_b, cam_b, pose_ab, pose_ba, tol_b, tol_a, min_views=1):
    """(xyz, rgb, normals, confidence, views uint8) of the fused cloud: the base view's pixels with views >= min_views out of the fused map
    first, then (min_views == 1) the rest of view b out of its own map; maps = (w, score), cams [21] as `dense_oracle.cloud` takes them."""
    _, w_out, score_out, views, claimed = fuse(keep_a, map_a[0], map_a[1], keep_b, map_b[0], map_b[1], pose_ab, tol_b)
    mask = (views >= min_views).astype(np.uint8)
    parts = [O.cloud(mask, w_out, score_out, img_a, cam_a) + (views[mask != 0],)]
    if min_views == 1:
        r = rest(keep_b, map_b[0], keep_a, map_a[0], pose_ba, tol_a, claimed)
        parts.append(O.cloud(r, map_b[0], map_b[1], img_b, cam_b) + (np.ones(int(r.sum()), np.uint8),))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(5))
