"""Row f-4 of the scope table: the first SfM consumers of the matches - relative orientation of the stereo pair and
linear triangulation (`src/icepy4d/sfm/geometry.py:31-76`, `sfm/two_view_geometry.py:38-110`,
`sfm/triangulation.py:153-186`). The reference uses OpenCV (`findEssentialMat`, `recoverPose`), which is absent here, so
parity of `estimate_pose` is unpinned (same interface, same conventions, checked on synthetic geometry); the linear
triangulation is pure numpy in the reference: host and device path here solve the reference's own system and are compared with the
reference's OUTPUTS (tests/golden/g10_triangulation.npz, written by importing the reference module; oracle/sfm_cpu.py restates it). Small host-side linear algebra on S <= 1e4 matched points: not a device workload; the RANSAC inside
`estimate_pose(engine=...)` generates and scores essential-matrix hypotheses on the device (`im_ransac_essential`, csrc/geometry.hip)
and `triangulate_points_linear(engine=...)` triangulates on the device (`im_triangulate_linear`); the cheirality test and the 5-7
match case (five-point solver on every 5-subset) stay host numpy: one 3 x 3 matrix.
The reference's classes on top (`RelativeOrientation`, `Triangulate`) and what `Triangulate.triangulate_two_views` runs by default -
`undistort_points`, `iterative_LS_triangulation`, point colours - are at the end of the module: per-point float64 kernels (csrc/sfm.hip),
for flat arrays of matched points and for every record of a gathered match table at once (`triangulate_table`)."""
import logging
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from .core.camera import _camera_params, _channel_map
from ._lib import ptr
from .engine import default_engine, to_device
from .matching.enums import GeometricVerification
from .matching.geometric_verification import geometric_verification

logger = logging.getLogger(__name__)


def _lift(P, ip) -> np.ndarray:
    """The reference's system for one point seen in n views (`triangulation.py:176-183`): unknowns X (4) and one depth per view,
    rows  P_i X - lambda_i x_i = 0  (3 n x (4 + n)); batched over leading dimensions of `ip`."""
    n = len(P)
    ip = [np.asarray(x, dtype=np.float64) for x in ip]
    lead = ip[0].shape[:-1]
    M = np.zeros(lead + (3 * n, 4 + n))
    for i in range(n):
        M[..., 3 * i:3 * i + 3, :4] = np.asarray(P[i], dtype=np.float64)
        M[..., 3 * i:3 * i + 3, 4 + i] = -ip[i]
    return M


def triangulate_nviews(P, ip) -> np.ndarray:
    """One point seen in n views (`triangulation.py:166-186`): P list of 3x4 projection matrices, ip list of homogeneous
    image points [x, y, 1]. Returns the homogeneous point normalised to X[3] = 1: the right singular vector of the smallest
    singular value of the reference's system (`_lift`), equal to the reference's result to the rounding of the SVD."""
    if len(ip) != len(P):
        raise ValueError("Number of points and number of cameras not equal.")
    X = np.linalg.svd(_lift(P, ip))[2][-1, :4]
    return X / X[3]


def triangulate_points_linear(P1, P2, x1, x2, engine=None) -> np.ndarray:
    """Two-view triangulation of n points (`triangulation.py:153-163`); x1, x2 are [n, 3] homogeneous image points. The reference's
    system per point (6 x 6: the point and one depth per view), solved for all points by ONE batched SVD instead of the reference's Python
    loop; with `engine=` on the device (`im_triangulate_linear`: one thread per point, one-sided Jacobi SVD in fp64). Both equal the reference's
    outputs (tests/golden/g10_triangulation.npz) to 1e-9 relative. Until round 5 both solved the four cross-product rows  x (P X) = 0
    instead - the same point on exact correspondences, a different least-squares problem on noisy ones (up to 5e-3 relative on 0.4 px noise)."""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    if len(x1) != len(x2):
        raise ValueError("Number of points don't match.")
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    if engine is not None:
        n = len(x1)
        d1, d2 = to_device(x1, engine.device), to_device(x2, engine.device)
        dX = torch.empty((n, 4), dtype=torch.float64, device=engine.device)
        p1, p2 = np.ascontiguousarray(P1.reshape(12)), np.ascontiguousarray(P2.reshape(12))
        engine.ctx.call("im_triangulate_linear", p1.ctypes.data, p2.ctypes.data, ptr(d1), ptr(d2), n, ptr(dX), engine.stream_ptr())
        return dX.cpu().numpy()
    if len(x1) == 0:
        return np.zeros((0, 4))
    X = np.linalg.svd(_lift([P1, P2], [x1, x2]))[2][:, -1, :4]
    return X / X[:, 3:4]


# ---- five-point relative pose (what cv2.findEssentialMat runs on a minimal sample; restated from the published algorithm:
# D. Nister, "An efficient solution to the five-point relative pose problem", PAMI 2004, in the action-matrix form of
# H. Stewenius, C. Engels, D. Nister, "Recent developments on direct relative orientation", ISPRS J. 2006)
_MONO = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
         (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_DEG = {d: [m for m in _MONO if sum(m) <= d] for d in (1, 2, 3)}


def _pmul(a: np.ndarray, da: int, b: np.ndarray, db: int) -> np.ndarray:
    """Product of two polynomials in (x, y, z) given as coefficient arrays [..., 4, 4, 4] (exponent of x, y, z) of total degree
    da, db (da + db <= 3); leading batch dimensions broadcast."""
    out = np.zeros(np.broadcast_shapes(a.shape, b.shape))
    for ma in _DEG[da]:
        ca = a[..., ma[0], ma[1], ma[2]]
        for mb in _DEG[db]:
            out[..., ma[0] + mb[0], ma[1] + mb[1], ma[2] + mb[2]] += ca * b[..., mb[0], mb[1], mb[2]]
    return out


def essential_five_point(x0: np.ndarray, x1: np.ndarray) -> np.ndarray:
    """All real essential matrices (up to 10) consistent with FIVE correspondences in normalised image coordinates
    (x1^T E x0 = 0): [m, 3, 3], each scaled to unit Frobenius norm; m = 0 for a degenerate sample."""
    x0, x1 = np.asarray(x0, np.float64), np.asarray(x1, np.float64)
    assert x0.shape == (5, 2) and x1.shape == (5, 2)
    h0, h1 = np.c_[x0, np.ones(5)], np.c_[x1, np.ones(5)]
    A = np.einsum("ni,nj->nij", h1, h0).reshape(5, 9)
    nullv = np.linalg.svd(A)[2][5:]                                   # E = x E1 + y E2 + z E3 + E4
    Eb = nullv.reshape(4, 3, 3)
    E = np.zeros((3, 3, 4, 4, 4))                                     # entries of E as linear polynomials
    for k, m in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))):
        E[:, :, m[0], m[1], m[2]] = Eb[k]
    # det(E) = 0
    def minor(r0, c0, r1, c1):
        return _pmul(E[r0, c0], 1, E[r1, c1], 1)
    det = (_pmul(E[0, 0], 1, minor(1, 1, 2, 2) - minor(1, 2, 2, 1), 2) - _pmul(E[0, 1], 1, minor(1, 0, 2, 2) - minor(1, 2, 2, 0), 2)
           + _pmul(E[0, 2], 1, minor(1, 0, 2, 1) - minor(1, 1, 2, 0), 2))
    # 2 E E^T E - trace(E E^T) E = 0
    EEt = np.zeros((3, 3, 4, 4, 4))
    for i in range(3):
        for j in range(3):
            EEt[i, j] = sum(_pmul(E[i, k], 1, E[j, k], 1) for k in range(3))
    tr = EEt[0, 0] + EEt[1, 1] + EEt[2, 2]
    eqs = [det]
    for i in range(3):
        for j in range(3):
            eqs.append(2.0 * sum(_pmul(EEt[i, k], 2, E[k, j], 1) for k in range(3)) - _pmul(tr, 2, E[i, j], 1))
    M = np.array([[e[m[0], m[1], m[2]] for m in _MONO] for e in eqs])         # 10 x 20
    try:
        B = np.linalg.solve(M[:, :10], M[:, 10:])                             # cubic monomials in terms of the lower ones
    except np.linalg.LinAlgError:
        return np.zeros((0, 3, 3))
    # action matrix of multiplication by x on the basis [x^2, xy, xz, y^2, yz, z^2, x, y, z, 1]
    At = np.zeros((10, 10))
    At[0:6] = -B[[0, 1, 2, 3, 4, 5]]              # x * {x^2, xy, xz, y^2, yz, z^2} = {x^3, x^2 y, x^2 z, x y^2, xyz, x z^2}
    At[6, 0] = At[7, 1] = At[8, 2] = At[9, 6] = 1.0    # x * {x, y, z, 1} = {x^2, xy, xz, x}
    w, V = np.linalg.eig(At)                       # x * b(solution) = At b(solution): the monomial vector is an eigenvector
    out = []
    for k in range(10):
        if abs(w[k].imag) > 1e-9 * max(1.0, abs(w[k])) or abs(V[9, k]) < 1e-14:
            continue
        v = (V[:, k] / V[9, k]).real
        Em = v[6] * Eb[0] + v[7] * Eb[1] + v[8] * Eb[2] + Eb[3]
        nrm = np.linalg.norm(Em)
        if np.isfinite(nrm) and nrm > 0:
            out.append(Em / nrm)
    return np.array(out).reshape(-1, 3, 3)


def _sampson_e(E: np.ndarray, x0: np.ndarray, x1: np.ndarray) -> np.ndarray:
    h0, h1 = np.c_[x0, np.ones(len(x0))], np.c_[x1, np.ones(len(x1))]
    Ex0, Etx1 = h0 @ E.T, h1 @ E
    return (h1 * Ex0).sum(1) ** 2 / np.maximum(Ex0[:, 0] ** 2 + Ex0[:, 1] ** 2 + Etx1[:, 0] ** 2 + Etx1[:, 1] ** 2, 1e-24)


def _estimate_pose_few(x0: np.ndarray, x1: np.ndarray, thr2: float):
    """5 <= n < 8 matches: every 5-subset through the five-point solver, the candidate with most inliers (then the smallest
    Sampson error sum, then the most points in front of both cameras) wins - what a RANSAC over minimal samples converges to."""
    from itertools import combinations
    best = None
    for idx in combinations(range(len(x0)), 5):
        for E in essential_five_point(x0[list(idx)], x1[list(idx)]):
            err = _sampson_e(E, x0, x1)
            mask = err < thr2
            n_front, R, t, front = _recover_pose(E, x0, x1, mask)
            key = (int(mask.sum()), n_front, -float(err[mask].sum()))
            if R is not None and (best is None or key > best[0]):
                inl = mask.copy()
                inl[np.flatnonzero(mask)[~front]] = False
                best = (key, R, t, inl)
    return None if best is None else best[1:]


def _essential_from_fundamental(F: np.ndarray) -> np.ndarray:
    u, _, vt = np.linalg.svd(F)
    return u @ np.diag([1.0, 1.0, 0.0]) @ vt


def _essential_ransac_on_device(engine, x0: np.ndarray, x1: np.ndarray, threshold: float, confidence: float, seed: int,
                                max_iters: int = 10000):
    """RANSAC over essential-matrix hypotheses generated and scored on the device (`im_ransac_essential`), in batches of 1024
    until the confidence criterion holds for the best inlier ratio; then one refit on the inliers of the winner (8-point on all
    of them, projected onto the essential manifold) that is kept if it does not lose inliers. Returns (E, inlier mask)."""
    from .matching.geometric_verification import DEVICE_BATCH, _eight_point, _needed, _sampson
    dev = engine.device
    d0, d1 = to_device(x0, dev, np.float32), to_device(x1, dev, np.float32)
    n = len(x0)
    dE = torch.empty(9, dtype=torch.float64, device=dev)
    dmask = torch.empty(n, dtype=torch.uint8, device=dev)
    dinfo = torch.empty(2, dtype=torch.int32, device=dev)
    best = (0, None, None)
    done, needed = 0, int(max_iters)
    while done < min(needed, int(max_iters)):
        engine.ctx.call("im_ransac_essential", ptr(d0), ptr(d1), n, DEVICE_BATCH, float(threshold), (int(seed) + done) & 0xFFFFFFFF,
                        ptr(dE), ptr(dmask), ptr(dinfo), engine.stream_ptr())
        done += DEVICE_BATCH
        cnt = int(dinfo[0].item())
        if cnt > best[0]:
            best = (cnt, dE.cpu().numpy().reshape(3, 3).copy(), dmask.cpu().numpy().astype(bool))
        needed = _needed(confidence, best[0] / n)
    if best[1] is None:
        return None, np.zeros(n, bool)
    cnt, E, mask = best
    if cnt >= 8:
        E2 = _essential_from_fundamental(_eight_point(x0[mask], x1[mask]))
        m2 = _sampson(E2, x0, x1) < threshold ** 2
        if int(m2.sum()) >= cnt:
            E, mask = E2 / np.linalg.norm(E2), m2
    return E, mask


def _recover_pose(E: np.ndarray, x0: np.ndarray, x1: np.ndarray, mask: np.ndarray):
    """The (R, t) of the four decompositions of E that puts most inliers in front of both cameras (what
    cv2.recoverPose does); x0, x1 are normalised image coordinates [n, 2]."""
    u, _, vt = np.linalg.svd(E)
    if np.linalg.det(u) < 0:
        u = -u
    if np.linalg.det(vt) < 0:
        vt = -vt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    h0 = np.c_[x0[mask], np.ones(int(mask.sum()))]
    h1 = np.c_[x1[mask], np.ones(int(mask.sum()))]
    P0 = np.eye(3, 4)
    best = (-1, None, None, None)
    for R in (u @ W @ vt, u @ W.T @ vt):
        for t in (u[:, 2], -u[:, 2]):
            P1 = np.c_[R, t]
            X = triangulate_points_linear(P0, P1, h0, h1)[:, :3]
            front = (X[:, 2] > 0) & ((X @ R.T + t)[:, 2] > 0)
            if int(front.sum()) > best[0]:
                best = (int(front.sum()), R, t, front)
    return best


def estimate_pose(kpts0: np.ndarray, kpts1: np.ndarray, K0: np.ndarray, K1: np.ndarray, thresh: float, conf: float = 0.9999,
                  engine=None, seed: int = 0, hypothesis_fn=None) -> Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """`estimate_pose` of the reference (`sfm/geometry.py:31-76`): (R [3,3], t [3], inliers [n] bool) with
    x_cam1 = R x_cam0 + t, t up to scale; None with fewer than 5 matches. The reference runs cv2.findEssentialMat (5-point
    RANSAC) + cv2.recoverPose; here, with 8 or more matches, the epipolar geometry of the NORMALISED coordinates is estimated by
    an 8-point RANSAC whose hypotheses are projected onto the essential manifold and scored ON THE DEVICE (`engine=...`:
    `im_ransac_essential`; with a `hypothesis_fn` test seam instead: the F-matrix RANSAC of `geometric_verification`, projected
    afterwards) and decomposed with the cheirality test; with 5-7 matches the five-point solver (`essential_five_point`) runs on every
    5-subset."""
    if len(kpts0) < 5:
        return None
    K0, K1 = np.asarray(K0, np.float64), np.asarray(K1, np.float64)
    f_mean = np.mean([K0[0, 0], K1[1, 1], K0[0, 0], K1[1, 1]])      # the reference's (sic) focal average, `geometry.py:60`
    norm_thresh = thresh / f_mean
    x0 = (np.asarray(kpts0, np.float64) - K0[[0, 1], [2, 2]][None]) / K0[[0, 1], [0, 1]][None]
    x1 = (np.asarray(kpts1, np.float64) - K1[[0, 1], [2, 2]][None]) / K1[[0, 1], [0, 1]][None]
    if len(x0) < 8:
        # fewer matches than the 8-point hypotheses of the RANSAC below need: the five-point solver on every 5-subset
        return _estimate_pose_few(x0, x1, norm_thresh ** 2)
    if engine is not None and hypothesis_fn is None:
        # device path: essential-matrix hypotheses (8-point, projected onto the essential manifold) generated and scored on the GPU
        E, mask = _essential_ransac_on_device(engine, x0, x1, norm_thresh, conf, seed)
        if E is None:
            raise AssertionError("Unable to estimate Essential matrix")
    else:
        F, mask = geometric_verification(x0.astype(np.float32), x1.astype(np.float32), GeometricVerification.PYDEGENSAC,
                                         threshold=norm_thresh, confidence=conf, seed=seed, engine=engine, hypothesis_fn=hypothesis_fn)
        if F is None:
            raise AssertionError("Unable to estimate Essential matrix")
        E = _essential_from_fundamental(F)
    n_front, R, t, front = _recover_pose(E, x0, x1, mask)
    inliers = mask.copy()
    inliers[np.flatnonzero(mask)[~front]] = False
    return R, t, inliers


# ---- projection and point colours (`sfm/geometry.py:79-100`, `sfm/interpolate_colors.py:13-92`): csrc/dsm.hip `im_project_colors`
def _points(points3d) -> np.ndarray:
    p = np.ascontiguousarray(points3d, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"expected an Nx3 array of points (got shape {p.shape})")
    return p


def _project_colors(engine, points: np.ndarray, cam: np.ndarray, image=None, chmap=None, want_proj=True):
    proj, col = _project_colors_device(engine, to_device(points, engine.device), cam, image, chmap, want_proj)
    return (None if proj is None else proj.cpu().numpy()), (None if col is None else col.cpu().numpy())


def _project_colors_device(engine, dp, cam: np.ndarray, image=None, chmap=None, want_proj=True):
    """`im_project_colors` on [n, 3] float64 points that are on the device already (`Triangulate`, `triangulate_table`: the points never
    visit the host between the triangulation and the colouring); `image` a host uint8 array or a device tensor. Device tensors out."""
    dev = engine.device
    n = len(dp)
    proj = torch.empty((n, 2), dtype=torch.float32, device=dev) if want_proj else None
    col = img = None
    h = w = cin = cout = 0
    if image is not None:
        h, w, cin = image.shape
        cout = len(chmap)
        img = image if torch.is_tensor(image) else to_device(image, dev)
        col = torch.empty((n, cout), dtype=torch.float64, device=dev)
    base = ptr(dp)
    engine.ctx.call("im_project_colors", base, 0, 3, base + 8, 0, 3, base + 16, 0, 3, 1 if n else 0, n, 0, cam.ctypes.data,
                    ptr(img), h, w, cin, None if chmap is None else chmap.ctypes.data, cout, ptr(proj), ptr(col), None, engine.stream_ptr())
    return proj, col


def project_points(points3d, camera, engine=None) -> np.ndarray:
    """`project_points` of the reference (`sfm/geometry.py:79-100`): [n, 2] float32 image coordinates of [n, 3] world points. The
    reference calls cv2.projectPoints; here it is restated elementwise in float64 on the device (R X + t, the perspective divide, Brown
    k1 k2 p1 p2 [k3 [k4 k5 k6]] rational distortion, fx x + cx) and cast to float32. R is used as given (no Rodrigues round trip)."""
    cam = _camera_params(camera)
    p = _points(points3d)
    return _project_colors(default_engine(engine), p, cam)[0]


def interpolate_point_colors(points3d, image, camera, convert_BRG2RGB=True, engine=None) -> np.ndarray:
    """`interpolate_point_colors` of the reference (`sfm/interpolate_colors.py:13-51`): [n, channels] float64 colours in [0, 1] of
    [n, 3] world points, sampled bilinearly (`bilinear_interpolate`: clipped corners, weights from the unclipped position) from a uint8
    image after `float32(v) / 255`; BGR is reversed to RGB first unless `convert_BRG2RGB=False`. Projection and sampling in one launch."""
    assert image.ndim == 3, "invalid input image. Image has not 3 channel"
    image = np.asarray(image)
    if image.dtype != np.uint8:
        raise ValueError(f"interpolate_point_colors: a uint8 image is expected (got {image.dtype})")
    chmap = _channel_map(image, convert_BRG2RGB)
    cam = _camera_params(camera)
    p = _points(points3d)
    return _project_colors(default_engine(engine), p, cam, image, chmap, want_proj=False)[1]


# ---- undistortion and least-squares triangulation of matched points (`sfm/geometry.py:103-118`, `thirdparty/triangulation.py:10-177`,
# `sfm/triangulation.py:42-148`, `sfm/two_view_geometry.py:38-197`): csrc/sfm.hip. No host fallback: `default_engine(engine)`.
DEFAULT_TOLERANCE = 3.0e-5      # depth convergence tolerance of `iterative_LS_triangulation`, absolute
MAX_SOLVES = 10                 # "Hartley suggests 10 iterations at most"


def _intrinsics(camera) -> np.ndarray:
    """[12] float64 for the kernels of csrc/sfm.hip: fx, fy, cx, cy, k1 k2 p1 p2 k3 k4 k5 k6. Reads only `.K` and `.dist`; distortion
    vectors of length 0, 4, 5 or 8, like `_camera_params`."""
    K = np.asarray(camera.K, np.float64).reshape(3, 3)
    dist = np.zeros(0) if camera.dist is None else np.asarray(camera.dist, np.float64).ravel()
    if len(dist) not in (0, 4, 5, 8):
        raise ValueError(f"undistort_points: distortion vectors of length 0, 4, 5 or 8 are supported (got {len(dist)})")
    if not (np.isfinite(K[0, 0]) and np.isfinite(K[1, 1]) and K[0, 0] != 0 and K[1, 1] != 0):
        raise ValueError("undistort_points: the focal lengths of K must be finite and non-zero")
    k = np.zeros(8)
    k[:len(dist)] = dist
    return np.ascontiguousarray(np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], k]))


def _projection(camera_or_P) -> np.ndarray:
    """[12] float64, row-major 3 x 4: a matrix as given (the upper 3 x 4 of a 4 x 4 one), `.P` of a camera, or K [R | t]."""
    P = camera_or_P
    if not isinstance(P, np.ndarray):
        P = P.P if hasattr(P, "P") else np.asarray(P.K, np.float64).reshape(3, 3) @ np.c_[np.asarray(P.R, np.float64).reshape(3, 3),
                                                                                          np.asarray(P.t, np.float64).reshape(3, 1)]
    P = np.asarray(P, np.float64)
    if P.ndim != 2 or P.shape[0] < 3 or P.shape[1] != 4:
        raise ValueError(f"expected a 3x4 projection matrix (got shape {P.shape})")
    return np.ascontiguousarray(P[0:3, 0:4]).reshape(12)


def _image_points(pts, dtype=np.float32) -> np.ndarray:
    p = np.ascontiguousarray(pts, dtype=dtype)
    if p.ndim == 3 and p.shape[1] == 1:          # cv2's [n, 1, 2] layout
        p = p[:, 0, :]
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"expected an Nx2 array of image points (got shape {p.shape})")
    return np.ascontiguousarray(p)


def undistort_points(pts, camera, engine=None) -> np.ndarray:
    """`undistort_points` of the reference (`sfm/geometry.py:103-118`): [n, 2] float32 image points with the lens distortion removed,
    in pixels of the same K. The reference calls cv2.undistortPoints(pts, K, dist, None, K); here its default path is restated in
    float64 on the device (`im_undistort_points`): x0 = (u - cx) / fx, FIVE fixed-point iterations of the Brown / rational model
    (OpenCV's default criteria; its icdist < 0 guard falls back to the distorted point), fx x + cx, cast to float32. Five iterations
    leave about 1e-6 px of the inverse undone on a 24 MP frame: that is the reference's result, not an error of this port."""
    cam = _intrinsics(camera)
    p = _image_points(pts)
    eng = default_engine(engine)
    d = to_device(p, eng.device)
    out = torch.empty_like(d)
    eng.ctx.call("im_undistort_points", ptr(d), len(p), cam.ctypes.data, ptr(out), eng.stream_ptr())
    return out.cpu().numpy()


def undistort_image(image, camera, out_path=None, engine=None):
    """`undistort_image` of the reference (`sfm/geometry.py:121-143`): a uint8 H x W [x C] image (numpy array or device tensor) with the
    lens distortion removed, in pixels of the same K; returns the same kind. The reference calls cv2.undistort(image, K, dist, None, K);
    here its 8-bit bilinear path is restated on the device (`im_undistort_image`, csrc/warp.hip; `utils/homography.py`): bit-identical
    with tests/warp_oracle.py, parity with an OpenCV binary not pinned. `out_path` writes through PIL, channels as given."""
    from .utils.homography import undistort_image as impl
    return impl(image, camera, out_path=out_path, engine=engine)


def _triangulate_device(eng, u1, u2, P1, P2, cam1=None, cam2=None, tolerance=DEFAULT_TOLERANCE, max_solves=MAX_SOLVES, want_und=False):
    """`im_triangulate_iterative` on host point arrays: device tensors (X [n, 3] float64, status [n] int32, und1, und2 [n, 2] float32 or None)."""
    f64 = cam1 is None and (np.asarray(u1).dtype == np.float64 or np.asarray(u2).dtype == np.float64)
    u1, u2 = _image_points(u1, np.float64 if f64 else np.float32), _image_points(u2, np.float64 if f64 else np.float32)
    if len(u1) != len(u2):
        raise ValueError("Number of points don't match.")
    if not (float(tolerance) >= 0.0):
        raise ValueError(f"the tolerance must be >= 0 (got {tolerance})")
    n, dev = len(u1), eng.device
    d1, d2 = to_device(u1, dev), to_device(u2, dev)
    dX = torch.empty((n, 3), dtype=torch.float64, device=dev)
    dst = torch.empty(n, dtype=torch.int32, device=dev)
    und1 = torch.empty((n, 2), dtype=torch.float32, device=dev) if want_und else None
    und2 = torch.empty((n, 2), dtype=torch.float32, device=dev) if want_und else None
    eng.ctx.call("im_triangulate_iterative", ptr(d1), ptr(d2), int(f64), n, P1.ctypes.data, P2.ctypes.data,
                 None if cam1 is None else cam1.ctypes.data, None if cam2 is None else cam2.ctypes.data, float(tolerance), int(max_solves),
                 ptr(dX), ptr(dst), ptr(und1), ptr(und2), eng.stream_ptr())
    return dX, dst, und1, und2


def iterative_LS_triangulation(u1, P1, u2, P2, tolerance=DEFAULT_TOLERANCE, engine=None) -> Tuple[np.ndarray, np.ndarray]:
    """`iterative_LS_triangulation` of the reference (`thirdparty/triangulation.py:79-177`; Hartley & Sturm 1997): (points [n, 3] float64,
    status [n] int64) from image points u1, u2 [n, 2] (pixels of P1, P2: float32 as `undistort_points` returns them, or float64) on the
    device (`im_triangulate_iterative`), one thread per point. The reference's recurrence, quirks included: the rows of the 4 x 3 system
    are re-weighted by 1 / depth CUMULATIVELY (the weights of all earlier solves stay on them), the stop test is |d_new - d| <= tolerance
    on both depths in absolute terms (d = 1 before the first solve), ten solves at most. Each solve is `cv2.solve(DECOMP_SVD)`'s
    definition, x = V S^+ U^T b with singular values <= 2 DBL_EPSILON * their sum treated as zero, by one-sided Jacobi.
    Status: 1 in front of both cameras, -1 only in front of the second, -2 only in front of the first, -3 behind both. The reference
    documents 0 for "not converged, in front of both", but its loop index never reaches 10, so the ten-solve exit is not flagged: a
    point that used all ten solves has status 1 like one that converged (0 only appears for a NaN depth). Kept as it is."""
    eng = default_engine(engine)
    dX, dst, _, _ = _triangulate_device(eng, u1, u2, _projection(np.asarray(P1)), _projection(np.asarray(P2)), tolerance=tolerance)
    return dX.cpu().numpy(), dst.cpu().numpy().astype(np.int64)


def linear_LS_triangulation(u1, P1, u2, P2, engine=None) -> Tuple[np.ndarray, np.ndarray]:
    """`linear_LS_triangulation` of the reference (`thirdparty/triangulation.py:10-76`): the first solve of the iterative form (the same
    kernel with one solve); (points [n, 3] float64, status [n] bool, all True)."""
    eng = default_engine(engine)
    dX, _, _, _ = _triangulate_device(eng, u1, u2, _projection(np.asarray(P1)), _projection(np.asarray(P2)), max_solves=1)
    X = dX.cpu().numpy()
    return X, np.ones(len(X), dtype=bool)


class Triangulate:
    """`Triangulate` of the reference (`sfm/triangulation.py:42-148`): cameras = list of camera objects (`.K .dist .R .t`, and `.P` or it is
    formed as K [R | t]), image_points = list of [n, 2] arrays of matched image points, one per camera. Results in `points3d` / `colors`
    (and `status`, the per-point status of the iterative triangulation)."""

    def __init__(self, cameras=None, image_points=None, engine=None) -> None:
        self.cameras = cameras
        self.image_points = image_points
        self.engine = engine
        self.points3d = None
        self.colors = None
        self.status = None

    def triangulate_two_views(self, views_ids=(0, 1), approach: str = "iterative_LS_triangulation", compute_colors: bool = False,
                              image: np.ndarray = None, cam_id: int = 0) -> np.ndarray:
        """[n, 3] float64 points of the two views. "iterative_LS_triangulation" (default): undistortion of both point sets and the
        iterative triangulation in ONE launch, and with `compute_colors` the colours of `image` seen by `cameras[cam_id]` in a second one
        that reads the points on the device. "linear_triangulation": `triangulate_points_linear` on the undistorted points (as in the
        reference this branch computes no colours). Any other approach leaves `points3d` as it was, like the reference."""
        i0, i1 = views_ids[0], views_ids[1]
        c0, c1 = self.cameras[i0], self.cameras[i1]
        if approach == "iterative_LS_triangulation":
            if compute_colors:
                assert image is not None and type(image) == np.ndarray, "Invalid input image for interpolating point colors"
            eng = default_engine(self.engine)
            dX, dst, _, _ = _triangulate_device(eng, self.image_points[i0], self.image_points[i1], _projection(c0), _projection(c1),
                                                _intrinsics(c0), _intrinsics(c1))
            self.points3d = dX.cpu().numpy()
            self.status = dst.cpu().numpy().astype(np.int64)
            logger.info("Point triangulation succeded: %s.", self.status.sum() / max(self.status.size, 1))
            if compute_colors:
                self.colors = _colors_of_device_points(eng, dX, image, self.cameras[cam_id], True)
            return self.points3d
        if approach == "linear_triangulation":
            eng = default_engine(self.engine)
            p0 = undistort_points(self.image_points[i0], c0, engine=eng).astype(np.float64)
            p1 = undistort_points(self.image_points[i1], c1, engine=eng).astype(np.float64)
            X = triangulate_points_linear(_projection(c0).reshape(3, 4), _projection(c1).reshape(3, 4), np.c_[p0, np.ones(len(p0))],
                                          np.c_[p1, np.ones(len(p1))], engine=eng)
            self.points3d = X[:, :3] / X[:, 3:4]
        return self.points3d

    def triangulate_nviews(self) -> np.ndarray:
        """One point seen by every camera: `image_points` = list of homogeneous image points [x, y, 1], one per camera."""
        return triangulate_nviews([_projection(c).reshape(3, 4) for c in self.cameras], self.image_points)

    def interpolate_colors_from_image(self, image: np.ndarray, camera, convert_BRG2RGB: bool = True) -> np.ndarray:
        assert self.points3d is not None, "points 3D are not available, Triangulate homologous points first."
        self.colors = interpolate_point_colors(self.points3d, image, camera, convert_BRG2RGB=convert_BRG2RGB, engine=self.engine)
        return self.colors


def _colors_of_device_points(eng, dX, image, camera, convert_BRG2RGB=True):
    """`interpolate_point_colors` on points that are on the device: [n, channels] float64 on the host."""
    assert image.ndim == 3, "invalid input image. Image has not 3 channel"
    if not (isinstance(image, np.ndarray) and image.dtype == np.uint8) and not (hasattr(image, "device") and str(image.dtype) == "torch.uint8"):
        raise ValueError(f"interpolate_point_colors: a uint8 image is expected (got {image.dtype})")
    chmap = _channel_map(image, convert_BRG2RGB)
    if len(dX) == 0:
        return np.zeros((0, len(chmap)))
    return _project_colors_device(eng, dX, _camera_params(camera), image, chmap, want_proj=False)[1].cpu().numpy()


class TableReconstruction(NamedTuple):
    """What `triangulate_table` returns: per-epoch views (lists of length E) into one array each, and the offsets [E + 1] int64."""
    points3d: list
    status: list
    colors: Optional[list]
    offsets: np.ndarray


def _camera_pairs(cameras) -> list:
    """[cam0, cam1] -> [[cam0, cam1]]; a list of pairs as it is."""
    return [cameras] if len(cameras) == 2 and not isinstance(cameras[0], (list, tuple)) else list(cameras)


def _camera_table(cameras, n_records: int) -> np.ndarray:
    """[n_cams, 2, 24] float64: P (12), fx fy cx cy, k1..k6 in OpenCV order per camera; one pair, or one pair per record."""
    pairs = _camera_pairs(cameras)
    if len(pairs) not in (1, n_records):
        raise ValueError(f"triangulate_table: one camera pair or one per record ({n_records}) is expected (got {len(pairs)})")
    out = np.empty((len(pairs), 2, 24))
    for e, pair in enumerate(pairs):
        if len(pair) != 2:
            raise ValueError("triangulate_table: a camera pair has two cameras")
        for v, c in enumerate(pair):
            out[e, v, :12] = _projection(c)
            out[e, v, 12:] = _intrinsics(c)
    return out


def triangulate_table(table, max_kpts: int, cameras, engine=None, undistort: bool = True, image=None, cam_id: int = 1,
                      tolerance: float = DEFAULT_TOLERANCE, convert_BRG2RGB: bool = True) -> TableReconstruction:
    """`Triangulate(...).triangulate_two_views(compute_colors=..., cam_id=1)` for EVERY epoch of a gathered match table at once
    (`sequence.py`: int32 [E, 8 + 6 max_kpts] records with the keypoint payload, a device tensor or a host array). `cameras` is one pair
    [cam0, cam1] for all epochs or a list of E pairs. Per epoch the matched keypoints are taken in ascending keypoint-0 index (the
    reference's `kpts0[matches0 > -1]`, `kpts1[matches0[matches0 > -1]]`), undistorted (unless `undistort=False`) and triangulated in one
    launch over all records; a failed record (n_matches = -1) and an empty one give zero points. `image` (uint8 [h, w, c], or a list of
    E of them) adds the colours seen by camera `cam_id` of the epoch's pair, read from the points on the device.
    Returns per-epoch views of points3d [n_e, 3] float64, status [n_e] int64, colors [n_e, channels] float64 (or None), and offsets [E + 1]."""
    from .sequence import record_words
    eng = default_engine(engine)
    dev = eng.device
    K = int(max_kpts)
    t = table if torch.is_tensor(table) else torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32))
    if t.dtype != torch.int32 or t.ndim != 2 or t.shape[1] != record_words(K, True):
        raise ValueError(f"triangulate_table: an int32 table with rows of {record_words(K, True)} words (max_kpts = {K}, with_keypoints=True) "
                         f"is expected (got {t.dtype}, shape {tuple(t.shape)})")
    t = t.to(dev).contiguous()
    E = int(t.shape[0])
    images = None
    if image is not None:
        images = list(image) if isinstance(image, (list, tuple)) else [image]
        if len(images) not in (1, E):
            raise ValueError(f"triangulate_table: one image or one per record ({E}) is expected (got {len(images)})")
    cams = _camera_table(cameras, E) if E else np.zeros((1, 2, 24))
    if images is not None and len(images) == 1 and len(cams) != 1 and E > 1:
        raise ValueError("triangulate_table: one image needs one camera pair (with a camera pair per record give an image per record)")
    dcams = to_device(cams, dev)
    M = int(t[:, 3].clamp(min=0).sum().item()) if E else 0
    doff = torch.empty(E + 1, dtype=torch.int64, device=dev)
    dX = torch.empty((M, 3), dtype=torch.float64, device=dev)
    dst = torch.empty(M, dtype=torch.int32, device=dev)
    eng.ctx.call("im_triangulate_table", ptr(t), E, K, ptr(dcams), len(cams), int(bool(undistort)), float(tolerance), MAX_SOLVES, M,
                 ptr(doff), ptr(dX) if M else None, ptr(dst) if M else None, None, None, eng.stream_ptr())
    offsets = doff.cpu().numpy()
    if int(offsets[-1]) != M:
        raise RuntimeError(f"triangulate_table: the table changed during the call ({int(offsets[-1])} matches, {M} expected)")
    X, status = dX.cpu().numpy(), dst.cpu().numpy().astype(np.int64)
    cuts = offsets[1:-1]
    colors = None
    if images is not None and E:
        pairs = _camera_pairs(cameras)
        if len(images) == 1:
            colors = np.split(_colors_of_device_points(eng, dX, images[0], pairs[0][cam_id], convert_BRG2RGB), cuts)
        else:
            colors = [_colors_of_device_points(eng, dX[int(offsets[e]):int(offsets[e + 1])], images[e], pairs[e if len(pairs) > 1 else 0][cam_id],
                                               convert_BRG2RGB) for e in range(E)]
    if E == 0:
        return TableReconstruction([], [], None if images is None else [], offsets)
    return TableReconstruction(np.split(X, cuts), np.split(status, cuts), colors, offsets)


class RelativeOrientation:
    """`RelativeOrientation` of the reference (`sfm/two_view_geometry.py:38-197`): cameras = [cam0, cam1] (`core.Camera`), features = the
    matched image points [n, 2] of each. The estimation runs in `estimate_pose` / `geometric_verification` (RANSAC on the device)."""

    def __init__(self, cameras, features, engine=None) -> None:
        self.cameras = cameras
        self.features = features
        self.engine = engine

    def estimate_pose(self, threshold: float = 1.0, confidence: float = 0.9999, scale_factor=None) -> np.ndarray:
        """Relative pose of camera 1 from the matches, chained with the pose of camera 0; updates `cameras[1]`'s extrinsics and returns
        the inlier mask. With `scale_factor` the translation (estimated up to scale) is multiplied by it."""
        assert self.cameras[0].extrinsics is not None, \
            "Extrinsics matrix is not available for camera 0. Please, compute it before running RelativeOrientation estimation."
        ret = estimate_pose(self.features[0], self.features[1], self.cameras[0].K, self.cameras[1].K, thresh=threshold, conf=confidence,
                            engine=default_engine(self.engine))
        if ret is None:
            raise ValueError("RelativeOrientation.estimate_pose: at least 5 matches are needed")
        R, t, valid = ret
        logger.info("Relative Orientation - valid points: %d/%d", valid.sum(), len(valid))
        if scale_factor is not None:
            t = t * scale_factor
        else:
            logger.warning("No scaling factor (e.g., computed from camera baseline) is provided. Two-view-geometry estimated up to a scale factor.")
        # camera 1 relative to camera 0 first, then its pose chained with camera 0's: world <- cam0 <- cam1 (`two_view_geometry.py:99-105`)
        cam1 = self.cameras[1]
        cam1.update_extrinsics(cam1.Rt_to_extrinsics(R, t))
        cam1.update_extrinsics(cam1.pose_to_extrinsics(self.cameras[0].pose @ cam1.pose))
        return valid

    def get_scale_factor_from_baseline(self, baseline_world: float) -> float:
        """baseline_world / |C0 - C1|: the factor that brings the model's baseline to the one measured in the world."""
        return baseline_world / np.linalg.norm(self.cameras[0].C - self.cameras[1].C)

    def estimate_F_matrix(self, threshold: float = 1, confidence: float = 0.9999, max_iters: int = 10000, **_pydegensac_options):
        """(F [3, 3], inlier mask [n] bool) by `geometric_verification` (the reference calls pydegensac here, whose remaining options are
        accepted and not used); `features` keep the inliers only, as in the reference."""
        self.F, self.inlMask = geometric_verification(self.features[0], self.features[1], GeometricVerification.PYDEGENSAC,
                                                      threshold=threshold, confidence=confidence, max_iters=max_iters,
                                                      engine=default_engine(self.engine))
        self.features[0] = self.features[0][self.inlMask]
        self.features[1] = self.features[1][self.inlMask]
        return self.F, self.inlMask


# ---- two-view bundle adjustment with control points (csrc/ba.hip, csrc/ba_point.h) -------------------------------------------------
BA_DIM, BA_CAM, BA_CAMSTATE, BA_STATE, BA_RECORD, BA_SOL = 28, 14, 24, 8, 64, 512
BA_REC_COST0, BA_REC_COST1, BA_REC_LAMBDA, BA_REC_ACCEPTED, BA_REC_COUNT, BA_REC_STATUS, BA_REC_X, BA_REC_PIVOT, BA_REC_ITER = 0, 1, 2, 3, 4, 5, 6, 34, 62
BA_STATUS = {-1: "RUNNING", 0: "OK", 1: "MAX_ITER", 2: "STALLED", 3: "EMPTY", 4: "DEGENERATE"}
BA_PARAMETERS = ("w0", "w1", "w2", "dC0", "dC1", "dC2", "f", "cx", "cy", "k1", "k2", "p1", "p2", "k3")
BA_MASK_DEFAULT = 0x7F | (0x7F << 14)


class BundleResult(NamedTuple):
    """What `bundle_adjust` returns: new `Camera` objects (the originals untouched), the adjusted points [n, 3], the status name, the final
    cost 0.5 sum (residual / sigma)^2, sigma0 = sqrt(2 cost / max(rows - unknowns, 1)), the number of iterations, `history`
    [iterations, 64] (cost before, cost after, lambda, accepted, usable count, status after, the 28 steps, the 28 pivots, the iteration),
    `residuals` [n, 2, 3] (x, y, norm in pixels per camera, NaN where not seen) and the `state` [8] that a further call may resume from."""
    cameras: list
    points3d: np.ndarray
    status: str
    cost: float
    sigma0: float
    iterations: int
    history: np.ndarray
    residuals: np.ndarray
    state: np.ndarray


def ba_mask(free=("pose", "f"), cameras=(0, 1)) -> int:
    """The 28-bit mask that frees the named parameters of the named cameras: "pose" (w and dC), "rotation", "centre", "f", "cx", "cy",
    "k1", "k2", "p1", "p2", "k3", or "all". The default is what the driver's `optimizeCameras(fit_f=True)` names."""
    groups = {"pose": range(0, 6), "rotation": range(0, 3), "centre": range(3, 6), "all": range(0, BA_CAM)}
    mask = 0
    for name in free:
        if name in groups:
            bits = groups[name]
        elif name in BA_PARAMETERS[6:]:
            bits = [BA_PARAMETERS.index(name)]
        else:
            raise ValueError(f"ba_mask: unknown parameter {name!r}")
        for c in cameras:
            if c not in (0, 1):
                raise ValueError("ba_mask: cameras are 0 and 1")
            for b in bits:
                mask |= 1 << (BA_CAM * c + b)
    return mask


def _ba_camera_state(camera) -> np.ndarray:
    """[24] float64 of a camera object: R row-major, C, fx fy cx cy, k1 k2 p1 p2 k3 k4 k5 k6 (a shorter distortion vector is zero-filled)."""
    out = np.zeros(BA_CAMSTATE)
    R = np.asarray(camera.R, np.float64).reshape(3, 3)
    out[:9] = R.reshape(9)
    out[9:12] = -(R.T @ np.asarray(camera.t, np.float64).reshape(3))
    out[12:] = _intrinsics(camera)
    return out


def _ba_camera_from_state(camera, state: np.ndarray):
    """A copy of `camera` with K, extrinsics and distortion of the state [24]; the distortion vector keeps its length."""
    import copy
    new = copy.deepcopy(camera)
    K = np.array(camera.K, np.float64)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = state[12:16]
    new.update_K(K)
    R, C = state[:9].reshape(3, 3), state[9:12].reshape(3, 1)
    ext = np.eye(4)
    ext[:3, :3], ext[:3, 3:4] = R, -(R @ C)
    new.update_extrinsics(ext)
    if camera.dist is not None:
        d = np.array(camera.dist, np.float64)
        flat = d.reshape(-1)
        flat[:min(flat.size, 8)] = state[16:16 + min(flat.size, 8)]
        new.update_dist(d)
    return new


def _ba_options(lambda0, lambda_min, lambda_max, ftol, max_iter, ctol):
    if not (np.isfinite(lambda0) and lambda0 >= 0.0):
        raise ValueError(f"bundle_adjust: lambda0 must be finite and >= 0 (got {lambda0})")
    if not (0.0 < lambda_min <= lambda_max and np.isfinite(lambda_max)):
        raise ValueError(f"bundle_adjust: 0 < lambda_min <= lambda_max is expected (got {lambda_min}, {lambda_max})")
    if not (ftol >= 0.0 and ctol >= 0.0):
        raise ValueError(f"bundle_adjust: ftol and ctol must be >= 0 (got {ftol}, {ctol})")
    if int(max_iter) != max_iter or not 1 <= max_iter <= 10000:
        raise ValueError(f"bundle_adjust: max_iter must be an integer in 1..10000 (got {max_iter})")
    return np.array([lambda_min, lambda_max, ftol, float(max_iter), ctol])


def ba_problem(cameras, image_points, points3d, targets=None, camera_centers_world=None, image_sigma=1.0, target_image_sigma=None,
               target_accuracy=0.01, cam_accuracy=0.1) -> dict:
    """The arrays of one epoch in the layout of `im_ba_*` (host, float64): cams [48], X [n, 3], obs [n, 4], sig [n], prior [n, 6],
    cprior [12]; the tie points first, then the targets. `targets` = (image coordinates per camera: two [m, 2] arrays with NaN rows where a
    camera does not see the target, object coordinates [m, 3]); their start is the object coordinate and their prior sigma is
    `target_accuracy` (a scalar, [3] or [m, 3]; 0 leaves a component free). `camera_centers_world` = two [3] centres (or None per camera)
    with `cam_accuracy` (a scalar or [3])."""
    if len(cameras) != 2 or len(image_points) != 2:
        raise ValueError("bundle_adjust: two cameras and two arrays of image points are expected")
    X = np.ascontiguousarray(_points(points3d), np.float64)
    uv = [_image_points(p, np.float64) for p in image_points]
    if not (len(uv[0]) == len(uv[1]) == len(X)):
        raise ValueError(f"bundle_adjust: image_points and points3d must have one row per tie point (got {len(uv[0])}, {len(uv[1])}, {len(X)})")
    if not (np.isfinite(image_sigma) and image_sigma > 0.0):
        raise ValueError(f"bundle_adjust: image_sigma must be > 0 (got {image_sigma})")
    n = len(X)
    obs, sig, prior = np.concatenate(uv, 1).reshape(n, 4), np.full(n, float(image_sigma)), np.zeros((n, 6))
    if targets is not None:
        t_img, t_obj = targets
        t_obj = np.ascontiguousarray(t_obj, np.float64).reshape(-1, 3)
        t_uv = [np.asarray(p, np.float64).reshape(-1, 2) for p in t_img]
        if len(t_uv) != 2 or not (len(t_uv[0]) == len(t_uv[1]) == len(t_obj)):
            raise ValueError("bundle_adjust: targets = ([uv in camera 0 [m, 2], uv in camera 1 [m, 2]], object coordinates [m, 3])")
        acc = np.broadcast_to(np.asarray(target_accuracy, np.float64), t_obj.shape)
        if not (np.isfinite(acc).all() and (acc >= 0.0).all()):
            raise ValueError("bundle_adjust: target_accuracy must be finite and >= 0")
        ts = float(image_sigma if target_image_sigma is None else target_image_sigma)
        if not (np.isfinite(ts) and ts > 0.0):
            raise ValueError(f"bundle_adjust: target_image_sigma must be > 0 (got {ts})")
        X = np.concatenate([X, t_obj])
        obs = np.concatenate([obs, np.concatenate(t_uv, 1)])
        sig = np.concatenate([sig, np.full(len(t_obj), ts)])
        prior = np.concatenate([prior, np.concatenate([t_obj, acc], 1)])
    cprior = np.zeros(12)
    if camera_centers_world is not None:
        if len(camera_centers_world) != 2:
            raise ValueError("bundle_adjust: camera_centers_world holds one centre (or None) per camera")
        acc = np.broadcast_to(np.asarray(cam_accuracy, np.float64), (3,))
        if not (np.isfinite(acc).all() and (acc >= 0.0).all()):
            raise ValueError("bundle_adjust: cam_accuracy must be finite and >= 0")
        for c, centre in enumerate(camera_centers_world):
            if centre is not None:
                centre = np.asarray(centre, np.float64).reshape(-1)
                if centre.shape != (3,) or not np.isfinite(centre).all():
                    raise ValueError("bundle_adjust: a camera centre is three finite numbers")
                cprior[6 * c:6 * c + 3], cprior[6 * c + 3:6 * c + 6] = centre, acc
    cams = np.concatenate([_ba_camera_state(c) for c in cameras])
    return dict(cams=cams, X=X, obs=np.ascontiguousarray(obs), sig=sig, prior=np.ascontiguousarray(prior), cprior=cprior)


def ba_run_device(problems, mask, lambda0, opts, states=None, engine=None):
    """The whole loop of E epochs on the device: 4 launches per iteration for all epochs at once and ONE read-back at the end. `problems`:
    dicts as `ba_problem` returns them (host arrays or device tensors). Returns per epoch (cams [48], X [n, 3], state [8], history
    [iterations, 64], residuals [n, 2, 3])."""
    eng = default_engine(engine)
    dev, E = eng.device, len(problems)
    if E < 1:
        raise ValueError("bundle_adjust: at least one epoch is expected")
    f64 = lambda v, w: (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, np.float64))).to(dev, torch.float64).reshape(-1, w)
    X = [f64(p["X"], 3) for p in problems]
    off = np.concatenate([[0], np.cumsum([len(x) for x in X])]).astype(np.int64)
    M, max_points = int(off[-1]), int(np.diff(off).max())
    cat = lambda k, w: torch.cat([f64(p[k], w) for p in problems] + [torch.zeros((0 if M else 1, w), dtype=torch.float64, device=dev)]).contiguous()
    dX = torch.cat(X + [torch.zeros((0 if M else 1, 3), dtype=torch.float64, device=dev)])
    cams = torch.cat([f64(p["cams"], 2 * BA_CAMSTATE) for p in problems])
    cprior = torch.cat([f64(p["cprior"], 12) for p in problems]).contiguous()
    return _ba_split(off, *_ba_run_batched(eng, E, M, max_points, to_device(off, dev), dX, cat("obs", 4), cat("sig", 1), cat("prior", 6), cams, cprior,
                                           mask, lambda0, opts, states))


def _ba_run_batched(eng, E, M, max_points, doff, dX, obs, sig, prior, cams, cprior, mask, lambda0, opts, states=None):
    """The loop on arrays that are on the device already (doff [E + 1] int64, dX [max(M, 1), 3], obs, sig, prior, cams [E, 48], cprior
    [E, 12]): enqueues everything and returns device tensors (state, history, cams2, pts2, residuals) and the first history row of every
    epoch. Nothing is read back here; `max_points` bounds the points of an epoch."""
    dev, max_iter = eng.device, int(opts[3])
    pts2 = torch.zeros((2, max(M, 1), 3), dtype=torch.float64, device=dev)
    pts2[0] = dX
    cams2 = torch.zeros((2, E, 2 * BA_CAMSTATE), dtype=torch.float64, device=dev)
    cams2[0] = cams
    st = np.zeros((E, BA_STATE))
    st[:, 0], st[:, 3] = lambda0, -1.0
    if states is not None:
        st = np.ascontiguousarray(states, np.float64).reshape(E, BA_STATE).copy()
        st[:, 1], st[:, 2] = 0.0, 0.0                              # the current buffers are the ones handed in; the run goes on
        st[:, 3] = -1.0
    first = st[:, 4].astype(np.int64)
    if (first >= max_iter).any():
        raise ValueError("bundle_adjust: a resumed state has used its max_iter iterations already")
    state = to_device(st, dev)
    sol = torch.zeros((E, BA_SOL), dtype=torch.float64, device=dev)
    history = torch.zeros((max_iter, E, BA_RECORD), dtype=torch.float64, device=dev)
    res = torch.full((max(M, 1), 2, 3), float("nan"), dtype=torch.float64, device=dev)
    h_opts = np.ascontiguousarray(opts, np.float64)
    s, call = eng.stream_ptr(), eng.ctx.call
    for _ in range(max_iter - int(first.min())):
        call("im_ba_accumulate", ptr(doff), E, M, max_points, ptr(pts2), ptr(obs), ptr(sig), ptr(prior), ptr(cams2), ptr(state), None, s)
        call("im_ba_solve", ptr(doff), E, M, None, ptr(cams2), ptr(cprior), ptr(state), int(mask), ptr(sol), s)
        call("im_ba_step_points", ptr(doff), E, M, max_points, ptr(pts2), ptr(obs), ptr(sig), ptr(prior), ptr(cams2), ptr(state), ptr(sol), None, s)
        call("im_ba_decide", ptr(doff), E, M, None, ptr(cams2), ptr(cprior), ptr(state), ptr(sol), h_opts.ctypes.data, ptr(history), max_iter, s)
    call("im_ba_residuals", ptr(doff), E, M, max_points, ptr(pts2), ptr(obs), ptr(cams2), ptr(state), ptr(res), s)
    return state, history, cams2, pts2, res, first


def _ba_split(off, state, history, cams2, pts2, res, first) -> list:
    """The one read-back, and per epoch (cams [48], X [n, 3], state [8], history [iterations, 64], residuals [n, 2, 3])."""
    st, hist, cams_h, pts_h, res_h = state.cpu().numpy(), history.cpu().numpy(), cams2.cpu().numpy(), pts2.cpu().numpy(), res.cpu().numpy()
    out = []
    for e in range(len(st)):
        par, a, b = int(st[e, 1] != 0.0), int(off[e]), int(off[e + 1])
        out.append((cams_h[par, e].copy(), pts_h[par, a:b].copy(), st[e].copy(), hist[first[e]:int(st[e, 4]), e].copy(), res_h[a:b].copy()))
    return out


def _ba_result(cameras, problem, mask, out) -> BundleResult:
    cams, X, st, hist, res = out
    if len(hist):
        last = hist[-1]
        cost = float(last[BA_REC_COST1] if last[BA_REC_ACCEPTED] else last[BA_REC_COST0])
    else:
        cost = float("nan")
    rows = 2 * int(np.isfinite(res[:, :, 2]).sum()) + int((problem["prior"][:, 3:] > 0).sum()) + int((problem["cprior"].reshape(2, 6)[:, 3:] > 0).sum())
    unknowns = bin(int(mask)).count("1") + 3 * int(np.isfinite(res[:, :, 2]).any(1).sum())
    sigma0 = float(np.sqrt(2.0 * cost / max(rows - unknowns, 1)))
    new = [_ba_camera_from_state(c, cams[BA_CAMSTATE * i:BA_CAMSTATE * (i + 1)]) for i, c in enumerate(cameras)]
    return BundleResult(new, X, BA_STATUS[int(st[3])], cost, sigma0, len(hist), hist, res, st)


def bundle_adjust(cameras, image_points, points3d, targets=None, camera_centers_world=None, image_sigma=1.0, target_image_sigma=None,
                  target_accuracy=0.01, cam_accuracy=0.1, mask=BA_MASK_DEFAULT, lambda0=1e-3, lambda_min=1e-12, lambda_max=1e8, ftol=1e-9,
                  ctol=0.0, max_iter=30, state=None, engine=None, _run=None) -> BundleResult:
    """Bundle adjustment of ONE epoch (two cameras) on the device, where the driver calls `chunk.optimizeCameras(fit_f=True)`: the two
    `Camera`s, their matched image points [n, 2] each (distorted pixels, as the matcher gives them), the triangulated points [n, 3], and
    optionally the targets (image and object coordinates with `target_accuracy`) and the surveyed camera centres with `cam_accuracy`.
    Levenberg-Marquardt with the points eliminated over 14 parameters per camera (`BA_PARAMETERS`; `mask`, see `ba_mask`, frees poses and
    f by default), cost 0.5 sum (residual / sigma)^2, every sum in an order fixed by the point index: bit-identical to the restatement
    `tests/ba_oracle.py`. A definition of its own: parity with Metashape is unpinned; there is no b1 / b2, no robust loss and
    no covariance. `state` = the `state` of an earlier result resumes that run (with its lambda and iteration count) from the cameras and
    points that are handed in; since a target always starts at its object coordinates, a run with `targets` resumes bit for bit only
    through `ba_run_device` on the returned arrays, or with the adjusted targets passed as tie points. The originals are untouched."""
    if int(mask) != mask or not 0 <= int(mask) < (1 << BA_DIM):
        raise ValueError(f"bundle_adjust: the mask has {BA_DIM} bits (got {mask})")
    opts = _ba_options(lambda0, lambda_min, lambda_max, ftol, max_iter, ctol)
    problem = ba_problem(cameras, image_points, points3d, targets, camera_centers_world, image_sigma, target_image_sigma, target_accuracy,
                         cam_accuracy)
    run = _run if _run is not None else (lambda ps, m, l0, o, sts: ba_run_device(ps, m, l0, o, sts, engine=engine))
    out = run([problem], int(mask), float(lambda0), opts, None if state is None else [state])[0]
    return _ba_result(cameras, problem, mask, out)


def bundle_adjust_epochs(cameras, image_points, points3d, targets=None, camera_centers_world=None, engine=None, _run=None, mask=BA_MASK_DEFAULT,
                         lambda0=1e-3, lambda_min=1e-12, lambda_max=1e8, ftol=1e-9, ctol=0.0, max_iter=30, **problem_options) -> list:
    """`bundle_adjust` for EVERY epoch of a sequence at once: `cameras` one pair or a list of E pairs, `image_points` a list of E
    [uv0, uv1], `points3d` a list of E arrays (e.g. `triangulate_table(...).points3d`), `targets` None, one (image, object) TUPLE for all
    epochs or a LIST of E of them, `camera_centers_world` likewise (a tuple of two centres for all epochs, or a list of E). All epochs share the launches: 4 per iteration, one read-back at the end; each
    epoch stops on its own. Returns a list of E `BundleResult`, each bit-identical to the epoch run alone."""
    E = len(points3d)
    if len(image_points) != E:
        raise ValueError(f"bundle_adjust_epochs: image_points and points3d hold one entry per epoch (got {len(image_points)}, {E})")
    if int(mask) != mask or not 0 <= int(mask) < (1 << BA_DIM):
        raise ValueError(f"bundle_adjust_epochs: the mask has {BA_DIM} bits (got {mask})")
    pairs = _camera_pairs(cameras)
    if len(pairs) not in (1, E):
        raise ValueError(f"bundle_adjust_epochs: one camera pair or one per epoch ({E}) is expected (got {len(pairs)})")
    for name, v in (("targets", targets), ("camera_centers_world", camera_centers_world)):
        if isinstance(v, list) and len(v) != E:
            raise ValueError(f"bundle_adjust_epochs: a list of {name} holds one entry per epoch ({E}); a tuple is shared by all epochs")
    per = lambda v, e: v[e] if isinstance(v, list) else v
    opts = _ba_options(lambda0, lambda_min, lambda_max, ftol, max_iter, ctol)
    problems = [ba_problem(pairs[e if len(pairs) > 1 else 0], image_points[e], points3d[e], None if targets is None else per(targets, e),
                           None if camera_centers_world is None else per(camera_centers_world, e), **problem_options) for e in range(E)]
    run = _run if _run is not None else (lambda ps, m, l0, o, sts: ba_run_device(ps, m, l0, o, sts, engine=engine))
    outs = run(problems, int(mask), float(lambda0), opts, None)
    return [_ba_result(pairs[e if len(pairs) > 1 else 0], problems[e], mask, outs[e]) for e in range(E)]


def table_image_points(table, max_kpts: int) -> list:
    """Per record of a gathered match table with the keypoint payload: [uv0, uv1], the matched keypoints [n_e, 2] float64 in ascending
    keypoint-0 index, the order in which `triangulate_table` triangulates them; a failed or empty record gives zero rows."""
    from .sequence import decode_record, record_words
    t = table.cpu().numpy() if torch.is_tensor(table) else np.ascontiguousarray(table, dtype=np.int32)
    if t.dtype != np.int32 or t.ndim != 2 or t.shape[1] != record_words(int(max_kpts), True):
        raise ValueError(f"an int32 table with rows of {record_words(int(max_kpts), True)} words (max_kpts = {max_kpts}, with_keypoints=True) is "
                         f"expected (got {t.dtype}, shape {t.shape})")
    out = []
    for rec in t:
        d = decode_record(rec, int(max_kpts))
        m = d["matches0"] if d["n_matches"] > 0 else np.zeros(0, np.int64)
        hit = m > -1
        out.append([d["keypoints0"][:len(m)][hit].astype(np.float64), d["keypoints1"][m[hit]].astype(np.float64)])
    return out


def _table_observations(t, K: int, doff, M: int):
    """The matched keypoints of a gathered match table ON THE DEVICE, in the rows `im_triangulate_table` gives their points: obs
    [max(M, 1), 4] float64 = (u0, v0, u1, v1). As the kernel takes them: the entries 0 <= matches0[i] < K of a record in ascending i, the
    first n_matches of them, at rows doff[e] + rank; a row the record does not fill stays NaN (its point is NaN too). torch index
    arithmetic only, no read-back: surplus entries go to a spare last row that is cut off."""
    E, dev = int(t.shape[0]), t.device
    obs = torch.full((M + 1, 4), float("nan"), dtype=torch.float64, device=dev)
    if E and M:
        m = t[:, 8:8 + K].to(torch.int64)
        valid = (m >= 0) & (m < K)
        rank = torch.cumsum(valid.to(torch.int64), 1) - 1
        keep = valid & (rank < t[:, 3].clamp(min=0).to(torch.int64)[:, None])
        dest = torch.where(keep, doff[:E, None] + rank, torch.full_like(rank, M)).clamp(max=M)
        kp = t[:, 8 + 2 * K:].contiguous().view(torch.float32).reshape(E, 2, K, 2).to(torch.float64)
        uv1 = torch.gather(kp[:, 1], 1, m.clamp(0, K - 1)[:, :, None].expand(-1, -1, 2))
        obs[dest.reshape(-1)] = torch.cat([kp[:, 0], uv1], 2).reshape(E * K, 4)
    return obs[:max(M, 1)].contiguous() if M else torch.full((1, 4), float("nan"), dtype=torch.float64, device=dev)


def _triangulate_table_device(eng, table, K: int, cameras, undistort=True, tolerance=DEFAULT_TOLERANCE, launch=True):
    """`triangulate_table`'s launch with everything left on the device: (table, E, M, offsets [E + 1] int64, points [M, 3], status [M]);
    launch=False only uploads the table and sizes the arrays."""
    from .sequence import record_words
    t = table if torch.is_tensor(table) else torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32))
    if t.dtype != torch.int32 or t.ndim != 2 or t.shape[1] != record_words(K, True):
        raise ValueError(f"an int32 table with rows of {record_words(K, True)} words (max_kpts = {K}, with_keypoints=True) is expected "
                         f"(got {t.dtype}, shape {tuple(t.shape)})")
    dev = eng.device
    t = t.to(dev).contiguous()
    E = int(t.shape[0])
    cams = _camera_table(cameras, E) if E else np.zeros((1, 2, 24))
    dcams = to_device(cams, dev)
    M = int(t[:, 3].clamp(min=0).sum().item()) if E else 0            # before the launch: the outputs are sized by it
    doff = torch.zeros(E + 1, dtype=torch.int64, device=dev)
    dX = torch.empty((M, 3), dtype=torch.float64, device=dev)
    dst = torch.empty(M, dtype=torch.int32, device=dev)
    if launch:
        eng.ctx.call("im_triangulate_table", ptr(t), E, K, ptr(dcams), len(cams), int(bool(undistort)), float(tolerance), MAX_SOLVES, M,
                     ptr(doff), ptr(dX) if M else None, ptr(dst) if M else None, None, None, eng.stream_ptr())
    return t, E, M, doff, dX, dst


def bundle_adjust_table(table, max_kpts: int, cameras, reconstruction=None, targets=None, camera_centers_world=None, image_sigma=1.0,
                        target_image_sigma=None, target_accuracy=0.01, cam_accuracy=0.1, mask=BA_MASK_DEFAULT, lambda0=1e-3, lambda_min=1e-12,
                        lambda_max=1e8, ftol=1e-9, ctol=0.0, max_iter=30, undistort=True, engine=None, _run=None) -> list:
    """`bundle_adjust` for EVERY record of a gathered match table (`sequence.py`: int32 [E, 8 + 6 max_kpts] with the keypoint payload, a
    device tensor or a host array) without leaving the device between triangulation and the final read-back: `im_triangulate_table`
    leaves its points and offsets on the device, the matched keypoints are gathered there into the same rows, the targets (one (image,
    object) tuple for all epochs) are laid behind every epoch's tie points there, the four kernels run `max_iter` rounds for all epochs,
    and states, histories, cameras, points, residuals and offsets come back in ONE read-back. The only earlier read is the table's total
    match count, before the triangulation, which sizes the arrays. `cameras` is one pair or a list of E pairs. A point whose
    triangulation failed (NaN) is unusable and stays. `reconstruction` (a `TableReconstruction` of this table) replaces the
    triangulation by its points, uploaded. One `BundleResult` per record, each bit-identical to `bundle_adjust` on the record's own
    keypoints and points. (`_run`: the restatement in the device's place, for tests without one; then everything is host work.)"""
    K = int(max_kpts)
    if int(mask) != mask or not 0 <= int(mask) < (1 << BA_DIM):
        raise ValueError(f"bundle_adjust_table: the mask has {BA_DIM} bits (got {mask})")
    opts = _ba_options(lambda0, lambda_min, lambda_max, ftol, max_iter, ctol)
    if isinstance(targets, list) or isinstance(camera_centers_world, list):
        raise ValueError("bundle_adjust_table: targets and camera_centers_world are shared by all epochs (a tuple each); use bundle_adjust_epochs for one per epoch")
    pkw = dict(image_sigma=image_sigma, target_image_sigma=target_image_sigma, target_accuracy=target_accuracy, cam_accuracy=cam_accuracy)
    if _run is not None:
        uv = table_image_points(table, K)
        if reconstruction is None or len(reconstruction.points3d) != len(uv) or any(len(x) != len(p[0]) for x, p in zip(reconstruction.points3d, uv)):
            raise ValueError("bundle_adjust_table: the reconstruction does not belong to this table (points per record differ)")
        if not uv:
            return []
        return bundle_adjust_epochs(cameras, uv, list(reconstruction.points3d), targets=targets, camera_centers_world=camera_centers_world,
                                    _run=_run, mask=mask, lambda0=lambda0, lambda_min=lambda_min, lambda_max=lambda_max, ftol=ftol, ctol=ctol,
                                    max_iter=max_iter, **pkw)
    eng = default_engine(engine)
    dev = eng.device
    t, E, M, doff, dX, _ = _triangulate_table_device(eng, table, K, cameras, undistort=undistort, launch=reconstruction is None)
    if E == 0:
        return []
    if reconstruction is not None:
        if len(reconstruction.points3d) != E or int(np.asarray(reconstruction.offsets)[-1]) != M:
            raise ValueError("bundle_adjust_table: the reconstruction does not belong to this table (points per record differ)")
        dX = to_device(np.concatenate([np.asarray(x, np.float64).reshape(-1, 3) for x in reconstruction.points3d] + [np.zeros((0, 3))]), dev)
        doff = to_device(np.asarray(reconstruction.offsets, np.int64), dev)
    pairs = _camera_pairs(cameras)
    # what one epoch adds behind its tie points (targets) and its cameras and centre priors: ba_problem's own host logic on an empty epoch
    tail = [ba_problem(pairs[e if len(pairs) > 1 else 0], [np.zeros((0, 2)), np.zeros((0, 2))], np.zeros((0, 3)), targets, camera_centers_world, **pkw)
            for e in range(len(pairs))]
    m = len(tail[0]["X"])
    Mt = M + E * m
    obs_tie = _table_observations(t, K, doff, M)
    doff2 = doff + m * torch.arange(E + 1, dtype=torch.int64, device=dev)
    X = torch.zeros((max(Mt, 1), 3), dtype=torch.float64, device=dev)
    obs = torch.full((max(Mt, 1), 4), float("nan"), dtype=torch.float64, device=dev)
    sig = torch.full((max(Mt, 1),), float(image_sigma), dtype=torch.float64, device=dev)
    prior = torch.zeros((max(Mt, 1), 6), dtype=torch.float64, device=dev)
    if M:
        epoch = torch.searchsorted(doff[1:].contiguous(), torch.arange(M, dtype=torch.int64, device=dev), right=True)
        row = torch.arange(M, dtype=torch.int64, device=dev) + m * epoch
        X[row], obs[row] = dX, obs_tie[:M]
    if m:
        row = (doff2[1:, None] - m + torch.arange(m, dtype=torch.int64, device=dev)[None, :]).reshape(-1)
        X[row] = to_device(tail[0]["X"], dev).repeat(E, 1)
        obs[row] = to_device(tail[0]["obs"], dev).repeat(E, 1)
        sig[row] = to_device(tail[0]["sig"], dev).repeat(E)
        prior[row] = to_device(tail[0]["prior"], dev).repeat(E, 1)
    cams = to_device(np.stack([tail[e if len(tail) > 1 else 0]["cams"] for e in range(E)]), dev)
    cprior = to_device(np.stack([tail[e if len(tail) > 1 else 0]["cprior"] for e in range(E)]), dev)
    max_points = min(K + m, Mt)
    ran = _ba_run_batched(eng, E, Mt, max_points, doff2.contiguous(), X, obs, sig, prior, cams, cprior, mask, lambda0, opts)
    off2 = doff2.cpu().numpy()                                            # with the results: the one read-back
    outs = _ba_split(off2, *ran)
    obs_h, prior_h = obs.cpu().numpy(), prior.cpu().numpy()
    results = []
    for e in range(E):
        a, b = int(off2[e]), int(off2[e + 1])
        problem = dict(prior=prior_h[a:b], cprior=tail[e if len(tail) > 1 else 0]["cprior"])
        results.append(_ba_result(pairs[e if len(pairs) > 1 else 0], problem, mask, outs[e]))
    return results
