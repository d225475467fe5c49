"""`Camera` of the reference (`src/icepy4d/core/camera.py:39-460`): a pinhole camera that keeps ONE expression of its exterior orientation,
the 4 x 4 extrinsics matrix (world -> camera), and derives pose, centre, R, t and P from it. The numpy part is host algebra on 4 x 4
matrices and mirrors the reference's operation order (block matrices multiplied, not assembled: `pose = [I | C] [R' | 0]`); `project_point`
goes through `sfm.project_points` (device). Same names, same shapes: C and t are [3, 1] columns, as in the reference."""
from pathlib import Path
from typing import Tuple, Union

import numpy as np


def _block(mat: np.ndarray) -> np.ndarray:
    """4 x 4 homogeneous block of a 3 x 3 rotation ([R 0; 0 1]) or of a 3 x 1 translation ([I t; 0 1])."""
    out = np.eye(4)
    if mat.shape[1] == 3:
        out[0:3, 0:3] = mat
    elif mat.shape[1] == 1:
        out[0:3, 3:4] = mat
    else:
        raise ValueError(f"expected a 3x3 or a 3x1 matrix (got shape {mat.shape})")
    return out


def read_opencv_calibration(path: Union[str, Path]):
    """One line of floats: width height fx 0. cx 0. fy cy 0. 0. 1. k1 k2 p1 p2 [k3 [k4 k5 k6]] -> (w, h, K [3, 3], dist)."""
    path = Path(path)
    if not path.exists():
        raise FileNotFoundError(f"calibration file {path} does not exist")
    data = np.loadtxt(path).ravel()
    if len(data) not in (15, 16, 19):
        raise ValueError(f"{path}: expected 15, 16 or 19 values (got {len(data)})")
    return data[0], data[1], data[2:11].astype(float).reshape(3, 3), data[11:].astype(float)


class Camera:
    """Pinhole camera: image size, K, distortion vector (OpenCV order k1 k2 p1 p2 [k3 [k4 k5 k6]]) and extrinsics. The exterior
    orientation changes through `update_extrinsics` only; build its argument with `pose_to_extrinsics` or `Rt_to_extrinsics`."""

    def __init__(self, width, height, K: np.ndarray = None, dist: np.ndarray = None, R: np.ndarray = None, t: np.ndarray = None,
                 extrinsics: np.ndarray = None, calib_path: Union[str, Path] = None):
        self._w = width
        self._h = height
        self._K = K
        self._dist = dist
        self.reset_EO()
        if R is not None and t is not None:
            self._extrinsics = self.Rt_to_extrinsics(np.asarray(R, np.float64), np.asarray(t, np.float64))
        if extrinsics is not None:
            self._extrinsics = extrinsics
        if calib_path is not None:
            self.read_calibration_from_file(calib_path)

    def __repr__(self) -> str:
        f = None if self._K is None else self._K[0, 0]
        return f"Camera (f={f}, img_size={self._w, self._h})"

    @property
    def width(self):
        return self._w

    @property
    def height(self):
        return self._h

    @property
    def K(self) -> np.ndarray:
        return self._K

    @property
    def dist(self) -> np.ndarray:
        return self._dist

    @property
    def extrinsics(self) -> np.ndarray:
        """[R t; 0 1], world -> camera."""
        return self._extrinsics

    @property
    def pose(self) -> np.ndarray:
        """[R' C; 0 1], camera -> world."""
        return self.extrinsics_to_pose()

    @property
    def C(self) -> np.ndarray:
        """The projection centre in world coordinates, [3, 1]: -R' t."""
        return self.extrinsics_to_pose()[0:3, 3:4]

    @property
    def t(self) -> np.ndarray:
        return self._extrinsics[0:3, 3:4]

    @property
    def R(self) -> np.ndarray:
        return self._extrinsics[0:3, 0:3]

    @property
    def P(self) -> np.ndarray:
        """K [R | t], 3 x 4."""
        Rt = np.zeros((3, 4))
        Rt[:, 0:3] = self.R
        Rt[:, 3:4] = self.t
        return self.K @ Rt

    def update_K(self, K: np.ndarray) -> None:
        self._K = K

    def update_dist(self, dist: np.ndarray) -> None:
        self._dist = dist

    def update_extrinsics(self, extrinsics: np.ndarray) -> None:
        assert extrinsics.shape == (4, 4), "Wrong dimension of the extrinsics matrix. Please, provide a 4x4 numpy array (homogeneous coordinates)."
        assert extrinsics.dtype == np.float64, "Wrong data type of the extrinsics matrix. Please, provide a numpy array of np.float64."
        assert np.array_equal(extrinsics[3, :], np.array([0.0, 0.0, 0.0, 1.0])), \
            "Extrinsics must be in homogeneous coordinates (the last row of the matrix must be [0 0 0 1])."
        self._extrinsics = extrinsics

    def reset_EO(self) -> None:
        """Camera axes parallel to the world's, centre at the origin."""
        self._extrinsics = np.eye(4)

    def read_calibration_from_file(self, path: Union[str, Path]) -> None:
        self._w, self._h, self._K, self._dist = read_opencv_calibration(path)

    def extrinsics_to_pose(self, extrinsics: np.ndarray = None) -> np.ndarray:
        if extrinsics is None:
            extrinsics = self._extrinsics
        Rc = extrinsics[0:3, 0:3].T
        C = -np.dot(Rc, extrinsics[0:3, 3:4])
        return np.dot(_block(C), _block(Rc))

    def pose_to_extrinsics(self, pose: np.ndarray) -> np.ndarray:
        R = pose[0:3, 0:3].T
        t = -R @ pose[0:3, 3:4]
        return _block(t) @ _block(R)

    def Rt_to_extrinsics(self, R: np.ndarray, t: np.ndarray) -> np.ndarray:
        if t.ndim == 1 or t.shape == (1, 3):
            assert t.size == 3, "Invalid translation vector"
            t = t.reshape(3, 1)
        return _block(t) @ _block(R)

    def C_from_P(self, P: np.ndarray) -> np.ndarray:
        """-inv(P[:, :3]) P[:, 3], [3, 1]."""
        return -np.dot(np.linalg.inv(P[:, 0:3]), P[:, 3].reshape(3, 1))

    def build_pose_matrix(self, R: np.ndarray, C: np.ndarray) -> np.ndarray:
        if R.shape != (3, 3):
            raise ValueError("Wrong dimension of the R matrix. It must be a 3x3 numpy array")
        if C.shape == (3,) or C.shape == (1, 3):
            C = C.reshape(3, 1)
        elif C.shape != (3, 1):
            raise ValueError("Wrong dimension of the C vector. It must be a 3x1 or a 1x3 numpy array")
        pose = np.eye(4)
        pose[0:3, 0:3] = R
        pose[0:3, 3:4] = C
        return pose

    def factor_P(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """P = K [R | t] by RQ decomposition, the diagonal of K made positive: (K [3, 3], R [3, 3], t [3, 1])."""
        from scipy import linalg
        P = self.P
        K, R = linalg.rq(P[:, :3])
        T = np.diag(np.sign(np.diag(K)))
        if linalg.det(T) < 0:
            T[1, 1] *= -1
        K = np.dot(K, T)
        R = np.dot(T, R)
        t = np.dot(linalg.inv(K), P[:, 3]).reshape(3, 1)
        return K, R, t

    def project_point(self, points3d: np.ndarray, engine=None) -> np.ndarray:
        """[n, 3] world points -> [n, 2] float32 image points with the distortion applied (`sfm.project_points`, on the device)."""
        assert points3d.shape[1] == 3, "Wrong size of the input point array. Provide a nx3 numpy array."
        from ..sfm import project_points
        return project_points(points3d, self, engine=engine)


# ---- argument packing of `im_project_colors` (csrc/dsm.hip), shared by `sfm` and `utils.dsm_orthophoto`
def _camera_params(camera) -> np.ndarray:
    """[28] float64 for `im_project_colors`: fx, fy, cx, cy, R (row-major), t, k1 k2 p1 p2 k3 k4 k5 k6 s1..s4. Reads only `.K`, `.dist`,
    `.R` and `.t`, as the reference does. Distortion vectors of length 0, 4, 5 or 8 (OpenCV's forms without thin prism / tilt terms)."""
    K = np.asarray(camera.K, np.float64).reshape(3, 3)
    R = np.asarray(camera.R, np.float64).reshape(9)
    t = np.asarray(camera.t, np.float64).reshape(3)
    dist = np.zeros(0) if camera.dist is None else np.asarray(camera.dist, np.float64).ravel()
    if len(dist) not in (0, 4, 5, 8):
        raise ValueError(f"project_points: distortion vectors of length 0, 4, 5 or 8 are supported (got {len(dist)})")
    k = np.zeros(12)
    k[:len(dist)] = dist
    return np.ascontiguousarray(np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], R, t, k]))


def _channel_map(image: np.ndarray, convert_BRG2RGB: bool) -> np.ndarray:
    """Output channel -> image channel: cv2.cvtColor(BGR2RGB) keeps B, G, R reversed (and drops a fourth channel)."""
    c = image.shape[2]
    if convert_BRG2RGB:
        if c not in (3, 4):
            raise ValueError(f"interpolate_point_colors: BGR to RGB needs a 3- or 4-channel image (got {c})")
        return np.array([2, 1, 0], np.int32)
    if not 1 <= c <= 4:
        raise ValueError(f"interpolate_point_colors: 1 to 4 channels are supported (got {c})")
    return np.arange(c, dtype=np.int32)
