"""Rigid transforms of points and clouds (`src/icepy4d/utils/transformations.py`: `Rotrotranslation`, `convert_to_homogeneous`,
`convert_from_homogeneous`), applied on the device by `im_transform_points` (csrc/icp.hip). No CPU fallback: `transform` raises without a
HIP device; the matrix algebra (`T`, `T_inv`, the validity checks, file I/O) is host numpy as in the reference.

The apply is this library's own definition: p_a = ((M_a0*x + M_a1*y) + M_a2*z) + M_a3 in float64 without fused operations,
the last row of M taken as (0, 0, 0, 1) - the reference multiplies homogeneous columns with BLAS and divides by the last row, which
agrees within rounding (tests/golden/g21_transformations.npz). [n, 4] input is refused (ValueError): the reference appends a fifth row to
it and fails in the matrix product. The two `belvedere_*` constructors of the reference are site constants, not provided:
`read_T_from_file` serves."""
from pathlib import Path
from typing import Union

import numpy as np
import torch

from .._lib import ptr


def check_transform(T, what="transformation"):
    """A finite 4x4 float64 with last row (0, 0, 0, 1), or ValueError; host only."""
    M = np.asarray(T.detach().cpu() if isinstance(T, torch.Tensor) else T, np.float64)
    if M.shape != (4, 4):
        raise ValueError(f"{what} must be 4x4 (got {M.shape})")
    if not np.isfinite(M).all():
        raise ValueError(f"{what} must be finite")
    if not np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError(f"{what} must have (0, 0, 0, 1) in the last row")
    return np.ascontiguousarray(M)


def transform_points(T, x, as_vectors=False, engine=None):
    """`x` [n, 3] under the 4x4 `T` (numpy, or a device tensor of 16 float64), on the device: a new array. `as_vectors` leaves the
    translation out (normals). numpy in, numpy out; a tensor in, a tensor out."""
    from ..engine import default_engine, to_device
    from .point_cloud_filters import MAX_BALL_POINTS
    if not isinstance(T, torch.Tensor):
        T = check_transform(T)
    shape = tuple(x.shape) if hasattr(x, "shape") else np.shape(x)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"points must be [n, 3] (got {shape})")
    if shape[0] > MAX_BALL_POINTS:
        raise ValueError("at most 2^26 points")
    eng = default_engine(engine)
    dev = eng.device
    d_M = T.to(device=dev, dtype=torch.float64).contiguous() if isinstance(T, torch.Tensor) else to_device(T, dev, np.float64)
    d_x = x.to(device=dev, dtype=torch.float64).contiguous() if isinstance(x, torch.Tensor) else to_device(np.ascontiguousarray(x, np.float64), dev, np.float64)
    out = torch.empty_like(d_x)
    eng.ctx.call("im_transform_points", ptr(d_M), ptr(d_x), ptr(out), shape[0], 1 if as_vectors else 0, eng.stream_ptr())
    return out if isinstance(x, torch.Tensor) else out.cpu().numpy()


class Rotrotranslation:
    """A rigid transform in homogeneous coordinates, with the reference's names."""

    def __init__(self, t_mat: np.ndarray) -> None:
        assert isinstance(t_mat, np.ndarray) and t_mat.shape == (4, 4), "t_mat must be a 4x4 numpy array"
        if not np.allclose(t_mat[3], [0, 0, 0, 1]):
            raise ValueError("the last row of a homogeneous transform must be (0, 0, 0, 1)")
        R = t_mat[:3, :3]
        if not np.allclose(np.linalg.inv(R), R.T, rtol=1e-2):
            raise ValueError("the 3x3 block is not a rotation: its inverse differs from its transpose")
        self._t = t_mat

    @property
    def T(self):
        return self._t

    @property
    def T_inv(self):
        return np.linalg.inv(self._t)

    @classmethod
    def read_T_from_file(cls, file: Union[str, Path]):
        """A 4x4 matrix of whitespace-separated values, one row per line."""
        try:
            T = np.loadtxt(file)
        except Exception as e:
            raise ValueError(f"cannot read a matrix from {file}: {e}")
        if not isinstance(T, np.ndarray) or T.shape != (4, 4):
            raise ValueError(f"{file} must hold a 4x4 matrix")
        return cls(T)

    @staticmethod
    def _euclidean(x):
        assert isinstance(x, np.ndarray), "x must be a numpy array"
        if x.ndim != 2 or x.shape[1] != 3:
            raise ValueError(f"x must be [n, 3] in euclidean coordinates (got {x.shape}); homogeneous [n, 4] input is not supported")
        return x

    def _matrix(self, M):
        """M with the last row the constructor accepted within allclose replaced by the exact (0, 0, 0, 1) the kernel assumes."""
        M = np.array(M, np.float64)
        M[3] = (0.0, 0.0, 0.0, 1.0)
        return M

    def transform(self, x: np.ndarray, engine=None) -> np.ndarray:
        """T applied to [n, 3] points on the device: [n, 3]."""
        return transform_points(self._matrix(self.T), self._euclidean(x), engine=engine)

    def transform_inverse(self, x: np.ndarray, engine=None) -> np.ndarray:
        """inv(T) applied to [n, 3] points on the device: [n, 3]."""
        return transform_points(self._matrix(self.T_inv), self._euclidean(x), engine=engine)

    def transform_pcd(self, pcd_path: Union[str, Path], out_path: str = None, inverse: bool = False, engine=None):
        """The cloud of a .ply file under T (or its inverse): a `core.PointCloud` with the colours kept and the normals rotated, written
        to `out_path` when given."""
        from ..core.point_cloud import PointCloud
        try:
            pcd = PointCloud(pcd_path=str(pcd_path))
        except FileNotFoundError:
            raise FileNotFoundError(f"no point cloud at {pcd_path}")
        out = pcd.transform(self._matrix(self.T_inv if inverse else self.T), engine=engine)
        if out_path is not None:
            out.write_ply(out_path)
        return out

    def write_T_mat_to_csv(self, fname: str, sep: str = " "):
        with open(fname, "w") as f:
            f.writelines(sep.join(str(v) for v in row) + "\n" for row in self.T)


def convert_to_homogeneous(x: np.ndarray) -> np.ndarray:
    """2xn or 3xn euclidean coordinates -> 3xn or 4xn homogeneous, by a row of ones; None (and a message) for another number of rows."""
    x = np.array(x)
    ndim, npts = x.shape
    if ndim != 2 and ndim != 3:
        print("convert_to_homogeneous: x must have 2 or 3 rows")
        return None
    return np.concatenate((x, np.ones((1, npts), "float32")), axis=0)


def convert_from_homogeneous(x: np.ndarray) -> np.ndarray:
    """3xn or 4xn homogeneous coordinates -> 2xn or 3xn euclidean, divided by the last row; None (and a message) for another number of rows."""
    x = np.array(x)
    ndim, npts = x.shape
    if ndim != 3 and ndim != 4:
        print("convert_from_homogeneous: x must have 3 or 4 rows")
        return None
    return x[: ndim - 1, :] / x[ndim - 1, :]
