"""DSMs and orthophotos (reference `src/icepy4d/utils/dsm_orthophoto.py`): `DSM`, `build_dsm` and `generate_ortophoto` with the
reference's names, signatures, outputs and validation. The binning, the per-cell triangle search and interpolation, and the colouring
run on the device (csrc/dsm.hip: `im_dsm_round`, `im_dsm_group_mean`, `im_dsm_rasterize`, `im_project_colors`); the sorts of the binning
are torch's and the Delaunay triangulation is scipy's qhull on the host, on exactly the points the reference hands it, so the triangle
set is the reference's. Every entry point takes an optional `engine=` (default: the shared engine of device 0); there is no CPU
fallback: without a HIP device the calls raise.

Numerics. The binned points are bit-identical to pandas' group means. Every grid cell takes the lowest simplex index that contains it
(scipy's own inside test and tolerance) and the interpolation in scipy's operation order: z is bit-identical, on every cell, to the
brute-force restatement of that rule (tests/dsm_oracle.py `rasterize`; tests/test_gpu_dsm_edges.py, tests/test_dsm_cpu.py). Against the
reference itself (tests/test_gpu_dsm.py, g12) the NaN mask of the grid is the reference's and z is bit-identical wherever a cell lies
inside a unique triangle; on a shared edge or vertex scipy's directed walk may stop in a neighbouring triangle that contains the cell
as well, and the value then differs in the last bits. Projections, colours and orthophotos from the same DSM are bit-identical."""
from pathlib import Path

import numpy as np
import torch

from ..core.camera import _camera_params, _channel_map
from .._lib import ptr
from ..engine import default_engine, to_device


class DSM:
    """Class to store and manage DSM."""

    def __init__(self, xx, yy, zz, res):
        self.x = xx
        self.y = yy
        self.z = zz
        self.res = res


class _DeviceDSM(DSM):
    """What `build_dsm` returns: a `DSM` whose x / y meshgrids are formed on first access and whose grid also stays on the device,
    so `generate_ortophoto` does not upload it again. `z` is read-only: assigning a new array is fine (it is then uploaded)."""

    def __init__(self, xq, yq, zz, res, device_grid):
        self._xq, self._yq = xq, yq
        self._x = self._y = None
        zz.setflags(write=False)
        self.z, self.res = zz, res
        self._device = device_grid     # (engine, xq, yq, z) on the device
        self._z_host = zz

    @property
    def x(self):
        if self._x is None:
            self._x, self._y = np.meshgrid(self._xq, self._yq)
        return self._x

    @x.setter
    def x(self, v):
        self._x = v

    @property
    def y(self):
        if self._y is None:
            self._x, self._y = np.meshgrid(self._xq, self._yq)
        return self._y

    @y.setter
    def y(self, v):
        self._y = v


def _bin_on_device(eng, pts: np.ndarray, step: float):
    """Rounding, the reference's lexsort, grouping and Kahan means: (x, y, z) float32 of the groups on the device and on the host."""
    dev, n = eng.device, len(pts)
    dp = to_device(pts, dev)
    xr = torch.empty(n, dtype=torch.float32, device=dev)
    yr = torch.empty_like(xr)
    xykey, ykey, zkey = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
    st = eng.stream_ptr()
    eng.ctx.call("im_dsm_round", ptr(dp), n, float(np.float32(step)), ptr(xr), ptr(yr), ptr(xykey), ptr(ykey), ptr(zkey), st)
    # np.lexsort((y, z)): z first, then y, stable; then groupby's order: (x, y), rows kept in that order
    pa = torch.sort(ykey, stable=True).indices
    pb = pa[torch.sort(zkey[pa], stable=True).indices]
    pc = pb[torch.sort(xykey[pb], stable=True).indices]
    bx, by, bz = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
    ng = torch.empty(1, dtype=torch.int64, device=dev)
    eng.ctx.call("im_dsm_group_mean", ptr(dp), ptr(xr), ptr(yr), ptr(xykey), ptr(pb), ptr(pc), n, ptr(bx), ptr(by), ptr(bz), ptr(ng), st)
    G = int(ng.item())
    bx, by, bz = bx[:G], by[:G], bz[:G]
    return (bx, by, bz), (bx.cpu().numpy(), by.cpu().numpy(), bz.cpu().numpy())


def _rasterize(eng, dev_b, host_b, xq, yq, step, fill):
    """qhull on the host (scipy's Delaunay, what `LinearNDInterpolator` builds), the per-cell triangle and z on the device."""
    from scipy.spatial import Delaunay
    bx, by, bz = host_b
    tri = Delaunay(np.ascontiguousarray(np.stack([bx, by], 1), dtype=np.float64))   # raises QhullError as the reference does
    simp = np.ascontiguousarray(tri.simplices, dtype=np.int32)
    trans = np.ascontiguousarray(tri.transform, dtype=np.float64)
    dev = eng.device
    dz = torch.empty((len(yq), len(xq)), dtype=torch.float64, device=dev)
    dxq, dyq = to_device(xq, dev), to_device(yq, dev)
    if dz.numel():
        ds, dt = to_device(simp, dev), to_device(trans, dev)
        bounds = np.ascontiguousarray(np.r_[tri.min_bound, tri.max_bound], dtype=np.float64)
        eng.ctx.call("im_dsm_rasterize", ptr(dev_b[0]), ptr(dev_b[1]), ptr(dev_b[2]), ptr(ds), ptr(dt), len(simp), bounds.ctypes.data,
                     ptr(dxq), len(xq), ptr(dyq), len(yq), float(xq[0]), abs(float(step)), float(yq[0]), abs(float(step)), float(fill),
                     ptr(dz), eng.stream_ptr())
    return dxq, dyq, dz


def build_dsm(points3d, dsm_step=1, xlim=None, ylim=None, interp_method="linear", fill_value=np.nan, save_path=None, make_dsm_plot=False,
              engine=None):
    """`build_dsm` of the reference (`dsm_orthophoto.py:27-174`): bins the points to `dsm_step` (mean z per cell), triangulates the
    bins and interpolates z linearly on the grid np.arange(*xlim, dsm_step) x np.arange(*ylim, dsm_step). Returns a `DSM` with
    z [len(yq), len(xq)] float64, x / y its meshgrids and res = dsm_step. `interp_method` is ignored, as in the reference."""
    # Check dimensions of input array
    assert np.any(np.array(points3d.shape) == 3), "Invalid size of input points"
    if points3d.shape[0] == points3d.shape[1]:
        print("Warning: input vector has just 3 points. Unable to check validity of point dimensions.")
    if points3d.shape[0] == 3:
        points3d = points3d.T
    if save_path is not None:
        import rasterio  # noqa: F401  (the GeoTIFF writer below; raises before any device work when it is missing)
        save_path = Path(save_path)
    if make_dsm_plot:
        import matplotlib.pyplot  # noqa: F401

    pts = np.ascontiguousarray(points3d, dtype=np.float64)
    x, y = pts[:, 0], pts[:, 1]
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        raise ValueError("build_dsm: point coordinates must be finite")
    if xlim is None:
        xlim = [np.floor(x.min()), np.ceil(x.max())]
    if ylim is None:
        ylim = [np.floor(y.min()), np.ceil(y.max())]
    xq = np.arange(xlim[0], xlim[1], dsm_step)
    yq = np.arange(ylim[0], ylim[1], dsm_step)

    eng = default_engine(engine)
    dev_b, host_b = _bin_on_device(eng, pts, dsm_step)
    if isinstance(fill_value, str) and fill_value == "mean":
        fill_value = host_b[2].mean()
    dxq, dyq, dz = _rasterize(eng, dev_b, host_b, np.ascontiguousarray(xq, np.float64), np.ascontiguousarray(yq, np.float64),
                              dsm_step, fill_value)
    dsm_grid = dz.cpu().numpy()
    dsm = _DeviceDSM(xq, yq, dsm_grid, dsm_step, (eng, dxq, dyq, dz))

    if make_dsm_plot:
        _plot_dsm(dsm, points3d, save_path)
    if save_path is not None:
        _write_dsm_geotiff(dsm, xlim, ylim, dsm_step, fill_value, save_path)
    return dsm


def generate_ortophoto(image, dsm, camera, xlim=None, ylim=None, res=None, save_path=None, engine=None):
    """`generate_ortophoto` of the reference (`dsm_orthophoto.py:179-233`): every DSM cell with a z is projected into the oriented
    `image` (uint8, BGR as cv2 reads it) and coloured bilinearly; [rows, cols, 3] uint8 RGB, black where z is NaN. `camera` is any object
    with `.K`, `.dist`, `.R` and `.t`. A DSM from `build_dsm` is used from the device; any other `DSM` is uploaded."""
    if save_path is not None:
        import rasterio  # noqa: F401  (raises before any device work when it is missing)
    if res is None:
        res = dsm.res
    assert image.ndim == 3, "invalid input image. Image has not 3 channel"
    image = np.asarray(image)
    if image.dtype != np.uint8:
        raise ValueError(f"generate_ortophoto: a uint8 image is expected (got {image.dtype})")
    chmap = _channel_map(image, True)
    cam = _camera_params(camera)
    eng = default_engine(engine)
    dev = eng.device
    zz = dsm.z
    rows, cols = np.shape(zz)
    if isinstance(dsm, _DeviceDSM) and dsm._device[0] is eng and zz is dsm._z_host:
        _, dxq, dyq, dz = dsm._device
        px, sx, py, sy, pz = ptr(dxq), (0, 1), ptr(dyq), (1, 0), ptr(dz)
    else:
        tx, ty, tz = (to_device(np.broadcast_to(np.asarray(a, np.float64), (rows, cols)), dev) for a in (dsm.x, dsm.y, zz))
        px, sx, py, sy, pz = ptr(tx), (cols, 1), ptr(ty), (cols, 1), ptr(tz)
    h, w, cin = image.shape
    img = to_device(image, dev)
    out = torch.empty((rows, cols, 3), dtype=torch.uint8, device=dev)
    eng.ctx.call("im_project_colors", px, sx[0], sx[1], py, sy[0], sy[1], pz, cols, 1, rows, cols, 1, cam.ctypes.data, ptr(img), h, w, cin,
                 chmap.ctypes.data, 3, None, None, ptr(out), eng.stream_ptr())
    ortophoto = out.cpu().numpy()
    if save_path is not None:
        if xlim is None:
            xlim = [dsm.x[0, 0], dsm.x[0, -1]]
        if ylim is None:
            ylim = [dsm.y[0, 0], dsm.y[-1, 0]]
        _write_ortho_geotiff(ortophoto, xlim, ylim, res, save_path)
    return ortophoto


# ---- host-side outputs of the reference (`dsm_orthophoto.py:102-174`, `:213-231`). Never executed in this repository's tests:
# rasterio is not a dependency, and the plots are matplotlib only.
def _plot_dsm(dsm, points3d, save_path):
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots()
    dsm_plt = ax.contourf(dsm.x, dsm.y, dsm.z)
    ax.scatter(points3d[:, 0], points3d[:, 1], s=5, c=points3d[:, 2], marker="o", cmap="viridis", alpha=0.4, edgecolors="k")
    ax.axis("equal")
    ax.invert_yaxis()
    cbar = plt.colorbar(dsm_plt, ax=ax)
    cbar.set_label("z")
    ax.set_xlabel("x")
    ax.set_ylabel("y")
    ax.set_title("DSM interpolated from point cloud on plane X-Y")
    fig.tight_layout()
    if save_path is not None:
        plt.savefig(save_path.parent.joinpath(save_path.stem + "_plot.png"), bbox_inches="tight")


def _write_dsm_geotiff(dsm, xlim, ylim, dsm_step, fill_value, save_path):
    import rasterio
    from rasterio.transform import Affine
    save_path.parent.mkdir(parents=True, exist_ok=True)
    dsm_grid = dsm.z
    transform = Affine.translation(dsm.x[0, 0], dsm.y[0, 0]) * Affine.scale(dsm_step, -dsm_step)
    mask = np.invert(np.isnan(dsm_grid))
    with rasterio.open(save_path, "w", driver="GTiff", height=dsm_grid.shape[0], width=dsm_grid.shape[1], count=1, dtype="float32",
                       transform=transform) as dst:
        dst.write(dsm_grid, 1)
        if fill_value is not None:
            dst.write_mask(mask)
    if fill_value is not None:
        with rasterio.open(save_path.parent / (save_path.stem + "_msk.tif"), "w", driver="GTiff", height=dsm_grid.shape[0],
                           width=dsm_grid.shape[1], count=1, dtype="float32", transform=transform) as dst:
            dst.write(mask, 1)


def _write_ortho_geotiff(ortophoto, xlim, ylim, res, save_path):
    import rasterio
    from rasterio.transform import Affine
    save_path = Path(save_path)
    save_path.mkdir(parents=True, exist_ok=True)
    transform = Affine.translation(xlim[0] - res / 2, ylim[0] - res / 2) * Affine.scale(res, -res)
    with rasterio.open(save_path, "w", driver="GTiff", height=ortophoto.shape[0], width=ortophoto.shape[1], count=3, dtype="uint8",
                       transform=transform) as dst:
        dst.write(np.moveaxis(ortophoto, -1, 0))
