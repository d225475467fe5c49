"""Voxelization of the clouds of a series, on the device: the reference's `scripts/pcd_postprocessing/voxelization.py` (per epoch a
`VoxelGrid.create_from_point_cloud_within_bounds` over one fixed box, a text file with the centre and the mean colour of every filled
voxel written in a Python loop, and a cube mesh grown by `vox_mesh += cube` once per voxel) as two functions. `voxel_series` uploads the
clouds once, one behind the other, and serves all epochs with one pass of csrc/voxel.hip; `voxelize` is the script: it writes the files.
The script's `draw_geometries` call is not provided. No CPU fallback: without a HIP device these raise.

The definition is `post_processing/voxel_grid.py`'s (tests/voxel_oracle.py, bit-identical). PARITY WITH AN OPEN3D BINARY IS
UNPINNED."""
from pathlib import Path

import numpy as np

from .engine import default_engine
from .post_processing import voxel_grid as VG
from .post_processing.voxel_grid import VoxelGrid, write_triangle_mesh, write_voxel_centers, write_voxel_grid

VOXEL_SIZE = 0.2
BB_MIN = (-100, 130, 60)
BB_MAX = (30, 330, 120)


def voxel_series(clouds, voxel_size=VOXEL_SIZE, bb_min=BB_MIN, bb_max=BB_MAX, engine=None):
    """The `VoxelGrid` of every cloud (paths, `PointCloud`s or [n, 3] arrays; `(points, colors)` pairs for arrays with colours) under the one
    box bb_min .. bb_max. The clouds are uploaded once and go through one device pass; a series over the library's points-per-call limit
    is split. Colours are averaged when every cloud of the series has them."""
    grid = VG.make_grid(np.array(bb_min).astype(np.float64), np.array(bb_max).astype(np.float64), voxel_size)
    host = [VG.cloud_arrays(*c) if isinstance(c, tuple) else VG.cloud_arrays(c) for c in clouds]
    if not host:
        return []
    colours = all(c[1] is not None for c in host)
    host = [(c[0], c[1] if colours else None, None) for c in host]
    eng = default_engine(engine)
    out = [None] * len(host)
    for batch in VG._batches([len(c[0]) for c in host], VG.max_points()):
        results, _ = VG.device_pass(eng, [host[e] for e in batch], grid)
        for e, r in zip(batch, results):
            out[e] = VoxelGrid(grid, r, eng)
    return out


def voxelize(pcd_list, voxel_size=VOXEL_SIZE, bb_min=BB_MIN, bb_max=BB_MAX, out_dir=None, engine=None, write_grid=False, write_mesh=False):
    """The script: per cloud of `pcd_list` (paths of `.ply` files; or `PointCloud`s / arrays, then named cloud_<k>) the file
    `<stem>_voxel_<voxel_size>m.txt` in `out_dir` (default: the directory of the first path) with one line `x,y,z,r,g,b` per filled voxel;
    on request `voxel_grid.ply` and `vox_mesh.ply` of the last cloud, as the script leaves them. Returns the `VoxelGrid`s."""
    pcd_list = list(pcd_list)
    is_path = [isinstance(c, (str, bytes)) or hasattr(c, "__fspath__") for c in pcd_list]
    stems = [Path(c).stem if p else f"cloud_{k}" for k, (c, p) in enumerate(zip(pcd_list, is_path))]
    if out_dir is None:
        if not (pcd_list and is_path[0]):
            raise ValueError("out_dir is needed when the clouds are not files")
        out_dir = Path(pcd_list[0]).parent
    grids = voxel_series(pcd_list, voxel_size, bb_min, bb_max, engine)
    out_dir = Path(out_dir)
    for stem, grid in zip(stems, grids):
        write_voxel_centers(out_dir / f"{stem}_voxel_{voxel_size}m.txt", grid)
    if grids and write_grid:
        write_voxel_grid(out_dir / "voxel_grid.ply", grids[-1])
    if grids and write_mesh:
        write_triangle_mesh(out_dir / "vox_mesh.ply", *grids[-1].to_box_mesh())
    return grids
