"""Meshing of the clouds of a series: the reference's `scripts/pcd_postprocessing/point_cloud_meshing.py` (per `dense_*.ply` a
`MeshingPoisson(pcd, out_dir, cfg).run()` that leaves `sampled_{date}.ply`, which `volume_variations.dod_series` reads) as one function.
In `mesh_series` the Poisson solve is the caller's (`reconstruct`, or `cfg["mesh_path"]`: see `post_processing/open3d_fun.py:
MeshingPoisson`); `poisson_mesh_series` binds it to the dense-grid reconstruction of `post_processing/poisson.py` (csrc/poisson.hip).
The mesh filters, the hull crop, the sampling and the polygon crop run on the device (csrc/mesh.hip). No CPU fallback."""
from functools import partial
from pathlib import Path

from .engine import default_engine
from .post_processing.open3d_fun import MeshingPoisson
from .post_processing.poisson import poisson_reconstruct

CFG = {
    "do_SOR": False,
    "poisson_depth": 9,
    "min_mesh_denisty": 9,
    "save_mesh": False,
    "sample_mesh": True,
    "num_sampled_points": 4 * 10**6,
    "crop_polyline_path": "data/crop_polyline.poly",
}


def mesh_series(paths, out_dir, cfg=None, reconstruct=None, engine=None):
    """Runs `MeshingPoisson` over every cloud of `paths` with the script's configuration `CFG` overridden by `cfg`, all on one engine.
    Returns the paths of the sampled clouds (`out_dir/sampled_{date}.ply`) in the order of `paths`."""
    paths = [Path(p) for p in paths]
    cfg = {**CFG, **(cfg or {})}
    if not paths:
        return []
    eng = default_engine(engine)
    out = []
    for pcd in paths:
        m = MeshingPoisson(pcd, out_dir=out_dir, cfg=cfg, reconstruct=reconstruct, engine=eng)
        if not m.run():
            raise RuntimeError(f"Unable to mesh point cloud {pcd}")
        out.append(Path(out_dir) / f"sampled_{pcd.stem[pcd.stem.find('202'):]}.ply")
    return out


def poisson_mesh_series(paths, out_dir, cfg=None, engine=None):
    """`mesh_series` with the hook bound to `poisson_reconstruct` on the same engine: from `dense_*.ply` to `sampled_{date}.ply` without
    Open3D. `cfg["poisson_depth"]` is the depth of the dense grid (at most 9)."""
    eng = default_engine(engine) if paths else engine
    return mesh_series(paths, out_dir, cfg=cfg, reconstruct=partial(poisson_reconstruct, engine=eng), engine=eng)
