"""Writes tests/golden/g19_voxel.npz: the reference's voxelization script (`scripts/pcd_postprocessing/voxelization.py`: `voxelize`) run on
one small synthetic coloured epoch.

    python tools/gen_golden_voxel.py REFERENCE_ROOT

The reference script is loaded from its file, unchanged, and run with a temporary directory as the working directory that holds
`test/voxelization/dense_2022_05_01.ply`. Open3D is not installed, so `open3d` is a stub and THE STUB IS NOT OPEN3D: it is
tests/voxel_oracle.py, the numpy restatement of this project's own definition of a voxel grid, behind Open3D's names
(`geometry.VoxelGrid`, `geometry.TriangleMesh.create_box / paint_uniform_color / translate / scale / += / merge_close_vertices`, `io`,
`visualization.draw_geometries` as a no-op). `tqdm` is a stub that passes its iterable through.
The voxel indices and colours of this fixture are therefore the restatement's, not Open3D's. What the fixture pins is the reference's own
part: the arguments it passes (0.2 and its two bounds as float64), the text of its per-voxel lines, the name of its text file, and the
chain translate(index, relative=False), translate(0.5), scale(voxel_size, 0), translate(origin), merge_close_vertices its mesh goes through.
Input: a seeded front of 3000 points over 6 m x 4 m inside the script's box, 120 more outside it, colours stored as uchar. Coordinates are
multiples of 2^-10. Fixed zip timestamps: the file regenerates byte for byte."""
import importlib.util
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxel_oracle as O  # noqa: E402

OUT = O.GOLDEN
STEM = "dense_2022_05_01"
N_INSIDE, N_OUTSIDE = 3000, 120


def _save(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def cloud():
    """a steep front inside the script's box (-100..30, 130..330, 60..120) and a few points around it, outside"""
    rng = np.random.default_rng(2022)
    y, z = rng.uniform(200.0, 206.0, N_INSIDE), rng.uniform(80.0, 84.0, N_INSIDE)
    x = -20.0 + 0.5 * np.sin(y / 1.5) + 0.25 * (z - 80.0) + rng.normal(0, 0.02, N_INSIDE)
    inside = np.stack([x, y, z], 1)
    outside = rng.uniform((-140.0, 100.0, 40.0), (70.0, 360.0, 140.0), (4 * N_OUTSIDE, 3))
    lo, hi = np.array([-100.0, 130.0, 60.0]), np.array([30.0, 330.0, 120.0])
    outside = outside[~((outside >= lo) & (outside <= hi)).all(1)][:N_OUTSIDE]
    pts = np.concatenate([inside, outside])
    pts = np.round(pts[rng.permutation(len(pts))] * 1024.0) / 1024.0
    col = rng.integers(0, 256, (len(pts), 3)).astype(np.uint8)
    return pts, col


def main(ref_root):
    from icepy4d_amd.core.point_cloud import PointCloud
    o3d = types.ModuleType("open3d")
    o3d.geometry, o3d.io, o3d.visualization = O.geometry, O.io, O.visualization
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda it, *a, **k: it
    stubs = {"open3d": o3d, "tqdm": tq}
    name = "reference_voxelization"
    saved = {k: sys.modules.get(k) for k in list(stubs) + [name]}
    sys.modules.update(stubs)
    calls = []
    create = O.VoxelGrid.create_from_point_cloud_within_bounds

    def recording(pcd, voxel_size, min_bound, max_bound):
        calls.append((voxel_size, np.array(min_bound), np.array(max_bound)))
        return create(pcd, voxel_size, min_bound, max_bound)

    O.VoxelGrid.create_from_point_cloud_within_bounds = staticmethod(recording)
    O.WRITTEN.clear()
    pts, col = cloud()
    cwd = os.getcwd()
    try:
        with tempfile.TemporaryDirectory() as tmp:
            work = os.path.join(tmp, "test", "voxelization")
            PointCloud(points3d=pts, points_col=col / 255.0).write_ply(os.path.join(work, STEM + ".ply"))
            spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, "scripts/pcd_postprocessing/voxelization.py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[name] = mod
            spec.loader.exec_module(mod)
            os.chdir(tmp)
            mod.voxelize()
            os.chdir(cwd)
            texts = sorted(f for f in os.listdir(work) if f.endswith(".txt"))
            assert texts == [f"{STEM}_voxel_0.2m.txt"], texts
            with open(os.path.join(work, texts[0]), "rb") as f:
                text = f.read()
    finally:
        os.chdir(cwd)
        O.VoxelGrid.create_from_point_cloud_within_bounds = staticmethod(create)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert len(calls) == 1 and all(a.dtype == np.float64 for a in calls[0][1:]), calls
    grid, mesh = O.WRITTEN["voxel_grid.ply"], O.WRITTEN["vox_mesh.ply"]
    V = len(grid.result["counts"])
    assert grid.result["dropped"] == N_OUTSIDE and len(text.splitlines()) == V and len(mesh.triangles) == 12 * V
    g = {"points": pts, "colors_u8": col, "voxel_size": np.array([calls[0][0]], np.float64), "bb_min": calls[0][1], "bb_max": calls[0][2],
         "text": np.frombuffer(text, np.uint8), "text_name": np.frombuffer(texts[0].encode("ascii"), np.uint8),
         "grid_index": grid.result["grid_index"], "voxel_colors": grid.result["colors"], "counts": grid.result["counts"],
         "mesh_vertices": mesh.vertices, "mesh_vertex_colors": mesh.vertex_colors, "mesh_triangles": mesh.triangles.astype(np.int32)}
    _save(OUT, g)
    print(f"{V} voxels, {len(mesh.vertices)} mesh vertices, {len(text)} bytes of text")
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.0f} KB)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/gen_golden_voxel.py REFERENCE_ROOT  (a checkout of franioli/icepy4d)")
    main(sys.argv[1])
