"""ctypes binding of libicematch.so (C ABI in include/icematch.h).

The library is the product: there is no Python/torch fallback. If it is missing or fails to load, every
entry point raises. torch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("ICEMATCH_LIB") or os.path.join(CSRC, "libicematch.so")  # env override: A/B builds

_lib: Optional[C.CDLL] = None


class IcematchError(RuntimeError):
    """A call into libicematch.so returned non-zero (`Context.check`): out of device memory, a HIP error, a guard failure, bad arguments.
    Distinct from other RuntimeErrors (torch's, e.g. an `interpolate` size error out of a bad `resize` option) so that callers can tell a
    library / device failure - never to be swallowed - from a failure of an option (`matching/matchers.py` q7, `sequence.py`)."""

    def __init__(self, what: str, rc: int, message: str):
        super().__init__(f"{what} failed ({rc}): {message}")
        self.what, self.rc = what, rc


class LightGlueConf(C.Structure):
    _fields_ = [("depth_confidence", C.c_double), ("width_confidence", C.c_double),
                ("filter_threshold", C.c_double), ("n_layers", C.c_int), ("pruning_min_kpts", C.c_int)]


class SuperGlueConf(C.Structure):
    _fields_ = [("sinkhorn_iterations", C.c_int), ("match_threshold", C.c_double), ("n_layers", C.c_int)]


_P = C.c_void_p
_I = C.c_int
_F = C.c_float
_D = C.c_double
_L = C.c_longlong

# name -> argtypes; every symbol declared in include/icematch.h
SIGNATURES = {
    "im_version": [],
    "im_ctx_create": [_I, C.POINTER(_P)],
    "im_ctx_destroy": [_P],
    "im_last_error": [_P],
    "im_ctx_reserve": [_P, _I, _I, _I, _I],
    "im_profile_begin": [_P],
    "im_profile_end": [_P, C.c_char_p, C.c_size_t],
    "im_set_tensor": [_P, C.c_char_p, C.c_char_p, _P, C.c_size_t],
    "im_finalize_weights": [_P, C.c_char_p],
    "im_superpoint_forward": [_P, _P, _I, _I, _I, _I, _I, _F, _I, _I, _I, _P, _P, _P, _P, _P],
    "im_superpoint_candidates": [_P, _I, _P, _P],
    "im_lightglue_forward": [_P, _P, _P, _P, _P, C.POINTER(LightGlueConf), _P, _P, _P, _P, _P],
    "im_lightglue_forward_pairs": [_P, _I, _P, _P, _P, _P, C.POINTER(LightGlueConf), _P, _P, _P, _P, _P],
    "im_pack_records": [_P, _I, _P, _P, _P, _P, _I, _P, _P, _P],
    "im_superglue_forward": [_P, _P, _P, _P, _P, _P, C.POINTER(SuperGlueConf), _P, _P, _P, _P],
    "im_pack_record": [_P, _P, _P, _P, _P, _I, _P, _P],
    "im_debug_read": [_P, C.c_char_p, _P, C.c_size_t, _P],
    "im_debug_clock_probe": [_P, _I, _P, _P],
    "im_debug_guard_failures": [],
    "im_debug_guard_selftest": [_P, _P],
    "im_debug_guards_check": [_P, _P],
    "im_pyr_down": [_P, _P, _P, _I, _I, _I, _I, _P],
    "im_pyr_up": [_P, _P, _P, _I, _I, _I, _I, _P],
    "im_gemm_nt": [_P, _P, _P, _P, _P, _I, _I, _I, _F, _I, _P],
    "im_ffn_fused": [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P],
    "im_conv3x3": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "im_conv3x3_winograd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "im_flash_attn": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "im_block_proj_attn": [_P, _I, _P, _P, _P, _P, _P, _F, _P, _P, _I, _I, _P, _P, _P, _P, _P, _F, _P],
    "im_nms": [_P, _P, _P, _I, _I, _I, _I, _P],
    "im_select_topk": [_P, _P, _I, _I, _I, _I, _F, _I, _P, _P, _P, _P],
    "im_sample_descriptors": [_P, _P, _I, _I, _I, _P, _P, _P, _P],
    "im_assign_from_sim": [_P, _P, _I, _I, _I, _P, _P, _F, _P, _P, _P, _P, _P],
    "im_log_optimal_transport": [_P, _P, _I, _I, _I, _F, _I, _P, _P],
    "im_merge_tile_matches": [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "im_gather_rows": [_P, _P, _I, _P, _I, _P, _P],
    "im_ransac_fundamental": [_P, _P, _P, _I, _I, C.c_double, C.c_uint, _P, _P, _P, _P],
    "im_ransac_essential": [_P, _P, _P, _I, _I, C.c_double, C.c_uint, _P, _P, _P, _P],
    "im_triangulate_linear": [_P, _P, _P, _P, _P, _I, _P, _P],
    "im_forient": [_P, _P, _I, _I, _I, _I, _P, _P],
    "im_template_match_oc": [_P, _P, _I, _I, _P, _I, _I, _I, _P, _P, _I, _I, _I, _I, _P, _P],
    "im_template_match_corr": [_P, _P, _I, _I, _P, _I, _I, _I, _P, _P, _I, _I, _I, _I, _P, _P],
    "im_dsm_round": [_P, _P, _L, _F, _P, _P, _P, _P, _P, _P],
    "im_dsm_group_mean": [_P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P, _P],
    "im_dsm_rasterize": [_P, _P, _P, _P, _P, _P, _L, _P, _P, _I, _P, _I, _D, _D, _D, _D, _D, _P, _P],
    "im_project_colors": [_P, _P, _L, _L, _P, _L, _L, _P, _L, _L, _I, _I, _I, _P, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P],
    "im_undistort_points": [_P, _P, _L, _P, _P, _P],
    "im_triangulate_iterative": [_P, _P, _P, _I, _L, _P, _P, _P, _P, _D, _I, _P, _P, _P, _P, _P],
    "im_triangulate_table": [_P, _P, _I, _I, _P, _I, _I, _D, _I, _L, _P, _P, _P, _P, _P, _P],
    "im_binned_lds_capacity": [],
    "im_binned_cells": [_P, _P, _L, _I, _P, _P, _P, _P, _P, _I, _P, _P],
    "im_binned_stats": [_P, _P, _P, _L, _I, _L, _P, _I, _P, _P, _P],
    "im_tracked_points": [_P, _P, _P, _L, _P, _I, _P, _P, _P, _L, _P, _P, _P, _I, _P, _P, _P, _P, _P],
    "im_undistort_image": [_P, _P, _I, _I, _I, _I, _P, _P, _P],
    "im_warp_perspective": [_P, _P, _I, _I, _I, _I, _P, _I, _I, _P, _P],
    "im_knn_max_cells": [],
    "im_knn_cells": [_P, _P, _L, _P, _I, _I, _I, _P, _P],
    "im_knn_cell_ranges": [_P, _P, _L, _L, _P, _P],
    "im_knn_self": [_P, _P, _P, _P, _L, _P, _I, _I, _I, _I, _D, _P, _P, _P, _P, _P, _P, _P],
    "im_ball_features": [_P, _P, _P, _P, _L, _P, _I, _I, _I, _D, _P, _I, _P, _P, _P, _P, _P, _P, _P],
    "im_knn_cross": [_P, _P, _P, _P, _L, _P, _I, _I, _I, _P, _P, _L, _I, _D, _P, _P, _P, _P, _P],
    "im_ball_cross": [_P, _P, _P, _P, _L, _P, _I, _I, _I, _P, _P, _L, _D, _P, _P, _P, _P, _P, _P],
    "im_cyl_stats": [_P, _P, _P, _P, _L, _P, _I, _I, _I, _P, _P, _P, _L, _D, _D, _P, _P, _P, _P, _P, _P],
    "im_m3c2_finish": [_P, _P, _P, _P, _P, _L, _D, _D, _I, _P, _P, _P, _P],
    "im_icp_chunk": [],
    "im_transform_points": [_P, _P, _P, _P, _L, _I, _P],
    "im_icp_accumulate": [_P, _P, _L, _P, _P, _L, _P, _P, _P, _I, _L, _P, _P],
    "im_icp_finish": [_P, _P, _L, _L, _P, _P, _I, _P, _P],
    "im_ba_chunk": [],
    "im_ba_accumulate": [_P, _P, _I, _L, _L, _P, _P, _P, _P, _P, _P, _P, _P],
    "im_ba_solve": [_P, _P, _I, _L, _P, _P, _P, _P, C.c_uint, _P, _P],
    "im_ba_step_points": [_P, _P, _I, _L, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "im_ba_decide": [_P, _P, _I, _L, _P, _P, _P, _P, _P, _P, _P, _L, _P],
    "im_ba_residuals": [_P, _P, _I, _L, _L, _P, _P, _P, _P, _P, _P],
    "im_dense_tile_w": [],
    "im_dense_tile_h": [],
    "im_dense_sweep": [_P, _P, _I, _I, _P, _I, _I, _P, _P, _D, _D, _I, _I, _L, _D, _P, _P, _P, _P],
    "im_dense_consistency": [_P, _P, _P, _I, _I, _P, _P, _I, _I, _P, _D, _I, _P, _P],
    "im_dense_cloud": [_P, _P, _P, _P, _P, _I, _I, _I, _P, _L, _P, _P, _P, _P, _P, _P],
    "im_dense_sgm_max_planes": [],
    "im_dense_costs": [_P, _P, _I, _I, _P, _I, _I, _P, _P, _D, _D, _I, _I, _L, _P, _P],
    "im_dense_sgm": [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P],
    "im_dense_sgm_choose": [_P, _P, _P, _I, _I, _I, _D, _D, _D, _P, _P, _P, _P],
    "im_dense_fuse_link": [_P, _P, _P, _P, _I, _I, _P, _P, _P, _I, _I, _P, _D, _P, _P, _P, _P, _P, _P],
    "im_dense_fuse_rest": [_P, _P, _P, _I, _I, _P, _P, _I, _I, _P, _D, _P, _P, _P],
    "im_dense_slant": [_P, _P, _P, _I, _I, _D, _I, _D, _I, _P, _P, _P],
    "im_dense_refine": [_P, _P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _D, _I, _L, _I, _I, _P, _P, _P, _P],
    "im_flow_match": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _D, _P, _P, _P, _P, _P, _P],
    "im_flow_check": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _D, _P, _P],
    "im_flow_lift": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _I, _I, _P, _D, _D, _P, _P, _P, _P],
    "im_flow_prior_up": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P],
    "im_flow_match_field": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _L, _D, _P, _P, _P, _P, _P, _P, _P],
    "im_depth_tile_w": [],
    "im_depth_tile_h": [],
    "im_depth_components": [_P, _P, _I, _I, _I, _I, _P, _P, _P],
    "im_depth_drop_small": [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P],
    "im_depth_fill_holes": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _D, _D, _I, _P, _P, _P, _P, _P, _P],
    "im_dod_chunk": [],
    "im_dod_max_cells": [],
    "im_dod_max_batch_cells": [],
    "im_dod_bounds": [_P, _P, _P, _I, _I, _P, _P, _P],
    "im_dod_keys": [_P, _P, _P, _I, _P, _I, _I, _D, _P, _P, _P, _P],
    "im_dod_reduce": [_P, _P, _P, _I, _P, _I, _I, _D, _P, _P, _P, _P, _P, _P],
    "im_crop_polygon": [_P, _P, _L, _I, _I, _P, _I, _I, _P, _P, _P, _P],
    "im_voxel_max_points": [],
    "im_voxel_bounds": [_P, _P, _P, _I, _P, _P],
    "im_voxel_keys": [_P, _P, _P, _I, _P, _I, _P, _P, _P],
    "im_voxel_reduce": [_P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "im_voxel_mesh_corners": [_P, _P, _P, _L, _P, _P],
    "im_voxel_mesh": [_P, _P, _L, _P, _P, _P, _P, _P, _P, _P, _P],
    "im_mesh_max_items": [],
    "im_mesh_hull_chunk": [],
    "im_mesh_select": [_P, _P, _L, _P, _L, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P],
    "im_mesh_triangle_keys": [_P, _P, _L, _P, _P, _P],
    "im_mesh_vertex_keys": [_P, _P, _L, _P, _P, _P, _P],
    "im_mesh_edge_keys": [_P, _P, _L, _P, _P],
    "im_mesh_first_of_segment": [_P, _L, _P, _P, _P, _P, _P, _P, _P],
    "im_mesh_edge_census": [_P, _P, _L, _P, _P],
    "im_mesh_in_hull": [_P, _P, _L, _P, _I, _P, _P],
    "im_mesh_sample_table": [_P, _P, _L, _P, _L, _L, _P, _P, _P, _P],
    "im_mesh_sample": [_P, _P, _L, _P, _L, _P, _L, _L, _P, _P, _P, _P, _P, _P, _P],
    "im_poisson_max_depth": [],
    "im_poisson_max_points": [],
    "im_poisson_splat": [_P, _P, _P, _L, _P, _I, _P, _P],
    "im_poisson_divergence": [_P, _P, _I, _D, _P, _P],
    "im_poisson_jacobi": [_P, _P, _P, _I, _D, _P, _P],
    "im_poisson_restrict": [_P, _P, _P, _I, _D, _P, _P, _P],
    "im_poisson_prolong": [_P, _P, _I, _P, _P],
    "im_poisson_coarse": [_P, _P, _D, _P, _P],
    "im_poisson_reduce": [_P, _P, _P, _L, _P, _P],
    "im_poisson_census": [_P, _P, _D, _I, _P, _P, _P, _P],
    "im_poisson_extract": [_P, _P, _P, _D, _I, _P, _P, _P, _L, _L, _P, _P, _P, _P],
}


def build(force: bool = False) -> str:
    """Compile libicematch.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, capture_output=True)
    r = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building libicematch.so failed:\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}")
    return LIB_PATH


def load() -> C.CDLL:
    """Load the library (no compute is triggered). Raises if it is absent: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64: it must be the HIP runtime of the process (device pointers and streams
    # are shared with torch), so torch is imported before the library's NEEDED libamdhip64.so.7 is resolved.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           f"(there is no CPU/torch fallback for the matching hot path)")
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is missing
        fn.argtypes = argtypes
        fn.restype = C.c_char_p if name == "im_last_error" else (None if name == "im_ctx_destroy" else C.c_int)
    _lib = lib
    return lib


def ptr(t) -> int:
    """Device (or host) pointer of a torch tensor / numpy array; None -> NULL."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return t.data_ptr()
    return t.ctypes.data


def stream_ptr(device=None) -> Optional[int]:
    """The current HIP stream of `device` (a torch device or index; None = the process's current device). Callers that hold an
    engine pass its device: the stream must belong to the device the context's buffers live on, whatever device is current."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


class Context:
    """RAII wrapper of `im_ctx`."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = _P()
        rc = self.lib.im_ctx_create(device, C.byref(h))
        if rc != 0:
            raise RuntimeError(f"im_ctx_create(device={device}) failed with {rc} (is a HIP device visible?)")
        self.h = h
        self.device = device

    def check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.im_last_error(self.h)
            raise IcematchError(what, rc, msg.decode() if msg else "")

    def call(self, name: str, *args):
        self.check(getattr(self.lib, name)(self.h, *args), name)

    def close(self):
        if getattr(self, "h", None):
            self.lib.im_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
