"""The reference's `icepy4d.post_processing` on the device: volume variations between epoch clouds (`cloudcompare_fun.DemOfDifference`,
csrc/dod.hip), the polygon crop (`open3d_fun.filter_pcd_by_polyline`) and the pairing of a series' clouds (`utils.make_pairs`).
`MeshingPoisson` is not provided."""
from . import cloudcompare_fun, open3d_fun, utils  # noqa: F401
from .cloudcompare_fun import DemOfDifference  # noqa: F401
from .utils import find_closest_date_idx, make_pairs  # noqa: F401
