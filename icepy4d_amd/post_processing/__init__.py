"""The reference's `icepy4d.post_processing` on the device: volume variations between epoch clouds (`cloudcompare_fun.DemOfDifference`,
csrc/dod.hip), the polygon crop (`open3d_fun.filter_pcd_by_polyline`), the pairing of a series' clouds (`utils.make_pairs`) and voxel grids with their box meshes
(`voxel_grid.VoxelGrid`, csrc/voxel.hip), triangle meshes (`triangle_mesh.TriangleMesh`, csrc/mesh.hip) and `open3d_fun.MeshingPoisson`,
whose Poisson solve is a hook that `poisson.poisson_reconstruct` fills (a reconstruction on the dense grid of the finest
octree level, csrc/poisson.hip; not Open3D's solver), and the distances between two epoch clouds (`cloud_distance`: cloud-to-cloud and M3C2,
csrc/cloud_distance.hip; the reference has no counterpart) and the ICP that brings them into one frame first (`registration`, csrc/icp.hip)."""
from . import cloud_distance, cloudcompare_fun, open3d_fun, poisson, registration, triangle_mesh, utils, voxel_grid  # noqa: F401
from .open3d_fun import MeshingPoisson  # noqa: F401
from .triangle_mesh import TriangleMesh, read_triangle_mesh  # noqa: F401
from .cloudcompare_fun import DemOfDifference  # noqa: F401
from .voxel_grid import Voxel, VoxelGrid  # noqa: F401
from .utils import find_closest_date_idx, make_pairs  # noqa: F401
from .cloud_distance import CloudDistance, M3C2Result, cloud_to_cloud_distance, m3c2  # noqa: F401
from .poisson import PoissonField, extract_surface, poisson_field, poisson_reconstruct  # noqa: F401
from .registration import ICPConvergenceCriteria, RegistrationResult, evaluate_registration, registration_icp  # noqa: F401
