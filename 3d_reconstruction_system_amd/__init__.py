"""MI355X-native depth -> world point-cloud fusion (drop-in for the hot path of
rainfall1998/3D_reconstruction_system: transfer/pixel_to_camera.py, transfer/camera_to_world.py,
other_tools/transfer_T_icp.py).

The directory name is not a Python identifier; import it with
    r3d = importlib.import_module("3d_reconstruction_system_amd")

Every batch of points is computed in libr3d_hip.so (hand-written gfx950 HIP kernels behind the C ABI of
include/r3d.h).  There is no CPU path for batches: without the library or without an MI355X the compute
entry points raise.  What stays on the host is what SURVEY 8(b) puts there -- quaternion -> Rinv, 4x4 parsing,
text formatting / parsing and PNG decoding (native C++ in the same library) -- plus the reference's one-point
helper `point_camera(p1, r_inverse, t)` for up to 64 points (camera_to_world.py:57-59 is a single np.dot).
"""
from ._lib import (R3DError, R3DLibraryMissing, LIB_PATH, load as load_library,  # noqa: F401
                   DEPTH_U8, DEPTH_U16, DEPTH_F32, F32, F64)
from .device import Context, Camera, DeviceBuffer, default_context  # noqa: F401
from .fusion import (REF_INTRINSICS, unproject, fuse_frames, fuse_frames_rgb, se3_apply, apply_T,  # noqa: F401
                     unproject_device, fuse_frames_device, fuse_frames_rgb_device, fuse_frames_voxel_device,
                     apply_T_device)
from .poses import (scipy_transfer, get_r, pose_table, pose_to_T, read_pose_file, get_T, write_T,  # noqa: F401
                    str_tofloat)
from .voxelmap import VoxelGrid, DownSampled, voxel_down_sample  # noqa: F401
from .outliers import (knn, remove_statistical_outlier, remove_radius_outlier, StatisticalOutliers,  # noqa: F401
                       RadiusOutliers)
from .normals import (Normals, estimate_normals, estimate_normals_device, estimate_covariances,  # noqa: F401
                      fused_viewpoints)
from .segmentation import PlaneSegment, segment_plane, segment_planes, segment_plane_device  # noqa: F401
from .registration import (Fpfh, Matches, RansacResult, compute_fpfh, compute_fpfh_device, match_features,  # noqa: F401
                           registration_ransac, register_global, register_colored)
from .colored_icp import ColourGradients, colour_gradients, colour_gradients_device, icp_colored  # noqa: F401
from .posegraph import (PoseGraph, evaluate_registration, registration_information, registration_sums_device,  # noqa: F401
                        register_multiway)
from .tsdf import TSDFVolume, poses_w2c  # noqa: F401
from .surface import volume_for_cloud, reconstruct_surface  # noqa: F401
from .consistency import (window_sources, depth_consistency, depth_consistency_device, fuse_frames_consistent,  # noqa: F401
                          compact_rows_device)
from .mesh import (MeshComponents, mesh_components, mesh_components_device, remove_small_components,  # noqa: F401
                   remove_small_components_device, mesh_adjacency, mesh_adjacency_device, smooth_mesh, smooth_mesh_device,
                   compute_vertex_normals, vertex_normals_device, smooth_factors)
from . import mesh  # noqa: F401
from .evaluation import (MeshIndex, cloud_to_cloud_distance, cloud_to_mesh_distance, distance_stats, distance_colors,  # noqa: F401
                         evaluate_reconstruction, cloud_to_cloud_distance_device, distance_stats_device, distance_colors_device)
from .tracking import TrackDevice, track_sums  # noqa: F401
from . import cloud_io, device_text  # noqa: F401

__version__ = "0.2.0"
