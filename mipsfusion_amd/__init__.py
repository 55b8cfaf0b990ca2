"""MI355X-native implementation of the MIPS-Fusion render-and-optimise hot path.

Host side (this package) mirrors the reference's ``model.scene_rep`` / ``model.decoder`` /
``model.encodings`` interfaces; the arithmetic runs in hand-written HIP kernels for gfx950
behind the C ABI declared in ``include/mipsf.h`` (``mipsfusion_amd/csrc``).  There is no CPU
fallback: using an operator without the built library or without a GPU raises.
"""
__version__ = "0.1.0"

_MESH = ("marching_cubes", "extract_mesh", "extract_mesh2", "Mesh", "save_ply", "load_ply")
_SCENE_MESH = ("SubMap", "FusedVolume", "fuse_volume", "extract_scene_mesh", "submap_from_mesh", "voxel_occupancy", "point_mask")
_POSE_CORRECTOR = ("cloud_from_rays", "estimate_normals", "registration_icp", "switch_pose_rectifying", "IcpResult")
_POSE_GRAPH = ("adjacent_pairs", "global_ba_gate", "build_edges", "pose_graph_enqueue", "pose_graph_optimize", "rebase",
               "PoseGraphResult")
_SUBMAP_MANAGER = ("SubmapManager", "Decision", "derive_schedule", "frame_stats_enqueue", "overlap_enqueue")
_EVALUATE = ("sample_surface", "nearest_distance", "distance_stats", "reconstruction_metrics", "cull_to_views", "ReconMetrics",
             "DistanceStats")
_MESH_RENDER = ("render_mesh_depth", "depth_l1", "visible_points", "DepthMetrics", "render_mesh", "vertex_normals", "mesh_render_metrics",
                "MeshRender", "MeshRenderMetrics")
_TSDF = ("TSDFVolume", "TSDFCounts", "tsdf_mesh_from_frames", "mesh_from_rendered_depth", "Raycast", "TrackResult", "tsdf_odometry",
         "ColorTrackResult", "RemoveCounts", "ReintegrateCounts")
_SPARSE_TSDF = ("SparseTSDFVolume", "SparseTSDFCounts", "SparseRemoveCounts", "SparseReintegrateCounts", "ReleaseCounts", "RestoreCounts", "BrickArchive", "sparse_tsdf_mesh_from_frames", "sparse_tsdf_odometry")
# (the function image_metrics.image_metrics is reached through its module: the package attribute of that name IS the module)
_IMAGE_METRICS = ("psnr", "ssim", "ms_ssim", "render_metrics", "gaussian_window", "ImageMetrics", "RenderMetrics")
_TRAJECTORY = ("align_trajectory", "trajectory_metrics", "TrajectoryMetrics")


def __getattr__(name):
    # the mesh interface (mipsfusion_amd/mesh.py), resolved on first use so that importing the package stays free of torch
    if name in _MESH:
        from . import mesh
        return getattr(mesh, name)
    if name in _SCENE_MESH:                 # the scene as one mesh (mipsfusion_amd/scene_mesh.py), the same way
        from . import scene_mesh
        return getattr(scene_mesh, name)
    if name in _POSE_CORRECTOR:             # rectifying a switch pose by ICP (mipsfusion_amd/pose_corrector.py), the same way
        from . import pose_corrector
        return getattr(pose_corrector, name)
    if name in _POSE_GRAPH:                 # closing a loop: the sub-map pose graph (mipsfusion_amd/pose_graph.py), the same way
        from . import pose_graph
        return getattr(pose_graph, name)
    if name in _SUBMAP_MANAGER:             # sub-map decisions (mipsfusion_amd/submap_manager.py), the same way
        from . import submap_manager
        return getattr(submap_manager, name)
    if name in _EVALUATE:                   # scoring a mesh against ground truth (mipsfusion_amd/evaluate.py), the same way
        from . import evaluate
        return getattr(evaluate, name)
    if name in _MESH_RENDER:                # a mesh as depth, colour and normal images, depth L1, occlusion (mipsfusion_amd/mesh_render.py)
        from . import mesh_render
        return getattr(mesh_render, name)
    if name in _TSDF:                       # depth frames fused into a TSDF volume and meshed (mipsfusion_amd/tsdf.py), the same way
        from . import tsdf
        return getattr(tsdf, name)
    if name in _SPARSE_TSDF:                # the same volume kept only near surfaces, past 2^31 voxels (mipsfusion_amd/sparse_tsdf.py)
        from . import sparse_tsdf
        return getattr(sparse_tsdf, name)
    if name in _IMAGE_METRICS:              # rendered frames against captured ones: PSNR, SSIM, MS-SSIM (mipsfusion_amd/image_metrics.py)
        from . import image_metrics
        return getattr(image_metrics, name)
    if name in _TRAJECTORY:                 # aligned absolute trajectory error, host only (mipsfusion_amd/trajectory.py)
        from . import trajectory
        return getattr(trajectory, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
