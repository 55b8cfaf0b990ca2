"""ctypes binding of libmipsf_hip.so (C ABI: include/mipsf.h).

The product path has no fallback: a missing library raises at first use, and every
operator raises when its tensors are not on a GPU.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MIPSF_LIB (developer switch): an experiment build of the same C ABI (tools/micro/variant.sh) instead of the in-tree library
LIB_PATH = os.environ.get("MIPSF_LIB") or os.path.join(_HERE, "libmipsf_hip.so")
MAX_LEVELS = 32
FEAT_AOS, FEAT_LEVEL_MAJOR = 0, 1
PREC = {"f32": 0, "f16x3": 1, "f16": 2, "bf16x3": 3, "bf16x6": 4}      # MIPSF_PREC_* of include/mipsf.h


class GridMeta(C.Structure):
    _fields_ = [("n_levels", C.c_uint32), ("n_features", C.c_uint32), ("log2_hashmap_size", C.c_uint32),
                ("base_resolution", C.c_uint32), ("per_level_scale", C.c_float),
                ("log2_per_level_scale", C.c_float), ("n_params", C.c_uint32),
                ("offsets", C.c_uint32 * (MAX_LEVELS + 1)), ("resolutions", C.c_uint32 * MAX_LEVELS),
                ("scales", C.c_float * MAX_LEVELS)]


class DecoderWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w_pts0", "b_pts0", "w_pts2", "b_pts2", "w_rgb0", "b_rgb0",
                                          "w_sdf0", "b_sdf0", "w_sdf2", "b_sdf2")]


DecoderGrads = DecoderWeights   # same field order, non-const pointers


class RenderCfg(C.Structure):
    _fields_ = [("n_uniform", C.c_uint32), ("n_near", C.c_uint32), ("perturb", C.c_int), ("use_bound", C.c_int),
                ("bound_min", C.c_double * 3), ("bound_max", C.c_double * 3), ("half_len", C.c_double * 3),
                ("norm_factor", C.c_double), ("trunc", C.c_float), ("sc_factor", C.c_float),
                ("depth_trunc", C.c_float), ("rgb_missing_nonzero", C.c_int), ("emd_w", C.c_float)]


def _args(name, fields):
    """ctypes mirror of an argument block of include/mipsf.h (struct_size first; `new()` returns a zeroed, sized block)."""
    cls = type(name, (C.Structure,), {"_fields_": [("struct_size", C.c_uint32)] + fields})

    def new(**kw):
        a = cls()
        a.struct_size = C.sizeof(cls)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    cls.new = staticmethod(new)
    return cls


_VP, _CU, _CI = C.c_void_p, C.c_uint32, C.c_int
HashgridBwdArgs = _args("HashgridBwdArgs", [("M", _CU), ("x", _VP), ("params", _VP), ("dout", _VP), ("dparams", _VP), ("dx", _VP),
                                            ("scratch", _VP), ("counters", _VP), ("meta", C.POINTER(GridMeta)),
                                            ("feat_layout", _CI), ("flags", _CU)])
DecoderFwd16Args = _args("DecoderFwd16Args", [("M", _CU), ("packed16", _VP), ("feat", _VP), ("x", _VP), ("out", _VP), ("saved", _VP),
                                              ("tile_live_clear", _VP), ("feat_layout", _CI), ("precision", _CI),
                                              ("sdf_only", _CI), ("lean_record", _CI), ("packed16_floats", _CU)])
DecoderChain16Args = _args("DecoderChain16Args", [("M", _CU), ("packed16", _VP), ("x", _VP), ("out", _VP), ("dout", _VP),
                                                  ("saved", _VP), ("dfeat", _VP), ("dx", _VP), ("dact", _VP), ("tile_live", _VP),
                                                  ("feat_layout", _CI), ("flags", _CI), ("packed16_floats", _CU),
                                                  ("live_list", _VP)])
DecoderWgrad16Args = _args("DecoderWgrad16Args", [("M", _CU), ("packed16", _VP), ("feat", _VP), ("x", _VP), ("saved", _VP),
                                                  ("dact", _VP), ("tile_live", _VP), ("grads", C.POINTER(DecoderGrads)),
                                                  ("partial", _VP), ("feat_layout", _CI), ("arithmetic", _CI), ("flags", _CU),
                                                  ("packed16_floats", _CU), ("live_list", _VP)])
RenderFwdArgs = _args("RenderFwdArgs", [("N", _CU), ("S", _CU), ("raw", _VP), ("z_vals", _VP), ("target_rgb", _VP), ("target_d", _VP),
                                        ("counts", _VP), ("cfg", C.POINTER(RenderCfg)), ("rgb", _VP), ("depth", _VP),
                                        ("depth_var", _VP), ("disp", _VP), ("acc", _VP), ("weights", _VP), ("losses", _VP),
                                        ("partial", _VP), ("loss_weights", _VP), ("loss_total", _VP), ("ticket", _VP),
                                        ("sums", _VP), ("draw", _VP)])
RenderBwdArgs = _args("RenderBwdArgs", [("N", _CU), ("S", _CU), ("N_norm", _CU), ("raw", _VP), ("z_vals", _VP), ("target_rgb", _VP),
                                        ("target_d", _VP), ("counts", _VP), ("losses", _VP), ("cfg", C.POINTER(RenderCfg)),
                                        ("g_losses", _VP), ("g_total", _VP), ("loss_weights", _VP), ("g_rgb", _VP),
                                        ("g_depth", _VP), ("draw", _VP), ("flags", _CU)])
RENDER_BWD_KEEP_IF_UNIT = 1

# mipsf_buffer_size(which, n, a, b, meta): MIPSF_SIZE_* of include/mipsf.h
(SIZE_HASHGRID_BWD_SCRATCH, SIZE_HASHGRID_COUNTER_WORDS, SIZE_DECODER_PACKED, SIZE_DECODER_SAVED, SIZE_DECODER_DACT,
 SIZE_DECODER_WGRAD_PARTIAL, SIZE_DECODER_PACKED16, SIZE_DECODER_TILE_WORDS, SIZE_RENDER_PARTIAL, SIZE_PLACE_POSE_SCRATCH,
 SIZE_POSE_RAYS_SCRATCH, SIZE_HASHGRID_DET_SCRATCH, SIZE_DECODER_LIVE_LIST) = range(1, 14)
# live-sample list of mipsf_decoder_live_compact (MIPSF_LIVE_*)
LIVE_HEADER, LIVE_PAD = 16, 0xFFFFFFFF

# mipsf_hashgrid_bwd flags (MIPSF_HG_*) and the deterministic scatter's constants
HG_DPARAMS_ZERO, HG_ROUTED, HG_DETERMINISTIC = 1, 2, 4
HG_DET_PIECE = 512
HG_DET_MAX_ITEMS = 1 << 31
TILE_ORDER_MAX_M = 1 << 27
# mipsf_decoder_wgrad16 flags (MIPSF_WGRAD_*)
WGRAD_LEAN_DACT, WGRAD_DETERMINISTIC = 1, 2


ADAM_MAX_TENSORS = 16


class AdamTensors(C.Structure):
    _fields_ = [("count", C.c_uint32), ("param", C.c_void_p * ADAM_MAX_TENSORS), ("grad", C.c_void_p * ADAM_MAX_TENSORS),
                ("exp_avg", C.c_void_p * ADAM_MAX_TENSORS), ("exp_avg_sq", C.c_void_p * ADAM_MAX_TENSORS),
                ("numel", C.c_uint64 * ADAM_MAX_TENSORS)]


ADAM_MAX_GROUPS = 8
ADAM_SMALL_MAX_NUMEL = 16384


class AdamSmall(C.Structure):
    _fields_ = [("n_groups", C.c_uint32), ("n_tensors", C.c_uint32),
                ("step_dev", C.c_void_p * ADAM_MAX_GROUPS), ("hyper_dev", C.c_void_p * ADAM_MAX_GROUPS),
                ("lr", C.c_float * ADAM_MAX_GROUPS), ("beta1", C.c_float * ADAM_MAX_GROUPS),
                ("beta2", C.c_float * ADAM_MAX_GROUPS), ("eps", C.c_float * ADAM_MAX_GROUPS),
                ("weight_decay", C.c_float * ADAM_MAX_GROUPS),
                ("param", C.c_void_p * ADAM_MAX_TENSORS), ("grad", C.c_void_p * ADAM_MAX_TENSORS),
                ("exp_avg", C.c_void_p * ADAM_MAX_TENSORS), ("exp_avg_sq", C.c_void_p * ADAM_MAX_TENSORS),
                ("numel", C.c_uint32 * ADAM_MAX_TENSORS), ("group_of", C.c_uint32 * ADAM_MAX_TENSORS)]


_P = C.c_void_p
_U32, _U64, _I, _F, _D = C.c_uint32, C.c_uint64, C.c_int, C.c_float, C.c_double

# name -> (restype, argtypes); every symbol include/mipsf.h declares
SIGNATURES = {
    "mipsf_last_error": (C.c_char_p, []),
    "mipsf_abi_version": (_I, []),
    "mipsf_device_cu_count": (_I, []),
    "mipsf_buffer_size": (_U64, [_I, _U32, _U32, _U32, C.POINTER(GridMeta)]),
    "mipsf_hashgrid_meta_init": (_I, [C.POINTER(GridMeta), _U32, _U32, _U32, _U32, _D]),
    "mipsf_hashgrid_fwd": (_I, [_P, _P, _P, _P, _U32, C.POINTER(GridMeta), _I, _P]),
    "mipsf_hashgrid_dx_from_jac": (_I, [_P, _P, _P, _P, _U32, C.POINTER(GridMeta), _I, _P]),
    "mipsf_hashgrid_bwd": (_I, [C.POINTER(HashgridBwdArgs), _P]),
    "mipsf_hashgrid_route": (_I, [_P, _P, _U32, C.POINTER(GridMeta), _P]),    "mipsf_hashgrid_indices": (_I, [_P, _P, _U32, C.POINTER(GridMeta), _P]),
    "mipsf_freq_fwd": (_I, [_P, _P, _U32, _U32, _U32, _P]),
    "mipsf_freq_bwd": (_I, [_P, _P, _P, _U32, _U32, _U32, _P]),
    "mipsf_decoder_pack": (_I, [C.POINTER(DecoderWeights), _P, _P]),
    "mipsf_decoder_pack_host": (_I, [C.POINTER(DecoderWeights), _P]),
    "mipsf_decoder_fwd": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _U32, _P]),
    "mipsf_decoder_fwd_sdf": (_I, [_P, _P, _I, _P, _P, _I, _P, _U32, _P]),
    "mipsf_decoder_bwd": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, C.POINTER(DecoderGrads), _P, _P,
                               _U32, _P]),
    "mipsf_decoder_bwd_chain": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _U32, _P]),
    "mipsf_decoder_wgrad": (_I, [_P, _I, _P, _P, _I, _P, _P, C.POINTER(DecoderGrads), _P, _I, _U32, _P]),
    "mipsf_decoder_pack16": (_I, [C.POINTER(DecoderWeights), _P, _I, _P]),
    "mipsf_decoder_fwd16": (_I, [C.POINTER(DecoderFwd16Args), _P]),
    "mipsf_decoder_bwd_chain16": (_I, [C.POINTER(DecoderChain16Args), _P]),
    "mipsf_decoder_wgrad16": (_I, [C.POINTER(DecoderWgrad16Args), _P]),
    "mipsf_sample_rays": (_I, [_P, _P, _P, _P, _P, _P, _P, C.POINTER(RenderCfg), _P, _P, _P, _U32, _P]),
    "mipsf_normalise_points": (_I, [_P, C.POINTER(RenderCfg), _P, _U32, _P]),
    "mipsf_render_fwd": (_I, [C.POINTER(RenderFwdArgs), _P]),
    "mipsf_loss_finalize_sums": (_I, [_P, C.POINTER(RenderCfg), _U32, _U32, _P, _P, _P, _P]),
    "mipsf_render_bwd": (_I, [C.POINTER(RenderBwdArgs), _P]),
    "mipsf_gather_pose_place_fwd": (_I, [_P, _U64, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, C.POINTER(RenderCfg), _P, _P,
                                         _P, _P, _P, _P, _U32, _P]),
    "mipsf_place_pose_bwd": (_I, [_P, _P, C.POINTER(RenderCfg), _P, _U32, _U32, _P, _P, _P, _P, _P, _U32, _U32, _I, _P]),
    "mipsf_rays_bwd": (_I, [_P, _P, C.POINTER(RenderCfg), _P, _P, _U32, _U32, _P]),
    "mipsf_normalise_bwd": (_I, [_P, C.POINTER(RenderCfg), _P, _U32, _P]),
    "mipsf_pose_rays_fwd": (_I, [_P, _U64, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, _P, _U32, _P]),
    "mipsf_pose_handover": (_I, [_P, _I, _P, _P, _P]),
    "mipsf_pose_rays_bwd": (_I, [_P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, _U32, _I, _P]),
    "mipsf_adam_step": (_I, [_P, _P, _P, _P, _U64, _F, _F, _F, _F, _F, _U32, _P, _I, _P]),
    "mipsf_adam_advance_n": (_I, [_P, _P, _P, _P, _P, _U32, _P]),
    "mipsf_adam_step_multi": (_I, [C.POINTER(AdamTensors), _F, _F, _F, _F, _F, _U32, _P, _I, _P]),
    "mipsf_adam_step_small": (_I, [C.POINTER(AdamSmall), _I, _P]),
    "mipsf_adam_step_all": (_I, [C.POINTER(AdamSmall), _I, _P, _P]),
    "mipsf_ro_fitness": (_I, [_P, _U32, _P, _F, _P, _U32, _U32, _P]),
    "mipsf_ro_fitness_sdf": (_I, [_P, _P, _F, _P, _U32, _U32, _I, _P]),
    "mipsf_ro_particles": (_I, [_P, _P, _P, _P, C.POINTER(RenderCfg), _P, _P, _U32, _U32, _I, _P]),
    "mipsf_ro_update": (_I, [_P, _P, _P, _F, _F, _U32, _P]),
    "mipsf_gather_rays": (_I, [_P, _U64, _P, _U32, _P, _P, _P, _P, _P]),
}


# include/mipsf_mesh.h (the mesh extractor; a header of its own, so a table of its own)
SIZE_MCUBES_OFFSET_WORDS, SIZE_MCUBES_WELD_SLOTS, SIZE_MCUBES_WELD_WORDS = 20, 21, 22
MCUBES_BLOCK_CELLS = 4096
McubesArgs = _args("McubesArgs", [("X", _CU), ("Y", _CU), ("Z", _CU), ("isovalue", C.c_float), ("truncation", C.c_float),
                                  ("volume", _VP), ("cases", _VP), ("block_offsets", _VP), ("soup", _VP), ("cell_ids", _VP),
                                  ("capacity_tris", _CU)])
McubesWeldArgs = _args("McubesWeldArgs", [("T", _CU), ("soup", _VP), ("scratch", _VP), ("vertices", _VP), ("faces", _VP),
                                          ("counts", _VP), ("max_rounds", _CU)])
# include/mipsf_compact.h
COMPACT_SIGNATURES = {
    "mipsf_decoder_live_compact": (_I, [_P, _U32, _P, _P, _P, _I, _P]),
    "mipsf_hashgrid_dx_from_jac_list": (_I, [_P, _P, _P, _P, _U32, C.POINTER(GridMeta), _I, _P]),
    "mipsf_gather_pose_place_fwd_masked": (_I, [_P, _U64, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, C.POINTER(RenderCfg),
                                                _P, _P, _P, _P, _P, _P, _P, _U32, _P]),
    "mipsf_hashgrid_fwd_masked": (_I, [_P, _P, _P, _P, _P, _U32, _U32, C.POINTER(GridMeta), _I, _P]),
    "mipsf_hashgrid_dx_from_jac_masked": (_I, [_P, _P, _P, _P, _P, _P, _U32, _U32, C.POINTER(GridMeta), _I, _P]),
}

MESH_SIGNATURES = {
    "mipsf_mcubes_count": (_I, [C.POINTER(McubesArgs), _P]),
    "mipsf_mcubes_emit": (_I, [C.POINTER(McubesArgs), _P]),
    "mipsf_mcubes_weld": (_I, [C.POINTER(McubesWeldArgs), _P]),
}


# include/mipsf_fuse.h (the scene as one mesh: visibility, SDF fusion, connected components)
FUSE_KF_FLOATS = 16
FUSE_IN_BOX, FUSE_SEEN = 1, 2


class FusePoints(C.Structure):
    _fields_ = [("points", _VP), ("ticks", _VP * 3), ("dims", _CU * 3), ("lo", _CU * 3), ("size", _CU * 3), ("first", _CU), ("n", _CU)]


class FuseCamera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("W", C.c_float), ("H", C.c_float),
                ("edge", C.c_float), ("k", _CU), ("keyframes", _VP)]


FuseVisibilityArgs = _args("FuseVisibilityArgs", [("pts", FusePoints), ("cam", FuseCamera), ("seen", _VP)])
FuseLocalArgs = _args("FuseLocalArgs", [("pts", FusePoints), ("w2l", C.c_float * 12), ("sub", C.c_double * 3), ("div", C.c_double * 3),
                                        ("out", _VP)])
FuseAccumulateArgs = _args("FuseAccumulateArgs", [("pts", FusePoints), ("cam", FuseCamera), ("rows", _VP), ("n_rows", _CU),
                                                  ("channels", _CU), ("sigmoid", _CU), ("values", _VP), ("entropy", _VP),
                                                  ("value_stride", _CU), ("entropy_stride", _CU), ("use_obb", _CU),
                                                  ("obb_centre", C.c_double * 3), ("obb_axes", C.c_double * 9),
                                                  ("obb_half", C.c_double * 3), ("centroid", C.c_float * 3), ("sigma", C.c_float),
                                                  ("gauss_k", C.c_float), ("num", _VP), ("den", _VP), ("flags", _VP)])
FuseFinalizeArgs = _args("FuseFinalizeArgs", [("n", _CU), ("channels", _CU), ("num", _VP), ("den", _VP), ("flags", _VP), ("out", _VP),
                                              ("volume", _VP)])
FuseLabelArgs = _args("FuseLabelArgs", [("F", _CU), ("E", _CU), ("pairs", _VP), ("labels", _VP), ("counts", _VP), ("max_rounds", _CU),
                                        ("resume", _CU)])
FUSE_SIGNATURES = {
    "mipsf_fuse_visibility": (_I, [C.POINTER(FuseVisibilityArgs), _P]),
    "mipsf_fuse_local_points": (_I, [C.POINTER(FuseLocalArgs), _P]),
    "mipsf_fuse_accumulate": (_I, [C.POINTER(FuseAccumulateArgs), _P]),
    "mipsf_fuse_finalize": (_I, [C.POINTER(FuseFinalizeArgs), _P]),
    "mipsf_fuse_label_components": (_I, [C.POINTER(FuseLabelArgs), _P]),
}


# include/mipsf_icp.h (rectifying a switch pose: clouds from ray rows, grid, nearest neighbours, normals, point-to-plane ICP)
ICP_KNN = 30
ICP_RESULT_DOUBLES = 20
ICP_MAX_POINTS, ICP_MAX_CELLS = 1 << 27, 1 << 26
ICP_WS_CLOUD, ICP_WS_GRID, ICP_WS_REGISTER = 1, 2, 3
IcpCloudArgs = _args("IcpCloudArgs", [("n", _CU), ("k", _CU), ("rows_per_owner", _CU), ("rows", _VP), ("owner", _VP), ("poses", _VP),
                                      ("points", _VP), ("count", _VP), ("workspace", _VP)])
IcpBinArgs = _args("IcpBinArgs", [("n", _CU), ("max_cells", _CU), ("points", _VP), ("min_edge", C.c_double), ("grid", _VP)])
IcpNearestArgs = _args("IcpNearestArgs", [("n_source", _CU), ("n_target", _CU), ("max_cells", _CU), ("source", _VP), ("grid", _VP),
                                          ("max_dist", C.c_double), ("partner", _VP), ("d2", _VP)])
IcpNormalsArgs = _args("IcpNormalsArgs", [("n", _CU), ("max_cells", _CU), ("points", _VP), ("grid", _VP), ("normals", _VP),
                                          ("neighbours", _VP)])
IcpRegisterArgs = _args("IcpRegisterArgs", [("n_source", _CU), ("n_target", _CU), ("max_cells", _CU), ("max_iteration", _CU),
                                            ("source", _VP), ("grid", _VP), ("target_normals", _VP), ("max_dist", C.c_double),
                                            ("relative_fitness", C.c_double), ("relative_rmse", C.c_double), ("result", _VP),
                                            ("partner", _VP), ("workspace", _VP)])
ICP_SIGNATURES = {
    "mipsf_icp_workspace_bytes": (_U64, [_I, _U32, _U32]),
    "mipsf_icp_cloud": (_I, [C.POINTER(IcpCloudArgs), _P]),
    "mipsf_icp_bin": (_I, [C.POINTER(IcpBinArgs), _P]),
    "mipsf_icp_nearest": (_I, [C.POINTER(IcpNearestArgs), _P]),
    "mipsf_icp_normals": (_I, [C.POINTER(IcpNormalsArgs), _P]),
    "mipsf_icp_register": (_I, [C.POINTER(IcpRegisterArgs), _P]),
}


# include/mipsf_posegraph.h (closing a loop: Levenberg-Marquardt over the sub-maps' anchors, one launch)
POSEGRAPH_MAX_NODES, POSEGRAPH_MAX_EDGES, POSEGRAPH_LDS_NODES, POSEGRAPH_RESULT_DOUBLES = 64, 1024, 20, 8
POSEGRAPH_FACTORISATION_FAILED, POSEGRAPH_NAN_QUALITY, POSEGRAPH_BAD_EDGE = 1, 2, 4
PosegraphArgs = _args("PosegraphArgs", [("n_nodes", _CU), ("n_edges", _CU), ("input_f64", _CU), ("anchors", _VP), ("edges", _VP),
                                        ("observations", _VP), ("weights", _VP), ("steps", _CU), ("patience", _CU),
                                        ("max_rejects", _CU), ("reserved", _CU), ("decreasing", C.c_double), ("radius", C.c_double),
                                        ("min_diag", C.c_double), ("anchors_out", _VP), ("anchors_out32", _VP), ("result", _VP),
                                        ("workspace", _VP)])
POSEGRAPH_SIGNATURES = {
    "mipsf_posegraph_workspace_bytes": (_U64, [_U32, _U32]),
    "mipsf_posegraph_optimize": (_I, [C.POINTER(PosegraphArgs), _P]),
}


# include/mipsf_submap.h (sub-map management: per-keyframe statistics and the overlap region)
SUBMAP_MAX_BOXES, SUBMAP_MAX_TOP_KF, SUBMAP_HEADER_WORDS, SUBMAP_BOX_WORDS, SUBMAP_WORKSPACE_BYTES = 64, 10, 16, 12, 8192
SUBMAP_RECORD_WORDS = SUBMAP_HEADER_WORDS + SUBMAP_MAX_BOXES * SUBMAP_BOX_WORDS
SubmapFrameStatsArgs = _args("SubmapFrameStatsArgs", [("H", _CU), ("W", _CU), ("n_boxes", _CU), ("lat_a_h", _CU), ("lat_a_w", _CU),
                                                      ("lat_b_h", _CU), ("lat_b_w", _CU), ("lat_c_h", _CU), ("lat_c_w", _CU),
                                                      ("near", C.c_float), ("far", C.c_float), ("min_cr_len", C.c_float * 3),
                                                      ("reserved", _CU), ("rows", _VP), ("pose", _VP), ("boxes", _VP),
                                                      ("max_len", _VP), ("record", _VP), ("workspace", _VP)])
SubmapOverlapArgs = _args("SubmapOverlapArgs", [("H", _CU), ("W", _CU), ("lat_h", _CU), ("lat_w", _CU), ("n_related", _CU), ("k", _CU),
                                                ("n_slots", _CU), ("rows_per_slot", _CU), ("reserved", _CU),
                                                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                                                ("cam_W", C.c_double), ("cam_H", C.c_double), ("edge", C.c_double),
                                                ("target_box", C.c_float * 6), ("rows", _VP), ("pose", _VP), ("table", _VP),
                                                ("related_slots", _VP), ("related_poses", _VP), ("dist", _VP), ("top_poses", _VP),
                                                ("top_kf_masks", _VP), ("mask_final", _VP), ("count", _VP), ("target_d", _VP),
                                                ("rays_d_cam", _VP)])
SUBMAP_SIGNATURES = {
    "mipsf_submap_frame_stats": (_I, [C.POINTER(SubmapFrameStatsArgs), _P]),
    "mipsf_submap_overlap": (_I, [C.POINTER(SubmapOverlapArgs), _P]),
}


# include/mipsf_eval.h (scoring a mesh against ground truth: surface samples, nearest neighbour without a radius, statistics)
EVAL_MAX_FACES, EVAL_MAX_SAMPLES = 1 << 30, 1 << 27
EVAL_WS_SAMPLE, EVAL_WS_STATS = 1, 2
EVAL_OK, EVAL_NO_AREA, EVAL_AREA_OVERFLOW = 0, 1, 2
EVAL_SAMPLE_RECORD_BYTES, EVAL_STATS_RECORD_BYTES = 32, 64


class EvalSampleRecord(C.Structure):
    _fields_ = [("area", C.c_double), ("total_units", C.c_uint64), ("status", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class EvalStatsRecord(C.Structure):
    _fields_ = [("sum_d", C.c_double), ("sum_d2", C.c_double), ("max_d2", C.c_double), ("within", C.c_uint64), ("finite", C.c_uint64),
                ("reserved", C.c_uint64 * 3)]


EvalSampleArgs = _args("EvalSampleArgs", [("V", _CU), ("F", _CU), ("n", _CU), ("seed", _CU), ("vertices", _VP), ("faces", _VP),
                                          ("points", _VP), ("face_of", _VP), ("record", _VP), ("workspace", _VP)])
EvalNearestArgs = _args("EvalNearestArgs", [("n_source", _CU), ("n_target", _CU), ("max_cells", _CU), ("source", _VP), ("grid", _VP),
                                            ("index", _VP), ("d2", _VP)])
EvalStatsArgs = _args("EvalStatsArgs", [("n", _CU), ("d2", _VP), ("threshold", C.c_double), ("record", _VP), ("workspace", _VP)])
EVAL_SIGNATURES = {
    "mipsf_eval_workspace_bytes": (_U64, [_I, _U32]),
    "mipsf_eval_sample": (_I, [C.POINTER(EvalSampleArgs), _P]),
    "mipsf_eval_nearest": (_I, [C.POINTER(EvalNearestArgs), _P]),
    "mipsf_eval_stats": (_I, [C.POINTER(EvalStatsArgs), _P]),
}


# include/mipsf_raster.h (a mesh as per-pixel depth from a batch of poses; depth L1; the occlusion test of the culling)
RASTER_TILE, RASTER_MAX_FACES, RASTER_MAX_SIDE, RASTER_MAX_PIXELS, RASTER_MAX_ITEMS = 8, 1 << 30, 8192, 1 << 30, 0x7FFFFFFF
RASTER_WS_DEPTH, RASTER_WS_L1 = 1, 2
RASTER_STAGE_COUNT, RASTER_STAGE_SCAN, RASTER_STAGE_RASTER, RASTER_STAGE_RESOLVE = 1, 2, 4, 8
RASTER_L1_RECORD_BYTES = 64


class RasterL1Record(C.Structure):
    _fields_ = [("sum_all", C.c_double), ("sum_both", C.c_double), ("both", C.c_uint64), ("rec_only", C.c_uint64),
                ("gt_only", C.c_uint64), ("neither", C.c_uint64), ("reserved", C.c_uint64 * 2)]


RasterDepthArgs = _args("RasterDepthArgs", [("V", _CU), ("F", _CU), ("n", _CU), ("H", _CU), ("W", _CU), ("stages", _CU), ("reserved", _CU),
                                            ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                                            ("near", C.c_double), ("far", C.c_double), ("vertices", _VP), ("faces", _VP),
                                            ("poses", _VP), ("depth", _VP), ("face", _VP), ("workspace", _VP)])
RasterL1Args = _args("RasterL1Args", [("n", _CU), ("H", _CU), ("W", _CU), ("a", _VP), ("b", _VP), ("records", _VP), ("workspace", _VP)])
RasterVisibleArgs = _args("RasterVisibleArgs", [("m", _CU), ("n", _CU), ("H", _CU), ("W", _CU), ("reserved", _CU),
                                                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                                                ("edge", C.c_double), ("eps", C.c_double), ("points", _VP), ("depth", _VP),
                                                ("poses", _VP), ("max_depth", _VP), ("seen", _VP)])
RASTER_SIGNATURES = {
    "mipsf_raster_workspace_bytes": (_U64, [_I, _U32, _U32, _U32, _U32]),
    "mipsf_raster_depth": (_I, [C.POINTER(RasterDepthArgs), _P]),
    "mipsf_raster_l1": (_I, [C.POINTER(RasterL1Args), _P]),
    "mipsf_raster_visible": (_I, [C.POINTER(RasterVisibleArgs), _P]),
}


# include/mipsf_tsdf.h (depth frames fused into a TSDF volume; the colour of marched vertices)
TSDF_MAX_VOXELS, TSDF_MAX_SIDE, TSDF_VIEW_CHUNK, TSDF_BRICK = 0x7FFFFFFF, 8192, 256, (8, 8, 16)
TSDF_NO_CULL = 1
TSDF_MAX_BRICKS = 0xFFFFFF
TSDF_RECORD_WORDS = 2                      # uint64 updates, observed
TsdfIntegrateArgs = _args("TsdfIntegrateArgs", [("X", _CU), ("Y", _CU), ("Z", _CU), ("n", _CU), ("H", _CU), ("W", _CU), ("flags", _CU),
                                                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                                                ("trunc", C.c_double), ("depth_max", C.c_double), ("max_weight", C.c_double),
                                                ("ticks", _VP * 3), ("depth", _VP), ("rgb", _VP), ("poses", _VP), ("tsdf", _VP),
                                                ("weight", _VP), ("color", _VP), ("record", _VP)])
TsdfSampleArgs = _args("TsdfSampleArgs", [("X", _CU), ("Y", _CU), ("Z", _CU), ("m", _CU), ("reserved", _CU), ("points", _VP),
                                          ("weight", _VP), ("color", _VP), ("out", _VP)])
TSDF_SIGNATURES = {
    "mipsf_tsdf_integrate": (_I, [C.POINTER(TsdfIntegrateArgs), _P]),
    "mipsf_tsdf_sample": (_I, [C.POINTER(TsdfSampleArgs), _P]),
}


# include/mipsf_deintegrate.h (views taken out of the TSDF volume again: the inverse of mipsf_tsdf_integrate's running mean)
DEINTEGRATE_RECORD_WORDS = 4               # uint64 removed, missing, emptied, observed
DeintegrateArgs = _args("DeintegrateArgs", [("X", _CU), ("Y", _CU), ("Z", _CU), ("n", _CU), ("H", _CU), ("W", _CU), ("flags", _CU),
                                            ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                                            ("trunc", C.c_double), ("depth_max", C.c_double),
                                            ("ticks", _VP * 3), ("depth", _VP), ("rgb", _VP), ("poses", _VP), ("tsdf", _VP),
                                            ("weight", _VP), ("color", _VP), ("record", _VP)])
DEINTEGRATE_SIGNATURES = {
    "mipsf_deintegrate_views": (_I, [C.POINTER(DeintegrateArgs), _P]),
}


# include/mipsf_track.h (the volume as depth, normal and colour images by ray casting; a depth frame registered against them)
TRACK_MAX_SAMPLES, TRACK_TILE, TRACK_RESULT_DOUBLES, TRACK_MAX_ITERATION, TRACK_MAX_VIEWS = 0x100000, 16, 20, 1000, 65535
TRACK_NO_SKIP = 1
TRACK_WS_RAYCAST, TRACK_WS_REGISTER = 1, 2
TRACK_RECORD_WORDS = 2                     # uint64 hits, marked
TrackRaycastArgs = _args("TrackRaycastArgs", [("X", _CU), ("Y", _CU), ("Z", _CU), ("n", _CU), ("H", _CU), ("W", _CU), ("flags", _CU),
                                              ("origin", C.c_double * 3), ("voxel", C.c_double), ("trunc", C.c_double),
                                              ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                                              ("near", C.c_double), ("far", C.c_double), ("step", C.c_double), ("min_weight", C.c_double),
                                              ("tsdf", _VP), ("weight", _VP), ("color", _VP), ("poses", _VP), ("depth", _VP),
                                              ("normals", _VP), ("color_out", _VP), ("record", _VP), ("workspace", _VP)])
TrackRegisterArgs = _args("TrackRegisterArgs", [("H", _CU), ("W", _CU), ("max_iteration", _CU),
                                                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                                                ("depth_max", C.c_double), ("max_dist", C.c_double), ("relative_fitness", C.c_double),
                                                ("relative_rmse", C.c_double), ("model_depth", _VP), ("model_normals", _VP),
                                                ("pose_ref", _VP), ("live", _VP), ("pose_init", _VP), ("result", _VP), ("pose_out", _VP),
                                                ("partner", _VP), ("workspace", _VP)])
TRACK_SIGNATURES = {
    "mipsf_track_workspace_bytes": (_U64, [_I, _U32, _U32, _U32]),
    "mipsf_track_raycast": (_I, [C.POINTER(TrackRaycastArgs), _P]),
    "mipsf_track_register": (_I, [C.POINTER(TrackRegisterArgs), _P]),
}
# include/mipsf_track_color.h (the same registration with a photometric row per pair against the ray cast's colour image)
TRACK_COLOR_RESULT_DOUBLES, TRACK_WS_REGISTER_COLOR = 22, 3
TrackRegisterColorArgs = _args("TrackRegisterColorArgs", [("H", _CU), ("W", _CU), ("max_iteration", _CU),
                                                          ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                                                          ("depth_max", C.c_double), ("max_dist", C.c_double), ("relative_fitness", C.c_double),
                                                          ("relative_rmse", C.c_double), ("color_weight", C.c_double),
                                                          ("max_color_diff", C.c_double), ("relative_color_rmse", C.c_double),
                                                          ("model_depth", _VP), ("model_normals", _VP), ("model_color", _VP), ("pose_ref", _VP),
                                                          ("live", _VP), ("live_color", _VP), ("pose_init", _VP), ("result", _VP),
                                                          ("pose_out", _VP), ("partner", _VP), ("color_partner", _VP), ("workspace", _VP)])
TRACK_COLOR_SIGNATURES = {
    "mipsf_track_register_color": (_I, [C.POINTER(TrackRegisterColorArgs), _P]),
}


# include/mipsf_sparse.h (the TSDF volume kept only where a depth pixel put a surface: an index grid of bricks and a pool of slots)
SPARSE_BRICK_VOXELS, SPARSE_MAX_BRICKS, SPARSE_MAX_CAPACITY, SPARSE_MAX_STEPS, SPARSE_MAX_VIEWS = 1024, 0x7FFFFFFF, 0x100000, 4096, 65535
SPARSE_SCAN_TILE = 1024
SPARSE_NO_SKIP = 1
SPARSE_ALLOC_RECORD_WORDS = 4              # uint64 marked, created, dropped, in_use


class SparseVolume(C.Structure):
    _fields_ = [("X", _CU), ("Y", _CU), ("Z", _CU), ("capacity", _CU), ("origin", C.c_double * 3), ("voxel", C.c_double), ("ticks", _VP * 3),
                ("table", _VP), ("slot_brick", _VP), ("birth", _VP), ("count", _VP), ("tsdf", _VP), ("weight", _VP), ("color", _VP)]


SparseAllocateArgs = _args("SparseAllocateArgs", [("n", _CU), ("H", _CU), ("W", _CU), ("steps", _CU), ("reserved", _CU),
                                                  ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                                                  ("depth_max", C.c_double), ("band", C.c_double), ("vol", SparseVolume), ("depth", _VP),
                                                  ("poses", _VP), ("mark", _VP), ("scan", _VP), ("record", _VP)])
SparseIntegrateArgs = _args("SparseIntegrateArgs", [("n", _CU), ("H", _CU), ("W", _CU), ("flags", _CU), ("reserved", _CU),
                                                    ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                                                    ("trunc", C.c_double), ("depth_max", C.c_double), ("max_weight", C.c_double),
                                                    ("vol", SparseVolume), ("depth", _VP), ("rgb", _VP), ("poses", _VP), ("record", _VP)])
SparseGatherArgs = _args("SparseGatherArgs", [("lo", _CU * 3), ("hi", _CU * 3), ("reserved", _CU), ("vol", SparseVolume), ("tsdf", _VP),
                                              ("weight", _VP), ("color", _VP)])
SparseRaycastArgs = _args("SparseRaycastArgs", [("n", _CU), ("H", _CU), ("W", _CU), ("flags", _CU), ("reserved", _CU), ("trunc", C.c_double),
                                                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                                                ("near", C.c_double), ("far", C.c_double), ("step", C.c_double), ("min_weight", C.c_double),
                                                ("vol", SparseVolume), ("poses", _VP), ("depth", _VP), ("normals", _VP), ("color_out", _VP),
                                                ("record", _VP)])
SPARSE_SIGNATURES = {
    "mipsf_sparse_scan_words": (_U64, [_U32, _U32, _U32]),
    "mipsf_sparse_allocate": (_I, [C.POINTER(SparseAllocateArgs), _P]),
    "mipsf_sparse_integrate": (_I, [C.POINTER(SparseIntegrateArgs), _P]),
    "mipsf_sparse_gather": (_I, [C.POINTER(SparseGatherArgs), _P]),
    "mipsf_sparse_raycast": (_I, [C.POINTER(SparseRaycastArgs), _P]),
}


# include/mipsf_sparse_remove.h (views taken out of the sparse volume again; the per-brick history that tells which views a brick holds)
SPARSE_UNBORN, SPARSE_MAX_VIEW_ID = 0xFFFFFFFF, 0xFFFFFFFE
SPARSE_REMOVE_RECORD_WORDS = 5             # uint64 removed, missing, emptied, observed, bricks_emptied
SparseStampArgs = _args("SparseStampArgs", [("n", _CU), ("vol", SparseVolume), ("born", _VP), ("serial", _VP)])
SparseDeintegrateArgs = _args("SparseDeintegrateArgs", [("n", _CU), ("H", _CU), ("W", _CU), ("flags", _CU), ("reserved", _CU),
                                                        ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                                                        ("trunc", C.c_double), ("depth_max", C.c_double),
                                                        ("vol", SparseVolume), ("depth", _VP), ("rgb", _VP), ("poses", _VP), ("view_ids", _VP),
                                                        ("born", _VP), ("record", _VP)])
SPARSE_REMOVE_SIGNATURES = {
    "mipsf_sparse_stamp": (_I, [C.POINTER(SparseStampArgs), _P]),
    "mipsf_sparse_deintegrate": (_I, [C.POINTER(SparseDeintegrateArgs), _P]),
}


# include/mipsf_sparse_release.h (slots of the sparse volume given back, archived and restored)
SPARSE_RELEASE_OUTSIDE, SPARSE_RELEASE_EMPTY, SPARSE_RELEASE_ARCHIVE = 1, 2, 4
SPARSE_RESTORE_SCRATCH_WORDS = 16
SPARSE_RELEASE_RECORD_WORDS = 7            # uint64 candidates, released, released_outside, released_empty, deferred, moved, in_use
SPARSE_RESTORE_RECORD_WORDS = 7            # uint64 listed, invalid, duplicates, occupied, restored, dropped, in_use
SparseReleaseArgs = _args("SparseReleaseArgs", [("flags", _CU), ("archive_capacity", _CU), ("reserved", _CU), ("vol", SparseVolume), ("born", _VP),
                                                ("box", _VP), ("arch_brick", _VP), ("arch_born", _VP), ("arch_tsdf", _VP), ("arch_weight", _VP),
                                                ("arch_color", _VP), ("scratch", _VP), ("record", _VP)])
SparseRestoreArgs = _args("SparseRestoreArgs", [("m", _CU), ("vol", SparseVolume), ("born", _VP), ("arch_brick", _VP), ("arch_born", _VP),
                                                ("arch_tsdf", _VP), ("arch_weight", _VP), ("arch_color", _VP), ("mark", _VP), ("scan", _VP),
                                                ("scratch", _VP), ("record", _VP)])
SPARSE_RELEASE_SIGNATURES = {
    "mipsf_sparse_release_scratch_words": (_U64, [_U32]),
    "mipsf_sparse_release": (_I, [C.POINTER(SparseReleaseArgs), _P]),
    "mipsf_sparse_restore": (_I, [C.POINTER(SparseRestoreArgs), _P]),
}


# include/mipsf_sparse_mesh.h (the mesh of the sparse volume marched brick by brick; the colour of its vertices)
SPARSE_MESH_MAX_SIDE, SPARSE_MESH_SCAN_TILE = 21474, 1024
SPARSE_MESH_MAX_TRIS = 0x0FFFFFFF          # what the weld table of mipsf_mcubes_weld holds
SparseMeshArgs = _args("SparseMeshArgs", [("min_weight", C.c_float), ("vol", SparseVolume), ("cases", _VP), ("offsets", _VP), ("scan", _VP),
                                          ("soup", _VP), ("tri_slot", _VP), ("cell_ids", _VP), ("capacity_tris", _CU), ("reserved", _CU)])
SparseMeshWeldArgs = _args("SparseMeshWeldArgs", [("T", _CU), ("capacity_tris", _CU), ("max_rounds", _CU), ("vol", SparseVolume), ("soup", _VP),
                                                  ("tri_slot", _VP), ("scratch", _VP), ("vertices", _VP), ("faces", _VP), ("counts", _VP)])
SparseSampleArgs = _args("SparseSampleArgs", [("m", _CU), ("vol", SparseVolume), ("points", _VP), ("out", _VP)])
SPARSE_MESH_SIGNATURES = {
    "mipsf_sparse_mesh_scan_words": (_U64, [_U32]),
    "mipsf_sparse_mesh_count": (_I, [C.POINTER(SparseMeshArgs), _P]),
    "mipsf_sparse_mesh_emit": (_I, [C.POINTER(SparseMeshArgs), _P]),
    "mipsf_sparse_mesh_weld": (_I, [C.POINTER(SparseMeshWeldArgs), _P]),
    "mipsf_sparse_sample": (_I, [C.POINTER(SparseSampleArgs), _P]),
}


# include/mipsf_image.h (two image stacks compared: error sums, valid-region SSIM and its cs term, the MS-SSIM pyramid's 2 x 2 mean)
IMAGE_F32, IMAGE_F64 = 0, 1
IMAGE_WINDOW, IMAGE_TILE_H, IMAGE_TILE_W, IMAGE_MAX_CHANNELS, IMAGE_MAX_SIDE = 11, 16, 32, 4, 8192
IMAGE_MAX_PLANES, IMAGE_MAX_VALUES, IMAGE_ERROR_MAX_BLOCKS = 65535, 0x7FFFFFFF, 256
IMAGE_WS_ERROR, IMAGE_WS_SSIM = 1, 2
IMAGE_ERROR_RECORD_BYTES, IMAGE_SSIM_RECORD_BYTES = 32, 32


class ImageErrorRecord(C.Structure):
    _fields_ = [("sum_sq", C.c_double), ("sum_abs", C.c_double), ("max_abs", C.c_double), ("count", C.c_uint64)]


class ImageSsimRecord(C.Structure):
    _fields_ = [("sum_ssim", C.c_double), ("sum_cs", C.c_double), ("count", C.c_uint64), ("reserved", C.c_uint64)]


ImageErrorArgs = _args("ImageErrorArgs", [("n", _CU), ("H", _CU), ("W", _CU), ("C", _CU), ("dtype", _CU), ("a", _VP), ("b", _VP),
                                          ("records", _VP), ("workspace", _VP)])
ImageSsimArgs = _args("ImageSsimArgs", [("n", _CU), ("H", _CU), ("W", _CU), ("C", _CU), ("dtype", _CU), ("window", C.c_double * 11),
                                        ("C1", C.c_double), ("C2", C.c_double), ("a", _VP), ("b", _VP), ("records", _VP),
                                        ("workspace", _VP)])
ImagePool2Args = _args("ImagePool2Args", [("n", _CU), ("H", _CU), ("W", _CU), ("C", _CU), ("dtype", _CU), ("in_", _VP), ("out", _VP)])
IMAGE_SIGNATURES = {
    "mipsf_image_workspace_bytes": (_U64, [_I, _U32, _U32, _U32, _U32]),
    "mipsf_image_error": (_I, [C.POINTER(ImageErrorArgs), _P]),
    "mipsf_image_ssim": (_I, [C.POINTER(ImageSsimArgs), _P]),
    "mipsf_image_pool2": (_I, [C.POINTER(ImagePool2Args), _P]),
}


# include/mipsf_shade.h (per-vertex normals; the face image of mipsf_raster_depth as colour, normal and head-lit images)
SHADE_TILE, SHADE_MAX_FACES, SHADE_MAX_VERTICES, SHADE_MAX_SIDE, SHADE_MAX_PIXELS, SHADE_MAX_ITEMS = 8, 1 << 30, 0x7FFFFFFF, 8192, 1 << 30, 0x7FFFFFFF
SHADE_SHORT_SEGMENT = 32
SHADE_WS_VERTEX_NORMALS = 1
SHADE_FLAT, SHADE_SMOOTH = 1, 2
SHADE_RECORD_WORDS = 2                     # uint64 hits, shaded
ShadeVertexNormalsArgs = _args("ShadeVertexNormalsArgs", [("V", _CU), ("F", _CU), ("reserved", _CU), ("vertices", _VP), ("faces", _VP),
                                                          ("normals", _VP), ("workspace", _VP)])
ShadePixelsArgs = _args("ShadePixelsArgs", [("V", _CU), ("F", _CU), ("n", _CU), ("H", _CU), ("W", _CU), ("flags", _CU), ("reserved", _CU),
                                            ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                                            ("background", C.c_float * 3), ("reserved2", C.c_float), ("vertices", _VP), ("faces", _VP),
                                            ("poses", _VP), ("face", _VP), ("colors", _VP), ("vertex_normals", _VP), ("color", _VP),
                                            ("normals", _VP), ("shaded", _VP), ("record", _VP)])
SHADE_SIGNATURES = {
    "mipsf_shade_workspace_bytes": (_U64, [_I, _U32, _U32]),
    "mipsf_shade_vertex_normals": (_I, [C.POINTER(ShadeVertexNormalsArgs), _P]),
    "mipsf_shade_pixels": (_I, [C.POINTER(ShadePixelsArgs), _P]),
}


def buffer_size(which: int, n: int = 0, a: int = 0, b: int = 0, meta=None) -> int:
    """mipsf_buffer_size: elements of a scratch / record buffer (SIZE_* above)."""
    v = lib().mipsf_buffer_size(which, n, a, b, C.byref(meta) if meta is not None else None)
    if v == 0xFFFFFFFFFFFFFFFF:
        raise RuntimeError((lib().mipsf_last_error() or b"mipsf_buffer_size: bad query").decode())
    return int(v)


def hashgrid_counter_layout(meta) -> dict:
    """Word offsets of the routed scatter's counter block (csrc/hashgrid.hip make_plan; tests and probes): {bin counts | queue
    head + tickets (4) | arrivals | first item | parts}, one word per bin each.  Every word in front of `first` reads zero
    between calls."""
    end = buffer_size(SIZE_HASHGRID_COUNTER_WORDS, meta=meta)
    bins = (end - 4) // 4
    return {"count": 0, "nitems": bins, "arrive": bins + 4, "first": 2 * bins + 4, "parts": 3 * bins + 4, "end": end,
            "n_bins": bins}


def _all_signatures():
    return (list(SIGNATURES.items()) + list(MESH_SIGNATURES.items())
            + list(FUSE_SIGNATURES.items()) + list(ICP_SIGNATURES.items())
            + list(COMPACT_SIGNATURES.items()) + list(POSEGRAPH_SIGNATURES.items())
            + list(SUBMAP_SIGNATURES.items()) + list(EVAL_SIGNATURES.items())
            + list(RASTER_SIGNATURES.items()) + list(TSDF_SIGNATURES.items())
            + list(IMAGE_SIGNATURES.items()) + list(TRACK_SIGNATURES.items()) + list(TRACK_COLOR_SIGNATURES.items())
            + list(SHADE_SIGNATURES.items()) + list(SPARSE_SIGNATURES.items())
            + list(SPARSE_MESH_SIGNATURES.items()) + list(DEINTEGRATE_SIGNATURES.items())
            + list(SPARSE_REMOVE_SIGNATURES.items()) + list(SPARSE_RELEASE_SIGNATURES.items()))


def load(path: str) -> C.CDLL:
    """A build of the C ABI as a fresh handle with every signature applied and the ABI version checked; it is returned, not
    kept: lib() keeps the product's, use_library() lends a variant's (csrc/variants.mk) to a block of calls."""
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C mipsfusion_amd/csrc all variants`). There is no CPU fallback.")
    handle = C.CDLL(path)
    for name, (res, args) in _all_signatures():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    if handle.mipsf_abi_version() != 2:
        raise RuntimeError(f"{os.path.basename(path)} ABI version mismatch")
    return handle


_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load (once) and return the shared library; raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH)
    return _lib


def variant_path(name: str) -> str:
    """The variant library `name` of csrc/variants.mk, where `make variants` leaves it."""
    return os.path.join(_HERE, "variants", f"libmipsf_{name}.so")


@contextlib.contextmanager
def use_library(path: str):
    """Every call inside the block goes to the build at `path` (a variant library, or any build of the same C ABI): lib()
    returns its handle, so ops.* and every size query (mipsf_buffer_size: the variant's own plan) run unchanged.  The kept
    counter / ticket blocks are dropped on entry and on exit -- a block sized and left behind by one build's plan must not be
    handed to another build's kernels.  The device is synchronised first: a dropped block may still be in use by a launch in
    flight.  Not for concurrent use: the handle is a module global."""
    global _lib
    handle = load(path)

    def drop_kept_blocks():
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.synchronize()
        for cache in KEPT_BLOCK_CACHES:
            cache.clear()

    previous = _lib
    drop_kept_blocks()
    _lib = handle
    try:
        yield handle
    finally:
        drop_kept_blocks()
        _lib = previous


# Caches of caller-kept counter / ticket blocks (ops._scatter_counters, ops._zeroed_words, ops._pose_scratch, FusedAdam's
# ticket): a kernel finds them at zero and leaves them at zero -- IF it runs to completion.  A call that failed after launching
# part of its work may have left counts or tickets behind; every cache registered here is emptied when a call fails, so the
# next call starts from freshly zeroed blocks instead of silently miscounting.
KEPT_BLOCK_CACHES = []


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().mipsf_last_error().decode(errors="replace")
        for cache in KEPT_BLOCK_CACHES:
            cache.clear()
        raise RuntimeError(f"libmipsf_hip {what} failed (code {rc}): {msg}")


def stream_ptr() -> int:
    """hipStream_t of torch's current stream on the current device (raw query: 0.2 us instead of 2.6 us for
    torch.cuda.current_stream().cuda_stream -- it is called once per launch)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def dptr(t: Optional[torch.Tensor], dtype=torch.float32) -> Optional[int]:
    """Device pointer of a contiguous GPU tensor (None passes through as NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("mipsfusion_amd operators need GPU tensors (no CPU fallback exists)")
    if t.device.index != torch._C._cuda_getDevice():
        # launches go to the CURRENT device's current stream (stream_ptr): a tensor of another GPU would be a foreign
        # pointer there.  One process per GPU with torch.cuda.set_device(local_rank) is the supported arrangement.
        raise RuntimeError(f"tensor lives on cuda:{t.device.index} but the current device is "
                           f"cuda:{torch._C._cuda_getDevice()}; wrap the call in torch.cuda.device(tensor.device)")
    if t.dtype != dtype:
        raise RuntimeError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError("tensor must be contiguous")
    return t.data_ptr()


def make_grid_meta(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16,
                   per_level_scale=2.0) -> GridMeta:
    m = GridMeta()
    check(lib().mipsf_hashgrid_meta_init(C.byref(m), n_levels, n_features, log2_hashmap_size, base_resolution,
                                         float(per_level_scale)), "hashgrid_meta_init")
    return m
