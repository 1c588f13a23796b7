"""ctypes binding of libagile3d_hip.so (the C ABI declared in include/agile3d_hip.h).

The product path has no fallback: if the shared object is missing or a symbol cannot be
resolved, importing this module's ``load()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("A3D_LIB_PATH") or os.path.join(HERE, "libagile3d_hip.so")   # override: A/B of two builds

A3D_NUM_LEVELS = 5
A3D_MAX_QUERIES = 256
A3D_MAX_DEC_LAYERS = 8
POSENC_KINDS = {"fourier": 0, "sine": 1, "legacy": 2}   # A3D_POSENC_*: args.positional_encoding_type -> a3d_posenc kind
OP_STEM, OP_CONV3, OP_DOWN, OP_UP, OP_LINEAR = 0, 1, 2, 3, 4
BUF_NONE, BUF_EXT_OUT = -1, -2
(TAB_XYZB, TAB_NBR27, TAB_GMASK27, TAB_CHILD8, TAB_GMASKDOWN, TAB_UP8, TAB_GMASKUP, TAB_UPROWS,
 TAB_ORIGROW, TAB_ORDER27, TAB_PRE27, TAB_PREDOWN, TAB_PREUP) = range(13)

c_float_p = C.c_void_p  # device pointers travel as integers


class BufDesc(C.Structure):
    _fields_ = [("level", C.c_int32), ("channels", C.c_int32)]


class Op(C.Structure):
    _fields_ = [("kind", C.c_int32), ("level_in", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32),
                ("in_buf", C.c_int32), ("in_coff", C.c_int32), ("out_buf", C.c_int32), ("out_coff", C.c_int32),
                ("res_buf", C.c_int32), ("res_coff", C.c_int32), ("relu", C.c_int32),
                ("kernel_volume", C.c_int32),
                ("w_dev", C.c_void_p), ("scale_dev", C.c_void_p), ("shift_dev", C.c_void_p),
                ("proj_buf", C.c_int32), ("proj_coff", C.c_int32), ("proj_cin", C.c_int32), ("reserved_", C.c_int32),
                ("head_w_dev", C.c_void_p), ("head_bias_dev", C.c_void_p), ("head_cout", C.c_int32), ("reserved2_", C.c_int32)]


_LAYER_FIELDS = ["c2s_in_w", "c2s_in_b", "c2s_out_w", "c2s_out_b", "c2s_norm_w", "c2s_norm_b",
                 "c2c_in_w", "c2c_in_b", "c2c_out_w", "c2c_out_b", "c2c_norm_w", "c2c_norm_b",
                 "ffn_w1", "ffn_b1", "ffn_w2", "ffn_b2", "ffn_norm_w", "ffn_norm_b",
                 "s2c_in_w", "s2c_in_b", "s2c_out_w", "s2c_out_b", "s2c_norm_w", "s2c_norm_b",
                 "c2s_wk_packed", "c2s_wv_packed", "s2c_wq_packed", "s2c_wo_packed", "query_pack"]


class DecoderLayer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _LAYER_FIELDS]


class DecoderWeights(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("n_bg_queries", C.c_int32), ("dim_ff", C.c_int32),
                ("layers", DecoderLayer * A3D_MAX_DEC_LAYERS),
                ("decoder_norm_w", C.c_void_p), ("decoder_norm_b", C.c_void_p),
                ("mask_w0", C.c_void_p), ("mask_b0", C.c_void_p), ("mask_w2", C.c_void_p), ("mask_b2", C.c_void_p),
                ("bg_query_feat", C.c_void_p), ("bg_query_pos", C.c_void_p),
                ("gauss_B", C.c_void_p), ("time_table", C.c_void_p), ("mask_pack", C.c_void_p)]


class PackJob(C.Structure):
    """a3d_pack_job: one weight of a3d_pack_conv_weights_multi."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("K", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32),
                ("src_cin", C.c_int32), ("src_cout", C.c_int32), ("transposed", C.c_int32), ("flip", C.c_int32),
                ("c0", C.c_int32), ("chunk0", C.c_int32), ("pad_", C.c_int32)]


# the same record as numpy sees it: the rows of the table a3d_pack_conv_weights_multi reads
PACK_JOB = np.dtype([("src", "<u8"), ("dst", "<u8"), ("K", "<i4"), ("cin", "<i4"), ("cout", "<i4"), ("src_cin", "<i4"),
                     ("src_cout", "<i4"), ("transposed", "<i4"), ("flip", "<i4"), ("c0", "<i4"), ("chunk0", "<i4"), ("pad", "<i4")])
assert C.sizeof(PackJob) == PACK_JOB.itemsize == 56


def pack_job_table(rows, device):
    """The device table (uint8) of a3d_pack_conv_weights_multi from job rows, one tuple in ``PACK_JOB``'s field order each."""
    return torch.from_numpy(np.array(rows, dtype=PACK_JOB).view(np.uint8)).to(device)


class ProfEntry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("id", "bn", "kernel_volume", "cin", "cout", "n_out", "table", "level",
                                         "ksplit")] + [("ms", C.c_float)]


class DecoderSample(C.Structure):
    """a3d_decoder_sample: one batch sample of a3d_decoder_forward_batch."""
    _fields_ = [("feats128_dev", C.c_void_p), ("posenc_dev", C.c_void_p), ("n", C.c_int64),
                ("click_row", C.POINTER(C.c_int32)), ("click_obj", C.POINTER(C.c_int32)),
                ("click_time", C.POINTER(C.c_int32)), ("n_clicks", C.c_int32), ("n_objects", C.c_int32),
                ("logits_dev", C.c_void_p), ("workspace_dev", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("kv0_dev", C.c_void_p), ("kv0_state", C.c_int32), ("kv0_blocks", C.c_int32)]


class Dropout(C.Structure):
    """a3d_dropout: the dropout of one site of one batch sample (passed by value)."""
    _fields_ = [("seed", C.c_uint64), ("p", C.c_float), ("sample", C.c_int32), ("site_code", C.c_int32),
                ("reserved_", C.c_int32)]


class ClickSample(C.Structure):
    """a3d_click_sample: one sample of a3d_click_clusters_batch."""
    _fields_ = [("xyz_dev", C.c_void_p), ("pred_dev", C.c_void_p), ("labels_dev", C.c_void_p), ("n", C.c_int64),
                ("out_dev", C.c_void_p), ("n_out_dev", C.c_void_p), ("max_out", C.c_int32), ("workspace_dev", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("order_dev", C.c_void_p), ("inv_dev", C.c_void_p)]


class ArgmaxSample(C.Structure):
    """a3d_argmax_sample: one sample of a3d_argmax_labels_batch."""
    _fields_ = [("logits_dev", C.c_void_p), ("n", C.c_int64), ("n_classes", C.c_int32), ("n_clicks", C.c_int32),
                ("click_row", C.POINTER(C.c_int32)), ("click_obj", C.POINTER(C.c_int32)), ("pred_dev", C.c_void_p)]


class IouSample(C.Structure):
    """a3d_iou_sample: one sample of a3d_iou_counts_batch."""
    _fields_ = [("pred_dev", C.c_void_p), ("n_pred", C.c_int64), ("inverse_map_dev", C.c_void_p), ("labels_dev", C.c_void_p),
                ("n_full", C.c_int64)]


class NearestSource(C.Structure):
    """a3d_nearest_source: one row set of a3d_nearest_rows."""
    _fields_ = [("xyz_dev", C.c_void_p), ("n", C.c_int64), ("rows_out_dev", C.c_void_p)]


class PickResult(C.Structure):
    """a3d_pick_result: what a3d_pick_ray writes (index -1 = the ray meets no point)."""
    _fields_ = [("index", C.c_int32), ("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class PickMeshResult(C.Structure):
    """a3d_pick_mesh_result: what a3d_pick_mesh writes (face -1 = the ray meets no surface; flags bit 0 = a face index
    outside the vertex rows was skipped; u, v = the weights of the face's second and third vertex)."""
    _fields_ = [("face", C.c_int32), ("flags", C.c_int32), ("t", C.c_float), ("x", C.c_float), ("y", C.c_float),
                ("z", C.c_float), ("u", C.c_float), ("v", C.c_float)]


class SessionPaintArgs(C.Structure):
    """a3d_session_paint_args."""
    _fields_ = [("labels_qv_dev", C.c_void_p), ("n_qv", C.c_int64), ("inverse_map_dev", C.c_void_p), ("n_full", C.c_int64),
                ("xyz_full_dev", C.c_void_p), ("colors_full_dev", C.c_void_p), ("palette_dev", C.c_void_p),
                ("cubes_dev", C.c_void_p), ("n_palette", C.c_int32), ("n_cubes", C.c_int32), ("cube_size", C.c_float),
                ("reserved_", C.c_int32), ("label_full_dev", C.c_void_p), ("colors_out_dev", C.c_void_p),
                ("err_dev", C.c_void_p)]


class SessionEditArgs(C.Structure):
    """a3d_session_edit_args: the relabel half (labels_ori, instances, new_labels), the remap half (labels, lut, err)."""
    _fields_ = [("labels_ori_dev", C.c_void_p), ("instances_dev", C.c_void_p), ("new_labels_dev", C.c_void_p),
                ("n_full", C.c_int64), ("labels_dev", C.c_void_p), ("n_labels", C.c_int64), ("err_dev", C.c_void_p),
                ("n_objects", C.c_int32), ("reserved_", C.c_int32), ("lut", C.c_uint8 * 256)]


class SessionGuideSummary(C.Structure):
    """a3d_session_guide_summary: rows and contested rows per label, the complemented packed key of the least confident row (0 =
    none), the error word (bit 0 = a NaN margin, bit 1 = an inverse_map entry out of range)."""
    _fields_ = [("voxels", C.c_int32 * 256), ("contested", C.c_int32 * 256), ("least_key", C.c_uint64), ("err", C.c_int32),
                ("reserved_", C.c_int32)]


class SessionGuideArgs(C.Structure):
    """a3d_session_guide_args: the voxel half (logits -> labels, runner, margin, want), the vertex half (inverse_map, colours,
    palette -> margin_full, colors_out), the summary, the settings and the clicks by value."""
    _fields_ = [("logits_dev", C.c_void_p), ("n_qv", C.c_int64), ("inverse_map_dev", C.c_void_p), ("n_full", C.c_int64),
                ("colors_full_dev", C.c_void_p), ("palette_dev", C.c_void_p), ("labels_qv_dev", C.c_void_p),
                ("runner_qv_dev", C.c_void_p), ("margin_qv_dev", C.c_void_p), ("want_qv_dev", C.c_void_p),
                ("margin_full_dev", C.c_void_p), ("colors_out_dev", C.c_void_p), ("summary_dev", C.c_void_p),
                ("n_classes", C.c_int32), ("n_palette", C.c_int32), ("n_clicks", C.c_int32), ("threshold", C.c_float),
                ("full_margin", C.c_float), ("doubt", C.c_float * 3), ("click_row", C.c_int32 * 256),
                ("click_obj", C.c_uint8 * 256)]


class Piece(C.Structure):
    """a3d_piece: one connected piece -- its root (the smallest caller row), key, voxels, 1 if it holds a clicked row, and the
    inclusive bounding box in voxel coordinates."""
    _fields_ = [("root", C.c_int32), ("key", C.c_int32), ("voxels", C.c_int32), ("clicked", C.c_int32),
                ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]


class LabelPiecesArgs(C.Structure):
    """a3d_label_pieces_args: the scene and the keys, the optional lift to full resolution, the outputs (piece_qv, piece_full,
    the records, int32 [2] count and error word), the workspace, the settings and the clicked rows by value."""
    _fields_ = [("scene", C.c_void_p), ("n", C.c_int64), ("keys_dev", C.c_void_p), ("inverse_map_dev", C.c_void_p),
                ("n_full", C.c_int64), ("piece_qv_dev", C.c_void_p), ("piece_full_dev", C.c_void_p), ("out_dev", C.c_void_p),
                ("n_out_dev", C.c_void_p), ("workspace_dev", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("connectivity", C.c_int32), ("max_out", C.c_int32), ("n_clicks", C.c_int32), ("reserved_", C.c_int32),
                ("click_row", C.c_int32 * 256)]


class AbsorbSummary(C.Structure):
    """a3d_absorb_summary: small pieces (the capacity needed on overflow), relabelled pieces and voxels, kept-isolated pieces,
    the error word (A3D_ABSORB_OVERFLOW, A3D_ABSORB_BAD_LABEL)."""
    _fields_ = [("small_pieces", C.c_int32), ("relabelled_pieces", C.c_int32), ("relabelled_voxels", C.c_int32),
                ("kept_isolated", C.c_int32), ("err", C.c_int32), ("reserved_", C.c_int32 * 3)]


class AbsorbPiecesArgs(C.Structure):
    """a3d_absorb_pieces_args: the scene, the labels and their pieces, the output labels and summary, the workspace
    a3d_label_pieces used, the settings and the clicked rows by value."""
    _fields_ = [("scene", C.c_void_p), ("n", C.c_int64), ("labels_dev", C.c_void_p), ("piece_qv_dev", C.c_void_p),
                ("labels_out_dev", C.c_void_p), ("summary_dev", C.c_void_p), ("workspace_dev", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("min_voxels", C.c_int32), ("connectivity", C.c_int32),
                ("n_classes", C.c_int32), ("capacity", C.c_int32), ("n_clicks", C.c_int32), ("reserved_", C.c_int32),
                ("click_row", C.c_int32 * 256)]


A3D_SIMILAR_REF_NORMAL, A3D_SIMILAR_REF_FEAT = 1, 2
A3D_VOTE_OVERFLOW, A3D_VOTE_BAD_LABEL = 1, 2


class SimilarPiecesArgs(C.Structure):
    """a3d_similar_pieces_args: a3d_label_pieces' (keys_dev may be NULL), the normals and colours per voxel (either may be
    NULL), and by value the pairwise thresholds, ``oriented``, the reference test's flags, values and thresholds."""
    _fields_ = [("scene", C.c_void_p), ("n", C.c_int64), ("keys_dev", C.c_void_p), ("inverse_map_dev", C.c_void_p),
                ("n_full", C.c_int64), ("piece_qv_dev", C.c_void_p), ("piece_full_dev", C.c_void_p), ("out_dev", C.c_void_p),
                ("n_out_dev", C.c_void_p), ("workspace_dev", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("normal_qv_dev", C.c_void_p), ("feat_qv_dev", C.c_void_p), ("cos_min", C.c_float), ("tol2", C.c_float),
                ("oriented", C.c_int32), ("ref_flags", C.c_int32), ("ref_normal", C.c_float * 3), ("ref_cos_min", C.c_float),
                ("ref_feat", C.c_float * 3), ("ref_tol2", C.c_float),
                ("connectivity", C.c_int32), ("max_out", C.c_int32), ("n_clicks", C.c_int32), ("reserved_", C.c_int32),
                ("click_row", C.c_int32 * 256)]


class VoteSummary(C.Structure):
    """a3d_vote_summary: eligible pieces (the capacity needed on overflow), uniform, relabelled pieces and voxels, blocked and
    below-share pieces, the error word (A3D_VOTE_OVERFLOW, A3D_VOTE_BAD_LABEL)."""
    _fields_ = [("eligible_pieces", C.c_int32), ("uniform_pieces", C.c_int32), ("relabelled_pieces", C.c_int32),
                ("relabelled_voxels", C.c_int32), ("blocked_pieces", C.c_int32), ("below_share_pieces", C.c_int32),
                ("err", C.c_int32), ("reserved_", C.c_int32)]


class VotePiecesArgs(C.Structure):
    """a3d_vote_pieces_args: the scene, the labels and a partition, the output labels and summary, the workspace of the call
    that wrote the partition, the settings (min_voxels, n_classes, capacity, the share as a fraction) and the clicked rows."""
    _fields_ = [("scene", C.c_void_p), ("n", C.c_int64), ("labels_dev", C.c_void_p), ("piece_qv_dev", C.c_void_p),
                ("labels_out_dev", C.c_void_p), ("summary_dev", C.c_void_p), ("workspace_dev", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("min_voxels", C.c_int32), ("n_classes", C.c_int32), ("capacity", C.c_int32),
                ("share_num", C.c_int32), ("share_den", C.c_int32), ("n_clicks", C.c_int32), ("click_row", C.c_int32 * 256)]


class GrowSummary(C.Structure):
    """a3d_grow_summary: seeds, reached voxels, selected vertices, the largest dist reached, the error word
    (A3D_GROW_BAD_INDEX)."""
    _fields_ = [("seeds", C.c_int64), ("reached", C.c_int64), ("selected", C.c_int64), ("max_dist", C.c_int32),
                ("err", C.c_int32)]


class GrowVoxelsArgs(C.Structure):
    """a3d_grow_voxels_args: the scene, the keys (or NULL), the seeds per voxel and per vertex (one of them at least), the
    lift (inverse_map, n_full), the optional outputs, the summary, the workspace, and by value the connectivity, the limit and
    the face / edge / corner step costs."""
    _fields_ = [("scene", C.c_void_p), ("n", C.c_int64), ("keys_dev", C.c_void_p), ("seed_qv_dev", C.c_void_p),
                ("seed_full_dev", C.c_void_p), ("inverse_map_dev", C.c_void_p), ("n_full", C.c_int64),
                ("dist_qv_dev", C.c_void_p), ("owner_qv_dev", C.c_void_p), ("selected_full_dev", C.c_void_p),
                ("dist_full_dev", C.c_void_p), ("summary_dev", C.c_void_p), ("workspace_dev", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("connectivity", C.c_int32), ("limit", C.c_int32), ("cost", C.c_int32 * 3),
                ("reserved_", C.c_int32)]


class NormalsSummary(C.Structure):
    """a3d_normals_summary: counted vertices, voxels with and without a valid normal, the error word (A3D_NORMALS_RANGE,
    A3D_NORMALS_BAD_INDEX)."""
    _fields_ = [("counted", C.c_int64), ("valid", C.c_int64), ("invalid", C.c_int64), ("err", C.c_int32),
                ("reserved_", C.c_int32)]


class EstimateNormalsArgs(C.Structure):
    """a3d_estimate_normals_args: the scene, the vertices and their inverse map (or NULL), the optional outputs per voxel and
    per vertex, the summary, the workspace, and by value the fixed-point frame (origin, quantum, bits) and the viewpoint with
    its flag."""
    _fields_ = [("scene", C.c_void_p), ("n", C.c_int64), ("xyz_dev", C.c_void_p), ("inverse_map_dev", C.c_void_p),
                ("n_full", C.c_int64), ("normal_qv_dev", C.c_void_p), ("variation_qv_dev", C.c_void_p),
                ("count_qv_dev", C.c_void_p), ("moments_qv_dev", C.c_void_p), ("normal_full_dev", C.c_void_p),
                ("summary_dev", C.c_void_p), ("workspace_dev", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("origin", C.c_double * 3), ("quantum", C.c_double), ("viewpoint", C.c_double * 3), ("bits", C.c_int32),
                ("has_viewpoint", C.c_int32)]


class OrientSummary(C.Structure):
    """a3d_orient_summary: admitted rows, seeds, reached and unreached rows, flipped rows, conflicting edges, the largest dist,
    whether the last sweep was quiet, the error word (A3D_ORIENT_BAD_INDEX, A3D_ORIENT_BAD_COMPONENT)."""
    _fields_ = [("admitted", C.c_int64), ("seeds", C.c_int64), ("reached", C.c_int64), ("unreached", C.c_int64),
                ("flipped", C.c_int64), ("conflicts", C.c_int64), ("max_dist", C.c_int32), ("converged", C.c_int32),
                ("err", C.c_int32), ("reserved_", C.c_int32)]


class OrientNormalsArgs(C.Structure):
    """a3d_orient_normals_args: the scene, the normals per voxel, the seeds of either mode (marks and flips; components and
    positions), the lift (inverse_map, n_full), the optional outputs, the summary, the workspace, and by value the viewpoint,
    the mode, the connectivity, the number of sweeps and whether the call resumes."""
    _fields_ = [("scene", C.c_void_p), ("n", C.c_int64), ("normal_qv_dev", C.c_void_p), ("seed_qv_dev", C.c_void_p),
                ("seed_flip_dev", C.c_void_p), ("component_qv_dev", C.c_void_p), ("position_qv_dev", C.c_void_p),
                ("inverse_map_dev", C.c_void_p), ("n_full", C.c_int64), ("normal_out_qv_dev", C.c_void_p),
                ("flipped_qv_dev", C.c_void_p), ("dist_qv_dev", C.c_void_p), ("owner_qv_dev", C.c_void_p),
                ("normal_full_dev", C.c_void_p), ("summary_dev", C.c_void_p), ("workspace_dev", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("viewpoint", C.c_double * 3), ("mode", C.c_int32), ("connectivity", C.c_int32),
                ("sweeps", C.c_int32), ("resume", C.c_int32)]


class TransferSummary(C.Structure):
    """a3d_transfer_summary: matched, unmatched and non-finite queries, source rows left out as not finite, the error word
    (A3D_TRANSFER_UNKEYABLE, A3D_TRANSFER_SORT_FAILED)."""
    _fields_ = [("matched", C.c_int64), ("unmatched", C.c_int64), ("nonfinite", C.c_int64), ("source_left_out", C.c_int64),
                ("err", C.c_int32), ("reserved_", C.c_int32)]


class PrototypesSummary(C.Structure):
    """a3d_prototypes_summary: example rows summed, example rows left out (a channel beyond the fixed-point range or not finite),
    the error word (A3D_MATCH_BAD_CLASS)."""
    _fields_ = [("examples", C.c_int64), ("examples_left_out", C.c_int64), ("err", C.c_int32), ("reserved_", C.c_int32)]


class FeaturePrototypesArgs(C.Structure):
    """a3d_feature_prototypes_args: the features and the example classes per row, the integer sums and counts per class, the
    summary, the number of classes."""
    _fields_ = [("feats_dev", C.c_void_p), ("classes_dev", C.c_void_p), ("n", C.c_int64), ("sums_dev", C.c_void_p),
                ("count_dev", C.c_void_p), ("summary_dev", C.c_void_p), ("n_classes", C.c_int32), ("reserved_", C.c_int32)]


class MatchSummary(C.Structure):
    """a3d_match_summary: matched voxels per class, rows with a channel that is not finite, the error word (A3D_MATCH_BAD_CLASS,
    A3D_MATCH_BAD_INDEX, A3D_MATCH_BAD_PROTOTYPE)."""
    _fields_ = [("matched", C.c_int64 * 256), ("rows_nonfinite", C.c_int64), ("err", C.c_int32), ("reserved_", C.c_int32)]


class FeatureMatchArgs(C.Structure):
    """a3d_feature_match_args: the features, the prototypes and their classes, the optional candidate mask and lift
    (inverse_map, n_full), the outputs per voxel and per vertex, the summary, and by value cos_min and k."""
    _fields_ = [("feats_dev", C.c_void_p), ("n", C.c_int64), ("protos_dev", C.c_void_p), ("proto_class_dev", C.c_void_p),
                ("candidate_dev", C.c_void_p), ("inverse_map_dev", C.c_void_p), ("n_full", C.c_int64),
                ("match_qv_dev", C.c_void_p), ("best_qv_dev", C.c_void_p), ("score_qv_dev", C.c_void_p),
                ("match_full_dev", C.c_void_p), ("score_full_dev", C.c_void_p), ("summary_dev", C.c_void_p),
                ("cos_min", C.c_double), ("k", C.c_int32), ("reserved_", C.c_int32)]


class Plane(C.Structure):
    """a3d_plane: one plane of a3d_find_planes -- the normal (canonical sign) and offset (``normal . p = offset`` in scene
    coordinates), the inlier count, the peak's score and flat bin, the round, the integer sums of the final inliers (count, sum,
    mom), the integer form ``N . X = off`` and the rms distance of the inliers."""
    _fields_ = [("normal", C.c_float * 3), ("offset", C.c_float), ("inliers", C.c_int32), ("score", C.c_int32),
                ("round", C.c_int32), ("bin", C.c_int32), ("count", C.c_int64), ("sum", C.c_int64 * 3), ("mom", C.c_int64 * 6),
                ("off", C.c_int64), ("N", C.c_int32 * 3), ("rms", C.c_float)]


class PlanesSummary(C.Structure):
    """a3d_planes_summary: planes, rounds that passed the stop test, spent rounds, admitted rows, the rows left out per reason
    (A3D_PLANES_OUT_*), the error word (A3D_PLANES_BAD_INDEX)."""
    _fields_ = [("n_planes", C.c_int32), ("rounds", C.c_int32), ("spent", C.c_int32), ("admitted", C.c_int32),
                ("left_out", C.c_int32 * 5), ("err", C.c_int32), ("reserved_", C.c_int32 * 2)]


class PlanesOut(C.Structure):
    """a3d_planes_out: the records in the order found, then the summary."""
    _fields_ = [("plane", Plane * 16), ("summary", PlanesSummary)]


class FindPlanesArgs(C.Structure):
    """a3d_find_planes_args: the normals and positions per row, the optional candidate mask, the host's direction table, the
    optional lift (inverse_map, n_full), the outputs, the workspace, and by value the fixed-point frame and the settings."""
    _fields_ = [("normal_dev", C.c_void_p), ("pos_dev", C.c_void_p), ("candidate_dev", C.c_void_p), ("n", C.c_int64),
                ("table_dev", C.c_void_p), ("inverse_map_dev", C.c_void_p), ("n_full", C.c_int64), ("plane_qv_dev", C.c_void_p),
                ("plane_full_dev", C.c_void_p), ("out_dev", C.c_void_p), ("workspace_dev", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("origin", C.c_double * 3), ("quantum", C.c_double), ("cos_min", C.c_double),
                ("bin_width", C.c_int64), ("dist_tol", C.c_int64), ("bits", C.c_int32), ("min_voxels", C.c_int32),
                ("max_planes", C.c_int32), ("reserved_", C.c_int32)]


class ObjectMoments(C.Structure):
    """a3d_object_moments: one object of a labelling -- vertices and voxels, the sums of the fixed-point coordinates (X, Y, Z)
    and of their products (XX, XY, XZ, YY, YZ, ZZ), the covered surface in thirds of area quanta, the exact fp32 box."""
    _fields_ = [("vertices", C.c_int64), ("voxels", C.c_int64), ("sum", C.c_int64 * 3), ("mom", C.c_int64 * 6),
                ("area_thirds", C.c_int64), ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("reserved_", C.c_int32 * 2)]


class MeasureArgs(C.Structure):
    """a3d_measure_args: the vertices and their labels, optionally the voxels' labels and the faces, the records and the
    error word, and by value the fixed-point frame (origin, quantum, bits), the area quantum and the number of object ids."""
    _fields_ = [("xyz_dev", C.c_void_p), ("labels_dev", C.c_void_p), ("n", C.c_int64), ("labels_qv_dev", C.c_void_p),
                ("n_qv", C.c_int64), ("faces_dev", C.c_void_p), ("m", C.c_int64), ("out_dev", C.c_void_p),
                ("err_dev", C.c_void_p), ("origin", C.c_double * 3), ("quantum", C.c_double), ("area_quantum", C.c_double),
                ("n_classes", C.c_int32), ("bits", C.c_int32)]


class ExtentsArgs(C.Structure):
    """a3d_extents_args: the vertices and their labels, three axes per object, the (min, max) per (object, axis) and the
    error word."""
    _fields_ = [("xyz_dev", C.c_void_p), ("labels_dev", C.c_void_p), ("n", C.c_int64), ("axes_dev", C.c_void_p),
                ("out_dev", C.c_void_p), ("err_dev", C.c_void_p), ("n_classes", C.c_int32), ("reserved_", C.c_int32)]


class Camera(C.Structure):
    """a3d_camera: pixel (u, v)'s ray starts at o and runs along normalize(d00 + u du + v dv), evaluated in fp32."""
    _fields_ = [("o", C.c_float * 3), ("d00", C.c_float * 3), ("du", C.c_float * 3), ("dv", C.c_float * 3),
                ("width", C.c_int32), ("height", C.c_int32)]


class RenderHeader(C.Structure):
    """a3d_render_header: flags (bit 0 = a face index out of range, bit 1 = pair capacity too small, images untouched),
    the primitives every pixel tested, the (tile, primitive) pairs the call needs."""
    _fields_ = [("flags", C.c_int32), ("n_everywhere", C.c_int32), ("pairs_needed", C.c_int64)]


class RenderOut(C.Structure):
    """a3d_render_out: the images of a3d_render_mesh / a3d_render_points (u_dev, v_dev optional) and the header."""
    _fields_ = [("id_dev", C.c_void_p), ("t_dev", C.c_void_p), ("u_dev", C.c_void_p), ("v_dev", C.c_void_p),
                ("header_dev", C.c_void_p)]


class Section(C.Structure):
    """a3d_section: up to 8 planes (nx, ny, nz, c), each keeping the side n . p >= c, and a culling mode (meshes only)."""
    _fields_ = [("n_planes", C.c_int32), ("cull", C.c_int32), ("planes", (C.c_float * 4) * 8)]


class SelectSummary(C.Structure):
    """a3d_select_summary: selected vertices, vertices in view, flags (bit 0 = a coordinate that is not finite)."""
    _fields_ = [("selected", C.c_int64), ("in_view", C.c_int64), ("flags", C.c_int32), ("reserved_", C.c_int32)]


class SelectArgs(C.Structure):
    """a3d_select_args: the vertices, the camera and the fp32 rows of [du dv d00]^-1, the depth slack, the mask and (or NULL)
    the t image, the section (a HOST pointer or NULL), the selection and the summary."""
    _fields_ = [("xyz_dev", C.c_void_p), ("n", C.c_int64), ("camera", Camera), ("rows", C.c_float * 9), ("slack", C.c_float),
                ("mask_dev", C.c_void_p), ("t_dev", C.c_void_p), ("section", C.POINTER(Section)), ("selected_dev", C.c_void_p),
                ("summary_dev", C.c_void_p)]


class OverlaySummary(C.Structure):
    """a3d_overlay_summary: layer entries the call altered, vertices overridden after it, those whose manual label differs
    from the model's, the error word (bit 0 = a label outside 0..255 where it was used)."""
    _fields_ = [("changed", C.c_int64), ("overridden", C.c_int64), ("differing", C.c_int64), ("err", C.c_int32),
                ("reserved_", C.c_int32)]


class SessionOverlayArgs(C.Structure):
    """a3d_session_overlay_args: the model's labels, the manual layer (on, obj; in/out), the selection (or NULL), the colours and
    the palette, the outputs (NULL together: a pure layer update), the summary, the operation and its object."""
    _fields_ = [("labels_in_dev", C.c_void_p), ("n", C.c_int64), ("manual_on_dev", C.c_void_p), ("manual_obj_dev", C.c_void_p),
                ("selected_dev", C.c_void_p), ("colors_full_dev", C.c_void_p), ("palette_dev", C.c_void_p),
                ("labels_out_dev", C.c_void_p), ("colors_out_dev", C.c_void_p), ("summary_dev", C.c_void_p), ("op", C.c_int32),
                ("obj", C.c_int32), ("n_palette", C.c_int32), ("reserved_", C.c_int32)]


class ClickCluster(C.Structure):
    _fields_ = [("cluster_id", C.c_int32), ("row", C.c_int32), ("label", C.c_int32), ("pred", C.c_int32),
                ("error_size", C.c_float)]


A3D_MAX_CLICKS = 256
A3D_NEAREST_MAX_QUERIES = 64
A3D_NEAREST_MAX_SOURCES = 4
A3D_RENDER_MAX_SIZE = 4096
A3D_RENDER_TILE = 16
A3D_RENDER_BAD_INDEX, A3D_RENDER_OVERFLOW = 1, 2
A3D_SECTION_MAX_PLANES = 8
A3D_CULL_NONE, A3D_CULL_BACK, A3D_CULL_FRONT = 0, 1, 2
A3D_REGION_MAX_POINTS = 256
A3D_REGION_POLYGON, A3D_REGION_STROKE = 0, 1
A3D_REGION_REPLACE, A3D_REGION_ADD, A3D_REGION_SUBTRACT = 0, 1, 2
A3D_SELECT_NOT_FINITE = 1
A3D_OVERLAY_NONE, A3D_OVERLAY_PAINT, A3D_OVERLAY_ERASE = 0, 1, 2
A3D_MEASURE_RANGE, A3D_MEASURE_BAD_LABEL = 1, 2
A3D_MEASURE_MAX_BITS, A3D_MEASURE_MAX_Q, A3D_MEASURE_MAX_FACES = 20, 1 << 38, 1 << 23
A3D_MEASURE_BLOCK, A3D_MEASURE_CHUNK = 256, 1024
A3D_GROW_MAX_STEPS, A3D_GROW_BAD_INDEX = 1024, 1
A3D_NORMALS_RANGE, A3D_NORMALS_BAD_INDEX = 1, 2
A3D_ORIENT_MAX_ROWS, A3D_ORIENT_MAX_SWEEPS = 1 << 21, 4096
A3D_ORIENT_GIVEN, A3D_ORIENT_NEAREST = 0, 1
A3D_ORIENT_BAD_INDEX, A3D_ORIENT_BAD_COMPONENT = 1, 2
A3D_TRANSFER_UNKEYABLE, A3D_TRANSFER_SORT_FAILED = 1, 2
A3D_MATCH_CHANNELS, A3D_MATCH_QUANTUM_BITS, A3D_MATCH_FIXED_BITS = 128, 20, 40
A3D_MATCH_MAX_EXAMPLE_ROWS, A3D_MATCH_MAX_PROTOTYPES, A3D_MATCH_CHUNK = 1 << 22, 256, 16
A3D_MATCH_BAD_CLASS, A3D_MATCH_BAD_INDEX, A3D_MATCH_BAD_PROTOTYPE = 1, 2, 4
A3D_PLANES_MAX, A3D_PLANES_GRID, A3D_PLANES_BINS, A3D_PLANES_SCALE_BITS = 16, 16, 1024, 20
(A3D_PLANES_OUT_CANDIDATE, A3D_PLANES_OUT_NONFINITE, A3D_PLANES_OUT_ZERO, A3D_PLANES_OUT_FRAME,
 A3D_PLANES_OUT_BINS) = range(5)
A3D_PLANES_BAD_INDEX = 1
A3D_ERR_INVALID = -1
A3D_ERR_WORKSPACE = -5
PROF_DENSE = 11
PROF_NAMES = ["spconv", "splitk_epilogue", "stem", "c2s_attn", "query_chain", "s2c_attn", "ln_mask", "posenc",
              "scene_sort_levels", "scene_tables", "click_simulator", "dense_gemm"]

# name -> (restype, argtypes): every symbol include/agile3d_hip.h declares
SYMBOLS = {
    "a3d_version": (C.c_int, []),
    "a3d_last_error": (C.c_char_p, []),
    "a3d_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_profile_enable": (C.c_int, [C.c_int]),
    "a3d_profile_read": (C.c_int, [C.POINTER(ProfEntry), C.c_int]),
    "a3d_scene_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "a3d_sort_pairs_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "a3d_sort_pairs_u64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p]),
    "a3d_scene_create": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p,
                                   C.POINTER(C.c_void_p)]),
    "a3d_scene_destroy": (None, [C.c_void_p]),
    "a3d_scene_level_size": (C.c_int64, [C.c_void_p, C.c_int]),
    "a3d_scene_batch_ranges": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "a3d_scene_grid_dims": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "a3d_scene_table": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "a3d_pack_conv_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "a3d_conv_weight_packed_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "a3d_pack_conv_weights_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p]),
    "a3d_conv_deep_mode": (C.c_int, [C.c_int]),
    "a3d_program_workspace_bytes": (C.c_size_t, [C.c_void_p, C.POINTER(BufDesc), C.c_int, C.POINTER(Op), C.c_int]),
    "a3d_program_buffer_offset": (C.c_size_t, [C.c_void_p, C.POINTER(BufDesc), C.c_int, C.c_int]),
    "a3d_program_run": (C.c_int, [C.c_void_p, C.POINTER(BufDesc), C.c_int, C.POINTER(Op), C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_linear": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_posenc_fourier": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p]),
    "a3d_posenc_batch_workspace_bytes": (C.c_size_t, [C.c_int]),
    "a3d_posenc_fourier_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_posenc": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_size_t, C.c_void_p]),
    "a3d_posenc_batch": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_decoder_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "a3d_decoder_query_pack_floats": (C.c_size_t, [C.c_int32]),
    "a3d_decoder_mask_pack_floats": (C.c_size_t, []),
    "a3d_decoder_pack_query_weights": (C.c_int, [C.POINTER(DecoderWeights), C.c_int32, C.c_void_p, C.c_void_p]),
    "a3d_scene_wgrad_lists_bytes": (C.c_size_t, [C.c_void_p]),
    "a3d_scene_build_wgrad_lists": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_conv_wgrad_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "a3d_conv_wgrad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                 C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_conv_apply_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "a3d_conv_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_conv_state_bytes": (C.c_size_t, []),
    "a3d_conv_apply_acc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "a3d_conv_bn_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "a3d_conv_dgrad_bn": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_conv_bn_train_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int,
                                            C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_stem_wgrad_workspace_bytes": (C.c_size_t, [C.c_int]),
    "a3d_stem_wgrad_scene_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "a3d_stem_wgrad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p]),
    "a3d_bn_local_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_bn_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "a3d_bn_backward_sums": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_bn_backward_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "a3d_layernorm_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                        C.c_void_p, C.c_int, C.c_void_p]),
    "a3d_layernorm_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p,
                                         C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    "a3d_linear_wgrad_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "a3d_linear_wgrad": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_linear_wgrad_into_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "a3d_linear_wgrad_into": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                        C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_attn_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "a3d_softmax_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "a3d_softmax_rows_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "a3d_softmax_cols": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p]),
    "a3d_softmax_cols_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p]),
    "a3d_attn_apply_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int]),
    "a3d_attn_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float,
                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_group_max": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    "a3d_next_layer_mask_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "a3d_next_layer_mask": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_group_max_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "a3d_flash_c2s_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "a3d_flash_c2s_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_flash_c2s_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    "a3d_flash_s2c_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "a3d_flash_s2c_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "a3d_flash_s2c_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_dropout_mask": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
                                   C.c_void_p]),
    "a3d_flash_c2s_forward_dropout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, Dropout, C.c_void_p]),
    "a3d_flash_c2s_backward_dropout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_size_t, Dropout, C.c_void_p]),
    "a3d_flash_s2c_forward_dropout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                                C.c_void_p, Dropout, C.c_void_p]),
    "a3d_flash_s2c_backward_dropout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_size_t, Dropout, C.c_void_p]),
    "a3d_attn_dropout": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p, Dropout, C.c_void_p]),
    "a3d_dropout_rows_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, Dropout,
                                           C.c_void_p]),
    "a3d_dropout_rows_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, Dropout, C.c_void_p]),
    "a3d_sum_squares_workspace_bytes": (C.c_size_t, []),
    "a3d_sum_squares": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_sum_squares_accumulate": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_adamw_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double,
                                 C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "a3d_mt_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "a3d_sum_squares_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_adamw_step_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double,
                                       C.c_double, C.c_double, C.c_void_p]),
    "a3d_bn_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "a3d_bn_train_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                       C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_bn_train_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "a3d_column_sums": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                  C.c_void_p]),
    "a3d_decoder_forward_batch": (C.c_int, [C.POINTER(DecoderWeights), C.POINTER(DecoderSample), C.c_int, C.c_void_p]),
    "a3d_decoder_forward": (C.c_int, [C.POINTER(DecoderWeights), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_void_p]),
    "a3d_argmax_labels": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.c_int, C.c_void_p, C.c_void_p]),
    "a3d_iou_counts": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                 C.c_void_p]),
    "a3d_argmax_labels_batch_workspace_bytes": (C.c_size_t, [C.c_int]),
    "a3d_argmax_labels_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_iou_counts_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "a3d_click_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "a3d_click_clusters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_click_clusters_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "a3d_click_spatial_order_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "a3d_click_spatial_order": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_mask_losses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_float,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_quantize_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "a3d_sparse_quantize": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_int64), C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_click_loss_weights": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_int, C.c_float,
                                         C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "a3d_session_workspace_bytes": (C.c_size_t, []),
    "a3d_nearest_rows": (C.c_int, [C.POINTER(NearestSource), C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_size_t,
                                   C.c_void_p]),
    "a3d_pick_ray": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_void_p,
                               C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_pick_mesh": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_pick_ray_section": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float,
                                       C.POINTER(Section), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_pick_mesh_section": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                        C.POINTER(Section), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_section_ray": (C.c_int, [C.POINTER(Section), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "a3d_session_paint": (C.c_int, [C.POINTER(SessionPaintArgs), C.c_void_p]),
    "a3d_session_edit": (C.c_int, [C.POINTER(SessionEditArgs), C.c_void_p]),
    "a3d_session_guide": (C.c_int, [C.POINTER(SessionGuideArgs), C.c_void_p]),
    "a3d_pieces_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "a3d_label_pieces": (C.c_int, [C.POINTER(LabelPiecesArgs), C.c_void_p]),
    "a3d_absorb_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "a3d_absorb_pieces": (C.c_int, [C.POINTER(AbsorbPiecesArgs), C.c_void_p]),
    "a3d_similar_pieces": (C.c_int, [C.POINTER(SimilarPiecesArgs), C.c_void_p]),
    "a3d_similar_pair": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                   C.c_float, C.c_float, C.c_int]),
    "a3d_vote_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "a3d_vote_pieces": (C.c_int, [C.POINTER(VotePiecesArgs), C.c_void_p]),
    "a3d_grow_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "a3d_grow_voxels": (C.c_int, [C.POINTER(GrowVoxelsArgs), C.c_void_p]),
    "a3d_normals_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "a3d_estimate_normals": (C.c_int, [C.POINTER(EstimateNormalsArgs), C.c_void_p]),
    "a3d_normals_solve": (C.c_int, [C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_double,
                                    C.POINTER(C.c_double), C.POINTER(C.c_float)]),
    "a3d_orient_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "a3d_orient_normals": (C.c_int, [C.POINTER(OrientNormalsArgs), C.c_void_p]),
    "a3d_orient_edge": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "a3d_point_index_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "a3d_point_index_create": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p,
                                         C.POINTER(C.c_void_p)]),
    "a3d_point_index_destroy": (None, [C.c_void_p]),
    "a3d_point_index_nearest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "a3d_feature_prototypes": (C.c_int, [C.POINTER(FeaturePrototypesArgs), C.c_void_p]),
    "a3d_feature_match": (C.c_int, [C.POINTER(FeatureMatchArgs), C.c_void_p]),
    "a3d_planes_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "a3d_find_planes": (C.c_int, [C.POINTER(FindPlanesArgs), C.c_void_p]),
    "a3d_cull_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "a3d_render_shade_lit_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(Camera), C.c_float,
                                              C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
    "a3d_region_mask": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_float, C.c_int, C.c_void_p,
                                  C.c_void_p]),
    "a3d_select_vertices": (C.c_int, [C.POINTER(SelectArgs), C.c_void_p]),
    "a3d_session_overlay": (C.c_int, [C.POINTER(SessionOverlayArgs), C.c_void_p]),
    "a3d_measure_objects": (C.c_int, [C.POINTER(MeasureArgs), C.c_void_p]),
    "a3d_object_extents": (C.c_int, [C.POINTER(ExtentsArgs), C.c_void_p]),
    "a3d_render_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int64]),
    "a3d_render_camera_bounds": (C.c_int, [C.POINTER(Camera), C.POINTER(C.c_double)]),
    "a3d_render_mesh": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(Camera), C.POINTER(RenderOut),
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_render_points": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.POINTER(Camera), C.POINTER(RenderOut), C.c_void_p,
                                    C.c_size_t, C.c_void_p]),
    "a3d_render_mesh_section": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(Camera), C.POINTER(Section),
                                          C.POINTER(RenderOut), C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_render_points_section": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.POINTER(Camera), C.POINTER(Section),
                                            C.POINTER(RenderOut), C.c_void_p, C.c_size_t, C.c_void_p]),
    "a3d_render_shade": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                   C.POINTER(C.c_float), C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "a3d_vertex_normals": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "a3d_render_shade_lit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.POINTER(Camera), C.c_float, C.POINTER(C.c_float), C.c_void_p,
                                       C.c_void_p]),
    "a3d_render_shade_depth": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_int64, C.c_float, C.POINTER(C.c_float), C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p]),
    "a3d_render_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "a3d_render_annotate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                      C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_int, C.c_int,
                                      C.c_void_p]),
}

_lib = None


class A3DError(RuntimeError):
    pass


ABI_VERSION = 4   # include/agile3d_hip.h: A3D_ABI_VERSION


def load():
    """dlopen the in-tree library and bind every symbol.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if os.environ.get("A3D_CONV_EMU", "0") != "0":   # refuse rather than run the exact build under the old switch's name
        raise A3DError("A3D_CONV_EMU: the emulated-fp32 (bf16 x 6) convolution build was removed; unset the variable "
                       "or set it to 0 (every convolution runs the exact-fp32 build)")
    if not os.path.exists(LIB_PATH):
        raise A3DError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    got = lib.a3d_version()
    if got != ABI_VERSION:   # struct layouts / buffer contracts of another revision: refuse before the first real call
        raise A3DError(f"{LIB_PATH} speaks interface version {got}, this binding was written against {ABI_VERSION} "
                       "(include/agile3d_hip.h: A3D_ABI_VERSION); rebuild the library")
    _lib = lib
    return lib


def ptr(t):
    """The device pointer of ``t`` as the C ABI takes it (``None``: a null pointer); nothing is checked."""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # torch's own shortcut past the Stream object


def stream(device=None):
    """The current stream of ``device`` (a CUDA ``torch.device``; ``None``: the current device), what every library call launches
    on: ``torch.cuda.current_stream(device).cuda_stream``, read without building the ``Stream`` object where torch allows."""
    if _raw_stream is None or (device is not None and device.type != "cuda"):      # (torch refuses a device that is not CUDA)
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    index = torch.cuda.current_device() if device is None or device.index is None else device.index
    return C.c_void_p(_raw_stream(index))


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().a3d_last_error()
        raise A3DError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
