"""ctypes binding of the C ABI in include/vslam.h (visualslam_amd/lib/libvslam.so).

This is plumbing only: argument marshalling for numpy (host entry points) and for torch
CUDA tensors (device entry points).  All compute happens in the hand-written HIP kernels
behind the ABI; there is no fallback -- if the library is missing or HIP cannot run, the
calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# VSLAM_LIBRARY: development switch for A/B timing of two builds of the same library on one box
# (tools/ab_libs.sh); everything else uses the in-tree build.
LIB_PATH = os.environ.get("VSLAM_LIBRARY") or os.path.join(_HERE, "lib", "libvslam.so")
# the diagnostics build (-DVSLAM_DIAGNOSTICS: the reference-path environment switches); a test / tool that needs one starts its child
# process with VSLAM_LIBRARY=DIAG_LIB_PATH
DIAG_LIB_PATH = os.path.join(_HERE, "lib", "libvslam_diag.so")
CSRC = os.path.join(_HERE, "csrc")

MAX_OCTAVES = 16
NUM_LEVELS = 6
NUM_DOGS = 5

POINT_DTYPE = np.dtype([(n, "<i4") for n in ("row", "col", "value", "padding", "octave", "level")], align=True)
KP_DTYPE = np.dtype([("row", "<i4"), ("col", "<i4"), ("response", "<f4")], align=True)
NN2_DTYPE = np.dtype([("index", "<i4"), ("dist2", "<f4"), ("second_dist2", "<f4")], align=True)  # vslam_nn2
MATCH_DTYPE = np.dtype([("query", "<i4"), ("train", "<i4"), ("dist2", "<f4")], align=True)  # vslam_match
RNN_DTYPE = np.dtype([("index", "<i4"), ("dist2", "<f4")], align=True)  # vslam_rnn, 8 bytes
PLACE_CAND_DTYPE = np.dtype([("frame", "<i4"), ("score", "<u4"), ("norm", "<u4")], align=True)  # vslam_place_cand, 12 bytes
SET_PAIR_DTYPE = np.dtype([("query_set", "<i4"), ("train_set", "<i4")], align=True)  # vslam_set_pair, 8 bytes
LOOP_DTYPE = np.dtype([("query_set", "<i4"), ("train_set", "<i4"), ("slot", "<i4"), ("n_matches", "<u4"), ("n_inliers", "<u4")], align=True)  # vslam_loop, 20 bytes
KMEANS_ROUND_DTYPE = np.dtype([(n, "<u4") for n in ("assigned", "changed", "empty", "ran")], align=True)  # vslam_kmeans_round, 16 bytes
EPIPOLAR_HYP_DTYPE = np.dtype([("F", "<f8", (9,)), ("inliers", "<u4"), ("valid", "<i4")], align=True)  # vslam_epipolar_hyp, 80 bytes
EPIPOLAR_DTYPE = np.dtype([("F", "<f8", (9,)), ("n_matches", "<u4"), ("n_inliers", "<u4"), ("best", "<i4"), ("n_valid", "<u4")], align=True)  # vslam_epipolar, 88 bytes
HOMOGRAPHY_HYP_DTYPE = np.dtype([("H", "<f8", (9,)), ("G", "<f8", (9,)), ("inliers", "<u4"), ("valid", "<i4")], align=True)  # vslam_homography_hyp, 152 bytes
HOMOGRAPHY_DTYPE = np.dtype([("H", "<f8", (9,)), ("G", "<f8", (9,)), ("n_matches", "<u4"), ("n_inliers", "<u4"), ("best", "<i4"), ("n_valid", "<u4"),
                             ("n_epipolar", "<u4"), ("degenerate", "<i4")], align=True)  # vslam_homography, 168 bytes
GUIDED_PARAMS_DTYPE = np.dtype([("ratio2", "<f4"), ("max_desc_dist2", "<f4"), ("max_dist2", "<f8"), ("same_octave", "<i4"), ("reserved", "<u4")],
                               align=True)  # vslam_guided_params, 24 bytes
GUIDED_HF_PARAMS_DTYPE = np.dtype([("ratio2", "<f4"), ("max_desc_dist2", "<f4"), ("max_dist2", "<f8"), ("max_transfer2", "<f8"), ("same_octave", "<i4"),
                                   ("reserved", "<u4")], align=True)  # vslam_guided_hf_params, 32 bytes
REFIT_DTYPE = np.dtype([("n_before", "<u4"), ("n_after", "<u4"), ("accepted", "<u4"), ("stop", "<i4")], align=True)  # vslam_refit, 16 bytes
HREFIT_DTYPE = REFIT_DTYPE  # vslam_hrefit, 16 bytes: the fields and stop codes of vslam_refit
POSE_CAND_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("front", "<u4"), ("valid", "<i4")], align=True)  # vslam_pose_cand, 104 bytes
POSE_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("n_matches", "<u4"), ("n_front", "<u4"), ("best", "<i4"), ("valid", "<i4")], align=True)  # vslam_pose, 112 bytes
HPOSE_CAND_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("n", "<f8", (3,)), ("front", "<u4"), ("valid", "<i4")], align=True)  # vslam_hpose_cand, 128 bytes
HPOSE_DTYPE = np.dtype([("R", "<f8", (9,)), ("n", "<f8", (3,)), ("inv_d", "<f8"), ("spread", "<f8"), ("n_matches", "<u4"), ("n_support", "<u4"), ("front", "<u4"),
                        ("front_runner", "<u4"), ("kind", "<i4"), ("best", "<i4"), ("ambiguous", "<i4"), ("resolved", "<i4")], align=True)  # vslam_hpose, 144 bytes
HPOSE_NONE, HPOSE_PLANE, HPOSE_ROTATION = 0, 1, 2  # vslam_hpose.kind
# What the tools pass unless told otherwise: min_spread is the geometric mean of the largest spread of the planted
# pure rotations (6.527e-3) and the smallest of the planted planes (0.1273); a runner-up within 9 / 10 of the winner is a twin.
HPOSE_MIN_SPREAD, HPOSE_AMBIGUOUS_NUM, HPOSE_AMBIGUOUS_DEN = 0.0288, 9, 10
CHAIN_DTYPE = np.dtype([("W", "<f8", (9,)), ("w", "<f8", (3,)), ("C", "<f8", (3,)), ("Ct", "<f8", (3,)), ("scale", "<f8"), ("ratio", "<f8"), ("n_links", "<u4"),
                        ("segment", "<i4"), ("linked", "<i4"), ("valid", "<i4")], align=True)  # vslam_chain, 176 bytes
RESECT_HYP_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("inliers", "<u4"), ("valid", "<i4")], align=True)  # vslam_resect_hyp, 104 bytes
RESECT_CORR_DTYPE = np.dtype([("Y", "<f8", (3,)), ("u", "<f8"), ("v", "<f8"), ("b", "<u4"), ("reserved", "<u4")], align=True)  # vslam_resect_corr, 48 bytes
RESECT_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("n_obs", "<u4"), ("n_corr", "<u4"), ("n_inliers", "<u4"), ("best", "<i4"),
                         ("n_valid", "<u4"), ("reserved", "<u4")], align=True)  # vslam_resect, 120 bytes
RESECT_REFINE_DTYPE = np.dtype([("n_before", "<u4"), ("n_after", "<u4"), ("accepted", "<u4"), ("stop", "<i4"), ("cost_before", "<f8"),
                                ("cost_after", "<f8")], align=True)  # vslam_resect_refine, 32 bytes
FRAME_CAM_DTYPE = np.dtype([("W", "<f8", (9,)), ("w", "<f8", (3,)), ("segment", "<i4"), ("pair", "<i4"), ("side", "<i4"), ("valid", "<i4")],
                           align=True)  # vslam_frame_cam, 112 bytes
SIM3_HYP_DTYPE = np.dtype([("s", "<f8"), ("R", "<f8", (9,)), ("t", "<f8", (3,)), ("inliers", "<u4"), ("valid", "<i4")], align=True)  # vslam_sim3_hyp, 112 bytes
SIM3_CORR_DTYPE = np.dtype([("X", "<f8", (3,)), ("Y", "<f8", (3,)), ("uq", "<f8"), ("vq", "<f8"), ("ut", "<f8"), ("vt", "<f8"), ("b", "<u4"),
                            ("reserved", "<u4")], align=True)  # vslam_sim3_corr, 88 bytes
SIM3_DTYPE = np.dtype([("s", "<f8"), ("R", "<f8", (9,)), ("t", "<f8", (3,)), ("n_matches", "<u4"), ("n_corr", "<u4"), ("n_inliers", "<u4"), ("best", "<i4"),
                       ("n_valid", "<u4"), ("query_segment", "<i4"), ("train_segment", "<i4"), ("reserved", "<u4")], align=True)  # vslam_sim3, 136 bytes
# What the tools pass unless told otherwise: the squared reprojection threshold of loop alignment, in pixels^2.
SIM3_MAX_DIST2 = 16.0
TRACK_DTYPE = np.dtype([("X", "<f8", (3,)), ("det", "<f8"), ("n_views", "<u4"), ("n_ok", "<u4"), ("status", "<u4"), ("reserved", "<u4")],
                       align=True)  # vslam_track, 48 bytes
TRACK_REF_DTYPE = np.dtype([("head_record", "<u4"), ("pos", "<u4")], align=True)  # vslam_track_ref, 8 bytes
TRACK_SUMMARY_DTYPE = np.dtype([("n_heads", "<u4"), ("n_good", "<u4"), ("max_views", "<u4"), ("reserved", "<u4")], align=True)  # vslam_track_summary, 16 bytes
BUNDLE_CAM_DTYPE = np.dtype([("W", "<f8", (9,)), ("w", "<f8", (3,)), ("C", "<f8", (3,)), ("n_before", "<u4"), ("n_after", "<u4"), ("accepted", "<u4"),
                             ("rejected", "<u4"), ("invalid", "<u4"), ("skipped", "<u4"), ("cost_before", "<f8"), ("cost_after", "<f8")],
                            align=True)  # vslam_bundle_cam, 160 bytes
BUNDLE_POINT_DTYPE = np.dtype([("n_before", "<u4"), ("n_after", "<u4"), ("accepted", "<u4"), ("rejected", "<u4"), ("invalid", "<u4"), ("skipped", "<u4"),
                               ("cost_before", "<f8"), ("cost_after", "<f8")], align=True)  # vslam_bundle_point, 40 bytes


class VslamError(RuntimeError):
    def __init__(self, status: int, what: str, detail: str = ""):
        self.status = status
        super().__init__(f"{what}: status {status} ({_status_string(status)}){': ' + detail if detail else ''}")


class Params(C.Structure):
    _fields_ = [
        ("rows", C.c_int), ("cols", C.c_int), ("n_octaves", C.c_int), ("sigma0", C.c_double),
        ("harris_k", C.c_float), ("do_harris", C.c_int), ("extrema_window", C.c_int),
        ("min_contrast", C.c_int), ("localize", C.c_int), ("orient", C.c_int), ("harris_cap", C.c_uint32), ("dog_cap", C.c_uint32),
        ("oriented_cap", C.c_uint32), ("extrema_dense", C.c_int),
    ]


class BatchLayout(C.Structure):
    _fields_ = [
        ("n_octaves", C.c_int),
        ("rows", C.c_int * MAX_OCTAVES), ("cols", C.c_int * MAX_OCTAVES),
        ("lat_rows", C.c_int * MAX_OCTAVES), ("lat_cols", C.c_int * MAX_OCTAVES), ("lat_words", C.c_int * MAX_OCTAVES),
        ("pitch", C.c_int * MAX_OCTAVES),
        ("octave_offset", C.c_size_t * MAX_OCTAVES), ("pyramid_frame_bytes", C.c_size_t),
        ("bits_offset", C.c_size_t * MAX_OCTAVES), ("bits_frame_words", C.c_size_t),
        ("algorithmic_bytes_harris", C.c_size_t), ("algorithmic_bytes_dog", C.c_size_t),
    ]


BATCH_OUT_FIELDS = ("response", "nms_mask", "nms2", "harris_kps", "harris_counts", "pyramid", "extrema_bits", "dog_points", "dog_counts",
                    "oriented_points", "oriented_counts", "oriented_survivors", "descriptors", "descriptor_defined")


class BatchOut(C.Structure):
    """vslam_batch_out: struct_size, then (pointer, bytes behind it) per output."""
    _fields_ = [("struct_size", C.c_size_t)] + [f for n in BATCH_OUT_FIELDS for f in ((n, C.c_void_p), (n + "_bytes", C.c_size_t))]


class HostLists(C.Structure):
    """vslam_host_lists: the packed host-side lists of vslam_detect_batch_host."""
    _fields_ = [("struct_size", C.c_size_t),
                ("harris", C.c_void_p), ("harris_bytes", C.c_size_t), ("harris_offsets", C.c_void_p), ("harris_counts", C.c_void_p),
                ("dog", C.c_void_p), ("dog_bytes", C.c_size_t), ("dog_offsets", C.c_void_p), ("dog_counts", C.c_void_p)]


class Nn2(C.Structure):
    _fields_ = [("index", C.c_int32), ("dist2", C.c_float), ("second_dist2", C.c_float)]


class Match(C.Structure):
    _fields_ = [("query", C.c_int32), ("train", C.c_int32), ("dist2", C.c_float)]


class DescSets(C.Structure):
    """vslam_desc_sets: n sets of descriptor rows behind device pointers (desc_sets() fills one from torch tensors)."""
    _fields_ = [("desc", C.c_void_p), ("defined", C.c_void_p), ("points", C.c_void_p), ("counts", C.c_void_p), ("cap", C.c_uint32)]


class MatchOut(C.Structure):
    """vslam_match_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("nn", C.c_void_p), ("nn_bytes", C.c_size_t), ("matches", C.c_void_p), ("matches_bytes", C.c_size_t),
                ("match_counts", C.c_void_p), ("match_counts_bytes", C.c_size_t), ("match_cap", C.c_uint32)]


class Rnn(C.Structure):
    _fields_ = [("index", C.c_int32), ("dist2", C.c_float)]


class MatchMutualOut(C.Structure):
    """vslam_match_mutual_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("nn", C.c_void_p), ("nn_bytes", C.c_size_t), ("rnn", C.c_void_p), ("rnn_bytes", C.c_size_t),
                ("matches", C.c_void_p), ("matches_bytes", C.c_size_t), ("match_counts", C.c_void_p), ("match_counts_bytes", C.c_size_t),
                ("match_cap", C.c_uint32)]


class WordsOut(C.Structure):
    """vslam_words_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("words", C.c_void_p), ("words_bytes", C.c_size_t), ("word_dist2", C.c_void_p),
                ("word_dist2_bytes", C.c_size_t), ("hist", C.c_void_p), ("hist_bytes", C.c_size_t)]


class PlaceCand(C.Structure):
    _fields_ = [("frame", C.c_int32), ("score", C.c_uint32), ("norm", C.c_uint32)]


class PlaceParams(C.Structure):
    _fields_ = [("min_gap", C.c_uint32), ("max_candidates", C.c_uint32), ("num", C.c_uint32), ("den", C.c_uint32), ("min_score", C.c_uint32),
                ("reserved", C.c_uint32)]


class PlaceOut(C.Structure):
    """vslam_place_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("candidates", C.c_void_p), ("candidates_bytes", C.c_size_t), ("cand_counts", C.c_void_p),
                ("cand_counts_bytes", C.c_size_t), ("weights", C.c_void_p), ("weights_bytes", C.c_size_t), ("self_q", C.c_void_p),
                ("self_q_bytes", C.c_size_t), ("self_db", C.c_void_p), ("self_db_bytes", C.c_size_t), ("scores", C.c_void_p),
                ("scores_bytes", C.c_size_t)]


class KmeansParams(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("reserved", C.c_uint32)]


class KmeansRound(C.Structure):
    _fields_ = [("assigned", C.c_uint32), ("changed", C.c_uint32), ("empty", C.c_uint32), ("ran", C.c_uint32)]


class KmeansOut(C.Structure):
    """vslam_kmeans_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("vocab", C.c_void_p), ("vocab_bytes", C.c_size_t), ("sizes", C.c_void_p), ("sizes_bytes", C.c_size_t),
                ("report", C.c_void_p), ("report_bytes", C.c_size_t)]


class SetPair(C.Structure):
    _fields_ = [("query_set", C.c_int32), ("train_set", C.c_int32)]


class LoopParams(C.Structure):
    _fields_ = [("min_inliers", C.c_uint32), ("num", C.c_uint32), ("den", C.c_uint32), ("reserved", C.c_uint32)]


class Loop(C.Structure):
    _fields_ = [("query_set", C.c_int32), ("train_set", C.c_int32), ("slot", C.c_int32), ("n_matches", C.c_uint32), ("n_inliers", C.c_uint32)]


class LoopOut(C.Structure):
    """vslam_loop_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("loops", C.c_void_p), ("loops_bytes", C.c_size_t), ("loop_list", C.c_void_p),
                ("loop_list_bytes", C.c_size_t), ("n_loops", C.c_void_p), ("n_loops_bytes", C.c_size_t)]


class FrameCam(C.Structure):
    _fields_ = [("W", C.c_double * 9), ("w", C.c_double * 3), ("segment", C.c_int32), ("pair", C.c_int32), ("side", C.c_int32), ("valid", C.c_int32)]


class FrameWorldOut(C.Structure):
    """vslam_frame_world_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("cams", C.c_void_p), ("cams_bytes", C.c_size_t), ("index", C.c_void_p), ("index_bytes", C.c_size_t)]


class Sim3Side(C.Structure):
    """vslam_sim3_side: one end of the loops behind device (or, for sim3_host, host) pointers (sim3_side() fills one)."""
    _fields_ = [("cams", C.c_void_p), ("index", C.c_void_p), ("map", C.c_void_p), ("points", C.c_void_p), ("map_cap", C.c_uint32),
                ("point_cap", C.c_uint32), ("points_cap", C.c_uint32), ("n_map_pairs", C.c_uint32), ("n_frames", C.c_int32), ("reserved", C.c_int32)]


class Sim3Hyp(C.Structure):
    _fields_ = [("s", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3), ("inliers", C.c_uint32), ("valid", C.c_int32)]


class Sim3Corr(C.Structure):
    _fields_ = [("X", C.c_double * 3), ("Y", C.c_double * 3), ("uq", C.c_double), ("vq", C.c_double), ("ut", C.c_double), ("vt", C.c_double),
                ("b", C.c_uint32), ("reserved", C.c_uint32)]


class Sim3(C.Structure):
    _fields_ = [("s", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3), ("n_matches", C.c_uint32), ("n_corr", C.c_uint32),
                ("n_inliers", C.c_uint32), ("best", C.c_int32), ("n_valid", C.c_uint32), ("query_segment", C.c_int32), ("train_segment", C.c_int32),
                ("reserved", C.c_uint32)]


class Sim3Out(C.Structure):
    """vslam_sim3_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("models", C.c_void_p), ("models_bytes", C.c_size_t), ("inlier_bits", C.c_void_p),
                ("inlier_bits_bytes", C.c_size_t), ("hypotheses", C.c_void_p), ("hypotheses_bytes", C.c_size_t), ("correspondences", C.c_void_p),
                ("correspondences_bytes", C.c_size_t), ("links", C.c_void_p), ("links_bytes", C.c_size_t)]


class EpipolarHyp(C.Structure):
    _fields_ = [("F", C.c_double * 9), ("inliers", C.c_uint32), ("valid", C.c_int32)]


class Epipolar(C.Structure):
    _fields_ = [("F", C.c_double * 9), ("n_matches", C.c_uint32), ("n_inliers", C.c_uint32), ("best", C.c_int32), ("n_valid", C.c_uint32)]


class EpipolarParams(C.Structure):
    _fields_ = [("n_hypotheses", C.c_uint32), ("seed", C.c_uint32), ("max_dist2", C.c_double)]


class EpipolarOut(C.Structure):
    """vslam_epipolar_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("models", C.c_void_p), ("models_bytes", C.c_size_t), ("inlier_bits", C.c_void_p),
                ("inlier_bits_bytes", C.c_size_t), ("inliers", C.c_void_p), ("inliers_bytes", C.c_size_t), ("inlier_counts", C.c_void_p),
                ("inlier_counts_bytes", C.c_size_t), ("inlier_cap", C.c_uint32), ("hypotheses", C.c_void_p), ("hypotheses_bytes", C.c_size_t)]


class GuidedParams(C.Structure):
    _fields_ = [("ratio2", C.c_float), ("max_desc_dist2", C.c_float), ("max_dist2", C.c_double), ("same_octave", C.c_int32), ("reserved", C.c_uint32)]


class GuidedHfParams(C.Structure):
    _fields_ = [("ratio2", C.c_float), ("max_desc_dist2", C.c_float), ("max_dist2", C.c_double), ("max_transfer2", C.c_double), ("same_octave", C.c_int32),
                ("reserved", C.c_uint32)]


class RefitParams(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("max_dist2", C.c_double)]


class Refit(C.Structure):
    _fields_ = [("n_before", C.c_uint32), ("n_after", C.c_uint32), ("accepted", C.c_uint32), ("stop", C.c_int32)]


class RefitOut(C.Structure):
    """vslam_refit_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("models", C.c_void_p), ("models_bytes", C.c_size_t), ("info", C.c_void_p), ("info_bytes", C.c_size_t),
                ("inlier_bits", C.c_void_p), ("inlier_bits_bytes", C.c_size_t), ("inliers", C.c_void_p), ("inliers_bytes", C.c_size_t),
                ("inlier_counts", C.c_void_p), ("inlier_counts_bytes", C.c_size_t), ("inlier_cap", C.c_uint32)]


class HomographyHyp(C.Structure):
    _fields_ = [("H", C.c_double * 9), ("G", C.c_double * 9), ("inliers", C.c_uint32), ("valid", C.c_int32)]


class Homography(C.Structure):
    _fields_ = [("H", C.c_double * 9), ("G", C.c_double * 9), ("n_matches", C.c_uint32), ("n_inliers", C.c_uint32), ("best", C.c_int32),
                ("n_valid", C.c_uint32), ("n_epipolar", C.c_uint32), ("degenerate", C.c_int32)]


class HomographyParams(C.Structure):
    _fields_ = [("n_hypotheses", C.c_uint32), ("seed", C.c_uint32), ("max_dist2", C.c_double), ("degenerate_num", C.c_uint32),
                ("degenerate_den", C.c_uint32), ("min_inliers", C.c_uint32)]


class HomographyOut(C.Structure):
    """vslam_homography_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("models", C.c_void_p), ("models_bytes", C.c_size_t), ("inlier_bits", C.c_void_p),
                ("inlier_bits_bytes", C.c_size_t), ("inliers", C.c_void_p), ("inliers_bytes", C.c_size_t), ("inlier_counts", C.c_void_p),
                ("inlier_counts_bytes", C.c_size_t), ("inlier_cap", C.c_uint32), ("hypotheses", C.c_void_p), ("hypotheses_bytes", C.c_size_t),
                ("gated_models", C.c_void_p), ("gated_models_bytes", C.c_size_t)]


class HRefitParams(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("max_dist2", C.c_double), ("degenerate_num", C.c_uint32), ("degenerate_den", C.c_uint32),
                ("min_inliers", C.c_uint32)]


class HRefit(C.Structure):
    _fields_ = [("n_before", C.c_uint32), ("n_after", C.c_uint32), ("accepted", C.c_uint32), ("stop", C.c_int32)]


class HRefitOut(C.Structure):
    """vslam_hrefit_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("models", C.c_void_p), ("models_bytes", C.c_size_t), ("info", C.c_void_p), ("info_bytes", C.c_size_t),
                ("inlier_bits", C.c_void_p), ("inlier_bits_bytes", C.c_size_t), ("inliers", C.c_void_p), ("inliers_bytes", C.c_size_t),
                ("inlier_counts", C.c_void_p), ("inlier_counts_bytes", C.c_size_t), ("inlier_cap", C.c_uint32), ("gated_models", C.c_void_p),
                ("gated_models_bytes", C.c_size_t)]


class PoseParams(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class PoseCand(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("front", C.c_uint32), ("valid", C.c_int32)]


class Pose(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("n_matches", C.c_uint32), ("n_front", C.c_uint32), ("best", C.c_int32),
                ("valid", C.c_int32)]


class PoseOut(C.Structure):
    """vslam_pose_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("poses", C.c_void_p), ("poses_bytes", C.c_size_t), ("candidates", C.c_void_p),
                ("candidates_bytes", C.c_size_t), ("points", C.c_void_p), ("points_bytes", C.c_size_t), ("front_bits", C.c_void_p),
                ("front_bits_bytes", C.c_size_t)]


class HposeParams(C.Structure):
    _fields_ = [("K", PoseParams), ("max_dist2", C.c_double), ("min_spread", C.c_double), ("ambiguous_num", C.c_uint32), ("ambiguous_den", C.c_uint32),
                ("only_degenerate", C.c_int32), ("reserved", C.c_uint32)]


class HposeCand(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("n", C.c_double * 3), ("front", C.c_uint32), ("valid", C.c_int32)]


class Hpose(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("n", C.c_double * 3), ("inv_d", C.c_double), ("spread", C.c_double), ("n_matches", C.c_uint32),
                ("n_support", C.c_uint32), ("front", C.c_uint32), ("front_runner", C.c_uint32), ("kind", C.c_int32), ("best", C.c_int32),
                ("ambiguous", C.c_int32), ("resolved", C.c_int32)]


class HposeOut(C.Structure):
    """vslam_hpose_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("poses", C.c_void_p), ("poses_bytes", C.c_size_t), ("info", C.c_void_p), ("info_bytes", C.c_size_t),
                ("candidates", C.c_void_p), ("candidates_bytes", C.c_size_t), ("points", C.c_void_p), ("points_bytes", C.c_size_t),
                ("front_bits", C.c_void_p), ("front_bits_bytes", C.c_size_t)]


class ChainParams(C.Structure):
    _fields_ = [("min_links", C.c_uint32)]


class Chain(C.Structure):
    _fields_ = [("W", C.c_double * 9), ("w", C.c_double * 3), ("C", C.c_double * 3), ("Ct", C.c_double * 3), ("scale", C.c_double), ("ratio", C.c_double),
                ("n_links", C.c_uint32), ("segment", C.c_int32), ("linked", C.c_int32), ("valid", C.c_int32)]


class ChainOut(C.Structure):
    """vslam_chain_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("chain", C.c_void_p), ("chain_bytes", C.c_size_t), ("map", C.c_void_p), ("map_bytes", C.c_size_t),
                ("links", C.c_void_p), ("links_bytes", C.c_size_t), ("ratios", C.c_void_p), ("ratios_bytes", C.c_size_t)]


class ResectParams(C.Structure):
    _fields_ = [("n_hypotheses", C.c_uint32), ("seed", C.c_uint32), ("max_dist2", C.c_double), ("K", PoseParams)]


class ResectHyp(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("inliers", C.c_uint32), ("valid", C.c_int32)]


class ResectCorr(C.Structure):
    _fields_ = [("Y", C.c_double * 3), ("u", C.c_double), ("v", C.c_double), ("b", C.c_uint32), ("reserved", C.c_uint32)]


class Resect(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("n_obs", C.c_uint32), ("n_corr", C.c_uint32), ("n_inliers", C.c_uint32),
                ("best", C.c_int32), ("n_valid", C.c_uint32), ("reserved", C.c_uint32)]


class ResectOut(C.Structure):
    """vslam_resect_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("models", C.c_void_p), ("models_bytes", C.c_size_t), ("inlier_bits", C.c_void_p),
                ("inlier_bits_bytes", C.c_size_t), ("hypotheses", C.c_void_p), ("hypotheses_bytes", C.c_size_t), ("correspondences", C.c_void_p),
                ("correspondences_bytes", C.c_size_t), ("links", C.c_void_p), ("links_bytes", C.c_size_t)]


class Sim3Params(C.Structure):
    _fields_ = [("n_hypotheses", C.c_uint32), ("seed", C.c_uint32), ("max_dist2", C.c_double), ("K", PoseParams)]


class ResectRefineParams(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("max_dist2", C.c_double), ("K", PoseParams)]


class ResectRefine(C.Structure):
    _fields_ = [("n_before", C.c_uint32), ("n_after", C.c_uint32), ("accepted", C.c_uint32), ("stop", C.c_int32), ("cost_before", C.c_double),
                ("cost_after", C.c_double)]


class ResectRefineOut(C.Structure):
    """vslam_resect_refine_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("models", C.c_void_p), ("models_bytes", C.c_size_t), ("info", C.c_void_p), ("info_bytes", C.c_size_t),
                ("inlier_bits", C.c_void_p), ("inlier_bits_bytes", C.c_size_t)]


class TracksParams(C.Structure):
    _fields_ = [("K", PoseParams), ("max_dist2", C.c_double), ("min_views", C.c_uint32), ("reserved", C.c_uint32)]


class TracksOut(C.Structure):
    """vslam_tracks_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("tracks", C.c_void_p), ("tracks_bytes", C.c_size_t), ("refs", C.c_void_p), ("refs_bytes", C.c_size_t),
                ("good_bits", C.c_void_p), ("good_bits_bytes", C.c_size_t), ("summary", C.c_void_p), ("summary_bytes", C.c_size_t)]


class BundleParams(C.Structure):
    _fields_ = [("K", PoseParams), ("max_dist2", C.c_double), ("min_views", C.c_uint32), ("sweeps", C.c_uint32)]


class BundleCam(C.Structure):
    _fields_ = [("W", C.c_double * 9), ("w", C.c_double * 3), ("C", C.c_double * 3), ("n_before", C.c_uint32), ("n_after", C.c_uint32),
                ("accepted", C.c_uint32), ("rejected", C.c_uint32), ("invalid", C.c_uint32), ("skipped", C.c_uint32), ("cost_before", C.c_double),
                ("cost_after", C.c_double)]


class BundlePoint(C.Structure):
    _fields_ = [("n_before", C.c_uint32), ("n_after", C.c_uint32), ("accepted", C.c_uint32), ("rejected", C.c_uint32), ("invalid", C.c_uint32),
                ("skipped", C.c_uint32), ("cost_before", C.c_double), ("cost_after", C.c_double)]


class BundleOut(C.Structure):
    """vslam_bundle_out: struct_size, then every pointer with the bytes behind it."""
    _fields_ = [("struct_size", C.c_size_t), ("tracks", C.c_void_p), ("tracks_bytes", C.c_size_t), ("cams", C.c_void_p), ("cams_bytes", C.c_size_t),
                ("point_info", C.c_void_p), ("point_info_bytes", C.c_size_t), ("member_bits", C.c_void_p), ("member_bits_bytes", C.c_size_t)]


class PyramidInfo(C.Structure):
    _fields_ = [
        ("n_octaves", C.c_int), ("n_levels", C.c_int), ("n_dogs", C.c_int), ("sigma0", C.c_double),
        ("rows", C.c_int * MAX_OCTAVES), ("cols", C.c_int * MAX_OCTAVES),
        ("sigma", (C.c_double * NUM_LEVELS) * MAX_OCTAVES), ("ksize", (C.c_int * NUM_LEVELS) * MAX_OCTAVES),
    ]


# name -> (restype, argtypes); mirrors include/vslam.h one to one
_P, _I, _Z, _D, _F = C.c_void_p, C.c_int, C.c_size_t, C.c_double, C.c_float
SIGNATURES = {
    "vslam_version": (_I, []),
    "vslam_status_string": (C.c_char_p, [_I]),
    "vslam_ctx_create": (_I, [_I, _P, C.POINTER(_P)]),
    "vslam_ctx_destroy": (_I, [_P]),
    "vslam_ctx_sync": (_I, [_P]),
    "vslam_last_error": (C.c_char_p, [_P]),
    "vslam_gauss_ksize_u8": (_I, [_D]),
    "vslam_gauss_taps_q8": (_I, [_I, _D, _P]),
    "vslam_sigma_at": (_D, [_D, _I, _I]),
    "vslam_auto_num_octaves": (_I, [_I, _I]),
    "vslam_half_size": (None, [_I, _I, C.POINTER(_I), C.POINTER(_I)]),
    "vslam_extrema_lattice": (None, [_I, _I, _I, C.POINTER(_I), C.POINTER(_I)]),
    "vslam_gaussian_blur_u8": (_I, [_P, _P, _I, _I, _Z, _I, _D, _P, _Z]),
    "vslam_sobel_k1_u8_f32": (_I, [_P, _P, _I, _I, _Z, _I, _I, _P, _Z]),
    "vslam_resize_linear2x_u8": (_I, [_P, _P, _I, _I, _Z, _P, _Z]),
    "vslam_resize_nearest_half_u8": (_I, [_P, _P, _I, _I, _Z, _P, _Z]),
    "vslam_convert_scale_abs_f32": (_I, [_P, _P, _I, _I, _Z, _P, _Z]),
    "vslam_harris_from_grad_f32": (_I, [_P, _P, _P, _I, _I, _Z, _F, _I, _P, _Z]),
    "vslam_harris_response_u8": (_I, [_P, _P, _I, _I, _Z, _F, _I, _P, _Z]),
    "vslam_nms_strict_u8": (_I, [_P, _P, _I, _I, _Z, _I, _P, _Z]),
    "vslam_nms_strict_f32": (_I, [_P, _P, _I, _I, _Z, _I, _P, _Z]),
    "vslam_nms2_f32": (_I, [_P, _P, _I, _I, _Z, _I, _P, _Z, C.POINTER(_F)]),
    "vslam_harris_keypoints_u8": (_I, [_P, _P, _I, _I, _Z, _F, _P, _Z, C.POINTER(_Z)]),
    "vslam_pyramid_build_u8": (_I, [_P, _P, _I, _I, _Z, _I, _D, C.POINTER(_P)]),
    "vslam_pyramid_destroy": (_I, [_P]),
    "vslam_pyramid_get_info": (_I, [_P, C.POINTER(PyramidInfo)]),
    "vslam_pyramid_get_base": (_I, [_P, _I, _P, _Z]),
    "vslam_pyramid_get_gauss": (_I, [_P, _I, _I, _P, _Z]),
    "vslam_pyramid_get_dog": (_I, [_P, _I, _I, _P, _Z]),
    "vslam_pyramid_get_gradients": (_I, [_P, _I, _I, _P, _P, _P, _P, _Z]),
    "vslam_dog_extrema": (_I, [_P, _P, _I, _I, _I, _P, _P, _Z, C.POINTER(_Z)]),
    "vslam_dog_extrema_dense": (_I, [_P, _P, _I, _I, _P, _P, _Z, C.POINTER(_Z)]),
    "vslam_dog_keypoints": (_I, [_P, _P, _I, _I, _P, _Z, C.POINTER(_Z)]),
    "vslam_localize_points": (_I, [_P, _P, _Z, _P, _P]),
    "vslam_filter_keypoints": (_I, [_P, _P, _I, _P, _Z, _P, _Z, C.POINTER(_Z)]),
    "vslam_cos_sin_deg": (None, [_F, C.POINTER(_F), C.POINTER(_F)]),
    "vslam_rotated_window_points": (_I, [_I, _I, _I, _F, _P]),
    "vslam_sift_descriptors": (_I, [_P, _P, _I, _P, _Z, _P, _P]),
    "vslam_descriptor_file_write": (_I, [C.c_char_p, _P, _Z]),
    "vslam_edge_response_windows": (_I, [_P, _P, _P, _I, _Z, _P]),
    "vslam_structure_matrix_windows": (_I, [_P, _P, _P, _I, _Z, _P]),
    "vslam_params_default": (None, [C.POINTER(Params), _I, _I]),
    "vslam_batch_layout_query": (_I, [C.POINTER(Params), C.POINTER(BatchLayout)]),
    "vslam_batch_out_required": (_I, [C.POINTER(Params), _I, C.POINTER(BatchOut)]),
    "vslam_detect_batch_dev": (_I, [_P, C.POINTER(Params), _P, _Z, _I, C.POINTER(BatchOut)]),
    "vslam_ctx_follow": (_I, [_P, _P]),
    "vslam_ctx_set_matrix_path": (_I, [_P, _I]),
    "vslam_ctx_get_matrix_path": (_I, [_P]),
    "vslam_ctx_side_stream_report": (_I, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vslam_ctx_tune_side_streams": (_I, [_P, _I]),
    "vslam_ctx_join_watch_report": (_I, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "vslam_ctx_set_side_stream_priority": (_I, [_P, _I]),
    "vslam_ctx_set_f32_fused": (_I, [_P, _I]),
    "vslam_ctx_get_f32_fused": (_I, [_P]),
    "vslam_ctx_set_join_watch": (_I, [_P, _I]),
    "vslam_ctx_pin_side_streams": (_I, [_P, _I]),
    "vslam_detect_batch_host": (_I, [_P, C.POINTER(Params), _P, _Z, _I, C.POINTER(HostLists)]),
    "vslam_pack_lists_dev": (_I, [_P, _P, _Z, C.c_uint32, _P, _I, _P, _Z, _P]),
    "vslam_pack_points16_dev": (_I, [_P, _P, C.c_uint32, _P, _I, _P, _Z, _P]),
    "vslam_points16_expand": (None, [_P, _Z, _P]),
    "vslam_count_totals_dev": (_I, [_P, _P, _P, _I, _P]),
    "vslam_match_dev": (_I, [_P, C.POINTER(DescSets), C.POINTER(DescSets), _I, _F, _I, C.POINTER(MatchOut)]),
    "vslam_match_host": (_I, [_P, _P, _P, _P, _Z, _P, _P, _P, _Z, _F, _I, _P, _P, _Z, C.POINTER(_Z)]),
    "vslam_match_mutual_dev": (_I, [_P, C.POINTER(DescSets), C.POINTER(DescSets), _I, _F, _I, C.POINTER(MatchMutualOut)]),
    "vslam_match_mutual_host": (_I, [_P, _P, _P, _P, _Z, _P, _P, _P, _Z, _F, _I, _P, _P, _P, _Z, C.POINTER(_Z)]),
    "vslam_match_guided_dev": (_I, [_P, C.POINTER(DescSets), C.POINTER(DescSets), _P, _I, C.POINTER(GuidedParams), C.POINTER(MatchOut)]),
    "vslam_match_guided_host": (_I, [_P, _P, _P, _P, _Z, _P, _P, _P, _Z, _P, C.POINTER(GuidedParams), _P, _P, _Z, C.POINTER(_Z)]),
    "vslam_match_guided_hf_dev": (_I, [_P, C.POINTER(DescSets), C.POINTER(DescSets), _P, _P, _I, C.POINTER(GuidedHfParams), C.POINTER(MatchOut)]),
    "vslam_match_guided_hf_host": (_I, [_P, _P, _P, _P, _Z, _P, _P, _P, _Z, _P, _P, C.POINTER(GuidedHfParams), _P, _P, _Z, C.POINTER(_Z)]),
    "vslam_epipolar_dev": (_I, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _I, C.POINTER(EpipolarParams), C.POINTER(EpipolarOut)]),
    "vslam_epipolar_host": (_I, [_P, _P, _Z, _P, _Z, _P, _Z, C.POINTER(EpipolarParams), _P, _P, _P, _Z, C.POINTER(_Z), _P]),
    "vslam_refit_dev": (_I, [_P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _I, C.POINTER(RefitParams), C.POINTER(RefitOut)]),
    "vslam_refit_host": (_I, [_P, _P, _P, _Z, _P, _Z, _P, _Z, C.POINTER(RefitParams), _P, _P, _P, _P, _Z, C.POINTER(_Z)]),
    "vslam_homography_dev": (_I, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _I, _P, C.POINTER(HomographyParams), C.POINTER(HomographyOut)]),
    "vslam_homography_host": (_I, [_P, _P, _Z, _P, _Z, _P, _Z, _P, C.POINTER(HomographyParams), _P, _P, _P, _Z, C.POINTER(_Z), _P, _P]),
    "vslam_hrefit_dev": (_I, [_P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _I, _P, C.POINTER(HRefitParams), C.POINTER(HRefitOut)]),
    "vslam_hrefit_host": (_I, [_P, _P, _P, _Z, _P, _Z, _P, _Z, _P, C.POINTER(HRefitParams), _P, _P, _P, _P, _Z, C.POINTER(_Z), _P]),
    "vslam_pose_dev": (_I, [_P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _I, C.POINTER(PoseParams), C.POINTER(PoseOut)]),
    "vslam_pose_host": (_I, [_P, _P, _P, _Z, _P, _Z, _P, _Z, C.POINTER(PoseParams), _P, _P, _P, _P]),
    "vslam_hpose_dev": (_I, [_P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _I, _P, C.POINTER(HposeParams), C.POINTER(HposeOut)]),
    "vslam_hpose_host": (_I, [_P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _I, _P, C.POINTER(HposeParams), C.POINTER(HposeOut)]),
    "vslam_chain_dev": (_I, [_P, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _I, C.POINTER(ChainParams), C.POINTER(ChainOut)]),
    "vslam_chain_host": (_I, [_P, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _I, C.POINTER(ChainParams), C.POINTER(ChainOut)]),
    "vslam_resect_dev": (_I, [_P, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_uint32, _I, C.POINTER(ResectParams),
                              C.POINTER(ResectOut)]),
    "vslam_resect_host": (_I, [_P, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_uint32, _I, C.POINTER(ResectParams),
                               C.POINTER(ResectOut)]),
    "vslam_resect_refine_dev": (_I, [_P, _P, _P, C.c_uint32, _I, C.POINTER(ResectRefineParams), C.POINTER(ResectRefineOut)]),
    "vslam_resect_refine_host": (_I, [_P, _P, _P, C.c_uint32, _I, C.POINTER(ResectRefineParams), C.POINTER(ResectRefineOut)]),
    "vslam_tracks_dev": (_I, [_P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _I, _P, _P, C.POINTER(TracksParams), C.POINTER(TracksOut)]),
    "vslam_tracks_host": (_I, [_P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _I, _P, _P, C.POINTER(TracksParams), C.POINTER(TracksOut)]),
    "vslam_bundle_dev": (_I, [_P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _I, _P, _P, _P, _P, _P, C.POINTER(BundleParams), C.POINTER(BundleOut)]),
    "vslam_bundle_host": (_I, [_P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _I, _P, _P, _P, _P, _P, C.POINTER(BundleParams), C.POINTER(BundleOut)]),
    "vslam_vocab_sample_dev": (_I, [_P, C.POINTER(DescSets), _I, C.c_uint32, _P, _Z, _P, _Z]),
    "vslam_words_dev": (_I, [_P, C.POINTER(DescSets), _I, _P, _P, C.c_uint32, C.POINTER(WordsOut)]),
    "vslam_words_host": (_I, [_P, _P, _P, _P, C.c_uint32, _I, _P, _P, C.c_uint32, C.POINTER(WordsOut)]),
    "vslam_place_dev": (_I, [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PlaceParams), C.POINTER(PlaceOut)]),
    "vslam_vocab_kmeans_dev": (_I, [_P, C.POINTER(DescSets), _I, _P, _P, C.c_uint32, C.POINTER(KmeansParams), C.POINTER(KmeansOut)]),
    "vslam_vocab_kmeans_host": (_I, [_P, _P, _P, _P, C.c_uint32, _I, _P, _P, C.c_uint32, C.POINTER(KmeansParams), C.POINTER(KmeansOut)]),
    "vslam_place_host": (_I, [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PlaceParams), C.POINTER(PlaceOut)]),
    "vslam_loop_pairs_dev": (_I, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _Z]),
    "vslam_match_pairs_dev": (_I, [_P, C.POINTER(DescSets), _I, C.POINTER(DescSets), _I, _P, _I, _F, _I, C.POINTER(MatchOut)]),
    "vslam_match_pairs_host": (_I, [_P, C.POINTER(DescSets), _I, C.POINTER(DescSets), _I, _P, _I, _F, _I, C.POINTER(MatchOut)]),
    "vslam_pair_points_dev": (_I, [_P, _P, _P, C.c_uint32, _P, _I, _P, C.c_uint32, _I, _P, C.c_uint32, _I, _P, _Z, _P, _Z, _P, _Z]),
    "vslam_loop_verdict_dev": (_I, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(LoopParams), C.POINTER(LoopOut)]),
    "vslam_loop_verdict_host": (_I, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(LoopParams), C.POINTER(LoopOut)]),
    "vslam_frame_world_dev": (_I, [_P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, _I, C.POINTER(FrameWorldOut)]),
    "vslam_frame_world_host": (_I, [_P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, _I, C.POINTER(FrameWorldOut)]),
    "vslam_sim3_dev": (_I, [_P, C.POINTER(Sim3Side), C.POINTER(Sim3Side), _P, _P, _P, C.c_uint32, _P, _I, C.POINTER(Sim3Params), C.POINTER(Sim3Out)]),
    "vslam_sim3_host": (_I, [_P, C.POINTER(Sim3Side), C.POINTER(Sim3Side), _P, _P, _P, C.c_uint32, _P, _I, C.POINTER(Sim3Params), C.POINTER(Sim3Out)]),
    "vslam_kernel_timing_enable": (_I, [_P, C.c_char_p]),
    "vslam_kernel_timing_read": (_I, [_P, C.POINTER(_I), C.POINTER(_D)]),
    "vslam_kernel_names": (C.c_char_p, []),
}


def build(force: bool = False) -> str:
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU): lib/libvslam.so, and beside it
    lib/libvslam_diag.so (DIAG_LIB_PATH: the same sources with -DVSLAM_DIAGNOSTICS, for the tests / tools that need a reference-path
    switch - never loaded by default)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(_HERE, "..", "include", "vslam.h")]
    newest = max(os.path.getmtime(s) for s in srcs)
    stale = force or any(not os.path.exists(q) or os.path.getmtime(q) < newest for q in (LIB_PATH, DIAG_LIB_PATH))
    if stale and not os.environ.get("VSLAM_LIBRARY"):
        r = subprocess.run(["make", "-j4", "-C", CSRC] + (["-B"] if force else []), capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("building libvslam.so failed:\n" + r.stdout + r.stderr)
    return LIB_PATH


_lib = None


def lib():
    """Load libvslam.so (raises if it has not been built: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing -- run __graft_entry__.build() (the product has no CPU fallback)")
        # One HIP runtime per process: torch bundles its own libamdhip64.so.7 / libhsa-runtime64
        # (same sonames as /opt/rocm).  If libvslam.so pulled in /opt/rocm's copy first, torch
        # would later mix it with its bundled HSA runtime and HIP fails to initialise.  So in a
        # Python process that has torch, let torch load its runtime first; libvslam.so then binds
        # to that same copy.  (C++ callers without torch simply use /opt/rocm's runtime.)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _status_string(s: int) -> str:
    try:
        return lib().vslam_status_string(s).decode()
    except Exception:
        return "?"


def gauss_ksize_u8(sigma: float) -> int:
    return lib().vslam_gauss_ksize_u8(float(sigma))


def gauss_taps_q8(n: int, sigma: float) -> np.ndarray:
    t = np.zeros(max(n, 1), np.uint16)
    rc = lib().vslam_gauss_taps_q8(n, float(sigma), t.ctypes.data)
    if rc:
        raise VslamError(rc, "vslam_gauss_taps_q8")
    return t


def sigma_at(sigma0: float, octave: int, level: int) -> float:
    return lib().vslam_sigma_at(float(sigma0), octave, level)


def auto_num_octaves(rows: int, cols: int) -> int:
    return lib().vslam_auto_num_octaves(rows, cols)


def half_size(rows: int, cols: int):
    r, c = C.c_int(), C.c_int()
    lib().vslam_half_size(rows, cols, C.byref(r), C.byref(c))
    return r.value, c.value


def extrema_lattice(rows: int, cols: int, window: int = 3):
    r, c = C.c_int(), C.c_int()
    lib().vslam_extrema_lattice(rows, cols, window, C.byref(r), C.byref(c))
    return r.value, c.value


def cos_sin_deg(theta_deg: float):
    c, s = C.c_float(), C.c_float()
    lib().vslam_cos_sin_deg(float(theta_deg), C.byref(c), C.byref(s))
    return np.float32(c.value), np.float32(s.value)


def rotated_window_points(cx: int, cy: int, window: int, theta_deg: float) -> np.ndarray:
    """Rotation::getRotatedWindowPoints: int32 [(window+1)^2, 2] = (x, y), rows outer."""
    xy = np.zeros(((max(window, 0) + 1) ** 2, 2), np.int32)
    rc = lib().vslam_rotated_window_points(int(cx), int(cy), int(window), float(theta_deg), xy.ctypes.data)
    if rc:
        raise VslamError(rc, "vslam_rotated_window_points")
    return xy


def descriptor_file_write(path: str, desc) -> None:
    """featureDescriptors.dat (Diff_of_Gauss.cpp:837-863): int32 {n, 128, 24} + n x 128 float32."""
    d = np.ascontiguousarray(desc, dtype=np.float32).reshape(-1, 128)
    rc = lib().vslam_descriptor_file_write(os.fsencode(path), d.ctypes.data, d.shape[0])
    if rc:
        raise VslamError(rc, "vslam_descriptor_file_write", path)


def points16_expand(packed) -> np.ndarray:
    """vslam_points16_expand (host): [m, 4] int32 / uint32 packed records -> [m] POINT_DTYPE records."""
    a = np.ascontiguousarray(packed).view(np.uint32).reshape(-1, 4)
    out = np.zeros(len(a), POINT_DTYPE)
    lib().vslam_points16_expand(a.ctypes.data, len(a), out.ctypes.data)
    return out


def default_params(rows: int, cols: int, **kw) -> Params:
    p = Params()
    lib().vslam_params_default(C.byref(p), rows, cols)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def batch_layout(p: Params) -> BatchLayout:
    L = BatchLayout()
    rc = lib().vslam_batch_layout_query(C.byref(p), C.byref(L))
    if rc:
        raise VslamError(rc, "vslam_batch_layout_query")
    return L


def batch_out_required(p: Params, n_frames: int) -> BatchOut:
    """Bytes every output buffer needs for n_frames frames (the x_bytes fields; pointers stay NULL)."""
    z = BatchOut()
    rc = lib().vslam_batch_out_required(C.byref(p), int(n_frames), C.byref(z))
    if rc:
        raise VslamError(rc, "vslam_batch_out_required")
    return z


def desc_sets(desc, counts, defined=None, points=None) -> DescSets:
    """vslam_desc_sets over CUDA tensors: desc f32 [n, cap, 128], counts int32 [n], defined uint8 [n, cap], points int32 [n, cap, 6] -
    the descriptors / oriented_counts / descriptor_defined / oriented_points tensors of detect_batch, or slices of them along the
    first dimension (desc[1:], counts[1:] ... are the train sets of consecutive-frame matching).  The tensors must outlive the call."""
    import torch

    if desc.dim() != 3 or desc.shape[2] != 128 or desc.dtype != torch.float32 or not desc.is_contiguous() or not desc.is_cuda:
        raise ValueError("desc_sets: desc must be a contiguous float32 CUDA tensor [n, cap, 128]")
    n, cap = desc.shape[0], desc.shape[1]
    if counts.numel() < n or counts.dtype != torch.int32 or not counts.is_contiguous():
        raise ValueError("desc_sets: counts must be int32 [n]")
    if defined is not None and not (defined.dtype == torch.uint8 and defined.is_contiguous() and tuple(defined.shape) == (n, cap)):
        raise ValueError("desc_sets: defined must be uint8 [n, cap]")
    if points is not None and not (points.dtype == torch.int32 and points.is_contiguous() and tuple(points.shape) == (n, cap, 6)):
        raise ValueError("desc_sets: points must be int32 [n, cap, 6]")
    s = DescSets(desc.data_ptr(), defined.data_ptr() if defined is not None else None, points.data_ptr() if points is not None else None,
                 counts.data_ptr(), cap)
    s.n = n
    return s


def sim3_side(cams, index, map, points, n_frames: int | None = None) -> Sim3Side:
    """A vslam_sim3_side over CUDA tensors (kept alive on the returned struct): cams - any contiguous tensor of n_frames * 112 bytes
    as frame_world() wrote it -, index int32 [n_frames, point_cap], map float64 [n_map_pairs, map_cap, 3] as chain() wrote it,
    points int32 [n_frames, points_cap, 6], the frames' point lists."""
    ok = all(t.is_contiguous() for t in (cams, index, map, points))
    ok = ok and index.dim() == 2 and index.element_size() == 4 and map.dim() == 3 and map.shape[2] * map.element_size() == 24
    ok = ok and points.dim() == 3 and points.shape[2] * points.element_size() == 24
    if not ok:
        raise ValueError("sim3_side: contiguous cams, index [n_frames, point_cap] int32, map [n_map_pairs, map_cap, 3] float64 and points "
                         "[n_frames, points_cap, 6] int32")
    nf = index.shape[0] if n_frames is None else int(n_frames)
    if cams.numel() * cams.element_size() < nf * 112 or index.shape[0] < nf or points.shape[0] < nf:
        raise ValueError("sim3_side: fewer rows than frames")
    s = Sim3Side(cams.data_ptr(), index.data_ptr(), map.data_ptr(), points.data_ptr(), map.shape[1], index.shape[1], points.shape[1], map.shape[0], nf, 0)
    s.keep = (cams, index, map, points)
    return s


def _host_sim3_side(stage, side, keep):
    """A vslam_sim3_side over the numpy arrays of a side dict (cams, index, map, points); the converted arrays are appended to keep."""
    cams, points = _records(side["cams"], FRAME_CAM_DTYPE), np.ascontiguousarray(side["points"], dtype=POINT_DTYPE)
    index, mp = np.ascontiguousarray(side["index"], dtype=np.int32), np.ascontiguousarray(side["map"], dtype=np.float64)
    nf = len(cams)
    if index.ndim != 2 or points.ndim != 2 or mp.ndim != 3 or mp.shape[2] != 3 or index.shape[0] != nf or points.shape[0] != nf:
        raise ValueError(f"{stage}: a side is cams [nf], index [nf, point_cap], map [n_map_pairs, map_cap, 3] and points [nf, points_cap]")
    keep += [cams, index, mp, points]
    return Sim3Side(cams.ctypes.data, index.ctypes.data, mp.ctypes.data, points.ctypes.data, mp.shape[1], index.shape[1], points.shape[1], mp.shape[0],
                    nf, 0)


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("expected a 2-D uint8 image")
    return a


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError("expected a 2-D float32 image")
    return a


def _nbytes(t):
    return t.numel() * t.element_size()


def _fill_out(out, buffers):
    """A vslam_*_out struct from its output tensors (device entry points) or numpy arrays (host entry points) by field name:
    struct_size, pointers, byte sizes."""
    out.struct_size = C.sizeof(out)
    for name, t in buffers.items():
        if t is not None:
            at, nbytes = (t.ctypes.data, t.nbytes) if isinstance(t, np.ndarray) else (t.data_ptr(), t.numel() * t.element_size())
            setattr(out, name, at)
            setattr(out, name + "_bytes", nbytes)
    return out


def _host_lists(matches, query_points, train_points):
    """The three lists of one host pair as flat record arrays."""
    return tuple(np.ascontiguousarray(a, dtype=dt).reshape(-1) for a, dt in ((matches, MATCH_DTYPE), (query_points, POINT_DTYPE), (train_points, POINT_DTYPE)))


# What the device entry points check before the library is called (each raises the ValueError of the first check that fails, with
# the stage in front), and what the batched host entry points do with their arrays.  None of it needs a context or the library.

def _check_tensors(stage, where, tensors, required):
    """Every tensor given (by argument name, in the order they are reported) is contiguous on the device `where` (a torch.device:
    Context.where); then every name in `required` is there."""
    for name, t in tensors.items():
        if t is not None and not (t.device == where and t.is_contiguous()):
            raise ValueError(f"{stage}: {name} must be a contiguous tensor on {where}")
    for name in required:
        if tensors[name] is None:
            raise ValueError(f"{stage}: {name} is required")


def _check_records(stage, name, t, width, shape):
    """t is [n, cap, k] with k elements of `width` bytes together; shape: how the message words it."""
    if t.dim() != 3 or t.shape[2] * t.element_size() != width:
        raise ValueError(f"{stage}: {name} must be {shape} 4-byte elements")


def _check_sets(stage, n, lists, counts, sizes):
    """n pairs are there: n rows in every tensor of `lists`, n 4-byte elements in every tensor of `counts`, and the bytes needed
    in every (tensor, bytes needed) pair of `sizes` (a tensor that is None needs none)."""
    ok = True
    for t in lists:
        ok = ok and t.shape[0] >= n
    for t in counts:
        ok = ok and t.element_size() == 4 and t.numel() >= n
    for t, need in sizes:
        ok = ok and (t is None or t.numel() * t.element_size() >= need)
    if not ok:
        raise ValueError(f"{stage}: fewer sets than pairs")


def _host_structure(stage, poses, matches):
    """poses [n] and matches [n, match_cap] of a batched host call as record arrays -> (poses, matches, n, match_cap)."""
    ps = np.ascontiguousarray(poses, dtype=POSE_DTYPE).reshape(-1)
    mt = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
    if mt.ndim != 2 or mt.shape[0] != len(ps):
        raise ValueError(f"{stage}: matches must be [n, match_cap]")
    return ps, mt, len(ps), mt.shape[1]


def _records(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _counts(a):
    return np.ascontiguousarray(a).astype(np.uint32).reshape(-1)


def _words(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_host_outs(stage, outs):
    """The optional outputs of a host call, rows of (name, array or None, dtype, elements): written in place, so each is exactly that."""
    for name, a, dt, size in outs:
        if a is not None and not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous and a.size == size):
            raise ValueError(f"{stage}: {name} must be a C-contiguous {np.dtype(dt).name} array of {size} elements")


def _ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data


STREAM_LEGACY = 1  # VSLAM_STREAM_LEGACY == hipStreamLegacy: the device's NULL stream


class Context:
    """One vslam_ctx: one GPU, one HIP stream.

    stream: None -> the context owns a private non-blocking stream (results are complete after
    ``sync()``; nothing orders it against torch's streams).  An integer is a hipStream_t handle, e.g.
    ``torch.cuda.current_stream().cuda_stream``; torch's default stream has handle 0, which is passed
    on as the legacy NULL stream (VSLAM_STREAM_LEGACY) -- NOT as "no stream" -- so that tensors made
    and read on that stream are ordered with the kernels by the stream itself."""

    def __init__(self, device: int = 0, stream: int | None = None):
        h = C.c_void_p()
        if stream is None:
            sp = None
        else:
            sp = C.c_void_p(int(stream) or STREAM_LEGACY)
        rc = lib().vslam_ctx_create(device, sp, C.byref(h))
        if rc:
            raise VslamError(rc, "vslam_ctx_create", "no usable HIP device" if rc == -2 else "")
        self._h = h
        self.device = device
        try:  # where the device entry points want their tensors (without torch there are none to check)
            import torch
            self.where = torch.device("cuda", device)
        except ImportError:
            self.where = None
        self._pyramids = weakref.WeakSet()  # the live Pyramid objects built on this context

    def close(self):
        if getattr(self, "_h", None):
            # a vslam_pyramid hands its device blocks back to its context when it is destroyed: one that outlived the context
            # (a caller's exception skipped its close(), the collector gets to it later) would write into freed host memory
            for py in list(self._pyramids):
                py.close()
            lib().vslam_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc, what):
        if rc:
            raise VslamError(rc, what, lib().vslam_last_error(self._h).decode())

    def sync(self):
        self._chk(lib().vslam_ctx_sync(self._h), "vslam_ctx_sync")

    # ---- host-buffer primitives
    def gaussian_blur_u8(self, img, ksize: int, sigma: float):
        img = _u8(img)
        out = np.empty_like(img)
        self._chk(lib().vslam_gaussian_blur_u8(self._h, img.ctypes.data, *img.shape, img.strides[0], ksize, float(sigma), out.ctypes.data, out.strides[0]), "vslam_gaussian_blur_u8")
        return out

    def sobel_k1(self, img, dx: int, dy: int):
        img = _u8(img)
        out = np.empty(img.shape, np.float32)
        self._chk(lib().vslam_sobel_k1_u8_f32(self._h, img.ctypes.data, *img.shape, img.strides[0], dx, dy, out.ctypes.data, out.strides[0]), "vslam_sobel_k1_u8_f32")
        return out

    def resize_linear2x(self, img):
        img = _u8(img)
        out = np.empty((2 * img.shape[0], 2 * img.shape[1]), np.uint8)
        self._chk(lib().vslam_resize_linear2x_u8(self._h, img.ctypes.data, *img.shape, img.strides[0], out.ctypes.data, out.strides[0]), "vslam_resize_linear2x_u8")
        return out

    def resize_nearest_half(self, img):
        img = _u8(img)
        out = np.empty(half_size(*img.shape), np.uint8)
        self._chk(lib().vslam_resize_nearest_half_u8(self._h, img.ctypes.data, *img.shape, img.strides[0], out.ctypes.data, max(out.strides[0], 1)), "vslam_resize_nearest_half_u8")
        return out

    def convert_scale_abs(self, x):
        x = _f32(x)
        out = np.empty(x.shape, np.uint8)
        self._chk(lib().vslam_convert_scale_abs_f32(self._h, x.ctypes.data, *x.shape, x.strides[0], out.ctypes.data, out.strides[0]), "vslam_convert_scale_abs_f32")
        return out

    # ---- Harris
    def harris_from_grad(self, ix, iy, k: float = 0.04, window: int = 3):
        ix, iy = _f32(ix), _f32(iy)
        if ix.shape != iy.shape:
            raise ValueError("Ix and Iy differ in shape")
        out = np.empty(ix.shape, np.float32)
        self._chk(lib().vslam_harris_from_grad_f32(self._h, ix.ctypes.data, iy.ctypes.data, *ix.shape, ix.strides[0], k, window, out.ctypes.data, out.strides[0]), "vslam_harris_from_grad_f32")
        return out

    def harris_response(self, img, k: float = 0.04, window: int = 3):
        img = _u8(img)
        out = np.empty(img.shape, np.float32)
        self._chk(lib().vslam_harris_response_u8(self._h, img.ctypes.data, *img.shape, img.strides[0], k, window, out.ctypes.data, out.strides[0]), "vslam_harris_response_u8")
        return out

    def nms_strict(self, x, window: int = 3):
        x = np.asarray(x)
        out = np.empty(x.shape, np.uint8)
        if x.dtype == np.uint8:
            x = _u8(x)
            rc = lib().vslam_nms_strict_u8(self._h, x.ctypes.data, *x.shape, x.strides[0], window, out.ctypes.data, out.strides[0])
        else:
            x = _f32(x)
            rc = lib().vslam_nms_strict_f32(self._h, x.ctypes.data, *x.shape, x.strides[0], window, out.ctypes.data, out.strides[0])
        self._chk(rc, "vslam_nms_strict")
        return out

    def nms2(self, resp, window: int = 5):
        resp = _f32(resp)
        out = np.empty(resp.shape, np.float32)
        tm = C.c_float()
        self._chk(lib().vslam_nms2_f32(self._h, resp.ctypes.data, *resp.shape, resp.strides[0], window, out.ctypes.data, out.strides[0], C.byref(tm)), "vslam_nms2_f32")
        return out, tm.value

    def harris_keypoints(self, img, k: float = 0.04, cap: int = 1 << 20):
        img = _u8(img)
        out = np.zeros(cap, KP_DTYPE)
        n = C.c_size_t()
        self._chk(lib().vslam_harris_keypoints_u8(self._h, img.ctypes.data, *img.shape, img.strides[0], k, out.ctypes.data, cap, C.byref(n)), "vslam_harris_keypoints_u8")
        return out[: min(n.value, cap)], n.value

    # ---- DoG
    def localize_points(self, diffs):
        """FeaturePointLocalization for n candidates: diffs int32 [n, 4] = (d_x, d_y, d_scale, value)
        -> (keep bool [n], value int32 [n])."""
        d = np.ascontiguousarray(diffs, dtype=np.int32).reshape(-1, 4)
        n = d.shape[0]
        keep = np.zeros(n, np.int32)
        val = np.zeros(n, np.int32)
        self._chk(lib().vslam_localize_points(self._h, d.ctypes.data, n, keep.ctypes.data, val.ctypes.data), "vslam_localize_points")
        return keep.astype(bool), val

    def edge_response_windows(self, gx_windows, gy_windows):
        """computeEdgeResponse for n gathered windows: f32 [n, elems] each -> f32 [n]."""
        gx = np.ascontiguousarray(gx_windows, dtype=np.float32)
        gy = np.ascontiguousarray(gy_windows, dtype=np.float32)
        assert gx.shape == gy.shape and gx.ndim == 2
        out = np.zeros(gx.shape[0], np.float32)
        self._chk(lib().vslam_edge_response_windows(self._h, gx.ctypes.data, gy.ctypes.data, gx.shape[1], gx.shape[0], out.ctypes.data), "vslam_edge_response_windows")
        return out

    def structure_matrix_windows(self, gx_windows, gy_windows):
        """StructureMatrix for n gathered windows: f32 [n, elems] each -> f32 [n, 3] = (Ix2, IxIy, Iy2)."""
        gx = np.ascontiguousarray(gx_windows, dtype=np.float32)
        gy = np.ascontiguousarray(gy_windows, dtype=np.float32)
        assert gx.shape == gy.shape and gx.ndim == 2
        out = np.zeros((gx.shape[0], 3), np.float32)
        self._chk(lib().vslam_structure_matrix_windows(self._h, gx.ctypes.data, gy.ctypes.data, gx.shape[1], gx.shape[0], out.ctypes.data), "vslam_structure_matrix_windows")
        return out

    def pyramid(self, img, n_octaves: int = 4, sigma0: float = 1.6):
        return Pyramid(self, img, n_octaves, sigma0)

    # ---- device-resident batch (torch CUDA tensors)
    def detect_batch(self, params: Params, frames, **outs):
        """frames: uint8 CUDA tensor [n, rows, cols]; outs: CUDA tensors by BatchOut field name."""
        n, bo, fstride = self._batch_args(params, frames, outs)
        self._chk(lib().vslam_detect_batch_dev(self._h, C.byref(params), frames.data_ptr(), fstride, n, C.byref(bo)), "vslam_detect_batch_dev")

    def _batch_args(self, params: Params, frames, outs):
        import torch

        n = frames.shape[0]
        L = batch_layout(params)  # raises on bad parameters before anything is checked against them
        N = params.rows * params.cols

        def need(name, t, dtype):
            # sizes are checked by the library itself (vslam_batch_out carries them); placement, dtype and
            # contiguity are properties of the tensor that only this wrapper can see
            if not (t.is_cuda and t.device.index == self.device):
                raise ValueError(f"detect_batch: {name} is not on cuda:{self.device}")
            if t.dtype not in dtype:
                raise ValueError(f"detect_batch: {name} has dtype {t.dtype}, expected one of {dtype}")
            if not t.is_contiguous():
                raise ValueError(f"detect_batch: {name} is not contiguous")

        if frames.dim() != 3 or tuple(frames.shape[1:]) != (params.rows, params.cols) or frames.stride(2) != 1 or frames.stride(1) != params.cols:
            raise ValueError("detect_batch: frames must be [n, rows, cols] uint8 with dense rows")
        if not (frames.is_cuda and frames.device.index == self.device and frames.dtype == torch.uint8):
            raise ValueError(f"detect_batch: frames must be uint8 on cuda:{self.device}")
        if n > 1 and frames.stride(0) < N:
            raise ValueError("detect_batch: frames overlap")
        i32, u8, f32, i64 = (torch.int32,), (torch.uint8,), (torch.float32,), (torch.int64, torch.uint64)
        spec = {
            "response": f32, "nms_mask": u8, "nms2": f32, "harris_kps": i32 + f32, "harris_counts": i32,
            "pyramid": u8, "extrema_bits": i64, "dog_points": i32, "dog_counts": i32,
            "oriented_points": i32, "oriented_counts": i32, "oriented_survivors": i32,
            "descriptors": f32, "descriptor_defined": u8,
        }
        bo = BatchOut()
        bo.struct_size = C.sizeof(BatchOut)
        for k, t in outs.items():
            if t is not None:
                if k not in spec:
                    raise ValueError(f"detect_batch: unknown output {k!r}")
                need(k, t, spec[k])
                setattr(bo, k, t.data_ptr())
                setattr(bo, k + "_bytes", t.numel() * t.element_size())
        return n, bo, (frames.stride(0) if n > 1 else N)  # a size-1 dimension may carry any stride

    def side_stream_report(self):
        """vslam_ctx_side_stream_report: (index of the side-stream pair the batched path runs on: 0 = the first created,
        state of the comparison: 0 not started, 1 measuring, 2 decided)."""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(lib().vslam_ctx_side_stream_report(self._h, C.byref(a), C.byref(b)), "vslam_ctx_side_stream_report")
        return a.value, b.value

    def set_side_stream_priority(self, low: bool):
        """vslam_ctx_set_side_stream_priority: low = True puts the two side streams at the device's lowest priority (yielding);
        the default is the context stream's priority.  Before the first batch call only."""
        self._chk(lib().vslam_ctx_set_side_stream_priority(self._h, int(bool(low))), "vslam_ctx_set_side_stream_priority")

    def join_watch_report(self):
        """vslam_ctx_join_watch_report: (level: 0 low-priority side streams / 1 flat priority / 2 no side streams, done,
        last measured fraction of a call the context's stream spent waiting for the side streams; -1: none yet)."""
        a, b, f = C.c_int(0), C.c_int(0), C.c_float(-1.0)
        self._chk(lib().vslam_ctx_join_watch_report(self._h, C.byref(a), C.byref(b), C.byref(f)), "vslam_ctx_join_watch_report")
        return a.value, bool(b.value), float(f.value)

    def set_matrix_path(self, on: bool):
        """vslam_ctx_set_matrix_path: OPT-IN matrix-core (MFMA) form of the LDS-tiled octave kernels; off by default."""
        self._chk(lib().vslam_ctx_set_matrix_path(self._h, 1 if on else 0), "vslam_ctx_set_matrix_path")

    def matrix_path(self) -> bool:
        return bool(lib().vslam_ctx_get_matrix_path(self._h))

    def set_f32_fused(self, on: bool):
        """vslam_ctx_set_f32_fused: the f32 stages with fused multiply-adds (an OpenCV that dispatches AVX2 + FMA3) instead of
        every product and sum rounded (its SSE2 baseline, the default); oracle.fma_variant is the checker's side of it."""
        self._chk(lib().vslam_ctx_set_f32_fused(self._h, 1 if on else 0), "vslam_ctx_set_f32_fused")

    def get_f32_fused(self) -> bool:
        return bool(lib().vslam_ctx_get_f32_fused(self._h))

    def set_join_watch(self, on: bool):
        """vslam_ctx_set_join_watch: False = this context takes no more join-lag measurements (stays at its level)."""
        self._chk(lib().vslam_ctx_set_join_watch(self._h, 1 if on else 0), "vslam_ctx_set_join_watch")

    def pin_side_streams(self, level: int):
        """vslam_ctx_pin_side_streams: 0 yielding / 1 the context stream's priority / 2 no side streams; before the first batch call."""
        self._chk(lib().vslam_ctx_pin_side_streams(self._h, int(level)), "vslam_ctx_pin_side_streams")

    def tune_side_streams(self, on: bool = True):
        """vslam_ctx_tune_side_streams: opt in to (or out of) the library's comparison of side-stream pairs; off by default."""
        self._chk(lib().vslam_ctx_tune_side_streams(self._h, 1 if on else 0), "vslam_ctx_tune_side_streams")

    def follow(self, leader: "Context"):
        """vslam_ctx_follow: this context's next work starts once `leader`'s latest batch is past its octave-0 kernels."""
        self._chk(lib().vslam_ctx_follow(self._h, leader._h), "vslam_ctx_follow")

    def detect_batch_host(self, params: Params, frames, harris_budget: int | None = None, dog_budget: int | None = None):
        """vslam_detect_batch_host: numpy uint8 frames [n, rows, cols] in, the packed lists out - no torch involved.
        Returns {"harris": (records, offsets, counts), "dog": (records, offsets, counts)}; a budget of 0 skips the list,
        None = room for every frame's full capacity."""
        fr = np.ascontiguousarray(frames, dtype=np.uint8)
        if fr.ndim != 3 or fr.shape[1:] != (params.rows, params.cols):
            raise ValueError("detect_batch_host: frames must be [n, rows, cols] uint8")
        n = fr.shape[0]
        hl = HostLists()
        hl.struct_size = C.sizeof(HostLists)
        res = {}
        keep = []
        for name, dtype, cap, budget in (("harris", KP_DTYPE, params.harris_cap, harris_budget), ("dog", POINT_DTYPE, params.dog_cap, dog_budget)):
            if budget == 0 or (name == "dog" and params.n_octaves == 0) or (name == "harris" and not params.do_harris):
                continue
            rec = np.zeros(n * cap if budget is None else budget, dtype)
            off = np.zeros(n + 1, np.uint64)
            cnt = np.zeros(n, np.uint32)
            setattr(hl, name, rec.ctypes.data)
            setattr(hl, name + "_bytes", rec.nbytes)
            setattr(hl, name + "_offsets", off.ctypes.data)
            setattr(hl, name + "_counts", cnt.ctypes.data)
            keep.append((name, rec, off, cnt))
        self._chk(lib().vslam_detect_batch_host(self._h, C.byref(params), fr.ctypes.data, params.rows * params.cols, n, C.byref(hl)), "vslam_detect_batch_host")
        for name, rec, off, cnt in keep:
            res[name] = (rec[: min(int(off[n]), len(rec))], off, cnt)
        return res

    def pack_lists(self, lists, counts, packed, offsets):
        """vslam_pack_lists_dev: lists [n, cap, k] (int32 / float32 records), counts [n] int32 -> packed (flat,
        any capacity), offsets [n + 1] int64.  CUDA tensors; asynchronous on the context stream."""
        n, cap = lists.shape[0], lists.shape[1]
        rb = lists[0, 0].numel() * lists.element_size()
        if not (lists.is_contiguous() and packed.is_contiguous() and counts.numel() >= n and offsets.numel() >= n + 1 and offsets.element_size() == 8):
            raise ValueError("pack_lists: bad tensors")
        self._chk(lib().vslam_pack_lists_dev(self._h, lists.data_ptr(), rb, cap, counts.data_ptr(), n, packed.data_ptr(),
                                             packed.numel() * packed.element_size(), offsets.data_ptr()), "vslam_pack_lists_dev")

    def pack_points16(self, lists, counts, packed, offsets):
        """vslam_pack_points16_dev: SLAM::point lists [n, cap, 6] int32, counts [n] int32 -> packed 16-byte records (any flat
        tensor; its byte size is the capacity), offsets [n + 1] int64.  CUDA tensors; asynchronous on the context stream."""
        n, cap = lists.shape[0], lists.shape[1]
        if not (lists.is_contiguous() and lists.shape[2] == 6 and lists.element_size() == 4 and packed.is_contiguous() and counts.numel() >= n and
                offsets.numel() >= n + 1 and offsets.element_size() == 8):
            raise ValueError("pack_points16: bad tensors")
        self._chk(lib().vslam_pack_points16_dev(self._h, lists.data_ptr(), cap, counts.data_ptr(), n, packed.data_ptr(),
                                                packed.numel() * packed.element_size(), offsets.data_ptr()), "vslam_pack_points16_dev")

    def count_totals(self, harris_counts, dog_counts, totals):
        """vslam_count_totals_dev: int32 [n] count tensors (either may be None) -> totals int64 [2], on the context stream."""
        n = (harris_counts if harris_counts is not None else dog_counts).numel()
        self._chk(lib().vslam_count_totals_dev(self._h, harris_counts.data_ptr() if harris_counts is not None else None,
                                               dog_counts.data_ptr() if dog_counts is not None else None, n, totals.data_ptr()), "vslam_count_totals_dev")

    def match(self, query: DescSets, train: DescSets, n_pairs: int | None = None, ratio2: float = 0.64, same_octave: bool = False,
              nn=None, matches=None, match_counts=None):
        """vslam_match_dev: pair j matches set j of `query` against set j of `train` (desc_sets()); asynchronous on the context stream.
        nn: int32 / float32 CUDA tensor of n_pairs * query.cap vslam_nn2 records (NN2_DTYPE), matches: n_pairs * match_cap vslam_match
        records (MATCH_DTYPE; match_cap = its second dimension), match_counts: int32 [n_pairs].  ratio2 is the SQUARED ratio."""
        n = min(query.n, train.n) if n_pairs is None else int(n_pairs)
        outs = dict(nn=nn, matches=matches, match_counts=match_counts)
        for name, t in outs.items():
            if t is not None and not (t.is_cuda and t.device.index == self.device and t.is_contiguous() and t.element_size() == 4):
                raise ValueError(f"match: {name} must be a contiguous 4-byte-element tensor on cuda:{self.device}")
        mo = _fill_out(MatchOut(), outs)
        if matches is not None:
            mo.match_cap = matches.shape[1]
        self._chk(lib().vslam_match_dev(self._h, C.byref(query), C.byref(train), n, float(ratio2), int(bool(same_octave)), C.byref(mo)), "vslam_match_dev")

    def match_host(self, q, t, ratio2: float = 0.64, same_octave: bool = False, q_defined=None, t_defined=None, q_points=None, t_points=None,
                   match_cap: int | None = None):
        """vslam_match_host: one pair of numpy descriptor arrays [n, 128] -> (nn [nq] NN2_DTYPE, matches MATCH_DTYPE, total accepted)."""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 128)
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1, 128)
        opt = [None if a is None else np.ascontiguousarray(a, dtype=dt) for a, dt in
               ((q_defined, np.uint8), (q_points, POINT_DTYPE), (t_defined, np.uint8), (t_points, POINT_DTYPE))]
        for a, rows in zip(opt, (len(q), len(q), len(t), len(t))):
            if a is not None and a.size != rows:
                raise ValueError("match_host: defined / points must have one entry per descriptor row")
        ptr = [None if a is None else a.ctypes.data for a in opt]
        cap = max(len(q), 1) if match_cap is None else int(match_cap)
        nn = np.zeros(len(q), NN2_DTYPE)
        matches = np.zeros(cap, MATCH_DTYPE)
        total = C.c_size_t()
        self._chk(lib().vslam_match_host(self._h, q.ctypes.data, ptr[0], ptr[1], len(q), t.ctypes.data, ptr[2], ptr[3], len(t), float(ratio2),
                                         int(bool(same_octave)), nn.ctypes.data, matches.ctypes.data, cap, C.byref(total)), "vslam_match_host")
        return nn, matches[: min(total.value, cap)], total.value

    def match_mutual(self, query: DescSets, train: DescSets, n_pairs: int | None = None, ratio2: float = 0.64, same_octave: bool = False,
                     nn=None, rnn=None, matches=None, match_counts=None):
        """vslam_match_mutual_dev: match() with the cross-check in the same pass; asynchronous on the context stream.  nn: as match()'s;
        rnn: int32 / float32 tensor of n_pairs * train.cap vslam_rnn records (RNN_DTYPE), the nearest query row of every train row;
        matches / match_counts: as match()'s, but the MUTUAL list - the accepted queries whose train row chose them back."""
        stage = "match_mutual"
        n = min(query.n, train.n) if n_pairs is None else int(n_pairs)
        outs = dict(nn=nn, rnn=rnn, matches=matches, match_counts=match_counts)
        _check_tensors(stage, self.where, outs, ())
        for name, t in outs.items():
            if t is not None and t.element_size() != 4:
                raise ValueError(f"{stage}: {name} must have 4-byte elements")
        if nn is None and rnn is None and match_counts is None:
            raise ValueError(f"{stage}: no output requested")
        if matches is not None and (match_counts is None or matches.dim() < 2):
            raise ValueError(f"{stage}: matches must be [n_pairs, match_cap, 3] and needs match_counts")
        mo = _fill_out(MatchMutualOut(), outs)
        if matches is not None:
            mo.match_cap = matches.shape[1]
        self._chk(lib().vslam_match_mutual_dev(self._h, C.byref(query), C.byref(train), n, float(ratio2), int(bool(same_octave)), C.byref(mo)),
                  "vslam_match_mutual_dev")

    def match_mutual_host(self, q, t, ratio2: float = 0.64, same_octave: bool = False, q_defined=None, t_defined=None, q_points=None, t_points=None,
                          match_cap: int | None = None):
        """vslam_match_mutual_host: one pair of numpy descriptor arrays [n, 128] -> (nn [nq] NN2_DTYPE, rnn [nt] RNN_DTYPE, matches
        MATCH_DTYPE: the mutual list, total mutual)."""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 128)
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1, 128)
        opt = [None if a is None else np.ascontiguousarray(a, dtype=dt) for a, dt in
               ((q_defined, np.uint8), (q_points, POINT_DTYPE), (t_defined, np.uint8), (t_points, POINT_DTYPE))]
        for a, rows in zip(opt, (len(q), len(q), len(t), len(t))):
            if a is not None and a.size != rows:
                raise ValueError("match_mutual_host: defined / points must have one entry per descriptor row")
        ptr = [None if a is None else a.ctypes.data for a in opt]
        cap = max(len(q), 1) if match_cap is None else int(match_cap)
        nn = np.zeros(len(q), NN2_DTYPE)
        rnn = np.zeros(len(t), RNN_DTYPE)
        matches = np.zeros(cap, MATCH_DTYPE)
        total = C.c_size_t()
        self._chk(lib().vslam_match_mutual_host(self._h, q.ctypes.data, ptr[0], ptr[1], len(q), t.ctypes.data, ptr[2], ptr[3], len(t), float(ratio2),
                                                int(bool(same_octave)), nn.ctypes.data, rnn.ctypes.data, matches.ctypes.data, cap, C.byref(total)),
                  "vslam_match_mutual_host")
        return nn, rnn, matches[: min(total.value, cap)], total.value

    def match_guided(self, query: DescSets, train: DescSets, models, n_pairs: int | None = None, ratio2: float = 0.64,
                     max_desc_dist2: float = float("inf"), max_dist2: float = 4.0, same_octave: bool = False, nn=None, matches=None,
                     match_counts=None):
        """vslam_match_guided_dev: match() restricted, per query row, to the train rows in its epipolar band under models[j].F;
        asynchronous on the context stream.  query / train: desc_sets() WITH points; models: the CUDA tensor epipolar(), refit() or
        homography()'s gate wrote (n_pairs * 88 bytes).  Outputs as match()'s.  ratio2 is the SQUARED ratio, max_desc_dist2 the
        absolute bound on an accepted d2 (inf: none), max_dist2 the SQUARED Sampson distance in pixels."""
        n = min(query.n, train.n) if n_pairs is None else int(n_pairs)
        outs = dict(nn=nn, matches=matches, match_counts=match_counts)
        for name, t in outs.items():
            if t is not None and not (t.is_cuda and t.device.index == self.device and t.is_contiguous() and t.element_size() == 4):
                raise ValueError(f"match_guided: {name} must be a contiguous 4-byte-element tensor on cuda:{self.device}")
        if not (models.is_cuda and models.device.index == self.device and models.is_contiguous()) or models.numel() * models.element_size() < n * 88:
            raise ValueError(f"match_guided: models must be a contiguous tensor of n_pairs * 88 bytes on cuda:{self.device}")
        mo = _fill_out(MatchOut(), outs)
        if matches is not None:
            mo.match_cap = matches.shape[1]
        prm = GuidedParams(float(ratio2), float(max_desc_dist2), float(max_dist2), int(bool(same_octave)), 0)
        self._chk(lib().vslam_match_guided_dev(self._h, C.byref(query), C.byref(train), models.data_ptr(), n, C.byref(prm), C.byref(mo)),
                  "vslam_match_guided_dev")

    def match_guided_host(self, q, t, q_points, t_points, model, ratio2: float = 0.64, max_desc_dist2: float = float("inf"), max_dist2: float = 4.0,
                          same_octave: bool = False, q_defined=None, t_defined=None, match_cap: int | None = None):
        """vslam_match_guided_host: one pair of numpy arrays (descriptors [n, 128], POINT_DTYPE points, one EPIPOLAR_DTYPE record) ->
        (nn [nq] NN2_DTYPE, matches MATCH_DTYPE, total accepted)."""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 128)
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1, 128)
        opt = [None if a is None else np.ascontiguousarray(a, dtype=dt) for a, dt in
               ((q_defined, np.uint8), (q_points, POINT_DTYPE), (t_defined, np.uint8), (t_points, POINT_DTYPE))]
        for a, rows in zip(opt, (len(q), len(q), len(t), len(t))):
            if a is not None and a.size != rows:
                raise ValueError("match_guided_host: defined / points must have one entry per descriptor row")
        ptr = [_ptr(a) for a in opt]
        mod = np.ascontiguousarray(model, dtype=EPIPOLAR_DTYPE).reshape(-1)[:1]
        cap = max(len(q), 1) if match_cap is None else int(match_cap)
        nn = np.zeros(len(q), NN2_DTYPE)
        matches = np.zeros(cap, MATCH_DTYPE)
        total = C.c_size_t()
        prm = GuidedParams(float(ratio2), float(max_desc_dist2), float(max_dist2), int(bool(same_octave)), 0)
        self._chk(lib().vslam_match_guided_host(self._h, q.ctypes.data, ptr[0], ptr[1], len(q), t.ctypes.data, ptr[2], ptr[3], len(t), mod.ctypes.data,
                                                C.byref(prm), nn.ctypes.data, matches.ctypes.data, cap, C.byref(total)), "vslam_match_guided_host")
        return nn, matches[: min(total.value, cap)], total.value

    def match_guided_hf(self, query: DescSets, train: DescSets, epipolar_models=None, homography_models=None, n_pairs: int | None = None,
                        ratio2: float = 0.64, max_desc_dist2: float = float("inf"), max_dist2: float = 4.0, max_transfer2: float = 4.0,
                        same_octave: bool = False, nn=None, matches=None, match_counts=None):
        """vslam_match_guided_hf_dev: match_guided() for every pair under the model that applies to it - the epipolar band where
        epipolar_models[j] has an F, a window of max_transfer2 (SQUARED pixels) around H x where only homography_models[j] has an H,
        nothing where neither has; asynchronous on the context stream.  epipolar_models: as match_guided()'s models (n_pairs * 88
        bytes; the intended one is homography()'s gate), homography_models: the CUDA tensor homography() wrote (n_pairs * 168 bytes);
        either may be None, not both.  Outputs as match()'s."""
        n = min(query.n, train.n) if n_pairs is None else int(n_pairs)
        stage = "match_guided_hf"
        if epipolar_models is None and homography_models is None:
            raise ValueError(f"{stage}: epipolar_models and homography_models are both None")
        outs = dict(nn=nn, matches=matches, match_counts=match_counts)
        _check_tensors(stage, self.where, dict(outs, epipolar_models=epipolar_models, homography_models=homography_models), ())
        for name, t in outs.items():
            if t is not None and t.element_size() != 4:
                raise ValueError(f"{stage}: {name} must have 4-byte elements")
        _check_sets(stage, n, (), (), ((epipolar_models, n * 88), (homography_models, n * 168)))
        mo = _fill_out(MatchOut(), outs)
        if matches is not None:
            mo.match_cap = matches.shape[1]
        prm = GuidedHfParams(float(ratio2), float(max_desc_dist2), float(max_dist2), float(max_transfer2), int(bool(same_octave)), 0)
        at = lambda t: None if t is None else t.data_ptr()
        self._chk(lib().vslam_match_guided_hf_dev(self._h, C.byref(query), C.byref(train), at(epipolar_models), at(homography_models), n, C.byref(prm),
                                                  C.byref(mo)), "vslam_match_guided_hf_dev")

    def match_guided_hf_host(self, q, t, q_points, t_points, epipolar_model=None, homography_model=None, ratio2: float = 0.64,
                             max_desc_dist2: float = float("inf"), max_dist2: float = 4.0, max_transfer2: float = 4.0, same_octave: bool = False,
                             q_defined=None, t_defined=None, match_cap: int | None = None):
        """vslam_match_guided_hf_host: one pair of numpy arrays (descriptors [n, 128], POINT_DTYPE points, one EPIPOLAR_DTYPE and / or
        one HOMOGRAPHY_DTYPE record) -> (nn [nq] NN2_DTYPE, matches MATCH_DTYPE, total accepted)."""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 128)
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1, 128)
        opt = [None if a is None else np.ascontiguousarray(a, dtype=dt) for a, dt in
               ((q_defined, np.uint8), (q_points, POINT_DTYPE), (t_defined, np.uint8), (t_points, POINT_DTYPE))]
        for a, rows in zip(opt, (len(q), len(q), len(t), len(t))):
            if a is not None and a.size != rows:
                raise ValueError("match_guided_hf_host: defined / points must have one entry per descriptor row")
        ptr = [_ptr(a) for a in opt]
        emod = None if epipolar_model is None else _records(epipolar_model, EPIPOLAR_DTYPE)[:1]
        hmod = None if homography_model is None else _records(homography_model, HOMOGRAPHY_DTYPE)[:1]
        cap = max(len(q), 1) if match_cap is None else int(match_cap)
        nn = np.zeros(len(q), NN2_DTYPE)
        matches = np.zeros(cap, MATCH_DTYPE)
        total = C.c_size_t()
        prm = GuidedHfParams(float(ratio2), float(max_desc_dist2), float(max_dist2), float(max_transfer2), int(bool(same_octave)), 0)
        self._chk(lib().vslam_match_guided_hf_host(self._h, q.ctypes.data, ptr[0], ptr[1], len(q), t.ctypes.data, ptr[2], ptr[3], len(t), _ptr(emod),
                                                   _ptr(hmod), C.byref(prm), nn.ctypes.data, matches.ctypes.data, cap, C.byref(total)),
                  "vslam_match_guided_hf_host")
        return nn, matches[: min(total.value, cap)], total.value

    def _two_view_lists(self, stage, n_pairs, required, tensors):
        """The checks epipolar() and pose() share over their tensors (by argument name, in the order they are reported) -> the number of pairs."""
        matches, match_counts, query_points, train_points = (tensors[k] for k in ("matches", "match_counts", "query_points", "train_points"))
        n = min(matches.shape[0], query_points.shape[0], train_points.shape[0]) if n_pairs is None else int(n_pairs)
        _check_tensors(stage, self.where, tensors, (required,))
        if matches.dim() != 3 or matches.shape[2] * matches.element_size() != 12 or query_points.dim() != 3 or train_points.dim() != 3:
            raise ValueError(f"{stage}: matches must be [n, match_cap, 3] 4-byte elements, the points [n, cap, 6]")
        if query_points.shape[2] * query_points.element_size() != 24 or train_points.shape[2] * train_points.element_size() != 24:
            raise ValueError(f"{stage}: points must be [n, cap, 6] int32")
        if min(matches.shape[0], match_counts.numel(), query_points.shape[0], train_points.shape[0]) < n or match_counts.element_size() != 4:
            raise ValueError(f"{stage}: fewer sets than pairs")
        return n

    def epipolar(self, matches, match_counts, query_points, train_points, n_pairs: int | None = None, n_hypotheses: int = 512, seed: int = 1,
                 max_dist2: float = 4.0, models=None, inlier_bits=None, inliers=None, inlier_counts=None, hypotheses=None):
        """vslam_epipolar_dev: the RANSAC fundamental matrix of every pair from the tensors match() and detect_batch() wrote;
        asynchronous on the context stream.  matches [n, match_cap, 3] (MATCH_DTYPE records), match_counts int32 [n], query_points /
        train_points int32 [n, cap, 6] (train_points = query_points[1:] for consecutive frames).  Outputs, CUDA tensors: models - any
        contiguous tensor of n_pairs * 88 bytes (EPIPOLAR_DTYPE after .cpu().numpy().view), inlier_bits int64 [n, (match_cap + 63) // 64],
        inliers [n, inlier_cap, 3] like matches, inlier_counts int32 [n], hypotheses n_pairs * n_hypotheses * 80 bytes
        (EPIPOLAR_HYP_DTYPE).  max_dist2 is the SQUARED Sampson distance in pixels."""
        outs = dict(models=models, inlier_bits=inlier_bits, inliers=inliers, inlier_counts=inlier_counts, hypotheses=hypotheses)
        n = self._two_view_lists("epipolar", n_pairs, "models", dict(matches=matches, match_counts=match_counts, query_points=query_points, train_points=train_points, **outs))
        eo = _fill_out(EpipolarOut(), outs)
        if inliers is not None:
            eo.inlier_cap = inliers.shape[1]
        prm = EpipolarParams(int(n_hypotheses), int(seed) & 0xFFFFFFFF, float(max_dist2))
        self._chk(lib().vslam_epipolar_dev(self._h, matches.data_ptr(), match_counts.data_ptr(), matches.shape[1], query_points.data_ptr(),
                                           query_points.shape[1], train_points.data_ptr(), train_points.shape[1], n, C.byref(prm), C.byref(eo)),
                  "vslam_epipolar_dev")

    def epipolar_host(self, matches, query_points, train_points, n_hypotheses: int = 512, seed: int = 1, max_dist2: float = 4.0,
                      inlier_cap: int | None = None, want_bits: bool = True, want_inliers: bool = True, want_hypotheses: bool = False):
        """vslam_epipolar_host: one pair of numpy arrays (MATCH_DTYPE, POINT_DTYPE, POINT_DTYPE) -> (model: one EPIPOLAR_DTYPE record,
        inlier_bits uint64 [(m + 63) // 64] or None, inliers MATCH_DTYPE or None, total inliers or None, hypotheses or None)."""
        mt, qp, tp = _host_lists(matches, query_points, train_points)
        m = len(mt)
        cap = max(m, 1) if inlier_cap is None else int(inlier_cap)
        model = np.zeros(1, EPIPOLAR_DTYPE)
        bits = np.zeros((m + 63) // 64, np.uint64) if want_bits else None
        inl = np.zeros(cap, MATCH_DTYPE) if want_inliers else None
        hyp = np.zeros(int(n_hypotheses), EPIPOLAR_HYP_DTYPE) if want_hypotheses else None
        total = C.c_size_t()
        prm = EpipolarParams(int(n_hypotheses), int(seed) & 0xFFFFFFFF, float(max_dist2))
        self._chk(lib().vslam_epipolar_host(self._h, _ptr(mt), m, _ptr(qp), len(qp), _ptr(tp), len(tp), C.byref(prm), model.ctypes.data, _ptr(bits),
                                            None if inl is None else inl.ctypes.data, cap, C.byref(total) if want_inliers else None, _ptr(hyp)),
                  "vslam_epipolar_host")
        return (model[0], bits, None if inl is None else inl[: min(total.value, cap)], total.value if want_inliers else None, hyp)

    def refit(self, models_in, matches, match_counts, query_points, train_points, n_pairs: int | None = None, rounds: int = 4, max_dist2: float = 4.0,
              models=None, info=None, inlier_bits=None, inliers=None, inlier_counts=None):
        """vslam_refit_dev: the least-squares refit of every pair's fundamental matrix over its inliers, between epipolar() and
        pose(); asynchronous on the context stream.  models_in: the tensor epipolar() wrote; matches / match_counts: the FULL list
        epipolar() read.  Outputs, CUDA tensors: models n_pairs * 88 bytes (may be models_in itself), info n_pairs * 16 bytes
        (REFIT_DTYPE), inlier_bits / inliers / inlier_counts as epipolar()'s, under the output F."""
        outs = dict(models=models, info=info, inlier_bits=inlier_bits, inliers=inliers, inlier_counts=inlier_counts)
        n = self._two_view_lists("refit", n_pairs, "models", dict(models_in=models_in, matches=matches, match_counts=match_counts, query_points=query_points, train_points=train_points, **outs))
        if models_in.numel() * models_in.element_size() < n * 88:
            raise ValueError("refit: models_in must hold n_pairs * 88 bytes")
        ro = _fill_out(RefitOut(), outs)
        if inliers is not None:
            ro.inlier_cap = inliers.shape[1]
        prm = RefitParams(int(rounds), float(max_dist2))
        self._chk(lib().vslam_refit_dev(self._h, models_in.data_ptr(), matches.data_ptr(), match_counts.data_ptr(), matches.shape[1],
                                        query_points.data_ptr(), query_points.shape[1], train_points.data_ptr(), train_points.shape[1], n,
                                        C.byref(prm), C.byref(ro)), "vslam_refit_dev")

    def refit_host(self, model, matches, query_points, train_points, rounds: int = 4, max_dist2: float = 4.0, inlier_cap: int | None = None,
                   want_bits: bool = True, want_inliers: bool = True):
        """vslam_refit_host: one pair of numpy arrays (one EPIPOLAR_DTYPE record, MATCH_DTYPE, POINT_DTYPE, POINT_DTYPE) -> (model: one
        EPIPOLAR_DTYPE record, info: one REFIT_DTYPE record, inlier_bits uint64 [(m + 63) // 64] or None, inliers MATCH_DTYPE or None,
        total inliers or None)."""
        mod = np.ascontiguousarray(model, dtype=EPIPOLAR_DTYPE).reshape(-1)[:1]
        mt, qp, tp = _host_lists(matches, query_points, train_points)
        m = len(mt)
        cap = max(m, 1) if inlier_cap is None else int(inlier_cap)
        out, info = np.zeros(1, EPIPOLAR_DTYPE), np.zeros(1, REFIT_DTYPE)
        bits = np.zeros((m + 63) // 64, np.uint64) if want_bits else None
        inl = np.zeros(cap, MATCH_DTYPE) if want_inliers else None
        total = C.c_size_t()
        prm = RefitParams(int(rounds), float(max_dist2))
        self._chk(lib().vslam_refit_host(self._h, mod.ctypes.data, _ptr(mt), m, _ptr(qp), len(qp), _ptr(tp), len(tp), C.byref(prm), out.ctypes.data,
                                         info.ctypes.data, _ptr(bits), None if inl is None else inl.ctypes.data, cap,
                                         C.byref(total) if want_inliers else None), "vslam_refit_host")
        return out[0], info[0], bits, None if inl is None else inl[: min(total.value, cap)], total.value if want_inliers else None

    def homography(self, matches, match_counts, query_points, train_points, n_pairs: int | None = None, n_hypotheses: int = 512, seed: int = 1,
                   max_dist2: float = 4.0, degenerate_num: int = 1, degenerate_den: int = 2, min_inliers: int = 16, epipolar_models=None,
                   models=None, inlier_bits=None, inliers=None, inlier_counts=None, hypotheses=None, gated_models=None):
        """vslam_homography_dev: the RANSAC homography of every pair over the lists epipolar() reads and, with epipolar_models (the
        models tensor epipolar() or refit() wrote), the degeneracy verdict; asynchronous on the context stream.  Outputs, CUDA
        tensors: models - any contiguous tensor of n_pairs * 168 bytes (HOMOGRAPHY_DTYPE after .cpu().numpy().view), inlier_bits /
        inliers / inlier_counts as epipolar()'s, hypotheses n_pairs * n_hypotheses * 152 bytes (HOMOGRAPHY_HYP_DTYPE), gated_models
        n_pairs * 88 bytes (may be epipolar_models itself): the epipolar models with every degenerate pair made "no model", for
        refit() and pose().  max_dist2 is the SQUARED transfer error in pixels, each direction."""
        outs = dict(models=models, inlier_bits=inlier_bits, inliers=inliers, inlier_counts=inlier_counts, hypotheses=hypotheses, gated_models=gated_models)
        n = self._two_view_lists("homography", n_pairs, "models", dict(matches=matches, match_counts=match_counts, query_points=query_points, train_points=train_points, epipolar_models=epipolar_models, **outs))
        if epipolar_models is not None and epipolar_models.numel() * epipolar_models.element_size() < n * 88:
            raise ValueError("homography: epipolar_models must hold n_pairs * 88 bytes")
        ho = _fill_out(HomographyOut(), outs)
        if inliers is not None:
            ho.inlier_cap = inliers.shape[1]
        prm = HomographyParams(int(n_hypotheses), int(seed) & 0xFFFFFFFF, float(max_dist2), int(degenerate_num), int(degenerate_den), int(min_inliers))
        self._chk(lib().vslam_homography_dev(self._h, matches.data_ptr(), match_counts.data_ptr(), matches.shape[1], query_points.data_ptr(),
                                             query_points.shape[1], train_points.data_ptr(), train_points.shape[1], n,
                                             None if epipolar_models is None else epipolar_models.data_ptr(), C.byref(prm), C.byref(ho)),
                  "vslam_homography_dev")

    def homography_host(self, matches, query_points, train_points, n_hypotheses: int = 512, seed: int = 1, max_dist2: float = 4.0,
                        degenerate_num: int = 1, degenerate_den: int = 2, min_inliers: int = 16, epipolar_model=None, inlier_cap: int | None = None,
                        want_bits: bool = True, want_inliers: bool = True, want_hypotheses: bool = False):
        """vslam_homography_host: one pair of numpy arrays (MATCH_DTYPE, POINT_DTYPE, POINT_DTYPE; epipolar_model: one EPIPOLAR_DTYPE
        record or None) -> (model: one HOMOGRAPHY_DTYPE record, inlier_bits uint64 [(m + 63) // 64] or None, inliers MATCH_DTYPE or
        None, total inliers or None, hypotheses or None, gated model: one EPIPOLAR_DTYPE record, or None without epipolar_model)."""
        mt, qp, tp = _host_lists(matches, query_points, train_points)
        m = len(mt)
        cap = max(m, 1) if inlier_cap is None else int(inlier_cap)
        epi = None if epipolar_model is None else np.ascontiguousarray(epipolar_model, dtype=EPIPOLAR_DTYPE).reshape(-1)[:1]
        model = np.zeros(1, HOMOGRAPHY_DTYPE)
        gated = None if epi is None else np.zeros(1, EPIPOLAR_DTYPE)
        bits = np.zeros((m + 63) // 64, np.uint64) if want_bits else None
        inl = np.zeros(cap, MATCH_DTYPE) if want_inliers else None
        hyp = np.zeros(int(n_hypotheses), HOMOGRAPHY_HYP_DTYPE) if want_hypotheses else None
        total = C.c_size_t()
        prm = HomographyParams(int(n_hypotheses), int(seed) & 0xFFFFFFFF, float(max_dist2), int(degenerate_num), int(degenerate_den), int(min_inliers))
        self._chk(lib().vslam_homography_host(self._h, _ptr(mt), m, _ptr(qp), len(qp), _ptr(tp), len(tp), None if epi is None else epi.ctypes.data,
                                              C.byref(prm), model.ctypes.data, _ptr(bits), None if inl is None else inl.ctypes.data, cap,
                                              C.byref(total) if want_inliers else None, _ptr(hyp), None if gated is None else gated.ctypes.data),
                  "vslam_homography_host")
        return (model[0], bits, None if inl is None else inl[: min(total.value, cap)], total.value if want_inliers else None, hyp,
                None if gated is None else gated[0])

    def hrefit(self, models_in, matches, match_counts, query_points, train_points, n_pairs: int | None = None, rounds: int = 4, max_dist2: float = 4.0,
               degenerate_num: int = 1, degenerate_den: int = 2, min_inliers: int = 16, epipolar_models=None, models=None, info=None,
               inlier_bits=None, inliers=None, inlier_counts=None, gated_models=None):
        """vslam_hrefit_dev: the least-squares refit of every pair's homography over its inliers, after homography() and before
        match_guided_hf() / hpose(); asynchronous on the context stream.  models_in: the tensor homography() wrote; matches /
        match_counts: the FULL list homography() read.  With epipolar_models (the tensor epipolar() or refit() wrote) the verdict is
        computed again from the new inlier count.  Outputs, CUDA tensors: models n_pairs * 168 bytes (may be models_in itself), info
        n_pairs * 16 bytes (HREFIT_DTYPE), inlier_bits / inliers / inlier_counts as homography()'s, under the output (H, G),
        gated_models n_pairs * 88 bytes (may be epipolar_models itself)."""
        outs = dict(models=models, info=info, inlier_bits=inlier_bits, inliers=inliers, inlier_counts=inlier_counts, gated_models=gated_models)
        n = self._two_view_lists("hrefit", n_pairs, "models", dict(models_in=models_in, matches=matches, match_counts=match_counts, query_points=query_points, train_points=train_points, epipolar_models=epipolar_models, **outs))
        if models_in.numel() * models_in.element_size() < n * 168:
            raise ValueError("hrefit: models_in must hold n_pairs * 168 bytes")
        if epipolar_models is not None and epipolar_models.numel() * epipolar_models.element_size() < n * 88:
            raise ValueError("hrefit: epipolar_models must hold n_pairs * 88 bytes")
        ro = _fill_out(HRefitOut(), outs)
        if inliers is not None:
            ro.inlier_cap = inliers.shape[1]
        prm = HRefitParams(int(rounds), float(max_dist2), int(degenerate_num), int(degenerate_den), int(min_inliers))
        self._chk(lib().vslam_hrefit_dev(self._h, models_in.data_ptr(), matches.data_ptr(), match_counts.data_ptr(), matches.shape[1],
                                         query_points.data_ptr(), query_points.shape[1], train_points.data_ptr(), train_points.shape[1], n,
                                         None if epipolar_models is None else epipolar_models.data_ptr(), C.byref(prm), C.byref(ro)),
                  "vslam_hrefit_dev")

    def hrefit_host(self, model, matches, query_points, train_points, rounds: int = 4, max_dist2: float = 4.0, degenerate_num: int = 1,
                    degenerate_den: int = 2, min_inliers: int = 16, epipolar_model=None, inlier_cap: int | None = None, want_bits: bool = True,
                    want_inliers: bool = True):
        """vslam_hrefit_host: one pair of numpy arrays (one HOMOGRAPHY_DTYPE record, MATCH_DTYPE, POINT_DTYPE, POINT_DTYPE; epipolar_model:
        one EPIPOLAR_DTYPE record or None) -> (model: one HOMOGRAPHY_DTYPE record, info: one HREFIT_DTYPE record, inlier_bits uint64
        [(m + 63) // 64] or None, inliers MATCH_DTYPE or None, total inliers or None, gated model: one EPIPOLAR_DTYPE record, or None
        without epipolar_model)."""
        mod = np.ascontiguousarray(model, dtype=HOMOGRAPHY_DTYPE).reshape(-1)[:1]
        mt, qp, tp = _host_lists(matches, query_points, train_points)
        m = len(mt)
        cap = max(m, 1) if inlier_cap is None else int(inlier_cap)
        epi = None if epipolar_model is None else np.ascontiguousarray(epipolar_model, dtype=EPIPOLAR_DTYPE).reshape(-1)[:1]
        out, info = np.zeros(1, HOMOGRAPHY_DTYPE), np.zeros(1, HREFIT_DTYPE)
        gated = None if epi is None else np.zeros(1, EPIPOLAR_DTYPE)
        bits = np.zeros((m + 63) // 64, np.uint64) if want_bits else None
        inl = np.zeros(cap, MATCH_DTYPE) if want_inliers else None
        total = C.c_size_t()
        prm = HRefitParams(int(rounds), float(max_dist2), int(degenerate_num), int(degenerate_den), int(min_inliers))
        self._chk(lib().vslam_hrefit_host(self._h, mod.ctypes.data, _ptr(mt), m, _ptr(qp), len(qp), _ptr(tp), len(tp),
                                          None if epi is None else epi.ctypes.data, C.byref(prm), out.ctypes.data, info.ctypes.data, _ptr(bits),
                                          None if inl is None else inl.ctypes.data, cap, C.byref(total) if want_inliers else None,
                                          None if gated is None else gated.ctypes.data), "vslam_hrefit_host")
        return (out[0], info[0], bits, None if inl is None else inl[: min(total.value, cap)], total.value if want_inliers else None,
                None if gated is None else gated[0])

    def pose(self, models, matches, match_counts, query_points, train_points, intrinsics, n_pairs: int | None = None, poses=None, candidates=None,
             points=None, front_bits=None):
        """vslam_pose_dev: the camera motion of every pair (x_train ~ R x_query + t, |t| = 1) and the 3-D point of every match
        record, from the models tensor epipolar() wrote and a match list - the intended one is epipolar()'s inliers / inlier_counts;
        asynchronous on the context stream.  intrinsics = (fx, fy, cx, cy).  Outputs, CUDA tensors: poses - any contiguous tensor of
        n_pairs * 112 bytes (POSE_DTYPE after .cpu().numpy().view), candidates n_pairs * 4 * 104 bytes (POSE_CAND_DTYPE), points
        float64 [n, match_cap, 3] (query-camera frame), front_bits int64 [n, (match_cap + 63) // 64]."""
        outs = dict(poses=poses, candidates=candidates, points=points, front_bits=front_bits)
        n = self._two_view_lists("pose", n_pairs, "poses", dict(models=models, matches=matches, match_counts=match_counts, query_points=query_points, train_points=train_points, **outs))
        if models.numel() * models.element_size() < n * 88:
            raise ValueError("pose: models must hold n_pairs * 88 bytes")
        po = _fill_out(PoseOut(), outs)
        prm = PoseParams(*(float(v) for v in intrinsics))
        self._chk(lib().vslam_pose_dev(self._h, models.data_ptr(), matches.data_ptr(), match_counts.data_ptr(), matches.shape[1],
                                       query_points.data_ptr(), query_points.shape[1], train_points.data_ptr(), train_points.shape[1], n,
                                       C.byref(prm), C.byref(po)), "vslam_pose_dev")

    def pose_host(self, model, matches, query_points, train_points, intrinsics, want_candidates: bool = True, want_points: bool = True,
                  want_bits: bool = True):
        """vslam_pose_host: one pair of numpy arrays (one EPIPOLAR_DTYPE record, MATCH_DTYPE, POINT_DTYPE, POINT_DTYPE) -> (pose: one
        POSE_DTYPE record, candidates [4] POSE_CAND_DTYPE or None, points float64 [m, 3] or None - None too when there is no winner -,
        front_bits uint64 [(m + 63) // 64] or None)."""
        mod = np.ascontiguousarray(model, dtype=EPIPOLAR_DTYPE).reshape(-1)[:1]
        mt, qp, tp = _host_lists(matches, query_points, train_points)
        m = len(mt)
        pose = np.zeros(1, POSE_DTYPE)
        cand = np.zeros(4, POSE_CAND_DTYPE) if want_candidates else None
        pts = np.zeros((max(m, 1), 3), np.float64) if want_points else None
        bits = np.zeros((m + 63) // 64, np.uint64) if want_bits else None
        prm = PoseParams(*(float(v) for v in intrinsics))
        self._chk(lib().vslam_pose_host(self._h, mod.ctypes.data, _ptr(mt), m, _ptr(qp), len(qp), _ptr(tp), len(tp), C.byref(prm), pose.ctypes.data,
                                        _ptr(cand), _ptr(pts), _ptr(bits)), "vslam_pose_host")
        return pose[0], cand, (pts[:m] if want_points and int(pose["best"][0]) >= 0 else None), bits

    def hpose(self, models, matches, match_counts, query_points, train_points, intrinsics, max_dist2: float = 4.0, min_spread: float = HPOSE_MIN_SPREAD,
              ambiguous_num: int = HPOSE_AMBIGUOUS_NUM, ambiguous_den: int = HPOSE_AMBIGUOUS_DEN, only_degenerate: bool = True, priors=None,
              n_pairs: int | None = None, poses=None, info=None, candidates=None, points=None, front_bits=None):
        """vslam_hpose_dev: pose from homography - (R, t), the plane and the 3-D points of the pairs a homography explains, written
        into the tensors pose() wrote; asynchronous on the context stream.  models: the tensor homography() wrote (n_pairs * 168
        bytes); matches / match_counts: the list pose() read; priors (optional): n_pairs * 112 bytes of POSE_DTYPE records, e.g. a COPY of
        the previous pairs' poses - it must not overlap an output.  Outputs, CUDA tensors: poses n_pairs * 112 bytes and info n_pairs * 144 bytes (HPOSE_DTYPE), both
        required; candidates n_pairs * 4 * 128 bytes (HPOSE_CAND_DTYPE), points float64 [n, match_cap, 3], front_bits int64
        [n, (match_cap + 63) // 64].  Only the pairs the call selects are written in poses, points and front_bits."""
        outs = dict(poses=poses, info=info, candidates=candidates, points=points, front_bits=front_bits)
        n = self._two_view_lists("hpose", n_pairs, "poses", dict(models=models, matches=matches, match_counts=match_counts, query_points=query_points, train_points=train_points, priors=priors, **outs))
        if info is None:
            raise ValueError("hpose: info is required")
        if models.numel() * models.element_size() < n * 168:
            raise ValueError("hpose: models must hold n_pairs * 168 bytes")
        if priors is not None and priors.numel() * priors.element_size() < n * 112:
            raise ValueError("hpose: priors must hold n_pairs * 112 bytes")
        ho = _fill_out(HposeOut(), outs)
        prm = HposeParams(PoseParams(*(float(v) for v in intrinsics)), float(max_dist2), float(min_spread), int(ambiguous_num), int(ambiguous_den),
                          int(bool(only_degenerate)), 0)
        self._chk(lib().vslam_hpose_dev(self._h, models.data_ptr(), matches.data_ptr(), match_counts.data_ptr(), matches.shape[1],
                                        query_points.data_ptr(), query_points.shape[1], train_points.data_ptr(), train_points.shape[1], n,
                                        None if priors is None else priors.data_ptr(), C.byref(prm), C.byref(ho)), "vslam_hpose_dev")

    def hpose_host(self, models, matches, match_counts, query_points, train_points, intrinsics, poses, max_dist2: float = 4.0,
                   min_spread: float = HPOSE_MIN_SPREAD, ambiguous_num: int = HPOSE_AMBIGUOUS_NUM, ambiguous_den: int = HPOSE_AMBIGUOUS_DEN,
                   only_degenerate: bool = True, priors=None, points=None, front_bits=None, want_candidates: bool = False):
        """vslam_hpose_host: the same call over numpy arrays - models [n] HOMOGRAPHY_DTYPE, matches [n, match_cap] MATCH_DTYPE,
        match_counts [n], query_points [n, query_cap] / train_points [n, train_cap] POINT_DTYPE, priors [n] POSE_DTYPE or None -
        -> (info [n] HPOSE_DTYPE, candidates [n, 4] HPOSE_CAND_DTYPE or None).  poses [n] POSE_DTYPE, points float64
        [n, match_cap, 3] and front_bits uint64 [n, (match_cap + 63) // 64] are written in place (C-contiguous arrays of exactly that
        type; points and front_bits optional): what the call leaves untouched keeps its bytes."""
        mod = _records(models, HOMOGRAPHY_DTYPE)
        n = len(mod)
        mt = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        qp, tp = np.ascontiguousarray(query_points, dtype=POINT_DTYPE), np.ascontiguousarray(train_points, dtype=POINT_DTYPE)
        if mt.ndim != 2 or qp.ndim != 2 or tp.ndim != 2 or not (mt.shape[0] == qp.shape[0] == tp.shape[0] == n):
            raise ValueError("hpose_host: matches, query_points and train_points must be [n, cap]")
        cap, cnt = mt.shape[1], _counts(match_counts)
        pri = None if priors is None else _records(priors, POSE_DTYPE)
        if len(cnt) != n or (pri is not None and len(pri) != n):
            raise ValueError("hpose_host: one count and one prior per pair")
        _check_host_outs("hpose_host", (("poses", poses, POSE_DTYPE, n), ("points", points, np.float64, n * cap * 3),
                                        ("front_bits", front_bits, np.uint64, n * ((cap + 63) // 64))))
        if poses is None:
            raise ValueError("hpose_host: poses is required")
        info = np.zeros(max(n, 1), HPOSE_DTYPE)
        cand = np.zeros((max(n, 1), 4), HPOSE_CAND_DTYPE) if want_candidates else None
        ho = _fill_out(HposeOut(), dict(poses=poses, info=info, candidates=cand, points=points, front_bits=front_bits))
        prm = HposeParams(PoseParams(*(float(v) for v in intrinsics)), float(max_dist2), float(min_spread), int(ambiguous_num), int(ambiguous_den),
                          int(bool(only_degenerate)), 0)
        self._chk(lib().vslam_hpose_host(self._h, mod.ctypes.data, mt.ctypes.data, cnt.ctypes.data, cap, qp.ctypes.data, qp.shape[1], tp.ctypes.data,
                                         tp.shape[1], n, None if pri is None else pri.ctypes.data, C.byref(prm), C.byref(ho)), "vslam_hpose_host")
        return info[:n], (None if cand is None else cand[:n])

    def chain(self, poses, matches, match_counts, points, front_bits, point_cap: int, min_links: int = 16, n_pairs: int | None = None, chain=None,
              map=None, links=None, ratios=None):
        """vslam_chain_dev: the poses and points pose() wrote for n consecutive pairs (pair j: frames j and j + 1), chained with the
        recovered scale into one world frame per segment; asynchronous on the context stream.  poses, matches [n, match_cap, 3],
        match_counts, points float64 [n, match_cap, 3] and front_bits [n, (match_cap + 63) // 64] are the tensors pose() read and
        wrote; point_cap is the capacity of the frames' point lists.  Outputs, CUDA tensors: chain - any contiguous tensor of
        n_pairs * 176 bytes (CHAIN_DTYPE after .cpu().numpy().view), map float64 [n, match_cap, 3] (world coordinates), links int32
        [n, match_cap], ratios float64 [n, match_cap]."""
        tensors = dict(poses=poses, matches=matches, match_counts=match_counts, points=points, front_bits=front_bits, chain=chain, map=map, links=links,
                       ratios=ratios)
        _check_tensors("chain", self.where, tensors, ("poses", "matches", "match_counts", "points", "front_bits", "chain"))
        _check_records("chain", "matches", matches, 12, "[n, match_cap, 3]")
        n, cap = matches.shape[0] if n_pairs is None else int(n_pairs), matches.shape[1]
        _check_sets("chain", n, (matches,), (match_counts,), ((poses, n * 112), (points, n * cap * 24), (front_bits, n * ((cap + 63) // 64) * 8)))
        co = _fill_out(ChainOut(), dict(chain=chain, map=map, links=links, ratios=ratios))
        prm = ChainParams(int(min_links))
        self._chk(lib().vslam_chain_dev(self._h, poses.data_ptr(), matches.data_ptr(), match_counts.data_ptr(), cap, points.data_ptr(),
                                        front_bits.data_ptr(), int(point_cap), n, C.byref(prm), C.byref(co)), "vslam_chain_dev")

    def chain_host(self, poses, matches, match_counts, points, front_bits, point_cap: int, min_links: int = 16, map=None, links=None, ratios=None):
        """vslam_chain_host: the same call over numpy arrays - poses [n] POSE_DTYPE, matches [n, match_cap] MATCH_DTYPE, match_counts
        [n], points float64 [n, match_cap, 3], front_bits uint64 [n, (match_cap + 63) // 64] - -> chain [n] CHAIN_DTYPE.  map float64
        [n, match_cap, 3], links int32 [n, match_cap] and ratios float64 [n, match_cap] are written in place when given (C-contiguous
        arrays of exactly that type); the rows the call leaves untouched keep their bytes."""
        ps, mt, n, cap = _host_structure("chain_host", poses, matches)
        cnt, pts, fb = _counts(match_counts), np.ascontiguousarray(points, dtype=np.float64), _words(front_bits)
        if len(cnt) != n or pts.size != n * cap * 3 or fb.size != n * ((cap + 63) // 64):
            raise ValueError("chain_host: one count, match_cap points and (match_cap + 63) // 64 words per pair")
        _check_host_outs("chain_host", (("map", map, np.float64, n * cap * 3), ("links", links, np.int32, n * cap), ("ratios", ratios, np.float64, n * cap)))
        chain = np.zeros(max(n, 1), CHAIN_DTYPE)
        co = _fill_out(ChainOut(), dict(chain=chain, map=map, links=links, ratios=ratios))
        prm = ChainParams(int(min_links))
        self._chk(lib().vslam_chain_host(self._h, ps.ctypes.data, mt.ctypes.data, cnt.ctypes.data, cap, pts.ctypes.data, fb.ctypes.data, int(point_cap), n,
                                         C.byref(prm), C.byref(co)), "vslam_chain_host")
        return chain[:n]

    def tracks(self, poses, matches, match_counts, front_bits, point_cap: int, chain, frame_points, intrinsics, max_dist2: float = 4.0,
               min_views: int = 2, n_pairs: int | None = None, tracks=None, refs=None, good_bits=None, summary=None):
        """vslam_tracks_dev: the records of consecutive pairs that saw one scene point linked into tracks, and every track's point
        triangulated from all of its views; asynchronous on the context stream.  poses, matches [n, match_cap, 3], match_counts and
        front_bits are the tensors chain() read, chain the records it wrote, frame_points [n + 1, point_cap, 6] the frames' point
        lists; intrinsics = (fx, fy, cx, cy).  Outputs, CUDA tensors: tracks - any contiguous tensor of n * match_cap * 48 bytes
        (TRACK_DTYPE after .cpu().numpy().view), refs n * match_cap * 8 bytes (TRACK_REF_DTYPE), good_bits [n, (match_cap + 63) // 64]
        8-byte words, summary n * 16 bytes (TRACK_SUMMARY_DTYPE)."""
        tensors = dict(poses=poses, matches=matches, match_counts=match_counts, front_bits=front_bits, chain=chain, frame_points=frame_points,
                       tracks=tracks, refs=refs, good_bits=good_bits, summary=summary)
        _check_tensors("tracks", self.where, tensors, ("poses", "matches", "match_counts", "front_bits", "chain", "frame_points", "tracks"))
        _check_records("tracks", "matches", matches, 12, "[n, match_cap, 3]")
        n, cap = matches.shape[0] if n_pairs is None else int(n_pairs), matches.shape[1]
        _check_sets("tracks", n, (matches,), (match_counts,), ((poses, n * 112), (chain, n * 176), (front_bits, n * ((cap + 63) // 64) * 8),
                                                               (frame_points, (n + 1) * int(point_cap) * 24)))
        to = _fill_out(TracksOut(), dict(tracks=tracks, refs=refs, good_bits=good_bits, summary=summary))
        prm = TracksParams(PoseParams(*(float(v) for v in intrinsics)), float(max_dist2), int(min_views), 0)
        self._chk(lib().vslam_tracks_dev(self._h, poses.data_ptr(), matches.data_ptr(), match_counts.data_ptr(), cap, front_bits.data_ptr(),
                                         int(point_cap), n, chain.data_ptr(), frame_points.data_ptr(), C.byref(prm), C.byref(to)), "vslam_tracks_dev")

    def tracks_host(self, poses, matches, match_counts, front_bits, point_cap: int, chain, frame_points, intrinsics, max_dist2: float = 4.0,
                    min_views: int = 2, tracks=None, refs=None, good_bits=None, summary=None):
        """vslam_tracks_host: the same call over numpy arrays - poses [n] POSE_DTYPE, matches [n, match_cap] MATCH_DTYPE, match_counts
        [n], front_bits uint64 [n, (match_cap + 63) // 64], chain [n] CHAIN_DTYPE, frame_points [n + 1, point_cap] POINT_DTYPE - ->
        tracks [n, match_cap] TRACK_DTYPE.  tracks (TRACK_DTYPE [n, match_cap]: the rows the call leaves untouched keep their bytes),
        refs (TRACK_REF_DTYPE [n, match_cap]), good_bits (uint64 [n, words]) and summary (TRACK_SUMMARY_DTYPE [n]) are written in
        place when given (C-contiguous arrays of exactly that type)."""
        ps, mt, n, cap = _host_structure("tracks_host", poses, matches)
        words = (cap + 63) // 64
        cnt, fb, ch, fp = _counts(match_counts), _words(front_bits), _records(chain, CHAIN_DTYPE), _records(frame_points, POINT_DTYPE)
        if len(cnt) != n or fb.size != n * words or len(ch) != n or len(fp) != (n + 1) * int(point_cap):
            raise ValueError("tracks_host: one count, one chain record and (match_cap + 63) // 64 words per pair, point_cap points per frame")
        if tracks is None:
            tracks = np.zeros((n, cap), TRACK_DTYPE)
        _check_host_outs("tracks_host", (("tracks", tracks, TRACK_DTYPE, n * cap), ("refs", refs, TRACK_REF_DTYPE, n * cap),
                                         ("good_bits", good_bits, np.uint64, n * words), ("summary", summary, TRACK_SUMMARY_DTYPE, n)))
        to = _fill_out(TracksOut(), dict(tracks=tracks, refs=refs, good_bits=good_bits, summary=summary))
        prm = TracksParams(PoseParams(*(float(v) for v in intrinsics)), float(max_dist2), int(min_views), 0)
        self._chk(lib().vslam_tracks_host(self._h, ps.ctypes.data, mt.ctypes.data, cnt.ctypes.data, cap, fb.ctypes.data, int(point_cap), n,
                                          ch.ctypes.data, fp.ctypes.data, C.byref(prm), C.byref(to)), "vslam_tracks_host")
        return tracks

    def bundle(self, poses, matches, match_counts, front_bits, point_cap: int, chain, frame_points, tracks_in, refs, intrinsics, max_dist2: float = 4.0,
               min_views: int = 2, sweeps: int = 4, n_pairs: int | None = None, cams_in=None, tracks=None, cams=None, point_info=None, member_bits=None):
        """vslam_bundle_dev: alternating Gauss-Newton over the tracks' points and the train cameras; asynchronous on the context
        stream.  poses .. frame_points are the tensors tracks() read, tracks_in and refs the tensors it wrote; cams_in (optional) n * 160
        bytes (BUNDLE_CAM_DTYPE: only W, w are read).  Outputs, CUDA tensors: tracks - n * match_cap * 48 bytes, may be tracks_in itself -,
        cams n * 160 bytes (BUNDLE_CAM_DTYPE), point_info n * match_cap * 40 bytes (BUNDLE_POINT_DTYPE), member_bits [n, 2, (match_cap +
        63) // 64] 8-byte words."""
        tensors = dict(poses=poses, matches=matches, match_counts=match_counts, front_bits=front_bits, chain=chain, frame_points=frame_points,
                       tracks_in=tracks_in, refs=refs, cams_in=cams_in, tracks=tracks, cams=cams, point_info=point_info, member_bits=member_bits)
        _check_tensors("bundle", self.where, tensors, ("poses", "matches", "match_counts", "front_bits", "chain", "frame_points", "tracks_in", "refs", "tracks", "cams"))
        _check_records("bundle", "matches", matches, 12, "[n, match_cap, 3]")
        n, cap = matches.shape[0] if n_pairs is None else int(n_pairs), matches.shape[1]
        _check_sets("bundle", n, (matches,), (match_counts,), ((poses, n * 112), (chain, n * 176), (front_bits, n * ((cap + 63) // 64) * 8),
                                                               (frame_points, (n + 1) * int(point_cap) * 24), (tracks_in, n * cap * 48),
                                                               (refs, n * cap * 8), (cams_in, n * 160)))
        bo = _fill_out(BundleOut(), dict(tracks=tracks, cams=cams, point_info=point_info, member_bits=member_bits))
        prm = BundleParams(PoseParams(*(float(v) for v in intrinsics)), float(max_dist2), int(min_views), int(sweeps))
        self._chk(lib().vslam_bundle_dev(self._h, poses.data_ptr(), matches.data_ptr(), match_counts.data_ptr(), cap, front_bits.data_ptr(),
                                         int(point_cap), n, chain.data_ptr(), frame_points.data_ptr(), tracks_in.data_ptr(), refs.data_ptr(),
                                         None if cams_in is None else cams_in.data_ptr(), C.byref(prm), C.byref(bo)), "vslam_bundle_dev")

    def bundle_host(self, poses, matches, match_counts, front_bits, point_cap: int, chain, frame_points, tracks_in, refs, intrinsics,
                    max_dist2: float = 4.0, min_views: int = 2, sweeps: int = 4, cams_in=None, tracks=None, point_info=None, member_bits=None):
        """vslam_bundle_host: the same call over numpy arrays (the shapes of tracks_host; tracks_in [n, match_cap] TRACK_DTYPE, refs [n,
        match_cap] TRACK_REF_DTYPE, cams_in [n] BUNDLE_CAM_DTYPE or None) -> (tracks [n, match_cap] TRACK_DTYPE, cams [n] BUNDLE_CAM_DTYPE).
        tracks (default: a copy of tracks_in), point_info (BUNDLE_POINT_DTYPE [n, match_cap]) and member_bits (uint64 [n, 2, words]) are
        written in place when given (C-contiguous arrays of exactly that type)."""
        ps, mt, n, cap = _host_structure("bundle_host", poses, matches)
        words = (cap + 63) // 64
        cnt, fb, ch, fp = _counts(match_counts), _words(front_bits), _records(chain, CHAIN_DTYPE), _records(frame_points, POINT_DTYPE)
        ti, rf, ci = _records(tracks_in, TRACK_DTYPE), _records(refs, TRACK_REF_DTYPE), None if cams_in is None else _records(cams_in, BUNDLE_CAM_DTYPE)
        if (len(cnt) != n or fb.size != n * words or len(ch) != n or len(fp) != (n + 1) * int(point_cap) or len(ti) != n * cap or len(rf) != n * cap
                or (ci is not None and len(ci) != n)):
            raise ValueError("bundle_host: one count, one chain record, one camera and (match_cap + 63) // 64 words per pair, match_cap tracks and refs, "
                             "point_cap points per frame")
        if tracks is None:
            tracks = ti.reshape(n, cap).copy()
        _check_host_outs("bundle_host", (("tracks", tracks, TRACK_DTYPE, n * cap), ("point_info", point_info, BUNDLE_POINT_DTYPE, n * cap),
                                         ("member_bits", member_bits, np.uint64, n * 2 * words)))
        cams = np.zeros(max(n, 1), BUNDLE_CAM_DTYPE)
        bo = _fill_out(BundleOut(), dict(tracks=tracks, cams=cams, point_info=point_info, member_bits=member_bits))
        prm = BundleParams(PoseParams(*(float(v) for v in intrinsics)), float(max_dist2), int(min_views), int(sweeps))
        self._chk(lib().vslam_bundle_host(self._h, ps.ctypes.data, mt.ctypes.data, cnt.ctypes.data, cap, fb.ctypes.data, int(point_cap), n,
                                          ch.ctypes.data, fp.ctypes.data, ti.ctypes.data, rf.ctypes.data, None if ci is None else ci.ctypes.data,
                                          C.byref(prm), C.byref(bo)), "vslam_bundle_host")
        return tracks, cams[:n]

    def resect(self, poses, matches, match_counts, points, front_bits, point_cap: int, obs_matches, obs_counts, train_points, intrinsics,
               n_hypotheses: int = 512, seed: int = 0, max_dist2: float = 4.0, n_pairs: int | None = None, models=None, inlier_bits=None,
               hypotheses=None, correspondences=None, links=None):
        """vslam_resect_dev: the camera of frame j + 1 relative to frame j from the points pair j - 1 triangulated (the tensors
        chain() reads: poses, matches [n, match_cap, 3], match_counts, points, front_bits, point_cap) and their observations -
        obs_matches [n, obs_cap, 3] with obs_counts (any match list of the pairs: the same tensors, or match()'s raw list) and
        train_points [n, train_cap, 6]; intrinsics = (fx, fy, cx, cy).  Asynchronous on the context stream.  Outputs, CUDA tensors:
        models - any contiguous tensor of n_pairs * 120 bytes (RESECT_DTYPE after .cpu().numpy().view), inlier_bits [n, (obs_cap +
        63) // 64] 8-byte words, hypotheses n * n_hypotheses * 104 bytes (RESECT_HYP_DTYPE), correspondences n * obs_cap * 48 bytes
        (RESECT_CORR_DTYPE), links int32 [n, obs_cap]."""
        tensors = dict(poses=poses, matches=matches, match_counts=match_counts, points=points, front_bits=front_bits, obs_matches=obs_matches,
                       obs_counts=obs_counts, train_points=train_points, models=models, inlier_bits=inlier_bits, hypotheses=hypotheses,
                       correspondences=correspondences, links=links)
        _check_tensors("resect", self.where, tensors, ("poses", "matches", "match_counts", "points", "front_bits", "obs_matches", "obs_counts", "train_points", "models"))
        _check_records("resect", "matches", matches, 12, "[n, cap, 3]")
        _check_records("resect", "obs_matches", obs_matches, 12, "[n, cap, 3]")
        _check_records("resect", "train_points", train_points, 24, "[n, train_cap, 6]")
        n = matches.shape[0] if n_pairs is None else int(n_pairs)
        cap, ocap, tcap = matches.shape[1], obs_matches.shape[1], train_points.shape[1]
        _check_sets("resect", n, (matches, obs_matches, train_points), (match_counts, obs_counts),
                    ((poses, n * 112), (points, n * cap * 24), (front_bits, n * ((cap + 63) // 64) * 8)))
        ro = _fill_out(ResectOut(), dict(models=models, inlier_bits=inlier_bits, hypotheses=hypotheses, correspondences=correspondences, links=links))
        prm = ResectParams(int(n_hypotheses), int(seed) & 0xFFFFFFFF, float(max_dist2), PoseParams(*(float(v) for v in intrinsics)))
        self._chk(lib().vslam_resect_dev(self._h, poses.data_ptr(), matches.data_ptr(), match_counts.data_ptr(), cap, points.data_ptr(),
                                         front_bits.data_ptr(), int(point_cap), obs_matches.data_ptr(), obs_counts.data_ptr(), ocap,
                                         train_points.data_ptr(), tcap, n, C.byref(prm), C.byref(ro)), "vslam_resect_dev")

    def resect_host(self, poses, matches, match_counts, points, front_bits, point_cap: int, obs_matches, obs_counts, train_points, intrinsics,
                    n_hypotheses: int = 512, seed: int = 0, max_dist2: float = 4.0, inlier_bits=None, hypotheses=None, correspondences=None,
                    links=None):
        """vslam_resect_host: the same call over numpy arrays - poses [n] POSE_DTYPE, matches [n, match_cap] MATCH_DTYPE, match_counts
        [n], points float64 [n, match_cap, 3], front_bits uint64 [n, (match_cap + 63) // 64], obs_matches [n, obs_cap] MATCH_DTYPE,
        obs_counts [n], train_points [n, train_cap] POINT_DTYPE - -> models [n] RESECT_DTYPE.  inlier_bits uint64 [n, (obs_cap + 63) //
        64], hypotheses [n, n_hypotheses] RESECT_HYP_DTYPE, correspondences [n, obs_cap] RESECT_CORR_DTYPE and links int32 [n, obs_cap]
        are written in place when given (C-contiguous arrays of exactly that type); the rows the call leaves untouched keep their
        bytes."""
        ps = np.ascontiguousarray(poses, dtype=POSE_DTYPE).reshape(-1)
        mt, ob, tp = (np.ascontiguousarray(a, dtype=dt) for a, dt in ((matches, MATCH_DTYPE), (obs_matches, MATCH_DTYPE), (train_points, POINT_DTYPE)))
        n = len(ps)
        if any(a.ndim != 2 or a.shape[0] != n for a in (mt, ob, tp)):
            raise ValueError("resect_host: matches, obs_matches and train_points must be [n, capacity]")
        cap, ocap, tcap = mt.shape[1], ob.shape[1], tp.shape[1]
        cnt, ocnt, pts, fb = _counts(match_counts), _counts(obs_counts), np.ascontiguousarray(points, dtype=np.float64), _words(front_bits)
        if len(cnt) != n or len(ocnt) != n or pts.size != n * cap * 3 or fb.size != n * ((cap + 63) // 64):
            raise ValueError("resect_host: one count, match_cap points and (match_cap + 63) // 64 words per pair")
        outs = (("inlier_bits", inlier_bits, np.uint64, n * ((ocap + 63) // 64)), ("hypotheses", hypotheses, RESECT_HYP_DTYPE, n * int(n_hypotheses)),
                ("correspondences", correspondences, RESECT_CORR_DTYPE, n * ocap), ("links", links, np.int32, n * ocap))
        _check_host_outs("resect_host", outs)
        models = np.zeros(max(n, 1), RESECT_DTYPE)
        ro = _fill_out(ResectOut(), dict(models=models, inlier_bits=inlier_bits, hypotheses=hypotheses, correspondences=correspondences, links=links))
        prm = ResectParams(int(n_hypotheses), int(seed) & 0xFFFFFFFF, float(max_dist2), PoseParams(*(float(v) for v in intrinsics)))
        self._chk(lib().vslam_resect_host(self._h, ps.ctypes.data, mt.ctypes.data, cnt.ctypes.data, cap, pts.ctypes.data, fb.ctypes.data, int(point_cap),
                                          ob.ctypes.data, ocnt.ctypes.data, ocap, tp.ctypes.data, tcap, n, C.byref(prm), C.byref(ro)),
                  "vslam_resect_host")
        return models[:n]

    def resect_refine(self, models_in, correspondences, obs_cap: int, intrinsics, rounds: int = 4, max_dist2: float = 4.0, n_pairs: int | None = None,
                      models=None, info=None, inlier_bits=None):
        """vslam_resect_refine_dev: the Gauss-Newton refinement of every pair's resected pose over all its inliers, after resect();
        asynchronous on the context stream.  models_in: the tensor resect() wrote (n_pairs * 120 bytes); correspondences: the dense
        list of the same call (n_pairs * obs_cap * 48 bytes); intrinsics = (fx, fy, cx, cy).  Outputs, CUDA tensors: models n_pairs *
        120 bytes (may be models_in itself), info n_pairs * 32 bytes (RESECT_REFINE_DTYPE), inlier_bits [n, (obs_cap + 63) // 64]
        8-byte words, indexed by observation record like resect()'s, under the output pose."""
        tensors = dict(models_in=models_in, correspondences=correspondences, models=models, info=info, inlier_bits=inlier_bits)
        _check_tensors("resect_refine", self.where, tensors, ("models_in", "correspondences", "models"))
        n = _nbytes(models_in) // 120 if n_pairs is None else int(n_pairs)
        if _nbytes(models_in) < n * 120 or _nbytes(correspondences) < n * int(obs_cap) * 48:
            raise ValueError("resect_refine: models_in must hold n_pairs * 120 bytes, correspondences n_pairs * obs_cap * 48")
        ro = _fill_out(ResectRefineOut(), dict(models=models, info=info, inlier_bits=inlier_bits))
        prm = ResectRefineParams(int(rounds), float(max_dist2), PoseParams(*(float(v) for v in intrinsics)))
        self._chk(lib().vslam_resect_refine_dev(self._h, models_in.data_ptr(), correspondences.data_ptr(), int(obs_cap), n, C.byref(prm), C.byref(ro)),
                  "vslam_resect_refine_dev")

    def resect_refine_host(self, models_in, correspondences, intrinsics, rounds: int = 4, max_dist2: float = 4.0, inlier_bits=None):
        """vslam_resect_refine_host: the same call over numpy arrays - models_in [n] RESECT_DTYPE, correspondences [n, obs_cap]
        RESECT_CORR_DTYPE - -> (models [n] RESECT_DTYPE, info [n] RESECT_REFINE_DTYPE).  inlier_bits uint64 [n, (obs_cap + 63) // 64]
        is written in place when given; the words the call leaves untouched keep their bytes."""
        mi = np.ascontiguousarray(models_in, dtype=RESECT_DTYPE).reshape(-1)
        cs = np.ascontiguousarray(correspondences, dtype=RESECT_CORR_DTYPE)
        n = len(mi)
        if cs.ndim != 2 or cs.shape[0] != n:
            raise ValueError("resect_refine_host: correspondences must be [n, obs_cap]")
        ocap = cs.shape[1]
        words = n * ((ocap + 63) // 64)
        _check_host_outs("resect_refine_host", (("inlier_bits", inlier_bits, np.uint64, words),))
        models, info = np.zeros(max(n, 1), RESECT_DTYPE), np.zeros(max(n, 1), RESECT_REFINE_DTYPE)
        ro = _fill_out(ResectRefineOut(), dict(models=models, info=info, inlier_bits=inlier_bits))
        prm = ResectRefineParams(int(rounds), float(max_dist2), PoseParams(*(float(v) for v in intrinsics)))
        self._chk(lib().vslam_resect_refine_host(self._h, mi.ctypes.data, cs.ctypes.data, ocap, n, C.byref(prm), C.byref(ro)), "vslam_resect_refine_host")
        return models[:n], info[:n]

    def vocab_sample(self, sets: DescSets, vocab, vocab_defined, n_sets: int | None = None):
        """vslam_vocab_sample_dev: a vocabulary of K = vocab.shape[0] words copied from the rows of `sets` (desc_sets()) by the header's
        rule; asynchronous on the context stream.  vocab: float32 [K, 128], vocab_defined: uint8 [K], both outputs."""
        stage = "vocab_sample"
        _check_tensors(stage, self.where, dict(vocab=vocab, vocab_defined=vocab_defined), ("vocab", "vocab_defined"))
        if vocab.dim() != 2 or vocab.shape[1] != 128 or vocab.element_size() != 4:
            raise ValueError(f"{stage}: vocab must be float32 [K, 128]")
        if vocab_defined.element_size() != 1:
            raise ValueError(f"{stage}: vocab_defined must have 1-byte elements")
        n = sets.n if n_sets is None else int(n_sets)
        self._chk(lib().vslam_vocab_sample_dev(self._h, C.byref(sets), n, vocab.shape[0], vocab.data_ptr(), _nbytes(vocab), vocab_defined.data_ptr(),
                                               _nbytes(vocab_defined)), "vslam_vocab_sample_dev")

    def words(self, sets: DescSets, vocab, vocab_defined=None, n_sets: int | None = None, words=None, word_dist2=None, hist=None):
        """vslam_words_dev: the nearest word of every row of `sets` (desc_sets()) among the K = vocab.shape[0] rows of vocab (float32
        [K, 128]; vocab_defined uint8 [K] or None); asynchronous on the context stream.  words: int32 [n_sets, cap], word_dist2: float32
        [n_sets, cap], hist: int32 [n_sets, K] (written whole) - each optional, at least one."""
        stage = "words"
        outs = dict(words=words, word_dist2=word_dist2, hist=hist)
        _check_tensors(stage, self.where, dict(vocab=vocab, vocab_defined=vocab_defined, **outs), ("vocab",))
        if vocab.dim() != 2 or vocab.shape[1] != 128 or vocab.element_size() != 4:
            raise ValueError(f"{stage}: vocab must be float32 [K, 128]")
        K = vocab.shape[0]
        if vocab_defined is not None and (vocab_defined.element_size() != 1 or vocab_defined.numel() < K):
            raise ValueError(f"{stage}: vocab_defined must be uint8 [K]")
        for name, t in outs.items():
            if t is not None and t.element_size() != 4:
                raise ValueError(f"{stage}: {name} must have 4-byte elements")
        if words is None and word_dist2 is None and hist is None:
            raise ValueError(f"{stage}: no output requested")
        n = sets.n if n_sets is None else int(n_sets)
        _check_sets(stage, n, (), (), ((words, n * sets.cap * 4), (word_dist2, n * sets.cap * 4), (hist, n * K * 4)))
        wo = _fill_out(WordsOut(), outs)
        self._chk(lib().vslam_words_dev(self._h, C.byref(sets), n, vocab.data_ptr(), vocab_defined.data_ptr() if vocab_defined is not None else None,
                                        K, C.byref(wo)), "vslam_words_dev")

    def words_host(self, desc, counts, vocab, defined=None, vocab_defined=None, want_words: bool = True, want_dist2: bool = True,
                   want_hist: bool = True, fill: int = -1):
        """vslam_words_host: numpy desc [n_sets, cap, 128], counts [n_sets], vocab [K, 128] -> (words int32 [n_sets, cap], word_dist2
        float32 [n_sets, cap], hist uint32 [n_sets, K]); an output that is not wanted is None.  Rows past a set's count keep `fill`
        (words) and NaN (word_dist2)."""
        stage = "words_host"
        desc = np.ascontiguousarray(desc, dtype=np.float32)
        vocab = np.ascontiguousarray(vocab, dtype=np.float32).reshape(-1, 128)
        if desc.ndim != 3 or desc.shape[2] != 128:
            raise ValueError(f"{stage}: desc must be [n_sets, cap, 128]")
        n, cap, K = desc.shape[0], desc.shape[1], len(vocab)
        counts = _counts(counts)
        if len(counts) != n:
            raise ValueError(f"{stage}: one count per set")
        defined = None if defined is None else np.ascontiguousarray(defined, dtype=np.uint8)
        vocab_defined = None if vocab_defined is None else np.ascontiguousarray(vocab_defined, dtype=np.uint8)
        if (defined is not None and defined.size != n * cap) or (vocab_defined is not None and vocab_defined.size != K):
            raise ValueError(f"{stage}: defined must have one entry per descriptor row, vocab_defined one per word")
        words = np.full((n, cap), fill, np.int32) if want_words else None
        dist2 = np.full((n, cap), np.nan, np.float32) if want_dist2 else None
        hist = np.zeros((n, K), np.uint32) if want_hist else None
        wo = _fill_out(WordsOut(), dict(words=words, word_dist2=dist2, hist=hist))
        self._chk(lib().vslam_words_host(self._h, desc.ctypes.data, None if defined is None else defined.ctypes.data, counts.ctypes.data, cap, n,
                                         vocab.ctypes.data, None if vocab_defined is None else vocab_defined.ctypes.data, K, C.byref(wo)),
                  "vslam_words_host")
        return words, dist2, hist

    def vocab_kmeans(self, sets: DescSets, vocab_in, rounds: int, vocab_defined=None, n_sets: int | None = None, vocab=None, sizes=None,
                     report=None):
        """vslam_vocab_kmeans_dev: `rounds` rounds of Lloyd's algorithm over the rows of `sets` (desc_sets()) from the K = vocab_in.shape[0]
        words of vocab_in (float32 [K, 128]; vocab_defined uint8 [K] or None); asynchronous on the context stream.  vocab: float32
        [K, 128], the trained words (None: vocab_in itself, in place); sizes: int32 [K] and report: int32 [rounds, 4]
        (KMEANS_ROUND_DTYPE), each optional."""
        stage = "vocab_kmeans"
        vocab = vocab_in if vocab is None else vocab
        tensors = dict(vocab_in=vocab_in, vocab_defined=vocab_defined, vocab=vocab, sizes=sizes, report=report)
        _check_tensors(stage, self.where, tensors, ("vocab_in", "vocab"))
        for name in ("vocab_in", "vocab"):
            t = tensors[name]
            if t.dim() != 2 or t.shape[1] != 128 or t.element_size() != 4:
                raise ValueError(f"{stage}: {name} must be float32 [K, 128]")
        K = vocab_in.shape[0]
        if vocab.shape[0] != K:
            raise ValueError(f"{stage}: vocab must have vocab_in's K rows")
        if vocab_defined is not None and (vocab_defined.element_size() != 1 or vocab_defined.numel() < K):
            raise ValueError(f"{stage}: vocab_defined must be uint8 [K]")
        for name in ("sizes", "report"):
            if tensors[name] is not None and tensors[name].element_size() != 4:
                raise ValueError(f"{stage}: {name} must have 4-byte elements")
        n = sets.n if n_sets is None else int(n_sets)
        _check_sets(stage, n, (), (), ((sizes, K * 4), (report, int(rounds) * 16)))
        ko = _fill_out(KmeansOut(), dict(vocab=vocab, sizes=sizes, report=report))
        kp = KmeansParams(int(rounds), 0)
        self._chk(lib().vslam_vocab_kmeans_dev(self._h, C.byref(sets), n, vocab_in.data_ptr(), vocab_defined.data_ptr() if vocab_defined is not None else None,
                                               K, C.byref(kp), C.byref(ko)), "vslam_vocab_kmeans_dev")

    def vocab_kmeans_host(self, desc, counts, vocab_in, rounds: int, defined=None, vocab_defined=None, want_sizes: bool = True,
                          want_report: bool = True):
        """vslam_vocab_kmeans_host: numpy desc [n_sets, cap, 128], counts [n_sets], vocab_in [K, 128] -> (vocab float32 [K, 128], sizes
        uint32 [K], report KMEANS_ROUND_DTYPE [rounds]); an output that is not wanted is None."""
        stage = "vocab_kmeans_host"
        desc = np.ascontiguousarray(desc, dtype=np.float32)
        vocab_in = np.ascontiguousarray(vocab_in, dtype=np.float32).reshape(-1, 128)
        if desc.ndim != 3 or desc.shape[2] != 128:
            raise ValueError(f"{stage}: desc must be [n_sets, cap, 128]")
        n, cap, K = desc.shape[0], desc.shape[1], len(vocab_in)
        counts = _counts(counts)
        if len(counts) != n:
            raise ValueError(f"{stage}: one count per set")
        defined = None if defined is None else np.ascontiguousarray(defined, dtype=np.uint8)
        vocab_defined = None if vocab_defined is None else np.ascontiguousarray(vocab_defined, dtype=np.uint8)
        if (defined is not None and defined.size != n * cap) or (vocab_defined is not None and vocab_defined.size != K):
            raise ValueError(f"{stage}: defined must have one entry per descriptor row, vocab_defined one per word")
        vocab = np.zeros((K, 128), np.float32)
        sizes = np.zeros(K, np.uint32) if want_sizes else None
        report = np.zeros(max(int(rounds), 0), KMEANS_ROUND_DTYPE) if want_report else None
        ko = _fill_out(KmeansOut(), dict(vocab=vocab, sizes=sizes, report=report))
        kp = KmeansParams(int(rounds), 0)
        self._chk(lib().vslam_vocab_kmeans_host(self._h, desc.ctypes.data, None if defined is None else defined.ctypes.data, counts.ctypes.data, cap, n,
                                                vocab_in.ctypes.data, None if vocab_defined is None else vocab_defined.ctypes.data, K, C.byref(kp),
                                                C.byref(ko)), "vslam_vocab_kmeans_host")
        return vocab, sizes, report

    @staticmethod
    def _place_params(min_gap, max_candidates, num, den, min_score):
        return PlaceParams(int(min_gap), int(max_candidates), int(num), int(den), int(min_score), 0)

    def place(self, hist_q, hist_db=None, q_first: int = 0, db_first: int = 0, min_gap: int = 1, max_candidates: int = 3, num: int = 1, den: int = 5,
              min_score: int = 0, candidates=None, cand_counts=None, weights=None, self_q=None, self_db=None, scores=None):
        """vslam_place_dev: loop candidates of the frames q_first + i (hist_q int32 [nq, K]) among the frames db_first + j (hist_db
        [nd, K]; None: hist_q itself); asynchronous on the context stream.  candidates: int32 [nq, max_candidates, 3] (PLACE_CAND_DTYPE),
        cand_counts [nq], weights [K], self_q [nq], self_db [nd], scores [nq, nd]: each optional, candidates needs cand_counts."""
        stage = "place"
        hist_db = hist_q if hist_db is None else hist_db
        outs = dict(candidates=candidates, cand_counts=cand_counts, weights=weights, self_q=self_q, self_db=self_db, scores=scores)
        _check_tensors(stage, self.where, dict(hist_q=hist_q, hist_db=hist_db, **outs), ("hist_q", "hist_db"))
        for name, t in dict(hist_q=hist_q, hist_db=hist_db, **outs).items():
            if t is not None and t.element_size() != 4:
                raise ValueError(f"{stage}: {name} must have 4-byte elements")
        if hist_q.dim() != 2 or hist_db.dim() != 2 or hist_q.shape[1] != hist_db.shape[1]:
            raise ValueError(f"{stage}: hist_q and hist_db must be [frames, K] with one K")
        if all(t is None for t in outs.values()):
            raise ValueError(f"{stage}: no output requested")
        if candidates is not None and cand_counts is None:
            raise ValueError(f"{stage}: candidates needs cand_counts")
        nq, nd, K = hist_q.shape[0], hist_db.shape[0], hist_q.shape[1]
        po = _fill_out(PlaceOut(), outs)
        pp = self._place_params(min_gap, max_candidates, num, den, min_score)
        self._chk(lib().vslam_place_dev(self._h, hist_q.data_ptr(), nq, int(q_first), hist_db.data_ptr(), nd, int(db_first), K, C.byref(pp), C.byref(po)),
                  "vslam_place_dev")

    def place_host(self, hist_q, hist_db=None, q_first: int = 0, db_first: int = 0, min_gap: int = 1, max_candidates: int = 3, num: int = 1,
                   den: int = 5, min_score: int = 0, want_scores: bool = True, fill: int = -1):
        """vslam_place_host over numpy histograms [frames, K] -> dict(candidates [nq, c] PLACE_CAND_DTYPE, cand_counts, weights, self_q,
        self_db, scores (None unless want_scores)).  Candidate slots past a frame's count keep `fill` in every field's bytes."""
        stage = "place_host"
        hq = np.ascontiguousarray(hist_q).astype(np.uint32, copy=False)
        hd = hq if hist_db is None else np.ascontiguousarray(hist_db).astype(np.uint32, copy=False)
        if hq.ndim != 2 or hd.ndim != 2 or hq.shape[1] != hd.shape[1]:
            raise ValueError(f"{stage}: hist_q and hist_db must be [frames, K] with one K")
        nq, nd, K = hq.shape[0], hd.shape[0], hq.shape[1]
        c = int(max_candidates)
        r = dict(candidates=np.full((nq, max(c, 0), 3), fill, np.int32).view(PLACE_CAND_DTYPE).reshape(nq, max(c, 0)),
                 cand_counts=np.zeros(nq, np.uint32), weights=np.zeros(K, np.uint32), self_q=np.zeros(nq, np.uint32), self_db=np.zeros(nd, np.uint32),
                 scores=np.zeros((nq, nd), np.uint32) if want_scores else None)
        po = _fill_out(PlaceOut(), r)
        pp = self._place_params(min_gap, max_candidates, num, den, min_score)
        self._chk(lib().vslam_place_host(self._h, _ptr(hq), nq, int(q_first), _ptr(hd), nd, int(db_first), K, C.byref(pp), C.byref(po)),
                  "vslam_place_host")
        return r

    # ---- loop verification: the defaults of min_inliers and num / den are the ones DESIGN 5.28 measures
    LOOP_MIN_INLIERS, LOOP_NUM, LOOP_DEN = 12, 2, 5

    def loop_pairs(self, candidates, cand_counts, pairs, db_first: int = 0, nd: int | None = None):
        """vslam_loop_pairs_dev: the pair table of place()'s outputs; asynchronous on the context stream.  candidates: int32
        [nq, c, 3], cand_counts: int32 [nq], pairs: int32 [nq * c, 2] (SET_PAIR_DTYPE), written whole.  nd: the database frames
        (None: nq, a batch searched in itself)."""
        stage = "loop_pairs"
        _check_tensors(stage, self.where, dict(candidates=candidates, cand_counts=cand_counts, pairs=pairs), ("candidates", "cand_counts", "pairs"))
        if candidates.dim() != 3 or candidates.shape[2] * candidates.element_size() != 12:
            raise ValueError(f"{stage}: candidates must be [nq, c, 3] 4-byte elements")
        nq, c = candidates.shape[0], candidates.shape[1]
        _check_sets(stage, nq, (), (cand_counts,), ())
        self._chk(lib().vslam_loop_pairs_dev(self._h, candidates.data_ptr(), cand_counts.data_ptr(), nq, c, int(db_first), nq if nd is None else int(nd),
                                             pairs.data_ptr(), _nbytes(pairs)), "vslam_loop_pairs_dev")

    def match_pairs(self, query: DescSets, train: DescSets, pairs, n_pairs: int | None = None, ratio2: float = 0.64, same_octave: bool = False,
                    nn=None, matches=None, match_counts=None, n_query_sets: int | None = None, n_train_sets: int | None = None):
        """vslam_match_pairs_dev: slot p of `pairs` (int32 [n_pairs, 2], SET_PAIR_DTYPE) matches set pairs[p].query_set of `query`
        against set pairs[p].train_set of `train` (desc_sets(); the two may be one buffer); asynchronous on the context stream.
        nn, matches, match_counts as match()'s, indexed by the slot."""
        stage = "match_pairs"
        outs = dict(nn=nn, matches=matches, match_counts=match_counts)
        _check_tensors(stage, self.where, dict(pairs=pairs, **outs), ("pairs",))
        for name, t in dict(pairs=pairs, **outs).items():
            if t is not None and t.element_size() != 4:
                raise ValueError(f"{stage}: {name} must have 4-byte elements")
        n = pairs.numel() // 2 if n_pairs is None else int(n_pairs)
        if pairs.numel() < 2 * n:
            raise ValueError(f"{stage}: fewer slots than pairs")
        mo = _fill_out(MatchOut(), outs)
        if matches is not None:
            mo.match_cap = matches.shape[1]
        self._chk(lib().vslam_match_pairs_dev(self._h, C.byref(query), query.n if n_query_sets is None else int(n_query_sets), C.byref(train),
                                              train.n if n_train_sets is None else int(n_train_sets), pairs.data_ptr(), n, float(ratio2),
                                              int(bool(same_octave)), C.byref(mo)), "vslam_match_pairs_dev")

    def match_pairs_host(self, query, query_counts, train, train_counts, pairs, ratio2: float = 0.64, same_octave: bool = False, query_defined=None,
                         train_defined=None, query_points=None, train_points=None, match_cap: int | None = None, nn=None, matches=None):
        """vslam_match_pairs_host over numpy arrays: query [nqs, qcap, 128], train [nts, tcap, 128] (may be the same array), counts [n],
        defined [n, cap] / points [n, cap] (POINT_DTYPE) or None, pairs SET_PAIR_DTYPE [n_pairs] -> (nn [n_pairs, qcap] NN2_DTYPE,
        matches [n_pairs, match_cap] MATCH_DTYPE, match_counts [n_pairs]).  nn / matches: arrays whose bytes the untouched rows keep
        (None: zeros)."""
        stage = "match_pairs_host"
        same = train is query
        q = np.ascontiguousarray(query, dtype=np.float32)
        t = q if same else np.ascontiguousarray(train, dtype=np.float32)
        if q.ndim != 3 or t.ndim != 3 or q.shape[2] != 128 or t.shape[2] != 128:
            raise ValueError(f"{stage}: query and train must be [n_sets, cap, 128]")
        pr = _records(pairs, SET_PAIR_DTYPE)
        qc = _counts(query_counts)
        tc = qc if same else _counts(train_counts)
        if len(qc) != q.shape[0] or len(tc) != t.shape[0]:
            raise ValueError(f"{stage}: one count per set")
        opt = [None if a is None else np.ascontiguousarray(a, dtype=dt) for a, dt in
               ((query_defined, np.uint8), (query_points, POINT_DTYPE), (train_defined, np.uint8), (train_points, POINT_DTYPE))]
        for a, rows in zip(opt, (q.shape[0] * q.shape[1],) * 2 + (t.shape[0] * t.shape[1],) * 2):
            if a is not None and a.size != rows:
                raise ValueError(f"{stage}: defined / points must have one entry per descriptor row")
        cap = max(q.shape[1], 1) if match_cap is None else int(match_cap)
        n = len(pr)
        nn = np.zeros((n, q.shape[1]), NN2_DTYPE) if nn is None else nn
        matches = np.zeros((n, cap), MATCH_DTYPE) if matches is None else matches
        _check_host_outs(stage, (("nn", nn, NN2_DTYPE, n * q.shape[1]), ("matches", matches, MATCH_DTYPE, n * cap)))
        counts = np.zeros(n, np.uint32)
        mo = _fill_out(MatchOut(), dict(nn=nn, matches=matches, match_counts=counts))
        mo.match_cap = cap
        Q = DescSets(q.ctypes.data, _ptr(opt[0]), _ptr(opt[1]), qc.ctypes.data, q.shape[1])
        T = DescSets(t.ctypes.data, _ptr(opt[2]), _ptr(opt[3]), tc.ctypes.data, t.shape[1])
        self._chk(lib().vslam_match_pairs_host(self._h, C.byref(Q), q.shape[0], C.byref(T), t.shape[0], pr.ctypes.data, n, float(ratio2),
                                               int(bool(same_octave)), C.byref(mo)), "vslam_match_pairs_host")
        return nn, matches, counts

    def pair_points(self, matches, match_counts, pairs, query_points, train_points, query_points_out, train_points_out, local,
                    n_pairs: int | None = None):
        """vslam_pair_points_dev: the points of every matched record of every slot, gathered so that epipolar(local, match_counts,
        query_points_out, train_points_out) and the stages after it run on the slots; asynchronous on the context stream.  matches
        [n_pairs, match_cap, 3], match_counts int32 [n_pairs], pairs int32 [n_pairs, 2], query_points / train_points int32 [n_sets, cap, 6];
        outputs: query_points_out / train_points_out int32 [n_pairs, match_cap, 6], local [n_pairs, match_cap, 3]."""
        stage = "pair_points"
        t = dict(matches=matches, match_counts=match_counts, pairs=pairs, query_points=query_points, train_points=train_points,
                 query_points_out=query_points_out, train_points_out=train_points_out, local=local)
        _check_tensors(stage, self.where, t, tuple(t))
        _check_records(stage, "matches", matches, 12, "[n, match_cap, 3]")
        _check_records(stage, "query_points", query_points, 24, "[n, cap, 6]")
        _check_records(stage, "train_points", train_points, 24, "[n, cap, 6]")
        n = matches.shape[0] if n_pairs is None else int(n_pairs)
        _check_sets(stage, n, (matches,), (match_counts,), ((pairs, n * 8),))
        self._chk(lib().vslam_pair_points_dev(self._h, matches.data_ptr(), match_counts.data_ptr(), matches.shape[1], pairs.data_ptr(), n,
                                              query_points.data_ptr(), query_points.shape[1], query_points.shape[0], train_points.data_ptr(),
                                              train_points.shape[1], train_points.shape[0], query_points_out.data_ptr(), _nbytes(query_points_out),
                                              train_points_out.data_ptr(), _nbytes(train_points_out), local.data_ptr(), _nbytes(local)),
                  "vslam_pair_points_dev")

    def loop_verdict(self, models, pairs, nq: int, c: int, n_train_sets: int, min_inliers: int | None = None, num: int | None = None,
                     den: int | None = None, loops=None, loop_list=None, n_loops=None):
        """vslam_loop_verdict_dev: the verified loop of each of nq query frames from the models of its c slots (models: nq * c * 88
        bytes as epipolar() wrote them, pairs int32 [nq * c, 2]); asynchronous on the context stream.  loops: int32 [nq, 5] (LOOP_DTYPE),
        loop_list: int32 [nq], n_loops: int32 [1] - each optional, loop_list needs n_loops."""
        stage = "loop_verdict"
        outs = dict(loops=loops, loop_list=loop_list, n_loops=n_loops)
        _check_tensors(stage, self.where, dict(models=models, pairs=pairs, **outs), ("models", "pairs"))
        if all(t is None for t in outs.values()):
            raise ValueError(f"{stage}: no output requested")
        if loop_list is not None and n_loops is None:
            raise ValueError(f"{stage}: loop_list needs n_loops")
        _check_sets(stage, 0, (), (), ((models, nq * c * 88), (pairs, nq * c * 8)))
        lp = self._loop_params(min_inliers, num, den)
        lo = _fill_out(LoopOut(), outs)
        self._chk(lib().vslam_loop_verdict_dev(self._h, models.data_ptr(), pairs.data_ptr(), int(nq), int(c), int(n_train_sets), C.byref(lp), C.byref(lo)),
                  "vslam_loop_verdict_dev")

    @classmethod
    def _loop_params(cls, min_inliers, num, den):
        return LoopParams(cls.LOOP_MIN_INLIERS if min_inliers is None else int(min_inliers), cls.LOOP_NUM if num is None else int(num),
                          cls.LOOP_DEN if den is None else int(den), 0)

    def loop_verdict_host(self, models, pairs, c: int, n_train_sets: int, min_inliers: int | None = None, num: int | None = None,
                          den: int | None = None, fill: int = -1):
        """vslam_loop_verdict_host over numpy records: models EPIPOLAR_DTYPE [nq * c], pairs SET_PAIR_DTYPE [nq * c] -> (loops LOOP_DTYPE
        [nq], loop_list int32 [nq] whose entries past n_loops keep `fill`, n_loops)."""
        stage = "loop_verdict_host"
        md, pr = _records(models, EPIPOLAR_DTYPE), _records(pairs, SET_PAIR_DTYPE)
        c = int(c)
        if c < 1 or len(md) != len(pr) or len(pr) % c:
            raise ValueError(f"{stage}: models and pairs must be [nq * c]")
        nq = len(pr) // c
        loops, lst, n = np.zeros(nq, LOOP_DTYPE), np.full(nq, fill, np.int32), np.zeros(1, np.uint32)
        lp = self._loop_params(min_inliers, num, den)
        lo = _fill_out(LoopOut(), dict(loops=loops, loop_list=lst, n_loops=n))
        self._chk(lib().vslam_loop_verdict_host(self._h, md.ctypes.data if nq else loops.ctypes.data, pr.ctypes.data if nq else loops.ctypes.data, nq, c,
                                                int(n_train_sets), C.byref(lp), C.byref(lo)), "vslam_loop_verdict_host")
        return loops, lst, int(n[0])

    def frame_world(self, poses, matches, match_counts, front_bits, point_cap: int, chain, cams, index, n_pairs: int | None = None):
        """vslam_frame_world_dev: the output of chain() seen per frame - cams, any contiguous tensor of (n + 1) * 112 bytes
        (FRAME_CAM_DTYPE after .cpu().numpy().view), and index int32 [n + 1, point_cap], the lowest live record of a frame's source
        pair per feature or -1; asynchronous on the context stream.  poses, matches [n, match_cap, 3], match_counts, front_bits and
        point_cap are what chain() read, chain the tensor it wrote (n * 176 bytes).  The world point of feature k of frame f is
        map[cams[f].pair][index[f][k]] of chain()'s map."""
        stage = "frame_world"
        tensors = dict(poses=poses, matches=matches, match_counts=match_counts, front_bits=front_bits, chain=chain, cams=cams, index=index)
        _check_tensors(stage, self.where, tensors, tuple(tensors))
        _check_records(stage, "matches", matches, 12, "[n, match_cap, 3]")
        n, cap = matches.shape[0] if n_pairs is None else int(n_pairs), matches.shape[1]
        nf = n + 1 if n else 0
        _check_sets(stage, n, (matches,), (match_counts,), ((poses, n * 112), (front_bits, n * ((cap + 63) // 64) * 8), (chain, n * 176),
                                                              (cams, nf * 112), (index, nf * int(point_cap) * 4)))
        fo = _fill_out(FrameWorldOut(), dict(cams=cams, index=index))
        self._chk(lib().vslam_frame_world_dev(self._h, poses.data_ptr(), matches.data_ptr(), match_counts.data_ptr(), cap, front_bits.data_ptr(),
                                              int(point_cap), chain.data_ptr(), n, C.byref(fo)), "vslam_frame_world_dev")

    def frame_world_host(self, poses, matches, match_counts, front_bits, point_cap: int, chain):
        """vslam_frame_world_host: the same call over numpy arrays - poses [n] POSE_DTYPE, matches [n, match_cap] MATCH_DTYPE,
        match_counts [n], front_bits uint64 [n, (match_cap + 63) // 64], chain [n] CHAIN_DTYPE - -> (cams [n + 1] FRAME_CAM_DTYPE, index
        int32 [n + 1, point_cap]); both empty for n == 0."""
        ps, mt, n, cap = _host_structure("frame_world_host", poses, matches)
        cnt, fb, ch = _counts(match_counts), _words(front_bits), _records(chain, CHAIN_DTYPE)
        if len(cnt) != n or fb.size != n * ((cap + 63) // 64) or len(ch) != n:
            raise ValueError("frame_world_host: one count, one chain record and (match_cap + 63) // 64 words per pair")
        nf = n + 1 if n else 0
        cams, index = np.zeros(max(nf, 1), FRAME_CAM_DTYPE), np.full((max(nf, 1), int(point_cap)), -1, np.int32)
        fo = _fill_out(FrameWorldOut(), dict(cams=cams, index=index))
        self._chk(lib().vslam_frame_world_host(self._h, ps.ctypes.data, mt.ctypes.data, cnt.ctypes.data, cap, fb.ctypes.data, int(point_cap),
                                               ch.ctypes.data, n, C.byref(fo)), "vslam_frame_world_host")
        return cams[:nf], index[:nf]

    def sim3(self, query: Sim3Side, train: Sim3Side, pairs, matches, match_counts, intrinsics, select_bits=None, n_hypotheses: int = 512,
             seed: int = 0, max_dist2: float = SIM3_MAX_DIST2, n_pairs: int | None = None, models=None, inlier_bits=None, hypotheses=None,
             correspondences=None, links=None):
        """vslam_sim3_dev: one similarity (s, R, t), y_train_world = s R x_query_world + t, per slot of a set-pair table, by RANSAC
        over the 3-D points the two frames of a slot have in their own world frames; asynchronous on the context stream.  query and
        train: sim3_side() of each end (the same object for loops inside one run); pairs int32 [n, 2]; matches [n, match_cap, 3] and
        match_counts as match_pairs() wrote them; select_bits [n, (match_cap + 63) // 64] 8-byte words, optional (epipolar()'s
        inlier_bits over pair_points()'s local list); intrinsics = (fx, fy, cx, cy).  Outputs, CUDA tensors: models - any contiguous
        tensor of n * 136 bytes (SIM3_DTYPE after .cpu().numpy().view), inlier_bits [n, (match_cap + 63) // 64] 8-byte words,
        hypotheses n * n_hypotheses * 112 bytes (SIM3_HYP_DTYPE), correspondences n * match_cap * 88 bytes (SIM3_CORR_DTYPE), links
        int32 [n, match_cap, 2]."""
        stage = "sim3"
        tensors = dict(pairs=pairs, matches=matches, match_counts=match_counts, select_bits=select_bits, models=models, inlier_bits=inlier_bits,
                       hypotheses=hypotheses, correspondences=correspondences, links=links)
        _check_tensors(stage, self.where, tensors, ("pairs", "matches", "match_counts", "models"))
        _check_records(stage, "matches", matches, 12, "[n, match_cap, 3]")
        n, cap = matches.shape[0] if n_pairs is None else int(n_pairs), matches.shape[1]
        _check_sets(stage, n, (matches,), (match_counts,), ((pairs, n * 8), (select_bits, n * ((cap + 63) // 64) * 8)))
        so = _fill_out(Sim3Out(), dict(models=models, inlier_bits=inlier_bits, hypotheses=hypotheses, correspondences=correspondences, links=links))
        prm = Sim3Params(int(n_hypotheses), int(seed) & 0xFFFFFFFF, float(max_dist2), PoseParams(*(float(v) for v in intrinsics)))
        self._chk(lib().vslam_sim3_dev(self._h, C.byref(query), C.byref(train), pairs.data_ptr(), matches.data_ptr(), match_counts.data_ptr(), cap,
                                       None if select_bits is None else select_bits.data_ptr(), n, C.byref(prm), C.byref(so)), "vslam_sim3_dev")

    def sim3_host(self, query, train, pairs, matches, match_counts, intrinsics, select_bits=None, n_hypotheses: int = 512, seed: int = 0,
                  max_dist2: float = SIM3_MAX_DIST2, inlier_bits=None, hypotheses=None, correspondences=None, links=None):
        """vslam_sim3_host: the same call over numpy arrays.  query and train: dicts of cams [nf] FRAME_CAM_DTYPE, index int32 [nf,
        point_cap], map float64 [n_map_pairs, map_cap, 3] and points [nf, points_cap] POINT_DTYPE (one dict for both: the side goes up
        once); pairs [n] SET_PAIR_DTYPE, matches [n, match_cap] MATCH_DTYPE, match_counts [n], select_bits uint64 [n, (match_cap + 63)
        // 64] or None -> models [n] SIM3_DTYPE.  inlier_bits uint64 [n, words], hypotheses [n, n_hypotheses] SIM3_HYP_DTYPE,
        correspondences [n, match_cap] SIM3_CORR_DTYPE and links int32 [n, match_cap, 2] are written in place when given (C-contiguous
        arrays of exactly that type); the rows the call leaves untouched keep their bytes."""
        stage = "sim3_host"
        keep = []
        sq = _host_sim3_side(stage, query, keep)
        st = sq if train is query else _host_sim3_side(stage, train, keep)
        pr, mt = _records(pairs, SET_PAIR_DTYPE), np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        n = len(pr)
        if mt.ndim != 2 or mt.shape[0] != n:
            raise ValueError(f"{stage}: matches must be [n, match_cap]")
        cap, cnt = mt.shape[1], _counts(match_counts)
        words = (cap + 63) // 64
        sel = None if select_bits is None else _words(select_bits)
        if len(cnt) != n or (sel is not None and sel.size != n * words):
            raise ValueError(f"{stage}: one count and (match_cap + 63) // 64 select words per slot")
        outs = (("inlier_bits", inlier_bits, np.uint64, n * words), ("hypotheses", hypotheses, SIM3_HYP_DTYPE, n * int(n_hypotheses)),
                ("correspondences", correspondences, SIM3_CORR_DTYPE, n * cap), ("links", links, np.int32, n * cap * 2))
        _check_host_outs(stage, outs)
        models = np.zeros(max(n, 1), SIM3_DTYPE)
        so = _fill_out(Sim3Out(), dict(models=models, inlier_bits=inlier_bits, hypotheses=hypotheses, correspondences=correspondences, links=links))
        prm = Sim3Params(int(n_hypotheses), int(seed) & 0xFFFFFFFF, float(max_dist2), PoseParams(*(float(v) for v in intrinsics)))
        at = lambda a: a.ctypes.data if a.size else models.ctypes.data  # (no slots: a pointer that is never followed)
        self._chk(lib().vslam_sim3_host(self._h, C.byref(sq), C.byref(st), at(pr), at(mt), at(cnt), cap, None if sel is None else sel.ctypes.data, n,
                                        C.byref(prm), C.byref(so)), "vslam_sim3_host")
        return models[:n]

    def kernel_timing_enable(self, name: str | None):
        self._chk(lib().vslam_kernel_timing_enable(self._h, name.encode() if name else None), "vslam_kernel_timing_enable")

    def kernel_timing_read(self):
        n, ms = C.c_int(), C.c_double()
        self._chk(lib().vslam_kernel_timing_read(self._h, C.byref(n), C.byref(ms)), "vslam_kernel_timing_read")
        return n.value, ms.value


class Pyramid:
    """vslam_pyramid: the Gaussian / DoG stacks of one image, resident in HBM."""

    def __init__(self, ctx: Context, img, n_octaves: int = 4, sigma0: float = 1.6):
        img = _u8(img)
        self.ctx = ctx
        h = C.c_void_p()
        ctx._chk(lib().vslam_pyramid_build_u8(ctx._h, img.ctypes.data, *img.shape, img.strides[0], n_octaves, float(sigma0), C.byref(h)), "vslam_pyramid_build_u8")
        self._h = h
        ctx._pyramids.add(self)
        info = PyramidInfo()
        lib().vslam_pyramid_get_info(h, C.byref(info))
        self.n_octaves = info.n_octaves
        self.sizes = [(info.rows[o], info.cols[o]) for o in range(info.n_octaves)]
        self.sigmas = [[info.sigma[o][l] for l in range(NUM_LEVELS)] for o in range(info.n_octaves)]
        self.ksizes = [[info.ksize[o][l] for l in range(NUM_LEVELS)] for o in range(info.n_octaves)]

    def _get(self, fn, what, o, *lvl):
        if not 0 <= o < self.n_octaves:
            out = np.empty((1, 1), np.uint8)
        else:
            out = np.empty(self.sizes[o], np.uint8)
        self.ctx._chk(fn(self._h, o, *lvl, out.ctypes.data, out.strides[0]), what)
        return out

    def base(self, o):
        return self._get(lib().vslam_pyramid_get_base, "vslam_pyramid_get_base", o)

    def gauss(self, o, l):
        return self._get(lib().vslam_pyramid_get_gauss, "vslam_pyramid_get_gauss", o, l)

    def dog(self, o, l):
        return self._get(lib().vslam_pyramid_get_dog, "vslam_pyramid_get_dog", o, l)

    def gradients(self, o, l):
        """(grad_x, grad_y, magnitude, orientation[deg]) of Gaussian level (o, l), computed on demand."""
        shape = self.sizes[o] if 0 <= o < self.n_octaves else (1, 1)
        outs = [np.empty(shape, np.float32) for _ in range(4)]
        self.ctx._chk(lib().vslam_pyramid_get_gradients(self._h, o, l, *[a.ctypes.data for a in outs], outs[0].strides[0]), "vslam_pyramid_get_gradients")
        return tuple(outs)

    def extrema(self, octave: int, window: int = 3, min_contrast: int = 8, cap: int = 1 << 22):
        """(mask[3, lat_rows, lat_cols] u8 unpacked from the bitmask, points, total count)."""
        lr, lc = extrema_lattice(*self.sizes[octave], window) if 0 <= octave < self.n_octaves else (0, 0)
        wpr = (lc + 63) // 64
        bits = np.zeros((3, lr, max(wpr, 1)), np.uint64)
        pts = np.zeros(cap, POINT_DTYPE)
        n = C.c_size_t()
        self.ctx._chk(lib().vslam_dog_extrema(self.ctx._h, self._h, octave, window, min_contrast, bits.ctypes.data, pts.ctypes.data, cap, C.byref(n)), "vslam_dog_extrema")
        mask = np.unpackbits(bits.view(np.uint8), axis=-1, bitorder="little")[..., :lc] if lc else np.zeros((3, lr, 0), np.uint8)
        return mask, pts[: min(n.value, cap)], n.value

    def extrema_dense(self, octave: int, min_contrast: int = 8, cap: int = 1 << 22):
        """Extension: dense 3x3x3 test on every pixel; (mask[3, rows, cols] u8, points, total count)."""
        r, c = self.sizes[octave] if 0 <= octave < self.n_octaves else (0, 0)
        wpr = (c + 63) // 64
        bits = np.zeros((3, r, max(wpr, 1)), np.uint64)
        pts = np.zeros(cap, POINT_DTYPE)
        n = C.c_size_t()
        self.ctx._chk(lib().vslam_dog_extrema_dense(self.ctx._h, self._h, octave, min_contrast, bits.ctypes.data, pts.ctypes.data, cap, C.byref(n)), "vslam_dog_extrema_dense")
        mask = np.unpackbits(bits.view(np.uint8), axis=-1, bitorder="little")[..., :c] if c else np.zeros((3, r, 0), np.uint8)
        return mask, pts[: min(n.value, cap)], n.value

    def keypoints(self, octave: int, window: int = 3, cap: int = 1 << 22):
        """initialKeypointDetection incl. FeaturePointLocalization: (points, total count)."""
        pts = np.zeros(cap, POINT_DTYPE)
        n = C.c_size_t()
        self.ctx._chk(lib().vslam_dog_keypoints(self.ctx._h, self._h, octave, window, pts.ctypes.data, cap, C.byref(n)), "vslam_dog_keypoints")
        return pts[: min(n.value, cap)], n.value

    def filter_keypoints(self, octave: int, kps, cap: int = 1 << 22):
        """filterKeypoints for one octave: (oriented points, total count)."""
        kps = np.ascontiguousarray(kps, dtype=POINT_DTYPE)
        out = np.zeros(cap, POINT_DTYPE)
        n = C.c_size_t()
        self.ctx._chk(lib().vslam_filter_keypoints(self.ctx._h, self._h, octave, kps.ctypes.data, len(kps), out.ctypes.data, cap, C.byref(n)), "vslam_filter_keypoints")
        return out[: min(n.value, cap)], n.value

    def sift_descriptors(self, octave: int, oriented):
        """SIFT() for one octave's oriented keypoints: (desc f32 [n, 128], defined bool [n])."""
        kps = np.ascontiguousarray(oriented, dtype=POINT_DTYPE)
        desc = np.zeros((len(kps), 128), np.float32)
        ok = np.zeros(max(len(kps), 1), np.uint8)
        self.ctx._chk(lib().vslam_sift_descriptors(self.ctx._h, self._h, octave, kps.ctypes.data, len(kps), desc.ctypes.data, ok.ctypes.data), "vslam_sift_descriptors")
        return desc, ok[: len(kps)].astype(bool)

    def close(self):
        if getattr(self, "_h", None):
            lib().vslam_pyramid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
