"""ctypes binding of liballwave_hip.so (include/allwave_hip.h).

This is the product path: it never imports oracle/ and has no CPU fallback -- a missing library
or a missing GPU raises immediately.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AWV_HIP_LIB") or os.path.join(_HERE, "liballwave_hip.so")

AWV_OK = 0
AWV_ERR_NO_DEVICE = -1
AWV_ERR_ARG = -3
AWV_ERR_STATE = -6
AWV_ERR_SINK = -7
AWV_ST_COMPLETED = 0
AWV_ST_CAPACITY = 1
AWV_ST_ABOVE_BOUND = 4
AWV_F_KEEP_ON_DEVICE = 1
AWV_F_FORCE_INT32 = 2
AWV_F_NO_PACKED_SEQ = 4
AWV_F_ONE_WAVE = 8
AWV_F_FOUR_WAVES = 16
AWV_F_NO_ARENA_PROBE = 32
AWV_F_SINGLE_STEP = 64
AWV_F_NO_CHAIN = 128
AWV_F_NO_WIDE16 = 256
AWV_F_NO_DEEP = 512
AWV_F_NO_RERUN = 1024
AWV_F_NO_TWIN = 2048
AWV_F_TWIN_TOP_ONLY = 4096
AWV_F_NO_TWIN_BASE = 8192
AWV_F_NO_ROW_REUSE = 16384
AWV_F_ROW_REUSE_LEVEL1 = 32768
#: WFA orientation (awv_orient_pairs / awv_orient_decide)
AWV_ORIENT_FORWARD = 0
AWV_ORIENT_REVERSE = 1
AWV_ORIENT_UNDECIDED = 2
AWV_ORIENT_BY_BOUND = 0
AWV_ORIENT_BY_EDITS = 1
AWV_ORIENT_FULL = 1
AWV_ORIENT_SKIP_RATIO = 8
AWV_ORIENT_NO_EDITS = 2 ** 64 - 1
AWV_ORIENT_HI_NONE = 2 ** 31 - 1
#: verification (awv_verify_result.code), in order of precedence
AWV_VF_OK = 0
AWV_VF_SKIPPED = 1
AWV_VF_BAD_OP = 2
AWV_VF_OVERRUN = 3
AWV_VF_M_DIFFERS = 4
AWV_VF_X_EQUAL = 5
AWV_VF_SHORT = 6
AWV_VF_COUNTS = 7
AWV_VF_PENALTY = 8
#: clipping (awv_clip_result.code)
AWV_CL_OK = 0
AWV_CL_SKIPPED = 1
AWV_CL_EMPTY = 2
AWV_CL_BAD_OP = 3
AWV_CLIP_MAX_BONUS = 32767
#: normalization: the engine's mode / a call's direction, and awv_norm_result.code
AWV_NORM_OFF = 0
AWV_NORM_LEFT = 1
AWV_NORM_RIGHT = 2
AWV_NM_OK = 0
AWV_NM_SKIPPED = 1
AWV_NM_BAD_OP = 2
AWV_NM_LENGTHS = 3
#: the cs difference string: a call's mode, and awv_cs_text.code
AWV_CS_SHORT = 1
AWV_CS_LONG = 2
AWV_CST_OK = 0
AWV_CST_SKIPPED = 1
AWV_CST_BAD_OP = 2
AWV_CST_LENGTHS = 3
#: per-base depth: the roles whose tracks a column is added to, and awv_cov_item.code
AWV_COV_TARGET = 1
AWV_COV_QUERY = 2
AWV_COV_BOTH = 3
AWV_CV_OK = 0
AWV_CV_SKIPPED = 1
AWV_CV_BAD_OP = 2
AWV_CV_LENGTHS = 3
#: the allele table: awv_variant.type, awv_var_item.code and the hash (base and modulus are part of the contract)
AWV_VAR_SNV = 0
AWV_VAR_DEL = 1
AWV_VAR_INS = 2
AWV_VAR_HASH_BASE = 0x1b873593a5c1f2e7
AWV_VAR_HASH_MOD = (1 << 61) - 1
AWV_VR_OK = 0
AWV_VR_SKIPPED = 1
AWV_VR_BAD_OP = 2
AWV_VR_LENGTHS = 3
#: `fold` of awv_variants_cigars: the unfolded events, the call's folded table, or into the engine's table
AWV_VTAB_EVENTS = 0
AWV_VTAB_FOLDED = 1
AWV_VTAB_ACCUMULATE = 2
#: liftover: the side a region lies on (a mask of both for lift_begin), awv_lift_result.code and awv_lift_row.flags
AWV_LIFT_FROM_TARGET = 1
AWV_LIFT_FROM_QUERY = 2
AWV_LIFT_FROM_BOTH = 3
AWV_LF_OK = 0
AWV_LF_SKIPPED = 1
AWV_LF_BAD_OP = 2
AWV_LF_LENGTHS = 3
AWV_LF_UNALIGNED = 4
AWV_LF_OUTSIDE = 5
AWV_LIFT_ROW_REVCOMP = 1
AWV_LIFT_ROW_FROM_QUERY = 2
#: awv_msa_item.code
AWV_MS_OK = 0
AWV_MS_SKIPPED = 1
AWV_MS_BAD_OP = 2
AWV_MS_LENGTHS = 3
AWV_MS_NOT_CHOSEN = 4
#: sketch kinds of device pair planning (awv_sketch)
AWV_SK_CANONICAL = 0
AWV_SK_FORWARD = 1
AWV_SK_REVCOMP = 2

#: every symbol include/allwave_hip.h declares
EXPORTS = ("awv_abi_version", "awv_last_error", "awv_engine_create", "awv_engine_destroy",
           "awv_engine_set_sequences", "awv_align_pairs", "awv_align_one", "awv_score_pairs", "awv_engine_stats",
           "awv_score_pairs_bounded", "awv_orient_pairs", "awv_orient_decide", "awv_orient_settling_bound",
           "awv_sketch", "awv_sketch_copy", "awv_sketch_pair_counts", "awv_sketch_rows", "awv_sketch_knn", "awv_keep_pairs",
           "awv_align_pairs_verified", "awv_verify_cigars", "awv_verify_one_host", "awv_engine_verify_stats",
           "awv_align_ranges", "awv_align_ranges_verified", "awv_score_ranges", "awv_verify_ranges",
           "awv_align_pairs_bounded", "awv_align_ranges_bounded", "awv_divergence_bound",
           "awv_clip_one_host", "awv_clip_cigars", "awv_align_pairs_clipped", "awv_align_ranges_clipped", "awv_engine_clip_stats",
           "awv_twin_stats",
           "awv_split_slots", "awv_split_layout_pairs", "awv_split_layout_ranges", "awv_split_one_host", "awv_split_cigars",
           "awv_align_pairs_split", "awv_align_ranges_split", "awv_engine_split_stats",
           "awv_normalize_one_host", "awv_normalize_cigars", "awv_normalize_ranges", "awv_engine_set_normalize",
           "awv_engine_normalize_stats",
           "awv_encode_one_host", "awv_encode_cigars", "awv_align_pairs_encoded", "awv_align_ranges_encoded", "awv_engine_encode_stats",
           "awv_cs_one_host", "awv_cs_cigars", "awv_cs_ranges", "awv_align_pairs_cs", "awv_align_ranges_cs", "awv_engine_cs_stats",
           "awv_coverage_one_host", "awv_engine_coverage_begin", "awv_engine_coverage_read", "awv_coverage_cigars", "awv_coverage_ranges",
           "awv_engine_coverage_stats",
           "awv_variants_one_host", "awv_variants_fold_host", "awv_engine_variants_begin", "awv_engine_variants_end", "awv_engine_variants_read", "awv_engine_variants_stats",
           "awv_variants_cigars", "awv_variants_ranges", "awv_variants_fold",
           "awv_lift_one_host", "awv_lift_cigars", "awv_lift_ranges", "awv_engine_lift_begin", "awv_engine_lift_read", "awv_engine_lift_stats",
           "awv_msa_host", "awv_msa_cigars", "awv_msa_ranges", "awv_engine_msa_stats")


class EngineConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("workgroups", C.c_int32), ("max_batch_pairs", C.c_int64),
                ("max_arena_bytes", C.c_int64), ("flags", C.c_int32), ("first_row_cols", C.c_int32),
                ("max_scratch_bytes", C.c_int64)]


class Penalties(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("match", "mismatch", "gap_open1", "gap_ext1", "gap_open2", "gap_ext2", "two_piece")]

    @classmethod
    def from_scores(cls, scores):
        """(m,x,o,e) or (m,x,o1,e1,o2,e2) -> aligner construction of
        /root/reference/src/alignment.rs:263-289 (4 scores: gap-affine, incl. the "edit" mode
        x,x,x; 6 scores: 2-piece)."""
        s = [int(v) for v in scores]
        if len(s) == 6:
            return cls(s[0], s[1], s[2], s[3], s[4], s[5], 1)
        if len(s) == 4:
            return cls(s[0], s[1], s[2], s[3], 0, 0, 0)
        raise ValueError("Invalid number of scores: %d. Expected 4 or 6 values." % len(s))


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("h2d_ms", C.c_double), ("d2h_ms", C.c_double),
                ("launches", C.c_uint64), ("cell_steps", C.c_uint64), ("extend_steps", C.c_uint64),
                ("n_breakpoints", C.c_uint64), ("n_base", C.c_uint64), ("overlap_scans", C.c_uint64),
                ("aligned_bp", C.c_uint64), ("pairs_completed", C.c_uint64), ("scratch_bytes", C.c_uint64),
                ("prof", C.c_uint64 * 14), ("restarts", C.c_uint64), ("multi_cell_steps", C.c_uint64), ("windows", C.c_uint64 * 4),
                ("clock_cycles", C.c_uint64), ("clock_ticks", C.c_uint64), ("clock_tick_khz", C.c_uint64),
                ("deep_cell_steps", C.c_uint64)]


class VerifyStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("pairs", C.c_uint64), ("failed", C.c_uint64), ("columns", C.c_uint64)]


class ClipStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("pairs", C.c_uint64), ("empty", C.c_uint64), ("columns", C.c_uint64)]


class SplitStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("pairs", C.c_uint64), ("segments", C.c_uint64), ("empty", C.c_uint64), ("columns", C.c_uint64),
                ("columns_scanned", C.c_uint64)]


class NormStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("pairs", C.c_uint64), ("records_moved", C.c_uint64), ("runs", C.c_uint64),
                ("runs_moved", C.c_uint64), ("columns_moved", C.c_uint64), ("columns", C.c_uint64)]


class EncodeStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("pairs", C.c_uint64), ("runs", C.c_uint64), ("text_bytes", C.c_uint64), ("columns", C.c_uint64)]


class CsStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("pairs", C.c_uint64), ("failed", C.c_uint64), ("text_bytes", C.c_uint64), ("columns", C.c_uint64)]


class VariantsStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("fold_ms", C.c_double), ("items", C.c_uint64), ("failed", C.c_uint64), ("columns", C.c_uint64),
                ("snv", C.c_uint64), ("ins", C.c_uint64), ("del_", C.c_uint64), ("rows", C.c_uint64), ("folds", C.c_uint64), ("capacity_rows", C.c_uint64)]


class CovStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("items", C.c_uint64), ("failed", C.c_uint64), ("columns", C.c_uint64), ("boundaries", C.c_uint64),
                ("reads", C.c_uint64)]


class LiftStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("records", C.c_uint64), ("columns", C.c_uint64), ("queries", C.c_uint64), ("ok", C.c_uint64),
                ("skipped", C.c_uint64), ("bad_op", C.c_uint64), ("lengths", C.c_uint64), ("unaligned", C.c_uint64), ("outside", C.c_uint64)]


class MsaStats(C.Structure):
    _fields_ = [("width_ms", C.c_double), ("scan_ms", C.c_double), ("emit_ms", C.c_double), ("items", C.c_uint64), ("failed", C.c_uint64),
                ("columns", C.c_uint64), ("runs", C.c_uint64), ("bases", C.c_uint64), ("bytes", C.c_uint64)]


PAIR_DTYPE = np.dtype([("q_idx", "<i4"), ("t_idx", "<i4"), ("q_revcomp", "<i4")])
#: awv_range_pair: the query interval on the query's forward strand (PAF convention), also with q_revcomp
RANGE_DTYPE = np.dtype([("q_idx", "<i4"), ("t_idx", "<i4"), ("q_revcomp", "<i4"), ("q_beg", "<i4"), ("q_end", "<i4"),
                        ("t_beg", "<i4"), ("t_end", "<i4")])
RESULT_DTYPE = np.dtype([("status", "<i4"), ("penalty", "<i4"), ("score", "<i4"), ("cigar_len", "<u4"),
                         ("cigar_off", "<u8"), ("num_matches", "<i4"), ("num_mismatches", "<i4"),
                         ("num_ins", "<i4"), ("num_del", "<i4"), ("q_end", "<i4"), ("t_end", "<i4")])
#: awv_verify_result
VERIFY_DTYPE = np.dtype([("code", "<i4"), ("reserved", "<i4"), ("column", "<i8"), ("penalty", "<i8")])
#: awv_clip_result: the best-scoring segment [col_beg, col_end) of an op string, as a slice description
CLIP_DTYPE = np.dtype([("code", "<i4"), ("reserved", "<i4"), ("score", "<i8"), ("col_beg", "<u4"), ("col_end", "<u4"),
                       ("q_skip", "<i4"), ("t_skip", "<i4"), ("num_matches", "<i4"), ("num_mismatches", "<i4"),
                       ("num_ins", "<i4"), ("num_del", "<i4"), ("penalty", "<i4"), ("reserved2", "<i4")])
#: awv_split_index: what the split found for one record; its segments are CLIP_DTYPE records in the caller's slot region
SPLIT_INDEX_DTYPE = np.dtype([("code", "<i4"), ("count", "<i4"), ("column", "<i8")])
#: awv_norm_result: what normalization did to one op string (columns_moved: the smallest offending column under AWV_NM_BAD_OP)
NORM_DTYPE = np.dtype([("code", "<i4"), ("runs_moved", "<i4"), ("columns_moved", "<i8"), ("max_shift", "<i4"), ("reserved", "<i4")])
#: awv_cigar_text: where a record's run-length text lies in its call's or batch's text arena, and its run count
CIGAR_TEXT_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("runs", "<u4")])
#: awv_cs_text: where a record's cs text lies in its call's or batch's cs arena, and its code
CS_TEXT_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("code", "<i4")])
#: awv_cs_slice: columns [col_beg, col_end) of an op string, and the bases consumed before col_beg (the fields of a clip)
CS_SLICE_DTYPE = np.dtype([("col_beg", "<u4"), ("col_end", "<u4"), ("q_skip", "<i4"), ("t_skip", "<i4")])
#: awv_cov_item: what one item added to the depth tracks
COV_ITEM_DTYPE = np.dtype([("code", "<i4"), ("aligned_cols", "<u4"), ("matched_cols", "<u4"), ("boundaries", "<u4")])
#: awv_variant: one row of the allele table (or one event: count 1), 40 bytes
VARIANT_DTYPE = np.dtype([("t_idx", "<i4"), ("pos", "<i4"), ("type", "<i4"), ("len", "<i4"), ("hash", "<u8"), ("rep", "<u8"), ("count", "<u4"),
                          ("reserved", "<u4")])
#: awv_var_item: the code and the events of one item
VAR_ITEM_DTYPE = np.dtype([("code", "<i4"), ("snv", "<u4"), ("ins", "<u4"), ("del", "<u4")])
#: awv_lift_query: [beg, end) on the forward strand of record `record`'s target (from 1) or query (from 2)
LIFT_QUERY_DTYPE = np.dtype([("record", "<i8"), ("from", "<i4"), ("beg", "<i4"), ("end", "<i4"), ("reserved", "<i4")])
#: awv_lift_result: the code, the aligned core as a slice of the record's op string, the two intervals and the slice's op counts
LIFT_DTYPE = np.dtype([("code", "<i4"), ("reserved", "<i4"), ("col_beg", "<u4"), ("col_end", "<u4"), ("q_skip", "<i4"), ("t_skip", "<i4"),
                       ("src_beg", "<i4"), ("src_end", "<i4"), ("dst_beg", "<i4"), ("dst_end", "<i4"), ("num_matches", "<i4"),
                       ("num_mismatches", "<i4"), ("num_ins", "<i4"), ("num_del", "<i4")])
#: awv_region: [beg, end) of resident sequence seq, forward strand
REGION_DTYPE = np.dtype([("seq", "<i4"), ("beg", "<i4"), ("end", "<i4")])
#: awv_lift_row: one region lifted through one alignment; the table is sorted by all fields in this order
LIFT_ROW_DTYPE = np.dtype([("region", "<i4"), ("q_idx", "<i4"), ("t_idx", "<i4"), ("flags", "<i4"), ("src_beg", "<i4"), ("src_end", "<i4"),
                           ("dst_beg", "<i4"), ("dst_end", "<i4"), ("num_matches", "<i4"), ("num_mismatches", "<i4"), ("num_ins", "<i4"),
                           ("num_del", "<i4")])
#: awv_msa_item: the code, the index into the call's targets (-1: not chosen), the row within the block (0: none), the bases placed
#: and the first and one-past-last non-gap column of the row
MSA_ITEM_DTYPE = np.dtype([("code", "<i4"), ("target", "<i4"), ("row", "<i4"), ("bases", "<u4"), ("col_beg", "<i8"), ("col_end", "<i8")])
#: awv_msa_target: the block of target t_idx is rows x width bytes at byte `off` of the arena
MSA_TARGET_DTYPE = np.dtype([("t_idx", "<i4"), ("rows", "<i4"), ("width", "<i8"), ("off", "<u8")])
#: awv_score_result
SCORE_DTYPE = np.dtype([("status", "<i4"), ("penalty", "<i4")])

#: awv_orient_result
ORIENT_DTYPE = np.dtype([("is_reverse", "<i4"), ("how", "<i4"), ("lo_f", "<i4"), ("hi_f", "<i4"), ("lo_r", "<i4"), ("hi_r", "<i4"),
                         ("edits_f", "<u8"), ("edits_r", "<u8"), ("rounds", "<i4"), ("reserved", "<i4")])

SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p)
#: awv_cs_sink: the sink of a cs call also takes the batch's cs arena
CS_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)

_LIB = None


def load():
    """Loads the in-tree library; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.awv_abi_version.restype = C.c_int
        L.awv_last_error.restype = C.c_char_p
        L.awv_engine_create.argtypes = [C.POINTER(EngineConfig), C.POINTER(C.c_void_p)]
        L.awv_engine_destroy.argtypes = [C.c_void_p]
        L.awv_engine_destroy.restype = None
        L.awv_engine_set_sequences.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.awv_align_pairs.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_void_p, C.c_int64, C.c_void_p,
                                      SINK_FN, C.c_void_p]
        L.awv_align_one.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_char_p, C.c_int32, C.c_char_p, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_size_t]
        L.awv_score_pairs.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        L.awv_engine_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.awv_twin_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64 * 4)]
        L.awv_score_pairs_bounded.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.awv_orient_pairs.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        L.awv_orient_decide.argtypes = [C.POINTER(Penalties), C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.awv_orient_settling_bound.argtypes = [C.POINTER(Penalties), C.c_int32, C.c_int32]
        L.awv_orient_settling_bound.restype = C.c_int32
        L.awv_align_pairs_verified.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                               SINK_FN, C.c_void_p]
        L.awv_verify_cigars.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64,
                                        C.c_void_p]
        L.awv_verify_one_host.argtypes = [C.POINTER(Penalties), C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, C.c_int64,
                                          C.c_void_p, C.c_void_p]
        L.awv_engine_verify_stats.argtypes = [C.c_void_p, C.POINTER(VerifyStats)]
        L.awv_align_ranges.argtypes = L.awv_align_pairs.argtypes
        L.awv_align_ranges_verified.argtypes = L.awv_align_pairs_verified.argtypes
        L.awv_score_ranges.argtypes = L.awv_score_pairs_bounded.argtypes
        L.awv_verify_ranges.argtypes = L.awv_verify_cigars.argtypes
        L.awv_align_pairs_bounded.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                              SINK_FN, C.c_void_p]
        L.awv_align_ranges_bounded.argtypes = L.awv_align_pairs_bounded.argtypes
        L.awv_divergence_bound.argtypes = [C.POINTER(Penalties), C.c_int32, C.c_int32, C.c_double]
        L.awv_divergence_bound.restype = C.c_int32
        L.awv_clip_one_host.argtypes = [C.POINTER(Penalties), C.c_int32, C.c_char_p, C.c_int64, C.c_void_p]
        L.awv_clip_cigars.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.awv_align_pairs_clipped.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_void_p, SINK_FN, C.c_void_p]
        L.awv_align_ranges_clipped.argtypes = L.awv_align_pairs_clipped.argtypes
        L.awv_engine_clip_stats.argtypes = [C.c_void_p, C.POINTER(ClipStats)]
        L.awv_split_slots.argtypes = [C.c_int32, C.c_int64, C.c_int64]
        L.awv_split_slots.restype = C.c_int64
        L.awv_split_layout_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p]
        L.awv_split_layout_ranges.argtypes = L.awv_split_layout_pairs.argtypes
        L.awv_split_one_host.argtypes = [C.POINTER(Penalties), C.c_int32, C.c_int64, C.c_char_p, C.c_int64, C.c_void_p, C.c_int64,
                                         C.POINTER(C.c_int64), C.c_void_p]
        L.awv_split_cigars.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64,
                                       C.c_void_p, C.c_void_p, C.c_void_p]
        L.awv_align_pairs_split.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, SINK_FN, C.c_void_p]
        L.awv_align_ranges_split.argtypes = L.awv_align_pairs_split.argtypes
        L.awv_engine_split_stats.argtypes = [C.c_void_p, C.POINTER(SplitStats)]
        L.awv_normalize_one_host.argtypes = [C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, C.c_int64, C.c_void_p,
                                             C.c_void_p]
        L.awv_normalize_cigars.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.awv_normalize_ranges.argtypes = L.awv_normalize_cigars.argtypes
        L.awv_engine_set_normalize.argtypes = [C.c_void_p, C.c_int32]
        L.awv_engine_normalize_stats.argtypes = [C.c_void_p, C.POINTER(NormStats)]
        L.awv_encode_one_host.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.awv_encode_cigars.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                        C.POINTER(C.c_uint64)]
        L.awv_align_pairs_encoded.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, SINK_FN, C.c_void_p]
        L.awv_align_ranges_encoded.argtypes = L.awv_align_pairs_encoded.argtypes
        L.awv_engine_encode_stats.argtypes = [C.c_void_p, C.POINTER(EncodeStats)]
        L.awv_cs_one_host.argtypes = [C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.c_void_p]
        L.awv_cs_cigars.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_uint64, C.POINTER(C.c_uint64)]
        L.awv_cs_ranges.argtypes = L.awv_cs_cigars.argtypes
        L.awv_align_pairs_cs.argtypes = [C.c_void_p, C.POINTER(Penalties), C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, CS_SINK_FN, C.c_void_p]
        L.awv_align_ranges_cs.argtypes = L.awv_align_pairs_cs.argtypes
        L.awv_engine_cs_stats.argtypes = [C.c_void_p, C.POINTER(CsStats)]
        L.awv_coverage_one_host.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.awv_engine_coverage_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int64]
        L.awv_engine_coverage_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.awv_coverage_cigars.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.awv_coverage_ranges.argtypes = L.awv_coverage_cigars.argtypes
        L.awv_engine_coverage_stats.argtypes = [C.c_void_p, C.POINTER(CovStats)]
        L.awv_variants_one_host.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        L.awv_variants_fold_host.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.awv_engine_variants_begin.argtypes = [C.c_void_p, C.c_int64, C.c_uint64]
        L.awv_engine_variants_end.argtypes = [C.c_void_p]
        L.awv_engine_variants_read.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.awv_engine_variants_stats.argtypes = [C.c_void_p, C.POINTER(VariantsStats)]
        L.awv_variants_cigars.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_uint64, C.POINTER(C.c_uint64)]
        L.awv_variants_ranges.argtypes = L.awv_variants_cigars.argtypes
        L.awv_variants_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.awv_lift_one_host.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_int64,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.awv_lift_cigars.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.awv_lift_ranges.argtypes = L.awv_lift_cigars.argtypes
        L.awv_engine_lift_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64]
        L.awv_engine_lift_read.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.awv_engine_lift_stats.argtypes = [C.c_void_p, C.POINTER(LiftStats)]
        L.awv_msa_host.argtypes = [C.c_char_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.awv_msa_cigars.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.awv_msa_ranges.argtypes = L.awv_msa_cigars.argtypes
        L.awv_engine_msa_stats.argtypes = [C.c_void_p, C.POINTER(MsaStats)]
        _LIB = L
    return _LIB


def lift_from(side):
    """None / "target" / "query" / "both" (or an AWV_LIFT_FROM_* value) -> 0 (off) / AWV_LIFT_FROM_*."""
    sides = {None: 0, "target": AWV_LIFT_FROM_TARGET, "query": AWV_LIFT_FROM_QUERY, "both": AWV_LIFT_FROM_BOTH,
             AWV_LIFT_FROM_TARGET: AWV_LIFT_FROM_TARGET, AWV_LIFT_FROM_QUERY: AWV_LIFT_FROM_QUERY, AWV_LIFT_FROM_BOTH: AWV_LIFT_FROM_BOTH}
    if isinstance(side, bool) or side not in sides:
        raise ValueError("liftover side: None, 'target', 'query' or 'both', not %r" % (side,))
    return sides[side]


def _struct_array(rows, dtype, what):
    """A contiguous array of `dtype` from one, or from rows of its fields in order."""
    if isinstance(rows, np.ndarray) and rows.dtype == dtype:
        return np.ascontiguousarray(rows)
    out = np.zeros(len(rows), dtype=dtype)
    names = [n for n in dtype.names if n != "reserved"]
    for k, row in enumerate(rows):
        if len(row) != len(names):
            raise ValueError("%s: %d fields per entry (%s)" % (what, len(names), ", ".join(names)))
        for name, val in zip(names, row):
            out[k][name] = val if not isinstance(val, str) else lift_from(val)
    return out


def coverage_roles(coverage):
    """None / "target" / "query" / "both" (or an AWV_COV_* value) -> 0 (off) / AWV_COV_*."""
    roles = {None: 0, "target": AWV_COV_TARGET, "query": AWV_COV_QUERY, "both": AWV_COV_BOTH,
             AWV_COV_TARGET: AWV_COV_TARGET, AWV_COV_QUERY: AWV_COV_QUERY, AWV_COV_BOTH: AWV_COV_BOTH}
    if isinstance(coverage, bool) or coverage not in roles:
        raise ValueError("coverage: None, 'target', 'query' or 'both', not %r" % (coverage,))
    return roles[coverage]


def cs_mode(cs):
    """None / "short" / "long" (or an AWV_CS_* value) -> 0 (off) / AWV_CS_SHORT / AWV_CS_LONG."""
    modes = {None: 0, "short": AWV_CS_SHORT, "long": AWV_CS_LONG, AWV_CS_SHORT: AWV_CS_SHORT, AWV_CS_LONG: AWV_CS_LONG}
    if isinstance(cs, bool) or cs not in modes:
        raise ValueError("cs: None, 'short' or 'long', not %r" % (cs,))
    return modes[cs]


def norm_mode(normalize):
    """None / "off" / "left" / "right" (or an AWV_NORM_* value) -> AWV_NORM_*."""
    modes = {None: AWV_NORM_OFF, "off": AWV_NORM_OFF, "left": AWV_NORM_LEFT, "right": AWV_NORM_RIGHT,
             AWV_NORM_OFF: AWV_NORM_OFF, AWV_NORM_LEFT: AWV_NORM_LEFT, AWV_NORM_RIGHT: AWV_NORM_RIGHT}
    if isinstance(normalize, bool) or normalize not in modes:
        raise ValueError("normalize: None, 'left' or 'right'")
    return modes[normalize]


class EngineError(RuntimeError):
    def __init__(self, code, where):
        msg = load().awv_last_error()
        super().__init__("%s failed with %d: %s" % (where, code, (msg or b"").decode(errors="replace")))
        self.code = code


class RowsDoNotFit(Exception):
    """variants_read / variants_cigars / variants_ranges with a `cap` smaller than the table: nothing was written; n_rows is
    what it takes (and items, for the calls on records, what the pass made of them)."""

    def __init__(self, n_rows, items=None):
        super().__init__("%d rows do not fit the buffer" % n_rows)
        self.n_rows = int(n_rows)
        self.items = items


class Engine:
    """One engine per GPU (owns device copies of the sequences, scratch arenas, one stream)."""

    def __init__(self, device=0, workgroups=0, max_batch_pairs=0, max_arena_bytes=0, flags=0, max_scratch_bytes=0, first_row_cols=0):
        L = load()
        self._h = C.c_void_p()
        cfg = EngineConfig(device, workgroups, max_batch_pairs, max_arena_bytes, flags, first_row_cols, max_scratch_bytes)
        rc = L.awv_engine_create(C.byref(cfg), C.byref(self._h))
        if rc != AWV_OK:
            self._h = C.c_void_p()
            raise EngineError(rc, "awv_engine_create")
        self.nseq = 0

    def close(self):
        if getattr(self, "_h", None):
            load().awv_engine_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def set_sequences(self, seqs):
        """seqs: list of bytes, or (uint8 array, uint64 offsets[n+1])."""
        if isinstance(seqs, tuple):
            data = np.ascontiguousarray(seqs[0], dtype=np.uint8)
            offs = np.ascontiguousarray(seqs[1], dtype=np.uint64)
        else:
            offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
            data = np.frombuffer(b"".join(bytes(s) for s in seqs), dtype=np.uint8)
            if data.size == 0:
                data = np.zeros(1, dtype=np.uint8)
        n = len(offs) - 1
        rc = load().awv_engine_set_sequences(self._h, n, data.ctypes.data, offs.ctypes.data)
        if rc != AWV_OK:
            raise EngineError(rc, "awv_engine_set_sequences")
        self.nseq = n
        self._seq_offsets = offs.astype(np.int64)

    @staticmethod
    def _pair_array(pairs):
        if not (isinstance(pairs, np.ndarray) and pairs.dtype == PAIR_DTYPE):
            a = np.asarray(pairs, dtype=np.int32)
            a = a.reshape(len(a), -1) if len(a) else np.zeros((0, 2), dtype=np.int32)
            p = np.zeros(len(a), dtype=PAIR_DTYPE)
            if len(a):
                p["q_idx"], p["t_idx"] = a[:, 0], a[:, 1]
                if a.shape[1] > 2:
                    p["q_revcomp"] = a[:, 2]
            pairs = p
        return np.ascontiguousarray(pairs)

    @staticmethod
    def _range_array(ranges):
        if not (isinstance(ranges, np.ndarray) and ranges.dtype == RANGE_DTYPE):
            a = np.asarray(ranges, dtype=np.int32)
            a = a.reshape(len(a), 7) if len(a) else np.zeros((0, 7), dtype=np.int32)
            r = np.zeros(len(a), dtype=RANGE_DTYPE)
            for k, name in enumerate(RANGE_DTYPE.names):
                r[name] = a[:, k]
            ranges = r
        return np.ascontiguousarray(ranges)

    def align_ranges(self, scores, ranges, want_cigars=True, verify=False, max_penalty=None, clip=None, _sink_hook=None, split=None,
                     normalize=None, encode=False, cs=None):
        """align_pairs on interval pairs (awv_align_ranges / awv_align_ranges_verified).  ranges: int array [n,7] (q_idx, t_idx,
        q_revcomp, q_beg, q_end, t_beg, t_end) or a RANGE_DTYPE array; the query interval is on the query's forward strand.
        The records' q_end / t_end are consumed lengths, relative to the range.  max_penalty: as for align_pairs
        (awv_align_ranges_bounded); clip, split, normalize, encode: as for align_pairs (awv_align_ranges_clipped,
        awv_align_ranges_split, awv_align_ranges_encoded); cs: as for align_pairs (awv_align_ranges_cs)."""
        return self._align("awv_align_ranges", scores, self._range_array(ranges), want_cigars, verify, max_penalty, clip, _sink_hook, split,
                           normalize, encode, cs)

    def score_ranges(self, scores, ranges, max_penalty=None):
        """score_pairs on interval pairs (awv_score_ranges).  max_penalty: None, or one bound per range (negative: none)."""
        pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
        ranges = self._range_array(ranges)
        bounds = None
        if max_penalty is not None:
            bounds = np.ascontiguousarray(np.broadcast_to(np.asarray(max_penalty, dtype=np.int32), (len(ranges),)))
            bounds = bounds if len(bounds) else np.zeros(1, dtype=np.int32)
        out = np.zeros(max(len(ranges), 1), dtype=SCORE_DTYPE)[:len(ranges)]
        rc = load().awv_score_ranges(self._h, C.byref(pen), ranges.ctypes.data, len(ranges), None if bounds is None else bounds.ctypes.data,
                                     out.ctypes.data)
        if rc != AWV_OK:
            raise EngineError(rc, "awv_score_ranges")
        return out

    def verify_ranges(self, scores, ranges, results, arena):
        """verify_cigars on interval pairs (awv_verify_ranges)."""
        return self._verify("awv_verify_ranges", scores, self._range_array(ranges), results, arena)

    def align_pairs(self, scores, pairs, want_cigars=True, verify=False, max_penalty=None, clip=None, _sink_hook=None, split=None,
                    normalize=None, encode=False, cs=None):
        """pairs: int array [n,2] (q,t) or [n,3] (q,t,revcomp), or a PAIR_DTYPE array.
        Returns (results structured array, list of op-byte strings or None); verify=True: every finished pair is checked on
        the device (awv_align_pairs_verified) and a VERIFY_DTYPE array comes back as a third value.
        max_penalty: None = no bound; an int >= 0: one bound for every pair; an array or a list: one bound per pair, a
        negative entry leaving that pair unbounded (awv_align_pairs_bounded).  A pair proved above its bound comes back
        AWV_ST_ABOVE_BOUND with penalty bound + 1, no CIGAR (None in the list) and zero counts.
        clip: None, or the match bonus a (1 .. 32767): every finished pair's op string is clipped to its best-scoring segment
        on the device (awv_align_pairs_clipped) and a CLIP_DTYPE array comes back as one more value, after the verify array
        when there is one.  Records and CIGARs are the unclipped call's: the clip describes a slice.
        _sink_hook: a test aid, not part of the interface -- with clip, called as _sink_hook(first, n, clips) inside every sink
        callback, clips being the CLIP_DTYPE array of the whole call as filled so far.
        split: None, or (a, min_score): every finished pair's op string is split into all its maximal segments that score at
        least min_score (awv_align_pairs_split; not together with clip).  One more value comes back, after the verify array
        when there is one: (index, segments), a SPLIT_INDEX_DTYPE array with one entry per pair and the list of each pair's
        segments as CLIP_DTYPE arrays, in column order.  With split, _sink_hook is called as _sink_hook(first, n, (index,
        seg_first, slots)) -- the call's raw storage as filled so far.
        normalize: None, "left" or "right": every finished pair's gap runs are moved to their left- (right-) normal place on
        the device before the check, the clip, the split and the copy back (awv_engine_set_normalize for this call; the
        engine's mode is off again afterwards).  Records are those of the unnormalized call; normalize_stats() reports.
        encode=True: every finished pair's op string -- normalized, and clipped to its segment, when those are asked for -- is
        turned into its run-length text on the device (awv_align_pairs_encoded; not together with split), and the text comes
        back in the op bytes' place: the second value is the list of texts (bytes; b"" for a pair that is not completed or has
        no clip; None throughout without want_cigars or under AWV_F_KEEP_ON_DEVICE), and one more value comes last, the
        CIGAR_TEXT_DTYPE array (offsets relative to each batch's text arena).  Records, the verify and the clip arrays are the
        call's without encode; encode_stats() reports.
        cs="short" / "long": every finished pair's cs difference string -- of the normalized string, and of the clip's segment,
        when those are asked for -- is made on the device (awv_align_pairs_cs; not together with split).  One more value comes
        back, last of all: (texts, csout), the list of cs texts (bytes; b"" for a pair without one; None without want_cigars or
        under AWV_F_KEEP_ON_DEVICE) and the CS_TEXT_DTYPE array (offsets relative to each batch's cs arena).  Everything else
        is the call's without cs; cs_stats() reports."""
        return self._align("awv_align_pairs", scores, self._pair_array(pairs), want_cigars, verify, max_penalty, clip, _sink_hook, split,
                           normalize, encode, cs)

    def split_layout(self, pairs_or_ranges, match_bonus, min_score):
        """awv_split_layout_pairs / awv_split_layout_ranges: seg_first (uint64, n + 1) for a PAIR_DTYPE / RANGE_DTYPE array (or
        what align_pairs takes) over the resident set."""
        arr = pairs_or_ranges if isinstance(pairs_or_ranges, np.ndarray) and pairs_or_ranges.dtype in (PAIR_DTYPE, RANGE_DTYPE) \
            else self._pair_array(pairs_or_ranges)
        arr = np.ascontiguousarray(arr)
        fn = "awv_split_layout_ranges" if arr.dtype == RANGE_DTYPE else "awv_split_layout_pairs"
        seg_first = np.zeros(len(arr) + 1, dtype=np.uint64)
        rc = getattr(load(), fn)(self._h, arr.ctypes.data, len(arr), int(match_bonus), int(min_score), seg_first.ctypes.data)
        if rc != AWV_OK:
            raise EngineError(rc, fn)
        return seg_first

    @staticmethod
    def _segment_lists(index, seg_first, slots):
        return [slots[int(seg_first[i]):int(seg_first[i]) + int(index["count"][i])].copy() for i in range(len(index))]

    def set_normalize(self, normalize):
        """awv_engine_set_normalize: the mode every later aligning call of this engine reads (None / "left" / "right")."""
        rc = load().awv_engine_set_normalize(self._h, norm_mode(normalize))
        if rc != AWV_OK:
            raise EngineError(rc, "awv_engine_set_normalize")

    def _align(self, fn, scores, pairs, want_cigars, verify, max_penalty=None, clip=None, _sink_hook=None, split=None, normalize=None,
               encode=False, cs=None):
        """_align_plain under the engine mode `normalize` (None: the mode is left alone)."""
        if norm_mode(normalize) == AWV_NORM_OFF:
            return self._align_plain(fn, scores, pairs, want_cigars, verify, max_penalty, clip, _sink_hook, split, encode, cs)
        self.set_normalize(normalize)
        try:
            return self._align_plain(fn, scores, pairs, want_cigars, verify, max_penalty, clip, _sink_hook, split, encode, cs)
        finally:
            self.set_normalize(None)

    def _align_plain(self, fn, scores, pairs, want_cigars, verify, max_penalty=None, clip=None, _sink_hook=None, split=None, encode=False, cs=None):
        """awv_align_pairs / awv_align_ranges (`fn`; verify: its _verified variant; max_penalty: its _bounded variant; clip: its
        _clipped variant, which takes the other two as well) on a contiguous PAIR_DTYPE / RANGE_DTYPE array."""
        pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
        bounds = None
        if max_penalty is not None:
            if np.ndim(max_penalty) == 0 and int(max_penalty) < 0:
                raise ValueError("max_penalty must be >= 0 (None: no bound)")
            bounds = np.ascontiguousarray(np.broadcast_to(np.asarray(max_penalty, dtype=np.int32), (len(pairs),))) \
                if np.ndim(max_penalty) == 0 else np.ascontiguousarray(max_penalty, dtype=np.int32)
            if bounds.shape != (len(pairs),):
                raise ValueError("max_penalty: need one bound per pair")
            bounds = bounds if len(bounds) else np.zeros(1, dtype=np.int32)
        res = np.zeros(len(pairs), dtype=RESULT_DTYPE)
        cigars = [None] * len(pairs) if want_cigars else None
        cres = np.zeros(max(len(pairs), 1), dtype=CLIP_DTYPE)[:len(pairs)] if clip is not None else None
        sp = None
        tres = np.zeros(max(len(pairs), 1), dtype=CIGAR_TEXT_DTYPE)[:len(pairs)] if encode else None
        if encode and split is not None:
            raise ValueError("encode and split exclude each other")
        mode = cs_mode(cs)
        if mode and split is not None:
            raise ValueError("cs and split exclude each other")
        csres = np.zeros(max(len(pairs), 1), dtype=CS_TEXT_DTYPE)[:len(pairs)] if mode else None
        cs_texts = [None] * len(pairs) if mode and want_cigars else None
        if split is not None:
            if clip is not None:
                raise ValueError("split and clip exclude each other")
            a, min_score = int(split[0]), int(split[1])
            seg_first = self.split_layout(pairs, a, min_score)
            sp = (np.zeros(max(len(pairs), 1), dtype=SPLIT_INDEX_DTYPE)[:len(pairs)], seg_first,
                  np.zeros(max(int(seg_first[-1]), 1), dtype=CLIP_DTYPE))

        def _sink(user, first, n, rptr, arena):
            if _sink_hook is not None and cres is not None:
                _sink_hook(int(first), int(n), cres)
            if _sink_hook is not None and sp is not None:
                _sink_hook(int(first), int(n), sp)
            if cigars is not None and arena and tres is not None:  # the arena is the batch's text arena
                for i in range(first, first + n):
                    cigars[i] = C.string_at(arena + int(tres["off"][i]), int(tres["len"][i]))
            elif cigars is not None and arena:
                r = np.ctypeslib.as_array(C.cast(rptr, C.POINTER(C.c_uint8)), shape=(n * RESULT_DTYPE.itemsize,))
                r = r.view(RESULT_DTYPE)
                for i in range(n):
                    if r["status"][i] == 0:
                        cigars[first + i] = C.string_at(arena + int(r["cigar_off"][i]), int(r["cigar_len"][i]))
            return 0

        def _cs_sink(user, first, n, rptr, arena, cs_arena):
            if cs_texts is not None and cs_arena:
                for i in range(first, first + n):
                    cs_texts[i] = C.string_at(cs_arena + int(csres["off"][i]), int(csres["len"][i]))
            return _sink(user, first, n, rptr, arena)

        ptr = lambda arr: None if arr is None else arr.ctypes.data
        vres = np.zeros(max(len(pairs), 1), dtype=VERIFY_DTYPE)[:len(pairs)] if verify else None  # (a required vout is one also for an empty list)
        bonus = 0 if clip is None else int(clip)
        # the richest form the request names, and what that form takes between the list and the sink
        if mode:
            suffix, args = "_cs", (ptr(bounds), bonus, ptr(res), ptr(vres), ptr(cres), ptr(tres), mode, ptr(csres))
        elif sp is not None:
            suffix, args = "_split", (ptr(bounds), a, min_score, ptr(res), ptr(vres), ptr(sp[1]), ptr(sp[0]), ptr(sp[2]))
        elif tres is not None:
            suffix, args = "_encoded", (ptr(bounds), bonus, ptr(res), ptr(vres), ptr(cres), ptr(tres))
        elif cres is not None:
            suffix, args = "_clipped", (ptr(bounds), bonus, ptr(res), ptr(vres), ptr(cres))
        elif bounds is not None:
            suffix, args = "_bounded", (ptr(bounds), ptr(res), ptr(vres))
        elif verify:
            suffix, args = "_verified", (ptr(res), ptr(vres))
        else:
            suffix, args = "", (ptr(res),)
        sink_fn, sink = (CS_SINK_FN, _cs_sink) if mode else (SINK_FN, _sink)
        cb = sink_fn(sink) if want_cigars or (_sink_hook is not None and (cres is not None or sp is not None)) else sink_fn()
        rc = getattr(load(), fn + suffix)(self._h, C.byref(pen), pairs.ctypes.data, len(pairs), *args, cb, None)
        if rc != AWV_OK:
            raise EngineError(rc, fn + suffix)
        found = None if sp is None else (sp[0], self._segment_lists(*sp))
        texts = (cs_texts, csres) if mode else None
        return (res, cigars) + tuple(x for x in (vres, cres, found, tres, texts) if x is not None)

    def verify_cigars(self, scores, pairs, results, arena):
        """awv_verify_cigars: checks caller-supplied records (a RESULT_DTYPE array whose cigar_off / cigar_len point into
        `arena`, bytes or a uint8 array) against the resident sequences on the device.  Returns a VERIFY_DTYPE array."""
        return self._verify("awv_verify_cigars", scores, self._pair_array(pairs), results, arena)

    def _verify(self, fn, scores, pairs, results, arena):
        """awv_verify_cigars / awv_verify_ranges (`fn`) on a contiguous PAIR_DTYPE / RANGE_DTYPE array."""
        pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
        results = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
        if results.shape != (len(pairs),):
            raise ValueError("results: need one record per pair")
        arena = np.frombuffer(bytes(arena), dtype=np.uint8) if not isinstance(arena, np.ndarray) else np.ascontiguousarray(arena, dtype=np.uint8)
        nbytes = int(arena.size)
        if nbytes == 0:
            arena = np.zeros(1, dtype=np.uint8)
        vres = np.zeros(max(len(pairs), 1), dtype=VERIFY_DTYPE)[:len(pairs)]
        rc = getattr(load(), fn)(self._h, C.byref(pen), pairs.ctypes.data, len(pairs), results.ctypes.data, arena.ctypes.data, nbytes,
                                 vres.ctypes.data)
        if rc != AWV_OK:
            raise EngineError(rc, fn)
        return vres

    def normalize_cigars(self, direction, pairs, results, arena):
        """awv_normalize_cigars: moves the gap runs of caller-supplied records (a RESULT_DTYPE array whose cigar_off / cigar_len
        point into `arena`, bytes or a uint8 array) to their left- / right-normal place against the resident sequences, on
        the device.  Returns (the normalized arena as a new uint8 array, a NORM_DTYPE array)."""
        return self._normalize("awv_normalize_cigars", direction, self._pair_array(pairs), results, arena)

    def normalize_ranges(self, direction, ranges, results, arena):
        """normalize_cigars on interval pairs (awv_normalize_ranges)."""
        return self._normalize("awv_normalize_ranges", direction, self._range_array(ranges), results, arena)

    def _normalize(self, fn, direction, pairs, results, arena):
        results = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
        if results.shape != (len(pairs),):
            raise ValueError("results: need one record per pair")
        arena = np.frombuffer(bytes(arena), dtype=np.uint8).copy() if not isinstance(arena, np.ndarray) else np.array(arena, dtype=np.uint8)
        nbytes = int(arena.size)
        buf = arena if nbytes else np.zeros(1, dtype=np.uint8)
        nres = np.zeros(max(len(pairs), 1), dtype=NORM_DTYPE)[:len(pairs)]
        rc = getattr(load(), fn)(self._h, norm_mode(direction), pairs.ctypes.data, len(pairs), results.ctypes.data, buf.ctypes.data, nbytes,
                                 nres.ctypes.data)
        if rc != AWV_OK:
            raise EngineError(rc, fn)
        return arena, nres

    def encode_cigars(self, results, arena, slices=None, want_text=True, text_cap=None):
        """awv_encode_cigars: the run-length texts of caller-supplied records (a RESULT_DTYPE array whose cigar_off / cigar_len
        point into `arena`, bytes or a uint8 array), made on the device; needs no sequence set.  slices: None, or an [n, 2]
        array of (col_beg, col_end) -- record i is encoded over those columns of its string.  Returns (texts, tout, text_bytes):
        the text arena as a uint8 array, a CIGAR_TEXT_DTYPE array and the arena's size.  want_text=False is the measuring call
        (text_buf == NULL, text_cap == 0) and gives texts None; text_cap: the buffer's size (default: measured first, so that it
        fits) -- a buffer smaller than text_bytes is left untouched and comes back as it was, filled with 0xff."""
        results = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
        sl = None
        if slices is not None:
            sl = np.ascontiguousarray(np.asarray(slices, dtype=np.uint32).reshape(-1, 2))
            if sl.shape != (len(results), 2):
                raise ValueError("slices: need one (col_beg, col_end) per record")
            sl = sl if len(sl) else np.zeros((1, 2), dtype=np.uint32)
        tout = np.zeros(max(len(results), 1), dtype=CIGAR_TEXT_DTYPE)[:len(results)]
        return self._text_call("awv_encode_cigars", (results.ctypes.data, len(results)), *self._arena_array(arena), sl, tout, want_text, text_cap)

    def _text_call(self, fn, head, arena, nbytes, sl, out, want_text, text_cap):
        """The text calls awv_encode_cigars / awv_cs_cigars / awv_cs_ranges (`fn`): their arguments are the engine, `head`, the
        arena and its size (as _arena_array gives them), the slices (`sl`: an array, or None), the per-record array `out`, the text
        buffer and its size, and where the text's size goes.  Returns (texts, out, text_bytes) as encode_cigars documents."""
        total = C.c_uint64(0)

        def call(buf, cap):
            rc = getattr(load(), fn)(self._h, *head, arena.ctypes.data, nbytes, None if sl is None else sl.ctypes.data, out.ctypes.data,
                                     None if buf is None else buf.ctypes.data, cap, C.byref(total))
            if rc != AWV_OK:
                raise EngineError(rc, fn)

        if not want_text:
            call(None, 0)
            return None, out, int(total.value)
        if text_cap is None:
            call(None, 0)
            text_cap = int(total.value)
        text = np.full(max(int(text_cap), 1), 0xff, dtype=np.uint8)
        call(text, int(text_cap))
        return text[:int(text_cap)], out, int(total.value)

    def cs_cigars(self, cs, pairs, results, arena, slices=None, want_text=True, text_cap=None):
        """awv_cs_cigars: the cs texts ("short" / "long") of caller-supplied records (a RESULT_DTYPE array whose cigar_off /
        cigar_len point into `arena`, bytes or a uint8 array) against the resident sequences, made on the device.  slices: None,
        or a CS_SLICE_DTYPE array (or [n, 4] integers: col_beg, col_end, q_skip, t_skip).  Returns (texts, csout, text_bytes):
        the cs arena as a uint8 array, a CS_TEXT_DTYPE array and the arena's size.  want_text=False is the measuring call
        (text_buf == NULL, text_cap == 0) and gives texts None; text_cap: the buffer's size (default: measured first, so that it
        fits) -- a buffer smaller than text_bytes is left untouched and comes back as it was, filled with 0xff."""
        return self._cs("awv_cs_cigars", cs, self._pair_array(pairs), results, arena, slices, want_text, text_cap)

    def cs_ranges(self, cs, ranges, results, arena, slices=None, want_text=True, text_cap=None):
        """cs_cigars on interval pairs (awv_cs_ranges)."""
        return self._cs("awv_cs_ranges", cs, self._range_array(ranges), results, arena, slices, want_text, text_cap)

    @staticmethod
    def _slice_array(slices, n):
        """None, a CS_SLICE_DTYPE array or [n, 4] integers (col_beg, col_end, q_skip, t_skip) -> None or a contiguous CS_SLICE_DTYPE array."""
        if slices is None:
            return None
        if isinstance(slices, np.ndarray) and slices.dtype == CS_SLICE_DTYPE:
            sl = np.ascontiguousarray(slices)
        else:
            raw = np.asarray(slices, dtype=np.int64).reshape(-1, 4)
            sl = np.zeros(len(raw), dtype=CS_SLICE_DTYPE)
            for k, name in enumerate(("col_beg", "col_end", "q_skip", "t_skip")):
                sl[name] = raw[:, k]
        if sl.shape != (n,):
            raise ValueError("slices: need one slice per record")
        return sl if len(sl) else np.zeros(1, dtype=CS_SLICE_DTYPE)

    @staticmethod
    def _arena_array(arena):
        """bytes or a uint8 array -> (a contiguous uint8 array, its size); an empty arena is a one-byte stand-in of size 0."""
        arena = np.frombuffer(bytes(arena), dtype=np.uint8) if not isinstance(arena, np.ndarray) else np.ascontiguousarray(arena, dtype=np.uint8)
        nbytes = int(arena.size)
        return (arena if nbytes else np.zeros(1, dtype=np.uint8)), nbytes

    def _item_call(self, pairs, results, arena, slices):
        """The opening of every call on caller-supplied records with slices (cs, coverage, variants, lift, msa; `pairs`: the pair
        or range array) -> (the records as a RESULT_DTYPE array, one per pair; the slices as _slice_array gives them; the arena
        and its size as _arena_array gives them)."""
        results = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
        if results.shape != (len(pairs),):
            raise ValueError("results: need one record per pair")
        return (results, self._slice_array(slices, len(results))) + self._arena_array(arena)

    def _cs(self, fn, cs, pairs, results, arena, slices, want_text, text_cap):
        mode = cs if isinstance(cs, int) and not isinstance(cs, bool) else cs_mode(cs)  # (an integer goes through as it is: the library refuses a bad one)
        results, sl, arena, nbytes = self._item_call(pairs, results, arena, slices)
        csout = np.zeros(max(len(results), 1), dtype=CS_TEXT_DTYPE)[:len(results)]
        return self._text_call(fn, (mode, pairs.ctypes.data, len(pairs), results.ctypes.data), arena, nbytes, sl, csout, want_text, text_cap)

    def coverage_begin(self, roles="both", clip_min_score=0):
        """awv_engine_coverage_begin: from now on every aligning call of this engine adds its contributing alignments to two
        per-base depth tracks on the device.  roles: "target", "query", "both" (or an AWV_COV_* mask); None or 0 ends coverage
        and frees the accumulators, as set_sequences does.  clip_min_score: the least score of a clip that contributes."""
        r = roles if isinstance(roles, int) and not isinstance(roles, bool) else coverage_roles(roles)  # (an integer goes through as it is)
        rc = load().awv_engine_coverage_begin(self._h, r, int(clip_min_score))
        if rc != AWV_OK:
            raise EngineError(rc, "awv_engine_coverage_begin")

    def coverage_read(self):
        """awv_engine_coverage_read: the depth so far, as (offsets, aligned, matched) -- sequence s owns entries
        [offsets[s], offsets[s + 1]) of the two uint32 arrays, one per forward-strand base.  Accumulation goes on afterwards."""
        offs = getattr(self, "_seq_offsets", np.zeros(1, dtype=np.int64))
        total = int(offs[-1])
        aligned = np.zeros(max(total, 1), dtype=np.uint32)
        matched = np.zeros(max(total, 1), dtype=np.uint32)
        rc = load().awv_engine_coverage_read(self._h, aligned.ctypes.data, matched.ctypes.data, total)
        if rc != AWV_OK:
            raise EngineError(rc, "awv_engine_coverage_read")
        return offs.copy(), aligned[:total], matched[:total]

    def coverage_cigars(self, pairs, results, arena, slices=None):
        """awv_coverage_cigars: adds caller-supplied records (a RESULT_DTYPE array whose cigar_off / cigar_len point into
        `arena`, bytes or a uint8 array) to the engine's depth tracks, on the device.  slices: as for cs_cigars.  Returns a
        COV_ITEM_DTYPE array."""
        return self._coverage("awv_coverage_cigars", self._pair_array(pairs), results, arena, slices)

    def coverage_ranges(self, ranges, results, arena, slices=None):
        """coverage_cigars on interval pairs (awv_coverage_ranges)."""
        return self._coverage("awv_coverage_ranges", self._range_array(ranges), results, arena, slices)

    def _coverage(self, fn, pairs, results, arena, slices):
        results, sl, arena, nbytes = self._item_call(pairs, results, arena, slices)
        items = np.zeros(max(len(results), 1), dtype=COV_ITEM_DTYPE)[:len(results)]
        rc = getattr(load(), fn)(self._h, pairs.ctypes.data, len(pairs), results.ctypes.data, arena.ctypes.data, nbytes,
                                 None if sl is None else sl.ctypes.data, items.ctypes.data)
        if rc != AWV_OK:
            raise EngineError(rc, fn)
        return items

    def coverage_stats(self):
        """awv_engine_coverage_stats: kernel_ms, items, failed, columns, boundaries, reads since coverage_begin."""
        return self._stats("awv_engine_coverage_stats", CovStats)

    def msa_cigars(self, pairs, results, arena, targets, slices=None, want_blocks=True, cap=None):
        """awv_msa_cigars: the target-anchored multiple alignments of `targets` (distinct sequence indices) from caller-supplied
        records (a RESULT_DTYPE array whose cigar_off / cigar_len point into `arena`, bytes or a uint8 array), on the device.
        slices: as for cs_cigars.  Returns (items, tgts, buf, msa_bytes): a MSA_ITEM_DTYPE array, a MSA_TARGET_DTYPE array, the
        arena of blocks as a uint8 array (target j's block is buf[off : off + rows * width].reshape(rows, width)) and its size.
        want_blocks=False is the measuring call (buf == NULL, cap == 0) and gives buf None; cap: the buffer's size (default:
        measured first, so that it fits) -- a buffer smaller than msa_bytes is left untouched and comes back filled with 0xff."""
        return self._msa("awv_msa_cigars", self._pair_array(pairs), results, arena, targets, slices, want_blocks, cap)

    def msa_ranges(self, ranges, results, arena, targets, slices=None, want_blocks=True, cap=None):
        """msa_cigars on interval pairs (awv_msa_ranges)."""
        return self._msa("awv_msa_ranges", self._range_array(ranges), results, arena, targets, slices, want_blocks, cap)

    def _msa(self, fn, pairs, results, arena, targets, slices, want_blocks, cap):
        results, sl, arena, nbytes = self._item_call(pairs, results, arena, slices)
        tg = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
        nt = len(tg)
        if nt == 0:
            tg = np.zeros(1, dtype=np.int32)
        items = np.zeros(max(len(results), 1), dtype=MSA_ITEM_DTYPE)[:len(results)]
        tgts = np.zeros(max(nt, 1), dtype=MSA_TARGET_DTYPE)[:nt]
        size = C.c_uint64(0)

        def call(buf, cap_):
            rc = getattr(load(), fn)(self._h, pairs.ctypes.data, len(pairs), results.ctypes.data, arena.ctypes.data, nbytes,
                                     None if sl is None else sl.ctypes.data, tg.ctypes.data, nt, items.ctypes.data, tgts.ctypes.data,
                                     None if buf is None else buf.ctypes.data, cap_, C.byref(size))
            if rc != AWV_OK:
                raise EngineError(rc, fn)

        if not want_blocks:
            call(None, 0)
            return items, tgts, None, int(size.value)
        if cap is None:
            call(None, 0)
            cap = int(size.value)
        buf = np.full(max(int(cap), 1), 0xff, dtype=np.uint8)
        call(buf, int(cap))
        return items, tgts, buf[:int(cap)], int(size.value)

    def msa_stats(self):
        """awv_engine_msa_stats: width_ms, scan_ms, emit_ms, items, failed, columns, runs, bases, bytes of the last msa_* call."""
        return self._stats("awv_engine_msa_stats", MsaStats)

    def lift_cigars(self, pairs, results, arena, queries, slices=None):
        """awv_lift_cigars: lifts intervals through caller-supplied records (a RESULT_DTYPE array whose cigar_off / cigar_len point
        into `arena`, bytes or a uint8 array), on the device.  queries: a LIFT_QUERY_DTYPE array, or (record, from, beg, end) rows
        with from "target" / "query" (or AWV_LIFT_FROM_*), in any order.  slices: as for cs_cigars.  Returns a LIFT_DTYPE array, entry
        j the answer to query j."""
        return self._lift("awv_lift_cigars", self._pair_array(pairs), results, arena, queries, slices)

    def lift_ranges(self, ranges, results, arena, queries, slices=None):
        """lift_cigars on interval pairs (awv_lift_ranges)."""
        return self._lift("awv_lift_ranges", self._range_array(ranges), results, arena, queries, slices)

    def _lift(self, fn, pairs, results, arena, queries, slices):
        results, sl, arena, nbytes = self._item_call(pairs, results, arena, slices)
        q = _struct_array(queries, LIFT_QUERY_DTYPE, "queries")
        nq = len(q)
        if nq == 0:
            q = np.zeros(1, dtype=LIFT_QUERY_DTYPE)
        lout = np.zeros(max(nq, 1), dtype=LIFT_DTYPE)[:nq]
        rc = getattr(load(), fn)(self._h, pairs.ctypes.data, len(pairs), results.ctypes.data, arena.ctypes.data, nbytes,
                                 None if sl is None else sl.ctypes.data, q.ctypes.data, nq, lout.ctypes.data)
        if rc != AWV_OK:
            raise EngineError(rc, fn)
        return lout

    def lift_begin(self, regions, from_="target", clip_min_score=0):
        """awv_engine_lift_begin: from now on every aligning call of this engine lifts `regions` (a REGION_DTYPE array or (seq, beg,
        end) rows, forward strand) through its contributing alignments, on the device, and appends the lifted ones to a table.
        from_: the side the regions lie on, "target", "query", "both" (or an AWV_LIFT_FROM_* mask); None or 0 ends the table, as
        set_sequences does.  clip_min_score: the least score of a clip that contributes."""
        mask = from_ if isinstance(from_, int) and not isinstance(from_, bool) else lift_from(from_)  # (an integer goes through as it is)
        g = _struct_array(regions if regions is not None else [], REGION_DTYPE, "regions")
        n = len(g)
        if n == 0:
            g = np.zeros(1, dtype=REGION_DTYPE)
        rc = load().awv_engine_lift_begin(self._h, g.ctypes.data, n, mask, int(clip_min_score))
        if rc != AWV_OK:
            raise EngineError(rc, "awv_engine_lift_begin")

    def lift_read(self, cap=None):
        """awv_engine_lift_read: the table so far, a LIFT_ROW_DTYPE array sorted by all its fields, region first.  cap: the rows
        the buffer holds (None: measured first); when the table is larger nothing is written and RowsDoNotFit is raised."""
        n = C.c_uint64(0)
        if cap is None:
            rc = load().awv_engine_lift_read(self._h, None, 0, C.byref(n))
            if rc != AWV_OK:
                raise EngineError(rc, "awv_engine_lift_read")
            cap = n.value
        rows = np.zeros(max(int(cap), 1), dtype=LIFT_ROW_DTYPE)
        rc = load().awv_engine_lift_read(self._h, rows.ctypes.data, int(cap), C.byref(n))
        if rc != AWV_OK:
            raise EngineError(rc, "awv_engine_lift_read")
        if n.value > int(cap):
            raise RowsDoNotFit(n.value)
        return rows[:n.value].copy()

    def lift_stats(self):
        """awv_engine_lift_stats: kernel_ms, records, columns, queries and the queries per code since lift_begin."""
        return self._stats("awv_engine_lift_stats", LiftStats)

    def variants_begin(self, clip_min_score=0, reserve_rows=0):
        """awv_engine_variants_begin: from now on every aligning call of this engine appends its contributing alignments' (site,
        allele) events to a table on the device.  reserve_rows: the row buffer's first size (0: the default)."""
        rc = load().awv_engine_variants_begin(self._h, int(clip_min_score), int(reserve_rows))
        if rc != AWV_OK:
            raise EngineError(rc, "awv_engine_variants_begin")

    def variants_end(self):
        """awv_engine_variants_end: ends the table and frees its buffer; later aligning calls append nothing."""
        rc = load().awv_engine_variants_end(self._h)
        if rc != AWV_OK:
            raise EngineError(rc, "awv_engine_variants_end")

    def variants_read(self, cap=None):
        """awv_engine_variants_read: the folded table so far, a VARIANT_DTYPE array in key order.  cap: the rows the buffer holds
        (None: measured first, by a read without a buffer -- a fold of its own); when the table is larger nothing is written and
        RowsDoNotFit is raised."""
        n = C.c_uint64(0)
        if cap is None:
            rc = load().awv_engine_variants_read(self._h, None, 0, C.byref(n))
            if rc != AWV_OK:
                raise EngineError(rc, "awv_engine_variants_read")
            cap = n.value
        rows = np.zeros(max(int(cap), 1), dtype=VARIANT_DTYPE)
        rc = load().awv_engine_variants_read(self._h, rows.ctypes.data, int(cap), C.byref(n))
        if rc != AWV_OK:
            raise EngineError(rc, "awv_engine_variants_read")
        if n.value > int(cap):
            raise RowsDoNotFit(n.value)
        return rows[:n.value].copy()

    def variants_stats(self):
        """awv_engine_variants_stats: kernel_ms, fold_ms, items, failed, columns, snv, ins, del_, rows, folds, capacity_rows since variants_begin."""
        return self._stats("awv_engine_variants_stats", VariantsStats)

    def variants_cigars(self, pairs, results, arena, slices=None, fold=AWV_VTAB_EVENTS, cap=None):
        """awv_variants_cigars: the events of caller-supplied records (a RESULT_DTYPE array whose cigar_off / cigar_len point
        into `arena`, bytes or a uint8 array) against the resident set, on the device.  fold: AWV_VTAB_EVENTS (the count-1 events
        in record order, then column order), AWV_VTAB_FOLDED (the call's table) or AWV_VTAB_ACCUMULATE (into the engine's table).
        Returns (a VAR_ITEM_DTYPE array, a VARIANT_DTYPE array); under AWV_VTAB_ACCUMULATE the second entry is the number of
        events appended.  cap: the rows the buffer holds (None: one row per column of the records, which no item exceeds, so the
        pass runs once); when there are more rows nothing is written and RowsDoNotFit is raised."""
        return self._variants("awv_variants_cigars", self._pair_array(pairs), results, arena, slices, fold, cap)

    def variants_ranges(self, ranges, results, arena, slices=None, fold=AWV_VTAB_EVENTS, cap=None):
        """variants_cigars on interval pairs (awv_variants_ranges)."""
        return self._variants("awv_variants_ranges", self._range_array(ranges), results, arena, slices, fold, cap)

    def _variants(self, fn, pairs, results, arena, slices, fold, cap):
        results, sl, arena, nbytes = self._item_call(pairs, results, arena, slices)
        items = np.zeros(max(len(results), 1), dtype=VAR_ITEM_DTYPE)[:len(results)]
        n = C.c_uint64(0)

        def call(rows, room):
            rc = getattr(load(), fn)(self._h, pairs.ctypes.data, len(pairs), results.ctypes.data, arena.ctypes.data, nbytes,
                                     None if sl is None else sl.ctypes.data, int(fold), items.ctypes.data, None if rows is None else rows.ctypes.data, room,
                                     C.byref(n))
            if rc != AWV_OK:
                raise EngineError(rc, fn)

        if fold == AWV_VTAB_ACCUMULATE:
            call(None, 0)
            return items, int(n.value)
        if cap is None:  # an event takes a column or more
            done = results["status"] == 0
            width = results["cigar_len"].astype(np.int64) if sl is None else np.minimum(sl["col_end"].astype(np.int64) - sl["col_beg"].astype(np.int64), results["cigar_len"].astype(np.int64))
            cap = int(np.maximum(width, 0)[done].sum())
        rows = np.zeros(max(int(cap), 1), dtype=VARIANT_DTYPE)
        call(rows, int(cap))
        if n.value > int(cap):
            raise RowsDoNotFit(n.value, items)
        return items, rows[:n.value].copy()

    def variants_fold(self, rows):
        """awv_variants_fold: events or rows (VARIANT_DTYPE) sorted by key and reduced on the device; a new array."""
        rows = np.array(rows, dtype=VARIANT_DTYPE, copy=True).reshape(-1)
        buf = rows if len(rows) else np.zeros(1, dtype=VARIANT_DTYPE)
        n = C.c_uint64(0)
        rc = load().awv_variants_fold(self._h, buf.ctypes.data, len(rows), C.byref(n))
        if rc != AWV_OK:
            raise EngineError(rc, "awv_variants_fold")
        return rows[:n.value].copy()

    def _stats(self, fn_name, cls):
        """One of the awv_engine_*_stats getters: the engine's `cls` record."""
        st = cls()
        rc = getattr(load(), fn_name)(self._h, C.byref(st))
        if rc != AWV_OK:
            raise EngineError(rc, fn_name)
        return st

    def cs_stats(self):
        """awv_engine_cs_stats: kernel_ms, pairs, failed, text_bytes, columns of the last cs call."""
        return self._stats("awv_engine_cs_stats", CsStats)

    def encode_stats(self):
        """awv_engine_encode_stats: kernel_ms, pairs, runs, text_bytes, columns of the last encoding call."""
        return self._stats("awv_engine_encode_stats", EncodeStats)

    def normalize_stats(self):
        """awv_engine_normalize_stats: kernel_ms, pairs, records_moved, runs, runs_moved, columns_moved, columns of the last
        normalizing call."""
        return self._stats("awv_engine_normalize_stats", NormStats)

    def clip_cigars(self, scores, match_bonus, results, arena):
        """awv_clip_cigars: clips caller-supplied records (a RESULT_DTYPE array whose cigar_off / cigar_len point into `arena`,
        bytes or a uint8 array) to their best-scoring segments on the device; needs no sequence set.  Returns a CLIP_DTYPE
        array."""
        pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
        results = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
        arena = np.frombuffer(bytes(arena), dtype=np.uint8) if not isinstance(arena, np.ndarray) else np.ascontiguousarray(arena, dtype=np.uint8)
        nbytes = int(arena.size)
        if nbytes == 0:
            arena = np.zeros(1, dtype=np.uint8)
        cres = np.zeros(max(len(results), 1), dtype=CLIP_DTYPE)[:len(results)]
        rc = load().awv_clip_cigars(self._h, C.byref(pen), int(match_bonus), results.ctypes.data, len(results), arena.ctypes.data, nbytes,
                                    cres.ctypes.data)
        if rc != AWV_OK:
            raise EngineError(rc, "awv_clip_cigars")
        return cres

    def split_cigars(self, scores, match_bonus, min_score, results, arena, seg_first=None, slots=None):
        """awv_split_cigars: splits caller-supplied records (as for clip_cigars) into all their segments that score at least
        min_score, on the device; needs no sequence set.  seg_first (uint64, n + 1; default: what the slot rule requires,
        awv_split_slots over each cigar_len) and slots (a CLIP_DTYPE array written in place; default: a zeroed one) are the
        caller's segment storage.  Returns (index, segments): a SPLIT_INDEX_DTYPE array and the list of each record's
        segments as CLIP_DTYPE arrays."""
        pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
        results = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
        arena = np.frombuffer(bytes(arena), dtype=np.uint8) if not isinstance(arena, np.ndarray) else np.ascontiguousarray(arena, dtype=np.uint8)
        nbytes = int(arena.size)
        if nbytes == 0:
            arena = np.zeros(1, dtype=np.uint8)
        if seg_first is None:
            need = [split_slots(match_bonus, min_score, int(r["cigar_len"])) if r["status"] == AWV_ST_COMPLETED else 0 for r in results]
            seg_first = np.concatenate(([0], np.cumsum(need, dtype=np.uint64))).astype(np.uint64)
        seg_first = np.ascontiguousarray(seg_first, dtype=np.uint64)
        if seg_first.shape != (len(results) + 1,):
            raise ValueError("seg_first: need one entry per record and one more")
        if slots is None:
            slots = np.zeros(max(int(seg_first[-1]), 1), dtype=CLIP_DTYPE)
        if slots.dtype != CLIP_DTYPE or not slots.flags.c_contiguous or len(slots) < int(seg_first.max()):
            raise ValueError("slots: need a contiguous CLIP_DTYPE array that holds seg_first's regions")
        index = np.zeros(max(len(results), 1), dtype=SPLIT_INDEX_DTYPE)[:len(results)]
        rc = load().awv_split_cigars(self._h, C.byref(pen), int(match_bonus), int(min_score), results.ctypes.data, len(results),
                                     arena.ctypes.data, nbytes, seg_first.ctypes.data, index.ctypes.data, slots.ctypes.data)
        if rc != AWV_OK:
            raise EngineError(rc, "awv_split_cigars")
        return index, self._segment_lists(index, seg_first, slots)

    def split_stats(self):
        """awv_engine_split_stats: kernel_ms, pairs, segments, empty, columns, columns_scanned of the last splitting call."""
        return self._stats("awv_engine_split_stats", SplitStats)

    def clip_stats(self):
        """awv_engine_clip_stats: kernel_ms, pairs, empty, columns of the last clipping call."""
        return self._stats("awv_engine_clip_stats", ClipStats)

    def verify_stats(self):
        """awv_engine_verify_stats: kernel_ms, pairs, failed, columns of the last verifying call."""
        return self._stats("awv_engine_verify_stats", VerifyStats)

    def score_pairs(self, scores, pairs, max_penalty=None):
        """Score-only alignment (awv_score_pairs): the optimal penalty of every pair, no CIGAR.  pairs as for align_pairs.
        max_penalty: None = no bound; else pairs whose penalty exceeds it come back AWV_ST_ABOVE_BOUND with penalty
        max_penalty + 1; an array or a list: one bound per pair (awv_score_pairs_bounded; a negative entry: no bound for
        that pair).  Returns a SCORE_DTYPE structured array (status, penalty)."""
        pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
        pairs = self._pair_array(pairs)
        if max_penalty is not None and np.ndim(max_penalty) > 0:
            bounds = np.ascontiguousarray(max_penalty, dtype=np.int32)
            if bounds.shape != (len(pairs),):
                raise ValueError("max_penalty: need one bound per pair")
            out = np.zeros(max(len(pairs), 1), dtype=SCORE_DTYPE)[:len(pairs)]
            bounds = bounds if len(bounds) else np.zeros(1, dtype=np.int32)
            rc = load().awv_score_pairs_bounded(self._h, C.byref(pen), pairs.ctypes.data, len(pairs), bounds.ctypes.data, out.ctypes.data)
            if rc != AWV_OK:
                raise EngineError(rc, "awv_score_pairs_bounded")
            return out
        bound = -1 if max_penalty is None else int(max_penalty)
        if max_penalty is not None and bound < 0:
            raise ValueError("max_penalty must be >= 0 (None: no bound)")
        out = np.zeros(max(len(pairs), 1), dtype=SCORE_DTYPE)[:len(pairs)]  # (out is required, also for an empty list)
        rc = load().awv_score_pairs(self._h, C.byref(pen), pairs.ctypes.data, len(pairs), bound, out.ctypes.data)
        if rc != AWV_OK:
            raise EngineError(rc, "awv_score_pairs")
        return out

    def orient_pairs(self, scores, pairs, full=False):
        """WFA orientation (awv_orient_pairs) under the orientation penalties `scores`: per pair whether the query is to be
        reverse-complemented, decided from bounded strand scores where those prove it (how == AWV_ORIENT_BY_BOUND) and from
        the edit counts of two full alignments where they do not (AWV_ORIENT_BY_EDITS); full=True: two full alignments for
        every pair.  pairs as for align_pairs (a third column is ignored).  Returns an ORIENT_DTYPE structured array."""
        pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
        pairs = self._pair_array(pairs)
        out = np.zeros(max(len(pairs), 1), dtype=ORIENT_DTYPE)[:len(pairs)]
        rc = load().awv_orient_pairs(self._h, C.byref(pen), pairs.ctypes.data, len(pairs), AWV_ORIENT_FULL if full else 0, out.ctypes.data)
        if rc != AWV_OK:
            raise EngineError(rc, "awv_orient_pairs")
        return out

    def align_one(self, scores, pattern, text):
        """Mirror of wf.align + wf.score + wf.cigar (alignment.rs:231-236). Returns (result, op_bytes)."""
        pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
        pattern, text = bytes(pattern), bytes(text)
        res = np.zeros(1, dtype=RESULT_DTYPE)
        cap = len(pattern) + len(text) + 1
        buf = C.create_string_buffer(cap)
        rc = load().awv_align_one(self._h, C.byref(pen), pattern, len(pattern), text, len(text), res.ctypes.data,
                                  buf, cap)
        if rc != AWV_OK:
            raise EngineError(rc, "awv_align_one")
        return res[0], buf.raw[:int(res[0]["cigar_len"])]

    def stats(self):
        return self._stats("awv_engine_stats", Stats)

    def twin_stats(self):
        """awv_twin_stats of the last align_pairs call: (twin units, searches run shared, searches run per orientation
        inside twin units, shared searches whose two breakpoints were not mirrors)."""
        out = (C.c_uint64 * 4)()
        rc = load().awv_twin_stats(self._h, C.byref(out))
        if rc != AWV_OK:
            raise EngineError(rc, "awv_twin_stats")
        return tuple(int(v) for v in out)


def verify_one_host(scores, pattern, text, cigar, claimed):
    """awv_verify_one_host: the verification contract on the host (needs no device; the yardstick the kernel is tested
    against).  claimed: one RESULT_DTYPE record.  Returns one VERIFY_DTYPE record."""
    pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
    pattern, text, cigar = bytes(pattern), bytes(text), bytes(cigar)
    rec = np.zeros(1, dtype=RESULT_DTYPE)
    rec[0] = tuple(claimed) if isinstance(claimed, (list, tuple)) else claimed
    out = np.zeros(1, dtype=VERIFY_DTYPE)
    rc = load().awv_verify_one_host(C.byref(pen), pattern, len(pattern), text, len(text), cigar, len(cigar), rec.ctypes.data,
                                    out.ctypes.data)
    if rc != AWV_OK:
        raise EngineError(rc, "awv_verify_one_host")
    return out[0]


def normalize_one_host(direction, pattern, text, cigar):
    """awv_normalize_one_host: the normalization contract on the host (needs no device; the yardstick the kernel is tested
    against).  direction: "left" / "right".  Returns (op bytes, one NORM_DTYPE record); the bytes are the input's on any
    code but AWV_NM_OK."""
    pattern, text, cigar = bytes(pattern), bytes(text), bytes(cigar)
    buf = C.create_string_buffer(max(len(cigar), 1))
    out = np.zeros(1, dtype=NORM_DTYPE)
    rc = load().awv_normalize_one_host(norm_mode(direction), pattern, len(pattern), text, len(text), cigar, len(cigar), buf, out.ctypes.data)
    if rc != AWV_OK:
        raise EngineError(rc, "awv_normalize_one_host")
    return buf.raw[:len(cigar)], out[0]


def encode_one_host(cigar, cap=None):
    """awv_encode_one_host: the run-length text of an op string on the host (needs no device; the yardstick the kernels are
    tested against).  Returns (text, one CIGAR_TEXT_DTYPE record); cap: the buffer's size (default: enough) -- with a buffer
    smaller than the text, the text is b"" and the record still holds its length and run count."""
    cigar = bytes(cigar)
    size = 2 * len(cigar) if cap is None else int(cap)
    buf = C.create_string_buffer(max(size, 1))
    out = np.zeros(1, dtype=CIGAR_TEXT_DTYPE)
    rc = load().awv_encode_one_host(cigar, len(cigar), buf, size, out.ctypes.data)
    if rc != AWV_OK:
        raise EngineError(rc, "awv_encode_one_host")
    n = int(out[0]["len"])
    return (buf.raw[:n] if n <= size else b""), out[0]


def cs_one_host(cs, pattern, text, cigar, slice=None, cap=None):
    """awv_cs_one_host: the cs text ("short" / "long") of an op string over `pattern` and `text` on the host (needs no device;
    the yardstick the kernels are tested against).  slice: None, or (col_beg, col_end, q_skip, t_skip).  Returns (text, one
    CS_TEXT_DTYPE record); cap: the buffer's size (default: enough) -- with a buffer too small for the text nothing is written
    and the text comes back empty, the record still says how long it is."""
    pattern, text, cigar = bytes(pattern), bytes(text), bytes(cigar)
    size = 3 * len(cigar) + 16 if cap is None else int(cap)
    buf = C.create_string_buffer(max(size, 1))
    out = np.zeros(1, dtype=CS_TEXT_DTYPE)
    sl = None
    if slice is not None:
        sl = np.zeros(1, dtype=CS_SLICE_DTYPE)
        sl[0] = tuple(int(v) for v in slice)
    rc = load().awv_cs_one_host(cs_mode(cs), pattern, len(pattern), text, len(text), cigar, len(cigar), None if sl is None else sl.ctypes.data, buf, size,
                                out.ctypes.data)
    if rc != AWV_OK:
        raise EngineError(rc, "awv_cs_one_host")
    n = int(out[0]["len"])
    return (buf.raw[:n] if n <= size else b""), out[0]


def coverage_one_host(roles, q_revcomp, qlen, tlen, cigar, span=None, slice=None, q_tracks=None, t_tracks=None):
    """awv_coverage_one_host: adds one item to per-base depth tracks on the host (needs no device; the yardstick the kernel is
    tested against).  roles: "target" / "query" / "both" (or an AWV_COV_* mask); span: None (the whole of both sequences) or
    (pb, pe, tb, te) in pattern / text coordinates; slice: None, or (col_beg, col_end, q_skip, t_skip).  q_tracks / t_tracks:
    (aligned, matched) pairs of contiguous uint32 arrays with qlen / tlen entries, added to in place (None: new zeroed ones;
    the same pair may be passed for both, for a sequence aligned with itself).  Returns (one COV_ITEM_DTYPE record, q_tracks,
    t_tracks)."""
    cigar = bytes(cigar)
    r = roles if isinstance(roles, int) and not isinstance(roles, bool) else coverage_roles(roles)
    pb, pe, tb, te = (0, qlen, 0, tlen) if span is None else (int(v) for v in span)
    if q_tracks is None:
        q_tracks = (np.zeros(qlen, dtype=np.uint32), np.zeros(qlen, dtype=np.uint32))
    if t_tracks is None:
        t_tracks = (np.zeros(tlen, dtype=np.uint32), np.zeros(tlen, dtype=np.uint32))
    for tr, ln in ((q_tracks, qlen), (t_tracks, tlen)):
        for a in tr:
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"] and a.shape == (ln,)):
                raise ValueError("tracks: contiguous uint32 arrays with one entry per base")
    sl = None
    if slice is not None:
        sl = np.zeros(1, dtype=CS_SLICE_DTYPE)
        sl[0] = tuple(int(v) for v in slice)
    out = np.zeros(1, dtype=COV_ITEM_DTYPE)
    rc = load().awv_coverage_one_host(r, int(bool(q_revcomp)), qlen, tlen, pb, pe, tb, te, cigar, len(cigar), None if sl is None else sl.ctypes.data,
                                      q_tracks[0].ctypes.data, q_tracks[1].ctypes.data, t_tracks[0].ctypes.data, t_tracks[1].ctypes.data,
                                      out.ctypes.data)
    if rc != AWV_OK:
        raise EngineError(rc, "awv_coverage_one_host")
    return out[0], q_tracks, t_tracks


def msa_host(text, items, want_block=True):
    """awv_msa_host: one target's multiple alignment on the host (needs no device; the yardstick the kernels are tested
    against).  text: the target's bytes; items: (pattern, ops, span, slice) per item -- pattern the aligned copy of the query (its
    reverse complement for a q_revcomp pair), ops the op bytes (None: a record that is not completed), span None (the whole of
    both sequences) or (pb, pe, tb, te), slice None or (col_beg, col_end, q_skip, t_skip).  Returns (ins, width, codes, block):
    the widths of the len + 1 slots, W, the items' codes and the block as a 2-D uint8 array (None with want_block=False)."""
    text = bytes(text)
    n = len(items)
    pats = [bytes(it[0]) for it in items]
    ops = [None if it[1] is None else bytes(it[1]) for it in items]
    parr = (C.c_char_p * max(n, 1))(*pats)
    carr = (C.c_char_p * max(n, 1))(*[o if o is not None else b"" for o in ops])
    plens = np.array([len(p) for p in pats] + [0], dtype=np.int32)
    clens = np.array([-1 if o is None else len(o) for o in ops] + [0], dtype=np.int64)
    rects = np.zeros((max(n, 1), 4), dtype=np.int32)
    any_slice = any(it[3] is not None for it in items)
    sl = np.zeros(max(n, 1), dtype=CS_SLICE_DTYPE)
    for k, it in enumerate(items):
        rects[k] = (0, len(pats[k]), 0, len(text)) if it[2] is None else tuple(int(v) for v in it[2])
        sl[k] = (0, max(int(clens[k]), 0), 0, 0) if it[3] is None else tuple(int(v) for v in it[3])
    ins = np.zeros(len(text) + 1, dtype=np.uint32)
    codes = np.zeros(max(n, 1), dtype=np.int32)
    width, size = C.c_int64(0), C.c_uint64(0)

    def call(block, cap):
        rc = load().awv_msa_host(text, len(text), n, C.cast(parr, C.c_void_p), plens.ctypes.data, rects.ctypes.data, C.cast(carr, C.c_void_p),
                                 clens.ctypes.data, sl.ctypes.data if any_slice else None, ins.ctypes.data, C.byref(width), codes.ctypes.data,
                                 None if block is None else block.ctypes.data, cap, C.byref(size))
        if rc != AWV_OK:
            raise EngineError(rc, "awv_msa_host")

    call(None, 0)
    if not want_block:
        return ins, int(width.value), codes[:n], None
    block = np.zeros(max(int(size.value), 1), dtype=np.uint8)
    call(block, int(size.value))
    rows = int(size.value) // int(width.value) if width.value else 1 + int((codes[:n] == AWV_MS_OK).sum())
    return ins, int(width.value), codes[:n], block[:int(size.value)].reshape(rows, int(width.value))


def lift_one_host(from_, q_revcomp, qlen, tlen, cigar, beg, end, span=None, slice=None):
    """awv_lift_one_host: [beg, end) of the source's forward strand lifted through one item, on the host (needs no device; the
    yardstick the kernel is tested against).  from_: "target" / "query" (or AWV_LIFT_FROM_*); span: None (the whole of both
    sequences) or (pb, pe, tb, te) in pattern / text coordinates; slice: None, or (col_beg, col_end, q_skip, t_skip).  Returns one
    LIFT_DTYPE record."""
    cigar = bytes(cigar)
    f = from_ if isinstance(from_, int) and not isinstance(from_, bool) else lift_from(from_)
    pb, pe, tb, te = (0, qlen, 0, tlen) if span is None else (int(v) for v in span)
    sl = None
    if slice is not None:
        sl = np.zeros(1, dtype=CS_SLICE_DTYPE)
        sl[0] = tuple(int(v) for v in slice)
    out = np.zeros(1, dtype=LIFT_DTYPE)
    rc = load().awv_lift_one_host(f, int(bool(q_revcomp)), qlen, tlen, pb, pe, tb, te, cigar, len(cigar), None if sl is None else sl.ctypes.data,
                                  int(beg), int(end), out.ctypes.data)
    if rc != AWV_OK:
        raise EngineError(rc, "awv_lift_one_host")
    return out[0]


def variants_one_host(q_idx, t_idx, q_revcomp, pattern, tlen, cigar, span=None, slice=None):
    """awv_variants_one_host: the events of one item, in column order, on the host (needs no device; the yardstick the kernel is
    tested against).  pattern: the aligned copy of the query (its reverse complement for a q_revcomp pair); span: None (the
    whole of both sequences) or (pb, pe, tb, te); slice: None, or (col_beg, col_end, q_skip, t_skip).  Returns (one
    VAR_ITEM_DTYPE record, a VARIANT_DTYPE array of count-1 events)."""
    cigar, pattern = bytes(cigar), bytes(pattern)
    qlen = len(pattern)
    pb, pe, tb, te = (0, qlen, 0, tlen) if span is None else (int(v) for v in span)
    sl = None
    if slice is not None:
        sl = np.zeros(1, dtype=CS_SLICE_DTYPE)
        sl[0] = tuple(int(v) for v in slice)
    out = np.zeros(1, dtype=VAR_ITEM_DTYPE)
    cap = len(cigar) + 1
    events = np.zeros(cap, dtype=VARIANT_DTYPE)
    n = C.c_uint64(0)
    rc = load().awv_variants_one_host(int(q_idx), int(t_idx), int(bool(q_revcomp)), pattern, qlen, int(tlen), pb, pe, tb, te, cigar, len(cigar),
                                      None if sl is None else sl.ctypes.data, events.ctypes.data, cap, C.byref(n), out.ctypes.data)
    if rc != AWV_OK:
        raise EngineError(rc, "awv_variants_one_host")
    return out[0], events[:int(n.value)]


def variants_fold_host(rows):
    """awv_variants_fold_host: events or rows (VARIANT_DTYPE) sorted by key and reduced (sum of count, min of rep); a new array."""
    rows = np.array(rows, dtype=VARIANT_DTYPE, copy=True).reshape(-1)
    buf = rows if len(rows) else np.zeros(1, dtype=VARIANT_DTYPE)
    n = C.c_uint64(0)
    rc = load().awv_variants_fold_host(buf.ctypes.data, len(rows), C.byref(n))
    if rc != AWV_OK:
        raise EngineError(rc, "awv_variants_fold_host")
    return rows[:int(n.value)].copy()


def clip_one_host(scores, match_bonus, cigar):
    """awv_clip_one_host: the clipping contract on the host (needs no device; the yardstick the kernel is tested against).
    Returns one CLIP_DTYPE record."""
    pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
    cigar = bytes(cigar)
    out = np.zeros(1, dtype=CLIP_DTYPE)
    rc = load().awv_clip_one_host(C.byref(pen), int(match_bonus), cigar, len(cigar), out.ctypes.data)
    if rc != AWV_OK:
        raise EngineError(rc, "awv_clip_one_host")
    return out[0]


def split_slots(match_bonus, min_score, m):
    """awv_split_slots: floor(match_bonus * m / min_score), the most segments an op string with m matches can split into.
    Needs no device."""
    n = load().awv_split_slots(int(match_bonus), int(min_score), int(m))
    if n < 0:
        raise EngineError(AWV_ERR_ARG, "awv_split_slots")
    return int(n)


def split_one_host(scores, match_bonus, min_score, cigar, cap=None):
    """awv_split_one_host: the splitting contract on the host (needs no device; the yardstick the kernel is tested against).
    Returns (index record, CLIP_DTYPE array of the segments in column order); cap: the slots to offer (default: the slot
    rule's bound for a string of this length) -- the segments beyond it are counted, not returned."""
    pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
    cigar = bytes(cigar)
    if cap is None:
        cap = max(load().awv_split_slots(int(match_bonus), int(min_score), len(cigar)), 0)
    cap = min(int(cap), len(cigar))  # (a segment holds at least one column)
    out = np.zeros(max(cap, 1), dtype=CLIP_DTYPE)
    index = np.zeros(1, dtype=SPLIT_INDEX_DTYPE)
    count = C.c_int64(0)
    rc = load().awv_split_one_host(C.byref(pen), int(match_bonus), int(min_score), cigar, len(cigar), out.ctypes.data, cap, C.byref(count),
                                   index.ctypes.data)
    if rc != AWV_OK:
        raise EngineError(rc, "awv_split_one_host")
    return index[0], out[:min(int(count.value), cap)].copy()


def divergence_bound(scores, plen, tlen, d):
    """awv_divergence_bound: the penalty no alignment of divergence <= d of a plen x tlen pair can exceed, divergence =
    (#X + #I + #D) / columns.  -1: no bound (d >= 1, or it would pass INT32_MAX).  Needs no device."""
    pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
    b = load().awv_divergence_bound(C.byref(pen), int(plen), int(tlen), float(d))
    if b < -1:
        raise EngineError(AWV_ERR_ARG, "awv_divergence_bound")
    return b


def orient_decide(scores, lo_f, hi_f, lo_r, hi_r):
    """awv_orient_decide: AWV_ORIENT_FORWARD / _REVERSE / _UNDECIDED from the strands' proved penalty intervals (hi =
    AWV_ORIENT_HI_NONE: bounded only below).  Needs no device."""
    pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
    rc = load().awv_orient_decide(C.byref(pen), int(lo_f), int(hi_f), int(lo_r), int(hi_r))
    if rc < 0:
        raise EngineError(rc, "awv_orient_decide")
    return rc


def orient_settling_bound(scores, known_is_reverse, penalty):
    """awv_orient_settling_bound: the bound the other strand is searched under once one strand's penalty is known
    (-1: the known penalty settles the pair alone; AWV_ORIENT_HI_NONE: no bound).  Needs no device."""
    pen = scores if isinstance(scores, Penalties) else Penalties.from_scores(scores)
    b = load().awv_orient_settling_bound(C.byref(pen), 1 if known_is_reverse else 0, int(penalty))
    if b < -1:
        raise EngineError(AWV_ERR_ARG, "awv_orient_settling_bound")
    return b
