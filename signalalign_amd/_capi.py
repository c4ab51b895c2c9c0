"""ctypes mirror of include/signalalign_hip.h.  No arithmetic happens here."""
import ctypes as C
import time
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

FLAG_EXACT = 1
FLAG_FORCE_GENERIC = 2
FLAG_DEVICE_TO_ITSELF = 8
FLAG_INPUTS_IN_HOST_BLOCK = 16
FLAG_VC_ROWS = 32
FLAG_PAIRS8 = 64
FLAG_SITE_CALLS = 128
FLAG_POSITION_CALLS = 256
FLAG_TWO_DIST_ALL_KERNELS = 512
SITE_MAX_LETTERS = 8


class SaError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        msg = lib().sa_strerror(code).decode() if _LIB is not None else str(code)
        super().__init__("%s: %s (%d)" % (what, msg, code))


ABI = {}    # C type name -> its one mirror here: a _Struct class, or the np.dtype of a struct that is only read as numpy records


class _Struct(C.Structure):
    """A C.Structure that mirrors the C type _c_name_ of the header _c_header_; stating the name registers it in ABI."""
    _c_header_ = "include/signalalign_hip.h"

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        ABI[cls._c_name_] = cls


def _record_dtype(c_name, fields):
    """the np.dtype that mirrors the C struct c_name, registered in ABI"""
    ABI[c_name] = np.dtype(fields)
    return ABI[c_name]


class Params(_Struct):
    _c_name_ = "sa_params_t"
    _fields_ = [("threshold", C.c_double), ("diagonal_expansion", C.c_int64), ("trace_back_diagonals", C.c_int64),
                ("min_diags_between_trace_back", C.c_int64), ("split_matrix_bigger_than_this", C.c_int64)]


class HdpDesc(_Struct):
    _c_name_ = "sa_hdp_desc_t"
    _fields_ = [("num_dps", C.c_int64), ("grid_length", C.c_int64), ("grid_start", C.c_double),
                ("grid_stop", C.c_double), ("parent", C.POINTER(C.c_int64)), ("observed", C.POINTER(C.c_uint8)),
                ("post_pred", C.POINTER(C.POINTER(C.c_double))), ("slopes", C.POINTER(C.POINTER(C.c_double)))]


class Job(_Struct):
    _c_name_ = "sa_job_t"
    _fields_ = [("ref", C.c_char_p), ("ref_len", C.c_int64), ("events", C.POINTER(C.c_double)),
                ("event_stride", C.c_int64), ("n_events", C.c_int64), ("anchor_x", C.POINTER(C.c_int64)),
                ("anchor_y", C.POINTER(C.c_int64)), ("n_anchors", C.c_int64), ("scale", C.c_double),
                ("shift", C.c_double), ("var", C.c_double), ("ends", C.c_uint)]


JOB_LEFT_END_NOT_RAGGED, JOB_RIGHT_END_NOT_RAGGED = 1, 2   # sa_job_t.ends (alignmentHasRaggedLeftEnd / RightEnd, inverted)


class SiteCall(_Struct):
    _c_name_ = "sa_site_call_t"
    _fields_ = [("x", C.c_int32), ("n_letters", C.c_int32), ("letters", C.c_char * SITE_MAX_LETTERS),
                ("units", C.c_int64 * SITE_MAX_LETTERS), ("prob", C.c_double * SITE_MAX_LETTERS)]


class PositionCall(_Struct):
    _c_name_ = "sa_position_call_t"
    _fields_ = [("p", C.c_int32), ("n_rows", C.c_int32), ("n_letters", C.c_int32), ("pad", C.c_int32),
                ("letters", C.c_char * SITE_MAX_LETTERS), ("sum", C.c_double * SITE_MAX_LETTERS),
                ("prob", C.c_double * SITE_MAX_LETTERS)]


class SnpSite(_Struct):
    _c_name_ = "sa_snp_site_t"
    _fields_ = [("pos", C.c_int64), ("strand", C.c_int32), ("pad", C.c_int32), ("p", C.c_double * 4)]


class SnpJobMap(_Struct):
    _c_name_ = "sa_snp_job_map_t"
    _fields_ = [("contig", C.c_int32), ("pos_sign", C.c_int32), ("pos0", C.c_int64), ("x0", C.c_int64), ("x_sign", C.c_int32),
                ("strand", C.c_int32), ("direction", C.c_int32), ("pad", C.c_int32), ("run", C.c_int64), ("group", C.c_int64)]


class ProfileJobMap(_Struct):
    _c_name_ = "sa_profile_job_map_t"
    _fields_ = [("contig", C.c_int32), ("pos_sign", C.c_int32), ("pos0", C.c_int64)]


PROFILE_DIRECT = 1


class TruthSite(_Struct):
    _c_name_ = "sa_truth_site_t"
    _fields_ = [("contig", C.c_int32), ("mapped_strand", C.c_int32), ("pos", C.c_int64), ("change_to", C.c_char), ("pad", C.c_char * 7)]


class ScoreJobMap(_Struct):
    _c_name_ = "sa_score_job_map_t"
    _fields_ = [("contig", C.c_int32), ("x_sign", C.c_int32), ("x0", C.c_int64), ("strand", C.c_int32), ("mapped_strand", C.c_int32),
                ("true_letter", C.c_int32), ("pad", C.c_int32)]


class TrainSite(_Struct):
    _c_name_ = "sa_train_site_t"
    _fields_ = [("contig", C.c_int32), ("mapped_strand", C.c_int32), ("pos", C.c_int64)]


class TrainJobMap(_Struct):
    _c_name_ = "sa_train_job_map_t"
    _fields_ = [("contig", C.c_int32), ("x_sign", C.c_int32), ("x0", C.c_int64), ("site_strand", C.c_int32), ("pad", C.c_int32)]


class CallScoresCounts(_Struct):
    _c_name_ = "sa_call_scores_counts_t"
    _fields_ = [("unlabelled", C.c_int64), ("other_sites", C.c_int64)]


SORT_TILE = 4096
TRUTH_SITE_DTYPE, TRAIN_SITE_DTYPE, TRAIN_JOB_MAP_DTYPE = np.dtype(TruthSite), np.dtype(TrainSite), np.dtype(TrainJobMap)
CALL_SCORE_ROW_DTYPE = _record_dtype("sa_call_score_row_t", [
    ("level", "<i4"), ("group", "<i4"), ("letter", "S1"), ("pad", "S1", (7,)), ("n_pos", "<i8"), ("n_neg", "<i8"), ("auc2", "<u8"),
    ("auc", "<f8"), ("tp", "<i8"), ("fp", "<i8"), ("tn", "<i8"), ("fn", "<i8")])


class DeviationParams(_Struct):
    _c_name_ = "sa_deviation_params_t"
    _fields_ = [("threshold", C.c_int32), ("bucket_size", C.c_int32), ("n_buckets", C.c_int32)]


class DeviationJob(_Struct):
    _c_name_ = "sa_deviation_job_t"
    _fields_ = [("anchor_x", C.POINTER(C.c_int64)), ("anchor_y", C.POINTER(C.c_int64)), ("n_anchors", C.c_int64), ("n_events", C.c_int64)]


DEV_NO_GUIDE, DEV_NO_RECORDS = 1, 2
DEV_DIRECT, DEV_EVENTS, DEV_WINDOW = 1, 2, 4
DEVIATION_READ_DTYPE = _record_dtype("sa_deviation_read_t", [
    ("status", "<i4"), ("n_sets", "<i4"), ("set_first", "<i8"), ("n_aligned", "<i8"), ("n_flagged", "<i8"), ("n_on_mea", "<i8"),
    ("sum_abs", "<i8"), ("max_abs", "<i4"), ("max_abs_mea", "<i4"), ("max_event", "<i4"), ("pad", "<i4")])
DEVIATION_SET_DTYPE = _record_dtype("sa_deviation_set_t", [
    ("first_event", "<i4"), ("last_event", "<i4"), ("count", "<i4"), ("peak", "<i4"), ("mea_peak", "<i4"), ("center_event", "<i4"),
    ("open_end", "<i4"), ("pad", "<i4")])
DEVIATION_EVENT_DTYPE = _record_dtype("sa_deviation_event_t", [("best_x", "<i4"), ("guide", "<i4"), ("diff", "<i4"), ("flags", "<u4")])


class LabelJob(_Struct):
    _c_name_ = "sa_label_job_t"
    _fields_ = [("raw_start", C.POINTER(C.c_int64)), ("raw_length", C.POINTER(C.c_int64)), ("n_events", C.c_int64), ("n_samples", C.c_int64),
                ("ref_first", C.c_int64), ("ref_step", C.c_int32), ("base_shift", C.c_int32)]


LABEL_NO_RECORDS, LABEL_NO_PATH = 1, 2
LABEL_MEA, LABEL_FULL, LABEL_BANDS, LABEL_SAMPLES, LABEL_TIMES = 1, 2, 4, 8, 16
LABEL_SAMPLE_TILE = 4096
LABEL_KERNELS = ("count", "scan_events", "scatter", "order", "full", "find", "scan_path", "band_acc", "scan_bands", "job_scan", "mea_emit",
                 "band_emit", "reads", "fill")     # SA_LABEL_K_*: the order of sa_signal_labels_last_kernel_ms
LABEL_SEGMENT_DTYPE = _record_dtype("sa_label_segment_t", [
    ("raw_start", "<i8"), ("raw_length", "<i8"), ("reference_index", "<i8"), ("x", "<i4"), ("y", "<i4"), ("kmer_id", "<i4"),
    ("prob_units", "<i4")])
LABEL_BAND_DTYPE = _record_dtype("sa_label_band_t", [
    ("raw_start", "<i8"), ("raw_length", "<i8"), ("reference_index", "<i8"), ("x", "<i4"), ("n_records", "<i4")])
LABEL_READ_DTYPE = _record_dtype("sa_label_read_t", [("status", "<i4"), ("minus_strand", "<i4")] + [(n, "<i8") for n in (
    "mea_first", "n_mea", "full_first", "n_full", "band_first", "n_bands", "sample_first", "n_samples", "mea_without_record",
    "n_positions", "skipped_positions", "stay_events", "labelled_samples", "first_sample", "end_sample")])


class CallqParams(_Struct):
    _c_name_ = "sa_callq_params_t"
    _fields_ = [("bin_lo", C.c_int64), ("bin_width", C.c_int64), ("n_bins", C.c_int32), ("min_gap", C.c_int32)]


class CallqJob(_Struct):
    _c_name_ = "sa_callq_job_t"
    _fields_ = [("anchor_x", C.POINTER(C.c_int64)), ("anchor_y", C.POINTER(C.c_int64)), ("n_anchors", C.c_int64),
                ("raw_start", C.POINTER(C.c_int64)), ("raw_length", C.POINTER(C.c_int64)), ("n_events", C.c_int64)]


CQ_NO_GUIDE, CQ_NO_SITES, CQ_NO_PATH = 1, 2, 4
CQ_CALLS, CQ_BAND_DIRECT = 1, 2
CQ_MAX_BINS = 1024
CQ_KERNELS = ("band", "calls", "gaps")     # the order of sa_call_quality_last_kernel_ms
CALLQ_READ_DTYPE = _record_dtype("sa_callq_read_t", [("status", "<i4"), ("max_x", "<i4")] + [(n, "<i8") for n in (
    "n_calls", "n_correct", "n_unlabelled", "n_other_sites", "n_outside", "sum_abs_delta2", "max_abs_delta2", "n_path", "n_gaps",
    "sum_gap", "max_gap", "call_first", "gap_first")])
CALLQ_CALL_DTYPE = _record_dtype("sa_callq_call_t", [
    ("raw_start", "<i8"), ("raw_length", "<i8"), ("delta2", "<i8"), ("prob_true", "<f8"), ("x", "<i4"), ("guide_event", "<i4"),
    ("true_letter", "<i4"), ("correct", "<i4"), ("outside", "<i4"), ("pad", "<i4")])
CALLQ_GAP_DTYPE = _record_dtype("sa_callq_gap_t", [("y_before", "<i4"), ("y_after", "<i4"), ("gap", "<i8")])
PROFILE_SITE_DTYPE = _record_dtype("sa_profile_site_t", [
    ("pos", "<i8"), ("contig", "<i4"), ("read_count", "<i4"), ("kmer_count", "<i8"), ("entropy_units", "<i8"),
    ("units", "<i8", (SITE_MAX_LETTERS,)), ("entropy", "<f8"), ("prob", "<f8", (SITE_MAX_LETTERS,)), ("ref", "S1"), ("pad", "S1", (7,))])
SNP_SITE_DTYPE = np.dtype(SnpSite)
SNP_MARGINAL_DTYPE = _record_dtype("sa_snp_marginal_t", [
    ("pos", "<i8"), ("contig", "<i4"), ("depth", "<i4"), ("fwd", "<f8", (4,)), ("bwd", "<f8", (4,)), ("prob", "<f8", (4,)),
    ("delta", "<f8"), ("called", "S1"), ("ref", "S1"), ("is_proposal", "i1"), ("pad", "S1", (5,))])


class Pair(_Struct):
    _c_name_ = "sa_pair_t"
    _fields_ = [("prob_e7", C.c_int64), ("x", C.c_int32), ("y", C.c_int32), ("path", C.c_int32),
                ("kmer_id", C.c_int32)]


class BatchStats(_Struct):
    _c_name_ = "sa_batch_stats_t"
    _fields_ = [("cells_forward", C.c_double), ("cells_backward", C.c_double), ("ms_forward", C.c_double),
                ("ms_backward", C.c_double), ("ms_fold", C.c_double), ("ms_total_device", C.c_double),
                ("f_bytes", C.c_double), ("n_regions", C.c_int64), ("n_segments", C.c_int64),
                ("n_checkpoints", C.c_int64), ("n_fast_regions", C.c_int64), ("n_chunks", C.c_int64),
                ("n_groups", C.c_int64), ("n_ring_regions", C.c_int64), ("n_strip_regions", C.c_int64),
                ("device_bytes", C.c_double)]


class EaJob(_Struct):
    _c_name_ = "sa_ea_job_t"
    _fields_ = [("sequence", C.c_char_p), ("seq_len", C.c_int64), ("event_mean", C.POINTER(C.c_double)),
                ("n_events", C.c_int64), ("scale", C.c_double), ("shift", C.c_double), ("var", C.c_double)]


class GuideJob(_Struct):
    _c_name_ = "sa_guide_job_t"
    _fields_ = [("read", C.c_char_p), ("read_len", C.c_int64), ("ref", C.c_char_p), ("ref_len", C.c_int64), ("diag", C.c_int64)]


class GuideParams(_Struct):
    _c_name_ = "sa_guide_params_t"
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32),
                ("ambiguous", C.c_int32), ("band", C.c_int32), ("min_read_fraction", C.c_double)]


class GuideResult(_Struct):
    _c_name_ = "sa_guide_result_t"
    _fields_ = [("status", C.c_int32), ("score", C.c_int64), ("read_start", C.c_int64), ("read_end", C.c_int64),
                ("ref_start", C.c_int64), ("ref_end", C.c_int64), ("op_first", C.c_int64), ("n_ops", C.c_int64)]


class RefIndexInfo(_Struct):
    _c_name_ = "sa_ref_index_info_t"
    _fields_ = [("n_contigs", C.c_int64), ("total_bases", C.c_int64), ("n_entries", C.c_int64), ("q", C.c_int32), ("device", C.c_int32),
                ("host_bytes", C.c_int64), ("device_bytes", C.c_int64), ("build_seconds", C.c_double)]


class LocateParams(_Struct):
    _c_name_ = "sa_locate_params_t"
    _fields_ = [("read_bases", C.c_int32), ("max_occ", C.c_int32), ("span", C.c_int32), ("min_votes", C.c_int32), ("max_hits", C.c_int32)]


class LocateResult(_Struct):
    _c_name_ = "sa_locate_result_t"
    _fields_ = [("status", C.c_int32), ("contig", C.c_int32), ("reverse", C.c_int32), ("pos", C.c_int64), ("key", C.c_int64),
                ("votes", C.c_int64), ("second_votes", C.c_int64), ("hits", C.c_int64), ("seeds", C.c_int64), ("repetitive", C.c_int64)]


class Cigar(_Struct):
    _c_name_ = "sa_cigar_t"
    _c_header_ = "signalalign_amd/csrc/sa_io.h"
    _fields_ = [("contig1", C.c_char_p), ("contig2", C.c_char_p), ("start1", C.c_int64), ("end1", C.c_int64),
                ("start2", C.c_int64), ("end2", C.c_int64), ("strand1", C.c_int), ("strand2", C.c_int),
                ("score", C.c_double), ("n_ops", C.c_int64), ("op_type", C.POINTER(C.c_int32)),
                ("op_len", C.POINTER(C.c_int64))]


class RawJob(_Struct):
    _c_name_ = "sa_raw_job_t"
    _fields_ = [("raw", C.POINTER(C.c_int16)), ("n_samples", C.c_int64), ("digitisation", C.c_float), ("offset", C.c_float),
                ("range", C.c_float), ("sample_rate", C.c_float), ("start_time", C.c_float)]


class DetectorParams(_Struct):
    _c_name_ = "sa_detector_params_t"
    _fields_ = [("window_length1", C.c_int32), ("window_length2", C.c_int32), ("threshold1", C.c_float),
                ("threshold2", C.c_float), ("peak_height", C.c_float)]


# inc/event_detection.h: event_detection_defaults / event_detection_rna (window_length1, window_length2, threshold1,
# threshold2, peak_height)
DETECTOR_DNA = (3, 6, 1.4, 9.0, 0.2)
DETECTOR_RNA = (7, 14, 2.5, 9.0, 1.0)
RAW_NO_PEAK = 16
RAW_MAP_LENGTH = 32


class RawNpRead(_Struct):
    _c_name_ = "sa_raw_npread_t"
    _fields_ = [("status", C.c_int32), ("n_events", C.c_int64), ("events4", C.POINTER(C.c_double)),
                ("kmer_idx", C.POINTER(C.c_int32)), ("move", C.POINTER(C.c_int32)), ("p_model_state", C.POINTER(C.c_double)),
                ("raw_start", C.POINTER(C.c_int64)), ("raw_length", C.POINTER(C.c_int64)), ("read_len", C.c_int64),
                ("strand_event_map", C.POINTER(C.c_int64)), ("mom_shift", C.c_double), ("mom_scale", C.c_double)]


class RawRead(_Struct):
    _c_name_ = "sa_rawread_t"
    _c_header_ = "signalalign_amd/csrc/sa_io.h"
    _fields_ = [("digitisation", C.c_float), ("offset", C.c_float), ("range", C.c_float), ("sample_rate", C.c_float),
                ("start_time", C.c_float), ("n_samples", C.c_int64), ("seq_len", C.c_int64), ("sequence", C.c_void_p),
                ("samples", C.POINTER(C.c_int16))]


RAW_EVENT_DTYPE = _record_dtype("sa_raw_event_t", [
    ("raw_start", "<i8"), ("raw_length", "<i8"), ("mean", "<f8"), ("stdv", "<f8"), ("start", "<f8"), ("length", "<f8"),
    ("kmer_idx", "<i4"), ("move", "<i4"), ("p_model_state", "<f8")])


class MeaJob(_Struct):
    _c_name_ = "sa_mea_job_t"
    _fields_ = [("event_idx", C.POINTER(C.c_int32)), ("ref_idx", C.POINTER(C.c_int32)), ("posterior", C.POINTER(C.c_double)),
                ("n", C.c_int64), ("shortest_ref_per_event", C.POINTER(C.c_int32)), ("n_events", C.c_int64)]


MEA_INF = 2 ** 31 - 1
MEA_STATUS = {0: "ok", 1: "empty", 2: "single event", 3: "no forward edge", 4: "no path", 5: "bad event index"}


class PlanInfo(_Struct):
    _c_name_ = "sa_plan_info_t"
    _fields_ = [("n_regions", C.c_int64), ("n_segments", C.c_int64), ("n_checkpoints", C.c_int64),
                ("cells_forward", C.c_double), ("cells_backward", C.c_double), ("f_cellpaths", C.c_int64),
                ("max_span", C.c_int64), ("n_fast_regions", C.c_int64), ("n_ring_regions", C.c_int64)]


PAIR_DTYPE, POSITION_CALL_DTYPE, SITE_CALL_DTYPE = np.dtype(Pair), np.dtype(PositionCall), np.dtype(SiteCall)


class MixtureParams(_Struct):
    _c_name_ = "sa_mixture_params_t"
    _fields_ = [("n_components", C.c_int32), ("max_iter", C.c_int32), ("tol", C.c_double), ("reg_covar", C.c_double)]


class HmmView(_Struct):
    _c_name_ = "sa_hmm_view_t"
    _fields_ = [("type", C.c_int), ("n_states", C.c_int), ("n_alpha", C.c_int), ("k", C.c_int), ("alphabet", C.c_char * 64),
                ("n_kmers", C.c_int64), ("transitions", C.POINTER(C.c_double)), ("likelihood", C.POINTER(C.c_double)),
                ("event_model", C.POINTER(C.c_double)), ("event_expectations", C.POINTER(C.c_double)),
                ("posteriors", C.POINTER(C.c_double)), ("observed", C.POINTER(C.c_uint8)), ("threshold", C.c_double),
                ("n_assignments", C.c_int64), ("assignment_events", C.POINTER(C.c_double)),
                ("assignment_kmers", C.POINTER(C.c_char)), ("has_model", C.c_int)]


class HdpStateInfo(_Struct):
    _c_name_ = "sa_hdp_state_info_t"
    _fields_ = ([(n, C.c_int64) for n in ("num_dps", "depth", "grid_length", "n_data", "n_factors", "n_base_factors", "n_observed",
                                          "base_dp", "alphabet_size", "kmer_length")] +
                [(n, C.c_double) for n in ("mu", "nu", "alpha", "beta", "grid_start", "grid_stop")] +
                [(n, C.c_int) for n in ("splines_finalized", "has_data", "sample_gamma")] +
                [("data", C.POINTER(C.c_double)), ("data_dp", C.POINTER(C.c_int64)), ("gamma", C.POINTER(C.c_double)),
                 ("grid", C.POINTER(C.c_double)), ("dp_parent", C.POINTER(C.c_int64)),
                 ("dp_num_factor_children", C.POINTER(C.c_int64)), ("dp_depth", C.POINTER(C.c_int64)),
                 ("observed", C.POINTER(C.c_uint8)), ("row_of_dp", C.POINTER(C.c_int64)), ("post", C.POINTER(C.c_double)),
                 ("slope", C.POINTER(C.c_double)), ("f_type", C.POINTER(C.c_int64)), ("f_parent", C.POINTER(C.c_int64)),
                 ("f_ref", C.POINTER(C.c_int64)), ("f_params", C.POINTER(C.c_double)), ("f_n_children", C.POINTER(C.c_int64))])


# Every function bound from the library: name -> (restype, argtypes), in the order of include/signalalign_hip.h.  lib() applies
# it; nothing is called through ctypes' guessed widths.  Opaque handles and caller-typed buffers are void pointers.
_P, _vp, _str = C.POINTER, C.c_void_p, C.c_char_p
_pf64, _pi64, _pi32, _pvp, _pstr = _P(C.c_double), _P(C.c_int64), _P(C.c_int32), _P(C.c_void_p), _P(C.c_char_p)
SIGNATURES = {
    "sa_pair_roundtrip": (C.c_int, [_vp, _vp, C.c_int64]),
    "sa_model_create": (C.c_int, [_pvp, C.c_int, _str, C.c_int, _pf64, _pf64, _P(HdpDesc)]),
    "sa_model_load": (C.c_int, [_pvp, _str, _str]),
    "sa_model_destroy": (None, [_vp]),
    "sa_model_alphabet": (C.c_int, [_vp, _str, _pi32, _pi32]),
    "sa_model_table5": (_pf64, [_vp]),
    "sa_model_set_to_hdp_expected_values": (C.c_int, [_vp]),
    "sa_kmer_id": (C.c_int64, [_vp, _str]),
    "sa_model_set_emission": (C.c_int, [_vp, C.c_int]),
    "sa_model_clone_with_table": (C.c_int, [_pvp, _vp, _pf64]),
    "sa_default_ambig": (None, [_pstr]),
    "sa_load_ambig": (C.c_int, [_str, _pstr]),
    "sa_batch_create": (C.c_int, [_pvp, _vp, _P(Params), _P(Job), C.c_int64, _pstr, C.c_int, C.c_uint]),
    "sa_batch_create_noise_scaled": (C.c_int, [_pvp, _vp, _P(Params), _P(Job), _pf64, C.c_int64, _pstr, C.c_int, C.c_uint]),
    "sa_batch_run": (C.c_int, [_vp]),
    "sa_batch_create_deferred": (C.c_int, [_pvp, _vp, _P(Params), _P(Job), C.c_int64, _pstr, C.c_int, C.c_uint]),
    "sa_batch_prepare": (C.c_int, [_vp]),
    "sa_batch_start": (C.c_int, [_vp]),
    "sa_batch_wait": (C.c_int, [_vp]),
    "sa_batch_n_pairs": (C.c_int, [_vp, C.c_int64, _pi64]),
    "sa_batch_pairs": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64]),
    "sa_batch_all_pairs_summary": (C.c_int, [_vp, C.c_int64, _pi64, _pi64]),
    "sa_batch_pairs16": (C.c_int, [_vp, C.c_int64, _pvp, _pi64]),
    "sa_batch_pairs16_all": (C.c_int, [_vp, _pvp, _pi64]),
    "sa_batch_pairs8": (C.c_int, [_vp, C.c_int64, _pvp, _pi64]),
    "sa_batch_pairs8_all": (C.c_int, [_vp, _pvp, _pi64]),
    "sa_batch_pairs_all": (C.c_int, [_vp, _vp, C.c_int64, _pi64]),
    "sa_batch_release_device": (C.c_int, [_vp]),
    "sa_batch_stats": (C.c_int, [_vp, _P(BatchStats)]),
    "sa_batch_job_cells": (C.c_int, [_vp, C.c_int64, _pf64, _pf64]),
    "sa_batch_destroy": (None, [_vp]),
    "sa_align_batch": (C.c_int, [_vp, _P(Params), _P(Job), C.c_int64, _pstr, C.c_int, C.c_uint, _P(_P(Pair)), _pi64]),
    "sa_expect_batch": (C.c_int, [_vp, _P(Params), _P(Job), C.c_int64, _pstr, C.c_int, C.c_uint, _pf64, _pf64, _pvp, _pi64]),
    "sa_expect_last_stats": (C.c_int, [_P(BatchStats)]),
    "sa_plan_describe": (C.c_int, [_vp, _P(Params), _P(Job), _pstr, C.c_uint, _P(PlanInfo), _pi64, C.c_int64, _pi64, C.c_int64,
                                   _pi64, C.c_int64]),
    "sa_plan_check_path_records": (C.c_int64, [_vp, _P(Params), _P(Job), _pstr, _pi64]),
    "sa_dplan_compare": (C.c_int, [_vp, _P(Params), _P(Job), C.c_int64, _pstr, C.c_int, C.c_uint]),
    "sa_scalings_mom": (C.c_int, [_vp, _str, C.c_int64, _pf64, C.c_int64, C.c_uint, _pf64, _pf64]),
    "sa_event_align_batch": (C.c_int, [_vp, _P(EaJob), C.c_int64, C.c_int, C.c_uint, _pvp, _pi64, _pi32, _pf64, _pf64]),
    "sa_event_align_release": (None, []),
    "sa_detect_events_batch": (C.c_int, [_P(RawJob), C.c_int64, _P(DetectorParams), C.c_int, C.c_uint, _pvp, _pi64, _pi32, _pf64]),
    "sa_raw_event_align_batch": (C.c_int, [_vp, _P(RawJob), _pstr, C.c_int64, _P(DetectorParams), C.c_int, C.c_uint, _pvp, _pi64,
                                           _pvp, _pi64, _pi32, _pf64, _pf64, _pf64]),
    "sa_detect_release": (None, []),
    "sa_npread_from_raw_batch": (C.c_int, [_vp, _P(RawJob), _pstr, C.c_int64, _P(DetectorParams), C.c_int, C.c_uint,
                                           _P(RawNpRead), _pf64]),
    "sa_raw_npread_free": (None, [_P(RawNpRead), C.c_int64]),
    "sa_npread_last_finish_ms": (C.c_double, []),
    "sa_raw_npread_write": (C.c_int, [_P(RawNpRead), _str, _vp, _str]),
    "sa_fasta_subsequence": (C.c_int, [_str, _str, C.c_int64, C.c_int64, C.c_int, _pvp]),
    "sa_format_f6": (C.c_int, [_str, C.c_double]),
    "sa_format_py_round6": (C.c_int, [_str, C.c_double]),
    "sa_pool_configure": (C.c_int, [C.c_int64, C.c_int64]),
    "sa_host_alloc": (_vp, [C.c_size_t]),
    "sa_host_free": (None, [_vp]),
    "sa_pool_release": (None, []),
    "sa_pool_release_device": (None, []),
    "sa_mea_batch": (C.c_int, [_P(MeaJob), C.c_int64, C.c_int, C.c_uint, _pvp, _pi64, _pf64, _pi32, _pi32, _pf64]),
    "sa_mea_release": (None, []),
    "sa_batch_mea": (C.c_int, [_vp, C.c_uint, _pvp, _pi64, _pf64, _pi32, _pf64]),
    "sa_mea_printed_posterior": (C.c_double, [C.c_int64]),
    "sa_mea_printed_posterior_device": (C.c_int, [C.c_int64, C.c_int64, _pf64, C.c_int]),
    "sa_mea_params": (C.c_int64, [_pi64, _pi64, _pf64, C.c_int64, _pi32, _pi32, _pf64, _pi32, _pi64]),
    "sa_batch_site_calls": (C.c_int, [_vp, C.c_uint, _P(_P(SiteCall)), _pi64, _pf64]),
    "sa_batch_position_calls": (C.c_int, [_vp, C.c_uint, _P(_P(PositionCall)), _pi64, _pi32, _pi32, _pf64]),
    "sa_site_calls_records": (C.c_int, [_vp, _P(Job), C.c_int64, _pstr, _pi64, _pi32, _pi32, _pi64, C.c_int, _P(_P(SiteCall)), _pi64, _pf64]),
    "sa_position_calls_records": (C.c_int, [_vp, _P(Job), C.c_int64, _pstr, _pi64, _pi32, _pi32, _pi64, C.c_int, _P(_P(PositionCall)),
                                            _pi64, _pi32, _pi32, _pf64]),
    "sa_snp_substitute": (C.c_int, [_str, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_char, _str]),
    "sa_snp_site_window": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, _pi64, _pi64]),
    "sa_snp_write_read": (C.c_int, [_str, _str, _str, _str, C.c_int, _P(SnpSite), C.c_int64]),
    "sa_snp_marginals_create": (C.c_int, [_pvp, _pi64, C.c_int64, C.c_int64, C.c_int]),
    "sa_snp_marginals_destroy": (None, [_vp]),
    "sa_snp_marginals_add_sites": (C.c_int, [_vp, C.c_int32, C.c_int64, C.c_int, _vp, C.c_int64]),
    "sa_snp_marginals_add_batch": (C.c_int, [_vp, _vp, _P(SnpJobMap), C.c_int64, _pf64]),
    "sa_snp_marginals_checkpoint": (C.c_int, [_vp]),
    "sa_snp_marginals_rollback": (C.c_int, [_vp]),
    "sa_snp_marginals_finish": (C.c_int, [_vp, C.c_int64, _pstr, _pvp, _pi64, _pf64]),
    "sa_snp_group_sites": (C.c_int, [_pi64, _pf64, C.c_int64, C.c_int64, C.c_int, _pi64, _pi64]),
    "sa_snp_substitute_sites": (C.c_int, [_str, C.c_int64, C.c_int64, C.c_int, _pi64, C.c_int64, C.c_char, _str]),
    "sa_snp_apply_calls": (C.c_int, [_str, C.c_int64, _vp, C.c_int64, C.c_int32, _str]),
    "sa_snp_write_marginals": (C.c_int, [_str, _pstr, _vp, C.c_int64]),
    "sa_position_profile_create": (C.c_int, [_pvp, _vp, _pi64, C.c_int64, C.c_int]),
    "sa_position_profile_destroy": (None, [_vp]),
    "sa_position_profile_add_batch": (C.c_int, [_vp, _vp, _P(ProfileJobMap), C.c_int64, C.c_uint, _pf64]),
    "sa_position_profile_add_records": (C.c_int, [_vp, _P(ProfileJobMap), C.c_int64, _pi64, _pi32, _pi32, _pi64, C.c_uint, _pf64]),
    "sa_position_profile_checkpoint": (C.c_int, [_vp]),
    "sa_position_profile_rollback": (C.c_int, [_vp]),
    "sa_position_profile_finish": (C.c_int, [_vp, _pstr, _pvp, _pi64, _P(C.c_uint32), _pf64]),
    "sa_position_profile_write": (C.c_int, [_str, _str, C.c_uint32, _pstr, _vp, C.c_int64]),
    "sa_profile_entropy_term": (C.c_int64, [C.c_int64]),
    "sa_sort_u64": (C.c_int, [_vp, C.c_int64, _vp, C.c_int, _pf64]),
    "sa_call_scores_create": (C.c_int, [_pvp, _str, C.c_int32, C.c_double, _vp, C.c_int64, C.c_int]),
    "sa_call_scores_destroy": (None, [_vp]),
    "sa_call_scores_add_batch": (C.c_int, [_vp, _vp, _P(ScoreJobMap), C.c_int64, _pf64]),
    "sa_call_scores_add_records": (C.c_int, [_vp, C.c_int32, C.c_int32, _pf64, _P(C.c_int8), C.c_int64]),
    "sa_call_scores_checkpoint": (C.c_int, [_vp]),
    "sa_call_scores_rollback": (C.c_int, [_vp]),
    "sa_call_scores_finish": (C.c_int, [_vp, _pvp, _pi64, _pvp, _P(CallScoresCounts), _pf64]),
    "sa_call_scores_write": (C.c_int, [_str, _str, C.c_int32, _vp, C.c_int64, _pi64]),
    "sa_batch_guide_deviation": (C.c_int, [_vp, _P(DeviationJob), C.c_int64, _pvp, _pi64, _P(DeviationParams), C.c_uint, _vp, _pvp,
                                           _pi64, _pi32, _pi64, _pvp, _pf64]),
    "sa_guide_deviation_records": (C.c_int, [_P(DeviationJob), C.c_int64, _pi64, _pi32, _pi32, _pi64, _pvp, _pi64,
                                             _P(DeviationParams), C.c_int, C.c_uint, _vp, _pvp, _pi64, _pi32, _pi64, _pvp, _pf64]),
    "sa_guide_deviation_release": (None, []),
    "sa_batch_signal_labels": (C.c_int, [_vp, _P(LabelJob), C.c_int64, _pvp, _pi64, C.c_uint, _vp, _pvp, _pvp, _pvp, _pvp, _pf64]),
    "sa_signal_labels_records": (C.c_int, [_P(LabelJob), C.c_int64, _pi64, _pi32, _pi32, _pi32, _pi64, _pvp, _pi64, C.c_int, C.c_uint,
                                           _vp, _pvp, _pvp, _pvp, _pvp, _pf64]),
    "sa_signal_labels_release": (None, []),
    "sa_signal_labels_last_kernel_ms": (C.c_int, [_pf64, C.c_int32]),
    "sa_batch_call_quality": (C.c_int, [_vp, _vp, _P(ScoreJobMap), _P(CallqJob), C.c_int64, _pvp, _pi64, _P(CallqParams), C.c_uint, _vp,
                                        _pvp, _pi64, _pvp, _pi64, _pi64, _pi64, _pf64]),
    "sa_call_quality_records": (C.c_int, [_vp, _P(ScoreJobMap), _P(CallqJob), C.c_int64, _pi64, _pi32, _pf64, _P(C.c_uint8), _pi64, _pi32,
                                          _pi32, _pvp, _pi64, _P(CallqParams), C.c_uint, _vp, _pvp, _pi64, _pvp, _pi64, _pi64, _pi64,
                                          _pf64]),
    "sa_call_quality_release": (None, []),
    "sa_call_quality_last_kernel_ms": (C.c_int, [_pf64, C.c_int32]),
    "sa_kmer_table_create": (C.c_int, [_pvp, _vp, C.c_int64, C.c_double, C.c_int]),
    "sa_kmer_table_destroy": (None, [_vp]),
    "sa_kmer_table_add_batch": (C.c_int, [_vp, _vp, _P(Job), C.c_int64, C.c_int, _pf64]),
    "sa_kmer_table_add_rows": (C.c_int, [_vp, C.c_int, _pi32, _pf64, _pf64, C.c_int64]),
    "sa_kmer_table_rows": (C.c_int, [_vp, C.c_int, _pvp, _pi64]),
    "sa_kmer_table_write": (C.c_int, [_vp, C.c_int, _str, C.c_int]),
    "sa_kmer_table_checkpoint": (C.c_int, [_vp]),
    "sa_kmer_table_rollback": (C.c_int, [_vp]),
    "sa_kmer_table_set_positions": (C.c_int, [_vp, _vp, C.c_int64]),
    "sa_kmer_table_add_batch_at": (C.c_int, [_vp, _vp, _P(Job), C.c_int64, C.c_int, _vp, _pf64]),
    "sa_kmer_table_position_counts": (C.c_int, [_vp, _pvp, _pvp, _pi64]),
    "sa_kmer_table_add_at_times": (C.c_int, [_vp, _pf64]),
    "sa_kmer_table_stats": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _pf64]),
    "sa_model_write_trained": (C.c_int, [_str, _vp, C.c_double, C.c_double, C.c_int, _vp, _str]),
    "sa_kmer_table_mixture": (C.c_int, [_vp, C.c_int, _pi32, C.c_int64, _P(MixtureParams), _pf64, _vp, _pf64]),
    "sa_kmer_table_mixture_start": (C.c_int, [_vp, C.c_int, _pi32, C.c_int64, _P(MixtureParams), _pf64]),
    "sa_mixture_assign": (C.c_int, [_vp, C.c_double, _pi32, _pi32, _pf64]),
    "sa_motif_kmer_pairs": (C.c_int, [C.c_int, _str, _str, _str, _pvp, _pi64]),
    "sa_kmer_table_kde": (C.c_int, [_vp, C.c_int, _pi32, C.c_int64, _pf64, C.c_int64, C.c_double, _pf64, _pi64, _pf64]),
    "sa_format_py_repr": (C.c_int, [_str, C.c_double]),
    "sa_f6_units_device": (C.c_int, [_pf64, C.c_int64, _pi64, _pi32, _pi32, C.c_int]),
    "sa_f6_units": (C.c_int, [C.c_double, _pi64, _pi32]),
    "sa_plan_digest": (C.c_int, [_vp, _P(Params), _P(Job), C.c_int64, _pstr, C.c_uint, C.c_int, _P(PlanInfo), _P(C.c_uint64)]),
    "sa_guide_to_anchors": (C.c_int64, [C.c_int64, C.c_int64, C.c_int, C.c_int64, _pi32, _pi64, C.c_int64, C.c_int64, _pi64, _pi64,
                                        C.c_int64]),
    "sa_remap_anchors": (C.c_int64, [_pi64, _pi64, C.c_int64, _pi64, C.c_int64, _pi64, _pi64]),
    "sa_estimate_params": (C.c_int, [_vp, _pf64, _pi64, _pf64, C.c_int64, _str, C.c_int64, _pf64]),
    "sa_guide_align_batch": (C.c_int, [_P(GuideJob), C.c_int64, _P(GuideParams), C.c_int, C.c_uint, _P(GuideResult), _pvp, _pvp,
                                       _pf64]),
    "sa_guide_release": (None, []),
    "sa_guide_seed": (C.c_int, [_str, C.c_int64, _str, C.c_int64, C.c_int, _pi64, _pi32, _pi64, _pi64]),
    "sa_guide_format_cigar": (C.c_int64, [_str, C.c_int64, C.c_int64, _str, C.c_int64, C.c_int64, C.c_int, C.c_int64, _pi32, _pi64,
                                          C.c_int64, _str, C.c_int64]),
    "sa_ref_index_build": (C.c_int, [_pvp, _pstr, _pstr, _pi64, C.c_int64, C.c_int]),
    "sa_ref_index_build_fasta": (C.c_int, [_pvp, _str, C.c_int]),
    "sa_ref_index_info": (C.c_int, [_vp, _P(RefIndexInfo)]),
    "sa_ref_index_entries": (C.c_int, [_vp, _pvp, _pvp, _pvp, _pvp]),
    "sa_ref_index_contig": (C.c_int, [_vp, C.c_int64, _pstr, _pi64, _pi64]),
    "sa_ref_index_destroy": (None, [_vp]),
    "sa_guide_locate_batch": (C.c_int, [_vp, _pstr, _pi64, C.c_int64, _P(LocateParams), C.c_uint, _P(LocateResult), _pf64]),
    "sa_locate_release": (None, []),
    "sa_locate_window": (C.c_int, [_vp, _P(LocateResult), C.c_int64, C.c_int32, _pi64, _pi64]),
    "sa_hdp_state_load": (C.c_int, [_pvp, _str]),
    "sa_hdp_state_write": (C.c_int, [_vp, _str]),
    "sa_hdp_state_info": (C.c_int, [_vp, _P(HdpStateInfo)]),
    "sa_hdp_state_free": (None, [_vp]),
    "sa_hdp_state_distr_sample": (C.c_int, [_vp, C.c_int, _pf64]),
    "sa_hdp_state_sample_weights": (C.c_int, [_vp, _P(_pi64), _P(_pi64), _P(_pf64), _pi64]),
    "sa_hdp_finalize_distributions": (C.c_int, [_pf64, C.c_int64, _pf64, C.c_int64, C.c_int64, C.c_int, _pf64, _pf64]),
    "sa_hmm_create": (C.c_int, [_pvp, _vp, C.c_int, C.c_double, C.c_double, C.c_double]),
    "sa_hmm_destroy": (None, [_vp]),
    "sa_hmm_view": (C.c_int, [_vp, _P(HmmView)]),
    "sa_hmm_set_event_model": (C.c_int, [_vp, _pf64]),
    "sa_hmm_add_expectations": (C.c_int, [_vp, _pf64, C.c_double]),
    "sa_hmm_add_emission_expectation": (C.c_int, [_vp, C.c_int64, C.c_double, C.c_double]),
    "sa_hmm_add_assignment": (C.c_int, [_vp, _str, C.c_double]),
    "sa_hmm_write": (C.c_int, [_vp, _str]),
    "sa_hmm_load": (C.c_int, [_pvp, _str, C.c_int, C.c_double, C.c_double]),
    "sa_hmm_add_expectations_file": (C.c_int, [_vp, _str]),
    "sa_hmm_normalize": (C.c_int, [_vp]),
    "sa_hmm_load_into_model": (C.c_int, [_vp, _vp]),
    "sa_model_transitions10": (C.c_int, [_vp, _pf64]),
    "sa_hdp_state_new": (C.c_int, [_pvp, C.c_int, _str, C.c_int64, _pi64, _pf64, _pf64, _pf64, C.c_double, C.c_double, C.c_int64,
                                   C.c_double, C.c_double, C.c_double, C.c_double]),
    "sa_hdp_state_new_tree": (C.c_int, [_pvp, C.c_int64, C.c_int64, _pi64, _pf64, _pf64, _pf64, C.c_double, C.c_double, C.c_int64,
                                        C.c_double, C.c_double, C.c_double, C.c_double]),
    "sa_hdp_nig_params_from_table": (C.c_int, [_pf64, C.c_int64, _pf64, _pf64, _pf64, _pf64]),
    "sa_hdp_state_pass_data": (C.c_int, [_vp, _pf64, _pi64, C.c_int64]),
    "sa_hdp_state_pass_assignments": (C.c_int, [_vp, _str, _pf64, C.c_int64]),
    "sa_hdp_state_pass_assignment_file": (C.c_int, [_vp, _str, _str, _pi64]),
    "sa_hdp_state_kmer_dp": (C.c_int, [_vp, _str]),
    "sa_hdp_state_gibbs": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_int, C.c_int]),
    "sa_hdp_state_finalize": (C.c_int, [_vp, C.c_int]),
    "sa_hdp_state_samples_taken": (C.c_int64, [_vp]),
    "sa_hdp_digamma": (C.c_double, [C.c_double]),
    "sa_hdp_trigamma": (C.c_double, [C.c_double]),
    "sa_hdp_distances": (C.c_int, [_pf64, C.c_int64, _pf64, C.c_int64, C.c_int, C.c_int, _pf64, _pf64]),
    "sa_hdp_distances_release": (None, []),
    "sa_hdp_distances_paired": (C.c_int, [_pf64, C.c_int64, _pf64, _pf64, C.c_int64, C.c_int, C.c_int, _pf64, _pf64]),
    "sa_hdp_state_densities": (C.c_int, [_vp, _pi64, C.c_int64, _pf64, C.c_int64, C.c_int, _pf64]),
    "sa_hdp_state_distances": (C.c_int, [_vp, C.c_int, C.c_int, _pf64, _pf64]),
    "sa_hdp_state_distance_pairs": (C.c_int, [_vp, C.c_int, _pi64, _pi64, C.c_int64, C.c_int, _pf64]),
    "sa_hdp_state_compare": (C.c_int, [_vp, _pi64, _vp, _pi64, C.c_int64, C.c_int, C.c_int, _pf64]),
    "sa_hdp_state_vs_gaussian": (C.c_int, [_vp, _pi64, C.c_int64, _pf64, _pf64, C.c_int, _vp, _pf64]),
    "sa_hdp_state_alphabet": (C.c_int, [_vp, _str]),
    "sa_device_count": (C.c_int, []),
    "sa_device_memory": (C.c_int, [C.c_int, _pi64, _pi64]),
    "sa_strerror": (_str, [C.c_int]),
    "sa_version": (_str, []),
    "sa_free": (None, [_vp]),
}
IO_SIGNATURES = {      # the loaders of signalalign_amd/csrc/sa_io.h that the package binds: exported, not in the public header
    "sa_rawread_is": (C.c_int, [_str]),
    "sa_rawread_load": (C.c_int, [_str, _P(_P(RawRead))]),
    "sa_rawread_free": (None, [_P(RawRead)]),
    "sa_cigar_load": (C.c_int, [_str, _P(_P(Cigar))]),
    "sa_cigar_free": (None, [_P(Cigar)]),
}
EXPORTS = list(SIGNATURES)     # the public header's functions


def library_path():
    # SA_LIBRARY: load another build of the same ABI (probes/host_asan.sh: the host sources under AddressSanitizer)
    return os.environ.get("SA_LIBRARY") or os.path.join(_HERE, "lib", "libsignalalign_hip.so")


def build(force=False):
    """Compile the HIP library and the CLI in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    so = library_path()
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    srcs.append(os.path.join(_HERE, "..", "include", "signalalign_hip.h"))
    stale = force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs)
    if stale and not os.environ.get("SA_LIBRARY"):
        subprocess.check_call(["make", "-C", _HERE, "-s", "all"])
    return so


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = library_path()
    if not os.path.exists(so):
        raise ImportError("libsignalalign_hip.so is not built (run __graft_entry__.build()); there is no fallback")
    L = C.CDLL(so)
    for table in (SIGNATURES, IO_SIGNATURES):
        for name, (restype, argtypes) in table.items():
            fn = getattr(L, name)       # (a symbol the library lacks is an error here, not at its first call)
            fn.restype, fn.argtypes = restype, argtypes
    _LIB = L
    return L


def _chk(rc, what):
    if rc != 0:
        raise SaError(rc, what)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _copy_out(ptr, shape, dtype, free=True):
    """`shape` records of `dtype` copied out of the library's array at `ptr`, which is then released with sa_free (free=False: it
    stays the library's)"""
    out = np.zeros(shape, dtype=dtype)
    if out.nbytes:
        C.memmove(out.ctypes.data, ptr, out.nbytes)
    if free:
        lib().sa_free(ptr)
    return out


def _timing(stats, kernel_ms, t0=None):
    """kernel_ms -- and call_ms, the C call alone without the wrapper's marshalling, when it was timed from t0 -- into the optional
    stats dict"""
    if stats is not None:
        stats["kernel_ms"] = kernel_ms.value
        if t0 is not None:
            stats["call_ms"] = (time.perf_counter() - t0) * 1e3


def _records(struct, dicts):
    """(a C array of `struct` with one element per dict, filled by the struct's own field list but its padding; their number)"""
    dicts = list(dicts)
    arr = (struct * max(len(dicts), 1))()
    names = [f for f, _ in struct._fields_ if f != "pad"]
    for i, d in enumerate(dicts):
        for f in names:
            setattr(arr[i], f, int(d[f]))
    return arr, len(dicts)


class _Handle:
    """Owner of one library handle (self._h): close() hands it to the class's destroy function (_DESTROY) once, as does collection."""
    _DESTROY = None
    _h = None

    def close(self):
        if self._h:
            getattr(lib(), self._DESTROY)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count():
    return lib().sa_device_count()


def default_params(threshold=0.01, expansion=50, trace_back=100, min_diags=1000, split=3000 * 3000):
    """signalMachine defaults (impl/signalMachine.c:487-490) with the Python driver's -g 100."""
    e = expansion if expansion % 2 == 0 else expansion + 1
    return Params(threshold, e, trace_back, min_diags, split)


def default_ambig(table=None):
    arr = (C.c_char_p * 256)()
    if table is None:
        lib().sa_default_ambig(arr)
    else:
        for k, v in table.items():
            arr[ord(k)] = v.encode()
    return arr


class Model(_Handle):
    """StateMachine3 / StateMachine3_HDP as the C library holds it."""
    _DESTROY = "sa_model_destroy"

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def create(cls, alphabet, k, transitions10, table5, hdp=None):
        h = C.c_void_p()
        t10, tb = _f64(transitions10), _f64(table5)
        _chk(lib().sa_model_create(C.byref(h), 3, alphabet.encode(), k, _dp(t10), _dp(tb), hdp), "sa_model_create")
        return cls(h)

    @classmethod
    def load(cls, model_path, nhdp_path=None):
        h = C.c_void_p()
        _chk(lib().sa_model_load(C.byref(h), model_path.encode(), nhdp_path.encode() if nhdp_path else None),
             "sa_model_load")
        return cls(h)

    def alphabet(self):
        buf = C.create_string_buffer(64)
        na, k = C.c_int(), C.c_int()
        lib().sa_model_alphabet(self._h, buf, C.byref(na), C.byref(k))
        return buf.value.decode(), k.value

    def table5(self):
        alpha, k = self.alphabet()
        n = 5 * len(alpha) ** k
        return np.ctypeslib.as_array(lib().sa_model_table5(self._h), shape=(n,))

    def kmer_id(self, kmer):
        return lib().sa_kmer_id(self._h, kmer.encode())

    def transitions10(self):
        """the model's transitions as the ten tokens of a .model file's second line (linear space)"""
        out = np.zeros(10, dtype=np.float64)
        _chk(lib().sa_model_transitions10(self._h, _dp(out)), "sa_model_transitions10")
        return out

    def set_emission(self, emission):
        """0: MeanOnly (signalMachine's), 1: the two-distribution emission (sa_model_set_emission)."""
        _chk(lib().sa_model_set_emission(self._h, int(emission)), "sa_model_set_emission")

    def clone_with_table(self, table5):
        """sa_model_clone_with_table: the same model with another emission table (a read's own noise scaling)."""
        h = C.c_void_p()
        tb = _f64(table5)
        _chk(lib().sa_model_clone_with_table(C.byref(h), self._h, _dp(tb)), "sa_model_clone_with_table")
        return Model(h)

    def set_to_hdp_expected_values(self):
        _chk(lib().sa_model_set_to_hdp_expected_values(self._h), "sa_model_set_to_hdp_expected_values")


def _make_jobs(jobs):
    """jobs: list of dicts(ref:str, events: (n,) or (n,4) float64, ax, ay, scale, shift, var[, ragged=(left, right)]);
    ragged: the last two arguments of getAlignedPairsUsingAnchors, default (1, 1) as signalMachine passes them."""
    n = len(jobs)
    arr = (Job * max(n, 1))()
    keep = []
    for i, j in enumerate(jobs):
        ev = np.ascontiguousarray(j["events"], dtype=np.float64)
        stride = 1 if ev.ndim == 1 else ev.shape[1]
        ax = np.ascontiguousarray(j["ax"], dtype=np.int64)
        ay = np.ascontiguousarray(j["ay"], dtype=np.int64)
        rb = j["ref"].encode() if isinstance(j["ref"], str) else j["ref"]
        keep.append((ev, ax, ay, rb))
        rl, rr = j.get("ragged", (1, 1))
        arr[i] = Job(rb, len(rb), _dp(ev), stride, ev.shape[0], _ip(ax), _ip(ay), len(ax), j.get("scale", 1.0),
                     j.get("shift", 0.0), j.get("var", 1.0),
                     (0 if rl else JOB_LEFT_END_NOT_RAGGED) | (0 if rr else JOB_RIGHT_END_NOT_RAGGED))
    return arr, keep


class HostBlock(_Handle):
    """sa_host_alloc: one page-locked block; empty(shape, dtype) carves 8-byte aligned numpy arrays out of it (for the event
    records and anchor arrays of jobs passed with FLAG_INPUTS_IN_HOST_BLOCK)."""
    _DESTROY = "sa_host_free"

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self._h = lib().sa_host_alloc(self.nbytes)
        if not self._h:
            raise SaError(-2, "sa_host_alloc")
        self._buf = (C.c_char * self.nbytes).from_address(self._h)
        self._used = 0

    def empty(self, shape, dtype):
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) if np.ndim(shape) else int(shape)
        off = (self._used + 7) & ~7
        if off + n * dt.itemsize > self.nbytes:
            raise ValueError("HostBlock: full")
        self._used = off + n * dt.itemsize
        return np.frombuffer(self._buf, dtype=dt, count=n, offset=off).reshape(shape)

    def close(self):
        self._buf = None
        super().close()


def jobs_bytes_in_block(jobs):
    """Bytes a HostBlock needs for these jobs' event records and anchors."""
    n = 0
    for j in jobs:
        n += (np.asarray(j["events"]).size * 8 + 7) & ~7
        n += 2 * 8 * len(j["ax"])
    return n + 64


class JobArray:
    """A list of jobs marshalled once into the C array sa_batch_create takes (a C caller has it anyway; building it costs
    Python several milliseconds per thousand reads).  Pass it to Batch in place of the list.
    host_block=True: the event records and anchor arrays are copied into one sa_host_alloc block (self.block), as a caller
    that reads its inputs straight into page-locked memory has them; pass FLAG_INPUTS_IN_HOST_BLOCK with it."""

    def __init__(self, jobs, host_block=False, interleaved=False):
        self.n = len(jobs)
        self.block = None
        if host_block:
            self.block = HostBlock(jobs_bytes_in_block(jobs))
            moved = [dict(j) for j in jobs]
            if interleaved:          # read after read: events, anchors, events, ...
                order = [(q, key) for q in moved for key in ("events", "ax", "ay")]
            else:                    # all event records, then all anchors (the library then sends the block in two pieces)
                order = [(q, "events") for q in moved] + [(q, key) for q in moved for key in ("ax", "ay")]
            for q, key in order:
                src = np.asarray(q[key], dtype=np.float64 if key == "events" else np.int64)
                q[key] = self.block.empty(src.shape, src.dtype)
                q[key][...] = src
            jobs = moved
        self.jobs = jobs    # (host_block: the dicts whose arrays live in the block)
        self.arr, self._keep = _make_jobs(jobs)


class Batch(_Handle):
    """sa_batch_t: plan + HBM-resident inputs; run() launches the kernels."""
    _DESTROY = "sa_batch_destroy"

    def __init__(self, model, params, jobs, ambig=None, device=0, flags=0, deferred=False, noise=None):
        """deferred=True: sa_batch_create_deferred (the plan is collected on the batch's first use; the job arrays and the
        ambiguity table are kept alive by this object).
        noise: one (scale_sd, var_sd) per job -- sa_batch_create_noise_scaled (needs FLAG_TWO_DIST_ALL_KERNELS and a
        two-distribution model; not with deferred)."""
        self._h = C.c_void_p()
        if isinstance(jobs, JobArray):
            self.n_jobs, arr, self._keep = jobs.n, jobs.arr, jobs
        else:
            self.n_jobs = len(jobs)
            arr, self._keep = _make_jobs(jobs)
        self._arr = arr   # (KmerTable.add_batch hands the jobs over again)
        amb = ambig if ambig is not None else default_ambig()
        self._amb, self._model = amb, model
        self._flags = int(flags)
        if noise is not None:
            if deferred:
                raise ValueError("Batch: noise= and deferred=True do not go together")
            nz = np.ascontiguousarray(noise, dtype=np.float64).reshape(-1, 2)
            if nz.shape[0] != self.n_jobs:
                raise ValueError("Batch: noise= needs one (scale_sd, var_sd) per job")
            _chk(lib().sa_batch_create_noise_scaled(C.byref(self._h), model._h, C.byref(params), arr, _dp(nz), self.n_jobs, amb, device,
                                                    flags), "sa_batch_create_noise_scaled")
            return
        fn, name = (lib().sa_batch_create_deferred, "sa_batch_create_deferred") if deferred else (lib().sa_batch_create, "sa_batch_create")
        _chk(fn(C.byref(self._h), model._h, C.byref(params), arr, self.n_jobs, amb, device, flags), name)

    def run(self):
        _chk(lib().sa_batch_run(self._h), "sa_batch_run")

    def release_device(self):
        """sa_batch_release_device: the working storage in HBM back to the allocator, the results kept"""
        _chk(lib().sa_batch_release_device(self._h), "sa_batch_release_device")

    def prepare(self):
        """sa_batch_prepare: a deferred batch's plan and launch lists now (while the batch before it runs)."""
        _chk(lib().sa_batch_prepare(self._h), "sa_batch_prepare")

    def start(self):
        """sa_batch_start: run on a library thread; wait() joins it."""
        _chk(lib().sa_batch_start(self._h), "sa_batch_start")

    def wait(self):
        _chk(lib().sa_batch_wait(self._h), "sa_batch_wait")

    def pairs(self, job):
        n = C.c_int64()
        _chk(lib().sa_batch_n_pairs(self._h, job, C.byref(n)), "sa_batch_n_pairs")
        out = np.zeros(n.value, dtype=PAIR_DTYPE)
        if n.value:
            _chk(lib().sa_batch_pairs(self._h, job, out.ctypes.data, n.value), "sa_batch_pairs")
        return out

    def pairs16(self, job):
        """sa_batch_pairs16: the job's packed 16-byte records in place (a view into the batch's pinned result block, valid until
        the batch runs again or is closed): uint64 array [n, 2] of (a, b), see sa_pair16_t."""
        n, ptr = C.c_int64(), C.c_void_p()
        _chk(lib().sa_batch_pairs16(self._h, job, C.byref(ptr), C.byref(n)), "sa_batch_pairs16")
        if n.value == 0:
            return np.zeros((0, 2), dtype=np.uint64)
        buf = (C.c_uint64 * (2 * n.value)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 2)

    def pairs8(self, job):
        """sa_batch_pairs8 (a FLAG_PAIRS8 batch): the job's records decoded into a structured array (x, y, prob_e7)"""
        ptr, n = C.c_void_p(), C.c_int64()
        _chk(lib().sa_batch_pairs8(self._h, job, C.byref(ptr), C.byref(n)), "sa_batch_pairs8")
        out = np.zeros(n.value, dtype=[("x", np.int32), ("y", np.int32), ("prob_e7", np.int64)])
        if n.value:
            r = np.frombuffer((C.c_uint64 * n.value).from_address(ptr.value), dtype=np.uint64)
            out["x"] = (r & np.uint64(0xfffff)).astype(np.int32)
            out["y"] = ((r >> np.uint64(20)) & np.uint64(0xfffff)).astype(np.int32)
            out["prob_e7"] = (r >> np.uint64(40)).astype(np.int64)
        return out

    def results_view(self, first=None):
        """sa_batch_pairs16_all: what a finished batch holds, without copying anything -- (uint64 view [total, 2] of every job's
        packed records, first) with job j's records at view[first[j]:first[j + 1]].  `first`: an int64 array of n_jobs + 1
        entries to reuse.  (A FLAG_PAIRS8 batch: sa_batch_pairs8_all, a view [total, 1].)"""
        if first is None:
            first = np.zeros(self.n_jobs + 1, dtype=np.int64)
        ptr = C.c_void_p()
        if self._flags & FLAG_PAIRS8:
            _chk(lib().sa_batch_pairs8_all(self._h, C.byref(ptr), _ip(first)), "sa_batch_pairs8_all")
            total = int(first[self.n_jobs])
            if total == 0:
                return np.zeros((0, 1), dtype=np.uint64), first
            return np.frombuffer((C.c_uint64 * total).from_address(ptr.value), dtype=np.uint64).reshape(-1, 1), first
        _chk(lib().sa_batch_pairs16_all(self._h, C.byref(ptr), _ip(first)), "sa_batch_pairs16_all")
        total = int(first[self.n_jobs])
        if total == 0:
            return np.zeros((0, 2), dtype=np.uint64), first
        buf = (C.c_uint64 * (2 * total)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 2), first

    def pairs_all(self, out=None):
        """sa_batch_pairs_all: every job's pairs as sa_pair_t, expanded on the library's host threads.  Returns (rows, first)
        with rows[first[j]:first[j + 1]] job j's.  `out`: a PAIR_DTYPE array to reuse (large enough)."""
        first = np.zeros(self.n_jobs + 1, dtype=np.int64)
        rc = lib().sa_batch_pairs_all(self._h, None, 0, _ip(first))
        if rc not in (0, -1):
            _chk(rc, "sa_batch_pairs_all")
        total = int(first[-1])
        if out is None or len(out) < total:
            out = np.empty(total, dtype=PAIR_DTYPE)
        _chk(lib().sa_batch_pairs_all(self._h, out.ctypes.data, len(out), _ip(first)), "sa_batch_pairs_all")
        return out[:total], first

    def all_pairs_summary(self, job):
        """(number of pairs, sum of their prob_e7) over every pair above the threshold -- with FLAG_VC_ROWS including the rows the
        device dropped"""
        n, s = C.c_int64(0), C.c_int64(0)
        _chk(lib().sa_batch_all_pairs_summary(self._h, job, C.byref(n), C.byref(s)), "sa_batch_all_pairs_summary")
        return int(n.value), int(s.value)

    def n_pairs(self, job):
        n = C.c_int64()
        _chk(lib().sa_batch_n_pairs(self._h, job, C.byref(n)), "sa_batch_n_pairs")
        return n.value

    def mea(self, stats=None):
        """sa_batch_mea: the maximum-expected-accuracy path of every read of this (finished) batch, built from the pairs
        that are still on the device.  Returns per job (path [n, 2] of (x, y), best sum, status)."""
        n = self.n_jobs
        ptrs = (C.c_void_p * max(n, 1))()
        cnt = np.zeros(max(n, 1), dtype=np.int64)
        sums = np.zeros(max(n, 1), dtype=np.float64)
        st = np.zeros(max(n, 1), dtype=np.int32)
        kms = C.c_double()
        t0 = time.perf_counter()
        _chk(lib().sa_batch_mea(self._h, 0, ptrs, _ip(cnt), _dp(sums), _i32p(st), C.byref(kms)), "sa_batch_mea")
        _timing(stats, kms, t0)
        return [(_copy_out(ptrs[i], (int(cnt[i]), 2), np.int32), float(sums[i]), int(st[i])) for i in range(n)]

    def site_calls(self, stats=None):
        """sa_batch_site_calls (a batch created with FLAG_SITE_CALLS, after run()): per job a dict of numpy arrays -- x [n] (k-mer
        index of each reported site), letters [n] (its sorted letters as a str), units [n, 8] (printed posterior summed per
        letter, in 1e-6) and prob [n, 8] (units / their sum); columns past a site's letter count are 0."""
        n = self.n_jobs
        ptrs = (C.POINTER(SiteCall) * max(n, 1))()
        cnt = np.zeros(max(n, 1), dtype=np.int64)
        kms = C.c_double()
        t0 = time.perf_counter()
        _chk(lib().sa_batch_site_calls(self._h, 0, ptrs, _ip(cnt), C.byref(kms)), "sa_batch_site_calls")
        _timing(stats, kms, t0)
        return _site_calls_out(ptrs, cnt, n)

    def position_calls(self, stats=None):
        """sa_batch_position_calls (a batch created with FLAG_POSITION_CALLS, after run()): per job a dict -- p [n] (ambiguous
        position in the job's ref), n_rows [n], letters [n] (sorted, as a str), sum [n, 8] (printed posterior summed per letter in
        row order), prob [n, 8] (sum / total); columns past a position's letter count are 0 -- and x_min, x_max (the smallest and
        largest x of the job's records, -1 without records)."""
        n = self.n_jobs
        ptrs = (C.POINTER(PositionCall) * max(n, 1))()
        cnt = np.zeros(max(n, 1), dtype=np.int64)
        xmin = np.zeros(max(n, 1), dtype=np.int32)
        xmax = np.zeros(max(n, 1), dtype=np.int32)
        kms = C.c_double()
        t0 = time.perf_counter()
        _chk(lib().sa_batch_position_calls(self._h, 0, ptrs, _ip(cnt), _i32p(xmin), _i32p(xmax), C.byref(kms)),
             "sa_batch_position_calls")
        _timing(stats, kms, t0)
        return _position_calls_out(ptrs, cnt, xmin, xmax, n)

    def stats(self):
        s = BatchStats()
        _chk(lib().sa_batch_stats(self._h, C.byref(s)), "sa_batch_stats")
        return s


def _site_calls_out(ptrs, cnt, n):
    """the per-job dicts of Batch.site_calls / site_calls_records from the library's arrays, which are released"""
    out = []
    for i in range(n):
        rec = _copy_out(ptrs[i], int(cnt[i]), SITE_CALL_DTYPE)
        letters = np.array([b"".join(r["letters"][:r["n_letters"]]).decode() for r in rec], dtype=object)
        out.append({"x": rec["x"].copy(), "letters": letters, "units": rec["units"].copy(), "prob": rec["prob"].copy()})
    return out


def _position_calls_out(ptrs, cnt, xmin, xmax, n):
    """the per-job dicts of Batch.position_calls / position_calls_records from the library's arrays, which are released"""
    out = []
    for i in range(n):
        rec = _copy_out(ptrs[i], int(cnt[i]), POSITION_CALL_DTYPE)
        letters = np.array([b"".join(r["letters"][:r["n_letters"]]).decode() for r in rec], dtype=object)
        out.append({"p": rec["p"].copy(), "n_rows": rec["n_rows"].copy(), "letters": letters, "sum": rec["sum"].copy(),
                    "prob": rec["prob"].copy(), "x_min": int(xmin[i]), "x_max": int(xmax[i])})
    return out


def _calls_records_args(refs, first, x, kmer_id, prob_e7):
    """what site_calls_records and position_calls_records share: jobs of which only ref / ref_len are set, and the record arrays"""
    refs = [r.encode() if isinstance(r, str) else r for r in refs]
    n = len(refs)
    arr = (Job * max(n, 1))()
    for i, r in enumerate(refs):
        arr[i].ref, arr[i].ref_len = r, len(r)
    first, x, kmer_id, prob_e7 = _i64(first), _i32(x), _i32(kmer_id), _i64(prob_e7)
    if len(first) != n + 1 or not (len(x) == len(kmer_id) == len(prob_e7)) or int(first[-1]) != len(x):
        raise ValueError("first: n_jobs + 1 offsets into x, kmer_id and prob_e7, which have one entry per record")
    return n, arr, (refs, first, x, kmer_id, prob_e7)


def site_calls_records(model, refs, first, x, kmer_id, prob_e7, ambig=None, device=0, stats=None):
    """sa_site_calls_records: Batch.site_calls' result from records the caller holds -- refs: one reference per job; job j's records
    are first[j] .. first[j + 1) of x, kmer_id, prob_e7; ambig as Batch takes it"""
    n, arr, keep = _calls_records_args(refs, first, x, kmer_id, prob_e7)
    amb = ambig if ambig is not None else default_ambig()
    ptrs = (C.POINTER(SiteCall) * max(n, 1))()
    cnt = np.zeros(max(n, 1), dtype=np.int64)
    kms = C.c_double()
    t0 = time.perf_counter()
    _chk(lib().sa_site_calls_records(model._h, arr, n, amb, _ip(keep[1]), _i32p(keep[2]), _i32p(keep[3]), _ip(keep[4]), int(device), ptrs,
                                     _ip(cnt), C.byref(kms)), "sa_site_calls_records")
    _timing(stats, kms, t0)
    return _site_calls_out(ptrs, cnt, n)


def position_calls_records(model, refs, first, x, kmer_id, prob_e7, ambig=None, device=0, stats=None):
    """sa_position_calls_records: Batch.position_calls' result from records the caller holds, the arguments as site_calls_records';
    the row order is the records' order within their job"""
    n, arr, keep = _calls_records_args(refs, first, x, kmer_id, prob_e7)
    amb = ambig if ambig is not None else default_ambig()
    ptrs = (C.POINTER(PositionCall) * max(n, 1))()
    cnt = np.zeros(max(n, 1), dtype=np.int64)
    xmin = np.zeros(max(n, 1), dtype=np.int32)
    xmax = np.zeros(max(n, 1), dtype=np.int32)
    kms = C.c_double()
    t0 = time.perf_counter()
    _chk(lib().sa_position_calls_records(model._h, arr, n, amb, _ip(keep[1]), _i32p(keep[2]), _i32p(keep[3]), _ip(keep[4]), int(device), ptrs,
                                         _ip(cnt), _i32p(xmin), _i32p(xmax), C.byref(kms)), "sa_position_calls_records")
    _timing(stats, kms, t0)
    return _position_calls_out(ptrs, cnt, xmin, xmax, n)


def expect_batch(model, params, jobs, ambig=None, device=0, flags=0, pseudocount=0.0):
    """sa_expect_batch: per job the 3x3 transition expectations (from*3+to), the summed log-likelihood and the HDP
    assignments as (reference position, event index) arrays."""
    if isinstance(jobs, JobArray):
        n, arr, keep = jobs.n, jobs.arr, jobs
    else:
        n = len(jobs)
        arr, keep = _make_jobs(jobs)
    amb = ambig if ambig is not None else default_ambig()
    trans = np.full((max(n, 1), 9), pseudocount, dtype=np.float64)
    lik = np.zeros(max(n, 1), dtype=np.float64)
    ptrs = (C.c_void_p * max(n, 1))()
    cnt = np.zeros(max(n, 1), dtype=np.int64)
    _chk(lib().sa_expect_batch(model._h, C.byref(params), arr, n, amb, device, flags, _dp(trans), _dp(lik), ptrs,
                               _ip(cnt)), "sa_expect_batch")
    assigns = [_copy_out(ptrs[j], (int(cnt[j]), 2), np.int64) for j in range(n)]
    del keep
    return trans[:n], lik[:n], assigns


def expect_last_stats():
    """sa_expect_last_stats: BatchStats of this thread's last expect_batch call."""
    s = BatchStats()
    _chk(lib().sa_expect_last_stats(C.byref(s)), "sa_expect_last_stats")
    return s


def plan_describe(model, params, job, ambig=None, flags=0):
    """Host-only view of the plan of ONE job: regions, band rows, traceback segments (no GPU needed)."""
    arr, keep = _make_jobs([job])
    amb = ambig if ambig is not None else default_ambig()
    info = PlanInfo()
    nev = arr[0].n_events
    lx = max(arr[0].ref_len, 0)
    cap_rows = int(lx + nev + 8 * (arr[0].n_anchors + 4))
    regions = np.zeros(4 * (arr[0].n_anchors + 2), dtype=np.int64)
    rows = np.zeros(3 * cap_rows, dtype=np.int64)
    segs = np.zeros(4 * (cap_rows + 16), dtype=np.int64)   # (one segment per diagonal at most)
    _chk(lib().sa_plan_describe(model._h, C.byref(params), arr, amb, flags, C.byref(info), _ip(regions),
                                len(regions) // 4, _ip(rows), cap_rows, _ip(segs), len(segs) // 4), "sa_plan_describe")
    nrow = 0
    reg = regions[:4 * info.n_regions].reshape(-1, 4)
    for r in reg:
        nrow += (r[2] - r[0]) + (r[3] - r[1]) + 1
    return info, reg, rows[:3 * nrow].reshape(-1, 3), segs[:4 * info.n_segments].reshape(-1, 4)


FLAG_RNA = 4


def scalings_mom(model, sequence, event_means, flags=0):
    """sa_scalings_mom: (shift, scale) by the method of moments (impl/eventAligner.c:784-843)."""
    ev = _f64(event_means)
    sb = sequence.encode()
    sh, sc = C.c_double(), C.c_double()
    _chk(lib().sa_scalings_mom(model._h, sb, len(sb), _dp(ev), len(ev), flags, C.byref(sh), C.byref(sc)), "sa_scalings_mom")
    return sh.value, sc.value


def event_align_batch(model, jobs, device=0, flags=0, stats=None):
    """sa_event_align_batch.  jobs: dicts(sequence, event_mean, scale, shift, var=1).  Returns per job
    (kmer_idx array, event_idx array, status); stats (a dict, optional) receives cells per job and the kernel time."""
    n = len(jobs)
    arr = (EaJob * max(n, 1))()
    keep = []
    for i, j in enumerate(jobs):
        ev = _f64(j["event_mean"])
        sb = j["sequence"].encode()
        keep.append((ev, sb))
        arr[i] = EaJob(sb, len(sb), _dp(ev), len(ev), j["scale"], j["shift"], j.get("var", 1.0))
    ptrs = (C.c_void_p * max(n, 1))()
    cnt = np.zeros(max(n, 1), dtype=np.int64)
    st = np.zeros(max(n, 1), dtype=np.int32)
    cells = np.zeros(max(n, 1), dtype=np.float64)
    kms = C.c_double()
    t0 = time.perf_counter()
    _chk(lib().sa_event_align_batch(model._h, arr, n, device, flags, ptrs, _ip(cnt), _i32p(st), _dp(cells), C.byref(kms)),
         "sa_event_align_batch")
    _timing(stats, kms, t0)
    if stats is not None:
        stats["cells"] = cells[:n].copy()
    out = []
    for i in range(n):
        a = _copy_out(ptrs[i], (int(cnt[i]), 2), np.int32)
        out.append((a[:, 0].copy(), a[:, 1].copy(), int(st[i])))
    del keep
    return out


GUIDE_NO_ALIGNMENT, GUIDE_SHORT, GUIDE_BAND_EDGE, GUIDE_EMPTY, GUIDE_TRACE = 1, 2, 4, 8, 16


def guide_params(match=2, mismatch=-4, gap_open=4, gap_extend=2, ambiguous=-1, band=128, min_read_fraction=0.5):
    return GuideParams(match, mismatch, gap_open, gap_extend, ambiguous, band, min_read_fraction)


def guide_align_batch(jobs, params=None, device=0, stats=None):
    """sa_guide_align_batch.  jobs: (read, window) or (read, window, diag) tuples, or dicts(read, ref, diag=0); params: a
    GuideParams (guide_params()) or None for the defaults.  Returns per job a dict(status, score, read_start, read_end,
    ref_start, ref_end, ops) with ops a list of (type, length) in read order -- what guide_to_anchors takes."""
    n = len(jobs)
    arr = (GuideJob * max(n, 1))()
    keep = []
    for i, j in enumerate(jobs):
        if isinstance(j, dict):
            j = (j["read"], j["ref"], j.get("diag", 0))
        rb, wb = j[0].encode("latin-1"), j[1].encode("latin-1")
        keep.append((rb, wb))
        arr[i] = GuideJob(rb, len(rb), wb, len(wb), int(j[2]) if len(j) > 2 else 0)
    res = (GuideResult * max(n, 1))()
    pt, pl = C.c_void_p(), C.c_void_p()
    kms = C.c_double()
    t0 = time.perf_counter()
    _chk(lib().sa_guide_align_batch(arr, n, C.byref(params) if params is not None else None, device, 0, res, C.byref(pt), C.byref(pl),
                                    C.byref(kms)), "sa_guide_align_batch")
    _timing(stats, kms, t0)
    tot = sum(int(res[i].n_ops) for i in range(n))
    ot, ol = _copy_out(pt, tot, np.int32), _copy_out(pl, tot, np.int64)
    out = []
    for i in range(n):
        r = res[i]
        a, z = int(r.op_first), int(r.op_first + r.n_ops)
        out.append(dict(status=int(r.status), score=int(r.score), read_start=int(r.read_start), read_end=int(r.read_end),
                        ref_start=int(r.ref_start), ref_end=int(r.ref_end),
                        ops=[(int(t), int(ln)) for t, ln in zip(ot[a:z], ol[a:z])]))
    del keep
    return out


def guide_release():
    lib().sa_guide_release()


def guide_seed(read, window, try_both_strands=True):
    """sa_guide_seed -> dict(found, diag, reverse, votes, hits)"""
    rb, wb = read.encode("latin-1"), window.encode("latin-1")
    d, v, h, rev = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
    rc = lib().sa_guide_seed(rb, len(rb), wb, len(wb), 1 if try_both_strands else 0, C.byref(d), C.byref(rev), C.byref(v), C.byref(h))
    if rc < 0:
        raise SaError(int(rc), "sa_guide_seed")
    return dict(found=rc == 0, diag=int(d.value), reverse=bool(rev.value), votes=int(v.value), hits=int(h.value))


def guide_format_cigar(label, read_start, read_end, contig, ref_start, ref_end, forward, score, ops):
    """sa_guide_format_cigar: the exonerate line (no newline) of an alignment; ref_start < ref_end are forward-strand contig
    coordinates"""
    t = np.array([o[0] for o in ops], dtype=np.int32)
    ln = np.array([o[1] for o in ops], dtype=np.int64)
    args = (label.encode(), read_start, read_end, contig.encode(), ref_start, ref_end, 1 if forward else 0, int(score), _i32p(t), _ip(ln), len(ops))
    need = lib().sa_guide_format_cigar(*args, None, 0)
    if need < 0:
        raise SaError(int(need), "sa_guide_format_cigar")
    buf = C.create_string_buffer(int(need) + 1)
    lib().sa_guide_format_cigar(*args, buf, need + 1)
    return buf.value.decode()


LOCATE_NONE, LOCATE_AMBIGUOUS, LOCATE_OVERFLOW, LOCATE_EMPTY = 1, 2, 4, 8
LOCATE_FIELDS = ("status", "contig", "reverse", "pos", "key", "votes", "second_votes", "hits", "seeds", "repetitive")


class RefIndex(_Handle):
    """sa_ref_index_t: the 15-mer index of a whole reference (device < 0: host only)"""
    _DESTROY = "sa_ref_index_destroy"

    def __init__(self, handle):
        self._h = handle

    def contig(self, i):
        """(name, start in the concatenation, length)"""
        name, start, ln = C.c_char_p(), C.c_int64(), C.c_int64()
        _chk(lib().sa_ref_index_contig(self._h, i, C.byref(name), C.byref(start), C.byref(ln)), "sa_ref_index_contig")
        return name.value.decode(), int(start.value), int(ln.value)


def ref_index_build(names, seqs, device=0, lens=None):
    """sa_ref_index_build over (name, sequence) lists; lens overrides the sequences' own lengths (the argument checks)"""
    n = len(names)
    nb = [x.encode("latin-1") if x is not None else None for x in names]
    sb = [x.encode("latin-1") if x is not None else None for x in seqs]
    na, sq = (C.c_char_p * max(n, 1))(*nb), (C.c_char_p * max(n, 1))(*sb)
    ln = (C.c_int64 * max(n, 1))(*(lens if lens is not None else [len(x) for x in sb]))
    h = C.c_void_p()
    _chk(lib().sa_ref_index_build(C.byref(h), na, sq, ln, n, device), "sa_ref_index_build")
    return RefIndex(h)


def ref_index_build_fasta(path, device=0):
    h = C.c_void_p()
    _chk(lib().sa_ref_index_build_fasta(C.byref(h), path.encode(), device), "sa_ref_index_build_fasta")
    return RefIndex(h)


def ref_index_info(index):
    """sa_ref_index_info -> dict(n_contigs, total_bases, n_entries, q, device, host_bytes, device_bytes, build_seconds)"""
    info = RefIndexInfo()
    _chk(lib().sa_ref_index_info(index._h, C.byref(info)), "sa_ref_index_info")
    return {f: getattr(info, f) for f, _ in RefIndexInfo._fields_}


def ref_index_entries(index):
    """sa_ref_index_entries -> dict(codes uint32, pos int32, table int32, starts int64): copies of the host arrays"""
    info = ref_index_info(index)
    p = [C.c_void_p() for _ in range(4)]
    _chk(lib().sa_ref_index_entries(index._h, *[C.byref(x) for x in p]), "sa_ref_index_entries")
    shapes = ((info["n_entries"], np.uint32), (info["n_entries"], np.int32), ((1 << info["q"]) + 1, np.int32), (info["n_contigs"] + 1, np.int64))
    out = [_copy_out(ptr, n, dt, free=False) for ptr, (n, dt) in zip(p, shapes)]      # (the arrays stay the index's)
    return dict(codes=out[0], pos=out[1], table=out[2], starts=out[3], q=int(info["q"]), total=int(info["total_bases"]))


def locate_params(read_bases=2000, max_occ=32, span=128, min_votes=8, max_hits=8192):
    return LocateParams(read_bases, max_occ, span, min_votes, max_hits)


def guide_locate_batch(index, reads, params=None, stats=None):
    """sa_guide_locate_batch: per read a dict of sa_locate_result_t's fields (LOCATE_FIELDS); params: a LocateParams or None"""
    n = len(reads)
    rb = [r.encode("latin-1") for r in reads]
    arr = (C.c_char_p * max(n, 1))(*rb)
    ln = (C.c_int64 * max(n, 1))(*[len(r) for r in rb])
    res = (LocateResult * max(n, 1))()
    kms = C.c_double()
    t0 = time.perf_counter()
    _chk(lib().sa_guide_locate_batch(index._h, arr, ln, n, C.byref(params) if params is not None else None, 0, res, C.byref(kms)),
         "sa_guide_locate_batch")
    _timing(stats, kms, t0)
    return [{f: int(getattr(res[i], f)) for f in LOCATE_FIELDS} for i in range(n)]


def locate_release():
    lib().sa_locate_release()


def locate_window(index, result, read_len, band=128):
    """sa_locate_window -> (start, end) in the contig's coordinates"""
    r = LocateResult(**{f: result[f] for f in LOCATE_FIELDS})
    a, b = C.c_int64(), C.c_int64()
    _chk(lib().sa_locate_window(index._h, C.byref(r), read_len, band, C.byref(a), C.byref(b)), "sa_locate_window")
    return int(a.value), int(b.value)


def cigar_load(path):
    """sa_cigar_load -> dict(contig1, contig2, start1, end1, start2, end2, strand1, strand2, score, ops)"""
    pc = C.POINTER(Cigar)()
    _chk(lib().sa_cigar_load(path.encode(), C.byref(pc)), "sa_cigar_load")
    c = pc.contents
    out = dict(contig1=c.contig1.decode(), contig2=c.contig2.decode(), start1=int(c.start1), end1=int(c.end1), start2=int(c.start2),
               end2=int(c.end2), strand1=int(c.strand1), strand2=int(c.strand2), score=float(c.score),
               ops=[(int(c.op_type[i]), int(c.op_len[i])) for i in range(c.n_ops)])
    lib().sa_cigar_free(pc)
    return out


def _raw_jobs(jobs):
    """jobs: dicts(raw int16 array, digitisation, offset, range, sample_rate, start_time)"""
    n = len(jobs)
    arr = (RawJob * max(n, 1))()
    keep = []
    for i, j in enumerate(jobs):
        raw = np.ascontiguousarray(j["raw"], dtype=np.int16)
        keep.append(raw)
        arr[i] = RawJob(raw.ctypes.data_as(_P(C.c_int16)), len(raw), j["digitisation"], j["offset"], j["range"],
                        j["sample_rate"], j["start_time"])
    return arr, keep


def _detector_params(params):
    return None if params is None else C.byref(DetectorParams(*params))


def detect_events_batch(jobs, params=None, rna=False, device=0, stats=None):
    """sa_detect_events_batch: one RAW_EVENT_DTYPE array per read (time order).  params: (window_length1, window_length2,
    threshold1, threshold2, peak_height), default DETECTOR_DNA / DETECTOR_RNA; stats (a dict, optional) receives the
    per-read status words (RAW_NO_PEAK) and the kernel time."""
    n = len(jobs)
    arr, keep = _raw_jobs(jobs)
    ptrs = (C.c_void_p * max(n, 1))()
    cnt = np.zeros(max(n, 1), dtype=np.int64)
    st = np.zeros(max(n, 1), dtype=np.int32)
    kms = C.c_double()
    _chk(lib().sa_detect_events_batch(arr, n, _detector_params(params), device, FLAG_RNA if rna else 0, ptrs, _ip(cnt), _i32p(st),
                                      C.byref(kms)), "sa_detect_events_batch")
    del keep
    _timing(stats, kms)
    if stats is not None:
        stats["status"] = st[:n].copy()
    return [_copy_out(ptrs[i], int(cnt[i]), RAW_EVENT_DTYPE) for i in range(n)]


def raw_event_align_batch(model, jobs, sequences, rna=False, params=None, device=0, stats=None):
    """sa_raw_event_align_batch (load_from_raw2 for a batch).  Returns per read a dict: events (RAW_EVENT_DTYPE, time
    order), model_state (k-mer string per event, "" unmapped), kmer_idx / event_idx (the event aligner's pairs, event
    indices in the aligned order: reversed for RNA), status, shift, scale."""
    n = len(jobs)
    arr, keep = _raw_jobs(jobs)
    seqs = [s.encode() for s in sequences]
    sp = (C.c_char_p * max(n, 1))(*seqs)
    ev_p, pr_p = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))()
    ev_n, pr_n = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
    st = np.zeros(max(n, 1), dtype=np.int32)
    sh, sc = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    kms = C.c_double()
    _chk(lib().sa_raw_event_align_batch(model._h, arr, sp, n, _detector_params(params), device, FLAG_RNA if rna else 0, ev_p,
                                        _ip(ev_n), pr_p, _ip(pr_n), _i32p(st), _dp(sh), _dp(sc), C.byref(kms)),
         "sa_raw_event_align_batch")
    del keep
    _timing(stats, kms)
    k = model.alphabet()[1]
    out = []
    for i in range(n):
        ev = _copy_out(ev_p[i], int(ev_n[i]), RAW_EVENT_DTYPE)
        a = _copy_out(pr_p[i], (int(pr_n[i]), 2), np.int32)
        seq = sequences[i].replace("U", "T") if rna else sequences[i]
        kmers = [seq[p:p + k][::-1] if rna else seq[p:p + k] for p in range(len(seq) - k + 1)]
        ms = [kmers[x] if x >= 0 else "" for x in ev["kmer_idx"].tolist()]
        out.append(dict(events=ev, model_state=ms, kmer_idx=a[:, 0].copy(), event_idx=a[:, 1].copy(), status=int(st[i]),
                        shift=float(sh[i]), scale=float(sc[i])))
    return out


def detect_release():
    lib().sa_detect_release()


def npread_from_raw_batch(model, jobs, sequences, params=None, device=0, flags=0, stats=None, write=None):
    """sa_npread_from_raw_batch: per read a dict with status, read_len, shift, scale and -- when status is 0 -- events4
    (n x 4: mean, stdv, length, start - start of row 0), kmer_idx, move, p_model_state, raw_start, raw_length and
    strand_event_map; a failed read has None in their place.  write: optional list of paths (None to skip a read) that
    sa_raw_npread_write writes before the results are released.  stats (a dict, optional): kernel_ms and finish_ms
    (k_raw_finish alone)."""
    n = len(jobs)
    arr, keep = _raw_jobs(jobs)
    seqs = [s.encode() for s in sequences]
    sp = (C.c_char_p * max(n, 1))(*seqs)
    res = (RawNpRead * max(n, 1))()
    kms = C.c_double()
    _chk(lib().sa_npread_from_raw_batch(model._h, arr, sp, n, _detector_params(params), device, flags, res, C.byref(kms)),
         "sa_npread_from_raw_batch")
    del keep
    _timing(stats, kms)
    if stats is not None:
        stats["finish_ms"] = lib().sa_npread_last_finish_ms()
    out = []
    try:
        for i in range(n):
            r = res[i]
            d = dict(status=int(r.status), read_len=int(r.read_len), shift=float(r.mom_shift), scale=float(r.mom_scale),
                     n_events=int(r.n_events))
            ne = int(r.n_events)
            for name, width in (("events4", 4), ("kmer_idx", 1), ("move", 1), ("p_model_state", 1), ("raw_start", 1),
                                ("raw_length", 1), ("strand_event_map", 0)):
                ptr = getattr(r, name)
                if not ptr:
                    d[name] = None
                    continue
                cnt = int(r.read_len) if width == 0 else ne * width
                a = np.ctypeslib.as_array(ptr, shape=(cnt,)).copy()
                d[name] = a.reshape(ne, 4) if width == 4 else a
            out.append(d)
            if write is not None and write[i] is not None:
                _chk(lib().sa_raw_npread_write(C.byref(r), seqs[i], model._h, os.fsencode(write[i])), "sa_raw_npread_write")
    finally:
        lib().sa_raw_npread_free(res, n)
    return out


def rawread_load(path):
    """sa_rawread_load (the CLI's loader of a raw-read file): dict(raw, digitisation, offset, range, sample_rate, start_time,
    sequence); raises SaError as the loader refuses."""
    pr = C.POINTER(RawRead)()
    _chk(lib().sa_rawread_load(os.fsencode(path), C.byref(pr)), "sa_rawread_load")
    r = pr.contents
    out = dict(raw=np.ctypeslib.as_array(r.samples, shape=(int(r.n_samples),)).copy(), digitisation=float(r.digitisation),
               offset=float(r.offset), range=float(r.range), sample_rate=float(r.sample_rate), start_time=float(r.start_time),
               sequence=C.string_at(r.sequence, int(r.seq_len)).decode())
    lib().sa_rawread_free(pr)
    return out


def mea_batch(jobs, device=0, flags=0, stats=None):
    """sa_mea_batch.  jobs: dicts(event_idx, ref_idx, posterior, shortest) -- the COO posterior matrix and
    shortest_ref_per_event (np.inf or MEA_INF for events without rows).  Returns per job (path [n, 2] of (ref, event),
    best sum, status, number of final forward edges)."""
    n = len(jobs)
    arr = (MeaJob * max(n, 1))()
    keep = []
    for i, j in enumerate(jobs):
        ev, rf, po = _i32(j["event_idx"]), _i32(j["ref_idx"]), _f64(j["posterior"])
        sh = np.asarray(j["shortest"], dtype=np.float64)
        sh = np.ascontiguousarray(np.where(np.isfinite(sh), sh, MEA_INF).astype(np.int32))
        keep.append((ev, rf, po, sh))
        arr[i] = MeaJob(_i32p(ev), _i32p(rf), _dp(po), len(ev), _i32p(sh), len(sh))
    ptrs = (C.c_void_p * max(n, 1))()
    cnt = np.zeros(max(n, 1), dtype=np.int64)
    sums = np.zeros(max(n, 1), dtype=np.float64)
    st = np.zeros(max(n, 1), dtype=np.int32)
    ne = np.zeros(max(n, 1), dtype=np.int32)
    kms = C.c_double()
    t0 = time.perf_counter()
    _chk(lib().sa_mea_batch(arr, n, device, flags, ptrs, _ip(cnt), _dp(sums), _i32p(st), _i32p(ne), C.byref(kms)), "sa_mea_batch")
    _timing(stats, kms, t0)
    out = [(_copy_out(ptrs[i], (int(cnt[i]), 2), np.int32), float(sums[i]), int(st[i]), int(ne[i])) for i in range(n)]
    del keep
    return out


def mea_params(reference_index, event_index, posterior):
    """sa_mea_params: event-table columns -> (event_idx, ref_idx, posterior, shortest_ref_per_event)."""
    ri, ei, po = _i64(reference_index), _i64(event_index), _f64(posterior)
    n = len(ri)
    rows = np.zeros(max(n, 1), dtype=np.int32)
    cols = np.zeros(max(n, 1), dtype=np.int32)
    data = np.zeros(max(n, 1), dtype=np.float64)
    sh = np.zeros(int(ei.max() - ei.min() + 1) if n else 1, dtype=np.int32)
    ne = C.c_int64()
    m = lib().sa_mea_params(_ip(ri), _ip(ei), _dp(po), n, _i32p(rows), _i32p(cols), _dp(data), _i32p(sh), C.byref(ne))
    if m < 0:
        _chk(int(m), "sa_mea_params")
    return rows[:m].copy(), cols[:m].copy(), data[:m].copy(), sh


def plan_digest(model, params, jobs, ambig=None, flags=0, threads=0):
    """Host-only: plan a batch with `threads` planner threads; returns (PlanInfo, digest of everything uploaded)."""
    arr, keep = _make_jobs(jobs)
    amb = ambig if ambig is not None else default_ambig()
    info, dig = PlanInfo(), C.c_uint64()
    _chk(lib().sa_plan_digest(model._h, C.byref(params), arr, len(jobs), amb, flags, threads, C.byref(info), C.byref(dig)),
         "sa_plan_digest")
    del keep
    return info, dig.value


def guide_to_anchors(start1, end1, strand1, start2, ops, trim):
    t = np.array([o[0] for o in ops], dtype=np.int32)
    ln = np.array([o[1] for o in ops], dtype=np.int64)
    cap = int(ln.sum()) + 1
    ax, ay = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64)
    n = lib().sa_guide_to_anchors(start1, end1, int(strand1), start2, _i32p(t), _ip(ln), len(t), trim, _ip(ax), _ip(ay), cap)
    if n < 0:
        raise SaError(int(n), "sa_guide_to_anchors")
    return ax[:n].copy(), ay[:n].copy()


def remap_anchors(ax, ay, event_map, map_offset):
    axa, aya, em = _i64(ax), _i64(ay), _i64(event_map)
    ox, oy = np.zeros(len(axa) + 1, dtype=np.int64), np.zeros(len(axa) + 1, dtype=np.int64)
    n = lib().sa_remap_anchors(_ip(axa), _ip(aya), len(axa), _ip(em), map_offset, _ip(ox), _ip(oy))
    if n < 0:
        raise SaError(int(n), "sa_remap_anchors")
    return ox[:n].copy(), oy[:n].copy()


def estimate_params(model, table5, strand_event_map, events4, strand_read):
    em = _i64(strand_event_map)
    out = np.zeros(7, dtype=np.float64)
    _chk(lib().sa_estimate_params(model._h, _dp(table5), _ip(em), _dp(events4), events4.shape[0],
                                  strand_read.encode(), len(strand_read), _dp(out)), "sa_estimate_params")
    return dict(zip(["scale", "shift", "var", "drift", "scale_sd", "var_sd", "shift_sd"], out.tolist()))


def plan_check_path_records(model, params, job, ambig=None):
    """Host-only test hook: (wrong entries, entries checked) of the per-path neighbour records of `job`'s plan."""
    arr, keep = _make_jobs([job])
    amb = ambig if ambig is not None else default_ambig()
    n = C.c_int64(0)
    bad = lib().sa_plan_check_path_records(model._h, C.byref(params), arr, amb, C.byref(n))
    if bad < 0:
        _chk(int(bad), "sa_plan_check_path_records")
    return int(bad), int(n.value)


def dplan_compare(model, params, jobs, ambig=None, device=0, flags=0):
    """Test hook (GPU): 0 when the device planner and the host planner produce identical arrays for `jobs`."""
    if isinstance(jobs, JobArray):
        arr, keep, n = jobs.arr, jobs, jobs.n
    else:
        arr, keep = _make_jobs(jobs)
        n = len(jobs)
    amb = ambig if ambig is not None else default_ambig()
    rc = lib().sa_dplan_compare(model._h, C.byref(params), arr, n, amb, device, flags)
    del keep
    if rc < 0:
        _chk(rc, "sa_dplan_compare")
    return rc


def pool_configure(device_limit_bytes=-1, pinned_limit_bytes=-1):
    """Bounds of what the caching allocators may keep parked between batches (sa_pool_configure); -1 leaves a bound as it is."""
    _chk(lib().sa_pool_configure(int(device_limit_bytes), int(pinned_limit_bytes)), "sa_pool_configure")


def device_memory(device=0):
    """(free bytes, total bytes) of the GPU's HBM; what the library's caching allocator holds counts as free."""
    f, t = C.c_int64(), C.c_int64()
    _chk(lib().sa_device_memory(device, C.byref(f), C.byref(t)), "sa_device_memory")
    return f.value, t.value


HMM_GAUSSIAN, HMM_HDP = 0, 1


class Hmm(_Handle):
    """sa_hmm_t: the expectations object of the EM loop (Hmm / ContinuousPairHmm / HdpHmm, impl/continuousHmm.c).  The numpy arrays
    `transitions`, `event_model`, `event_expectations`, `posteriors`, `observed` are VIEWS of the object's own storage."""
    _DESTROY = "sa_hmm_destroy"

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def create(cls, model, kind=HMM_GAUSSIAN, threshold=0.0, transitions_pseudocount=0.0, emissions_pseudocount=0.0):
        h = C.c_void_p()
        _chk(lib().sa_hmm_create(C.byref(h), model._h, kind, threshold, transitions_pseudocount, emissions_pseudocount),
             "sa_hmm_create")
        return cls(h)

    @classmethod
    def load(cls, path, kind=HMM_GAUSSIAN, transitions_pseudocount=0.0, emissions_pseudocount=0.0):
        h = C.c_void_p()
        _chk(lib().sa_hmm_load(C.byref(h), os.fsencode(path), kind, transitions_pseudocount, emissions_pseudocount), "sa_hmm_load")
        return cls(h)

    def view(self):
        v = HmmView()
        _chk(lib().sa_hmm_view(self._h, C.byref(v)), "sa_hmm_view")
        return v

    def _arr(self, ptr, n, dtype=np.float64):
        if not ptr or n == 0:
            return np.zeros(0, dtype=dtype)
        return np.ctypeslib.as_array(ptr, shape=(int(n),))

    @property
    def transitions(self):
        return self._arr(self.view().transitions, 9).reshape(3, 3)

    @property
    def likelihood(self):
        return float(self.view().likelihood[0])

    @property
    def event_model(self):
        v = self.view()
        return self._arr(v.event_model, 5 * v.n_kmers).reshape(-1, 5)

    @property
    def event_expectations(self):
        v = self.view()
        return self._arr(v.event_expectations, 2 * v.n_kmers).reshape(-1, 2)

    @property
    def posteriors(self):
        v = self.view()
        return self._arr(v.posteriors, v.n_kmers)

    @property
    def observed(self):
        v = self.view()
        return self._arr(v.observed, v.n_kmers, np.uint8)

    def assignments(self):
        """(k-mers as a list of str, event means as an array) of an HdpHmm"""
        v = self.view()
        n, k = int(v.n_assignments), int(v.k)
        if n == 0:
            return [], np.zeros(0)
        raw = C.string_at(v.assignment_kmers, n * k).decode()
        return [raw[i * k:(i + 1) * k] for i in range(n)], np.ctypeslib.as_array(v.assignment_events, shape=(n,)).copy()

    def set_event_model(self, table5):
        t = _f64(table5)
        _chk(lib().sa_hmm_set_event_model(self._h, _dp(t)), "sa_hmm_set_event_model")

    def add_expectations(self, trans9, likelihood):
        t = _f64(trans9).reshape(-1)
        _chk(lib().sa_hmm_add_expectations(self._h, _dp(t), float(likelihood)), "sa_hmm_add_expectations")

    def add_emission_expectation(self, kmer_index, mean, p):
        _chk(lib().sa_hmm_add_emission_expectation(self._h, int(kmer_index), float(mean), float(p)), "sa_hmm_add_emission_expectation")

    def add_assignment(self, kmer, event_mean):
        _chk(lib().sa_hmm_add_assignment(self._h, kmer.encode(), float(event_mean)), "sa_hmm_add_assignment")

    def write(self, path):
        _chk(lib().sa_hmm_write(self._h, os.fsencode(path)), "sa_hmm_write")

    def add_expectations_file(self, path):
        """HMM.add_expectations_file: a read's .expectations file added to this object's accumulators"""
        _chk(lib().sa_hmm_add_expectations_file(self._h, os.fsencode(path)), "sa_hmm_add_expectations_file")

    def normalize(self):
        _chk(lib().sa_hmm_normalize(self._h), "sa_hmm_normalize")

    def load_into_model(self, model):
        _chk(lib().sa_hmm_load_into_model(model._h, self._h), "sa_hmm_load_into_model")


class HdpState(_Handle):
    """The whole state of a serialised NanoporeHDP (sa_hdp_state_*: the deterministic pieces of the HDP rebuild).  Arrays are
    copies (numpy) of the views sa_hdp_state_info hands out."""
    _DESTROY = "sa_hdp_state_free"

    def __init__(self, path=None, _handle=None):
        self._h = _handle if _handle is not None else C.c_void_p()
        if _handle is None:
            _chk(lib().sa_hdp_state_load(C.byref(self._h), os.fsencode(path)), "sa_hdp_state_load")
        self.info = HdpStateInfo()
        self.refresh()

    def refresh(self):
        """the info views again (after a call that changed the state: data passed, a sampling run, finalisation)"""
        _chk(lib().sa_hdp_state_info(self._h, C.byref(self.info)), "sa_hdp_state_info")

    @classmethod
    def new(cls, layout, alphabet, kmer_length, grid, nig, gamma=None, gamma_alpha=None, gamma_beta=None, groups=None):
        """sa_hdp_state_new: a NanoporeHDP without data.  layout: HDP_LAYOUT_*; grid = (start, stop, length); nig = (mu, nu, alpha,
        beta); gamma: fixed concentration parameters by depth, or gamma_alpha / gamma_beta: a Gamma prior on them."""
        h = C.c_void_p()
        g, ga, gb = (None if v is None else _f64(v) for v in (gamma, gamma_alpha, gamma_beta))
        gr = None if groups is None else _i64(groups)
        depth = 2 if int(layout) == HDP_LAYOUT_FLAT else 3   # (the C entry point reads `depth` values of each vector it is given)
        for v in (g, ga, gb):
            if v is not None and len(v) != depth:
                raise SaError(-1, "sa_hdp_state_new: %d concentration parameters for a layout of depth %d" % (len(v), depth))
        if gr is not None and len(gr) != len(alphabet):
            raise SaError(-1, "sa_hdp_state_new: one group per letter of the alphabet")
        _chk(lib().sa_hdp_state_new(C.byref(h), int(layout), alphabet.encode(), int(kmer_length), None if gr is None else _ip(gr),
                                    None if g is None else _dp(g), None if ga is None else _dp(ga), None if gb is None else _dp(gb),
                                    float(grid[0]), float(grid[1]), int(grid[2]), float(nig[0]), float(nig[1]), float(nig[2]), float(nig[3])),
             "sa_hdp_state_new")
        return cls(_handle=h)

    @classmethod
    def new_tree(cls, parents, depth, grid, nig, gamma=None, gamma_alpha=None, gamma_beta=None):
        """sa_hdp_state_new_tree: a plain HierarchicalDirichletProcess over the tree `parents` (-1 for the base DP)"""
        h = C.c_void_p()
        pa = _i64(parents)
        g, ga, gb = (None if v is None else _f64(v) for v in (gamma, gamma_alpha, gamma_beta))
        for v in (g, ga, gb):
            if v is not None and len(v) != int(depth):
                raise SaError(-1, "sa_hdp_state_new_tree: %d concentration parameters for depth %d" % (len(v), int(depth)))
        _chk(lib().sa_hdp_state_new_tree(C.byref(h), len(pa), int(depth), _ip(pa), None if g is None else _dp(g),
                                         None if ga is None else _dp(ga), None if gb is None else _dp(gb), float(grid[0]), float(grid[1]),
                                         int(grid[2]), float(nig[0]), float(nig[1]), float(nig[2]), float(nig[3])), "sa_hdp_state_new_tree")
        return cls(_handle=h)

    def pass_data(self, data, dp_ids):
        d, i = _f64(data), _i64(dp_ids)
        _chk(lib().sa_hdp_state_pass_data(self._h, _dp(d), _ip(i), len(d)), "sa_hdp_state_pass_data")
        self.refresh()

    def pass_assignments(self, kmers, events):
        """(k-mers as a list of str or one concatenated str, event means): hdpHmm_loadFromFile's hand-over"""
        km = kmers if isinstance(kmers, str) else "".join(kmers)
        e = _f64(events)
        _chk(lib().sa_hdp_state_pass_assignments(self._h, km.encode(), _dp(e), len(e)), "sa_hdp_state_pass_assignments")
        self.refresh()

    def pass_assignment_file(self, path, strand=None):
        n = C.c_int64()
        _chk(lib().sa_hdp_state_pass_assignment_file(self._h, os.fsencode(path), None if strand is None else strand.encode(), C.byref(n)),
             "sa_hdp_state_pass_assignment_file")
        self.refresh()
        return n.value

    def kmer_dp(self, kmer):
        return lib().sa_hdp_state_kmer_dp(self._h, kmer.encode())

    def gibbs(self, num_samples, burn_in, thinning, seed=1, device=0, verbose=False):
        _chk(lib().sa_hdp_state_gibbs(self._h, int(num_samples), int(burn_in), int(thinning), int(seed), device, 1 if verbose else 0),
             "sa_hdp_state_gibbs")
        self.refresh()

    def finalize(self, device=0):
        _chk(lib().sa_hdp_state_finalize(self._h, device), "sa_hdp_state_finalize")
        self.refresh()

    def samples_taken(self):
        return int(lib().sa_hdp_state_samples_taken(self._h))

    def write(self, path):
        _chk(lib().sa_hdp_state_write(self._h, os.fsencode(path)), "sa_hdp_state_write")

    def array(self, name):
        """a copy of one of the info views, shaped: per data point, per DP, per factor (f_params: n_factors x 5), post / slope:
        n_observed x grid_length"""
        i = self.info
        n = {"data": i.n_data, "data_dp": i.n_data, "gamma": i.depth, "grid": i.grid_length, "dp_parent": i.num_dps,
             "dp_num_factor_children": i.num_dps, "dp_depth": i.num_dps, "observed": i.num_dps, "row_of_dp": i.num_dps,
             "post": i.n_observed * i.grid_length, "slope": i.n_observed * i.grid_length, "f_type": i.n_factors,
             "f_parent": i.n_factors, "f_ref": i.n_factors, "f_params": 5 * i.n_factors, "f_n_children": i.n_factors}[name]
        p = getattr(i, name)
        a = np.ctypeslib.as_array(p, shape=(int(n),)).copy() if n > 0 else np.zeros(0)
        if name in ("post", "slope"):
            a = a.reshape(int(i.n_observed), int(i.grid_length))
        if name == "f_params":
            a = a.reshape(int(i.n_factors), 5)
        return a

    def sample_weights(self):
        """sa_hdp_state_sample_weights (host code): (row_start, col, w) of one sample's weights, CSR over the observed DPs' rows"""
        rs, col, w, nnz = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_double)(), C.c_int64()
        _chk(lib().sa_hdp_state_sample_weights(self._h, C.byref(rs), C.byref(col), C.byref(w), C.byref(nnz)),
             "sa_hdp_state_sample_weights")
        n = int(nnz.value)
        return _copy_out(rs, int(self.info.n_observed) + 1, np.int64), _copy_out(col, n, np.int64), _copy_out(w, n, np.float64)

    def alphabet(self):
        buf = C.create_string_buffer(64)
        _chk(lib().sa_hdp_state_alphabet(self._h, buf), "sa_hdp_state_alphabet")
        return buf.value.decode()

    def densities(self, dp_ids, x, device=0):
        """sa_hdp_state_densities: dir_proc_density of every DP id at every query point, len(dp_ids) x len(x) (GPU)"""
        ids, q = _i64(dp_ids).ravel(), _f64(x).ravel()
        out = np.empty((len(ids), len(q)), dtype=np.float64)
        _chk(lib().sa_hdp_state_densities(self._h, _ip(ids), len(ids), _dp(q), len(q), device, _dp(out)), "sa_hdp_state_densities")
        return out

    def distances(self, metric, device=0, stats=None):
        """sa_hdp_state_distances: the whole memo over the observed DPs, triangular over the rows of row_of_dp (GPU)"""
        n = int(self.info.n_observed)
        out = np.empty(max(n * (n - 1) // 2, 1), dtype=np.float64)
        ms = C.c_double(0.0)
        _chk(lib().sa_hdp_state_distances(self._h, int(metric), device, _dp(out), C.byref(ms)), "sa_hdp_state_distances")
        _timing(stats, ms)
        return out[:n * (n - 1) // 2]

    def distance_pairs(self, metric, dp1, dp2, device=0):
        """sa_hdp_state_distance_pairs: get_dir_proc_distance for pairs of DP ids (GPU)"""
        a, b = _i64(dp1).ravel(), _i64(dp2).ravel()
        if len(a) != len(b):
            raise SaError(-1, "distance_pairs: as many first ids as second ids")
        out = np.empty(max(len(a), 1), dtype=np.float64)
        _chk(lib().sa_hdp_state_distance_pairs(self._h, int(metric), _ip(a), _ip(b), len(a), device, _dp(out)),
             "sa_hdp_state_distance_pairs")
        return out[:len(a)]

    def compare(self, other, dp1, dp2, metric, device=0):
        """sa_hdp_state_compare: compare_hdp_distrs, this state's grid is the master (GPU)"""
        a, b = _i64(dp1).ravel(), _i64(dp2).ravel()
        if len(a) != len(b):
            raise SaError(-1, "compare: as many first ids as second ids")
        out = np.empty(max(len(a), 1), dtype=np.float64)
        _chk(lib().sa_hdp_state_compare(self._h, _ip(a), other._h, _ip(b), len(a), int(metric), device, _dp(out)), "sa_hdp_state_compare")
        return out[:len(a)]

    def vs_gaussian(self, dp_ids, mean, sd, device=0, stats=None):
        """sa_hdp_state_vs_gaussian: structured array (HDP_GAUSS_CMP_DTYPE), entry i the stored distribution of DP dp_ids[i]
        against the normal density (mean[i], sd[i]) on the state's grid (GPU).  stats (a dict): kernel_ms"""
        ids, m, s = _i64(dp_ids).ravel(), _f64(mean).ravel(), _f64(sd).ravel()
        if not len(ids) == len(m) == len(s):
            raise SaError(-1, "vs_gaussian: one mean and one sd per DP id")
        out = np.zeros(max(len(ids), 1), dtype=HDP_GAUSS_CMP_DTYPE)
        ms = C.c_double(0.0)
        _chk(lib().sa_hdp_state_vs_gaussian(self._h, _ip(ids), len(ids), _dp(m), _dp(s), device, out.ctypes.data, C.byref(ms)),
             "sa_hdp_state_vs_gaussian")
        _timing(stats, ms)
        return out[:len(ids)]

    def distr_sample(self, device=0):
        """sa_hdp_state_distr_sample: what one sample of this state adds to every observed DP's collector (GPU)"""
        out = np.zeros((int(self.info.n_observed), int(self.info.grid_length)), dtype=np.float64)
        _chk(lib().sa_hdp_state_distr_sample(self._h, device, _dp(out)), "sa_hdp_state_distr_sample")
        return out


HDP_LAYOUT_FLAT, HDP_LAYOUT_MULTISET, HDP_LAYOUT_MIDDLE_NTS, HDP_LAYOUT_COMPOSITION, HDP_LAYOUT_GROUP_MULTISET = 0, 1, 2, 3, 4
HDP_METRIC_KL, HDP_METRIC_HELLINGER, HDP_METRIC_L2, HDP_METRIC_SHANNON_JENSEN = 0, 1, 2, 3
HDP_GAUSS_CMP_DTYPE = _record_dtype("sa_hdp_gauss_cmp_t", [("kl_bits", "<f8"), ("hellinger", "<f8"), ("mode_delta", "<f8"), ("status", "<i4"), ("pad", "<i4")])


def hdp_distances(grid, rows, metric, device=0, stats=None):
    """sa_hdp_distances: all pairs among the rows (n_rows x grid_length, one grid) -- the triangular vector, [(i - 1) * i / 2 + j]
    for i > j (GPU).  stats (a dict): kernel_ms"""
    g, r = _f64(grid), _f64(rows)
    if r.ndim != 2 or g.ndim != 1 or r.shape[1] != len(g):
        raise SaError(-1, "hdp_distances: rows must be n_rows x len(grid)")
    n = r.shape[0]
    out = np.empty(max(n * (n - 1) // 2, 1), dtype=np.float64)
    ms = C.c_double(0.0)
    _chk(lib().sa_hdp_distances(_dp(g), len(g), _dp(r), n, int(metric), device, _dp(out), C.byref(ms)), "sa_hdp_distances")
    _timing(stats, ms)
    return out[:n * (n - 1) // 2]


def hdp_distances_paired(grid, a, b, metric, device=0, stats=None):
    """sa_hdp_distances_paired: row i of a against row i of b (GPU)"""
    g, pa, pb = _f64(grid), _f64(a), _f64(b)
    if pa.ndim != 2 or pa.shape != pb.shape or g.ndim != 1 or pa.shape[1] != len(g):
        raise SaError(-1, "hdp_distances_paired: a and b must both be n x len(grid)")
    out = np.empty(max(pa.shape[0], 1), dtype=np.float64)
    ms = C.c_double(0.0)
    _chk(lib().sa_hdp_distances_paired(_dp(g), len(g), _dp(pa), _dp(pb), pa.shape[0], int(metric), device, _dp(out), C.byref(ms)),
         "sa_hdp_distances_paired")
    _timing(stats, ms)
    return out[:pa.shape[0]]


def hdp_distances_release():
    lib().sa_hdp_distances_release()


def hdp_nig_params_from_table(table5):
    """sa_hdp_nig_params_from_table: (mu, nu, alpha, beta) by maximum likelihood from a lookup table (5 doubles per k-mer)"""
    t = _f64(table5).reshape(-1)
    out = [C.c_double() for _ in range(4)]
    _chk(lib().sa_hdp_nig_params_from_table(_dp(t), len(t) // 5, *[C.byref(o) for o in out]), "sa_hdp_nig_params_from_table")
    return tuple(o.value for o in out)


def hdp_finalize_distributions(grid, collectors, samples, device=0):
    """sa_hdp_finalize_distributions: (collectors / samples, spline slopes), both n_rows x grid_length (GPU)"""
    grid = _f64(grid)
    s = _f64(collectors).reshape(-1, len(grid))
    y, k = np.zeros_like(s), np.zeros_like(s)
    _chk(lib().sa_hdp_finalize_distributions(_dp(grid), len(grid), _dp(s), s.shape[0], int(samples), device, _dp(y), _dp(k)),
         "sa_hdp_finalize_distributions")
    return y, k


# ---- Gaussian k-mer emission training (sa_kmer_table_*, sa_model_write_trained) ----------------------------------------
KMER_ROW_DTYPE = _record_dtype("sa_kmer_row_t", [("descaled_units", "<i8"), ("run", "<i8"), ("kmer_id", "<i4"), ("prob_units", "<i4"),
                           ("neg_zero", "<i4"), ("pad", "<i4")])
KMER_STAT_DTYPE = _record_dtype("sa_kmer_stat_t", [("n", "<i8"), ("m", "<f8"), ("s", "<f8")])
MIXTURE_FIT_DTYPE = _record_dtype("sa_mixture_fit_t", [("n", "<i8"), ("kmer_id", "<i4"), ("n_iter", "<i4"), ("converged", "<i4"), ("status", "<i4"),
                              ("lower_bound", "<f8"), ("weight", "<f8", (4,)), ("mean", "<f8", (4,)), ("sd", "<f8", (4,))])


class KmerTable(_Handle):
    """sa_kmer_table_t: per strand (0 't', 1 'c') and path k-mer the max_per_kmer rows of largest printed posterior
    (>= min_prob), kept in HBM across add_batch / add_rows calls."""
    _DESTROY = "sa_kmer_table_destroy"

    def __init__(self, model, max_per_kmer=10, min_prob=0.8, device=0):
        self._h = C.c_void_p()
        self._model = model
        _chk(lib().sa_kmer_table_create(C.byref(self._h), model._h, int(max_per_kmer), float(min_prob), int(device)),
             "sa_kmer_table_create")

    def add_batch(self, batch, strand=0, stats=None):
        """the rows of a finished Batch (its own job array supplies event means, scalings and references)"""
        kms = C.c_double()
        _chk(lib().sa_kmer_table_add_batch(self._h, batch._h, batch._arr, batch.n_jobs, int(strand), C.byref(kms)),
             "sa_kmer_table_add_batch")
        _timing(stats, kms)

    def set_positions(self, sites):
        """sa_kmer_table_set_positions: from now on only rows that cover one of `sites` are offered.  sites: a TRAIN_SITE_DTYPE
        array, or an iterable of (contig index, position, site strand 0 '+' / 1 '-')"""
        if isinstance(sites, np.ndarray) and sites.dtype == TRAIN_SITE_DTYPE:
            t = np.ascontiguousarray(sites)
        else:
            sites = list(sites)
            t = np.zeros(len(sites), dtype=TRAIN_SITE_DTYPE)
            for i, (contig, pos, strand) in enumerate(sites):
                t[i]["contig"], t[i]["pos"], t[i]["mapped_strand"] = int(contig), int(pos), int(strand)
        _chk(lib().sa_kmer_table_set_positions(self._h, t.ctypes.data if len(t) else None, len(t)), "sa_kmer_table_set_positions")

    def add_batch_at(self, batch, job_map, strand=0, stats=None):
        """sa_kmer_table_add_batch_at: add_batch on a table with positions; job_map: a TRAIN_JOB_MAP_DTYPE array, or per job a dict
        with the fields of sa_train_job_map_t (contig, x_sign, x0, site_strand)"""
        if isinstance(job_map, np.ndarray) and job_map.dtype == TRAIN_JOB_MAP_DTYPE:
            m = np.ascontiguousarray(job_map)
            mp, n = m.ctypes.data, len(m)
        else:
            mp, n = _records(TrainJobMap, job_map)
        kms = C.c_double()
        _chk(lib().sa_kmer_table_add_batch_at(self._h, batch._h, batch._arr, n, int(strand), mp if n else None, C.byref(kms)),
             "sa_kmer_table_add_batch_at")
        if stats is not None:
            parts = np.zeros(2)
            _chk(lib().sa_kmer_table_add_at_times(self._h, _dp(parts)), "sa_kmer_table_add_at_times")
            stats["kernel_ms"], stats["mask_ms"], stats["counts_ms"] = kms.value, float(parts[0]), float(parts[1])

    def position_counts(self):
        """sa_kmer_table_position_counts: (sites: TRAIN_SITE_DTYPE array in (contig, strand, position) order, counts: int64 array)"""
        sp, cp = C.c_void_p(), C.c_void_p()
        n = np.zeros(1, dtype=np.int64)
        _chk(lib().sa_kmer_table_position_counts(self._h, C.byref(sp), C.byref(cp), _ip(n)), "sa_kmer_table_position_counts")
        return _copy_out(sp, int(n[0]), TRAIN_SITE_DTYPE), _copy_out(cp, int(n[0]), np.int64)

    def add_rows(self, kmer_ids, descaled, prob, strand=0):
        k, d, p = _i32(kmer_ids), _f64(descaled), _f64(prob)
        assert len(k) == len(d) == len(p)
        _chk(lib().sa_kmer_table_add_rows(self._h, int(strand), _i32p(k), _dp(d), _dp(p), len(k)), "sa_kmer_table_add_rows")

    def rows(self, strand=0):
        """structured array (KMER_ROW_DTYPE): k-mer ascending, posterior descending, then run order"""
        ptr = C.c_void_p()
        n = np.zeros(1, dtype=np.int64)
        _chk(lib().sa_kmer_table_rows(self._h, int(strand), C.byref(ptr), _ip(n)), "sa_kmer_table_rows")
        return _copy_out(ptr, int(n[0]), KMER_ROW_DTYPE)

    def write(self, path, strand=-1, append=False):
        _chk(lib().sa_kmer_table_write(self._h, int(strand), os.fsencode(path), int(bool(append))), "sa_kmer_table_write")

    def checkpoint(self):
        _chk(lib().sa_kmer_table_checkpoint(self._h), "sa_kmer_table_checkpoint")

    def rollback(self):
        _chk(lib().sa_kmer_table_rollback(self._h), "sa_kmer_table_rollback")

    def stats(self, strand=0, use_median=False, info=None):
        """structured array (KMER_STAT_DTYPE), one entry per kmer_id"""
        alpha, k = self._model.alphabet()
        nk = len(alpha) ** k
        out = np.zeros(nk, dtype=KMER_STAT_DTYPE)
        kms = C.c_double()
        _chk(lib().sa_kmer_table_stats(self._h, int(strand), int(bool(use_median)), out.ctypes.data, C.byref(kms)),
             "sa_kmer_table_stats")
        _timing(info, kms)
        return out

    def _mixture_args(self, kmer_ids, n_components, max_iter, tol, reg_covar):
        alpha, k = self._model.alphabet()
        ids = None if kmer_ids is None else _i32(kmer_ids)
        nj = len(alpha) ** k if ids is None else len(ids)
        p = MixtureParams(int(n_components), int(max_iter), float(tol), float(reg_covar))
        return ids, nj, p, (None if ids is None else _i32p(ids))

    def mixture(self, kmer_ids=None, n_components=2, strand=0, max_iter=100, tol=1e-3, reg_covar=1e-6, init=None, info=None):
        """sa_kmer_table_mixture: structured array (MIXTURE_FIT_DTYPE), one entry per k-mer id of `kmer_ids` (None: every
        k-mer of the model); init: None or an array n_jobs x 3 x K (weights, means, sds)"""
        ids, nj, p, idp = self._mixture_args(kmer_ids, n_components, max_iter, tol, reg_covar)
        out = np.zeros(nj, dtype=MIXTURE_FIT_DTYPE)
        ini = None
        if init is not None:
            ini = _f64(init).reshape(-1)
            assert len(ini) == nj * 3 * int(n_components)
        kms = C.c_double()
        _chk(lib().sa_kmer_table_mixture(self._h, int(strand), idp, nj, C.byref(p), None if ini is None else _dp(ini),
                                         out.ctypes.data, C.byref(kms)), "sa_kmer_table_mixture")
        _timing(info, kms)
        return out

    def mixture_start(self, kmer_ids=None, n_components=2, strand=0, reg_covar=1e-6):
        """sa_kmer_table_mixture_start: the default start of every job, n_jobs x 3 x K (weights, means, sds)"""
        ids, nj, p, idp = self._mixture_args(kmer_ids, n_components, 1, 0.0, reg_covar)
        out = np.zeros((nj, 3, int(n_components)), dtype=np.float64)
        _chk(lib().sa_kmer_table_mixture_start(self._h, int(strand), idp, nj, C.byref(p), _dp(out)), "sa_kmer_table_mixture_start")
        return out

    def kde(self, x, kmer_ids=None, bandwidth=0.5, strand=0, info=None):
        """sa_kmer_table_kde: the log density of a Gaussian kernel density estimate over each k-mer's rows at the query points x,
        n_jobs x len(x), one row per k-mer id of `kmer_ids` (None: every k-mer of the model); -inf for a k-mer without rows.
        info (a dict): kernel_ms, n_rows (per job)"""
        alpha, k = self._model.alphabet()
        ids = None if kmer_ids is None else _i32(kmer_ids).ravel()
        nj = len(alpha) ** k if ids is None else len(ids)
        q = _f64(x).ravel()
        out = np.empty((nj, len(q)), dtype=np.float64)
        n_rows = np.zeros(max(nj, 1), dtype=np.int64)
        kms = C.c_double()
        _chk(lib().sa_kmer_table_kde(self._h, int(strand), None if ids is None else _i32p(ids), nj, _dp(q), len(q), float(bandwidth),
                                     _dp(out), _ip(n_rows), C.byref(kms)), "sa_kmer_table_kde")
        _timing(info, kms)
        if info is not None:
            info["n_rows"] = n_rows[:nj]
        return out


def model_write_trained(prior_path, stats, out_path, weight=100.0, min_sd=0.0, mod_only=False, kmer_mask=None):
    st = np.ascontiguousarray(stats, dtype=KMER_STAT_DTYPE)
    mask = None if kmer_mask is None else np.ascontiguousarray(kmer_mask, dtype=np.uint8)
    _chk(lib().sa_model_write_trained(os.fsencode(prior_path), st.ctypes.data, float(weight), float(min_sd), int(bool(mod_only)),
                                      None if mask is None else mask.ctypes.data, os.fsencode(out_path)), "sa_model_write_trained")


def mixture_assign(fit, canonical_mean):
    """sa_mixture_assign: (match, other, distance) of one fitted two-component entry of KmerTable.mixture"""
    f = np.ascontiguousarray(fit, dtype=MIXTURE_FIT_DTYPE).reshape(1)
    a, b, d = C.c_int32(), C.c_int32(), C.c_double()
    _chk(lib().sa_mixture_assign(f.ctypes.data, float(canonical_mean), C.byref(a), C.byref(b), C.byref(d)), "sa_mixture_assign")
    return int(a.value), int(b.value), float(d.value)


def motif_kmer_pairs(k, canonical_motif, modified_motif, alphabet=None):
    """sa_motif_kmer_pairs: sorted list of (canonical k-mer, modified k-mer)"""
    ptr = C.c_void_p()
    n = np.zeros(1, dtype=np.int64)
    _chk(lib().sa_motif_kmer_pairs(int(k), canonical_motif.encode(), modified_motif.encode(),
                                   None if alphabet is None else alphabet.encode(), C.byref(ptr), _ip(n)), "sa_motif_kmer_pairs")
    raw = C.string_at(ptr, int(n[0]) * 2 * (int(k) + 1)) if n[0] else b""
    lib().sa_free(ptr)
    w = int(k) + 1
    return [(raw[2 * i * w:2 * i * w + k].decode(), raw[(2 * i + 1) * w:(2 * i + 1) * w + k].decode()) for i in range(int(n[0]))]


def snp_substitute(ref, contig_pos_of_ref0, reversed=False, step=10, phase=0, letter="X"):
    """sa_snp_substitute: `letter` at the window's positions whose contig coordinate is = phase (mod step), the rest upper-cased"""
    b = ref.encode() if isinstance(ref, str) else bytes(ref)
    out = C.create_string_buffer(len(b) + 1)
    _chk(lib().sa_snp_substitute(b, len(b), int(contig_pos_of_ref0), 1 if reversed else 0, int(step), int(phase),
                                 letter.encode()[:1], out), "sa_snp_substitute")
    return out.raw[:len(b)].decode()


def snp_site_window(min_ref_index, max_ref_index, step):
    """sa_snp_site_window: (lo, hi) of the sites call_methyls visits with a step offset"""
    lo, hi = C.c_int64(), C.c_int64()
    _chk(lib().sa_snp_site_window(int(min_ref_index), int(max_ref_index), int(step), C.byref(lo), C.byref(hi)), "sa_snp_site_window")
    return int(lo.value), int(hi.value)


def snp_write_read(path, fast5_input, read_id, contig, backward, sites):
    """sa_snp_write_read: `sites` an iterable of (pos, strand 0/1, (pA, pC, pG, pT)), the step files' lines in file order"""
    sites = list(sites)
    arr = (SnpSite * max(len(sites), 1))()
    for i, (pos, strand, p) in enumerate(sites):
        arr[i].pos, arr[i].strand = int(pos), int(strand)
        for q in range(4):
            arr[i].p[q] = float(p[q])
    _chk(lib().sa_snp_write_read(path.encode(), fast5_input.encode(), read_id.encode(), contig.encode(), 1 if backward else 0,
                                 arr, len(sites)), "sa_snp_write_read")


class _ContigAcc(_Handle):
    """What the tables kept in HBM over contig positions share: the lengths, checkpoint / rollback / close by the prefix of the
    C functions' names (_PREFIX), and the two ends of finish."""
    _PREFIX = None

    _DESTROY = property(lambda self: self._PREFIX + "destroy")

    def _create(self, contig_lens, create):
        """create(handle by reference, lengths, their number) is the table's own sa_*_create call"""
        self._h = C.c_void_p()
        lens = _i64(contig_lens)
        self.n_contigs = len(lens)
        self.contig_lens = [int(v) for v in lens]
        _chk(create(C.byref(self._h), _ip(lens), len(lens)), self._PREFIX + "create")

    def _call(self, name):
        _chk(getattr(lib(), self._PREFIX + name)(self._h), self._PREFIX + name)

    def checkpoint(self):
        self._call("checkpoint")

    def rollback(self):
        self._call("rollback")

    def _refs(self, ref_by_contig):
        """ref_by_contig as finish passes it on: NULL, or one C string per contig"""
        if ref_by_contig is None:
            return None
        keep = [r.encode() if isinstance(r, str) else bytes(r) for r in ref_by_contig]
        if len(keep) != self.n_contigs or any(len(r) < n for r, n in zip(keep, self.contig_lens)):
            raise ValueError("ref_by_contig: one sequence per contig, each at least as long as its contig")
        return (C.c_char_p * len(keep))(*keep)

    def _finish(self, dtype, stats, call):
        """call(sites by reference, their number, kernel_ms by reference) is the table's own sa_*_finish call; the sites are
        copied out of the library's array, which is freed"""
        ptr = C.c_void_p()
        n = np.zeros(1, dtype=np.int64)
        kms = C.c_double()
        _chk(call(C.byref(ptr), _ip(n), C.byref(kms)), self._PREFIX + "finish")
        _timing(stats, kms)
        return _copy_out(ptr, int(n[0]), dtype)


class SnpMarginals(_ContigAcc):
    """sa_snp_marginals_t: per contig position a forward and a backward sum of (pA, pC, pG, pT) over reads and a row count,
    kept in HBM across add_sites / add_batch calls.  step >= 1: add_batch filters by call_methyls' window; 0: no window."""
    _PREFIX = "sa_snp_marginals_"

    def __init__(self, contig_lens, step=0, device=0):
        self._create(contig_lens, lambda h, lens, n: lib().sa_snp_marginals_create(h, lens, n, int(step), int(device)))

    def add_sites(self, contig, sites, direction, run=0):
        """rows of one read: `sites` a SNP_SITE_DTYPE array, or an iterable of (pos, strand 0/1, (pA, pC, pG, pT))"""
        if isinstance(sites, np.ndarray) and sites.dtype == SNP_SITE_DTYPE:
            arr = np.ascontiguousarray(sites)
        else:
            sites = list(sites)
            arr = np.zeros(len(sites), dtype=SNP_SITE_DTYPE)
            for i, (pos, strand, p) in enumerate(sites):
                arr[i]["pos"], arr[i]["strand"], arr[i]["p"] = int(pos), int(strand), p
        _chk(lib().sa_snp_marginals_add_sites(self._h, int(contig), int(run), 1 if direction else 0, arr.ctypes.data, len(arr)),
             "sa_snp_marginals_add_sites")

    def add_batch(self, batch, job_map, stats=None):
        """chained onto a finished Batch created with FLAG_POSITION_CALLS; job_map: per job a dict with the fields of
        sa_snp_job_map_t (contig, pos0, pos_sign, x0, x_sign, strand, direction, run, group)"""
        arr, n = _records(SnpJobMap, job_map)
        kms = (C.c_double * 2)()
        _chk(lib().sa_snp_marginals_add_batch(self._h, batch._h, arr, n, kms), "sa_snp_marginals_add_batch")
        if stats is not None:
            stats["kernel_ms_position_fold"], stats["kernel_ms"] = kms[0], kms[1]

    def finish(self, min_depth=1, ref_by_contig=None, stats=None):
        """structured array (SNP_MARGINAL_DTYPE): the sites with rows, in (contig, position) order"""
        refs = self._refs(ref_by_contig)
        return self._finish(SNP_MARGINAL_DTYPE, stats,
                            lambda ptr, n, kms: lib().sa_snp_marginals_finish(self._h, int(min_depth), refs, ptr, n, kms))


class PositionProfile(_ContigAcc):
    """sa_position_profile_t: per contig position the pile-up of all reads' posteriors (multipleAlignmentAnalysis.py) as integer
    sums, kept in HBM across add_batch / add_records calls."""
    _PREFIX = "sa_position_profile_"

    def __init__(self, model, contig_lens, device=0):
        self.alphabet = model.alphabet()[0]
        self._create(contig_lens, lambda h, lens, n: lib().sa_position_profile_create(h, model._h, lens, n, int(device)))

    def add_batch(self, batch, job_map, flags=0, stats=None):
        """chained onto a finished Batch; job_map: per job a dict with contig, pos0, pos_sign (sa_profile_job_map_t)"""
        arr, n = _records(ProfileJobMap, job_map)
        kms = C.c_double()
        _chk(lib().sa_position_profile_add_batch(self._h, batch._h, arr, n, int(flags), C.byref(kms)), "sa_position_profile_add_batch")
        _timing(stats, kms)

    def add_records(self, job_map, first, x, kmer_id, prob_e7, flags=0, stats=None):
        """records from elsewhere: job j's are first[j] .. first[j + 1) of x, kmer_id, prob_e7"""
        arr, n = _records(ProfileJobMap, job_map)
        first, x, kmer_id, prob_e7 = _i64(first), _i32(x), _i32(kmer_id), _i64(prob_e7)
        if len(first) != n + 1 or not (len(x) == len(kmer_id) == len(prob_e7)) or int(first[-1]) != len(x):
            raise ValueError("first: n_jobs + 1 offsets into x, kmer_id and prob_e7, which have one entry per record")
        kms = C.c_double()
        _chk(lib().sa_position_profile_add_records(self._h, arr, n, _ip(first), _i32p(x), _i32p(kmer_id), _ip(prob_e7), int(flags),
                                                   C.byref(kms)), "sa_position_profile_add_records")
        _timing(stats, kms)

    def finish(self, ref_by_contig=None, stats=None):
        """(structured array of PROFILE_SITE_DTYPE in (contig, position) order, letters_seen bit mask)"""
        refs = self._refs(ref_by_contig)
        seen = C.c_uint32()
        out = self._finish(PROFILE_SITE_DTYPE, stats,
                           lambda ptr, n, kms: lib().sa_position_profile_finish(self._h, refs, ptr, n, C.byref(seen), kms))
        return out, int(seen.value)


def position_profile_write(path, alphabet, letters_seen, contig_names, sites):
    """sa_position_profile_write: the file of multipleAlignmentAnalysis.py"""
    m = np.ascontiguousarray(sites, dtype=PROFILE_SITE_DTYPE)
    keep = [c.encode() for c in contig_names]
    names = (C.c_char_p * max(len(keep), 1))(*keep)
    _chk(lib().sa_position_profile_write(os.fsencode(path), alphabet.encode(), int(letters_seen), names, m.ctypes.data, len(m)),
         "sa_position_profile_write")


def profile_entropy_term(units):
    return int(lib().sa_profile_entropy_term(int(units)))


def sort_u64(keys, device=0, stats=None):
    """sa_sort_u64: the keys ascending, sorted on the device"""
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    out = np.empty_like(k)
    kms = C.c_double()
    _chk(lib().sa_sort_u64(k.ctypes.data, len(k), out.ctypes.data, int(device), C.byref(kms)), "sa_sort_u64")
    _timing(stats, kms)
    return out


class CallScores(_Handle):
    """sa_call_scores_t: the scores of site calls against known truth, kept in HBM per (level, read strand, letter, class) across
    add_batch / add_records calls; finish gives AUC, confusion and curve counts per (level, strand group, letter)."""
    _DESTROY = "sa_call_scores_destroy"

    def __init__(self, letters, truth=(), n_bins=1000, threshold=0.500000001, device=0):
        """truth: a TRUTH_SITE_DTYPE array, or an iterable of (contig index, position, mapped strand 0 '+' / 1 '-', change_to)"""
        self._h = C.c_void_p()
        self.letters, self.n_bins, self.threshold = letters, int(n_bins), float(threshold)
        if isinstance(truth, np.ndarray) and truth.dtype == TRUTH_SITE_DTYPE:
            t = np.ascontiguousarray(truth)
        else:
            truth = list(truth)
            t = np.zeros(len(truth), dtype=TRUTH_SITE_DTYPE)
            for i, (contig, pos, mapped, letter) in enumerate(truth):
                t[i]["contig"], t[i]["pos"], t[i]["mapped_strand"], t[i]["change_to"] = int(contig), int(pos), int(mapped), letter.encode()
        _chk(lib().sa_call_scores_create(C.byref(self._h), letters.encode(), self.n_bins, self.threshold, t.ctypes.data, len(t), int(device)),
             "sa_call_scores_create")

    def add_batch(self, batch, job_map, stats=None):
        """chained onto a finished Batch created with FLAG_SITE_CALLS; job_map: per job a dict with the fields of sa_score_job_map_t
        (contig, x0, x_sign, strand, mapped_strand, true_letter)"""
        arr, n = _records(ScoreJobMap, job_map)
        kms = C.c_double()
        _chk(lib().sa_call_scores_add_batch(self._h, batch._h, arr, n, C.byref(kms)), "sa_call_scores_add_batch")
        _timing(stats, kms)

    def add_records(self, level, strand, prob, true_letter):
        """scores made elsewhere: prob n x len(letters), true_letter n indices into letters"""
        prob = _f64(prob).reshape(-1, len(self.letters))
        tl = np.ascontiguousarray(true_letter, dtype=np.int8)
        if len(tl) != len(prob):
            raise ValueError("one true letter per record")
        _chk(lib().sa_call_scores_add_records(self._h, int(level), int(strand), _dp(prob), tl.ctypes.data_as(_P(C.c_int8)), len(tl)),
             "sa_call_scores_add_records")

    def checkpoint(self):
        _chk(lib().sa_call_scores_checkpoint(self._h), "sa_call_scores_checkpoint")

    def rollback(self):
        _chk(lib().sa_call_scores_rollback(self._h), "sa_call_scores_rollback")

    def finish(self, stats=None):
        """(rows: CALL_SCORE_ROW_DTYPE array; curves: int64 array rows x 2 x (n_bins + 1), tp_ge then fp_ge; counts: dict)"""
        rows_p, curves_p = C.c_void_p(), C.c_void_p()
        n = np.zeros(1, dtype=np.int64)
        counts = CallScoresCounts()
        kms = C.c_double()
        _chk(lib().sa_call_scores_finish(self._h, C.byref(rows_p), _ip(n), C.byref(curves_p), C.byref(counts), C.byref(kms)),
             "sa_call_scores_finish")
        rows = _copy_out(rows_p, int(n[0]), CALL_SCORE_ROW_DTYPE)
        curves = _copy_out(curves_p, (int(n[0]), 2, self.n_bins + 1), np.int64)
        _timing(stats, kms)
        return rows, curves, dict(unlabelled=int(counts.unlabelled), other_sites=int(counts.other_sites))


def call_scores_write(summary_path, curves_path, n_bins, rows, curves=None):
    """sa_call_scores_write: the summary and (curves_path not None) the curves of CallScores.finish"""
    r = np.ascontiguousarray(rows, dtype=CALL_SCORE_ROW_DTYPE)
    c = _i64(curves if curves is not None else np.zeros(0))
    _chk(lib().sa_call_scores_write(os.fsencode(summary_path), os.fsencode(curves_path) if curves_path is not None else None, int(n_bins),
                                    r.ctypes.data, len(r), _ip(c)), "sa_call_scores_write")


def _deviation_call(jobs, mea, params, flags, call):
    """what batch_guide_deviation and guide_deviation_records share: the argument arrays, the call, the outputs as a dict"""
    jobs = list(jobs)
    n = len(jobs)
    arr = (DeviationJob * max(n, 1))()
    keep = []
    for i, j in enumerate(jobs):
        ax, ay = _i64(j["ax"]), _i64(j["ay"])
        if len(ax) != len(ay):
            raise ValueError("a job's ax and ay have one entry per anchor")
        keep.append((ax, ay))
        arr[i] = DeviationJob(_ip(ax), _ip(ay), len(ax), int(j["n_events"]))
    paths, n_mea = None, None
    if mea is not None:
        if len(mea) != n:
            raise ValueError("mea: one path per job")
        paths = (C.c_void_p * max(n, 1))()
        n_mea = np.zeros(max(n, 1), dtype=np.int64)
        for i, m in enumerate(mea):
            m = m[0] if isinstance(m, tuple) else m          # (Batch.mea() returns (path, sum, status) per job)
            m = _i32(m).reshape(-1, 2)
            keep.append(m)
            paths[i], n_mea[i] = m.ctypes.data, len(m)
    p = None
    if params is not None:
        p = params if isinstance(params, DeviationParams) else DeviationParams(*[int(v) for v in params])
    nb = p.n_buckets if p is not None else 64
    reads = np.zeros(n, dtype=DEVIATION_READ_DTYPE)
    hist = np.zeros((n, max(nb, 1)), dtype=np.int32)
    total = np.zeros(max(nb, 1), dtype=np.int64)
    sets_p, ev_p, n_sets, kms = C.c_void_p(), C.c_void_p(), np.zeros(1, dtype=np.int64), C.c_double()
    tail = (C.byref(p) if p is not None else None, int(flags), reads.ctypes.data, C.byref(sets_p), _ip(n_sets),
            _i32p(hist), _ip(total), C.byref(ev_p) if flags & DEV_EVENTS else None, C.byref(kms))
    call(arr, n, paths, _ip(n_mea) if n_mea is not None else None, tail)
    sets = _copy_out(sets_p, int(n_sets[0]), DEVIATION_SET_DTYPE)
    out = {"reads": reads, "sets": sets, "hist": hist, "total_hist": total, "kernel_ms": kms.value}
    if flags & DEV_EVENTS:
        out["events"] = _copy_out(ev_p, sum(int(j["n_events"]) for j in jobs), DEVIATION_EVENT_DTYPE)
    return out


def batch_guide_deviation(batch, jobs, mea=None, params=None, flags=0):
    """sa_batch_guide_deviation, chained onto a finished Batch: how far every event's best-posterior position lies from the guide.
    jobs: per job a dict with ax, ay (the job's anchors) and n_events -- the batch's own job dicts serve when they carry n_events,
    else len(events) is taken; mea: per job its MEA path ([n, 2] of (x, y), or Batch.mea()'s tuples), or None;
    params: (threshold, bucket_size, n_buckets), None for (10, 5, 64).  Returns a dict: reads (DEVIATION_READ_DTYPE), sets
    (DEVIATION_SET_DTYPE, job j's at reads["set_first"][j]), hist [n_jobs, n_buckets], total_hist, kernel_ms and, with DEV_EVENTS,
    events (DEVIATION_EVENT_DTYPE, job after job)."""
    jobs = [j if "n_events" in j else dict(ax=j["ax"], ay=j["ay"], n_events=len(j["events"])) for j in jobs]

    def call(arr, n, paths, n_mea, tail):
        _chk(lib().sa_batch_guide_deviation(batch._h, arr, n, paths, n_mea, *tail), "sa_batch_guide_deviation")
    return _deviation_call(jobs, mea, params, flags, call)


def guide_deviation_records(jobs, first, x, y, prob_e7, mea=None, params=None, device=0, flags=0):
    """sa_guide_deviation_records: the same from records the caller holds, job j's being first[j] .. first[j + 1) of x, y, prob_e7"""
    first, x, y, prob_e7 = _i64(first), _i32(x), _i32(y), _i64(prob_e7)
    if len(first) != len(jobs) + 1 or not (len(x) == len(y) == len(prob_e7)) or int(first[-1]) != len(x):
        raise ValueError("first: n_jobs + 1 offsets into x, y and prob_e7, which have one entry per record")

    def call(arr, n, paths, n_mea, tail):
        _chk(lib().sa_guide_deviation_records(arr, n, _ip(first), _i32p(x), _i32p(y), _ip(prob_e7), paths, n_mea, tail[0], int(device),
                                              *tail[1:]), "sa_guide_deviation_records")
    return _deviation_call(jobs, mea, params, flags, call)


def guide_deviation_release():
    lib().sa_guide_deviation_release()


def _label_call(jobs, mea, flags, call):
    """what batch_signal_labels and signal_labels_records share: the argument arrays, the call, the outputs per read"""
    jobs = list(jobs)
    n = len(jobs)
    arr = (LabelJob * max(n, 1))()
    keep = []
    for i, j in enumerate(jobs):
        rs, rl = _i64(j["raw_start"]), _i64(j["raw_length"])
        if len(rs) != len(rl):
            raise ValueError("a job's raw_start and raw_length have one entry per event")
        keep.append((rs, rl))
        arr[i] = LabelJob(_ip(rs), _ip(rl), int(j.get("n_events", len(rs))), int(j["n_samples"]), int(j.get("ref_first", 0)),
                          int(j.get("ref_step", 1)), int(j.get("base_shift", 0)))
    paths, n_mea = None, None
    if mea is not None:
        if len(mea) != n:
            raise ValueError("mea: one path per job")
        paths = (C.c_void_p * max(n, 1))()
        n_mea = np.zeros(max(n, 1), dtype=np.int64)
        for i, m in enumerate(mea):
            m = m[0] if isinstance(m, tuple) else m          # (Batch.mea() returns (path, sum, status) per job)
            if m is None:
                continue                                     # a NULL path
            m = _i32(m).reshape(-1, 2)
            keep.append(m)
            paths[i], n_mea[i] = m.ctypes.data, len(m)
    flags = int(flags)
    reads = np.zeros(n, dtype=LABEL_READ_DTYPE)
    ptrs = [C.c_void_p() for _ in range(4)]
    kms = C.c_double()
    wanted = [bool(flags & f) for f in (LABEL_MEA, LABEL_FULL, LABEL_BANDS, LABEL_SAMPLES)]
    tail = (flags, reads.ctypes.data) + tuple(C.byref(p) if w else None for p, w in zip(ptrs, wanted)) + (C.byref(kms),)
    call(arr, n, paths, _ip(n_mea) if n_mea is not None else None, tail)

    def total(first, count):
        return int(reads[first][-1] + reads[count][-1]) if n else 0
    out = {"reads": reads, "kernel_ms": kms.value}
    sets = (("mea", "mea_first", "n_mea", LABEL_SEGMENT_DTYPE), ("full", "full_first", "n_full", LABEL_SEGMENT_DTYPE),
            ("bands", "band_first", "n_bands", LABEL_BAND_DTYPE), ("samples", "sample_first", "n_samples", np.dtype(np.int32)))
    for (name, first, count, dtype), p, w in zip(sets, ptrs, wanted):
        if w:
            flat = _copy_out(p, total(first, count), dtype)
            out[name] = [flat[int(r[first]):int(r[first] + r[count])] for r in reads]
    return out


def batch_signal_labels(batch, jobs, mea=None, flags=LABEL_MEA):
    """sa_batch_signal_labels, chained onto a finished Batch: the labelled signal of every read.  jobs: per job a dict with raw_start,
    raw_length (per event), n_samples and, optionally, ref_first (0), ref_step (1), base_shift (0); mea: per job its MEA path ([n, 2]
    of (x, y), Batch.mea()'s tuples, or None), or None.  Returns a dict: reads (LABEL_READ_DTYPE), kernel_ms and, per flag, mea and
    full (per read LABEL_SEGMENT_DTYPE records), bands (LABEL_BAND_DTYPE) and samples (int32), each a list with one array per read."""
    def call(arr, n, paths, n_mea, tail):
        _chk(lib().sa_batch_signal_labels(batch._h, arr, n, paths, n_mea, *tail), "sa_batch_signal_labels")
    return _label_call(jobs, mea, flags, call)


def signal_labels_records(jobs, first, x, y, kmer_id, prob_e7, mea=None, device=0, flags=LABEL_MEA):
    """sa_signal_labels_records: the same from records the caller holds, job j's being first[j] .. first[j + 1) of x, y, kmer_id and
    prob_e7, in sa_batch_pairs order"""
    first, x, y, kmer_id, prob_e7 = _i64(first), _i32(x), _i32(y), _i32(kmer_id), _i64(prob_e7)
    if len(first) != len(jobs) + 1 or not (len(x) == len(y) == len(kmer_id) == len(prob_e7)) or int(first[-1]) != len(x):
        raise ValueError("first: n_jobs + 1 offsets into x, y, kmer_id and prob_e7, which have one entry per record")

    def call(arr, n, paths, n_mea, tail):
        _chk(lib().sa_signal_labels_records(arr, n, _ip(first), _i32p(x), _i32p(y), _i32p(kmer_id), _ip(prob_e7), paths, n_mea,
                                            int(device), *tail), "sa_signal_labels_records")
    return _label_call(jobs, mea, flags, call)


def signal_labels_release():
    lib().sa_signal_labels_release()


def signal_labels_last_kernel_ms():
    """{kernel: HIP-event ms} of the process's last call with LABEL_TIMES"""
    out = np.zeros(len(LABEL_KERNELS), dtype=np.float64)
    n = lib().sa_signal_labels_last_kernel_ms(_dp(out), len(out))
    assert n == len(LABEL_KERNELS)
    return dict(zip(LABEL_KERNELS, out.tolist()))


def _callq_call(scores, job_map, jobs, mea, params, flags, hist, call):
    """what batch_call_quality and call_quality_records share: the argument arrays, the call, the outputs as a dict"""
    jobs = list(jobs)
    n = len(jobs)
    marr, nm = _records(ScoreJobMap, job_map)
    if nm != n:
        raise ValueError("job_map: one entry per job")
    arr = (CallqJob * max(n, 1))()
    keep = []
    for i, j in enumerate(jobs):
        ax, ay, rs, rl = _i64(j["ax"]), _i64(j["ay"]), _i64(j["raw_start"]), _i64(j["raw_length"])
        if len(ax) != len(ay) or len(rs) != len(rl):
            raise ValueError("a job's ax and ay have one entry per anchor, its raw_start and raw_length one per event")
        keep.append((ax, ay, rs, rl))
        arr[i] = CallqJob(_ip(ax), _ip(ay), len(ax), _ip(rs), _ip(rl), int(j.get("n_events", len(rs))))
    paths, n_mea = None, None
    if mea is not None:
        if len(mea) != n:
            raise ValueError("mea: one path per job")
        paths = (C.c_void_p * max(n, 1))()
        n_mea = np.zeros(max(n, 1), dtype=np.int64)
        for i, m in enumerate(mea):
            m = m[0] if isinstance(m, tuple) else m          # (Batch.mea() returns (path, sum, status) per job)
            if m is None:
                continue                                     # a NULL path
            m = _i32(m).reshape(-1, 2)
            keep.append(m)
            paths[i], n_mea[i] = m.ctypes.data, len(m)
    p = None
    if params is not None:
        p = params if isinstance(params, CallqParams) else CallqParams(*[int(v) for v in params])
    nb = p.n_bins if p is not None else 200
    slots = max(nb, 1) + 2
    flags = int(flags)
    reads = np.zeros(n, dtype=CALLQ_READ_DTYPE)
    per_job = np.zeros((n, slots, 2), dtype=np.int64) if hist else None
    total = np.zeros((slots, 2), dtype=np.int64)
    calls_p, gaps_p, n_calls, n_gaps, kms = C.c_void_p(), C.c_void_p(), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64), C.c_double()
    want = bool(flags & CQ_CALLS)
    tail = (paths, _ip(n_mea) if n_mea is not None else None, C.byref(p) if p is not None else None, flags, reads.ctypes.data,
            C.byref(calls_p) if want else None, _ip(n_calls) if want else None, C.byref(gaps_p), _ip(n_gaps),
            _ip(per_job) if hist else None, _ip(total), C.byref(kms))
    call(scores._h, marr, arr, n, tail)
    out = {"reads": reads, "gaps": _copy_out(gaps_p, int(n_gaps[0]), CALLQ_GAP_DTYPE), "total_hist": total, "kernel_ms": kms.value}
    if hist:
        out["hist"] = per_job
    if want:
        out["calls"] = _copy_out(calls_p, int(n_calls[0]), CALLQ_CALL_DTYPE)
    return out


def batch_call_quality(scores, batch, job_map, jobs, mea=None, params=None, flags=0, hist=True):
    """sa_batch_call_quality, chained onto a finished Batch created with FLAG_SITE_CALLS: every labelled site call against the
    distance of its band from the guide, and the breaks of the MEA paths.  scores: a CallScores (only read: its letters, threshold
    and positions table); job_map: per job the fields of sa_score_job_map_t, as CallScores.add_batch takes them; jobs: per job a
    dict with ax, ay (the job's anchors) and raw_start, raw_length (per event); mea: per job its MEA path ([n, 2] of (x, y),
    Batch.mea()'s tuples, or None), or None; params: (bin_lo, bin_width, n_bins, min_gap), None for (-10000, 100, 200, 30).
    Returns a dict: reads (CALLQ_READ_DTYPE), gaps (CALLQ_GAP_DTYPE, job j's at reads["gap_first"][j]), total_hist
    [n_bins + 2, 2] (wrong, correct), kernel_ms, with hist the per-job hist [n_jobs, n_bins + 2, 2] and, with CQ_CALLS, calls
    (CALLQ_CALL_DTYPE, job j's at reads["call_first"][j])."""
    def call(s, marr, arr, n, tail):
        _chk(lib().sa_batch_call_quality(s, batch._h, marr, arr, n, *tail), "sa_batch_call_quality")
    return _callq_call(scores, job_map, jobs, mea, params, flags, hist, call)


def call_quality_records(scores, job_map, jobs, site_first, site_x, site_prob, rec_first, rec_x, rec_y, site_other=None, mea=None,
                         params=None, flags=0, hist=True):
    """sa_call_quality_records: the same from sites and records the caller holds -- job j's sites site_first[j] .. site_first[j + 1)
    of site_x (ascending) with site_prob [n_sites, len(letters)] and, optionally, site_other (non-zero: a site of other letters),
    its records rec_first[j] .. rec_first[j + 1) of rec_x, rec_y"""
    site_first, site_x, rec_first, rec_x, rec_y = _i64(site_first), _i32(site_x), _i64(rec_first), _i32(rec_x), _i32(rec_y)
    site_prob = _f64(site_prob).reshape(-1, len(scores.letters))
    other = None if site_other is None else np.ascontiguousarray(site_other, dtype=np.uint8)
    if (len(site_first) != len(jobs) + 1 or len(rec_first) != len(jobs) + 1 or int(site_first[-1]) != len(site_x) or
            len(site_prob) != len(site_x) or (other is not None and len(other) != len(site_x)) or len(rec_x) != len(rec_y) or
            int(rec_first[-1]) != len(rec_x)):
        raise ValueError("site_first and rec_first: n_jobs + 1 offsets into the per-site and the per-record arrays")

    def call(s, marr, arr, n, tail):
        _chk(lib().sa_call_quality_records(s, marr, arr, n, _ip(site_first), _i32p(site_x), _dp(site_prob),
                                           other.ctypes.data_as(_P(C.c_uint8)) if other is not None else None, _ip(rec_first),
                                           _i32p(rec_x), _i32p(rec_y), *tail), "sa_call_quality_records")
    return _callq_call(scores, job_map, jobs, mea, params, flags, hist, call)


def call_quality_release():
    lib().sa_call_quality_release()


def call_quality_last_kernel_ms():
    """{kernel: HIP-event ms} of the process's last call-quality call"""
    out = np.zeros(len(CQ_KERNELS), dtype=np.float64)
    n = lib().sa_call_quality_last_kernel_ms(_dp(out), len(out))
    assert n == len(CQ_KERNELS)
    return dict(zip(CQ_KERNELS, out.tolist()))


def snp_group_sites(pos, delta, window=6, keep_last=True):
    """sa_snp_group_sites (group_sites_in_window): the position of the largest delta of every group"""
    p, d = _i64(pos), _f64(delta)
    assert len(p) == len(d)
    out = np.zeros(max(len(p), 1), dtype=np.int64)
    n = np.zeros(1, dtype=np.int64)
    _chk(lib().sa_snp_group_sites(_ip(p), _dp(d), len(p), int(window), 1 if keep_last else 0, _ip(out), _ip(n)), "sa_snp_group_sites")
    return [int(v) for v in out[:int(n[0])]]


def snp_substitute_sites(ref, contig_pos_of_ref0, sites, reversed=False, letter="X"):
    """sa_snp_substitute_sites: `letter` at the listed contig positions (ascending) inside the window, the rest upper-cased"""
    b = ref.encode() if isinstance(ref, str) else bytes(ref)
    s = _i64(sites)
    out = C.create_string_buffer(len(b) + 1)
    _chk(lib().sa_snp_substitute_sites(b, len(b), int(contig_pos_of_ref0), 1 if reversed else 0, _ip(s), len(s),
                                       letter.encode()[:1], out), "sa_snp_substitute_sites")
    return out.raw[:len(b)].decode()


def snp_apply_calls(ref, marginals, contig=0):
    """sa_snp_apply_calls: `ref` with every proposal's called base written in"""
    b = ref.encode() if isinstance(ref, str) else bytes(ref)
    m = np.ascontiguousarray(marginals, dtype=SNP_MARGINAL_DTYPE)
    out = C.create_string_buffer(len(b) + 1)
    _chk(lib().sa_snp_apply_calls(b, len(b), m.ctypes.data, len(m), int(contig), out), "sa_snp_apply_calls")
    return out.raw[:len(b)].decode()


def snp_write_marginals(path, contig_names, marginals):
    m = np.ascontiguousarray(marginals, dtype=SNP_MARGINAL_DTYPE)
    keep = [c.encode() for c in contig_names]
    names = (C.c_char_p * max(len(keep), 1))(*keep)
    _chk(lib().sa_snp_write_marginals(os.fsencode(path), names, m.ctypes.data, len(m)), "sa_snp_write_marginals")


def format_py_repr(v):
    buf = C.create_string_buffer(40)
    n = lib().sa_format_py_repr(buf, float(v))
    return buf.raw[:n].decode()


def f6_units(v):
    """host "%f" rounding of v: (units of 1e-6, negative-zero flag, rc)"""
    u = np.zeros(1, dtype=np.int64)
    z = C.c_int32()
    rc = lib().sa_f6_units(float(v), _ip(u), C.byref(z))
    return int(u[0]), int(z.value), rc


def f6_units_device(values, device=0):
    v = _f64(values)
    u = np.zeros(len(v), dtype=np.int64)
    z = np.zeros(len(v), dtype=np.int32)
    r = np.zeros(len(v), dtype=np.int32)
    _chk(lib().sa_f6_units_device(_dp(v), len(v), _ip(u), _i32p(z), _i32p(r), int(device)), "sa_f6_units_device")
    return u, z, r
