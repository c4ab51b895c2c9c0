"""signalalign_amd -- MI355X-native banded pair-HMM path of signalAlign.

The product is the C-ABI shared library `lib/libsignalalign_hip.so` (see include/signalalign_hip.h) and
the `bin/signalMachine` drop-in CLI; this package is a thin ctypes mirror of that ABI for tests, the
benchmark and Python callers.  There is no CPU fallback: without the built library, or without a GPU
for the compute calls, everything here raises.
"""
from ._capi import (Batch, JobArray, Model, Params, SaError, build, default_ambig, default_params, device_count, device_memory, pool_configure, lib,
                    library_path, plan_describe, plan_digest, plan_check_path_records, dplan_compare, expect_batch, expect_last_stats, scalings_mom, event_align_batch, detect_events_batch, raw_event_align_batch, detect_release, DETECTOR_DNA, DETECTOR_RNA, RAW_NO_PEAK, RAW_EVENT_DTYPE, mea_batch, mea_params, MEA_INF, guide_to_anchors, remap_anchors, estimate_params, PAIR_DTYPE,
                    FLAG_EXACT, FLAG_FORCE_GENERIC, FLAG_RNA, FLAG_DEVICE_TO_ITSELF, FLAG_VC_ROWS, FLAG_PAIRS8, FLAG_SITE_CALLS, FLAG_POSITION_CALLS, FLAG_TWO_DIST_ALL_KERNELS,
                    FLAG_INPUTS_IN_HOST_BLOCK, HostBlock, KmerTable, KMER_ROW_DTYPE, KMER_STAT_DTYPE, MIXTURE_FIT_DTYPE, MixtureParams, mixture_assign, motif_kmer_pairs, model_write_trained, snp_substitute, snp_site_window, snp_write_read, SnpMarginals, SnpJobMap, SNP_SITE_DTYPE, SNP_MARGINAL_DTYPE, snp_group_sites, snp_substitute_sites, snp_apply_calls, snp_write_marginals, PositionProfile, ProfileJobMap, PROFILE_SITE_DTYPE, PROFILE_DIRECT, position_profile_write, profile_entropy_term, batch_guide_deviation, guide_deviation_records, guide_deviation_release, DeviationParams, DeviationJob, DEV_NO_GUIDE, DEV_NO_RECORDS, DEV_DIRECT, DEV_EVENTS, DEV_WINDOW, DEVIATION_READ_DTYPE, DEVIATION_SET_DTYPE, DEVIATION_EVENT_DTYPE, POSITION_CALL_DTYPE, format_py_repr, f6_units, f6_units_device, HdpState, hdp_finalize_distributions, Hmm, HMM_GAUSSIAN, HMM_HDP, hdp_nig_params_from_table,
                    HDP_LAYOUT_FLAT, HDP_LAYOUT_MULTISET, HDP_LAYOUT_MIDDLE_NTS, HDP_LAYOUT_COMPOSITION, HDP_LAYOUT_GROUP_MULTISET,
                    HDP_METRIC_KL, HDP_METRIC_HELLINGER, HDP_METRIC_L2, HDP_METRIC_SHANNON_JENSEN, HDP_GAUSS_CMP_DTYPE, hdp_distances, hdp_distances_paired, hdp_distances_release,
                    GuideParams, guide_params, guide_align_batch, guide_release, guide_seed, guide_format_cigar, cigar_load,
                    GUIDE_NO_ALIGNMENT, GUIDE_SHORT, GUIDE_BAND_EDGE, GUIDE_EMPTY, GUIDE_TRACE,
                    RefIndex, LocateParams, locate_params, ref_index_build, ref_index_build_fasta, ref_index_info, ref_index_entries, guide_locate_batch,
                    locate_release, locate_window, LOCATE_NONE, LOCATE_AMBIGUOUS, LOCATE_OVERFLOW, LOCATE_EMPTY, LOCATE_FIELDS)

__all__ = ["Batch", "JobArray", "Model", "Params", "SaError", "build", "default_ambig", "default_params", "device_count", "device_memory", "pool_configure", "lib",
           "library_path", "plan_describe", "plan_digest", "plan_check_path_records", "dplan_compare", "expect_batch", "expect_last_stats", "scalings_mom", "event_align_batch", "detect_events_batch", "raw_event_align_batch", "detect_release", "DETECTOR_DNA", "DETECTOR_RNA", "RAW_NO_PEAK", "RAW_EVENT_DTYPE", "mea_batch", "mea_params", "MEA_INF", "guide_to_anchors", "remap_anchors", "estimate_params", "PAIR_DTYPE",
           "FLAG_EXACT", "FLAG_FORCE_GENERIC", "FLAG_RNA", "FLAG_DEVICE_TO_ITSELF", "FLAG_VC_ROWS", "FLAG_PAIRS8", "FLAG_SITE_CALLS", "FLAG_POSITION_CALLS", "FLAG_TWO_DIST_ALL_KERNELS",
           "FLAG_INPUTS_IN_HOST_BLOCK", "HostBlock", "KmerTable", "KMER_ROW_DTYPE", "KMER_STAT_DTYPE", "MIXTURE_FIT_DTYPE", "MixtureParams", "mixture_assign", "motif_kmer_pairs", "model_write_trained", "snp_substitute", "snp_site_window", "snp_write_read", "SnpMarginals", "SnpJobMap", "SNP_SITE_DTYPE", "SNP_MARGINAL_DTYPE", "snp_group_sites", "snp_substitute_sites", "snp_apply_calls", "snp_write_marginals", "PositionProfile", "ProfileJobMap", "PROFILE_SITE_DTYPE", "PROFILE_DIRECT", "position_profile_write", "profile_entropy_term", "batch_guide_deviation", "guide_deviation_records", "guide_deviation_release", "DeviationParams", "DeviationJob", "DEV_NO_GUIDE", "DEV_NO_RECORDS", "DEV_DIRECT", "DEV_EVENTS", "DEV_WINDOW", "DEVIATION_READ_DTYPE", "DEVIATION_SET_DTYPE", "DEVIATION_EVENT_DTYPE", "POSITION_CALL_DTYPE", "format_py_repr", "f6_units", "f6_units_device", "HdpState", "hdp_finalize_distributions", "Hmm", "HMM_GAUSSIAN", "HMM_HDP", "hdp_nig_params_from_table",
           "HDP_LAYOUT_FLAT", "HDP_LAYOUT_MULTISET", "HDP_LAYOUT_MIDDLE_NTS", "HDP_LAYOUT_COMPOSITION", "HDP_LAYOUT_GROUP_MULTISET",
           "HDP_METRIC_KL", "HDP_METRIC_HELLINGER", "HDP_METRIC_L2", "HDP_METRIC_SHANNON_JENSEN", "HDP_GAUSS_CMP_DTYPE", "hdp_distances", "hdp_distances_paired", "hdp_distances_release",
           "GuideParams", "guide_params", "guide_align_batch", "guide_release", "guide_seed", "guide_format_cigar", "cigar_load",
           "GUIDE_NO_ALIGNMENT", "GUIDE_SHORT", "GUIDE_BAND_EDGE", "GUIDE_EMPTY", "GUIDE_TRACE",
           "RefIndex", "LocateParams", "locate_params", "ref_index_build", "ref_index_build_fasta", "ref_index_info", "ref_index_entries", "guide_locate_batch",
           "locate_release", "locate_window", "LOCATE_NONE", "LOCATE_AMBIGUOUS", "LOCATE_OVERFLOW", "LOCATE_EMPTY", "LOCATE_FIELDS"]
