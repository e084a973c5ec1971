"""ctypes mirror of include/vlr.h (the C ABI of the engine).

Only struct layouts, constants and the signature of every entry point (SIGNATURES, at the end) live
here; nothing is computed.  Both the product binding (`varlociraptor_amd.engine`, which applies the
signatures to the library once, at load) and the test-only oracle binding (`oracle/oracle.py`) use
these definitions, because the oracle consumes exactly the same boundary structs as the engine.
"""
import ctypes as C

import numpy as np

ABI_VERSION = 14
MAX_SAMPLES = 16
N_BIAS = 6

# status codes
OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_HIP, ERR_INVALID_PRIOR, ERR_OOM = 0, -1, -2, -3, -4, -5, -6
LOCUS_NAN, LOCUS_UNDERFLOW, LOCUS_TABLE_FULL, LOCUS_TOO_DEEP = 1, 2, 4, 8
LOCUS_MISSING_DATA, LOCUS_SINGLETON_ADJ, LOCUS_FILTERED_ALN = 16, 32, 64

SPECTRUM_SET, SPECTRUM_RANGE = 0, 1
CMP_EQUAL, CMP_GREATER, CMP_GREATER_EQUAL, CMP_LESS, CMP_LESS_EQUAL, CMP_NOT_EQUAL = range(6)
NODE_SAMPLE, NODE_LFC, NODE_VARIANT, NODE_TRUE, NODE_FALSE = range(5)
INHERIT_NONE, INHERIT_MENDELIAN, INHERIT_CLONAL, INHERIT_SUBCLONAL = range(4)
VT_SNV, VT_MNV, VT_INDEL, VT_SV, VT_OTHER = range(5)

# packed observation flags
F_STRAND_SHIFT, F_ORIENT_SHIFT = 0, 2
F_READPOS_MAJOR, F_SOFTCLIPPED, F_PAIRED, F_MAX_MAPQ = 1 << 4, 1 << 5, 1 << 6, 1 << 7
F_ALTLOCUS_SHIFT = 8
F_HP_LEN_VALID = 1 << 10
F_HP_LEN_SHIFT = 16
STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH, STRAND_NONE = range(4)
ORIENT_F1R2, ORIENT_F2R1, ORIENT_NONE, ORIENT_OTHER = range(4)
ALTLOCUS_MAJOR, ALTLOCUS_SOME, ALTLOCUS_NONE = range(3)

BIAS_STRAND, BIAS_ORIENTATION, BIAS_POSITION, BIAS_SOFTCLIP, BIAS_HOMOPOLYMER, BIAS_ALTLOCUS = (1 << i for i in range(6))
BIAS_ALL = 0x3F
LOCUS_REMOVE_NONSTANDARD = 1 << 6
LOCUS_HAS_SNV = 1 << 7


class Spectrum(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("set_offset", C.c_int32), ("set_len", C.c_int32),
        ("left_exclusive", C.c_int32), ("right_exclusive", C.c_int32), ("_pad", C.c_int32),
        ("start", C.c_double), ("end", C.c_double),
    ]


class Node(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("sample", C.c_int32), ("sample_b", C.c_int32), ("cmp", C.c_int32),
        ("lfc_value", C.c_double), ("vafs", Spectrum), ("positive", C.c_int32),
        ("refbase", C.c_uint8), ("altbase", C.c_uint8), ("_pad", C.c_uint8 * 2),
        ("child_offset", C.c_int32), ("n_children", C.c_int32),
    ]


class Inheritance(C.Structure):
    _fields_ = [("kind", C.c_int32), ("from0", C.c_int32), ("from1", C.c_int32), ("somatic", C.c_int32)]


class ScenarioDesc(C.Structure):
    _fields_ = [
        ("n_samples", C.c_int32),
        ("resolution", C.POINTER(C.c_double)),
        ("contaminated_by", C.POINTER(C.c_int32)),
        ("contamination_fraction", C.POINTER(C.c_double)),
        ("universe_offset", C.POINTER(C.c_int32)),
        ("universe", C.POINTER(Spectrum)),
        ("uniform_prior", C.POINTER(C.c_uint8)),
        ("ploidy", C.POINTER(C.c_int32)),
        ("germline_mutation_rate", C.POINTER(C.c_double)),
        ("somatic_effective_mutation_rate", C.POINTER(C.c_double)),
        ("inheritance", C.POINTER(Inheritance)),
        ("heterozygosity", C.c_double),
        ("fraction_indel", C.c_double), ("fraction_mnv", C.c_double), ("fraction_sv", C.c_double),
        ("is_absent_only", C.c_int32),
        ("n_events", C.c_int32),
        ("event_names", C.POINTER(C.c_char_p)),
        ("event_root_offset", C.POINTER(C.c_int32)),
        ("root_index", C.POINTER(C.c_int32)),
        ("n_nodes", C.c_int32),
        ("nodes", C.POINTER(Node)),
        ("child_index", C.POINTER(C.c_int32)),
        ("vafs", C.POINTER(C.c_double)),
        ("variant_heterozygosity_ln", C.c_double),
        ("variant_somatic_effective_mutation_rate_ln", C.c_double),
    ]


class Batch(C.Structure):
    _fields_ = [
        ("n_loci", C.c_int64), ("n_samples", C.c_int32), ("_pad", C.c_int32), ("n_obs", C.c_int64),
        ("obs_offset", C.c_void_p),
        ("prob_mapping", C.c_void_p), ("prob_alt", C.c_void_p), ("prob_ref", C.c_void_p),
        ("prob_missed_allele", C.c_void_p), ("prob_sample_alt", C.c_void_p),
        ("prob_double_overlap", C.c_void_p), ("prob_hit_base", C.c_void_p),
        ("prob_hp_artifact", C.c_void_p), ("prob_hp_variant", C.c_void_p),
        ("flags", C.c_void_p),
        ("locus_flags", C.c_void_p), ("variant_type", C.c_void_p), ("ref_base", C.c_void_p), ("alt_base", C.c_void_p),
    ]


class Results(C.Structure):
    _fields_ = [
        ("n_loci", C.c_int64), ("n_out", C.c_int32), ("n_samples", C.c_int32),
        ("ln_posterior", C.c_void_p), ("ln_marginal", C.c_void_p), ("map_vaf", C.c_void_p),
        ("map_bias", C.c_void_p), ("best_event", C.c_void_p), ("status", C.c_void_p),
        ("afd_capacity", C.c_int32), ("_pad", C.c_int32),
        ("afd_count", C.c_void_p), ("afd_vaf", C.c_void_p), ("afd_lnprob", C.c_void_p),
        ("afd_text", C.c_void_p), ("afd_text_capacity", C.c_uint64), ("afd_text_span", C.c_void_p),
    ]


# column name -> dtype of the SoA observation columns of vlr_batch
OBS_COLUMNS = [
    ("prob_mapping", np.float32), ("prob_alt", np.float32), ("prob_ref", np.float32),
    ("prob_missed_allele", np.float32), ("prob_sample_alt", np.float32),
    ("prob_double_overlap", np.float32), ("prob_hit_base", np.float32),
    ("prob_hp_artifact", np.float32), ("prob_hp_variant", np.float32), ("flags", np.uint32),
]
LOCUS_COLUMNS = [("locus_flags", np.uint8), ("variant_type", np.uint8), ("ref_base", np.uint8), ("alt_base", np.uint8)]


def pack_flags(strand, orientation, readpos_major, softclipped, paired, max_mapq, alt_locus, hp_len=None):
    """Pack per-observation categorical features into the VLR_F_* bit layout (numpy arrays in, uint32 out)."""
    f = (np.asarray(strand, np.uint32) << F_STRAND_SHIFT) | (np.asarray(orientation, np.uint32) << F_ORIENT_SHIFT)
    f = f | np.where(readpos_major, F_READPOS_MAJOR, 0).astype(np.uint32)
    f = f | np.where(softclipped, F_SOFTCLIPPED, 0).astype(np.uint32)
    f = f | np.where(paired, F_PAIRED, 0).astype(np.uint32)
    f = f | np.where(max_mapq, F_MAX_MAPQ, 0).astype(np.uint32)
    f = f | (np.asarray(alt_locus, np.uint32) << F_ALTLOCUS_SHIFT)
    if hp_len is not None:
        hp = np.asarray(hp_len)
        valid = hp > -128  # -128 encodes None
        f = f | np.where(valid, F_HP_LEN_VALID, 0).astype(np.uint32)
        f = f | np.where(valid, (hp.astype(np.int8).view(np.uint8).astype(np.uint32)) << F_HP_LEN_SHIFT, 0).astype(np.uint32)
    return f.astype(np.uint32)


class BamStatsResult(C.Structure):
    """vlr_bamstats_counts (estimate alignment-properties, ABI 8)."""
    _fields_ = [("transitions", C.c_uint64 * 256),
                ("n_taken", C.c_int64), ("n_skipped", C.c_int64), ("n_not_usable", C.c_int64), ("n_softclips", C.c_int64),
                ("n_not_paired", C.c_int64), ("n_not_first", C.c_int64), ("n_mate_unmapped", C.c_int64), ("n_tid_mismatch", C.c_int64),
                ("max_del", C.c_int64), ("max_ins", C.c_int64), ("max_read_len", C.c_int64), ("max_mapq", C.c_int64),
                ("frac_max_softclip", C.c_double), ("has_softclip", C.c_int64),
                ("n_hop_keys", C.c_int64), ("n_insert_sizes", C.c_int64), ("seconds", C.c_double * 10)]


# vlr_basepileup_* (SNV / MNV allele supports from BAM records, ABI 10)
BASEPILEUP_MAX_LEN = 32
BASEPILEUP_SNV, BASEPILEUP_MNV = 0, 1
BASEPILEUP_BAD_RECORD, BASEPILEUP_OVERFLOW, BASEPILEUP_GUARD_DAMAGED = 1, 2, 4
BASEPILEUP_HIT_NEEDS_REALIGN, BASEPILEUP_HIT_READ_POS_OUT_OF_BOUNDS, BASEPILEUP_HIT_INVALID_STRAND_INFO, BASEPILEUP_HIT_LEADING_REFSKIP = 1, 2, 4, 8
BASEPILEUP_NO_READ_POSITION = 0xFFFFFFFF


class BasePileupHit(C.Structure):
    """vlr_basepileup_hit"""
    _fields_ = [("prob_ref", C.c_double), ("prob_alt", C.c_double), ("record", C.c_uint64), ("locus", C.c_uint32),
                ("read_position", C.c_uint32), ("third_allele", C.c_uint32), ("flag", C.c_uint16), ("strand", C.c_uint8),
                ("mapq", C.c_uint8), ("status", C.c_uint8), ("pad", C.c_uint8 * 7)]


BASEPILEUP_HIT_DTYPE = np.dtype([("prob_ref", "<f8"), ("prob_alt", "<f8"), ("record", "<u8"), ("locus", "<u4"), ("read_position", "<u4"),
                                 ("third_allele", "<u4"), ("flag", "<u2"), ("strand", "u1"), ("mapq", "u1"), ("status", "u1"), ("pad", "u1", (7,))])
assert C.sizeof(BasePileupHit) == 48 and BASEPILEUP_HIT_DTYPE.itemsize == 48


class BasePileupCounts(C.Structure):
    """vlr_basepileup_counts"""
    _fields_ = [("n_hits", C.c_int64), ("n_records", C.c_int64), ("n_rejected", C.c_int64), ("n_needs_realign", C.c_int64),
                ("status", C.c_uint64), ("needed_capacity", C.c_int64), ("first_bad_record", C.c_int64), ("seconds", C.c_double * 8)]


# vlr_indelpileup_* (indel allele supports from BAM records, ABI 12)
INDELPILEUP_MAX_WINDOW = 64
INDELPILEUP_DELETION, INDELPILEUP_INSERTION, INDELPILEUP_REPLACEMENT = 0, 1, 2
INDELPILEUP_EXACT, INDELPILEUP_FAST, INDELPILEUP_HOMOPOLYMER = 0, 1, 2
INDELPILEUP_BAD_RECORD, INDELPILEUP_OVERFLOW, INDELPILEUP_GUARD_DAMAGED = 1, 2, 4
INDELPILEUP_HIT_NO_OVERLAP, INDELPILEUP_HIT_LEADING_REFSKIP = 1, 2
INDELPILEUP_HIT_STRAND_INFO = 4   # vlr_fragpileup_open_realign only (ABI 14)


class IndelPileupHit(C.Structure):
    """vlr_indelpileup_hit"""
    _fields_ = [("ln_ref", C.c_double), ("ln_alt", C.c_double), ("record", C.c_uint64), ("ref_begin", C.c_int64), ("locus", C.c_uint32),
                ("ref_len", C.c_uint32), ("read_begin", C.c_uint32), ("read_len", C.c_uint32), ("dist_ref", C.c_int32), ("dist_alt", C.c_int32),
                ("flag", C.c_uint16), ("mapq", C.c_uint8), ("status", C.c_uint8), ("pad", C.c_uint8 * 4)]


INDELPILEUP_HIT_DTYPE = np.dtype([("ln_ref", "<f8"), ("ln_alt", "<f8"), ("record", "<u8"), ("ref_begin", "<i8"), ("locus", "<u4"), ("ref_len", "<u4"),
                                  ("read_begin", "<u4"), ("read_len", "<u4"), ("dist_ref", "<i4"), ("dist_alt", "<i4"), ("flag", "<u2"), ("mapq", "u1"),
                                  ("status", "u1"), ("pad", "u1", (4,))])
assert C.sizeof(IndelPileupHit) == 64 and INDELPILEUP_HIT_DTYPE.itemsize == 64


class IndelPileupCounts(C.Structure):
    """vlr_indelpileup_counts"""
    _fields_ = [("n_hits", C.c_int64), ("n_records", C.c_int64), ("n_rejected", C.c_int64), ("n_pairs", C.c_int64), ("x_bytes", C.c_int64),
                ("y_bytes", C.c_int64), ("status", C.c_uint64), ("needed_capacity", C.c_int64), ("first_bad_record", C.c_int64), ("seconds", C.c_double * 12)]


# vlr_fragpileup_* (fragment observations of SNV / MNV candidates from BAM records, ABI 13)
FRAGPILEUP_MAX_MEMBERS = 4096
FRAGPILEUP_BAD_RECORD, FRAGPILEUP_MEMBER_OVERFLOW, FRAGPILEUP_NAME_OVERFLOW, FRAGPILEUP_GUARD_DAMAGED, FRAGPILEUP_KEY_OVERFLOW = 1, 2, 4, 8, 16
FRAGPILEUP_ANY_OVERFLOW = FRAGPILEUP_MEMBER_OVERFLOW | FRAGPILEUP_NAME_OVERFLOW | FRAGPILEUP_KEY_OVERFLOW
FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS, FRAGPILEUP_LOCUS_TOO_MANY_ALT_LOCI = 1, 2
FRAGPILEUP_OBS_INVALID_RO = 16
FRAGPILEUP_EVIDENCE_OVERFLOW = 32          # status word of a realigning session (ABI 14)
FRAGPILEUP_OBS_REALIGN_STRAND_INFO = 32    # status byte of an observation (ABI 14)
FRAGPILEUP_SOFTCLIPPED, FRAGPILEUP_PAIRED, FRAGPILEUP_MAX_MAPQ, FRAGPILEUP_READPOS_MAJOR, FRAGPILEUP_HAS_XA = 1, 2, 4, 8, 16
FRAG_F1R2, FRAG_F2R1, FRAG_R1F2, FRAG_R2F1, FRAG_F1F2, FRAG_R1R2, FRAG_F2F1, FRAG_R2R1, FRAG_ORIENT_NONE = range(9)
FRAGPILEUP_NO_RECORD = 0xFFFFFFFFFFFFFFFF

FRAGPILEUP_OBS_DTYPE = np.dtype([("prob_ref", "<f8"), ("prob_alt", "<f8"), ("left", "<u8"), ("right", "<u8"), ("read_position", "<u4"),
                                 ("third_allele", "<u4"), ("len_sum", "<u4"), ("min_mapq", "u1"), ("orientation", "u1"), ("strand", "u1"),
                                 ("bits", "u1"), ("status", "u1"), ("alt_locus", "u1"), ("pad", "u1", (6,))])
FRAGPILEUP_LOCUS_DTYPE = np.dtype([("obs_offset", "<i8"), ("n_members", "<u4"), ("n_obs", "<u4"), ("major_read_position", "<u4"), ("status", "<u4")])
assert FRAGPILEUP_OBS_DTYPE.itemsize == 56 and FRAGPILEUP_LOCUS_DTYPE.itemsize == 24


class FragPileupCounts(C.Structure):
    """vlr_fragpileup_counts"""
    _fields_ = [("n_obs", C.c_int64), ("n_members", C.c_int64), ("n_records", C.c_int64), ("n_rejected", C.c_int64), ("n_loci_too_deep", C.c_int64),
                ("status", C.c_uint64), ("needed_members", C.c_int64), ("needed_name_bytes", C.c_int64), ("needed_keys", C.c_int64), ("first_bad_record", C.c_int64),
                ("seconds", C.c_double * 8)]


class FragPileupRealignCounts(C.Structure):
    """vlr_fragpileup_realign_counts"""
    _fields_ = [("n_evidences", C.c_int64), ("needed_evidences", C.c_int64), ("x_bytes", C.c_int64), ("y_bytes", C.c_int64), ("n_ranges", C.c_int64),
                ("seconds", C.c_double * 4)]


# vlr_fragpileup_open_indel / _read_indel (deletion and insertion candidates in the fragment session; additive, ABI stays 14)
FRAGPILEUP_MAX_INDEL_LEN = 4096
FRAGPILEUP_INDEL_NONPOSITIVE_ISIZE = 1
FRAGPILEUP_INDEL_OBS_DTYPE = np.dtype([("insert_size", "<i8"), ("len_left", "<u4"), ("len_right", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
FRAGPILEUP_INDEL_LOCUS_DTYPE = np.dtype([("max_del", "<u4"), ("max_ins", "<u4"), ("max_clip", "<u4"), ("max_clip_l_seq", "<u4")])
assert FRAGPILEUP_INDEL_OBS_DTYPE.itemsize == 24 and FRAGPILEUP_INDEL_LOCUS_DTYPE.itemsize == 16
# vlr_fragpileup_set_alt_variants / _alt_result / _read_alt_variants (the other alleles of a locus; additive, ABI stays 14)
FRAGPILEUP_MAX_ALT_VARIANTS = 15
FRAGPILEUP_ALT_HIT_DTYPE = np.dtype([("winner", "u1"), ("n_tied", "u1"), ("n_ref_side_hits", "u1"), ("pad", "u1", (5,))])
assert FRAGPILEUP_ALT_HIT_DTYPE.itemsize == 8


class FragPileupAltCounts(C.Structure):
    """vlr_fragpileup_alt_counts"""
    _fields_ = [("n_edit_pairs", C.c_int64), ("n_hmm_pairs", C.c_int64), ("n_competitors", C.c_int64), ("n_loci_with_competitors", C.c_int64)]


# vlr_fragpileup_open_methylation (<METH> candidates in the fragment session; additive, ABI stays 14)
METH_CONVERTED, METH_ANNOTATED = 0, 1


class RealignDesc(C.Structure):
    """vlr_realign_batch_desc"""
    _fields_ = [("n_pairs", C.c_int64), ("x_offset", C.c_void_p), ("x_bases", C.c_void_p), ("y_offset", C.c_void_p),
                ("y_bases", C.c_void_p), ("y_quals", C.c_void_p), ("max_edit_dist", C.c_void_p), ("gap", C.c_double * 4)]


class ObsSites(C.Structure):
    """vlr_obs_sites"""
    _fields_ = [
        ("n_loci", C.c_int64), ("n_contigs", C.c_int32), ("_pad", C.c_int32),
        ("contig_names", C.POINTER(C.c_char_p)), ("contig", C.c_void_p), ("pos", C.c_void_p), ("strings", C.c_void_p),
        ("id_offset", C.c_void_p), ("ref_offset", C.c_void_p), ("alt_offset", C.c_void_p),
        ("group_representative", C.c_void_p), ("heterozygosity_ln", C.c_void_p), ("somatic_effective_mutation_rate_ln", C.c_void_p),
        ("third_allele_evidence", C.c_void_p), ("imprecise", C.c_void_p), ("group_key", C.c_void_p),
    ]


# name -> (restype, argtypes) of every function include/vlr.h declares, in the header's order.  engine.lib() applies the table to
# the library once; tests/test_host_logic.py compares it with the header's prototypes (count, and pointer / 32-bit / 64-bit /
# float / double of every parameter and of the return value).  Opaque handles and plain arrays are c_void_p.
_FRAGPILEUP_OPEN_HEAD = [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int,
                         C.c_int64, C.c_int64, C.c_int64, C.c_int64]   # what vlr_fragpileup_open and vlr_fragpileup_open_realign share
SIGNATURES = {
    # ---- entry points: build, plans, batches
    "vlr_abi_version": (C.c_int, []),
    "vlr_build_id": (C.c_char_p, []),
    "vlr_last_error": (C.c_char_p, []),
    "vlr_plan_create": (C.c_int, [C.POINTER(ScenarioDesc), C.c_int, C.POINTER(C.c_void_p)]),
    "vlr_plan_destroy": (None, [C.c_void_p]),
    "vlr_plan_n_out": (C.c_int, [C.c_void_p]),
    "vlr_plan_n_samples": (C.c_int, [C.c_void_p]),
    "vlr_plan_set_max_depth": (C.c_int, [C.c_void_p, C.c_int]),
    "vlr_plan_set_max_obs": (C.c_int, [C.c_void_p, C.c_int]),
    "vlr_plan_fit_max_obs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "vlr_batch_run": (C.c_int, [C.c_void_p, C.POINTER(Batch), C.POINTER(Results), C.c_void_p]),
    "vlr_batch_run_host": (C.c_int, [C.c_void_p, C.POINTER(Batch), C.POINTER(Results)]),
    "vlr_batch_run_device_in": (C.c_int, [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(Results)]),
    # ---- one node, several devices
    "vlr_node_create": (C.c_int, [C.POINTER(ScenarioDesc), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "vlr_node_destroy": (None, [C.c_void_p]),
    "vlr_node_n_devices": (C.c_int, [C.c_void_p]),
    "vlr_node_device": (C.c_int, [C.c_void_p, C.c_int]),
    "vlr_node_plan": (C.c_void_p, [C.c_void_p, C.c_int]),
    "vlr_node_set_max_depth": (C.c_int, [C.c_void_p, C.c_int]),
    "vlr_node_set_max_obs": (C.c_int, [C.c_void_p, C.c_int]),
    "vlr_node_shard_range": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "vlr_node_batch_run_host": (C.c_int, [C.c_void_p, C.POINTER(Batch), C.POINTER(Results)]),
    # ---- page-locked host memory, buffer reservation, counters of a plan
    "vlr_host_alloc": (C.c_void_p, [C.c_size_t]),
    "vlr_host_free": (None, [C.c_void_p]),
    "vlr_plan_reserve": (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
    "vlr_plan_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "vlr_plan_last_instance": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vlr_plan_work_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]),
    "vlr_plan_fused_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]),
    # ---- read-vs-allele pair HMM, edit-distance pre-filter
    "vlr_realign_batch": (C.c_int, [C.c_int, C.POINTER(RealignDesc), C.c_void_p, C.c_void_p]),
    "vlr_realign_batch_host": (C.c_int, [C.c_int, C.POINTER(RealignDesc), C.c_void_p]),
    "vlr_realign_fast_batch": (C.c_int, [C.c_int, C.POINTER(RealignDesc), C.c_void_p, C.c_void_p]),
    "vlr_realign_fast_batch_host": (C.c_int, [C.c_int, C.POINTER(RealignDesc), C.c_void_p]),
    "vlr_realign_homopolymer_batch": (C.c_int, [C.c_int, C.POINTER(RealignDesc), C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
    "vlr_realign_homopolymer_batch_host": (C.c_int, [C.c_int, C.POINTER(RealignDesc), C.POINTER(C.c_double), C.c_void_p]),
    "vlr_edit_distance_batch": (C.c_int, [C.c_int, C.POINTER(RealignDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vlr_edit_distance_batch_host": (C.c_int, [C.c_int, C.POINTER(RealignDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    # ---- Bayesian FDR control, contamination estimation
    "vlr_fdr_threshold": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "vlr_contamination_posterior": (C.c_int, [C.c_int, C.c_int64] + [C.c_void_p] * 5 + [C.c_double] + [C.c_void_p] * 2 + [C.POINTER(C.c_double)]),
    # ---- alignment properties
    "vlr_bamstats_open": (C.c_int, [C.c_int, C.c_char_p, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]),
    "vlr_bamstats_add_bam": (C.c_int, [C.c_void_p, C.c_char_p]),
    "vlr_bamstats_result": (C.c_int, [C.c_void_p, C.POINTER(BamStatsResult)]),
    "vlr_bamstats_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "vlr_bamstats_close": (None, [C.c_void_p]),
    # ---- SNV / MNV allele supports from BAM records
    "vlr_basepileup_open": (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64,
                                      C.POINTER(C.c_void_p)]),
    "vlr_basepileup_add_bam": (C.c_int, [C.c_void_p, C.c_char_p]),
    "vlr_basepileup_result": (C.c_int, [C.c_void_p, C.POINTER(BasePileupCounts)]),
    "vlr_basepileup_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "vlr_basepileup_tables": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vlr_basepileup_close": (None, [C.c_void_p]),
    # ---- indel allele supports from BAM records
    "vlr_indelpileup_open": (C.c_int, [C.c_int, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]),
    "vlr_indelpileup_add_bam": (C.c_int, [C.c_void_p, C.c_char_p]),
    "vlr_indelpileup_result": (C.c_int, [C.c_void_p, C.POINTER(IndelPileupCounts)]),
    "vlr_indelpileup_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "vlr_indelpileup_read_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "vlr_indelpileup_close": (None, [C.c_void_p]),
    # ---- fragment observations of SNV / MNV candidates from BAM records
    "vlr_fragpileup_open": (C.c_int, _FRAGPILEUP_OPEN_HEAD + [C.POINTER(C.c_void_p)]),
    "vlr_fragpileup_add_bam": (C.c_int, [C.c_void_p, C.c_char_p]),
    "vlr_fragpileup_result": (C.c_int, [C.c_void_p, C.POINTER(FragPileupCounts)]),
    "vlr_fragpileup_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "vlr_fragpileup_close": (None, [C.c_void_p]),
    "vlr_fragpileup_open_realign": (C.c_int, _FRAGPILEUP_OPEN_HEAD + [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.c_int64,
                                                                      C.POINTER(C.c_void_p)]),
    "vlr_fragpileup_realign_result": (C.c_int, [C.c_void_p, C.POINTER(FragPileupRealignCounts)]),
    "vlr_fragpileup_read_realigned": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "vlr_fragpileup_open_indel": (C.c_int, [C.c_int, C.c_int64] + [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_char_p, C.c_int,
                                            C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    "vlr_fragpileup_read_indel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "vlr_fragpileup_set_alt_variants": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vlr_fragpileup_alt_result": (C.c_int, [C.c_void_p, C.POINTER(FragPileupAltCounts)]),
    "vlr_fragpileup_read_alt_variants": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "vlr_fragpileup_open_methylation": (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                                  C.POINTER(C.c_void_p)]),
    "vlr_methylation_tables": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    # ---- consumers of a calls file: filter-calls control-fdr / posterior-odds, estimate mutational-burden
    "vlr_calls_filter_fdr": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.c_double, C.c_uint32, C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "vlr_posterior_odds_keep": (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vlr_range_group_lse": (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vlr_callstats_last_kernel_ms": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vlr_calls_filter_odds": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "vlr_calls_mutational_burden": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_int, C.c_void_p, C.POINTER(C.c_int64)]),
    # ---- diagnostics
    "vlr_selftest_math": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "vlr_selftest_stream": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int]),
    "vlr_selftest_fdr_stages": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_double] + [C.c_void_p] * 6 + [C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    # ---- native ingest / emission
    "vlr_obs_read": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "vlr_obs_table_free": (None, [C.c_void_p]),
    "vlr_obs_table_batch": (C.c_int, [C.c_void_p, C.POINTER(Batch)]),
    "vlr_obs_table_sites": (C.c_int, [C.c_void_p, C.POINTER(ObsSites)]),
    "vlr_obs_write": (C.c_int, [C.c_char_p, C.POINTER(Batch), C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "vlr_calls_write": (C.c_int, [C.c_char_p, C.c_char_p, C.c_void_p, C.POINTER(Results), C.POINTER(C.c_char_p), C.c_int]),
    "vlr_obs_reader_open": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "vlr_obs_reader_next": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]),
    "vlr_obs_reader_close": (None, [C.c_void_p]),
    "vlr_calls_writer_open": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "vlr_calls_writer_append": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Results), C.POINTER(C.c_char_p), C.c_int]),
    "vlr_calls_writer_close": (C.c_int, [C.c_void_p]),
    "vlr_calls_writer_set_part": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "vlr_calls_concat_parts": (C.c_int, [C.c_char_p, C.POINTER(C.c_char_p), C.c_int]),
    "vlr_selftest_format_fixed": (C.c_int, [C.c_double, C.c_int, C.c_char_p, C.c_int]),
    "vlr_selftest_afd_text": (C.c_int, [C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32)]),
    "vlr_ingest_last_timings": (None, [C.POINTER(C.c_double)]),
    "vlr_ingest_total_timings": (None, [C.POINTER(C.c_double), C.c_int]),
    # ---- device front door
    "vlr_obs_reader_open_device": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "vlr_obs_reader_open_device_shard": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "vlr_obs_reader_shard_row_size": (C.c_int, []),
    "vlr_obs_reader_shard_counts": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vlr_obs_reader_shard_assign": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "vlr_node_obs_readers_open": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "vlr_obs_table_device_batch": (C.c_int, [C.c_void_p, C.POINTER(Batch)]),
    "vlr_obs_reader_set_host_columns": (C.c_int, [C.c_void_p, C.c_int]),
    "vlr_obs_table_summaries": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "vlr_obs_table_fetch_columns": (C.c_int, [C.c_void_p]),
    "vlr_obs_reader_set_async_columns": (C.c_int, [C.c_void_p, C.c_int]),
    "vlr_bgzf_inflate": (C.c_int, [C.c_int, C.c_char_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "vlr_ingest_device_timings": (None, [C.POINTER(C.c_double), C.c_int]),
    "vlr_ingest_device_trim": (None, []),
}

# exported by the library without a declaration in the header: developer aids that a test and a tool read
INTERNAL_SIGNATURES = {
    "vlr_launch_realign_pairs_per_wave": (C.c_int, []),                              # realign.last_pairs_per_wave
    "vlr_plan_profile_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),  # tools/profile_phases.py
}
