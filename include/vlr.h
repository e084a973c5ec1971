/*
 * vlr.h — C ABI of the MI355X-native per-locus Bayesian likelihood engine
 * (drop-in for the model-evaluation path of `varlociraptor call variants`).
 *
 * The reference (Rust, /root/reference = varlociraptor v8.9.3) has no FFI boundary;
 * the path sits behind the in-process trait boundary
 *     bio::stats::bayesian::model::Model::compute(events, &Data) -> ModelInstance
 * invoked once per record at src/calling/variants/calling.rs:760 (inside
 * Caller::call_record, calling.rs:720-842) and consumed by calling.rs:762-813 and
 * sample_infos (calling.rs:844-937).  This header is what a Rust `extern "C"` block
 * in calling.rs would bind instead: one *plan* per
 * (scenario, contig) replaces configure_model (calling.rs:632-718) and one
 * *batch run* replaces the per-record call_record loop for many records at once.
 *
 * Conventions
 *   - all functions return 0 (VLR_OK) or a negative vlr_status error code;
 *     vlr_last_error() gives a thread-local human readable message.
 *   - numeric invariants the reference enforces with assert!/panic!
 *     (likelihood.rs:113,150,191,217; modes/generic.rs:228) are surfaced per locus
 *     in vlr_results.status instead of aborting.
 *   - no torch / C++ types; plain pointers and sizes only.  Pointers inside
 *     vlr_batch / vlr_results are DEVICE pointers for vlr_batch_run and HOST
 *     pointers for vlr_batch_run_host.
 *   - results are in input order; loci are independent.
 *   - thread-safe across plans; a plan may be used from one thread at a time.
 */
#ifndef VLR_H
#define VLR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLR_ABI_VERSION 14  /* 3: vlr_plan_reserve takes the AFD capacity, 30 named events, vlr_node_*, homopolymer realignment; 4: device front door;
                             * 5: sharded device reader, calls-file parts, vlr_ingest_device_trim, CRC32 of BGZF members checked by both readers;
                             * 6: calls emission on the device — vlr_results.afd_text (FORMAT/AFD text), OBS text in the observation summaries,
                             *    vlr_obs_table_summaries;
                             * 7: vlr_contamination_posterior (`estimate contamination`);
                             * 8: vlr_bamstats_* (`estimate alignment-properties`);
                             * 9: vlr_posterior_odds_keep, vlr_range_group_lse, vlr_calls_filter_odds, vlr_calls_mutational_burden
                             *    (`filter-calls posterior-odds`, `estimate mutational-burden`);
                             * 10: vlr_basepileup_* (SNV / MNV allele supports from BAM records);
                             * 11: vlr_plan_fused_counters (the fused coefficient pass of the lean call kernel);
                             * 12: vlr_indelpileup_* (indel allele supports from BAM records);
                             * 13: vlr_fragpileup_* (fragment observations of SNV / MNV candidates from BAM records);
                             * 14: vlr_fragpileup_open_realign / _realign_result / _read_realigned (indel-bearing reads over SNV / MNV
                             *     candidates realigned inside the fragment session); still 14, purely additive: vlr_fragpileup_open_indel /
                             *     _read_indel (fragments of deletion / insertion candidates in the fragment session) and
                             *     vlr_fragpileup_open_methylation / vlr_methylation_tables (fragments of <METH> candidates); added within 14 as
                             *     well: vlr_fragpileup_set_alt_variants / _alt_result / _read_alt_variants (the other alleles of a locus on the
                             *     reference side of a realigned evidence) */
#define VLR_MAX_SAMPLES 16     /* samples per scenario supported by the device path   */
#define VLR_N_BIAS      6      /* strand, orientation, position, softclip, homopolymer, alt-locus */

/* ---------------------------------------------------------------- status codes */
typedef enum {
    VLR_OK                    = 0,
    VLR_ERR_INVALID_ARGUMENT  = -1,
    VLR_ERR_UNSUPPORTED       = -2,  /* scenario feature outside the device path */
    VLR_ERR_NO_DEVICE         = -3,  /* HIP runtime/device missing: the product path never falls back to CPU */
    VLR_ERR_HIP               = -4,
    VLR_ERR_INVALID_PRIOR     = -5,  /* prior.rs:788-825 CheckablePrior::check */
    VLR_ERR_OUT_OF_MEMORY     = -6
} vlr_status;

/* per-locus status bits (vlr_results.status) */
#define VLR_LOCUS_OK            0u
#define VLR_LOCUS_NAN           (1u << 0)  /* a density/likelihood became NaN (reference: panic)        */
#define VLR_LOCUS_UNDERFLOW     (1u << 1)  /* a per-observation likelihood left the f64 linear range    */
#define VLR_LOCUS_TABLE_FULL    (1u << 2)  /* visited-point table of a range chain overflowed           */
#define VLR_LOCUS_TOO_DEEP      (1u << 3)  /* pileup larger than the plan's LDS budget                  */
#define VLR_LOCUS_MISSING_DATA  (1u << 4)  /* all pileups empty (calling/variants/mod.rs:423-430)       */
#define VLR_LOCUS_SINGLETON_ADJ (1u << 5)  /* Hint::AdjustedSingletonEvidence (calling.rs:613-617)      */
#define VLR_LOCUS_FILTERED_ALN  (1u << 6)  /* Hint::FilteredNonStandardAlignments (calling.rs:618-622)  */

/* ---------------------------------------------------------------- scenario description
 * Flattened form of grammar::Scenario after normalisation for ONE contig
 * (grammar/mod.rs:129-279, grammar/vaftree.rs:168-305).  Samples are indexed in
 * BTreeMap key order (grammar/mod.rs:178-190).                                         */

typedef enum { VLR_SPECTRUM_SET = 0, VLR_SPECTRUM_RANGE = 1 } vlr_spectrum_kind;

/* grammar/formula.rs:1018-1047 VAFSpectrum, 1049-1056 VAFRange */
typedef struct {
    int32_t kind;            /* vlr_spectrum_kind */
    int32_t set_offset;      /* SET: first member in vlr_scenario_desc.vafs (ascending)  */
    int32_t set_len;         /* SET: number of members                                  */
    int32_t left_exclusive;  /* RANGE */
    int32_t right_exclusive; /* RANGE */
    int32_t _pad;
    double  start, end;      /* RANGE */
} vlr_spectrum;

/* utils/comparison.rs:4-12 */
typedef enum {
    VLR_CMP_EQUAL = 0, VLR_CMP_GREATER = 1, VLR_CMP_GREATER_EQUAL = 2,
    VLR_CMP_LESS = 3, VLR_CMP_LESS_EQUAL = 4, VLR_CMP_NOT_EQUAL = 5
} vlr_cmp;

/* grammar/vaftree.rs:63-81 NodeKind */
typedef enum {
    VLR_NODE_SAMPLE = 0, VLR_NODE_LFC = 1, VLR_NODE_VARIANT = 2,
    VLR_NODE_TRUE = 3, VLR_NODE_FALSE = 4
} vlr_node_kind;

typedef struct {
    int32_t kind;          /* vlr_node_kind                                              */
    int32_t sample;        /* SAMPLE: sample index; LFC: sample_a                        */
    int32_t sample_b;      /* LFC                                                        */
    int32_t cmp;           /* LFC: vlr_cmp (utils/log2_fold_change.rs:28-31)             */
    double  lfc_value;     /* LFC                                                        */
    vlr_spectrum vafs;     /* SAMPLE                                                     */
    int32_t positive;      /* VARIANT                                                    */
    uint8_t refbase;       /* VARIANT: IUPAC code (grammar/formula.rs:20-43)             */
    uint8_t altbase;
    uint8_t _pad[2];
    int32_t child_offset;  /* children = child_index[child_offset .. +n_children]        */
    int32_t n_children;
} vlr_node;

/* variants/model/prior.rs:41-46 */
typedef enum {
    VLR_INHERIT_NONE = 0, VLR_INHERIT_MENDELIAN = 1, VLR_INHERIT_CLONAL = 2, VLR_INHERIT_SUBCLONAL = 3
} vlr_inheritance_kind;

typedef struct {
    int32_t kind;      /* vlr_inheritance_kind */
    int32_t from0;     /* parent sample index  */
    int32_t from1;     /* second parent (mendelian) */
    int32_t somatic;   /* clonal: somatic flag */
} vlr_inheritance;

/* variants/model/mod.rs:139-160 VariantType, collapsed to what the path distinguishes
 * (grammar/mod.rs:420-431 VariantTypeFraction::get, calling.rs:517-534 is_snv_or_mnv) */
typedef enum {
    VLR_VT_SNV = 0, VLR_VT_MNV = 1, VLR_VT_INDEL = 2 /* INS|DEL|REP */, VLR_VT_SV = 3 /* INV|BND|DUP */,
    VLR_VT_OTHER = 4 /* METH, REF */, VLR_N_VARIANT_TYPES = 5
} vlr_variant_type;

typedef struct {
    int32_t n_samples;
    /* per sample [n_samples] */
    const double*  resolution;             /* grammar/mod.rs:445-447 (default 0.01)                    */
    const int32_t* contaminated_by;        /* -1: SampleModel::Normal; else Contaminated{by} (modes/generic.rs:464-470) */
    const double*  contamination_fraction; /* purity = 1 - fraction (modes/generic.rs:482-484)         */
    const int32_t* universe_offset;        /* [n_samples+1] into universe[]; Sample::contig_universe (grammar/mod.rs:503-579) */
    const vlr_spectrum* universe;
    /* prior (variants/model/prior.rs:61-80; calling.rs:1072-1087) */
    const uint8_t* uniform_prior;          /* sample declares `universe`                               */
    const int32_t* ploidy;                 /* -1 = None                                                */
    const double*  germline_mutation_rate;            /* NaN = None */
    const double*  somatic_effective_mutation_rate;   /* NaN = None */
    const vlr_inheritance* inheritance;
    double  heterozygosity;                /* species heterozygosity as plain probability; NaN = None  */
    double  fraction_indel, fraction_mnv, fraction_sv;  /* VariantTypeFraction (defaults 0.0125/0.001/0.01) */
    int32_t is_absent_only;                /* !--full-prior (calling.rs:1086)                          */
    /* event universe of the scenario, WITHOUT `absent` and without artifact twins
     * (both are added by the engine exactly like calling.rs:654-687); events must be given
     * in ascending name order (BTreeMap order of grammar/mod.rs:137).  At most 62 (more than 30: the
     * wide build of the kernels; VLR_ERR_UNSUPPORTED above).                                          */
    int32_t n_events;
    const char* const* event_names;
    const int32_t* event_root_offset;      /* [n_events+1] into root_index[]                           */
    const int32_t* root_index;             /* node ids of the VAFTree roots of each event              */
    int32_t n_nodes;
    const vlr_node* nodes;
    const int32_t* child_index;
    const double*  vafs;                   /* pool for SET spectra                                     */
    /* per-variant prior overrides from the candidate record's INFO HETEROZYGOSITY / SOMATIC_EFFECTIVE_MUTATION_RATE
     * (PHRED in the file, calling.rs:470-494), as LogProb; NaN = None.  The reference installs them together with the
     * contig's universe (calling.rs:704-713), i.e. they are plan data: when present they replace the (variant-type
     * scaled) species heterozygosity / the per-sample somatic rates (prior.rs:250-270).                          */
    double  variant_heterozygosity_ln;
    double  variant_somatic_effective_mutation_rate_ln;
} vlr_scenario_desc;

/* ---------------------------------------------------------------- observations (SoA)
 * One entry per ReadObservation (variants/evidence/observations/read_observation.rs:219-278)
 * as decoded from observation-format v15 (calling/variants/preprocessing/mod.rs:818-919).
 * All log-probabilities are MiniLogProb f16/f32 in the wire format (utils/mod.rs:449-474), so
 * f32 columns are lossless.  prob_mismapping / prob_single_overlap are derived
 * (read_observation.rs:283-292).                                                                     */

/* packed per-observation flags */
#define VLR_F_STRAND_SHIFT   0   /* 2 bits: 0 Forward 1 Reverse 2 Both 3 None (read_observation.rs:51-57)         */
#define VLR_F_ORIENT_SHIFT   2   /* 2 bits: 0 F1R2 1 F2R1 2 None 3 other/non-standard (bio_types SequenceReadPairOrientation) */
#define VLR_F_READPOS_MAJOR  (1u << 4)   /* ReadPosition::Major (read_observation.rs:125-129)                     */
#define VLR_F_SOFTCLIPPED    (1u << 5)
#define VLR_F_PAIRED         (1u << 6)
#define VLR_F_MAX_MAPQ       (1u << 7)
#define VLR_F_ALTLOCUS_SHIFT 8   /* 2 bits: 0 Major 1 Some 2 None (read_observation.rs:213-217)                   */
#define VLR_F_HP_LEN_VALID   (1u << 10)  /* homopolymer_indel_len is Some                                         */
#define VLR_F_HP_LEN_SHIFT   16  /* 8 bits: homopolymer_indel_len as int8                                         */

#define VLR_STRAND_FORWARD 0
#define VLR_STRAND_REVERSE 1
#define VLR_STRAND_BOTH    2
#define VLR_STRAND_NONE    3
#define VLR_ORIENT_F1R2    0
#define VLR_ORIENT_F2R1    1
#define VLR_ORIENT_NONE    2
#define VLR_ORIENT_OTHER   3
#define VLR_ALTLOCUS_MAJOR 0
#define VLR_ALTLOCUS_SOME  1
#define VLR_ALTLOCUS_NONE  2

/* bias-enable mask per locus = WorkItem.check_* (calling.rs:557-567) */
#define VLR_BIAS_STRAND      (1u << 0)
#define VLR_BIAS_ORIENTATION (1u << 1)
#define VLR_BIAS_POSITION    (1u << 2)
#define VLR_BIAS_SOFTCLIP    (1u << 3)
#define VLR_BIAS_HOMOPOLYMER (1u << 4)
#define VLR_BIAS_ALTLOCUS    (1u << 5)
/* locus flag: Pileup::remove_nonstandard_alignments applies (is_snv_or_mnv && !omit_read_orientation_bias;
 * calling.rs:590-598, pileup.rs:26-43) */
#define VLR_LOCUS_REMOVE_NONSTANDARD (1u << 6)
/* locus flag: record is an SNV (ref/alt single base) so Data.snv is Some (calling.rs:517-524) */
#define VLR_LOCUS_HAS_SNV    (1u << 7)

typedef struct {
    int64_t n_loci;
    int32_t n_samples;
    int32_t _pad;
    int64_t n_obs;                    /* total observations = obs_offset[n_loci*n_samples]               */
    /* pileup p = locus*n_samples + sample covers observations [obs_offset[p], obs_offset[p+1])           */
    const uint32_t* obs_offset;       /* [n_loci*n_samples + 1]                                           */
    const float* prob_mapping;        /* ln P(correctly mapped), already MAPQ-adjusted (preprocessing/mod.rs:951) */
    const float* prob_alt;
    const float* prob_ref;
    const float* prob_missed_allele;
    const float* prob_sample_alt;
    const float* prob_double_overlap;
    const float* prob_hit_base;
    const float* prob_hp_artifact;    /* prob_observable_at_homopolymer_artifact; NaN = None; column may be NULL */
    const float* prob_hp_variant;     /* prob_observable_at_homopolymer_variant;  NaN = None; column may be NULL */
    const uint32_t* flags;            /* VLR_F_*                                                          */
    /* per locus */
    const uint8_t* locus_flags;       /* VLR_BIAS_* | VLR_LOCUS_REMOVE_NONSTANDARD | VLR_LOCUS_HAS_SNV     */
    const uint8_t* variant_type;      /* vlr_variant_type (prior's variant_type_fraction)                 */
    const uint8_t* ref_base;          /* SNV only (modes/generic.rs:18-22)                                */
    const uint8_t* alt_base;
} vlr_batch;

/* ---------------------------------------------------------------- results
 * What calling.rs:762-813 + sample_infos (844-937) extract from the ModelInstance.                     */
typedef struct {
    int64_t n_loci;
    int32_t n_out;          /* = n_events + 2                                                             */
    int32_t n_samples;
    /* ln posterior probabilities [n_loci * n_out]: column 0 = `absent`, 1..n_events = scenario events
     * (clean twins, in the order of vlr_scenario_desc), n_events+1 = `artifact`
     * (ln-sum over artifact twins; calling.rs:785-799).  PROB_* in the BCF = -10/ln10 * value.           */
    double*  ln_posterior;
    double*  ln_marginal;   /* [n_loci] ln marginal of Model::compute (may be NULL)                       */
    double*  map_vaf;       /* [n_loci * n_samples] FORMAT/AF: MAP allele frequency; 0 if MAP is an artifact (calling.rs:875-887); NaN if no MAP */
    /* [n_loci * VLR_N_BIAS] bias state of the MAP estimate, identical for all samples of a locus
     * (modes/generic.rs:248-257): 0 = none, else strand 1 '+',2 '-'; orientation 1 '>',2 '<'; others 1.  */
    uint8_t* map_bias;
    int32_t* best_event;    /* [n_loci] index into the engine's event universe: 0 absent, 1+2*e clean e, 2+2*e artifact twin (may be NULL) */
    uint32_t* status;       /* [n_loci] VLR_LOCUS_* bits                                                   */
    /* optional AFD (calling.rs:889-928; FORMAT/AFD): for locus l and sample s the entries
     * afd_vaf/afd_lnprob[(l*S+s)*afd_capacity .. + min(afd_count[l*S+s], afd_capacity)]; unordered;
     * all NULL to skip.                                                                                  */
    int32_t  afd_capacity;
    int32_t  _pad;
    int32_t* afd_count;     /* [n_loci * n_samples]                                                        */
    double*  afd_vaf;       /* [n_loci * n_samples * afd_capacity] (f64: the BCF prints it with 3 decimals)      */
    double*  afd_lnprob;    /* [n_loci * n_samples * afd_capacity]                                         */
    /* (ABI 6) optional FORMAT/AFD TEXT, written on the device by vlr_batch_run_host / vlr_batch_run_device_in / vlr_node_batch_run_host
     * (HOST pointers; needs the afd_* buffers above): the list of locus l and sample s in the order and format of
     * Call::write_final_record (calling/variants/mod.rs:473-559) — entries by ascending allele frequency (stable), "%.3f=%.2f" of
     * (vaf, -10 ln p / ln 10) joined by ',' — at afd_text[afd_text_span[2 p] .. + afd_text_span[2 p + 1]], p = l * n_samples + s.
     * A length of 0xffffffff: not formatted (a value beyond 1e12, a NaN allele frequency, more than 1 024 entries, text buffer full) —
     * the list is in afd_vaf / afd_lnprob then, which are only copied to the host when some list of the call needs them.
     * vlr_calls_write / vlr_calls_writer_append take the text where it is given.  NULL: no text. */
    uint8_t*  afd_text;
    uint64_t  afd_text_capacity;
    uint32_t* afd_text_span;   /* [n_loci * n_samples * 2] */
} vlr_results;

/* ---------------------------------------------------------------- entry points */
typedef struct vlr_plan vlr_plan;

/* ABI version of the loaded library. */
int  vlr_abi_version(void);
/* Identity of the build: "<sha1 of the engine sources and the Makefile>" (measurement files under profiles/ carry the id of
 * the build they were taken from; the build-matrix test refuses variants built from other sources). */
const char* vlr_build_id(void);
/* Thread-local message of the last error. */
const char* vlr_last_error(void);

/* Compile a scenario (one contig) into a device plan: flattened VAFTrees, event universe incl.
 * `absent` and artifact twins, prior table, contamination wiring.  Replaces
 * Caller::configure_model (calling.rs:632-718) + GenericModelBuilder::build (modes/generic.rs:93-105). */
int  vlr_plan_create(const vlr_scenario_desc* scenario, int device, vlr_plan** out);
void vlr_plan_destroy(vlr_plan* plan);
/* Number of result columns (n_events + 2) and of engine events (1 + 2*n_events). */
int  vlr_plan_n_out(const vlr_plan* plan);
int  vlr_plan_n_samples(const vlr_plan* plan);

/* LDS budget knob: maximum pileup depth per sample the kernel reserves coefficient space for
 * (default 200 = the reference's max_depth default, src/variants/sample.rs:236).  Loci whose kept
 * observations exceed n_samples * depth are reported with VLR_LOCUS_TOO_DEEP.                           */
int  vlr_plan_set_max_depth(vlr_plan* plan, int per_sample_depth);

/* Finer form of the same knob: maximum number of kept observations of ONE locus summed over its samples.  A
 * caller that knows its batch (it decoded the pileups) sets this to the batch maximum: less LDS per
 * workgroup = more resident waves.  vlr_batch_run_host does this automatically.                          */
int  vlr_plan_set_max_obs(vlr_plan* plan, int max_obs_per_locus);

/* The same knob set FROM the batch: `obs_offset_host` are the n_loci * n_samples + 1 pileup offsets of the batch in host memory.
 * Picks the deepest locus — or, where a slightly smaller budget lets sixteen workgroups share a CU (the launcher then runs the
 * kernel build with four waves per SIMD), that budget, provided no locus exceeds it or at most 0.5 % of a batch of 100 000 loci or
 * more do; those take the deep launch (coefficients in the plan's HBM pool) like every locus above the LDS budget.  Returns the
 * budget (>= 1) or an error (< 0).  vlr_batch_run_host applies the same rule per chunk; callers of vlr_batch_run with device
 * batches call this.  (The reference has no such knob: its per-sample depth limit is preprocess's --max-depth, sample.rs:236.) */
int  vlr_plan_fit_max_obs(vlr_plan* plan, const uint32_t* obs_offset_host, int64_t n_loci);

/* Evaluate a batch of loci on the plan's device.  All pointers in `in` / `out` are device pointers.
 * `stream` is a hipStream_t (NULL = default stream); the call is stream-ordered and does not synchronise.
 * Replaces the per-record Caller::call_record (calling.rs:720-842) for n_loci records.                  */
int  vlr_batch_run(vlr_plan* plan, const vlr_batch* in, vlr_results* out, void* stream);

/* Same, but `in` / `out` hold host pointers: stages through device buffers owned by the plan,
 * synchronises before returning.  Still requires the GPU (no CPU fallback).                             */
int  vlr_batch_run_host(vlr_plan* plan, const vlr_batch* in, vlr_results* out);

/* (ABI 4) Device columns in, host results out: `in` holds DEVICE pointers (the batch of a device reader,
 * vlr_obs_table_device_batch), obs_offset_host is the host copy of in->obs_offset (vlr_obs_table_batch), `out` holds HOST
 * pointers.  Only the result buffers are staged; synchronises before returning.                              */
int  vlr_batch_run_device_in(vlr_plan* plan, const vlr_batch* in, const uint32_t* obs_offset_host, vlr_results* out);

/* ------------------------------------------------------------------------------------------------
 * One node, several devices (SURVEY.md 8 e): what the batching shim in Caller::call
 * (/root/reference/src/calling/variants/calling.rs:320-455) binds when the host drives N GPUs from ONE process.
 * vlr_node_create compiles the scenario once per device (devices = NULL, n_devices <= 0: every visible device; the same
 * device may be listed twice — two plans, two streams); vlr_node_batch_run_host cuts the host batch into the contiguous
 * blocks of vlr_node_shard_range (ceil(n / G) loci each, input order — the caller has already collapsed breakend groups
 * to their representatives, calling.rs:569-580, so no group straddles a shard), runs vlr_batch_run_host on one thread and
 * plan per device and returns when every record and AFD list sits at its input position in the caller's arrays.  No
 * collective: inside one process the shards write disjoint ranges of host memory (the multi-process harness,
 * varlociraptor_amd/dist.py, reassembles with one RCCL all-gather instead).  Errors: the first failing shard's code, its
 * message prefixed with the device.                                                                   */
typedef struct vlr_gpu_node vlr_gpu_node;
int  vlr_node_create(const vlr_scenario_desc* desc, int n_devices, const int* devices, vlr_gpu_node** out);
void vlr_node_destroy(vlr_gpu_node* node);
int  vlr_node_n_devices(const vlr_gpu_node* node);
int  vlr_node_device(const vlr_gpu_node* node, int shard);               /* HIP device of shard r */
vlr_plan* vlr_node_plan(vlr_gpu_node* node, int shard);                  /* borrowed: per-device knobs, counters */
int  vlr_node_set_max_depth(vlr_gpu_node* node, int per_sample_depth);   /* vlr_plan_set_max_depth on every plan */
int  vlr_node_set_max_obs(vlr_gpu_node* node, int max_obs_per_locus);
int  vlr_node_shard_range(int64_t n_loci, int n_shards, int shard, int64_t* l0, int64_t* l1);  /* pure arithmetic, no device */
int  vlr_node_batch_run_host(vlr_gpu_node* node, const vlr_batch* in, vlr_results* out);

/* Page-locked host memory for the arrays handed to vlr_batch_run_host (columns in, results out).  The staging
 * copies of vlr_batch_run_host are asynchronous; from pageable memory the runtime bounces them through its own
 * pinned buffer (about 14 GB/s here), from memory obtained here they are direct DMA and overlap the kernel of the
 * previous chunk.  The reference-side binding decodes the observation records (calling.rs:720-760) straight into
 * such arrays.  vlr_host_alloc returns NULL on failure (see vlr_last_error); vlr_host_free(NULL) is a no-op. */
void* vlr_host_alloc(size_t bytes);
void  vlr_host_free(void* p);

/* Size the plan's own device buffers (kernel scratch; with_afd != 0: AFD scratch and log) for batches of up to n_loci loci of
 * at most the configured observation count.  vlr_batch_run grows them on demand with hipMalloc/hipFree, which synchronise the
 * device: after vlr_plan_reserve with the largest batch size, vlr_batch_run only enqueues work on the stream.
 * with_afd: 0, or the afd_capacity of the result buffers that will be passed (1 if unknown: the per-entry key buffer is then grown by
 * the first vlr_batch_run).  The AFD log is budgeted (4 GiB per staging slot, VLR_AFD_LOG_BUDGET_MB): larger batches are walked in
 * sub-ranges of loci that share it.  Both staging slots of vlr_batch_run_host are sized. */
int  vlr_plan_reserve(vlr_plan* plan, int64_t n_loci, int with_afd);

/* Duration in milliseconds of the most recent kernel launch sequence of vlr_batch_run on this plan,
 * measured with HIP events on the launch stream (synchronises on the stop event).  For bench.py.       */
int  vlr_plan_last_kernel_ms(vlr_plan* plan, float* ms);

/* Measurement aid: which build of the call kernel the plan's most recent call launch took — *waves: its instance (waves per SIMD:
 * 2, 3, 4 or 6), *lean: 1 for the lean build (plans that need none of what it leaves out, launched without AFD lists;
 * VLR_NO_LEAN=1 forces the general build), 0 for the general or the wide build.                        */
int  vlr_plan_last_instance(const vlr_plan* plan, int* waves, int* lean);

/* Profiling aid: cumulative {pileup-likelihood evaluations, observation terms} executed by the kernels of this
 * plan since creation (or the last reset); synchronises the device.                                     */
int  vlr_plan_work_counters(vlr_plan* plan, unsigned long long* out2, int reset);

/* Measurement aid for the fused coefficient pass of the lean call kernel (two-sample plans launched without AFD lists): where
 * artifact hypotheses survive the gates of a locus, the surviving hypotheses are taken in groups of up to three: ONE pass over
 * the observation rows builds the coefficients of the group's first hypothesis and of the next two, whose sets are parked in
 * plan-owned device memory and reloaded at their turn (the two sets of a locus are reused by the next group).  out4 = cumulative {fused row passes, sets parked, sets reloaded, hypotheses redone by a row pass of
 * their own: rescue / all-ones terms, a hypothesis left alone in its group, or no parked set at all} since creation or the last reset (`reset` clears these four alone);
 * synchronises the device.  VLR_NO_FUSED_COEF=1, read per launch, keeps one row pass per hypothesis (all four stay 0);
 * VLR_FUSED_SETS=0|1 lowers the parked sets per locus.                                                 */
int  vlr_plan_fused_counters(vlr_plan* plan, unsigned long long* out4, int reset);

/* ------------------------------------------------------------------------------------------------
 * Read-vs-allele pair HMM: ln P(read window | allele) for a batch of pairs.
 * Replaces, batched, PairHMMRealigner::calculate_prob_allele -> bio PairHMM::prob_related
 * (/root/reference/src/variants/evidence/realignment/mod.rs:519-537) with the emission model of
 * realignment/pairhmm.rs:296-455 (match: 1 - P(miscall), mismatch: P(miscall) * 0.3333, insertion: P(miscall),
 * P(miscall) = 10^(-qual/10)), semiglobal in the allele (free start and end gaps, pairhmm.rs:186-205).
 * The caller (Realigner::allele_support, mod.rs:161-424) keeps the edit-distance pre-filter, builds the allele
 * windows (shrink_to_hit, pairhmm.rs:66-72) and normalises ref against alt.
 *
 * Pair p: allele bases x_bases[x_offset[p] .. x_offset[p+1]) (ASCII, case-insensitive), read window
 * y_bases / y_quals [y_offset[p] .. y_offset[p+1]) (ASCII bases, PHRED qualities without offset), at most 128 read bases
 * (EditDistanceCalculation::max_pattern_len, edit_distance.rs:145-147).  Qualities above 93 — the largest PHRED value a
 * SAM / FASTQ record can hold — are out of range: the scaling of the summing kernels is dimensioned for error
 * probabilities down to 10^-9.3.  max_edit_dist[p] >= 0 restricts the matrix
 * to cells reachable with at most that many edits (band = hit distance + 4, pairhmm.rs:20); < 0 or a NULL array:
 * full matrix.  gap[] = ln { P(gap in x) = prob_insertion_artifact, P(gap in y) = prob_deletion_artifact,
 * P(extend gap in x), P(extend gap in y) } (pairhmm.rs:119-180; -inf = no extension, the default); P(gap in x) +
 * P(gap in y) above one (beyond rounding) leaves no probability for a match and is VLR_ERR_INVALID_ARGUMENT.
 * ln_prob[p] <- result, -inf for an empty sequence, NaN for a read window above 128 bases.            */
typedef struct vlr_realign_batch_desc {
    int64_t n_pairs;
    const uint32_t* x_offset;       /* [n_pairs + 1] */
    const uint8_t*  x_bases;
    const uint32_t* y_offset;       /* [n_pairs + 1] */
    const uint8_t*  y_bases;
    const uint8_t*  y_quals;
    const int32_t*  max_edit_dist;  /* [n_pairs] or NULL */
    double gap[4];
} vlr_realign_batch_desc;

/* Device pointers, stream-ordered, no synchronisation. */
int vlr_realign_batch(int device, const vlr_realign_batch_desc* pairs, double* ln_prob, void* hip_stream);
/* Host pointers: stages the sequences, runs the kernel, returns when ln_prob is filled. */
int vlr_realign_batch_host(int device, const vlr_realign_batch_desc* pairs, double* ln_prob);

/* The `fast` realignment mode (--pairhmm-mode fast): replaces PathHMMRealigner::calculate_prob_allele
 * (/root/reference/src/variants/evidence/realignment/mod.rs:547-678) — the path probability of an optimal edit-distance alignment
 * (transition terms by the previous operation, emissions as above), best over the hit's alignments.  The reference takes the
 * alignments from bio's Myers traceback, which does not specify the choice among co-optimal alignments; ln_prob[p] here is the
 * best path probability over ALL alignments of minimal semiglobal edit distance (equal when unique, an upper bound otherwise).
 * max_edit_dist is not read.  Same conventions as vlr_realign_batch. */
int vlr_realign_fast_batch(int device, const vlr_realign_batch_desc* pairs, double* ln_prob, void* hip_stream);
int vlr_realign_fast_batch_host(int device, const vlr_realign_batch_desc* pairs, double* ln_prob);

/* The `homopolymer` realignment mode (--pairhmm-mode homopolymer, /root/reference/src/cli.rs:912-947): replaces
 * HomopolyPairHMMRealigner::calculate_prob_allele (/root/reference/src/variants/evidence/realignment/mod.rs:680-730) -> bio
 * HomopolyPairHMM::prob_related — the pair HMM of vlr_realign_batch with per-base hop states for homopolymer run errors (the mode
 * the reference's nanopore / PCR-homopolymer testcases run).  hop[16] = ln of HopParams (realignment/pairhmm.rs:207-295), each
 * group in the order A, C, G, T: prob_seq_homopolymer (start a run error in the read), prob_ref_homopolymer (in the allele),
 * prob_seq_extend_homopolymer, prob_ref_extend_homopolymer; -inf = impossible (the reference's default for all sixteen, which
 * makes the mode equal to vlr_realign_batch).  Same batch layout, band and result conventions as vlr_realign_batch. */
int vlr_realign_homopolymer_batch(int device, const vlr_realign_batch_desc* pairs, const double* hop, double* ln_prob, void* hip_stream);
int vlr_realign_homopolymer_batch_host(int device, const vlr_realign_batch_desc* pairs, const double* hop, double* ln_prob);

/* Edit-distance pre-filter of the same pairs: replaces EditDistanceCalculation::calc_best_hit
 * (/root/reference/src/variants/evidence/realignment/edit_distance.rs:164-260, bio Myers find_all_lazy) as far as
 * Realigner::prob_allele and the band of the pair HMM use it.  dist[p] = smallest semiglobal edit distance of the read
 * window against the allele window (free start and end in the allele; bases compared case-insensitively), end[p] = first
 * allele position (exclusive, 1-based) at which an alignment with that distance ends, n_hits[p] = number of such end
 * positions; dist = -1 for an empty sequence or a read window above 128 bases.  `end` and `n_hits` may be NULL.  y_quals,
 * max_edit_dist and gap of `pairs` are not read.  The band of vlr_realign_batch is max_edit_dist[p] = dist[p] + 4. */
int vlr_edit_distance_batch(int device, const vlr_realign_batch_desc* pairs, int32_t* dist, int32_t* end, int32_t* n_hits, void* hip_stream);
int vlr_edit_distance_batch_host(int device, const vlr_realign_batch_desc* pairs, int32_t* dist, int32_t* end, int32_t* n_hits);

/* ------------------------------------------------------------------------------------------------
 * Bayesian FDR control: the threshold search of `filter-calls control-fdr`
 * (/root/reference/src/filtration/fdr.rs:107-141): sort the posterior (ln) probabilities of the chosen events in
 * descending order, PEP = 1 - p (with smart != 0 the probabilities are first converted to 1 - p: they are PROB_ABSENT
 * [+ PROB_ARTIFACT] sums, fdr.rs:96-114), expected FDR = running mean of the PEPs (bio expected_fdr), threshold = probability of
 * the last entry whose expected FDR is <= alpha and whose PEP differs from its predecessor's.  ln_prob: host array of n
 * values (utils::collect_prob_dist, utils/mod.rs:236-270, any order).  *status: VLR_FDR_EMPTY (no values: the reference's
 * None), VLR_FDR_VALUE (*threshold set), VLR_FDR_LN_ONE (already the best entry exceeds alpha: threshold = ln 1),
 * VLR_FDR_NONE (no admissible entry: None).  The filtering pass (utils/mod.rs:288-374) stays with the caller. */
enum { VLR_FDR_EMPTY = 0, VLR_FDR_VALUE = 1, VLR_FDR_LN_ONE = 2, VLR_FDR_NONE = 3 };
int vlr_fdr_threshold(int device, const double* ln_prob, int64_t n, int smart, double alpha_ln, double* threshold, int* status);

/* ------------------------------------------------------------------------------------------------
 * Contamination estimation: the posterior grid of `estimate contamination` (estimation/contamination.rs:160-224).
 * Events: maximum somatic VAF mv_m in (0.25, 0.5, 0.75, 1.0) x contamination c_i = 0.0 + 0.01 i (i = 0..100, linspace);
 * ln_joint[m * 101 + i] = ln_prior[i] + sum over the observations o of term(o, m, i), where, with purity = 1.0 - c_i,
 *   purity == 0 (i = 100): term = ln(1 - e^ln_prob_denovo[o])       (LogProb::ln_one_minus_exp);
 *   otherwise:             term = pdf_o((mv_m * purity) * (map_vaf[o] / max_vaf))   (left to right, no FMA),
 * pdf_o(x) over the list of o (list_vaf / list_lnprob[list_offset[o] .. list_offset[o + 1]], VAF strictly ascending):
 *   a key equal to x: its value; x strictly between two keys x_a < x < x_b with values a, b: linear interpolation of the
 *   densities in probability space, a.ln_add_exp(ln((e^b - e^a) / (x_b - x_a)) + ln(x - x_a)) on rising and flat segments
 *   (the reference's formula) and a.ln_sub_exp(ln|slope| + ln(x - x_a)) on falling ones (e^b < e^a; the reference takes the ln
 *   of a negative number there, NaN: a deliberate deviation; should rounding put the subtrahend at or above a,
 *   the value is b); x left of the first key, right of the last, in an empty list, or NaN (max_vaf = 0): -inf.
 * Summation order (fixed: independent of the launch geometry, the scheduling and of how the caller split its input): the
 *   observations in blocks of VLR_CONTAM_BLOCK consecutive ones, each block summed sequentially in record order starting from
 *   0.0, the block sums added sequentially in block order starting from 0.0, then ln_prior[i] added.  The same input gives the
 *   same bits.  n_obs = 0 is legal: every likelihood is 0 (ln_joint = ln_prior).
 * NaN / -inf: a -inf term makes its event's sum -inf (IEEE addition: a NaN term, or -inf next to +inf, gives NaN); inputs are
 *   not checked for NaN other than the keys (a NaN key or keys out of order = VLR_ERR_INVALID_ARGUMENT, as are offsets that
 *   do not start at 0 or decrease).
 * *ln_marginal (contamination.rs:196-224, host side): per mv_m ln_simpsons_integrate_exp over the 101 joints (weights 1, 4, 2,
 *   ..., 4, 1; + ln(1 - 0) - ln 100 - ln 3), then ln_sum_exp of the four integrals (bio semantics).
 *   The posterior of an event is ln_joint - *ln_marginal.  ln_prior: [101], tabulated by the caller (ln 1 without an estimate).
 * All pointers are host pointers; the function uploads, launches on `device` and copies back (synchronous). */
#define VLR_CONTAM_BLOCK 128
#define VLR_CONTAM_N_C   101
#define VLR_CONTAM_N_MV  4
int vlr_contamination_posterior(int device, int64_t n_obs, const int64_t* list_offset, const double* list_vaf, const double* list_lnprob,
                                const double* map_vaf, const double* ln_prob_denovo, double max_vaf, const double* ln_prior,
                                double* ln_joint, double* ln_marginal);

/* ------------------------------------------------------------------------------------------------
 * Alignment properties: the per-record pass of `estimate alignment-properties` (estimation/alignment_properties.rs:148-463 with
 * cigar_stats :693-861; omit_insert_size = false, as the CLI calls it).  The BAM files given to vlr_bamstats_add_bam, in that order,
 * are streamed through the device reader (BGZF members inflated on the device, BAM records split there); the first max_records
 * records that pass the skip rule (mapq 0, duplicate, QC fail, unmapped, empty SEQ: skipped; secondary / supplementary kept) are
 * analysed against the reference at fasta_path (its .fai is required; only the contigs the analysed records lie on are read and
 * uploaded, case preserved).  window_bytes: inflated bytes per split (0: 64 MiB; tests force small windows).
 * vlr_bamstats_result fills a vlr_bamstats_counts with the integer counts: transitions[from * 16 + to] over the states MatchA..T (0-3), GapX 4, GapY 5,
 *   HopAX 6, HopAY 7, ..., HopTY 13, Other 14; the maxima (max_del / max_ins -1 = none; has_softclip = 0: frac_max_softclip none);
 *   the flag counters of the reference's warning (over the analysed records); n_skipped: records in front of the cap the skip rule
 *   dropped.  seconds: [0] file read, [1] upload + inflate of the feeds, [2] record split, [3] take + select kernels, [4] reference
 *   upload, [5] statistics kernel, [6] insert sizes back to the host, [7] total, [8] inflate kernels alone, [9] splits that fell back to the serial walk.
 * vlr_bamstats_read then copies the homopolymer-run counters (CigarStats::hop_counts) in ascending key order, key = raw base byte
 *   << 56 | k0 << 28 | k1, and the insert sizes (|TLEN| of a paired first-in-template record with its mate on the same contig, or
 *   end - pos of an unpaired record whose first EF aux tag is an integer 1; records with an I, D, S or H operation give none) in
 *   record order.  The finishing math (percentiles, parameters, model, JSON) is the caller's (varlociraptor_amd/alignprops.py).
 * Errors (VLR_ERR_INVALID_ARGUMENT, the message names the file and the record number): a malformed or truncated record, a corrupt
 *   BGZF member, a CIGAR that runs past its contig or its read where the reference would index out of bounds, a reference id out of
 *   range, a contig missing from the FASTA, a homopolymer key >= 2^28 - 1.  Counts are sums of integers: bit-reproducible whatever
 *   the window size or the launch geometry. */
typedef struct vlr_bamstats vlr_bamstats;
typedef struct {
    uint64_t transitions[256];
    int64_t  n_taken, n_skipped, n_not_usable, n_softclips;
    int64_t  n_not_paired, n_not_first, n_mate_unmapped, n_tid_mismatch;
    int64_t  max_del, max_ins, max_read_len, max_mapq;
    double   frac_max_softclip;
    int64_t  has_softclip;
    int64_t  n_hop_keys, n_insert_sizes;
    double   seconds[10];
} vlr_bamstats_counts;
int  vlr_bamstats_open(int device, const char* fasta_path, int64_t max_records, int64_t window_bytes, vlr_bamstats** out);
int  vlr_bamstats_add_bam(vlr_bamstats* s, const char* bam_path);
int  vlr_bamstats_result(vlr_bamstats* s, vlr_bamstats_counts* out);
int  vlr_bamstats_read(vlr_bamstats* s, uint64_t* hop_keys, uint64_t* hop_counts, int64_t n_hop, int64_t* insert_sizes, int64_t n_insert);
void vlr_bamstats_close(vlr_bamstats* s);

/* ------------------------------------------------------------------------------------------------
 * SNV / MNV allele supports from BAM records: the no-realignment branch of Snv::allele_support_per_read (variants/types/snv.rs:66-150)
 * and Mnv::allele_support_per_read (variants/types/mnv.rs:73-205) for every (record, locus) pair of a BAM file, restated in
 * varlociraptor_amd/basecalls.py.  The file goes through the device reader exactly as for vlr_bamstats_add_bam (BGZF members inflated on
 * the device, BAM records split there); one thread per record decodes the fixed head, drops unmapped / secondary / duplicate / QC-fail
 * records (variants/sample.rs:281-286; supplementary ones stay), finds the loci the alignment encloses (SingleLocus::overlap without
 * clips == Enclosing, variants/types/mod.rs:440-473) and scores each from the read's own bases (variants/evidence/bases.rs).
 * Loci: n_loci candidates sorted by (ref_id, start) — ref_id = index of the contig in the BAM header —, len = number of bases (1 for
 *   VLR_BASEPILEUP_SNV, 2 .. VLR_BASEPILEUP_MAX_LEN for VLR_BASEPILEUP_MNV; longer MNVs are refused here and scored by the caller with
 *   the restatement), ref_bases / alt_bases: the upper-case alleles one behind the other in locus order (sum of len bytes each).
 * realign_indel_reads != 0: a record with an I or D operation is not scored for the loci it encloses; it comes back as a hit with
 *   VLR_BASEPILEUP_HIT_NEEDS_REALIGN and no probabilities (realigning against SNV / MNV emission parameters is not part of this path).
 * hit_capacity: hits the session's device buffer holds.  More hits than that: nothing is written past the buffer, the status word
 *   carries VLR_BASEPILEUP_OVERFLOW and needed_capacity the exact count — open again with that capacity.
 * window_bytes: inflated bytes per split (0: 64 MiB; any value >= 1 is legal: a feed holds at least one BGZF member, and a record
 *   longer than the window grows it).  The hits do not depend on it, bit for bit.
 * vlr_basepileup_result: the counts, the status word (VLR_BASEPILEUP_BAD_RECORD: a record whose lengths overrun its block_size, whose
 *   aux fields are malformed, whose CIGAR has an unknown operation or consumes more bases than l_seq, or a file that ends inside a
 *   record — such a record gives no hits and is never followed; the records in front of it are scored), seconds: [0] file read,
 *   [1] upload + inflate, [2] record split, [3] count + scan + fill kernels, [4] hits to the host and the locus-major order, [5] total,
 *   [6] inflate kernels alone.
 * vlr_basepileup_read copies the n_hits hits (n = n_hits of the result): locus-major, in record order within a locus; `record` counts
 *   the records of all files given to the session so far, in file order.  Bit-identical from run to run and for every window_bytes.
 * vlr_basepileup_tables: the tables the kernel scores with — call[q] = ln(1 - 10^(-q/10)) (LogProb::ln_one_minus_exp of the miscall
 *   probability), miscall[q] = -q ln(10) / 10 — so that a restatement run on them must agree bit for bit. */
#define VLR_BASEPILEUP_MAX_LEN 32
enum { VLR_BASEPILEUP_SNV = 0, VLR_BASEPILEUP_MNV = 1 };
/* status word of a session */
#define VLR_BASEPILEUP_BAD_RECORD (1u << 0)
#define VLR_BASEPILEUP_OVERFLOW   (1u << 1)
#define VLR_BASEPILEUP_GUARD_DAMAGED (1u << 2)  /* the guard words behind the hit buffer changed: a defect of the fill pass, never expected */
/* status byte of a hit */
#define VLR_BASEPILEUP_HIT_NEEDS_REALIGN           (1u << 0)
#define VLR_BASEPILEUP_HIT_READ_POS_OUT_OF_BOUNDS  (1u << 1)  /* SI:Z shorter than the read position (Error::ReadPosOutOfBounds)          */
#define VLR_BASEPILEUP_HIT_INVALID_STRAND_INFO     (1u << 2)  /* SI:Z character outside "+-*." (Error::InvalidStrandInfo)                */
#define VLR_BASEPILEUP_HIT_LEADING_REFSKIP         (1u << 3)  /* read_pos fails on a CIGAR that begins with N (rust-htslib)              */
#define VLR_BASEPILEUP_NO_READ_POSITION 0xffffffffu
typedef struct {
    double   prob_ref, prob_alt;   /* ln P(read | ref allele), ln P(read | alt allele)                                                 */
    uint64_t record;               /* ordinal of the record                                                                            */
    uint32_t locus;                /* index of the locus in the arrays given at open                                                   */
    uint32_t read_position;        /* position in the read, leading hard clips included; VLR_BASEPILEUP_NO_READ_POSITION               */
    uint32_t third_allele;         /* third-allele evidence (edit distance); 0 = none                                                  */
    uint16_t flag;                 /* the record's FLAG & (0x1 paired | 0x10 reverse | 0x40 first in template)                         */
    uint8_t  strand;               /* 0 forward, 1 reverse, 2 both, 3 none (the VLR_F_STRAND values)                                   */
    uint8_t  mapq;
    uint8_t  status;               /* VLR_BASEPILEUP_HIT_*                                                                             */
    uint8_t  pad[7];
} vlr_basepileup_hit;
typedef struct vlr_basepileup vlr_basepileup;
typedef struct {
    int64_t  n_hits, n_records, n_rejected, n_needs_realign;
    uint64_t status;               /* VLR_BASEPILEUP_BAD_RECORD | VLR_BASEPILEUP_OVERFLOW | VLR_BASEPILEUP_GUARD_DAMAGED               */
    int64_t  needed_capacity;      /* hits the input produces (== n_hits unless VLR_BASEPILEUP_OVERFLOW)                               */
    int64_t  first_bad_record;     /* ordinal of the first bad record, -1 = none                                                       */
    double   seconds[8];
} vlr_basepileup_counts;
int  vlr_basepileup_open(int device, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int32_t* len, const uint8_t* kind,
                         const uint8_t* ref_bases, const uint8_t* alt_bases, int realign_indel_reads, int64_t hit_capacity, int64_t window_bytes,
                         vlr_basepileup** out);
int  vlr_basepileup_add_bam(vlr_basepileup* s, const char* bam_path);
int  vlr_basepileup_result(vlr_basepileup* s, vlr_basepileup_counts* out);
int  vlr_basepileup_read(vlr_basepileup* s, vlr_basepileup_hit* hits, int64_t n);
int  vlr_basepileup_tables(double call[256], double miscall[256]);
void vlr_basepileup_close(vlr_basepileup* s);

/* ------------------------------------------------------------------------------------------------
 * Indel allele supports from BAM records: the single-locus part of Realigner::allele_support (variants/evidence/realignment/mod.rs:
 * 161-424) for every (record, locus) pair of a BAM file, restated in varlociraptor_amd/readwindows.py (`evidence`).  The file goes
 * through the device reader exactly as for vlr_basepileup_add_bam.  One thread per record decodes and validates the record (the decode
 * and the flag rule of vlr_basepileup_*: unmapped / secondary / duplicate / QC-fail records dropped, supplementary ones kept), finds
 * the loci its alignment with its soft clips overlaps, and computes the candidate region of each (Realigner::candidate_region,
 * mod.rs:58-153, on rust-htslib's read_pos(pos, include_softclips = true, include_dels = true)); one wave per evidence then copies the
 * read window (bases unpacked from the 4-bit SEQ, qualities), the ref allele window from the contig and the locus's alt allele window
 * into the pair arrays of vlr_realign_batch_desc — pair 2e = (ref allele, read), pair 2e + 1 = (alt allele, read) —, and the engine's
 * own kernels score them: the edit-distance kernel, band = distance + 4 (-1 where there is no hit), then the pair HMM of `mode`.
 * Loci: n_loci candidates sorted by (ref_id, start) — ref_id = index of the contig in the BAM header —, [start, end) the locus
 *   (the anchor base of a deletion / insertion, the REF allele's interval of a replacement), kind VLR_INDELPILEUP_DELETION / _INSERTION /
 *   _REPLACEMENT (informational), and the alt allele window of locus k at alt_bases[alt_offset[k] .. alt_offset[k + 1]): it does
 *   not depend on the read and is computed by the caller (varlociraptor_amd/readwindows.py: indel_locus).
 * fasta_path: the reference (its .fai is required).  The contigs the loci lie on are read when a BAM file names them, upper-cased and
 *   uploaded; a locus on a contig the FASTA lacks, or with a ref_id the BAM header does not have, is VLR_ERR_INVALID_ARGUMENT from
 *   vlr_indelpileup_add_bam.  A record on a contig without loci, or with a reference id out of range, gives no hits.
 * window: --realignment-window, 1 .. VLR_INDELPILEUP_MAX_WINDOW (a read window must fit the 128 bases of the kernels); the ref window
 *   is window * 3 / 2 on either side of the breakpoint, clamped to the contig.
 * mode: VLR_INDELPILEUP_EXACT (vlr_realign_batch's kernel), _FAST (vlr_realign_fast_batch's; the band is not computed and stays -1)
 *   or _HOMOPOLYMER (vlr_realign_homopolymer_batch's; hop[16] as there, NULL otherwise).  gap[4] as in vlr_realign_batch_desc.
 * hit_capacity, window_bytes: as for vlr_basepileup_open; nothing is written past the hit buffer, VLR_INDELPILEUP_OVERFLOW comes with
 *   the exact needed_capacity, and the hits do not depend on window_bytes, bit for bit: a hit's place is a function of the record
 *   order alone.
 * keep_pairs != 0: the pair arrays are copied to the host as they are scored (for tests, and for callers that score them again in
 *   another mode); vlr_indelpileup_read_pairs hands them out in hit order.
 * A hit: ln_ref / ln_alt are the raw outputs of the pair-HMM kernel for the two pairs (the normalisation of mod.rs:359-385 is the
 *   caller's: varlociraptor_amd/realign.py normalize_support), dist_ref / dist_alt the edit distances (-1: no hit), [ref_begin,
 *   ref_begin + ref_len) the ref allele window on the contig, [read_begin, read_begin + read_len) the read window.  status
 *   VLR_INDELPILEUP_HIT_NO_OVERLAP: the candidate region does not overlap the read (mod.rs:186-199: supports ln 0.5 / ln 0.5);
 *   VLR_INDELPILEUP_HIT_LEADING_REFSKIP: read_pos fails on a CIGAR that begins with N.  Both come with empty windows, two empty pairs,
 *   ln -inf and distance -1.  An evidence whose read window is empty is not reported.
 * vlr_indelpileup_result: the counts, the status word (VLR_INDELPILEUP_BAD_RECORD as VLR_BASEPILEUP_BAD_RECORD: the record gives no hits
 *   and is never followed, the records in front of it are scored), x_bytes / y_bytes: the bytes of the pair arrays, seconds: [0] file
 *   read, [1] upload + inflate, [2] record split, [3] count + scan kernels, [4] fill + gather kernels, [5] edit-distance + band kernels,
 *   [6] the pair-HMM kernels alone, [7] collect kernel and the copy of kept pairs, [8] hits to the host and the locus-major order,
 *   [9] total of vlr_indelpileup_add_bam, [10] inflate kernels alone.
 * vlr_indelpileup_read copies the n_hits hits: locus-major, in record order within a locus; `record` counts the records of all files
 *   given to the session so far.  vlr_indelpileup_read_pairs (keep_pairs sessions): x_offset / y_offset [n_pairs + 1], x_bases
 *   [x_bytes], y_bases / y_quals [y_bytes], band [n_pairs], n_pairs = 2 * n_hits, in hit order.
 * NOT part of this path (Realigner::allele_support has them): the read-inferred third allele, alt_variants, merged multi-locus
 *   regions, homopolymer_indel_len, SI:Z strand information over an interval, mate merging with the insert-size term. */
#define VLR_INDELPILEUP_MAX_WINDOW 64
enum { VLR_INDELPILEUP_DELETION = 0, VLR_INDELPILEUP_INSERTION = 1, VLR_INDELPILEUP_REPLACEMENT = 2 };
enum { VLR_INDELPILEUP_EXACT = 0, VLR_INDELPILEUP_FAST = 1, VLR_INDELPILEUP_HOMOPOLYMER = 2 };
/* status word of a session */
#define VLR_INDELPILEUP_BAD_RECORD (1u << 0)
#define VLR_INDELPILEUP_OVERFLOW   (1u << 1)
#define VLR_INDELPILEUP_GUARD_DAMAGED (1u << 2)  /* the guard words behind the hit buffer changed: a defect, never expected */
/* status byte of a hit */
#define VLR_INDELPILEUP_HIT_NO_OVERLAP      (1u << 0)
#define VLR_INDELPILEUP_HIT_LEADING_REFSKIP (1u << 1)
#define VLR_INDELPILEUP_HIT_STRAND_INFO     (1u << 2)  /* vlr_fragpileup_open_realign only: the record carries an SI:Z tag (not scored) */
typedef struct {
    double   ln_ref, ln_alt;       /* ln P(read window | ref allele), ln P(read window | alt allele): raw kernel outputs               */
    uint64_t record;               /* ordinal of the record                                                                            */
    int64_t  ref_begin;            /* start of the ref allele window on the contig                                                     */
    uint32_t locus;                /* index of the locus in the arrays given at open                                                   */
    uint32_t ref_len;              /* bases of the ref allele window                                                                   */
    uint32_t read_begin, read_len; /* the read window                                                                                  */
    int32_t  dist_ref, dist_alt;   /* edit distance of the read window against the ref / alt allele window; -1 = no hit                */
    uint16_t flag;                 /* the record's FLAG & (0x1 paired | 0x10 reverse | 0x40 first in template)                         */
    uint8_t  mapq;
    uint8_t  status;               /* VLR_INDELPILEUP_HIT_*                                                                            */
    uint8_t  pad[4];
} vlr_indelpileup_hit;
typedef struct vlr_indelpileup vlr_indelpileup;
typedef struct {
    int64_t  n_hits, n_records, n_rejected, n_pairs;
    int64_t  x_bytes, y_bytes;     /* bytes of the pair arrays (allele windows; read windows)                                          */
    uint64_t status;               /* VLR_INDELPILEUP_BAD_RECORD | VLR_INDELPILEUP_OVERFLOW | VLR_INDELPILEUP_GUARD_DAMAGED            */
    int64_t  needed_capacity;      /* hits the input produces (== n_hits unless VLR_INDELPILEUP_OVERFLOW)                              */
    int64_t  first_bad_record;     /* ordinal of the first bad record, -1 = none                                                       */
    double   seconds[12];
} vlr_indelpileup_counts;
int  vlr_indelpileup_open(int device, const char* fasta_path, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int64_t* end,
                          const uint8_t* kind, const uint64_t* alt_offset, const uint8_t* alt_bases, int window, int mode, const double gap[4],
                          const double* hop, int keep_pairs, int64_t hit_capacity, int64_t window_bytes, vlr_indelpileup** out);
int  vlr_indelpileup_add_bam(vlr_indelpileup* s, const char* bam_path);
int  vlr_indelpileup_result(vlr_indelpileup* s, vlr_indelpileup_counts* out);
int  vlr_indelpileup_read(vlr_indelpileup* s, vlr_indelpileup_hit* hits, int64_t n);
int  vlr_indelpileup_read_pairs(vlr_indelpileup* s, uint32_t* x_offset, uint8_t* x_bases, int64_t x_bytes, uint32_t* y_offset, uint8_t* y_bases,
                                uint8_t* y_quals, int64_t y_bytes, int32_t* band, int64_t n_pairs);
void vlr_indelpileup_close(vlr_indelpileup* s);

/* ------------------------------------------------------------------------------------------------
 * Fragment observations of SNV / MNV candidates from BAM records: Variant::extract_observations (variants/types/mod.rs:283-407) with
 * Snv / Mnv::is_valid_evidence and allele_support, Evidence::read_orientation / softclipped / len / is_paired, min_mapq and
 * major_read_position (read_observation.rs), restated in varlociraptor_amd/fragments.py.  Two stages:
 *   member pass (vlr_fragpileup_add_bam, per chunk of the device reader): one thread per record; a valid record (the flag rule of
 *     vlr_basepileup_*) whose START lies in [start - window, end) of a locus on its contig is a member of that locus — the test is on
 *     the start position alone, as rust-htslib's RecordBuffer::fetch keeps records.  A member carries the record's features (FLAG, MAPQ,
 *     l_seq, soft-clip test, orientation from RO:Z or the flags, whether it has an XA:Z tag) and, where the record encloses the locus,
 *     its allele support (the scoring of vlr_basepileup_*).  Members and the QNAMEs of records with members accumulate on the device
 *     at places that are prefix sums over the record order.
 *   fragment pass (vlr_fragpileup_result): the members are brought locus-major; one workgroup per locus sorts its members in LDS by
 *     (QNAME bytes, record ordinal), takes per run of equal names the first record as `left` and the last one that the
 *     first-and-last-in-template condition (mod.rs:329-334) does not skip as `right`, drops pairs with a MAPQ of 0 and fragments of
 *     which no record encloses the locus, merges the supports (AlleleSupport::merge), drops a merged strand of None, and writes the
 *     observations in name order; the mode of the read positions of alt-supporting observations (calc_major_feature) sets
 *     VLR_FRAGPILEUP_READPOS_MAJOR.  A locus with more than VLR_FRAGPILEUP_MAX_MEMBERS members comes back with
 *     VLR_FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS and no observations: the caller finishes it.
 *   The XA:Z entries of a member record (ExactAltLoci::from, read_observation.rs:167-210) go into a key pool as (64-bit FNV-1a of the
 *     contig bytes, position bucketed to 10 x max_read_len: locus_to_bucket) — two contig names that collide in 64 bits would be merged —;
 *     the fragment pass takes the mode of the keys of all observations of a locus (major_alt_locus) and writes each observation's
 *     alt_locus class (ReadObservation::process).  A locus whose observations carry more than VLR_FRAGPILEUP_MAX_MEMBERS keys comes
 *     back with VLR_FRAGPILEUP_LOCUS_TOO_MANY_ALT_LOCI and no observations.
 * Left to the caller (two libm calls per observation and a sequential ln_sum_exp): prob_hit_base = -ln(len_sum) and the MAPQ
 *   adjustment, from len_sum and min_mapq (fragments.py).
 * Loci, realign_indel_reads, window_bytes: as for vlr_basepileup_open.  window: bases in front of a locus' start in which a member may
 *   start (>= 0).  max_mapq: the alignment properties' value (is_max_mapq).  max_read_len <= 0 is an invalid argument.
 * member_capacity / name_capacity / key_capacity: members, QNAME bytes and alt-locus keys the session's device buffers hold.  More than
 *   that: nothing is written past a buffer, the status word carries VLR_FRAGPILEUP_MEMBER_OVERFLOW / _NAME_OVERFLOW / _KEY_OVERFLOW and
 *   needed_members / needed_name_bytes / needed_keys the exact need — open again with them.  Guard words sit behind every buffer (VLR_FRAGPILEUP_GUARD_DAMAGED is never expected).
 * vlr_fragpileup_result: seconds [0] file read, [1] upload + inflate, [2] record split, [3] member pass kernels, [4] fragment pass
 *   kernels, [5] total of add_bam, [6] inflate kernels alone, [7] observations to the host.
 * vlr_fragpileup_read: n_obs observations locus-major (name order within a locus) and n_loci locus records.  Bit-identical from run to
 *   run, for every window_bytes and for every split of the input into files.
 *
 * Realignment of indel-bearing reads (vlr_fragpileup_open_realign; snv.rs:72-86, mnv.rs:83, Realigner::allele_support, realignment/
 *   mod.rs:161-424): a session opened through this entry does not hand a record that encloses a locus and carries an I or D operation
 *   back flagged, it realigns it in the same pass over the file.  The arguments of vlr_fragpileup_open (realign_indel_reads = 0 scores every read from its alignment, as there)
 *   and fasta_path / realign_window (--indel-window, 1 .. VLR_INDELPILEUP_MAX_WINDOW) / mode / gap / hop as for vlr_indelpileup_open,
 *   evidence_capacity (realigned evidences the device buffers hold; the pair bytes are sized from it) and pair_byte_limit (pair bytes
 *   scored in one launch, 0 = 2^31: the uint32 offsets of vlr_realign_batch_desc; a smaller value only cuts the evidences into more
 *   ranges).  Per chunk the member pass counts the record's evidences and their pair bytes beside its members (a fourth prefix sum
 *   over the record order decides an evidence's place: no atomic), writes each as a vlr_indelpileup_hit — the candidate region
 *   (mod.rs:58-153) on [start, start + len), the ref allele window = the region's ref interval —, and one wave per evidence gathers
 *   the read window, the ref allele window from the upper-cased contig and the alt allele window of Snv / MnvEmissionParams
 *   ([max(0, start - rw), min(start + len + rw, contig length)), rw = realign_window * 3 / 2, the locus bytes replaced by the ALT
 *   allele) into pair arrays that accumulate over the session.  vlr_fragpileup_result scores them once per range (edit distance,
 *   band = distance + 4 except in fast mode, the pair HMM of `mode`: the kernels of vlr_realign_batch), brings the raw scores to the
 *   host, normalises them (mod.rs:358-376; std::log1p / std::exp), and a small kernel writes them into the members: strand = the
 *   record's when the supports differ, else none (mod.rs:409-413), no read position, no third-allele evidence.  The fragment pass
 *   behind it is the one of every session.  An evidence without overlap or with an empty read window gets ln 0.5 / ln 0.5.
 *   Refused, as a status of the observation: a CIGAR that begins with N (VLR_BASEPILEUP_HIT_LEADING_REFSKIP) and a record with an
 *   SI:Z tag (VLR_FRAGPILEUP_OBS_REALIGN_STRAND_INFO).  NOT mirrored: the read-inferred third allele (mod.rs:317-348),
 *   homopolymer_indel_len; the other alleles of a locus (alt_variants) only with vlr_fragpileup_set_alt_variants (below).  More evidences than evidence_capacity: VLR_FRAGPILEUP_EVIDENCE_OVERFLOW, nothing is written past a buffer,
 *   vlr_fragpileup_realign_result gives the exact need.  The observations do not depend on window_bytes, the split into files or
 *   pair_byte_limit, bit for bit.
 * vlr_fragpileup_realign_result (after vlr_fragpileup_result): the evidence counts; seconds [0] window gather kernels, [1]
 *   edit-distance + band kernels, [2] pair-HMM kernels, [3] collect, normalisation on the host and the kernel that writes the members.
 * vlr_fragpileup_read_realigned: the n_evidences realigned evidences in record order (loci ascending within a record) as
 *   vlr_indelpileup_hit: raw scores, distances, window coordinates, status. */
#define VLR_FRAGPILEUP_MAX_MEMBERS 4096   /* LDS per workgroup: 4 B sort index + 2 B rank per member + scan cells = 26 KiB, six workgroups per CU */
/* status word of a session */
#define VLR_FRAGPILEUP_BAD_RECORD      (1u << 0)
#define VLR_FRAGPILEUP_MEMBER_OVERFLOW (1u << 1)
#define VLR_FRAGPILEUP_NAME_OVERFLOW   (1u << 2)
#define VLR_FRAGPILEUP_GUARD_DAMAGED   (1u << 3)
#define VLR_FRAGPILEUP_KEY_OVERFLOW    (1u << 4)
#define VLR_FRAGPILEUP_EVIDENCE_OVERFLOW (1u << 5)
/* status of a locus */
#define VLR_FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS  (1u << 0)
#define VLR_FRAGPILEUP_LOCUS_TOO_MANY_ALT_LOCI (1u << 1)
/* status byte of an observation: the VLR_BASEPILEUP_HIT_* bits of its records' hits, and */
#define VLR_FRAGPILEUP_OBS_INVALID_RO  (1u << 4)   /* an RO:Z value that names no orientation (Error::InvalidReadOrientationInfo) */
#define VLR_FRAGPILEUP_OBS_REALIGN_STRAND_INFO (1u << 5)   /* a record that needs realignment carries an SI:Z tag: not scored */
/* bits of an observation */
#define VLR_FRAGPILEUP_SOFTCLIPPED    (1u << 0)
#define VLR_FRAGPILEUP_PAIRED         (1u << 1)
#define VLR_FRAGPILEUP_MAX_MAPQ       (1u << 2)
#define VLR_FRAGPILEUP_READPOS_MAJOR  (1u << 3)
#define VLR_FRAGPILEUP_HAS_XA         (1u << 4)
/* orientation: F1R2 = 0, F2R1 = 1 and None = 8 as the observation format writes them; the order of the other six is this ABI's own */
enum { VLR_FRAG_F1R2 = 0, VLR_FRAG_F2R1 = 1, VLR_FRAG_R1F2 = 2, VLR_FRAG_R2F1 = 3, VLR_FRAG_F1F2 = 4, VLR_FRAG_R1R2 = 5, VLR_FRAG_F2F1 = 6,
       VLR_FRAG_R2R1 = 7, VLR_FRAG_ORIENT_NONE = 8 };
#define VLR_FRAGPILEUP_NO_RECORD 0xffffffffffffffffull
typedef struct {
    double   prob_ref, prob_alt;   /* merged supports                                                                                  */
    uint64_t left, right;          /* record ordinals; right = VLR_FRAGPILEUP_NO_RECORD for a single read                              */
    uint32_t read_position;        /* VLR_BASEPILEUP_NO_READ_POSITION = none                                                           */
    uint32_t third_allele;         /* summed third-allele evidence, 0 = none                                                           */
    uint32_t len_sum;              /* l_seq(left) + l_seq(right)                                                                       */
    uint8_t  min_mapq;
    uint8_t  orientation;          /* VLR_FRAG_*                                                                                       */
    uint8_t  strand;               /* VLR_STRAND_*                                                                                     */
    uint8_t  bits;                 /* VLR_FRAGPILEUP_SOFTCLIPPED ... _HAS_XA                                                           */
    uint8_t  status;
    uint8_t  alt_locus;            /* VLR_ALTLOCUS_*                                                                                   */
    uint8_t  pad[6];
} vlr_fragpileup_obs;
typedef struct {
    int64_t  obs_offset;           /* first observation of the locus                                                                   */
    uint32_t n_members, n_obs;
    uint32_t major_read_position;  /* VLR_BASEPILEUP_NO_READ_POSITION = none                                                           */
    uint32_t status;               /* VLR_FRAGPILEUP_LOCUS_*                                                                           */
} vlr_fragpileup_locus;
typedef struct vlr_fragpileup vlr_fragpileup;
typedef struct {
    int64_t  n_obs, n_members, n_records, n_rejected, n_loci_too_deep;
    uint64_t status;
    int64_t  needed_members, needed_name_bytes, needed_keys;
    int64_t  first_bad_record;     /* -1 = none */
    double   seconds[8];
} vlr_fragpileup_counts;
int  vlr_fragpileup_open(int device, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int32_t* len, const uint8_t* kind,
                         const uint8_t* ref_bases, const uint8_t* alt_bases, int realign_indel_reads, int64_t window, int max_mapq, int max_read_len,
                         int64_t member_capacity, int64_t name_capacity, int64_t key_capacity, int64_t window_bytes, vlr_fragpileup** out);
int  vlr_fragpileup_add_bam(vlr_fragpileup* s, const char* bam_path);
int  vlr_fragpileup_result(vlr_fragpileup* s, vlr_fragpileup_counts* out);
int  vlr_fragpileup_read(vlr_fragpileup* s, vlr_fragpileup_obs* obs, int64_t n_obs, vlr_fragpileup_locus* loci, int64_t n_loci);
void vlr_fragpileup_close(vlr_fragpileup* s);
typedef struct {
    int64_t  n_evidences;          /* realigned evidences (0 on VLR_FRAGPILEUP_EVIDENCE_OVERFLOW)                                      */
    int64_t  needed_evidences;     /* evidences the input produces                                                                     */
    int64_t  x_bytes, y_bytes;     /* bytes of the pair arrays                                                                         */
    int64_t  n_ranges;             /* ranges the evidences were scored in                                                              */
    double   seconds[4];
} vlr_fragpileup_realign_counts;
int  vlr_fragpileup_open_realign(int device, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int32_t* len, const uint8_t* kind,
                                 const uint8_t* ref_bases, const uint8_t* alt_bases, int realign_indel_reads, int64_t window, int max_mapq,
                                 int max_read_len, int64_t member_capacity, int64_t name_capacity, int64_t key_capacity, int64_t window_bytes, const char* fasta_path,
                                 int realign_window, int mode, const double gap[4], const double* hop, int64_t evidence_capacity,
                                 int64_t pair_byte_limit, vlr_fragpileup** out);
int  vlr_fragpileup_realign_result(vlr_fragpileup* s, vlr_fragpileup_realign_counts* out);
int  vlr_fragpileup_read_realigned(vlr_fragpileup* s, vlr_indelpileup_hit* hits, int64_t n);
/* Deletion and insertion candidates in the fragment session (deletion.rs:41-85, 158-197, insertion.rs:57-61, 139-157, insert_size.rs:
 *   17-45; the rule is stated once, at the head of csrc/vlr_fragpileup.h).  vlr_fragpileup_open_indel takes the arguments of
 *   vlr_fragpileup_open_realign with the loci given as for vlr_indelpileup_open — [start, end) of a deletion (the anchor base and the
 *   deleted bases but the last) or [start, start + 1) of an insertion, kind VLR_INDELPILEUP_DELETION / _INSERTION, the alt allele
 *   window of locus k = alt_bases[alt_offset[k] .. alt_offset[k + 1]) — and has_insert_size (do the alignment properties carry an
 *   insert size?).  A locus longer than VLR_FRAGPILEUP_MAX_INDEL_LEN, an alt window longer than that plus twice the ref window, or
 *   any other kind is refused at open (VLR_ERR_INVALID_ARGUMENT, the locus named).  The caller gives only deletions whose three fetch
 *   loci (start, centerpoint, end - 1) merge into one fetch, so that membership is the window test of every session on [start, end).
 *   Every member of a locus is realigned (the evidences, their places, the gather, the scoring and the write into the members are those
 *   of vlr_fragpileup_open_realign, with the locus's own alt window); the session also keeps, in arrays only it allocates, a 32-byte side
 *   record per member (pos, end_pos, the four clip lengths) and per locus the maxima of its members' longest D, longest I and largest
 *   soft clip / l_seq (integer maxima, a total order: order-independent).  The fragment pass forms one observation per fragment
 *   with the validity rule of the kind and writes beside it a vlr_fragpileup_indel_obs.  The insert-size support, prob_sample_alt
 *   and the running maxima of the alignment properties need libm and stay with the caller (varlociraptor_amd/fragments.py).
 *   vlr_fragpileup_read, vlr_fragpileup_realign_result and vlr_fragpileup_read_realigned work on such a session as on a realigning one.
 *   NOT mirrored: the read-inferred third allele, homopolymer_indel_len and the prob_observable_at_homopolymer_*
 *   fields, max_depth subsampling, report_fragment_ids, replacements, SVs, breakends, deletions with more than one fetch.
 * vlr_fragpileup_read_indel (after vlr_fragpileup_result): n_obs side records parallel to the observations of vlr_fragpileup_read and
 *   n_loci records of maxima. */
#define VLR_FRAGPILEUP_MAX_INDEL_LEN 4096
#define VLR_FRAGPILEUP_INDEL_NONPOSITIVE_ISIZE (1u << 0)   /* insert size <= 0: the assertion of insert_size.rs:38-42 */
typedef struct {
    int64_t  insert_size;          /* of a deletion pair in a session with an insert size; 0 = none                                    */
    uint32_t len_left, len_right;  /* l_seq of the two records (len_right = 0 for a single read)                                       */
    uint32_t flags;                /* VLR_FRAGPILEUP_INDEL_*                                                                           */
    uint32_t pad;
} vlr_fragpileup_indel_obs;
typedef struct {
    uint32_t max_del, max_ins;     /* longest D / I operation of the locus's members (0 = none)                                        */
    uint32_t max_clip, max_clip_l_seq;  /* the largest soft clip / l_seq of the members, as the pair; l_seq = 0: no soft clip          */
} vlr_fragpileup_indel_locus;
int  vlr_fragpileup_open_indel(int device, int64_t n_loci, const int32_t* ref_id, const int64_t* start, const int64_t* end, const uint8_t* kind,
                               const uint64_t* alt_offset, const uint8_t* alt_bases, int64_t window, int max_mapq, int max_read_len,
                               int64_t member_capacity, int64_t name_capacity, int64_t key_capacity, int64_t window_bytes, const char* fasta_path,
                               int realign_window, int mode, const double gap[4], const double* hop, int64_t evidence_capacity,
                               int64_t pair_byte_limit, int has_insert_size, vlr_fragpileup** out);
int  vlr_fragpileup_read_indel(vlr_fragpileup* s, vlr_fragpileup_indel_obs* extra_obs, int64_t n_obs, vlr_fragpileup_indel_locus* extra_loci, int64_t n_loci);
/* The other alleles of a locus (`alt_variants`: utils/variant_buffer.rs:203-222, realignment/mod.rs:250-292, prob_allele 426-479; the rule
 *   is stated once, at the head of csrc/vlr_altvariants.h).  vlr_fragpileup_set_alt_variants gives a session of vlr_fragpileup_open_realign
 *   or vlr_fragpileup_open_indel, once and before its first vlr_fragpileup_add_bam, the competitors of its loci: those of locus l are
 *   comp_offset[l] .. comp_offset[l + 1], at most VLR_FRAGPILEUP_MAX_ALT_VARIANTS each, the alt allele window of competitor c is
 *   comp_bases[comp_base_offset[c] .. comp_base_offset[c + 1]) (upper case, as the caller builds the alt window of that candidate).
 *   Refused with VLR_ERR_INVALID_ARGUMENT and a message that names the locus or competitor: a plain or methylation session, a second call,
 *   a call after a BAM was added, more than VLR_FRAGPILEUP_MAX_ALT_VARIANTS competitors at a locus, descending offsets, an empty window or
 *   one longer than the alt-window limit of the session (VLR_FRAGPILEUP_MAX_INDEL_LEN plus twice the ref window, int(1.5 * realign_window):
 *   the limit of vlr_fragpileup_open_indel, in either session, since an indel may compete with an MNV).  A refusal launches nothing and
 *   leaves the session as it was.
 *   Such a session scores an evidence in 2 + K pairs — (ref, read), (alt, read), (competitor i, read) — through the edit-distance
 *   kernel, selects per evidence the reference-side alleles at the minimum distance, compacts those pairs and the alt pair, runs the pair
 *   HMM of the session's mode over the compacted pairs alone and takes as ln_ref the largest score (the lowest index on equal scores),
 *   as dist_ref the minimum distance.  In a session of vlr_fragpileup_open_realign an MNV locus with a competitor realigns every
 *   enclosing record, with or without an I / D operation (mnv.rs:83); an SNV locus does not (snv.rs:76).  A session that never calls
 *   vlr_fragpileup_set_alt_variants launches the kernels it always launched.
 * vlr_fragpileup_alt_result (after vlr_fragpileup_result): how many pairs went through the edit-distance kernel and the pair HMM.
 * vlr_fragpileup_read_alt_variants: one record per evidence, parallel to vlr_fragpileup_read_realigned. */
#define VLR_FRAGPILEUP_MAX_ALT_VARIANTS 15
typedef struct {
    uint8_t  winner;               /* the reference-side allele that gave ln_ref: 0 = the reference, i = competitor i (1-based)         */
    uint8_t  n_tied;               /* reference-side alleles at the minimum edit distance (0: none had a hit)                          */
    uint8_t  n_ref_side_hits;      /* reference-side alleles with a hit                                                                */
    uint8_t  pad[5];
} vlr_fragpileup_alt_hit;
typedef struct {
    int64_t  n_edit_pairs;         /* pairs that went through the edit-distance kernel: the sum of 2 + K over the evidences            */
    int64_t  n_hmm_pairs;          /* pairs that went through the pair HMM: per evidence the tied set and the alt pair                 */
    int64_t  n_competitors;        /* competitors of the table                                                                         */
    int64_t  n_loci_with_competitors;
} vlr_fragpileup_alt_counts;
int  vlr_fragpileup_set_alt_variants(vlr_fragpileup* s, const uint64_t* comp_offset, const uint64_t* comp_base_offset, const uint8_t* comp_bases);
int  vlr_fragpileup_alt_result(vlr_fragpileup* s, vlr_fragpileup_alt_counts* out);
int  vlr_fragpileup_read_alt_variants(vlr_fragpileup* s, vlr_fragpileup_alt_hit* out, int64_t n_evidences);
/* Methylation candidates (ALT <METH>) in the fragment session (variants/types/methylation.rs; the rule is stated once, at the head of
 *   csrc/vlr_methylation.h).  vlr_fragpileup_open_methylation takes the arguments of vlr_fragpileup_open with the loci as (ref_id, start)
 *   only — the locus is [start, start + 1), the C of a CpG — and readtype: VLR_METH_CONVERTED (bisulfite / EM-seq reads: C / T forward,
 *   G / A reverse, scored with the tables of the SNV arm) or VLR_METH_ANNOTATED (reads with MM / ML tags: the 5mC map of the record, scored
 *   with vlr_methylation_tables).  A record of reverse orientation (unpaired: the reverse flag; paired: (reverse && first) || (!reverse &&
 *   !first)) is read at start + 1 and encloses the locus when pos <= start + 1 && end_pos >= start + 1; only records whose FLAG is one of
 *   0, 16, 83, 99, 147, 163 give support.  The read position of an observation is the position in SEQ, without a leading hard clip;
 *   third_allele is 0.  vlr_fragpileup_add_bam, _result, _read and _close work on such a session as on any other; the overflow statuses and
 *   the guard words are those of every session.  A record of any length is one thread's work (csrc/vlr_methylation.h says what it costs).
 *   NOT mirrored: max_depth subsampling, report_fragment_ids.
 * vlr_methylation_tables: ln((ml + 0.5) / 256) and ln(1 - exp of it) for ml = 0 .. 255, as the session scores with them. */
enum { VLR_METH_CONVERTED = 0, VLR_METH_ANNOTATED = 1 };
int  vlr_fragpileup_open_methylation(int device, int64_t n_loci, const int32_t* ref_id, const int64_t* start, int readtype, int64_t window, int max_mapq,
                                     int max_read_len, int64_t member_capacity, int64_t name_capacity, int64_t key_capacity, int64_t window_bytes,
                                     vlr_fragpileup** out);
int  vlr_methylation_tables(double ln_meth[256], double ln_unmeth[256]);

/* The whole of `varlociraptor filter-calls control-fdr` (/root/reference/src/filtration/fdr.rs:36-158, record typing
 * src/utils/collect_variants.rs:44-304, probability sums and the filtering pass src/utils/mod.rs:169-374): read the calls BCF
 * `in_path`, collect the posterior of `events` (names as on the command line: PROB_<UPPER CASE> INFO tags; tags the header does
 * not declare are dropped, none left = error "invalid FDR control events") per typed variant, find the threshold on `device`
 * (vlr_fdr_threshold), and write the kept records, byte for byte as they came, with the input's header to the BCF `out_path`.
 * mode: VLR_FDR_MODE_* (global = 0; LOCAL: threshold ln(1 - alpha); SMART: PROB_ABSENT [+ PROB_ARTIFACT] based, fdr.rs:96-114).
 * vartype: NULL = all variants, else "SNV" "MNV" "INS" "DEL" "BND" "INV" "DUP" "REP"; minlen / maxlen: -1 = open (length range
 * [minlen, maxlen) as Variant::is_type).  Records of one breakend EVENT share one decision.  n_kept / n_total may be NULL. */
enum { VLR_FDR_MODE_LOCAL = 1, VLR_FDR_MODE_SMART = 2, VLR_FDR_MODE_RETAIN_ARTIFACTS = 4 };
int vlr_calls_filter_fdr(const char* in_path, const char* out_path, int n_events, const char* const* events, double alpha, uint32_t mode,
                         const char* vartype, int64_t minlen, int64_t maxlen, int device, int n_threads, int64_t* n_kept, int64_t* n_total);

/* ------------------------------------------------------------------------------------------------
 * Posterior odds (filtration/posterior_odds.rs:62-79): one decision per allele.  ln_target[i]: ln-sum over the PROB_* tags of
 * the chosen events, ln_other[i]: ln-sum over every other PROB_* INFO tag of the header (both as utils::tags_prob_sum(.., None),
 * utils/mod.rs:177-212); valid[i]: bit 0 = ln_target is a value, bit 1 = ln_other is a value (a sum without values is the
 * reference's None; the double behind a cleared bit is not read for the decision).
 *   keep[i] = both valid && level(e^(ln_other[i] - ln_target[i])) < min_level,
 * level = bio's evidence_kass_raftery of the Bayes factor k: k <= 1 VLR_ODDS_NONE, <= 3 BARELY, <= 20 POSITIVE, <= 150 STRONG,
 * else VERY_STRONG (a NaN k, e.g. -inf against -inf, fails every comparison: VERY_STRONG).  ln_other == ln_target gives k = 1
 * exactly: NONE.  The device decides in log space on d = ln_other - ln_target: NONE for d < 2^-53 (exactly the d whose e^d a
 * correctly rounded exp returns as <= 1), then d <= ln 3, ln 20, ln 150; next to the reference's e^d <= b a decision can differ
 * only where d is within rounding of ln 3, ln 20 or ln 150.  n = 0 is legal.  Host pointers; uploads, launches on `device`,
 * copies back. */
enum { VLR_ODDS_NONE = 0, VLR_ODDS_BARELY = 1, VLR_ODDS_POSITIVE = 2, VLR_ODDS_STRONG = 3, VLR_ODDS_VERY_STRONG = 4 };
int vlr_posterior_odds_keep(int device, int64_t n, const double* ln_target, const double* ln_other, const uint8_t* valid, int min_level, uint8_t* keep);

/* ------------------------------------------------------------------------------------------------
 * ln_sum_exp per (range, group) cell: the reduction of `estimate mutational-burden` (estimation/mutational_burden.rs:186-190,
 * 214-346, where it is a BTreeMap range query, a hash grouping and a ln_sum_exp per minimum VAF).  n entries (vaf, ln_prob,
 * group in [0, n_groups)); n_ranges half-open ranges [lo[r], hi[r]) (hi = +inf: open).  An entry is in range r when
 * lo[r] <= vaf && vaf < hi[r] as f64 comparisons with the tabulated bounds — every range is tested on its own bounds (the
 * reference's ranges are no partition: neighbouring histogram edges are computed separately and may differ by an ulp).
 *   out[r * n_groups + g] = m + ln1p((c - 1) + S): m = maximum ln_prob of the cell, c = number of entries equal to m,
 *   S = sum of e^(ln_prob - m) over the entries below m (bio ln_sum_exp); -inf for a cell without
 *   entries or with only -inf entries.
 * Summation order of S (fixed: independent of the launch geometry, the scheduling and of how the entries were uploaded): the
 *   entries in chunks of VLR_LSE_CHUNK consecutive ones; within a chunk a cell's terms are added sequentially in entry order
 *   starting from 0.0; a cell's chunk sums are added sequentially in chunk order starting from 0.0.  m and c do not depend on
 *   any order.  No atomics: the same input gives the same bits.
 * n = 0 is legal (every cell -inf, no device is touched).  A NaN vaf is in no range (dropping it is the caller's business); a
 *   NaN ln_prob makes its cells NaN.  A group outside [0, n_groups), n_ranges outside [1, VLR_LSE_MAX_RANGES] or n_groups
 *   outside [1, VLR_LSE_MAX_GROUPS] = VLR_ERR_INVALID_ARGUMENT.  Host pointers; uploads, launches on `device`, copies back. */
#define VLR_LSE_CHUNK      4096
#define VLR_LSE_MAX_RANGES 128
#define VLR_LSE_MAX_GROUPS (14 * VLR_MAX_SAMPLES)
int vlr_range_group_lse(int device, int64_t n, const double* vaf, const double* ln_prob, const int32_t* group, int n_ranges, const double* lo,
                        const double* hi, int n_groups, double* out);

/* Diagnostics: device time in milliseconds (a hipEvent pair around the launches, copies excluded) of the kernels of this thread's
 * last vlr_range_group_lse (also inside vlr_calls_mutational_burden) and last vlr_posterior_odds_keep; either pointer may be NULL. */
int vlr_callstats_last_kernel_ms(double* range_group_lse_ms, double* posterior_odds_ms);

/* The whole of `varlociraptor filter-calls posterior-odds` (filtration/posterior_odds.rs:19-82): read the calls BCF `in_path`;
 * the header's PROB_* INFO descriptions must be PHRED scaled (utils::is_phred_scaled, utils/mod.rs:421-446: each ends with
 * "(PHRED)" or does not end with ")"), otherwise error "Event probabilities are not PHRED scaled" and no output file.  Target
 * tags: PROB_<UPPER CASE event> (utils::events_to_tags); other tags: the header's PROB_* INFO ids whose suffix equals none of
 * the event names AS GIVEN (posterior_odds.rs:39-52 — an event given in lower case is therefore summed on both sides, as in the
 * reference).  Per typed variant both ln-sums are formed here (record typing and tags_prob_sum as vlr_calls_filter_fdr's), the
 * decisions are made on `device` (vlr_posterior_odds_keep); a record is kept when any of its alleles is kept and is written byte
 * for byte with the input's header to the BCF `out_path`.  Deviation: the reference trims the removed alleles of a kept record
 * (Record::remove_alleles); this writes the record untrimmed — the same thing for the single-ALT records `call variants` writes.
 * min_level: VLR_ODDS_* (the --odds argument).  n_kept / n_total may be NULL. */
int vlr_calls_filter_odds(const char* in_path, const char* out_path, int n_events, const char* const* events, int min_level, int device, int n_threads,
                          int64_t* n_kept, int64_t* n_total);

/* The record pass and the reduction of `varlociraptor estimate mutational-burden` (estimation/mutational_burden.rs:93-190): read
 * the annotated calls BCF `in_path`; per record take FORMAT/AF of each of `samples` (a name the header lacks: error "Sample <name>
 * not found"); skip records that are not coding (is_valid_variant, :18-43: some ANN entry has |-field 7 == "protein_coding" and a
 * non-empty field 13; no ANN = not coding) or that lack one of the events' PROB_<UPPER CASE> tags (:141-156); the allele
 * probability is ln_add_exp over the events of the PHRED value as ln, starting from -inf; the signature is signatures()
 * (:482-515) with the 14 classes in declaration order DEL METH INS INV DUP BND MNV Complex C>A C>G C>T T>A T>C T>G (an SNV whose
 * bases are not ACGT is an error that names the record; the reference panics).  One entry per (sample, allele) whose AF is neither
 * NaN nor missing: (AF widened to f64, probability, group), in record order and within a record by sample name (byte order, as
 * the reference's BTreeMap of samples iterates), then allele.  group = index of the sample in `samples` * 14 + signature with by_sample != 0 (multibar mode: the key is (vartype, sample)), else the
 * signature alone (hist, curve and table modes: the reference keys on vartype only).  No entry at all: error "unable to estimate TMB
 * because no valid records were found in the given BCF/VCF" (errors.rs:32).  out_cells[r * G + g], G = by_sample ? n_samples * 14 : 14: vlr_range_group_lse of the entries over the given
 * ranges on `device` (the entries are uploaded in pieces, which does not change a bit); *n_entries may be NULL.  The per-megabase
 * scaling and the output are the caller's (varlociraptor_amd/burden.py). */
int vlr_calls_mutational_burden(const char* in_path, int n_events, const char* const* events, int n_samples, const char* const* samples, int by_sample,
                                int n_ranges, const double* lo, const double* hi, int device, int n_threads, double* out_cells, int64_t* n_entries);

/* Diagnostics: the DEVICE build of the platform-independent decision arithmetic (include/vlr_detmath.h; which = 0 det_exp,
 * 1 det_log1p_pos, 2 det_log2_ratio(a, b), 3 det_exp2) and of the kernel's mantissa logarithm (4), element-wise on host
 * arrays.  tests/test_gpu_math.py requires 0-3 to be bit-identical to the host build of the same header. */
int vlr_selftest_math(int device, int which, const double* a, const double* b, double* out, int64_t n);
/* Diagnostics: `reps` launches of a stream of known size in the engine's own access widths — mode 0 reads n f32 with
 * lane-contiguous 4-byte loads (4 n bytes per launch), mode 1 writes n f64 with lane-contiguous 8-byte stores (8 n bytes
 * per launch) — so that rocprofv3's FETCH_SIZE / WRITE_SIZE can be calibrated for them (tools/traffic_measure.sh). */
int vlr_selftest_stream(int device, int mode, int64_t n, int reps);
/* Diagnostics: vlr_fdr_threshold with its intermediate stages copied back (tests/test_gpu_fdr_stages.py).  Same inputs, same code
 * path (cap of values above ln 1, padding, staging, kernels, read-back, decision with the host fallback), same *threshold and
 * *status.  Host arrays, any of which may be NULL: sorted[n] = the keys after the descending sort; prob[n], pep_ln[n], cum[n] = the
 * probabilities after the optional `smart` conversion, ln PEP and the per-1024-block inclusive prefix sums of the linear PEPs as
 * the PEP kernel wrote them; block_offset[(n + 1023) / 1024] = the exclusive prefix sums of the block totals; best_raw[3] = the
 * result words as the device left them, before any host fallback: boundary index + 1 (0 = none), the bits of the expected FDR
 * of entry 0 (a double), the near-alpha flag.  n == 0: nothing but best_raw (zeros), *threshold and *status is written. */
int vlr_selftest_fdr_stages(int device, const double* ln_prob, int64_t n, int smart, double alpha_ln, double* sorted, double* prob, double* pep_ln,
                            double* cum, double* block_offset, int64_t* best_raw, double* threshold, int* status);

/* ---------------------------------------------------------------- native ingest / emission
 * The process boundary of `call variants` without htslib: observation files in (calling.rs:306-339 bcf::Reader,
 * preprocessing/mod.rs:818-919 read_observations, utils/mod.rs:449-474 MiniLogProb), calls file out
 * (calling/variants/mod.rs:178-600 Call::write_final_record).  BGZF blocks are inflated / deflated and records decoded /
 * encoded on n_threads host threads (<= 0: all hardware threads, at most 128). */
typedef struct vlr_obs_table vlr_obs_table;

/* Per-locus site data of a table (pointers owned by the table, valid until vlr_obs_table_free). */
typedef struct {
    int64_t n_loci;
    int32_t n_contigs;
    int32_t _pad;
    const char* const* contig_names;     /* [n_contigs]                                                              */
    const int32_t* contig;               /* [n_loci] index into contig_names                                         */
    const int64_t* pos;                  /* [n_loci] 1-based                                                         */
    const char* strings;                 /* NUL-terminated strings addressed by the offsets below                    */
    const uint64_t* id_offset;           /* [n_loci] record ID ("." if none)                                         */
    const uint64_t* ref_offset;          /* [n_loci] REF allele                                                      */
    const uint64_t* alt_offset;          /* [n_loci] ALT alleles, comma separated                                    */
    /* breakend groups (HaplotypeIdentifier, variants/model/mod.rs:87-133; calling.rs:569-580, 726-741): index of the first
     * locus with the same INFO EVENT / (ID, MATEID) pair — that locus is evaluated, the others copy its result        */
    const int64_t* group_representative; /* [n_loci] (= own index for ungrouped records)                             */
    /* variant-specific priors of the candidate record (calling.rs:470-494), natural log, NaN = absent               */
    const double* heterozygosity_ln;
    const double* somatic_effective_mutation_rate_ln;
    const int32_t* third_allele_evidence; /* [n_obs] output-only feature of the OBS string (mod.rs:283-287), -1 = None */
    const uint8_t* imprecise;            /* [n_loci] INFO IMPRECISE                                                  */
    /* (ABI 3) 64-bit hash of the group's identifier, 0 for ungrouped records: group_representative only looks inside one
     * table; a driver that streams a file in chunks (vlr_obs_reader_next) keeps key -> result of the first record and hands
     * it to the later breakends of the event, as the reference does across the whole file (calling.rs:569-580, 726-741) */
    const uint64_t* group_key;           /* [n_loci]                                                                 */
} vlr_obs_sites;

/* Read one observation file per sample (sample-index order; BCF2 in BGZF blocks, gzip or plain; text VCF accepted) into one
 * table: the SoA columns of vlr_batch in page-locked memory (vlr_host_alloc; plain memory when no device is present), pileup
 * p = locus * n_samples + sample.  locus_flags follow WorkItem.check_* (calling.rs:557-598) under the --omit-* mask.
 * Errors: missing format version 15 (calling.rs:324-339), records that differ between the files (calling.rs:369-390),
 * truncated vectors. */
int  vlr_obs_read(int n_samples, const char* const* paths, uint32_t omit_bias_mask, int n_threads, vlr_obs_table** out);
void vlr_obs_table_free(vlr_obs_table* table);
int  vlr_obs_table_batch(const vlr_obs_table* table, vlr_batch* out);   /* host pointers into the table, for vlr_batch_run_host */
int  vlr_obs_table_sites(const vlr_obs_table* table, vlr_obs_sites* out);
/* write_observations (preprocessing/mod.rs:921-1038) of sample `sample` of a HOST batch as an observation BCF; sites == NULL:
 * contig "1", positions 1.., alleles synthesised from variant_type / ref_base / alt_base.  third_allele_evidence may be NULL. */
int  vlr_obs_write(const char* path, const vlr_batch* in, int sample, const vlr_obs_sites* sites, const int32_t* third_allele_evidence, int n_threads);
/* The calls file for the loci of `table` from HOST results: path ending in ".bcf" -> BCF2 (BGZF), otherwise text VCF.
 * header_text: "##..." lines and the "#CHROM" line with the sample names; out_names[results->n_out]: the names behind the columns
 * of ln_posterior ("absent", the scenario events, "artifact") — INFO PROB_<NAME>, PHRED, f32, sorted by descending probability. */
int  vlr_calls_write(const char* path, const char* header_text, const vlr_obs_table* table, const vlr_results* results,
                     const char* const* out_names, int n_threads);
/* The same in pieces: a reader that delivers at most max_records records of every sample file per call (bounded memory; the
 * caller may overlap the read of the next chunk with the evaluation and emission of the previous one), and a writer that appends
 * one chunk per call.  vlr_obs_reader_next sets *out = NULL once the files are exhausted; every table is freed by the caller.
 * Breakend groups (vlr_obs_sites.group_representative) are formed within a chunk; group_key identifies an event across chunks. */
typedef struct vlr_obs_reader vlr_obs_reader;
int  vlr_obs_reader_open(int n_samples, const char* const* paths, uint32_t omit_bias_mask, int n_threads, vlr_obs_reader** out);
int  vlr_obs_reader_next(vlr_obs_reader* reader, int64_t max_records, vlr_obs_table** out);
void vlr_obs_reader_close(vlr_obs_reader* reader);
typedef struct vlr_calls_writer vlr_calls_writer;
int  vlr_calls_writer_open(const char* path, const char* header_text, vlr_calls_writer** out);
int  vlr_calls_writer_append(vlr_calls_writer* writer, const vlr_obs_table* table, const vlr_results* results, const char* const* out_names, int n_threads);
int  vlr_calls_writer_close(vlr_calls_writer* writer);   /* header (if nothing was appended), BGZF end-of-file member, close */
/* Several writers, one file (the shards of a sharded run, vlr_obs_reader_open_device_shard): every shard writes its records as a PART —
 * part 0 with the header, the others without (with_header = 0), none with the end-of-file member (with_eof = 0); BGZF members
 * concatenate, so vlr_calls_concat_parts(path, parts, n) copies the parts in shard order behind each other, appends the end-of-file
 * member and removes the part files.  BCF only. */
int  vlr_calls_writer_set_part(vlr_calls_writer* writer, int with_header, int with_eof);
int  vlr_calls_concat_parts(const char* path, const char* const* parts, int n_parts);
/* Measurement aid: wall seconds of the stages of the last vlr_obs_read ([0] file reads, [1] BGZF inflate, [2] parse + decode — summed
 * over the sample files, which run side by side — [3] all files, [4] merge into the table, [5] strings and groups, [6] total) and of
 * the last vlr_calls_write ([8] record encoding, [9] BGZF deflate + file write, [10] total). */
/* Diagnostics: the calls writer's own "%.<digits>f" (digits 0..3) of one value, for the tests to hold against printf. */
int  vlr_selftest_format_fixed(double v, int digits, char* out, int cap);
/* the device formatter of vlr_results.afd_text on host arrays (tests): n_lists lists of `capacity` slots; text / span as in vlr_results;
 * *n_unformatted = lists left to the arrays */
int  vlr_selftest_afd_text(int device, int64_t n_lists, int capacity, const int32_t* count, const double* vaf, const double* lnprob,
                           uint8_t* text, uint64_t text_capacity, uint32_t* span, uint32_t* n_unformatted);
void vlr_ingest_last_timings(double* out16);
/* The same indices summed over every vlr_obs_reader_next / vlr_calls_writer_append call since the last reset (reset != 0 clears
 * them after reading): what the streaming front door spends per stage over a whole file. */
void vlr_ingest_total_timings(double* out16, int reset);

/* ---- Device front door (ABI 4).  The same streaming reader with the BGZF inflate, the record split and the v15 decode as kernels
 * on `device` (csrc/vlr_inflate.hip, csrc/vlr_decode.hip): the compressed members cross PCIe, the inflated records and the SoA
 * columns are born in device memory.  Replaces the same reference rows as vlr_obs_reader_open (bcf::Reader over the observation
 * files, calling.rs:297-339; read_observations, preprocessing/mod.rs:818-919; MiniLogProb, utils/mod.rs:449-474).  BCF2 in BGZF
 * members only (the files `varlociraptor preprocess` writes); anything else: VLR_ERR_UNSUPPORTED, use vlr_obs_reader_open.
 * The tables of such a reader hold the batch twice: in device memory (vlr_obs_table_device_batch: the pointers vlr_batch_run takes,
 * valid until vlr_obs_table_free) and in page-locked host memory (vlr_obs_table_batch: what the calls writer formats DP / SAOBS /
 * SROBS / OBS from), both complete when vlr_obs_reader_next returns.  The CRC32 of every member is checked against its trailer on
 * the device (ABI 5; htslib does the same per block), like the host reader checks it on the CPU. */
int  vlr_obs_reader_open_device(int device, int n_samples, const char* const* paths, uint32_t omit_bias_mask, int n_threads, vlr_obs_reader** out);
/* Sharded device reader: N readers (the ranks of a torchrun job, the devices of a node) each inflate and decode about 1 / N of every
 * file instead of all of it.  The reference reads every record once (calling.rs:306-339, 357-367) and the loci shard across the GPUs
 * (north star): a shard is a contiguous range of records, every reader delivers the records of ITS range in file order.
 *   vlr_obs_reader_open_device_shard   inflates the members of the reader's byte share of every file (plus a lead-in and a tail of
 *                                      1/32 of the share, VLR_INGEST_SHARD_SLACK) and finds the record starts in them;
 *   vlr_obs_reader_shard_counts        out[n_samples][vlr_obs_reader_shard_row_size()]: what the other readers need to know (records that
 *                                      start in the share, where its first record starts and where the one behind its last record does);
 *   the caller gathers the rows of all shards (one small all-gather; plain memory inside one process) in shard order and calls
 *   vlr_obs_reader_shard_assign        on every reader: checks that consecutive shards meet in every file (a wrong guess of a record start
 *                                      shows here: VLR_ERR_INVALID_ARGUMENT, read unsharded), numbers the records, positions the files at
 *                                      the reader's range — the records of the FIRST file's share — and reports it (*first_record,
 *                                      *n_records; the ranges of all shards partition the file in shard order).
 * vlr_obs_reader_next then delivers that range like any reader.  Breakend groups and per-variant prior overrides that reach across
 * a shard boundary are the caller's business (the CLI refuses such files in sharded mode). */
int  vlr_obs_reader_open_device_shard(int device, int n_samples, const char* const* paths, uint32_t omit_bias_mask, int n_threads,
                                      int shard, int n_shards, vlr_obs_reader** out);
int  vlr_obs_reader_shard_row_size(void);
int  vlr_obs_reader_shard_counts(const vlr_obs_reader* reader, int64_t* out);
int  vlr_obs_reader_shard_assign(vlr_obs_reader* reader, const int64_t* all_rows, int64_t* first_record, int64_t* n_records);
/* The same for a node driven from one process (vlr_node_*): one sharded reader per device of the node, opened side by side, the
 * counts exchanged in memory; out[vlr_node_n_devices(node)].  Reader r delivers the records of shard r from device vlr_node_device(node, r):
 * its tables go to vlr_batch_run_device_in on vlr_node_plan(node, r), its calls to a part writer (vlr_calls_writer_set_part). */
int  vlr_node_obs_readers_open(vlr_gpu_node* node, int n_samples, const char* const* paths, uint32_t omit_bias_mask, int n_threads,
                               vlr_obs_reader** out);
int  vlr_obs_table_device_batch(const vlr_obs_table* table, vlr_batch* out);  /* VLR_ERR_INVALID_ARGUMENT for a table of a host reader */
/* keep == 0: the tables of this device reader do not bring the observation columns down to the host; instead a kernel (one wave per
 * pileup) derives what the calls writer formats from them — the OBS text itself (distinct observation keys counted, ordered and written
 * as in Call::write_final_record, calling/variants/mod.rs:233-360), the Kass-Raftery letters of SAOBS / SROBS, the prob_mapping runs
 * of DP — and only those summaries cross PCIe.  The observation arrays of vlr_obs_table_batch and
 * vlr_obs_sites.third_allele_evidence are then NOT filled until vlr_obs_table_fetch_columns copies them on demand (the writer does
 * that itself where it has to: pileups of more than 1 024 observations).  Default: keep.
 * vlr_obs_table_summaries: 1 when the calls writer will format this table from device summaries, 0 when from the columns;
 * *n_overflow (may be NULL) = pileups the kernel left to the columns. */
int  vlr_obs_reader_set_host_columns(vlr_obs_reader* reader, int keep);
int  vlr_obs_table_summaries(const vlr_obs_table* table, int64_t* n_overflow);
int  vlr_obs_table_fetch_columns(vlr_obs_table* table);
/* on != 0: vlr_obs_reader_next of this device reader returns while the copy of the observation columns to the host side of the
 * table is still in flight (the device side, what vlr_batch_run_device_in evaluates, is complete).  vlr_calls_writer_append and
 * vlr_obs_table_fetch_columns wait for it; a caller that reads the observation arrays of vlr_obs_table_batch itself calls
 * vlr_obs_table_fetch_columns first.  Default: off. */
int  vlr_obs_reader_set_async_columns(vlr_obs_reader* reader, int on);
/* The inflate stage alone, host buffers in and out (tests, tools): `bgzf` is a sequence of BGZF members (SAM spec 4.1), *out_bytes
 * receives the sum of their ISIZE fields (also when out_capacity is too small: VLR_ERR_INVALID_ARGUMENT then). */
int  vlr_bgzf_inflate(int device, const void* bgzf, int64_t n_bytes, void* out, int64_t out_capacity, int64_t* out_bytes);
/* Measurement aid of the device reader: seconds per stage summed since the last reset — [0] file read + member index, [1] H2D of the
 * compressed bytes, [2] inflate kernel, [3] record split, [4] INFO scan, [5] decode, [6] D2H of columns and cold records, [7] host
 * side (cold records, table), [8] total; [9] inflated bytes, [10] compressed bytes, [11] records, [12] chunks whose record split fell
 * back to the serial walk, [13] seconds of the inflate kernels alone (HIP events on their stream, summed over the files). */
void vlr_ingest_device_timings(double* out16, int reset);
/* Closed device readers leave their device buffers (inflate windows, member lists; hundreds of MB per file) parked for the next reader
 * of the process, bounded by VLR_INGEST_PARK_MB (default 2048).  A long-lived process calls this to hand all of it back to the device. */
void vlr_ingest_device_trim(void);

#ifdef __cplusplus
}
#endif
#endif /* VLR_H */
