/*
 * signalalign_hip.h -- C ABI of libsignalalign_hip.so: the MI355X-native replacement for
 * signalAlign's banded pair-HMM forward/backward/posterior path.
 *
 * Plain C: pointers and sizes only.  Every entry point names the reference interface it replaces
 * (paths relative to the upstream signalAlign tree).  The library never exits the process; it
 * returns 0 or a negative SA_E* code (sa_strerror()).  All device work is hand-written HIP for
 * gfx950; there is NO CPU fallback: without a usable GPU sa_batch_create()/sa_batch_run() fail with
 * SA_ENODEVICE.
 *
 * The seam is getAlignedPairsUsingAnchors()/getExpectationsUsingAnchors()
 * (inc/pairwiseAligner.h:406-429): a state machine, a k-mer sequence, an event sequence, a list of
 * anchor pairs and banding parameters go in; (floor(p*1e7), x, y, path k-mer) tuples come out.
 * Here the same call is batched over many reads so one launch fills the GPU.
 */
#ifndef SIGNALALIGN_HIP_H_
#define SIGNALALIGN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SA_OK 0
#define SA_EINVAL (-1)     /* bad argument                                        */
#define SA_ENOMEM (-2)     /* host or device allocation failed                    */
#define SA_ENODEVICE (-3)  /* no usable HIP device / HIP runtime error            */
#define SA_EALPHABET (-4)  /* reference k-mer has a character outside the alphabet
                              (the reference aborts in kmer_to_word, impl/nanopore_hdp.c:387-403) */
#define SA_EBAND (-5)      /* anchors produce an invalid diagonal (diagonal_construct throws,
                              impl/pairwiseAligner.c:98-103)                       */
#define SA_EIO (-6)        /* file could not be read / parsed                     */
#define SA_ESTATE (-7)     /* call out of order (e.g. results before run)         */
#define SA_EUNSUPPORTED (-8)

/* flags for sa_batch_create */
#define SA_FLAG_EXACT 1u          /* reference-ordered, un-contracted fp64 arithmetic on the device
                                     (slow kernels; bit-identical posteriors for Gaussian emissions) */
#define SA_FLAG_FORCE_GENERIC 2u  /* never pick the register-resident fast kernels */
#define SA_FLAG_RNA 4u            /* event alignment only: k-mers as build_kmer_list(..., rna=true) makes them (U -> T, reversed) */
#define SA_FLAG_DEVICE_TO_ITSELF 8u /* sa_batch_create_deferred only: every other batch on this device will have been destroyed
                                     before this one's first use -- its forward storage is sized for the memory they hold too
                                     (one batch at a time, the next one packed and planned while the current one runs).
                                     The promise is the caller's: if other batches still hold their storage at that first use
                                     (sa_batch_run / sa_batch_start, but also sa_batch_stats and sa_batch_job_cells, which
                                     complete the creation too), the working buffers may not fit and that call returns
                                     SA_ENOMEM; the batch can then only be destroyed */

#define SA_FLAG_VC_ROWS 32u        /* keep only the rows the variant-caller output prints (writePosteriorProbsVC, impl/signalMachine.c:161-232:
                                     pairs whose reference k-mer holds the ambiguity letter 'X'); every other pair is counted and
                                     summed on the device (sa_batch_all_pairs_summary: what the run's pair count and
                                     scoreByPosteriorProbabilityIgnoringGaps need) and never crosses PCIe.  signalMachine -s 1 sets it.
                                     Not for a batch that feeds sa_batch_mea (the path needs every pair: sa_batch_mea returns SA_ESTATE
                                     for such a batch) and not together with SA_FLAG_PAIRS8 (SA_EINVAL: an 8-byte record does not
                                     name the k-mer the filter looks at). */
#define SA_FLAG_PAIRS8 64u         /* the batch holds its pairs as 8-byte records (sa_pair8_t below) instead of 16-byte ones: half the
                                     bytes over PCIe for results of hundreds of millions of pairs (broad HDP densities at a low
                                     threshold).  Only for batches with ONE path per cell (no ambiguity letters: the pair's k-mer is
                                     the reference's at x, the path index 0 -- neither is stored) and fewer than 2^20 reference
                                     positions and events per job: SA_EUNSUPPORTED otherwise.  Read with sa_batch_pairs8 /
                                     sa_batch_pairs8_all; the 16-byte accessors, sa_batch_pairs(_all) and sa_batch_mea return
                                     SA_ESTATE on such a batch. */
#define SA_FLAG_INPUTS_IN_HOST_BLOCK 16u /* every job's `events`, `anchor_x` and `anchor_y` point into ONE block from sa_host_alloc
                                     (8-byte aligned inside it).  The library then does not read them on the host at all: the
                                     part of the block that holds them crosses PCIe with one DMA and a kernel checks the
                                     anchors, narrows them and gathers the event means out of their records -- what
                                     sa_batch_create otherwise does with host cores (416 MB per 2000 reads of 50 000 events
                                     in the reference's four-double records: two host threads cannot keep up with the GPU).
                                     A block laid out with all event records apart from all anchor arrays is sent in two
                                     pieces, and sa_batch_create returns while the event records are still travelling (on
                                     the batch's own stream, ahead of its kernels): the block must stay unchanged until the
                                     batch has RUN (sa_batch_run / sa_batch_wait has returned) or has been destroyed.  Pointers
                                     outside such a block: SA_EINVAL.  Everything else is as without the flag -- a read the
                                     device checks turn down sends the batch to the host planner, which reads the same
                                     memory and names the error -- and the flag is ignored by batches the host plans
                                     (SA_FLAG_EXACT, ...) and by sa_expect_batch's SA_EMISSION_TWO_DIST models.
                                     Layout: what crosses PCIe (and is held in HBM until the batch goes, counted in
                                     sa_batch_stats_t.device_bytes) is the COVERING RANGE of the batch's arrays -- of its event
                                     records and of its anchor arrays when the two lie apart, of everything otherwise -- so a
                                     batch's arrays should be contiguous in the block.  A batch whose covering ranges hold more
                                     than twice the bytes its jobs name (one arena shared by several batches, gaps) is packed
                                     by host threads instead, as without the flag: same results, none of the saving */
#define SA_FLAG_TWO_DIST_ALL_KERNELS 512u /* a Gaussian model with an SA_EMISSION_TWO_DIST* emission (sa_model_set_emission): every region
                                     goes to the kernel family it would get with SA_EMISSION_MEAN_ONLY -- register, ring or strip
                                     kernels -- and that family runs its two-distribution instance, instead of the whole batch
                                     falling back to the reference-ordered kernels as soon as one region holds an ambiguity
                                     letter or a band wider than a wave.  Opt-in: without the flag the routing (and so the
                                     arithmetic) of such a batch is what it was.  Ignored for SA_EMISSION_MEAN_ONLY models, with
                                     SA_FLAG_EXACT or SA_FLAG_FORCE_GENERIC and by the expectation pass (sa_expect_batch); a batch
                                     with a region that even a MeanOnly model would send to the memory-resident kernels falls
                                     back as without the flag.  SA_EUNSUPPORTED with an HDP model.  Required by
                                     sa_batch_create_noise_scaled. */

typedef struct sa_model sa_model_t; /* replaces StateMachine3 / StateMachine3_HDP (inc/stateMachine.h:150-190) */
typedef struct sa_batch sa_batch_t;

/* PairwiseAlignmentParameters (inc/pairwiseAligner.h, defaults impl/pairwiseAligner.c:2022-2037) */
typedef struct sa_params {
    double threshold;                      /* -D */
    int64_t diagonal_expansion;            /* -x, must be even (signalMachine rounds up: impl/signalMachine.c:675) */
    int64_t trace_back_diagonals;          /* -g */
    int64_t min_diags_between_trace_back;  /* 1000 */
    int64_t split_matrix_bigger_than_this; /* 3000*3000 */
} sa_params_t;

/* the slice of a deserialised .nhdp that alignment reads (impl/hdp.c:2588-2612, :2777-2806) */
typedef struct sa_hdp_desc {
    int64_t num_dps;
    int64_t grid_length;
    double grid_start, grid_stop;
    const int64_t *parent;        /* num_dps, -1 for the root                      */
    const uint8_t *observed;      /* num_dps (mark_observed_dps, impl/hdp.c:1132)  */
    const double *const *post_pred; /* num_dps pointers, NULL where unobserved     */
    const double *const *slopes;    /* num_dps pointers, NULL where absent         */
} sa_hdp_desc_t;

/* one alignment = one strand of one read: the arguments of getAlignedPairsUsingAnchors() */
typedef struct sa_job {
    const char *ref;        /* target nucleotides (may hold ambiguity letters); lX = ref_len - (k-1) */
    int64_t ref_len;
    const double *events;   /* event i's mean at events[i*event_stride]; already sliced to the guide alignment
                               (makeEventSequenceFromPairwiseAlignment, impl/signalMachine.c:442) and drift-adjusted */
    int64_t event_stride;   /* in doubles: 4 for the NB_EVENT_PARAMS layout, 1 for a dense mean vector */
    int64_t n_events;
    const int64_t *anchor_x; /* remapped + filtered anchors, (k-mer index, event index)  */
    const int64_t *anchor_y;
    int64_t n_anchors;
    double scale, shift, var; /* sM->scale/shift/var for this read (impl/signalMachine.c:755-757) */
    unsigned ends;          /* SA_JOB_*_END_NOT_RAGGED bits: the last two arguments of getAlignedPairsUsingAnchors(...,
                               bool alignmentHasRaggedLeftEnd, bool alignmentHasRaggedRightEnd) (inc/pairwiseAligner.h:406-414,
                               impl/pairwiseAligner.c:2052-2080), INVERTED so that a zeroed job is signalMachine's call (ragged on
                               both sides, impl/signalMachine.c:436-437).  A bit set = that end is NOT ragged: the alignment starts
                               in (0,0) in the match state / ends in (lX,lY) with the end-state transitions
                               (stateMachine3_startStateProb / _endStateProb, impl/stateMachine.c:1134-1173) and getSplitPoints
                               keeps the outer rectangle of a gap that is cut at that end (impl/pairwiseAligner.c:1910-1937);
                               the reference's own known-answer tests call it with (0, 0) (tests/stateMachineTests.c:943-947) */
} sa_job_t;
#define SA_JOB_LEFT_END_NOT_RAGGED 1u   /* alignmentHasRaggedLeftEnd == false  */
#define SA_JOB_RIGHT_END_NOT_RAGGED 2u  /* alignmentHasRaggedRightEnd == false */

/* stIntTuple4(floor(p*1e7), x, y, (char*)pathKmer)  (impl/pairwiseAligner.c:1405-1408) */
typedef struct sa_pair {
    int64_t prob_e7;
    int32_t x, y;
    int32_t path;    /* index of the path inside the cell (order of hdCell_construct2) */
    int32_t kmer_id; /* kmer_id() of the path's k-mer                                  */
} sa_pair_t;

/* The same tuple as it lives in HBM and crosses PCIe: 16 bytes instead of 24 (2000 x 5000-event reads return 9 million pairs
 * per batch; broad HDP densities at threshold 0.01 four hundred million).  This is what a finished batch HOLDS, in pinned host
 * memory, job after job in output order: sa_batch_pairs16 hands out a job's records in place (no copy), sa_batch_pairs and
 * sa_batch_pairs_all expand them into sa_pair_t.
 *   a = x (28 bits) | y (28 bits) << 28 | path bits 0..7 << 56        (the planners refuse matrices of 2^28 rows or columns
 *   b = kmer_id (32 bits) | prob_e7 (24 bits: <= 1e7) << 32 | path bits 8..15 << 56        and cells of more than 65535 paths) */
typedef struct sa_pair16 {
    uint64_t a, b;
} sa_pair16_t;
#if defined(__HIPCC__) || defined(__HIP__)
#define SA_PAIR16_ATTR __host__ __device__
#else
#define SA_PAIR16_ATTR
#endif
#define SA_PAIR16_FN static inline
#define SA_PAIR16_MAX_COORD (1ll << 28) /* x, y below this */
#define SA_PAIR16_MAX_PATHS 65536       /* paths per cell at most this */
SA_PAIR16_ATTR SA_PAIR16_FN sa_pair16_t sa_pair16_pack(int64_t prob_e7, int32_t x, int32_t y, int32_t path, int32_t kmer_id) {
    sa_pair16_t r;
    r.a = ((uint64_t) (uint32_t) x & 0xfffffffull) | (((uint64_t) (uint32_t) y & 0xfffffffull) << 28) |
          ((uint64_t) ((uint32_t) path & 0xffu) << 56);
    r.b = (uint64_t) (uint32_t) kmer_id | (((uint64_t) prob_e7 & 0xffffffull) << 32) |
          ((uint64_t) (((uint32_t) path >> 8) & 0xffu) << 56);
    return r;
}
SA_PAIR16_ATTR SA_PAIR16_FN sa_pair_t sa_pair16_unpack(sa_pair16_t r) {
    sa_pair_t o;
    o.x = (int32_t) (r.a & 0xfffffffull);
    o.y = (int32_t) ((r.a >> 28) & 0xfffffffull);
    o.path = (int32_t) (((r.a >> 56) & 0xffull) | (((r.b >> 56) & 0xffull) << 8));
    o.kmer_id = (int32_t) (uint32_t) (r.b & 0xffffffffull);
    o.prob_e7 = (int64_t) ((r.b >> 32) & 0xffffffull);
    return o;
}

/* SA_FLAG_PAIRS8: prob_e7 (24 bits: <= 1e7) << 40 | y (20 bits) << 20 | x (20 bits) */
typedef uint64_t sa_pair8_t;
#define SA_PAIR8_MAX_COORD (1ll << 20)
SA_PAIR16_ATTR SA_PAIR16_FN sa_pair8_t sa_pair8_pack(int64_t prob_e7, int32_t x, int32_t y) {
    return ((uint64_t) prob_e7 << 40) | (((uint64_t) (uint32_t) y & 0xfffffull) << 20) | ((uint64_t) (uint32_t) x & 0xfffffull);
}
SA_PAIR16_ATTR SA_PAIR16_FN void sa_pair8_unpack(sa_pair8_t r, int64_t *prob_e7, int32_t *x, int32_t *y) {
    *x = (int32_t) (r & 0xfffffull);
    *y = (int32_t) ((r >> 20) & 0xfffffull);
    *prob_e7 = (int64_t) (r >> 40);
}

/* Test hook (host only): `in` through the packed 16-byte record and back into `out`. */
int sa_pair_roundtrip(const sa_pair_t *in, sa_pair_t *out, int64_t n);

typedef struct sa_batch_stats {
    double cells_forward;    /* sum over forward diagonals of width*paths           */
    double cells_backward;   /* ditto for backward diagonals actually computed      */
    double ms_forward;       /* HIP-event time of the forward kernels, last run     */
    double ms_backward;      /* traceback stage: end of the forward sweep -> end of the last backward+posterior
                                kernel (the groups' launches overlap on two streams; fold/finalisation kernels of
                                earlier groups run inside this window)                                        */
    double ms_fold;          /* rest of the pass: fold (+ on-device finalisation) of the last group          */
    double ms_total_device;  /* first launch -> last kernel end                     */
    double f_bytes;          /* bytes of forward storage written (== read back)     */
    int64_t n_regions, n_segments, n_checkpoints;
    int64_t n_fast_regions;  /* regions handled by the register-resident kernels    */
    int64_t n_chunks;        /* passes needed to fit forward storage in HBM         */
    int64_t n_groups;        /* backward/posterior launches per pass (result copy of one overlaps the next) */
    int64_t n_ring_regions;  /* regions handled by the LDS-ring kernels (several paths per cell, or a band mostly wider
                                than a wave)                                           */
    int64_t n_strip_regions; /* of those: one-path regions swept in strips of 64 reference columns (register-resident,
                                no barrier; sa_strip.inc)                               */
    double device_bytes;     /* working storage of the batch in HBM: forward planes, emission plane (HDP), candidate and
                                result slots, checkpoint buffers -- what a caller sizes its pipeline depth with */
} sa_batch_stats_t;

/* ---- model -------------------------------------------------------------------------------------
 * Replaces stateMachine3_loadFromFile()'s result (impl/stateMachine.c:1440-1538):
 *   transitions10: the 10 tokens of the transition line, linear space;
 *   table5: 5*A^k doubles [level_mean level_sd noise_mean noise_sd noise_lambda] in kmer_id order.
 * hdp != NULL selects the HDP emission (stateMachine3HDP_cellCalculate, impl/stateMachine.c:1371);
 * the caller applies stateMachine3_setModelToHdpExpectedValues with sa_model_set_to_hdp_expected_values. */
int sa_model_create(sa_model_t **out, int n_states, const char *alphabet, int k, const double *transitions10,
                    const double *table5, const sa_hdp_desc_t *hdp);
int sa_model_load(sa_model_t **out, const char *model_path, const char *nhdp_path_or_null);
void sa_model_destroy(sa_model_t *m);
int sa_model_alphabet(const sa_model_t *m, char *out64, int *n_alpha, int *k);
const double *sa_model_table5(const sa_model_t *m);        /* EMISSION_MATCH_MATRIX view */
int sa_model_set_to_hdp_expected_values(sa_model_t *m);    /* impl/stateMachine.c:1275-1304 */
int64_t sa_kmer_id(const sa_model_t *m, const char *kmer); /* impl/nanopore_hdp.c:405-410 */
/* Which match / gapY emission a Gaussian model uses (the function pointers stateMachine3_construct takes, inc/stateMachine.h):
 *   SA_EMISSION_MEAN_ONLY  emissions_signal_strawManGetKmerEventMatchProbWithDescaling_MeanOnly (impl/stateMachine.c:557-605),
 *                          what signalMachine installs (impl/signalMachine.c:337); every kernel family
 *   SA_EMISSION_TWO_DIST   emissions_signal_strawManGetKmerEventMatchProbWithDescaling (:607-650): Gaussian on the descaled mean
 *                          x inverse Gaussian on the event noise -- what the reference's shipped output files were written with
 *                          (tests/test_oracle_reference_outputs.py).  Register kernels (round 6: k_fwd_fast_two / k_bwd_fast_two) when
 *                          every region of the batch holds one path per cell (sa_align_batch / sa_batch_*; not the expectation
 *                          pass); otherwise, and with SA_FLAG_EXACT, the reference-ordered memory-resident kernels (the batch then
 *                          behaves as with SA_FLAG_EXACT); jobs must hand over event records (event_stride >= 2: the
 *                          noise is a record's second value).  With SA_FLAG_TWO_DIST_ALL_KERNELS the ring and strip kernels run
 *                          two-distribution instances too (k_*_ring<..., TWO>, k_*_strip<..., TWO>) and no region sends the
 *                          batch to the reference-ordered kernels for its ambiguity letters or its band.  The noise columns
 *                          are the MODEL's, so the reads of a batch created with sa_batch_create share one noise scaling; the
 *                          reference rescales them per read (emissions_signal_scaleNoise): hand every job its two factors
 *                          with sa_batch_create_noise_scaled, or create a model per read from the rescaled table
 *                          sa_estimate_params leaves (sa_model_clone_with_table). */
#define SA_EMISSION_MEAN_ONLY 0
#define SA_EMISSION_TWO_DIST 1
/*   SA_EMISSION_TWO_DIST_SCALED_MODEL  emissions_signal_strawManGetKmerEventMatchProb (:659-700): the same two distributions on the
 *                          event mean AS IT IS -- no descaling, the job's scale / shift / var are not read; the model table was scaled
 *                          to the read instead (emissions_signal_scaleModel :743-779).  What getStateMachine3 installs (:1757-1765):
 *                          the emission of the reference's literal-data known answers (tests/stateMachineTests.c:441-698) and of its
 *                          scaled-model whole-read test (:842-852).  Same kernels and conditions as SA_EMISSION_TWO_DIST. */
#define SA_EMISSION_TWO_DIST_SCALED_MODEL 2
/* Event noise under an SA_EMISSION_TWO_DIST* model: every event's noise must be a finite number greater than zero; under
 * SA_EMISSION_TWO_DIST zero is legal too and is replaced by 1e-9 as the reference does (impl/stateMachine.c:619-621).  NaN, +-inf, a
 * negative value, and zero under SA_EMISSION_TWO_DIST_SCALED_MODEL give the reference a NaN total and no pairs; here sa_batch_create*
 * (and sa_expect_batch / sa_align_batch through it) refuses the whole batch with SA_EINVAL and one line on stderr that names the
 * job and the event, before anything is launched -- the rule of event means that are not finite (sa_batch_run).  A finite noise of
 * any size is legal: 1e300 gives that read a total of -inf and no pairs, and leaves the other reads' results alone.  An
 * SA_EMISSION_MEAN_ONLY model never reads the noise column. */
int sa_model_set_emission(sa_model_t *m, int emission);
/* A Gaussian model with the same alphabet, k-mer length, transitions and emission kind as `m` and the emission table `table5`
 * (5 * A^k doubles, copied): the per-read model the reference gets from emissions_signal_scaleNoise (impl/stateMachine.c:721-741)
 * -- sa_estimate_params leaves the rescaled table in its table5_inout argument. */
int sa_model_clone_with_table(sa_model_t **out, const sa_model_t *m, const double *table5);

/* ambiguity table: 256 entries (index = character), NULL = not ambiguous.
 * sa_default_ambig fills create_ambig_bases() (impl/pairwiseAligner.c:32-65);
 * sa_load_ambig reads the -a file (create_ambig_bases2, impl/pairwiseAligner.c:68-92); strings are
 * owned by a static/heap pool that lives until the process ends. */
void sa_default_ambig(const char **map256);
int sa_load_ambig(const char *path, const char **map256);

/* ---- batched getAlignedPairsUsingAnchors (impl/pairwiseAligner.c:2052-2080) --------------------
 * create: host-side planning (split regions, band tables, traceback segments) + upload to HBM.
 * run:    forward, backward/posterior and fold kernels; inputs are already resident.
 * pairs:  rows in the order signalMachine writes them (stable sort by x+y of the reference's list). */
int sa_batch_create(sa_batch_t **out, const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs,
                    int64_t n_jobs, const char *const *ambig256, int device, unsigned flags);
/* sa_batch_create with the noise columns of the model rescaled PER JOB: job j is aligned as if its model were
 * sa_model_clone_with_table(m, T_j), T_j = emissions_signal_scaleNoise (impl/stateMachine.c:721-741) of m's table with noise[j] --
 * noise_mean * scale_sd and noise_lambda * var_sd, each product rounded to a double before anything is derived from it.  The two
 * factors are out7[4] and out7[5] of sa_estimate_params.  What signalMachine --batch --emission twoDist needs: one batch, one
 * model, every read its own noise scaling.  Requires SA_FLAG_TWO_DIST_ALL_KERNELS, an SA_EMISSION_TWO_DIST* model and event
 * records (event_stride >= 2); every factor finite and > 0: SA_EINVAL otherwise.  The scaling exists in the register, ring and
 * strip kernels' two-distribution instances only: a batch with a region none of them takes (SA_FLAG_EXACT, SA_FLAG_FORCE_GENERIC,
 * threshold 0, a matrix whose storage does not fit, the ring kernels switched off) returns SA_EUNSUPPORTED -- it is never aligned
 * with the model's own noise without a word.  `noise` is copied. */
typedef struct sa_noise_scale { double scale_sd, var_sd; } sa_noise_scale_t;   /* out7[4], out7[5] of sa_estimate_params */
int sa_batch_create_noise_scaled(sa_batch_t **out, const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs,
                                 const sa_noise_scale_t *noise /* n_jobs */, int64_t n_jobs,
                                 const char *const *ambig256, int device, unsigned flags);
int sa_batch_run(sa_batch_t *b);
/* sa_batch_create in two halves, for a caller that streams batches (sa_batch_start / sa_batch_wait below).  The first half --
 * input checks, packing and upload of the reads, the planning kernels queued -- runs here; the second -- waiting for the plan,
 * working buffers, launch lists -- on the batch's first use (sa_batch_run or the thread of sa_batch_start, sa_batch_stats,
 * sa_batch_job_cells), so the calling thread does not wait for the GPU and can pack the next batch.  Same arguments and
 * results as sa_batch_create; what differs: `jobs` and `ambig256` must stay valid until that first use has returned (a read
 * the planning kernels turn down sends the batch to the host planner, which reads them again), and an error found by the
 * second half is returned by that first use instead.  A batch the planning kernels do not take at all (an ambiguity letter
 * with repeated options, SA_FLAG_EXACT, ...) is created completely, as by sa_batch_create. */
int sa_batch_create_deferred(sa_batch_t **out, const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs,
                             int64_t n_jobs, const char *const *ambig256, int device, unsigned flags);
/* Optional, between the two halves: waits for the plan and builds the launch lists -- the part of the second half that needs no
 * working storage -- so that a caller whose batches take the device one at a time (SA_FLAG_DEVICE_TO_ITSELF) can have it done
 * while the batch before is still running; the batch's first use then only takes its buffers.  Counts as a first use for the
 * lifetime of `jobs` / `ambig256`; returns what that part of the second half returns (and the first use returns it again). */
int sa_batch_prepare(sa_batch_t *b);
/* The same on a thread of the library's own: sa_batch_start returns at once, sa_batch_wait returns sa_batch_run's code.
 * Lets one caller thread plan the next batch (sa_batch_create is host work) while this one is on the GPU. */
int sa_batch_start(sa_batch_t *b);
int sa_batch_wait(sa_batch_t *b);
int sa_batch_n_pairs(const sa_batch_t *b, int64_t job, int64_t *n);
int sa_batch_pairs(const sa_batch_t *b, int64_t job, sa_pair_t *out, int64_t cap);
/* A job's number of pairs and the sum of their prob_e7 over ALL pairs above the threshold -- with SA_FLAG_VC_ROWS including the rows
 * that were dropped on the device (without the flag: of the rows the batch holds).  100 * sum / (n * 1e7) is
 * scoreByPosteriorProbabilityIgnoringGaps (impl/pairwiseAligner.c:407-412). */
int sa_batch_all_pairs_summary(const sa_batch_t *b, int64_t job, int64_t *n_all, int64_t *sum_prob_e7);
/* A job's pairs as the batch holds them: *out points at *n packed records (sa_pair16_t above) inside the batch's pinned result
 * block, valid until the batch is run again or destroyed.  Nothing is copied: this is where sa_batch_run / sa_batch_wait
 * leaves the results, and the form a caller that formats or forwards them reads (signalMachine's TSV writers, sa_batch_mea). */
int sa_batch_pairs16(const sa_batch_t *b, int64_t job, const sa_pair16_t **out, int64_t *n);
/* The whole batch at once: the records of all jobs are contiguous in job order; *out is the first record of job 0 and job j's
 * are (*out)[first[j] .. first[j + 1]) (`first`: n_jobs + 1 entries, may be NULL). */
int sa_batch_pairs16_all(const sa_batch_t *b, const sa_pair16_t **out, int64_t *first);
/* the same two for a batch created with SA_FLAG_PAIRS8 (8-byte records, in place, job after job) */
int sa_batch_pairs8(const sa_batch_t *b, int64_t job, const sa_pair8_t **out, int64_t *n);
int sa_batch_pairs8_all(const sa_batch_t *b, const sa_pair8_t **out, int64_t *first);
/* Every job's pairs expanded into sa_pair_t, job after job, on the library's host threads: out[first[j] .. first[j + 1]) are
 * job j's rows (`first` has n_jobs + 1 entries; may be NULL).  cap < total number of pairs: SA_EINVAL and *first is still
 * filled, so first[n_jobs] says how much room is needed. */
int sa_batch_pairs_all(const sa_batch_t *b, sa_pair_t *out, int64_t cap, int64_t *first);
/* A finished batch's working storage in HBM (everything sa_batch_stats_t.device_bytes counts) back to the library's allocator,
 * the results kept: the packed pairs in pinned host memory, the per-job offsets and the statistics stay readable until
 * sa_batch_destroy.  For a caller that holds batches for their results while further ones are created (signalMachine --twoD
 * keeps the template strand's batch while the complement's runs).  Afterwards sa_batch_run / sa_batch_start: SA_ESTATE;
 * sa_batch_mea still works (the pairs are uploaded again).  Before the batch has run, or between sa_batch_start and
 * sa_batch_wait: SA_ESTATE. */
int sa_batch_release_device(sa_batch_t *b);
int sa_batch_stats(const sa_batch_t *b, sa_batch_stats_t *out);
int sa_batch_job_cells(const sa_batch_t *b, int64_t job, double *cells_fwd, double *cells_bwd);
void sa_batch_destroy(sa_batch_t *b);

/* one-shot convenience: create + run + copy out.  pairs_out[j] is malloc'd (sa_free). */
int sa_align_batch(const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs, int64_t n_jobs,
                   const char *const *ambig256, int device, unsigned flags, sa_pair_t **pairs_out,
                   int64_t *n_pairs_out);

/* ---- batched getExpectationsUsingAnchors (impl/pairwiseAligner.c:2164-2184) --------------------
 * trans9_out[j*9 + from*3 + to] and likelihood_out[j] are ADDED to (the caller seeds pseudocounts, as
 * hmmContinuous_getExpectationsHmm does); HDP assignments (to==match && p>=threshold,
 * impl/pairwiseAligner.c:946-968) come back as (reference position, event index) pairs.
 * A read whose total probability is -inf (an event beyond the HDP's grid where the density is zero, an event mean or noise so large
 * that its squared deviation overflows: every path through the event has probability zero).  The reference adds -inf to the
 * likelihood and exp(-inf - -inf) = NaN to every transition expectation.  Here every group of ten diagonals whose total is -inf adds
 * -inf to likelihood_out[j] and NOTHING to trans9_out[j]: the read's likelihood is -inf -- the value to test for -- and its
 * expectations are those of the tracebacks that ended before the event, all zero when there is none.  The same from the register,
 * ring and memory-resident kernels; no other read of the batch is touched (tests/test_gpu_outlier_events.py). */
typedef struct sa_assignment {
    int64_t ref_pos;   /* index into job.ref of the cell's k-mer pointer (cX) */
    int64_t event;     /* index into the job's event array (cY)               */
} sa_assignment_t;
int sa_expect_batch(const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs, int64_t n_jobs,
                    const char *const *ambig256, int device, unsigned flags, double *trans9_out,
                    double *likelihood_out, sa_assignment_t **assign_out, int64_t *n_assign_out);

/* Test / measurement hook: the batch statistics (regions per kernel family, kernel times, passes) of the calling thread's last
 * sa_expect_batch. */
int sa_expect_last_stats(sa_batch_stats_t *out);

/* ---- planning introspection (host only, no GPU needed; used by the CPU test-suite) --------------
 * Builds the plan for ONE job and reports its geometry. */
typedef struct sa_plan_info {
    int64_t n_regions, n_segments, n_checkpoints;
    double cells_forward, cells_backward;
    int64_t f_cellpaths;   /* cell-paths of forward storage */
    int64_t max_span;      /* widest 3-row window in (x-y)/2 units          */
    int64_t n_fast_regions;
    int64_t n_ring_regions;
} sa_plan_info_t;
int sa_plan_describe(const sa_model_t *m, const sa_params_t *p, const sa_job_t *job, const char *const *ambig256,
                     unsigned flags, sa_plan_info_t *info,
                     int64_t *regions4_out, int64_t regions_cap,   /* x1,y1,x2,y2 per region             */
                     int64_t *rows3_out, int64_t rows_cap,         /* region,xmyL,xmyR per diagonal      */
                     int64_t *segs4_out, int64_t segs_cap);        /* region,start,from,to per traceback */

/* Test hook (host only): the per-path neighbour records the planner writes for regions with ambiguous positions, checked
 * against path_checkLegal (impl/pairwiseAligner.c:595-621) pair by pair.  Returns the number of wrong entries (0 = all
 * good) or a negative SA_E* code; *n_checked = entries examined. */
int64_t sa_plan_check_path_records(const sa_model_t *m, const sa_params_t *p, const sa_job_t *job,
                                   const char *const *ambig256, int64_t *n_checked);

/* Test hook (needs a GPU): plans the batch on the device and on the host and compares every array the kernels read.
 * 0: identical; > 0: bit mask of the arrays that differ (1 << 30: the batch is not one the device planner takes);
 * < 0: SA_E* code. */
int sa_dplan_compare(const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs, int64_t n_jobs,
                     const char *const *ambig256, int device, unsigned flags);

/* ---- event <-> k-mer pre-alignment (the step upstream of the pair-HMM) ------------
 * adaptive_banded_simple_event_align (impl/eventAligner.c:899-1235): adaptive banded Viterbi of a raw event table
 * against the k-mers of the basecalled sequence, with the state machine's MeanOnly match emission
 * (impl/eventAligner.c:1245-1247).  One wave per read on the GPU.  pairs_out[j] (malloc'd, sa_free) holds the
 * struct AlignedPair list {ref_pos = k-mer index, read_pos = event index} in ascending order; it is empty and
 * status_out[j] != 0 when the reference would have rejected the alignment (bit 0: average log emission < -5.2, bit 1:
 * first/last k-mer not reached, bit 2: more than 50 skipped k-mers in a row, bit 3: more than 5 events per k-mer).
 * Bit-identical to the CPU restatement; the reference's own literals are pinned through sa_raw_event_align_batch below. */
typedef struct sa_ea_job {
    const char *sequence;      /* nucleotides; a k-mer at every position (build_kmer_list, impl/eventAligner.c:755-782) */
    int64_t seq_len;
    const double *event_mean;  /* event_t.mean of the raw event table                                                  */
    int64_t n_events;
    double scale, shift, var;  /* update_SignalMachineWithNanoporeParameters (:845-849); see sa_scalings_mom           */
} sa_ea_job_t;
typedef struct sa_ea_pair {
    int32_t kmer_idx, event_idx;
} sa_ea_pair_t;
/* estimate_scalings_using_mom (impl/eventAligner.c:784-843): method of moments; the reference then uses var = 1 */
int sa_scalings_mom(const sa_model_t *m, const char *sequence, int64_t seq_len, const double *event_mean,
                    int64_t n_events, unsigned flags, double *shift_out, double *scale_out);
/* cells_out[j] (may be NULL): band cells filled for job j (the reference's `fills`); kernel_ms_out (may be NULL):
 * HIP-event time of the kernel.
 * SA_EINVAL, with one line on stderr and before any kernel is launched, when a job's scale, shift, var or one of its
 * event means is not a finite number: with a NaN event the reference's own traceback leaves the band and reads memory it
 * never wrote, so there is no result to reproduce (the pair-HMM batch refuses such an event the same way). */
int sa_event_align_batch(const sa_model_t *m, const sa_ea_job_t *jobs, int64_t n_jobs, int device, unsigned flags,
                         sa_ea_pair_t **pairs_out, int64_t *n_pairs_out, int32_t *status_out, double *cells_out,
                         double *kernel_ms_out);
/* sa_event_align_batch keeps its device and pinned-host scratch between calls (grow only, one workspace per process,
 * calls serialise on it); this returns the memory.  Safe to call at any time, also when nothing is held. */
void sa_event_align_release(void);

/* ---- event detection from raw current, chained into event alignment ------------------------------------------------
 * detect_events (impl/event_detection.c:268-330, Scrappie's t-statistic detector) for many reads in one call, and
 * load_from_raw2 (impl/eventAligner.c:1242-1300) up to the table fast5_set_basecall_event_table writes.  Events are
 * bit-identical to the reference's arithmetic: raw to pA in float, sum / sum of squares as sequential double folds (the
 * square a float product), compute_tstat's mix of double sums and float means, the short/long peak detector's integer
 * semantics, create_event's float mean and stdv.  Callers read the fast5 themselves: int16 samples plus the channel_id
 * attributes and the read's start_time, as floats (the reference reads them through H5T_NATIVE_FLOAT).
 * Departures from the reference's undefined behaviour: a read whose detector emits no peak is ONE event [0, n) and its
 * status has SA_RAW_NO_PEAK (the reference indexes peaks[-1]); n_samples == 0 is SA_EINVAL (the reference asserts).
 * No trimming: every caller of trim_and_segment_raw in the reference discards its result, so detection runs over all
 * n_samples. */
typedef struct sa_raw_job {
    const int16_t *raw;        /* Raw/Reads/Read_* /Signal, ADC counts                                              */
    int64_t n_samples;         /* 1 .. 2^31 - 1                                                                      */
    float digitisation, offset, range, sample_rate;  /* UniqueGlobalKey/channel_id (sample_rate: "sampling_rate")   */
    float start_time;          /* Raw/Reads/Read_* start_time                                                        */
} sa_raw_job_t;
typedef struct sa_detector_params {
    int32_t window_length1, window_length2;   /* >= 1 */
    float threshold1, threshold2, peak_height;
} sa_detector_params_t;
/* inc/event_detection.h: event_detection_defaults and event_detection_rna */
#define SA_DETECTOR_DNA {3, 6, 1.4f, 9.0f, 0.2f}
#define SA_DETECTOR_RNA {7, 14, 2.5f, 9.0f, 1.0f}
/* one row of the basecalled event table (basecalled_event, inc/eventAligner.h:16-26; event_table_to_basecalled_table,
 * impl/eventAligner.c:744-768): the detector's float values widened to double, start / length in seconds */
typedef struct sa_raw_event {
    int64_t raw_start, raw_length;
    double mean, stdv;
    double start, length;
    int32_t kmer_idx;          /* model_state as the k-mer position in the sequence (build_kmer_list order); -1: none */
    int32_t move;
    double p_model_state;      /* exp of the MeanOnly log emission of model_state under the MoM scalings; 0 unmapped */
} sa_raw_event_t;
#define SA_RAW_NO_PEAK 16      /* status bit: the detector emitted no peak (one event spans the read) */
/* params NULL: SA_DETECTOR_DNA, or SA_DETECTOR_RNA with SA_FLAG_RNA.  events_out[j] (malloc'd, sa_free) holds job j's
 * n_events_out[j] events in time order, kmer_idx -1.  status_out (may be NULL): 0 or SA_RAW_NO_PEAK per job;
 * kernel_ms_out (may be NULL): HIP-event time of the detection kernels. */
int sa_detect_events_batch(const sa_raw_job_t *jobs, int64_t n_jobs, const sa_detector_params_t *params, int device,
                           unsigned flags, sa_raw_event_t **events_out, int64_t *n_events_out, int32_t *status_out,
                           double *kernel_ms_out);
/* load_from_raw2 for a batch: detection as above; with SA_FLAG_RNA the events reversed (reverse_events); MoM scalings
 * (sa_scalings_mom on the events' means); sa_event_align_batch with var = 1; the base-to-event map on the host
 * (alignment_to_base_event_map, with its skip of a second pair on one event while the previous k-mer is 0, or for RNA
 * rna_alignment_to_base_event_map walked from the last pair, the table then reversed back to time order).
 * events_out[j] is in time order with kmer_idx / move / p_model_state filled for mapped events (the rows the reference
 * writes); pairs_out (may be NULL) receives sa_event_align_batch's pairs, event indices in the aligned order (reversed
 * for RNA); status_out: sa_event_align_batch's bits | SA_RAW_NO_PEAK (a non-zero EA status leaves every event unmapped);
 * shift_out / scale_out (may be NULL): the MoM scalings; kernel_ms_out (may be NULL): detection + alignment kernels. */
int sa_raw_event_align_batch(const sa_model_t *m, const sa_raw_job_t *jobs, const char *const *sequences, int64_t n_jobs,
                             const sa_detector_params_t *params, int device, unsigned flags, sa_raw_event_t **events_out,
                             int64_t *n_events_out, sa_ea_pair_t **pairs_out, int64_t *n_pairs_out, int32_t *status_out,
                             double *shift_out, double *scale_out, double *kernel_ms_out);
/* the detector's device and pinned-host scratch, kept between calls (grow only), returned */
void sa_detect_release(void);

/* ---- raw current -> the in-memory .npRead of a 1D read ---------------------------------------------------------------
 * What NanoporeRead (src/signalalign/nanoporeRead.py) holds for a 1D read after load_from_raw2 has written the basecalled
 * event table: the mapped rows (kmer_idx >= 0) of sa_raw_event_align_batch in time order, in the .npRead's own layout, and
 * the strand event map over them.  Detection, MoM scalings and event alignment are the entry points above (one detector, one
 * event aligner); the base-to-event map, the compaction to mapped rows and the table's seconds are one more kernel
 * (k_raw_finish, one wave per read) on the rows the detector left on the device -- bit-identical to
 * sa_raw_event_align_batch's rows; p_model_state and make_event_map (which compares those values) are computed on the host.
 * DNA, template strand: SA_FLAG_RNA returns SA_EUNSUPPORTED, and so does an HDP model (as sa_raw_event_align_batch).
 * SA_EINVAL, before any device use: a NULL array, n_jobs < 0, a read without samples, a sequence shorter than the model's k,
 * a detector window < 1. */
#define SA_RAW_MAP_LENGTH 32   /* status bit: the event map's length differs from the read's ("Read and event map lengths do not match") */
typedef struct sa_raw_npread {
    int32_t status;            /* sa_raw_event_align_batch's bits | SA_RAW_MAP_LENGTH; non-zero: nothing below is filled (the
                                  arrays are NULL, n_events 0) but read_len and the MoM scalings                             */
    int64_t n_events;          /* mapped rows only: the rows the reference writes to the basecalled table                    */
    double *events4;           /* n_events x {mean, stdv, length, start - start of row 0}: the .npRead layout, sa_job_t's stride 4 */
    int32_t *kmer_idx, *move;  /* per row */
    double *p_model_state;     /* per row */
    int64_t *raw_start, *raw_length;
    int64_t read_len;
    int64_t *strand_event_map; /* read_len entries: NanoporeRead.make_event_map (nanoporeRead.py:313-333) */
    double mom_shift, mom_scale;
} sa_raw_npread_t;
/* params NULL: SA_DETECTOR_DNA.  out: n_jobs entries, released with sa_raw_npread_free (a read's arrays are one allocation: do
 * not free them one by one).  A read the chain rejects fails alone: its status is set, its arrays are NULL, the others are
 * what they are without it.  kernel_ms_out (may be NULL): detection + alignment + finishing kernels. */
int  sa_npread_from_raw_batch(const sa_model_t *m, const sa_raw_job_t *jobs, const char *const *sequences, int64_t n_jobs,
                              const sa_detector_params_t *params, int device, unsigned flags,
                              sa_raw_npread_t *out, double *kernel_ms_out);
void sa_raw_npread_free(sa_raw_npread_t *r, int64_t n);
/* HIP-event time of k_raw_finish alone in the process's last sa_npread_from_raw_batch (probes/raw_front_door_rate.py) */
double sa_npread_last_finish_ms(void);
/* The fourteen lines of NanoporeRead.Write (nanoporeRead.py:438-540) for a 1D read: 2D length 0, the strand parameters
 * 1 1 1 1 1 0 twice and has-2D 0 (signalMachine estimates them anew), no complement, model states spelled from `sequence` at
 * kmer_idx, floats as Python prints a float64 (sa_format_py_repr), every list entry followed by a blank.  SA_EINVAL: NULL
 * argument, a read with status != 0, a sequence whose length is not read_len; SA_EIO: the file cannot be written. */
int  sa_raw_npread_write(const sa_raw_npread_t *r, const char *sequence, const sa_model_t *m, const char *path);

/* fastaHandler_getSubSequence (impl/fasta_handler.c:15-44, htslib faidx underneath): bases [start, end) of the record
 * `name` (the header's first word) of a FASTA file; strand == 0 asks htslib for [end, start - 1] as the reference does.
 * Uses <path>.fai when it exists, otherwise scans the file (nothing is written).  *out is freed with sa_free.
 * SA_EIO: file unreadable; SA_EINVAL: no such record. */
int sa_fasta_subsequence(const char *fasta_path, const char *name, int64_t start, int64_t end, int strand, char **out);
/* printf("%f") of v, character for character (the exact binary value rounded to six decimals, ties to even -- glibc's result),
 * without the stdio formatter: what the TSV writers (impl/signalMachine.c:89-270: nine "%f" per aligned pair) spend their time
 * in.  `out` needs 32 bytes for |v| < 9e15 (larger values, inf and nan go through snprintf: up to 320); a terminator is
 * written; returns the length. */
int sa_format_f6(char *out, double v);
/* How pandas' to_csv prints np.round(v, 6) -- Python's repr of that double ("0.5", "1.0", "0.123457", "5e-05"): the value
 * columns of AggregateOverReadsFull.write_data (src/signalalign/variantCaller.py:393-410).  For 0 <= v <= 1; `out` needs 32
 * bytes; returns the length. */
int sa_format_py_round6(char *out, double v);

/* Batches take their device and pinned-host storage from a caching allocator: what a destroyed batch held is kept and
 * handed to the next one (a pipeline that sees every read once creates and destroys a batch per few thousand reads;
 * allocation and release of its 25 GB cost more than its kernels).  What may stay PARKED between batches is bounded:
 * by default 90 % of the device's memory and 32 GB of pinned host memory (parked device blocks are handed back to the
 * runtime whenever an allocation of the process fails, so the cache never causes an out-of-memory by itself).
 * An embedding caller that shares the device or the host with other code sets its own bounds:
 *   sa_pool_configure(device_limit_bytes, pinned_limit_bytes)   a negative value leaves that bound as it is; 0 keeps nothing
 *       parked; blocks above a lowered bound are freed at once.  Wins over the environment.
 *   sa_pool_release()                                           returns everything that is parked right now.
 *   sa_pool_release_device()                                    ... the device blocks only (page-locked blocks stay parked)
 * sa_host_alloc / sa_host_free: page-locked host memory for a caller's own input arrays (SA_FLAG_INPUTS_IN_HOST_BLOCK); a
 * block belongs to the caller until sa_host_free, which must not be called before every batch created from it has run or has
 * been destroyed.
 * Environment (read when no limit was configured): SA_POOL=0 disables the cache, SA_POOL_LIMIT_GB bounds both kinds. */
int sa_pool_configure(int64_t device_limit_bytes, int64_t pinned_limit_bytes);
void *sa_host_alloc(size_t bytes);   /* NULL: no memory (or no device) */
void sa_host_free(void *block);      /* NULL or a pointer sa_host_alloc did not return: ignored */
void sa_pool_release(void);
void sa_pool_release_device(void);

/* ---- maximum-expected-accuracy path over a read's posteriors ----------------------------------
 * Replaces maximum_expected_accuracy_alignment + get_indexes_from_best_path (src/signalalign/mea_algorithm.py:25-197,
 * :248-264; called by mea_alignment_from_signal_align :323-341): the best monotone path through the sparse posterior
 * matrix, one (reference position, event) pair per event, bit-identical to the reference's choice among ties.
 * A job is what that function receives: the COO form of posterior_matrix (row = event, column = reference position,
 * row-major as scipy.sparse.coo_matrix(dense) yields it) and shortest_ref_per_event (INT32_MAX where the reference
 * holds inf).  sa_mea_params builds both from the columns of a signalAlign event table.  Pinned by the reference's
 * known-answer matrix (tests/golden/mea/kat_5x5.json). */
#define SA_MEA_OK 0
#define SA_MEA_EMPTY 1        /* no entries: the reference raises ValueError (min of an empty sequence, :42)   */
#define SA_MEA_SINGLE_EVENT 2 /* every entry belongs to the first event: IndexError at :61                      */
#define SA_MEA_NO_FRONT 3     /* an event starts with no forward edge left: IndexError at :106                  */
#define SA_MEA_NO_PATH 4      /* no final edge with a sum above 0: the reference returns the int 0 (:188-196)   */
#define SA_MEA_BAD_EVENT 5    /* event index outside shortest_ref_per_event: IndexError at :106                 */
#define SA_MEA_INF 2147483647 /* shortest_ref_per_event of an event without rows                                */
typedef struct sa_mea_job {
    const int32_t *event_idx;               /* COO row    */
    const int32_t *ref_idx;                 /* COO column */
    const double *posterior;                /* COO data   */
    int64_t n;
    const int32_t *shortest_ref_per_event;  /* indexed by event_idx */
    int64_t n_events;
} sa_mea_job_t;
typedef struct sa_mea_pair {
    int32_t ref_idx, event_idx;             /* get_indexes_from_best_path: [ref_pos, event_pos] */
} sa_mea_pair_t;
/* One wave per read.  path_out[j] (malloc'd, sa_free) holds n_path_out[j] pairs in path order; status_out[j] one of
 * SA_MEA_* (a failed read has no path and does not fail the call); sum_out[j] the best edge's sum; n_edges_out[j] the
 * number of final forward edges (return_all=True); any of the last four pointers may be NULL. */
int sa_mea_batch(const sa_mea_job_t *jobs, int64_t n_jobs, int device, unsigned flags, sa_mea_pair_t **path_out,
                 int64_t *n_path_out, double *sum_out, int32_t *status_out, int32_t *n_edges_out, double *kernel_ms_out);
void sa_mea_release(void); /* returns the scratch sa_mea_batch and sa_batch_mea keep between calls */
/* The same step chained onto a finished batch (after sa_batch_run), as mea_alignment_from_signal_align
 * (mea_algorithm.py:323-341) chains it onto signalAlign's output: every read's aligned pairs are still in HBM, one wave
 * per read builds the posterior matrix and shortest_ref_per_event from them there (what get_mea_params_from_events does
 * with the event table; the posterior is the one the TSV prints, six decimals) and the path kernels follow; only the
 * paths come back.  path_out[j] holds (ref_idx = x, event_idx = y) in the coordinates of sa_pair_t.  One entry per job
 * of the batch in every output array. */
int sa_batch_mea(sa_batch_t *b, unsigned flags, sa_mea_pair_t **path_out, int64_t *n_path_out, double *sum_out,
                 int32_t *status_out, double *kernel_ms_out);
/* "%f" of prob_e7 / 1e7 read back as a double: the posterior_probability column of the event table */
double sa_mea_printed_posterior(int64_t prob_e7);
/* the same, evaluated by the GPU for prob_e7 = first .. first + n - 1 (test hook: host and device must agree) */
int sa_mea_printed_posterior_device(int64_t first, int64_t n, double *out, int device);
/* get_mea_params_from_events (mea_algorithm.py:267-320), host side, sparse: from the reference_index, event_index and
 * posterior_probability columns of an event table (any row order) to the COO entries and shortest_ref_per_event.
 * The outputs need room for n entries / (max event - min event + 1) events; returns the number of COO entries and the
 * number of events in *n_events_out, or a negative SA_E* code. */
int64_t sa_mea_params(const int64_t *reference_index, const int64_t *event_index, const double *posterior, int64_t n,
                      int32_t *event_idx_out, int32_t *ref_idx_out, double *posterior_out, int32_t *shortest_out,
                      int64_t *n_events_out);

/* ---- per-site variant / methylation calls over a read's posteriors ----------------------------------
 * Replaces MarginalizeFullVariants.get_data (src/signalalign/variantCaller.py:92-187) over the full TSV
 * (writePosteriorProbsFull), chained onto a finished batch like sa_batch_mea: the pairs are read where they lie in HBM and
 * only the calls cross PCIe.
 *   site      a k-mer index x whose LAST letter, ref[x + k - 1], is an ambiguity letter of the batch's map (the reference tests
 *             aligned_kmer[k - 1], :152-154)
 *   letters   the distinct options of that letter, sorted (sorted(variants)); a pair's letter is its path k-mer's last letter,
 *             the last digit of kmer_id
 *   units     per letter, the sum over the site's pairs of the posterior the TSV prints ("%f" of prob_e7 / 1e7) in integers of
 *             1e-6: exact and independent of the order of summation
 *   prob      units[l] / sum of units (:157-172), the same double on the device and on the host
 * A site is reported when its pairs print a non-zero total (the reference asserts on a zero one).  x is the pair's k-mer index;
 * the TSV's reference_index of it is the CLI's business (signalMachine --site-calls).
 * SA_FLAG_SITE_CALLS at sa_batch_create / _deferred: the batch records its sites (one host pass over each reference) and keeps
 * them until it is destroyed -- nothing of this without the flag.  With SA_FLAG_VC_ROWS: SA_EINVAL (that flag drops the rows
 * this step reads); an ambiguity letter at a site with more than SA_SITE_MAX_LETTERS distinct options, or a site in a
 * SA_FLAG_PAIRS8 batch: SA_EUNSUPPORTED. */
#define SA_FLAG_SITE_CALLS 128u
#define SA_SITE_MAX_LETTERS 8
typedef struct sa_site_call {
    int32_t x, n_letters;                  /* k-mer index of the site, number of its letters              */
    char letters[SA_SITE_MAX_LETTERS];     /* sorted; not terminated when there are 8                     */
    int64_t units[SA_SITE_MAX_LETTERS];    /* printed posterior summed per letter, in 1e-6               */
    double prob[SA_SITE_MAX_LETTERS];      /* units[l] / sum(units)                                       */
} sa_site_call_t;
/* After sa_batch_run (also after sa_batch_release_device, SA_FLAG_EXACT, on every kernel family and with HDP models):
 * calls_out[j] (malloc'd, sa_free) holds job j's n_out[j] calls in ascending x; one entry per job of the batch.
 * kernel_ms_out (may be NULL): HIP-event time of the kernels.  SA_ESTATE: created without SA_FLAG_SITE_CALLS, or not run.
 * Deterministic: the sums are integer atomics. */
int sa_batch_site_calls(sa_batch_t *b, unsigned flags, sa_site_call_t **calls_out, int64_t *n_out, double *kernel_ms_out);
/* The same calls from records the caller holds, through the same kernels: job j's records are first[j] .. first[j + 1) of x,
 * kmer_id and prob_e7, in sa_batch_pairs order.  Of a job only ref and ref_len are read; `ambig` is the map sa_batch_create takes
 * (NULL: no site anywhere).  Checked before the device is touched, SA_EINVAL: first[0] != 0 or first not monotone; x outside
 * [0, ref_len - k]; kmer_id outside [0, n_alpha^k); prob_e7 outside [0, 10^7]; a NULL array with records.  More than
 * SA_SITE_MAX_LETTERS options at a site: SA_EUNSUPPORTED, as at creation.  calls_out / n_out: n_jobs entries, as above. */
int sa_site_calls_records(const sa_model_t *m, const sa_job_t *jobs, int64_t n_jobs, const char *const *ambig,
                          const int64_t *first /* n_jobs + 1 */, const int32_t *x, const int32_t *kmer_id, const int64_t *prob_e7,
                          int device, sa_site_call_t **calls_out, int64_t *n_out, double *kernel_ms_out);

/* ---- Per-position marginals: single-nucleotide probabilities ------------------------------------------------------------
 * Replaces CallMethylation.call_methyls (src/signalalign/scripts/alignmentAnalysisLib.py:159-247) over one full TSV per job, in
 * target coordinates, chained onto a finished batch like sa_batch_site_calls.
 *   position  an index p of the job's `ref` that holds an ambiguity letter of the batch's map
 *   rows      every record with x <= p <= x + k - 1; its letter is digit p - x of its path k-mer (kmer_id, first letter most
 *             significant: the path k-mer as the TSV prints it)
 *   sum       per letter, the printed posterior of those rows ("%f" of prob_e7 / 1e7 read back as a double, i.e. units / 1e6)
 *             added serially in row order (sa_batch_pairs order, the TSV's), starting from 0
 *   prob      sum[l] / total, total = ((0 + sum[0]) + sum[1]) + ... over the sorted letters -- the reference's bits
 * One record per (job, position with at least one row), in ascending p.  A position whose rows all print 0.000000 (possible
 * only with a threshold below 5e-7) has total 0: the reference divides by zero there (alignmentAnalysisLib.py:230-233,
 * ZeroDivisionError); here the record is reported with its n_rows, sum all 0.0 and prob all 0.0, the site calls' rule for a
 * zero sum.
 * x_min_out / x_max_out (n_jobs entries each, may be NULL): the smallest and largest x of the job's records, -1 for a job
 * without records.
 * SA_FLAG_POSITION_CALLS at sa_batch_create / _deferred: the batch records its ambiguous positions (one host pass over each
 * reference).  With SA_FLAG_VC_ROWS: SA_EINVAL; with SA_FLAG_PAIRS8, or an ambiguity letter with more than SA_SITE_MAX_LETTERS
 * distinct options: SA_EUNSUPPORTED (both at creation).  The call: SA_ESTATE when created without the flag or not run.  Works
 * after sa_batch_release_device and with SA_FLAG_EXACT (the records go up again).  Deterministic: counts and bucket slots are
 * integer atomics, every bucket is put in row order before it is folded. */
#define SA_FLAG_POSITION_CALLS 256u
typedef struct sa_position_call {
    int32_t p, n_rows, n_letters, pad;     /* position in the job's ref, covering rows, number of letters             */
    char letters[SA_SITE_MAX_LETTERS];     /* sorted; not terminated when there are 8                                  */
    double sum[SA_SITE_MAX_LETTERS];       /* printed posterior summed per letter, in row order                       */
    double prob[SA_SITE_MAX_LETTERS];      /* sum[l] / total                                                          */
} sa_position_call_t;
int sa_batch_position_calls(sa_batch_t *b, unsigned flags, sa_position_call_t **calls_out, int64_t *n_out, int32_t *x_min_out,
                            int32_t *x_max_out, double *kernel_ms_out);
/* The same calls from records the caller holds, through the same kernels; the arguments and their checks are those of
 * sa_site_calls_records (x is a k-mer index: 0 <= x <= ref_len - k), the row order is the records' order within their job.
 * A model with k > 32: SA_EUNSUPPORTED, as at creation. */
int sa_position_calls_records(const sa_model_t *m, const sa_job_t *jobs, int64_t n_jobs, const char *const *ambig,
                              const int64_t *first /* n_jobs + 1 */, const int32_t *x, const int32_t *kmer_id, const int64_t *prob_e7,
                              int device, sa_position_call_t **calls_out, int64_t *n_out, int32_t *x_min_out, int32_t *x_max_out,
                              double *kernel_ms_out);

/* ---- host helpers of signalMachine --snp-step (singleNucleotideProbabilities.py:551-723) -------------------------------
 * sa_snp_substitute: the window of replace_periodic_sequence_positions (utils/sequenceTools.py:207-254).  ref[i] lies at contig
 * coordinate c0 + i, or c0 - i when `reversed`; out[i] = `letter` where that coordinate is = phase (mod step), else ref[i] in
 * upper case.  `out` needs len + 1 bytes (terminated).  step < 1 or phase outside [0, step): SA_EINVAL. */
int sa_snp_substitute(const char *ref, int64_t len, int64_t contig_pos_of_ref0, int reversed, int64_t step, int64_t phase,
                      char letter, char *out);
/* the sites of call_methyls with a step offset: [*lo_out, *hi_out) with lo = (min_ref_index - step) floored to a multiple of
 * step and hi = (max_ref_index + step) raised to one; the sites of phase s are lo + s, lo + s + step, ... below hi */
int sa_snp_site_window(int64_t min_ref_index, int64_t max_ref_index, int64_t step, int64_t *lo_out, int64_t *hi_out);
/* one line of a marginals file: position (the TSV's reference_index), strand 0 't' / 1 'c', the probabilities of A, C, G, T */
typedef struct sa_snp_site {
    int64_t pos;
    int32_t strand, pad;
    double p[4];
} sa_snp_site_t;
/* <read_id>.tsv as discover_single_nucleotide_probabilities writes it (singleNucleotideProbabilities.py:655-718): the header
 * (contig empty when n == 0; strand "complement" when `backward`), then the lines sorted stably by position, the probabilities
 * as Python's str(float), in T G C A order when `backward`.  `sites` holds the step files' lines one file after the other. */
int sa_snp_write_read(const char *path, const char *fast5_input, const char *read_id, const char *contig, int backward,
                      const sa_snp_site_t *sites, int64_t n);

/* ---- Single-nucleotide probabilities marginalised over reads ----------------------------------------------------------------
 * Replaces call_sites_with_marginal_probs / scan_for_proposals (src/signalalign/scripts/variantCallingLib.py:114-164, :226-271)
 * over the per-read files of --snp-step: an accumulator holds, per contig position, a forward sum and a backward sum of four
 * doubles (A, C, G, T) and a row count, in HBM across batches, as sa_kmer_table_t holds its rows.
 *   rows of a site   every (read, strand) line whose contig and position name it
 *   order            calls in call order; inside one call ascending run ordinal, within a run strand t before c, then the order
 *                    given.  A caller that adds reads in ascending run order gets "run order" over the whole table.
 *   sums             (fwd if direction else bwd)[l] += p[l], doubles added serially in that order, starting from the sums the
 *                    accumulator holds: add(A); add(B) is add(A + B), bit for bit
 *   direction        (read mapped forward and strand t) or (read mapped backward and strand c)
 *   marginal         m = [fwd[0] + bwd[3], fwd[1] + bwd[2], fwd[2] + bwd[1], fwd[3] + bwd[0]], total = ((m[0] + m[1]) + m[2]) + m[3],
 *                    prob[l] = m[l] / total, called = the first letter of largest prob
 * Two deliberate differences from the reference: its loader (load_variant_call_data) predates the contig column that
 * CallMethylation.write now puts first and would mix contigs, so sites are grouped by (contig, position) here; and the row order
 * is run order, not a directory listing's (the same difference as sa_kmer_table's).
 * step >= 1: sa_snp_marginals_add_batch drops the positions outside call_methyls' window (sa_snp_site_window over the
 * reference_index of every record of a group's jobs); step == 0: no window.  Storage is 76 bytes per contig position (sums,
 * counts and the working arrays of an add) and as much again from the first checkpoint on: SA_ENOMEM when it does not fit,
 * SA_ENODEVICE without a GPU.  One add call takes at most 2^30 rows (SA_EUNSUPPORTED).  An add that fails on the device after its
 * first kernel leaves the accumulator unusable: every later call on it but destroy returns SA_ESTATE. */
typedef struct sa_snp_marginals sa_snp_marginals_t;
typedef struct sa_snp_job_map {   /* job j of a batch, for sa_snp_marginals_add_batch */
    int32_t contig, pos_sign;     /* index p of the job's ref lies at contig position pos0 + pos_sign * p (pos_sign +1 or -1) */
    int64_t pos0;
    int64_t x0;                   /* a record's x has the TSV's reference_index x0 + x_sign * x (adjustReferenceCoordinate)  */
    int32_t x_sign, strand;       /* strand 0 't', 1 'c'                                                                     */
    int32_t direction, pad;       /* 1: forward sum, 0: backward sum                                                         */
    int64_t run;                  /* run ordinal of the read                                                                 */
    int64_t group;                /* jobs with the same id are the strands of one read's one step file: they share a window */
} sa_snp_job_map_t;
typedef struct sa_snp_marginal {
    int64_t pos;
    int32_t contig, depth;        /* depth: rows of the site                                                                 */
    double fwd[4], bwd[4], prob[4];
    double delta;                 /* max(prob) - prob[reference letter]; 0 without an A/C/G/T reference letter               */
    char called, ref;             /* called: 'N' when total == 0; ref: upper-cased, 'N' without ref_by_contig                */
    char is_proposal, pad[5];     /* reference letter in ACGT and != called (and total != 0)                                 */
} sa_snp_marginal_t;
int sa_snp_marginals_create(sa_snp_marginals_t **out, const int64_t *contig_lens, int64_t n_contigs, int64_t step, int device);
void sa_snp_marginals_destroy(sa_snp_marginals_t *t);
/* rows computed elsewhere for one read (`run` orders rows inside one call only; all rows here share it): sites[i].pos is a
 * position of `contig`, sites[i].strand 0 or 1.  A position outside the contig, a strand that is neither: SA_EINVAL, nothing added. */
int sa_snp_marginals_add_sites(sa_snp_marginals_t *t, int32_t contig, int64_t run, int direction, const sa_snp_site_t *sites, int64_t n);
/* chained onto a finished batch created with SA_FLAG_POSITION_CALLS: the position calls are folded on the device by the code of
 * sa_batch_position_calls, mapped by map[j] and added; no call crosses PCIe.  Rows are ordered by (run, strand, job).  Not run,
 * or created without the flag: SA_ESTATE.  A kept position outside its contig, a bad contig, sign or strand: SA_EINVAL and
 * nothing is added.  kernel_ms_out[0]: the shared position fold, kernel_ms_out[1]: what follows it (may be NULL). */
int sa_snp_marginals_add_batch(sa_snp_marginals_t *t, sa_batch_t *b, const sa_snp_job_map_t *map, int64_t n_jobs, double *kernel_ms_out);
/* the contract of sa_kmer_table_checkpoint / _rollback; rollback without a checkpoint: SA_ESTATE */
int sa_snp_marginals_checkpoint(sa_snp_marginals_t *t);
int sa_snp_marginals_rollback(sa_snp_marginals_t *t);
/* marginal, normalisation, called base and comparison with the reference letter on the device; the sites with at least one row
 * and at least min_depth of them come back in (contig, position) order (*sites_out malloc'd, sa_free).  ref_by_contig (may be
 * NULL: no proposals): one sequence per contig, of at least the contig's length.  The accumulator is left as it is. */
int sa_snp_marginals_finish(sa_snp_marginals_t *t, int64_t min_depth, const char *const *ref_by_contig, sa_snp_marginal_t **sites_out,
                            int64_t *n_out, double *kernel_ms_out);
/* ---- host helpers of the error-correction loop (scripts/jamison.py, variantCallingLib.py) ----
 * sa_snp_group_sites: group_sites_in_window (jamison.py:66-83).  The n sites are sorted by (pos, delta); a group grows while the
 * next site lies less than `window` after the previous one, and yields the position of its largest delta (the first of equals).
 * The reference's loop stops with one site left over, so a trailing site that would start a group of its own is lost:
 * keep_last == 0 restates that, keep_last != 0 keeps the site.  out needs n entries. */
int sa_snp_group_sites(const int64_t *pos, const double *delta, int64_t n, int64_t window, int keep_last, int64_t *out, int64_t *n_out);
/* sa_snp_substitute with an ascending list of contig positions instead of a period (make_degenerate_reference with positions) */
int sa_snp_substitute_sites(const char *ref, int64_t len, int64_t contig_pos_of_ref0, int reversed, const int64_t *sites,
                            int64_t n_sites, char letter, char *out);
/* `ref` (contig `contig`, position 0 first) with the called base of every proposal of that contig written in: what
 * call_sites_with_marginal_probs(get_sites=False) returns.  update_reference_with_marginal_probs passes get_sites=True and so
 * gets a site list where it wants the sequence -- a reference bug; this is the intent.  out needs len + 1 bytes. */
int sa_snp_apply_calls(const char *ref, int64_t len, const sa_snp_marginal_t *marginals, int64_t n, int32_t contig, char *out);
/* one line per site, "contig\tsite\tdepth\tpA\tpC\tpG\tpT\tcalled\tref\tdelta\n", the doubles as Python's str(float) */
int sa_snp_write_marginals(const char *path, const char *const *contig_names, const sa_snp_marginal_t *marginals, int64_t n);

/* ---- Per-position profile of all reads' posteriors -----------------------------------------------------------------------------
 * Replaces src/signalalign/scripts/multipleAlignmentAnalysis.py (:52-69 is_forward_alignment, :118-242 main) over the full TSV of
 * every read: an accumulator holds, per contig position, integer sums in HBM across batches, as sa_snp_marginals_t holds its sums.
 *   a record         (x, kmer_id, prob_e7) of job j names k-mer index x of the job's ref.  For i in [0, k) it contributes to index
 *                    p = x + i, which lies at contig position pos0 + pos_sign * p (:163-170); the letter is digit i of kmer_id,
 *                    first letter most significant, complemented when pos_sign == -1 (A <-> T, C <-> G, every other letter itself)
 *   a contribution   kmer_count += 1; units[letter] += the printed posterior in 1e-6 ("%f" of prob_e7 / 1e7);
 *                    entropy_units += sa_profile_entropy_term(units): shannon_entropy's summand (:99-104)
 *                    llrint((q log2 q + (1 - q) log2 (1 - q)) 2^40), q = units / 1e6, 0 at q = 0 and q = 1
 *   spans            a job with records covers every contig position from the smallest to the largest its records touch;
 *                    read_count is the number of such jobs (aligned_file_count, :194-201, one file being one 1-D job).  A covered
 *                    position that no record touches is reported with kmer_count 0, ref 0 and zeros (:198-200)
 *   finish           every position with read_count > 0 or kmer_count > 0 in (contig, position) order; prob[l] = units[l] / sum of
 *                    units (0 when the sum is 0: the script divides by zero there); entropy = ((double) entropy_units 2^-40 /
 *                    kmer_count) / -2.0, +0.0 when entropy_units == 0; ref the upper-cased reference letter where kmer_count > 0
 *                    ('N' with ref_by_contig NULL); *letters_seen_out has bit l set when a contribution named letter l of the
 *                    model's alphabet (all_characters).  The accumulator is left as it is.
 * Every add is an integer atomic, so the table holds the same bits whatever the order, in one call or in many.
 * Three deliberate differences from the script: the sums are integers, not floats in np.mean's pairwise order; orientation comes
 * from the map (the script guesses it from the first rows, which breaks on 2-D files and on a leading palindrome); ref comes from
 * the reference (the script takes it from the first row that names the position).  Contigs come in index order (the script sorts
 * their names), and 1 - q of the entropy term is taken as (1e6 - units) / 1e6, which makes the term symmetric to the bit.
 * Storage is 8 * (2 + letters of the alphabet) + 4 bytes per contig position (52 for ACGT), with one position more per contig, and
 * as much again from the first checkpoint on: SA_ENOMEM when it does not fit, SA_ENODEVICE without a GPU.  An alphabet of more than
 * SA_SITE_MAX_LETTERS letters, or with one of A, C, G, T but not its complement: SA_EUNSUPPORTED at create.
 * All checks run before anything is added, and a refused call adds nothing: a bad contig index, a pos_sign that is not +-1, a mapped
 * position outside its contig: SA_EINVAL.  A device failure after the first accumulating kernel leaves the table unusable: every
 * later call on it but destroy returns SA_ESTATE. */
typedef struct sa_position_profile sa_position_profile_t;
typedef struct sa_profile_job_map {   /* job j of a batch or of sa_position_profile_add_records */
    int32_t contig, pos_sign;         /* index p of the job's ref lies at contig position pos0 + pos_sign * p (pos_sign +1 or -1) */
    int64_t pos0;
} sa_profile_job_map_t;               /* 16 bytes */
typedef struct sa_profile_site {
    int64_t pos;
    int32_t contig, read_count;            /* reads (jobs) whose span covers pos                                        */
    int64_t kmer_count;                    /* (record, letter) contributions                                            */
    int64_t entropy_units;                 /* sum of the rows' terms, units of 2^-40                                    */
    int64_t units[SA_SITE_MAX_LETTERS];    /* printed posterior per letter of the model's alphabet, 1e-6                */
    double entropy, prob[SA_SITE_MAX_LETTERS];
    char ref, pad[7];                      /* 0: no row names this position                                             */
} sa_profile_site_t;                       /* 176 bytes */
#define SA_PROFILE_DIRECT 1u               /* every contribution is a global atomic: no LDS window (the fallback path, and the A/B) */
int sa_position_profile_create(sa_position_profile_t **out, const sa_model_t *m, const int64_t *contig_lens, int64_t n_contigs, int device);
void sa_position_profile_destroy(sa_position_profile_t *t);
/* chained onto a finished batch: its records are read where the run left them in HBM (after sa_batch_release_device, and with
 * SA_FLAG_EXACT, they go up again); map[j] places job j.  Not run: SA_ESTATE; a SA_FLAG_PAIRS8 batch (no k-mer in the record):
 * SA_EUNSUPPORTED; a SA_FLAG_VC_ROWS batch (rows dropped), another device, n_jobs that is not the batch's, a model whose k or
 * alphabet size differs from the table's: SA_EINVAL.  kernel_ms_out (may be NULL): HIP-event time of the call's kernels. */
int sa_position_profile_add_batch(sa_position_profile_t *t, sa_batch_t *b, const sa_profile_job_map_t *map, int64_t n_jobs, unsigned flags,
                                  double *kernel_ms_out);
/* records from elsewhere: job j's are first[j] .. first[j + 1) (first[0] == 0).  A kmer_id outside the model, a prob_e7 outside
 * [0, 1e7], an x outside [0, 2^28): SA_EINVAL, nothing added. */
int sa_position_profile_add_records(sa_position_profile_t *t, const sa_profile_job_map_t *map, int64_t n_jobs, const int64_t *first /* n_jobs + 1 */,
                                    const int32_t *x, const int32_t *kmer_id, const int64_t *prob_e7, unsigned flags, double *kernel_ms_out);
/* the contract of sa_kmer_table_checkpoint / _rollback (the table is copied); rollback without a checkpoint: SA_ESTATE */
int sa_position_profile_checkpoint(sa_position_profile_t *t);
int sa_position_profile_rollback(sa_position_profile_t *t);
/* the spans' difference array scanned, the sites made and compacted on the device (*sites_out malloc'd, sa_free).  ref_by_contig
 * (may be NULL): one sequence per contig, of at least the contig's length. */
int sa_position_profile_finish(sa_position_profile_t *t, const char *const *ref_by_contig, sa_profile_site_t **sites_out, int64_t *n_out,
                               uint32_t *letters_seen_out, double *kernel_ms_out);
/* the script's file (:203-242): the header "#contig\tposition\tref_char\tshannon_entropy\tkmer_aln_count\tread_aln_count" and
 * "\tp<letter>" for every seen letter in sorted order, then one line per site, the doubles as Python's str(float), ref_char empty
 * when 0.  Host only.  The script's histogram on stderr (qualify_entropies) is not reproduced. */
int sa_position_profile_write(const char *path, const char *alphabet, uint32_t letters_seen, const char *const *contig_names,
                              const sa_profile_site_t *sites, int64_t n);
int64_t sa_profile_entropy_term(int64_t units);   /* test hook, host */

/* ---- Device-wide sort of 64-bit keys ---------------------------------------------------------------------------------------------
 * sorted_out[0 .. n) = keys[0 .. n) ascending (host arrays; the test hook of the sort that sa_call_scores_finish runs on arrays in
 * HBM): a least-significant-digit radix sort with 8-bit digits over tiles of SA_SORT_TILE keys; a digit in which all keys agree costs
 * no pass.  n < 0 or a NULL array with n > 0: SA_EINVAL; then SA_ENODEVICE without a GPU; n above 2^31 - 1: SA_EUNSUPPORTED; n == 0
 * succeeds and writes nothing.  kernel_ms_out (may be NULL): HIP-event time from the first kernel to the last. */
#define SA_SORT_TILE 4096
int sa_sort_u64(const uint64_t *keys, int64_t n, uint64_t *sorted_out, int device, double *kernel_ms_out);

/* ---- Site calls scored against known truth: AUC, ROC, confusion ------------------------------------------------------------------
 * Replaces the numbers of visualization/plot_variant_accuracy.py:44-175 over AggregateOverReadsFull.generate_labels / generate_labels2
 * (src/signalalign/variantCaller.py:413-442): an accumulator holds, in HBM across batches, append-only arrays of scores, one per
 * (level, read strand t / c, letter, class), and finish sorts them and counts.
 *   level      0 per site per read, 1 per read (the mean of a read strand's site probabilities), 2 per genomic site
 *   score      the probability of one letter, a double in [0, 1], kept as its bit pattern (non-negative doubles order as unsigned
 *              integers; -0.0 is stored as +0.0).  A call of n letters gives n scores: the true letter's to that letter's positive
 *              array, every other to its letter's negative array
 *   truth      a positions table (CustomAmbiguityPositions.parseAmbiguityFile, utils/sequenceTools.py:587-600) looked up by (contig,
 *              position, mapped strand) -- get_true_character's match of strand == forward_mapped; the first line of several that
 *              name one key wins (.values[0]) -- or one letter per read (generate_labels2)
 *   row        one per (level, strand group 0 t / 1 c / 2 both, letter) with at least one score, in that order:
 *              auc2 = sum over positives p of [2 #(negatives < p) + #(negatives == p)], the trapezoid area under the ROC curve over
 *              the distinct thresholds in units of 1 / (2 n_pos n_neg); auc = (double) auc2 / (2.0 n_pos n_neg), NaN when a count
 *              is 0; tp, fp = positives, negatives >= threshold, fn, tn the rest; and on the grid t_k = (double) k / (double) n_bins,
 *              k = 0 .. n_bins, tp_ge[k], fp_ge[k] = positives, negatives >= t_k.  The group of both strands is the union: its auc2
 *              has the cross terms (template positives against complement negatives and the reverse)
 * Every number is an integer count or one division of two integers: exact, independent of arrival order.  Two deliberate
 * differences from the script: no average precision (a floating-point sum over all thresholds, with no exact form), and the curve
 * is on a fixed grid, not at every distinct threshold.
 * An array grows through the caching allocator by doubling; one add takes at most 2^30 scores and an array at most 2^31 - 1
 * (SA_EUNSUPPORTED; for sa_call_scores_add_batch the bound is on the batch's sites, before they are labelled).  A device failure
 * after the first appending kernel leaves the accumulator unusable: every later call on it but destroy returns SA_ESTATE. */
typedef struct sa_call_scores sa_call_scores_t;
typedef struct sa_truth_site {        /* one line of the positions file */
    int32_t contig, mapped_strand;    /* mapped_strand 0 '+', 1 '-'; contig in [0, 2^21)                                           */
    int64_t pos;                      /* in [0, 2^41)                                                                              */
    char change_to, pad[7];           /* a letter of the accumulator's letters                                                     */
} sa_truth_site_t;                    /* 24 bytes */
typedef struct sa_score_job_map {     /* job j of a batch, for sa_call_scores_add_batch */
    int32_t contig, x_sign;           /* a site's x has the TSV's reference_index x0 + x_sign * x (x_sign +1 or -1)                */
    int64_t x0;
    int32_t strand, mapped_strand;    /* read strand 0 't', 1 'c'; mapped strand 0 '+', 1 '-'                                      */
    int32_t true_letter, pad;         /* index into letters: the read's label; -1: look every site up in the positions table       */
} sa_score_job_map_t;                 /* 32 bytes */
typedef struct sa_call_score_row {
    int32_t level, group;             /* group 0 template, 1 complement, 2 both                                                    */
    char letter, pad[7];
    int64_t n_pos, n_neg;
    uint64_t auc2;
    double auc;
    int64_t tp, fp, tn, fn;
} sa_call_score_row_t;                /* 80 bytes */
typedef struct sa_call_scores_counts {
    int64_t unlabelled;               /* calls dropped because the positions table does not name them (generate_labels drops them) */
    int64_t other_sites;              /* sites skipped because their letters are not the accumulator's                            */
} sa_call_scores_counts_t;
/* letters: 2 .. SA_SITE_MAX_LETTERS distinct characters in ascending order; n_bins >= 1; threshold not NaN; truth (may be NULL with
 * n_truth == 0) is copied, sorted and kept on the device.  SA_EINVAL otherwise, and for a truth line with a letter outside
 * `letters`, a strand that is neither, a contig or position outside the ranges above; then SA_ENODEVICE without a GPU. */
int sa_call_scores_create(sa_call_scores_t **out, const char *letters, int32_t n_bins, double threshold, const sa_truth_site_t *truth,
                          int64_t n_truth, int device);
void sa_call_scores_destroy(sa_call_scores_t *s);
/* chained onto a finished batch created with SA_FLAG_SITE_CALLS: the accumulate-and-normalise half of sa_batch_site_calls runs (the
 * same launches), a kernel labels every site with a non-zero total, and no call crosses PCIe.  Level 0: every site of every job.
 * Level 1: only jobs with true_letter >= 0 -- one lane per (job, letter) adds the site probabilities serially, in ascending
 * reference_index when the mapped strand is '+' and descending when '-' (variantCaller.py:141-144, :172-178), and divides by the
 * number of sites.  Not run, or created without the flag: SA_ESTATE.  n_jobs that is not the batch's, another device, a negative
 * contig, an x_sign that is not +-1, a strand or mapped strand that is neither, a true_letter outside [-1, letters): SA_EINVAL,
 * checked before anything is appended.  kernel_ms_out (may be NULL): HIP-event time of the call's kernels. */
int sa_call_scores_add_batch(sa_call_scores_t *s, sa_batch_t *b, const sa_score_job_map_t *map, int64_t n_jobs, double *kernel_ms_out);
/* scores made elsewhere: record i has prob[i * n_letters + l] for letter l and the true letter true_letter[i] (an index).  A level
 * outside 0..2, a strand outside 0..1, a letter index outside the letters, a NaN or a value outside [0, 1]: SA_EINVAL, nothing added. */
int sa_call_scores_add_records(sa_call_scores_t *s, int32_t level, int32_t strand, const double *prob, const int8_t *true_letter, int64_t n);
/* checkpoint records the arrays' lengths and the counts, rollback truncates to them: nothing is copied.  Rollback without a
 * checkpoint: SA_ESTATE */
int sa_call_scores_checkpoint(sa_call_scores_t *s);
int sa_call_scores_rollback(sa_call_scores_t *s);
/* the arrays sorted into scratch (the accumulator is left as it is) and every count made on the device by binary search.
 * *rows_out: the rows; *curves_out: per row tp_ge[n_bins + 1] then fp_ge[n_bins + 1] (both malloc'd, sa_free; curves_out and
 * counts_out may be NULL).  kernel_ms_out (may be NULL): HIP-event time from the first sort to the last count. */
int sa_call_scores_finish(sa_call_scores_t *s, sa_call_score_row_t **rows_out, int64_t *n_rows_out, int64_t **curves_out,
                          sa_call_scores_counts_t *counts_out, double *kernel_ms_out);
/* summary_path: "level\tstrand\tletter\tn_pos\tn_neg\tauc\ttp\tfp\ttn\tfn\taccuracy\tprecision\trecall" and one line per row (strand
 * t, c or all), accuracy = (tp + tn) / (n_pos + n_neg), precision = tp / (tp + fp), recall = tp / n_pos, each one division of two
 * integers, "nan" for 0 / 0, the doubles as Python's str(float).  curves_path (may be NULL; needs curves):
 * "level\tstrand\tletter\tk\tthreshold\ttp_ge\tfp_ge\ttpr\tfpr\tprecision" and n_bins + 1 lines per row.  Host only. */
int sa_call_scores_write(const char *summary_path, const char *curves_path, int32_t n_bins, const sa_call_score_row_t *rows,
                         int64_t n_rows, const int64_t *curves);

/* ---- Deviation of every read's alignment from its guide ------------------------------------------------------------------------
 * Replaces validateSignalAlignment.py over the embedded full table of every read: analyze_event_skips
 * (src/signalalign/visualization/plot_labelled_read.py:364-472), the histogram of absolute differences
 * (validateSignalAlignment.py:178-192) and flag_large_gaps (:103-142), from the records a batch leaves in HBM.  All of it in the
 * job's own coordinates (sa_pair_t): x the k-mer index in the job's ref, y the event index, the job's anchors the guide.
 *   best_x[y]     of the records with event index y the x of the one with the largest prob_e7, among equal prob_e7 the largest x; an
 *                 event with a record is ALIGNED
 *   guide[y]      anchor_x of the anchor with anchor_y == y; else (a + b) / 2 in integer division of the last anchor before and the
 *                 first anchor after y, or the one of the two that exists
 *   diff, abs     best_x[y] - guide[y] and its absolute value, of aligned events
 *   on the path   the MEA path handed in for the job holds a pair with that event_idx (its position is not looked at)
 *   histogram     bucket min(abs / bucket_size, n_buckets - 1), once per aligned event
 *   sets          the maximal runs of aligned events, in ascending y, with abs > threshold; events without records are skipped and
 *                 end no run.  Per set the first and last event, the count, the largest abs (peak), the largest abs among its events
 *                 on the path (mea_peak, 0 without one) and center_event = (sum of its y) / count in integer division
 *   per job       status 0, SA_DEV_NO_GUIDE (no anchors: every count 0) or SA_DEV_NO_RECORDS (anchors and no record); max_event is
 *                 the smallest y that attains max_abs (0 without aligned events)
 * Three deliberate differences from the script: ties between equal posteriors go to the largest x (the script leaves them to row
 * order; here the choice is an integer atomic maximum); a set still open when the read ends is reported, with open_end = 1 (the
 * script's loop closes a set only on the next unflagged event and drops it: a caller who wants the script's list drops those
 * sets); events are named by y (the script's EVENT_INDEX ranks raw starts of three tables of the fast5).
 * Everything is an integer, so the outputs do not depend on launch shape or order, and SA_DEV_WINDOW gives the same bits.
 * All argument checks run before any device work: threshold < 0, bucket_size < 1, n_buckets outside [1, 1024], an anchor_y that is
 * not strictly increasing or outside [0, 2^31), an anchor_x outside [0, 2^28), n_events outside [0, 2^28], a record or an MEA event
 * outside [0, n_events), a record's x outside [0, 2^28), a prob_e7 outside [0, 1e7]: SA_EINVAL.  More than 2^31 - 1 events in one
 * call: SA_EUNSUPPORTED.  Without a GPU: SA_ENODEVICE. */
#define SA_DEV_NO_GUIDE 1
#define SA_DEV_NO_RECORDS 2
#define SA_DEV_DIRECT 1u   /* every record is a global atomic maximum: no LDS window.  The default: on a batch of 2000 reads of 5000
                            * events the window did not beat it (profiles/guide_deviation.json), so the flag only names it */
#define SA_DEV_EVENTS 2u   /* *events_out: one sa_deviation_event_t per event of every job */
#define SA_DEV_WINDOW 4u   /* the records' maxima go through a window in LDS first (the A/B of SA_DEV_DIRECT; not together with it) */
#define SA_DEV_MAX_BUCKETS 1024
typedef struct sa_deviation_params { int32_t threshold, bucket_size, n_buckets; } sa_deviation_params_t;   /* NULL: {10, 5, 64} */
typedef struct sa_deviation_job { const int64_t *anchor_x, *anchor_y; int64_t n_anchors, n_events; } sa_deviation_job_t;
typedef struct sa_deviation_read { int32_t status, n_sets; int64_t set_first; int64_t n_aligned, n_flagged, n_on_mea, sum_abs;
                                   int32_t max_abs, max_abs_mea, max_event, pad; } sa_deviation_read_t;   /* 64 bytes */
typedef struct sa_deviation_set { int32_t first_event, last_event, count, peak, mea_peak, center_event, open_end, pad; } sa_deviation_set_t;
typedef struct sa_deviation_event { int32_t best_x, guide, diff; uint32_t flags; } sa_deviation_event_t;  /* bit 0 aligned, 1 on MEA, 2 flagged */
/* Outputs of both calls: reads_out[n_jobs]; *sets_out (malloc'd, sa_free) all jobs' sets back to back, job j's n_sets from
 * set_first on, *n_sets_out of them; hist_out[n_jobs * n_buckets] and total_hist_out[n_buckets] (the sum of the rows), either may
 * be NULL; with SA_DEV_EVENTS *events_out (malloc'd, sa_free), the events of every job back to back in job order, an unaligned
 * event all zeros (without the flag events_out may be NULL and is not touched); kernel_ms_out (may be NULL) the HIP-event time of
 * the call's kernels.  mea_path / n_mea: per job its MEA path (sa_batch_mea's), or both NULL: no event is on a path.
 * Chained onto a finished batch: the records are read where the run left them (16-byte and SA_FLAG_PAIRS8 records alike; after
 * sa_batch_release_device, and with SA_FLAG_EXACT, they go up again).  jobs[j] carries the batch's own anchors and n_events.  Not
 * run: SA_ESTATE; a SA_FLAG_VC_ROWS batch (rows dropped), n_jobs that is not the batch's, an n_events that differs: SA_EINVAL. */
int sa_batch_guide_deviation(sa_batch_t *b, const sa_deviation_job_t *jobs, int64_t n_jobs, const sa_mea_pair_t *const *mea_path,
                             const int64_t *n_mea, const sa_deviation_params_t *p, unsigned flags, sa_deviation_read_t *reads_out,
                             sa_deviation_set_t **sets_out, int64_t *n_sets_out, int32_t *hist_out, int64_t *total_hist_out,
                             sa_deviation_event_t **events_out, double *kernel_ms_out);
/* records from elsewhere: job j's are first[j] .. first[j + 1) (first[0] == 0) of x, y, prob_e7 */
int sa_guide_deviation_records(const sa_deviation_job_t *jobs, int64_t n_jobs, const int64_t *first /* n_jobs + 1 */, const int32_t *x,
                               const int32_t *y, const int64_t *prob_e7, const sa_mea_pair_t *const *mea_path, const int64_t *n_mea,
                               const sa_deviation_params_t *p, int device, unsigned flags, sa_deviation_read_t *reads_out,
                               sa_deviation_set_t **sets_out, int64_t *n_sets_out, int32_t *hist_out, int64_t *total_hist_out,
                               sa_deviation_event_t **events_out, double *kernel_ms_out);
void sa_guide_deviation_release(void); /* returns the scratch the two calls keep between calls */

/* ---- Labelled signal: reference position, k-mer and posterior of every stretch of raw current ------------------------------------
 * Replaces, over the records a batch leaves in HBM and the raw starts of a raw read (sa_raw_npread_t), what alignedsignal.py and
 * mea_algorithm.py build per read from the tables embedded in a fast5: CreateLabels.add_mea_labels through
 * match_events_with_signalalign, add_signal_align_predictions through create_label_from_events, fix_sa_reference_indexes,
 * match_ref_position_with_raw_start_band and AlignedSignal.generate_label_mapping.  All coordinates are the job's own (sa_pair_t):
 * x the k-mer index in the job's ref, y the event index.
 *   reference_index  ref_first + ref_step * x + base_shift: the reference_index the TSV prints for x (affine, step +1 or -1), moved
 *                    to the labelled base of the k-mer as fix_sa_reference_indexes does (base_shift)
 *   prob_units       sa_printed_units(prob_e7): the posterior the TSV prints, in units of 1e-6
 *   MEA set          SA_LABEL_MEA: one segment per pair of the job's MEA path, in path order (ascending y).  The record is the one at
 *                    cell (x, y); of several records of the cell the one with the lowest prob_e7, among equals the earliest in
 *                    sa_batch_pairs order (the row signalMachine's MEA output prints).  raw_start / raw_length are the job's at y.
 *                    A pair whose cell holds no record yields no segment and is counted in mea_without_record.
 *   full set         SA_LABEL_FULL: one segment per record, ordered by raw_start as np.sort(kind='mergesort') orders them:
 *                    raw_start strictly increases with y, so by y, equal y in sa_batch_pairs order
 *   bands            SA_LABEL_BANDS: one entry per x with a record, in ascending x: raw_start that of the smallest y among the
 *                    records of x, raw_length = raw_start[y_max] - raw_start[y_min] + raw_length[y_max], n_records their number
 *   per-sample map   SA_LABEL_SAMPLES (needs SA_LABEL_MEA): per sample t of the job the index i, within the job's MEA segments, of
 *                    the segment with start_i <= t < start_(i+1) -- for the last segment start <= t < start + length -- and -1 for
 *                    every other sample: a gap left by unmapped events belongs to the segment before it
 *   per job          status 0, SA_LABEL_NO_RECORDS, or (with SA_LABEL_MEA) SA_LABEL_NO_PATH: the path is NULL or empty, the full
 *                    set and the bands are still made, the MEA set is empty and every sample is -1.  Of each set the first entry
 *                    in the call's back-to-back array and the count (sample_first / n_samples: the job's part of the map, also
 *                    when it is not made).  Over the MEA segments: minus_strand = the first one's reference_index >= the last's
 *                    (check_strand_mapping; 0 without segments); n_positions = 1 + the consecutive segments whose x differ (the
 *                    distinct x of a monotone path); skipped_positions = the sum over consecutive segments of max(|dx| - 1, 0);
 *                    stay_events = the consecutive segments with dx == 0; first_sample = the first segment's raw_start,
 *                    end_sample = the last one's raw_start + raw_length, labelled_samples = their difference (the samples of the
 *                    map that are not -1); all 0 without segments.
 * Deliberate differences from the scripts: the bands are made for every position with a record (the script makes them for the
 * positions of a variant table only); a tie of posteriors within a cell goes to the earliest record (the script keeps what its sort
 * leaves); the k-mer is a kmer_id, spelled in full by the caller (the script's S5 field cuts a 6-mer to five letters).
 * Everything is an integer, so the outputs do not depend on launch shape or order and compare exactly.
 * All argument checks run before any device work, SA_EINVAL: a NULL array; n_events that differs from the batch's or lies outside
 * [0, 2^28]; a raw_start that is negative or not strictly increasing; raw_length < 1; raw_start + raw_length > n_samples; ref_step
 * other than +1 / -1; an MEA event or a record's y outside [0, n_events); an MEA path whose events do not strictly increase; an x
 * outside [0, 2^28); a prob_e7 outside [0, 1e7]; SA_LABEL_SAMPLES without SA_LABEL_MEA; an unknown flag.  More than 2^31 - 1 samples,
 * records, events or x slots (the sum over the jobs of x_max - x_min + 1, for the bands) in one call: SA_EUNSUPPORTED.  Without a GPU:
 * SA_ENODEVICE. */
#define SA_LABEL_NO_RECORDS 1
#define SA_LABEL_NO_PATH 2
#define SA_LABEL_MEA 1u
#define SA_LABEL_FULL 2u
#define SA_LABEL_BANDS 4u
#define SA_LABEL_SAMPLES 8u
#define SA_LABEL_TIMES 16u            /* a HIP event pair around every kernel: sa_signal_labels_last_kernel_ms (probes/signal_labels_rate.py) */
#define SA_LABEL_SAMPLE_TILE 4096     /* samples of one read that a block of the per-sample fill writes */
/* the kernels in launch order, as sa_signal_labels_last_kernel_ms numbers them */
#define SA_LABEL_K_COUNT 0
#define SA_LABEL_K_SCAN_EVENTS 1
#define SA_LABEL_K_SCATTER 2
#define SA_LABEL_K_ORDER 3
#define SA_LABEL_K_FULL 4
#define SA_LABEL_K_FIND 5
#define SA_LABEL_K_SCAN_PATH 6
#define SA_LABEL_K_BAND_ACC 7
#define SA_LABEL_K_SCAN_BANDS 8
#define SA_LABEL_K_JOB_SCAN 9
#define SA_LABEL_K_MEA_EMIT 10
#define SA_LABEL_K_BAND_EMIT 11
#define SA_LABEL_K_READS 12
#define SA_LABEL_K_FILL 13
#define SA_LABEL_N_KERNELS 14
typedef struct sa_label_job {
    const int64_t *raw_start, *raw_length;  /* per event y of the job: the rows of sa_raw_npread_t */
    int64_t n_events, n_samples;
    int64_t ref_first; int32_t ref_step;    /* the reference_index the TSV prints for x: ref_first + ref_step * x */
    int32_t base_shift;                     /* fix_sa_reference_indexes: added to every reference_index */
} sa_label_job_t;
typedef struct sa_label_segment { int64_t raw_start, raw_length, reference_index; int32_t x, y, kmer_id, prob_units; } sa_label_segment_t; /* 40 bytes */
typedef struct sa_label_band { int64_t raw_start, raw_length, reference_index; int32_t x, n_records; } sa_label_band_t;                 /* 32 bytes */
typedef struct sa_label_read { int32_t status, minus_strand; int64_t mea_first, n_mea, full_first, n_full, band_first, n_bands,
                               sample_first, n_samples, mea_without_record, n_positions, skipped_positions, stay_events,
                               labelled_samples, first_sample, end_sample; } sa_label_read_t;   /* 128 bytes */
/* Outputs of both calls: reads_out[n_jobs]; with its flag *mea_out, *full_out, *bands_out (malloc'd, sa_free): all jobs' entries
 * back to back, job j's n_mea / n_full / n_bands from mea_first / full_first / band_first on; with SA_LABEL_SAMPLES *samples_out
 * (malloc'd, sa_free): all jobs' samples back to back, job j's n_samples from sample_first on.  Without its flag a pointer may be
 * NULL and is not touched, and the set's counts are 0 (the full set's excepted: they are the job's records).  kernel_ms_out (may be
 * NULL): the HIP-event time of the call's kernels.  mea_path / n_mea: per job its MEA path (sa_batch_mea's), or both NULL.
 * Chained onto a finished batch: the records are read where the run left them (after sa_batch_release_device, and with
 * SA_FLAG_EXACT, they go up again).  Not run, a SA_FLAG_PAIRS8 batch (no k-mer in the record) or a SA_FLAG_VC_ROWS batch (rows
 * dropped): SA_ESTATE, as sa_batch_mea answers; n_jobs that is not the batch's: SA_EINVAL. */
int sa_batch_signal_labels(sa_batch_t *b, const sa_label_job_t *jobs, int64_t n_jobs, const sa_mea_pair_t *const *mea_path,
                           const int64_t *n_mea, unsigned flags, sa_label_read_t *reads_out, sa_label_segment_t **mea_out,
                           sa_label_segment_t **full_out, sa_label_band_t **bands_out, int32_t **samples_out, double *kernel_ms_out);
/* records from elsewhere: job j's are first[j] .. first[j + 1) (first[0] == 0) of x, y, kmer_id, prob_e7, in sa_batch_pairs order */
int sa_signal_labels_records(const sa_label_job_t *jobs, int64_t n_jobs, const int64_t *first /* n_jobs + 1 */, const int32_t *x,
                             const int32_t *y, const int32_t *kmer_id, const int64_t *prob_e7, const sa_mea_pair_t *const *mea_path,
                             const int64_t *n_mea, int device, unsigned flags, sa_label_read_t *reads_out, sa_label_segment_t **mea_out,
                             sa_label_segment_t **full_out, sa_label_band_t **bands_out, int32_t **samples_out, double *kernel_ms_out);
void sa_signal_labels_release(void); /* returns the scratch the two calls keep between calls */
/* The HIP-event time of each kernel of the process's last call with SA_LABEL_TIMES, out[SA_LABEL_K_*] (0 for a kernel that call did
 * not launch); at most n entries are written; returns SA_LABEL_N_KERNELS. */
int sa_signal_labels_last_kernel_ms(double *out, int32_t n);

/* ---- Call quality: call accuracy against the alignment's distance from its guide, and the breaks of the MEA path -------------------
 * Replaces visualization/plot_accuracy_vs_alignment_deviation.py (get_distance_from_guide_alignment, alignedsignal.py:388-425, over
 * match_ref_position_with_raw_start_band, :428-443, then true_false = data[label] > threshold) and
 * visualization/plot_breaks_in_alignments.py (find_gaps_in_alignment_data, :139-148, len(mea_data), percent_correct), from what a
 * finished SA_FLAG_SITE_CALLS batch leaves in HBM.  All of it in the job's own coordinates (sa_pair_t): x the k-mer index in the
 * job's ref, y the event index, the job's anchors the guide.  Everything is an integer but the one comparison of a probability.
 *   calls         the sites of the batch's site fold, labelled exactly as sa_call_scores_add_batch labels them, with the letters,
 *                 the threshold and the positions table of the sa_call_scores_t handed in and one sa_score_job_map_t per job
 *                 (true_letter >= 0 labels the whole read, -1 looks (contig, x0 + x_sign * x, mapped_strand) up).  A site with a
 *                 non-zero total whose kind has other letters counts in n_other_sites, one the table does not name in n_unlabelled;
 *                 neither goes further.  correct = prob[true_letter] > threshold (strict)
 *   band          SA_LABEL_BANDS' rule: over the records with the call's x, y_min and y_max; raw_start = raw_start[y_min],
 *                 raw_length = raw_start[y_max] - raw_start[y_min] + raw_length[y_max]; mid2 = 2 * raw_start + raw_length, twice the
 *                 script's v_position_middle
 *   guide row     the anchor with anchor_x == x (of several the first for x_sign +1, the last for -1: the one the script's walk in
 *                 ascending reference_index meets first); else for x_sign +1 the last anchor with anchor_x < x, for x_sign -1 the
 *                 first anchor with anchor_x > x.  A call is OUTSIDE the guide when that row does not exist (the script's iloc[-1]
 *                 wraps to the last row) or when no anchor has a reference_index at or beyond the call's (the script leaves NaN): it
 *                 counts in n_outside, has guide_event -1 and delta2 0, enters no histogram and no sum, and is still a call with its
 *                 correct flag.  Every call of a job without anchors is outside
 *   delta2        mid2 - 2 * guide_mid, twice the script's guide_delta; guide_mid = np.round(raw_start[ay] + raw_length[ay] / 2) in
 *                 integers: raw_start + raw_length / 2 for an even raw_length, else the even one of the two neighbours
 *   histogram     bin = floor((delta2 - 2 * bin_lo) / (2 * bin_width)) (a floor, not C's truncation); slot 0 is underflow
 *                 (delta2 < 2 * bin_lo), slot n_bins + 1 overflow, slot bin + 1 otherwise; hist[slot * 2 + correct], once per inside
 *                 call: (n_bins + 2) * 2 counts per job and summed over the call
 *   gaps          over consecutive pairs i - 1, i of the job's MEA path (ascending event order):
 *                 gap = raw_start[y_i] - (raw_start[y_(i-1)] + raw_length[y_(i-1)]), reported when gap > min_gap (strict)
 *   per job       status, bits: SA_CQ_NO_GUIDE (no anchors), SA_CQ_NO_SITES (no site with a non-zero total), SA_CQ_NO_PATH (the path
 *                 is NULL or empty).  n_calls counts the labelled calls, inside or outside.  sum_abs_delta2 and max_abs_delta2 are
 *                 over the inside calls; max_x is the smallest x that attains the maximum, -1 without an inside call.  The script's
 *                 accuracy and gap ratio are one division each, left to the caller: n_correct / n_calls, n_gaps / n_path
 * Deliberate differences from the scripts: every call finds its guide row on its own (the script advances one guide row per call, so
 * of two calls that share a gap between guide rows the second is measured against a later row); outside calls are named, not wrapped
 * or NaN; the accuracy-against-delta curve of 20 linspace bins is not made, the fixed-grid histogram of correct and wrong calls
 * carries it; sites are looked up in a positions table (the script labels a whole sample); the band is over the records of x (the
 * script makes it over the variant-caller rows of the position).
 * All argument checks run before any device work, SA_EINVAL: a NULL array; n_jobs that is not the batch's; n_events that differs
 * from the batch's or lies outside [0, 2^28]; a raw_start that is negative or not strictly increasing; raw_length < 1; anchors whose
 * anchor_y do not strictly increase or whose anchor_x decrease, an anchor_x outside [0, 2^28), an anchor_y outside [0, n_events); an
 * MEA event outside [0, n_events) or a path whose events do not strictly increase; bin_width < 1, bin_lo or bin_width beyond 2^40 in
 * magnitude, n_bins outside [1, SA_CQ_MAX_BINS], min_gap < 0; a map entry sa_call_scores_add_batch refuses; another device than the
 * accumulator's; an unknown flag.  sa_call_quality_records only: site_x not strictly ascending within a job or outside [0, 2^28); a
 * site_prob that is NaN or outside [0, 1]; a record's x outside [0, 2^28) or y outside [0, n_events); a site with no record of its
 * x.  A batch not run or created without SA_FLAG_SITE_CALLS: SA_ESTATE.  More than 2^31 - 1 sites, records, events or path pairs in
 * one call, or a raw_start + raw_length beyond 2^31 - 1: SA_EUNSUPPORTED.  Without a GPU: SA_ENODEVICE. */
#define SA_CQ_NO_GUIDE 1
#define SA_CQ_NO_SITES 2
#define SA_CQ_NO_PATH 4
#define SA_CQ_CALLS 1u          /* *calls_out: one sa_callq_call_t per labelled call */
#define SA_CQ_BAND_DIRECT 2u    /* every record is a global atomic pair into its site's y_min / y_max: no window in LDS.  The A/B of the
                                 * default, which first combines the records of a tile per site in LDS and won beyond the spread of
                                 * three calls on a site batch of 28 records per site (profiles/call_quality.json); same bytes */
#define SA_CQ_MAX_BINS 1024
typedef struct sa_callq_params { int64_t bin_lo, bin_width; int32_t n_bins, min_gap; } sa_callq_params_t;  /* NULL: {-10000, 100, 200, 30} */
typedef struct sa_callq_job { const int64_t *anchor_x, *anchor_y; int64_t n_anchors;
                              const int64_t *raw_start, *raw_length; int64_t n_events; } sa_callq_job_t;
typedef struct sa_callq_read { int32_t status, max_x; int64_t n_calls, n_correct, n_unlabelled, n_other_sites, n_outside, sum_abs_delta2,
                               max_abs_delta2, n_path, n_gaps, sum_gap, max_gap, call_first, gap_first; } sa_callq_read_t;   /* 112 bytes */
typedef struct sa_callq_call { int64_t raw_start, raw_length, delta2; double prob_true;   /* the band; prob_true the double the site fold holds */
                               int32_t x, guide_event, true_letter, correct, outside, pad; } sa_callq_call_t;               /* 56 bytes */
typedef struct sa_callq_gap  { int32_t y_before, y_after; int64_t gap; } sa_callq_gap_t;
/* Outputs of both calls: reads_out[n_jobs]; with SA_CQ_CALLS *calls_out (malloc'd, sa_free) all jobs' calls back to back, job j's
 * n_calls from call_first on in ascending x, *n_calls_out of them (without the flag both may be NULL and are not touched, and
 * call_first is 0); *gaps_out (malloc'd, sa_free) all jobs' gaps back to back in path order, job j's n_gaps from gap_first on,
 * *n_gaps_out of them; hist_out[n_jobs * (n_bins + 2) * 2] (may be NULL) and total_hist_out[(n_bins + 2) * 2] (the sum of the rows,
 * may be NULL); kernel_ms_out (may be NULL) the HIP-event time of the call's kernels, the site fold's among them.  mea_path / n_mea:
 * per job its MEA path (sa_batch_mea's; a job's may be NULL with n_mea 0), or both NULL.
 * `s` is only read -- its letters, threshold, positions table and device: nothing is appended to it, and sa_call_scores_finish
 * afterwards gives the rows it would have given.  Chained onto a finished batch the call runs the site fold itself, as
 * sa_call_scores_add_batch does, and reads the records where the run left them (after sa_batch_release_device, and with
 * SA_FLAG_EXACT, they go up again); jobs[j] carries the batch's own anchors and n_events and the raw read's starts and lengths. */
int sa_batch_call_quality(sa_call_scores_t *s, sa_batch_t *b, const sa_score_job_map_t *map, const sa_callq_job_t *jobs, int64_t n_jobs,
                          const sa_mea_pair_t *const *mea_path, const int64_t *n_mea, const sa_callq_params_t *p, unsigned flags,
                          sa_callq_read_t *reads_out, sa_callq_call_t **calls_out, int64_t *n_calls_out, sa_callq_gap_t **gaps_out,
                          int64_t *n_gaps_out, int64_t *hist_out, int64_t *total_hist_out, double *kernel_ms_out);
/* sites and records from elsewhere: job j's sites are site_first[j] .. site_first[j + 1) (site_first[0] == 0) of site_x, ascending,
 * with site_prob[i * n_letters + l] for letter l of the accumulator's letters; site_other (may be NULL) marks with a non-zero byte
 * the sites of other letters; job j's records are rec_first[j] .. rec_first[j + 1) of rec_x, rec_y.  Every site counts as one with a
 * non-zero total. */
int sa_call_quality_records(sa_call_scores_t *s, const sa_score_job_map_t *map, const sa_callq_job_t *jobs, int64_t n_jobs,
                            const int64_t *site_first /* n_jobs + 1 */, const int32_t *site_x, const double *site_prob,
                            const uint8_t *site_other, const int64_t *rec_first /* n_jobs + 1 */, const int32_t *rec_x,
                            const int32_t *rec_y, const sa_mea_pair_t *const *mea_path, const int64_t *n_mea, const sa_callq_params_t *p,
                            unsigned flags, sa_callq_read_t *reads_out, sa_callq_call_t **calls_out, int64_t *n_calls_out,
                            sa_callq_gap_t **gaps_out, int64_t *n_gaps_out, int64_t *hist_out, int64_t *total_hist_out,
                            double *kernel_ms_out);
void sa_call_quality_release(void); /* returns the scratch the two calls keep between calls */
/* The HIP-event time of the process's last call's kernels: out[0] k_cq_band, [1] k_cq_calls (both passes), [2] k_cq_gaps (both
 * passes) and the scans; at most n entries are written; returns 3. */
int sa_call_quality_last_kernel_ms(double *out, int32_t n);

/* ---- Gaussian k-mer emission training (trainModels.train_normal_emmissions, src/signalalign/train/trainModels.py:735-828)
 * A k-mer table keeps, per strand (0 = template 't', 1 = complement 'c') and path k-mer (kmer_id), the `max_per_kmer` rows of
 * largest printed posterior among the rows whose printed posterior is >= min_prob -- generate_top_n_kmers_from_sa_output
 * (build_alignments.py:76-275) over the assignments rows (kmer, strand, descaled, prob) -- in HBM across batches.
 *   printed   both values as the -s 2 file prints them, "%f": integers of 1e-6 (descaled: the CLI's descale() of the event mean
 *             and the path k-mer's level mean in the table of the model the table was created with, no fused multiply-add)
 *   ties      the row earlier in run order wins: batches and add_rows calls in call order, jobs in order, a job's rows in
 *             sa_batch_pairs order (the reference's order comes from a directory listing: the one deliberate difference)
 * sa_kmer_table_add_batch reads a finished batch's records where the run left them in HBM (16- or 8-byte ones); after
 * sa_batch_release_device, and with SA_FLAG_EXACT (host-finalised pairs), the records are first copied up again, all of them; `jobs` / `n_jobs` are the batch's own (event means, scalings and, for
 * 8-byte records, the references).  SA_FLAG_VC_ROWS batch: SA_EINVAL; not run: SA_ESTATE; a descaled value of magnitude
 * 2147.483648 or more (beyond +-2^31 units) or not finite, from a batch or in sa_kmer_table_add_rows: SA_EUNSUPPORTED.  max_per_kmer < 1 or min_prob outside [0, 1]: SA_EINVAL. */
typedef struct sa_kmer_table sa_kmer_table_t;
typedef struct sa_kmer_row {
    int64_t descaled_units;   /* "%f" of the descaled mean in 1e-6                                        */
    int64_t run;              /* run ordinal of the row                                                    */
    int32_t kmer_id, prob_units;
    int32_t neg_zero;         /* 1: the descaled value printed as "-0.000000"                             */
    int32_t pad;
} sa_kmer_row_t;
typedef struct sa_kmer_stat {
    int64_t n;                /* rows of the k-mer in the table (0: the k-mer is not trained)              */
    double m, s;              /* mean and population sd, or (use_median) median and MAD / ndtri(0.75)     */
} sa_kmer_stat_t;
int sa_kmer_table_create(sa_kmer_table_t **out, const sa_model_t *m, int64_t max_per_kmer, double min_prob, int device);
void sa_kmer_table_destroy(sa_kmer_table_t *t);
int sa_kmer_table_add_batch(sa_kmer_table_t *t, sa_batch_t *b, const sa_job_t *jobs, int64_t n_jobs, int strand, double *kernel_ms_out);
/* rows read back from assignments files (parsed "%f" values; strand as above) */
int sa_kmer_table_add_rows(sa_kmer_table_t *t, int strand, const int32_t *kmer_ids, const double *descaled, const double *prob, int64_t n);
/* the table's rows of a strand, k-mer ascending, posterior descending, then run order; *rows_out malloc'd (sa_free) */
int sa_kmer_table_rows(const sa_kmer_table_t *t, int strand, sa_kmer_row_t **rows_out, int64_t *n_out);
/* the rows as the table file prints them, "kmer\tstrand\tdescaled\tprob\n": strand 0 or 1, or -1 for both (t, then c); append
 * != 0 adds them to the end of an existing file */
int sa_kmer_table_write(const sa_kmer_table_t *t, int strand, const char *path, int append);
/* The table as it is now becomes the state sa_kmer_table_rollback returns to (rows and run ordinals): for a caller that may
 * have to add a slice of reads again (signalMachine --batch drops reads a batch's planner refuses and runs the rest again).
 * The arrays a strand had at the checkpoint are kept until the next checkpoint or destroy, not copied.  Rollback without a
 * checkpoint: SA_ESTATE. */
int sa_kmer_table_checkpoint(sa_kmer_table_t *t);
int sa_kmer_table_rollback(sa_kmer_table_t *t);
/* The table from the rows that cover labelled positions only -- trainModels.py:161-286 (generate_build_alignments_positions,
 * build_alignments_positions, get_kmers_covering_positions, filter_top_n_kmers, write_and_generate_build_alignments_positions)
 * without the full TSVs: a row with the TSV's reference_index ri on contig c covers the positions line (c, p, S) when
 * p - (k - 1) <= ri <= p (k the model's k-mer length; the same window for both site strands, as the reference has it) and S is the
 * site strand the reference pairs with the row: '+' for the t rows of a forward-mapped read and the c rows of a backward-mapped
 * one, '-' for the other two.  A row is OFFERED when its printed posterior is >= min_prob and it covers at least one line; the
 * offered rows go through the table's selection as every row does without positions (per strand and path k-mer, ties by run
 * order; a row's run ordinal counts every record of the run, offered or not).  Two deliberate differences from the script: it
 * pools t and c rows in filter_top_n_kmers, the table keeps them apart; its tie order comes from a directory listing and an
 * unstable sort, here it is run order.
 * Coverage counts: per distinct line (contig, position, strand) the number of offered rows that cover it over the whole run; a
 * row within k - 1 of two lines counts once for each.  Integers, independent of arrival order.
 * sa_kmer_table_set_positions: the lines are copied, sorted, deduplicated and kept on the table's device as packed 64-bit keys.
 * Only on an empty table (SA_ESTATE otherwise); n == 0 keeps nothing (and then nothing is ever offered); a strand that is neither,
 * a contig outside [0, 2^21), a position outside [0, 2^41): SA_EINVAL.  From then on sa_kmer_table_add_batch and
 * sa_kmer_table_add_rows return SA_ESTATE (they carry no coordinates) and sa_kmer_table_add_batch_at is the way in; on a table
 * without positions sa_kmer_table_add_batch_at returns SA_ESTATE.
 * sa_kmer_table_add_batch_at: sa_kmer_table_add_batch with map[j] placing job j.  One kernel sets a bit per reference position of
 * every job (one search of the keys each), the selection's passes test that bit, and one pass over the records adds the offered
 * ones to the counts.  n_jobs that is not the batch's, a contig outside the range, an x_sign that is not +-1, a site strand that is
 * neither, |x0| >= 2^42: SA_EINVAL, checked before anything is added.
 * sa_kmer_table_position_counts: the distinct lines in (contig, strand, position) order and their counts, both malloc'd
 * (sa_free); *n_out of them.  sa_kmer_table_checkpoint / _rollback cover the counts. */
typedef struct sa_train_site {        /* one line of the positions file (its first three columns) */
    int32_t contig, mapped_strand;    /* the ranges of sa_truth_site_t: mapped_strand 0 '+', 1 '-'; contig in [0, 2^21)            */
    int64_t pos;                      /* in [0, 2^41)                                                                              */
} sa_train_site_t;                    /* 16 bytes */
typedef struct sa_train_job_map {     /* job j of a batch, for sa_kmer_table_add_batch_at */
    int32_t contig, x_sign;           /* a record at x has the TSV's reference_index x0 + x_sign * x (x_sign +1 or -1)             */
    int64_t x0;
    int32_t site_strand, pad;         /* the site strand S its rows pair with, 0 '+', 1 '-'                                        */
} sa_train_job_map_t;                 /* 24 bytes */
int sa_kmer_table_set_positions(sa_kmer_table_t *t, const sa_train_site_t *sites, int64_t n);
int sa_kmer_table_add_batch_at(sa_kmer_table_t *t, sa_batch_t *b, const sa_job_t *jobs, int64_t n_jobs, int strand,
                               const sa_train_job_map_t *map, double *kernel_ms_out);
int sa_kmer_table_position_counts(const sa_kmer_table_t *t, sa_train_site_t **sites_out, int64_t **counts_out, int64_t *n_out);
/* HIP-event times of the last sa_kmer_table_add_batch_at: ms_out[0] the cover mask's kernel, ms_out[1] the counts pass (both are
 * part of that call's kernel_ms_out) */
int sa_kmer_table_add_at_times(const sa_kmer_table_t *t, double ms_out[2]);
/* per k-mer (out: one entry per kmer_id) statistics over the table's rows, computed exactly on the device: mean = the double
 * nearest S / (n 1e6), sd = sqrt of the double nearest (n Q - S^2) / (n^2 1e12); median and MAD exact in half / quarter units,
 * MAD converted and divided by 0.6744897501960817 (scipy's scale='normal') */
int sa_kmer_table_stats(const sa_kmer_table_t *t, int strand, int use_median, sa_kmer_stat_t *out, double *kernel_ms_out);
/* The M-step and HmmModel.write (hiddenMarkovModel.py:304-336), host only: the prior model file as written, and for every k-mer
 * with stats[id].n > 0 (and, with mod_only, a letter outside ACGT; with kmer_mask, mask[id] != 0)
 *   mean = (m n + mean0 w) / (n + w), sd = max((s n + sd0 w) / (n + w), min_sd), noise_lambda = mean^3 / sd^2
 * (set_kmer_event_mean_params, :900-909: the lambda is overwritten, a reference quirk kept on purpose).  Every number is
 * printed as Python's str(float). */
int sa_model_write_trained(const char *prior_model_path, const sa_kmer_stat_t *stats, double weight, double min_sd, int mod_only,
                           const uint8_t *kmer_mask, const char *out_path);
/* ---- Gaussian mixtures over a k-mer's rows (src/signalalign/mixture_model.py:42-186) ---------------------------------------
 * fit_model_to_kmer_dist / get_nanopore_gauss_mixture: a K-component Gaussian mixture (scalar variances) fitted by EM to
 * x_i = descaled_units_i / 1e6 over the rows of one (strand, k-mer), the rows in sa_kmer_table_rows order.  It is sklearn's
 * GaussianMixture.fit with n_init = 1 (max_iter 100, tol 1e-3, reg_covar 1e-6 are its defaults) from a deterministic start
 * instead of a random k-means draw:
 *   start    labels min(K - 1, floor(K (x_i - lo) / (hi - lo))) (lo / hi the k-mer's smallest / largest x; all 0 when equal),
 *            one M-step on the one-hot responsibilities; or, with `init`, the caller's weights, means and sds as they are
 *   M-step   nk_c = sum_i r_ic + 10 DBL_EPSILON, mean_c = sum r_ic x_i / nk_c, var_c = sum r_ic (x_i - mean_c)^2 / nk_c + reg_covar,
 *            weight_c = nk_c / sum_c nk_c
 *   E-step   lp_ic = -(log 2 pi + ((x_i - mean_c) / sd_c)^2) / 2 - log sd_c + log weight_c, norm_i = logsumexp_c lp_ic,
 *            r_ic = exp(lp_ic - norm_i), lower_bound = sum_i norm_i / n
 *   loop     lb = -inf; for it = 1 .. max_iter: prev = lb, E-step, M-step, stop (converged) when |lb - prev| < tol
 * The whole loop runs on the device, one work-group per job, in fp64.  A fit depends on the table's contents only, not on
 * how the table was filled: equal tables give equal bits.  A job is a k-mer id; the same list may be fitted for several K in
 * successive calls (AIC / BIC from lower_bound and n: 3K - 1 free parameters).
 * n_components outside 1..4, max_iter < 1, tol < 0 or not finite, reg_covar < 0 or not finite, a k-mer id outside the model,
 * an initial weight or sd that is not finite and positive, an initial mean that is not finite: SA_EINVAL. */
typedef struct sa_mixture_params { int32_t n_components, max_iter; double tol, reg_covar; } sa_mixture_params_t;
typedef struct sa_mixture_fit {
    int64_t n;                /* rows of the k-mer                                                           */
    int32_t kmer_id, n_iter, converged, status;   /* status 0 fitted, 1 fewer rows than components (the fields below are zero) */
    double lower_bound;       /* mean log-likelihood per row at the last E-step                              */
    double weight[4], mean[4], sd[4];             /* components in initialisation order                       */
} sa_mixture_fit_t;
/* kmer_ids NULL: every k-mer of the model (out: n_kmers entries).  init NULL, or n_jobs x 3K doubles (per job K weights, K means, K sds). */
int sa_kmer_table_mixture(const sa_kmer_table_t *t, int strand, const int32_t *kmer_ids, int64_t n_jobs,
                          const sa_mixture_params_t *p, const double *init, sa_mixture_fit_t *out, double *kernel_ms_out);
/* the start the call above makes for itself when init is NULL, in init's layout (a job with fewer rows than components: zeros);
 * handed back as init it gives the same fit, bit for bit */
int sa_kmer_table_mixture_start(const sa_kmer_table_t *t, int strand, const int32_t *kmer_ids, int64_t n_jobs,
                                const sa_mixture_params_t *p, double *init_out);
/* closest_to_canonical (mixture_model.py:92-104) of a fitted two-component mixture: *match_out the component whose mean is
 * nearest canonical_mean (strict < against an initial 1000, the first minimal index: component 0 and distance 1000 when
 * neither is nearer than that), *other_out the other one.  A fit with status != 0: SA_EINVAL.  Host only. */
int sa_mixture_assign(const sa_mixture_fit_t *fit, double canonical_mean, int32_t *match_out, int32_t *other_out, double *distance_out);
/* get_motif_kmer_pairs (mixture_model.py:189-200) over get_motif_kmers (utils/sequenceTools.py:332-374): the (canonical,
 * modified) k-mer pairs of every window of k letters over the motif's modified position, flanks from `alphabet` (NULL: "ATGC",
 * the reference's default).  The canonical k-mer has the first occurrence of the new letter replaced.  *pairs_out (sa_free):
 * *n_out pairs, sorted and without duplicates, each 2 (k + 1) bytes: the canonical k-mer, NUL, the modified k-mer, NUL.
 * Motifs of unequal length or not differing in exactly one letter, a canonical motif with a letter outside ACGT, k outside
 * 1..16: SA_EINVAL.  Host only. */
int sa_motif_kmer_pairs(int k, const char *canonical_motif, const char *modified_motif, const char *alphabet, char **pairs_out,
                        int64_t *n_out);
/* ---- Gaussian kernel density estimate over a k-mer's rows (plot_kmer_distribution, src/signalalign/hiddenMarkovModel.py:654-773)
 * KernelDensity(kernel="gaussian", bandwidth=h).score_samples (sklearn's default rtol = atol = 0) over x_i = descaled_units_i / 1e6,
 * the n rows of one (strand, k-mer), at any set of query points (not necessarily a linspace, nor sorted):
 *   log_density(q) = logsumexp_i(-((q - x_i) / h)^2 / 2) - log n - log h - log(2 pi) / 2
 * evaluated in fp64 on the device as: r = 1 / h; z_i = (q - x_i) r; e_i = -0.5 (z_i z_i); E = max_i e_i (the nearest row);
 * S = sum of exp(e_i - E) over the rows with e_i - E >= -64; (E + log S) - ((log n + log h) + log(2 pi) / 2).
 *   order   S is one accumulator per query point starting at 0.0, the rows added in ascending order of descaled_units (equal
 *           units give equal terms).  The value for one (k-mer, q, h) depends on the table's contents only -- not on the other
 *           jobs or points of the call, on chunking, or on how the table was filled: equal tables give equal bits
 *   cut     rows more than 64 below the largest exponent are not added: less than n exp(-64) < 7e-19 of a sum that is >= 1
 *   finite  E is taken out before exp: finite for every q for which ((q - x_i) / h)^2 does not overflow
 * kmer_ids NULL: every k-mer of the model (n_jobs is not read; out: n_kmers rows).  log_density_out: n_jobs x n_x doubles in ordinary
 * host memory, moved in chunks through the library's device scratch.  A k-mer without rows: n_rows_out 0 and a row of -INFINITY.
 * Checked before any device use -- SA_EINVAL: NULL t / x / log_density_out, strand outside 0..1, n_jobs < 0, n_x < 1, a bandwidth
 * that is not finite or <= 0, a non-finite x, a k-mer id outside the model; n_jobs == 0 succeeds and writes nothing.  A k-mer
 * with 2^32 rows or more: SA_EUNSUPPORTED.  kernel_ms_out (may be NULL): HIP-event time of the gather, sort and KDE kernels. */
int sa_kmer_table_kde(const sa_kmer_table_t *t, int strand, const int32_t *kmer_ids, int64_t n_jobs, const double *x, int64_t n_x,
                      double bandwidth, double *log_density_out /* n_jobs x n_x */, int64_t *n_rows_out /* n_jobs, may be NULL */,
                      double *kernel_ms_out /* may be NULL */);
/* Python's repr of a double (shortest round-trip digits); `out` needs 32 bytes; returns the length (test hook and writer) */
int sa_format_py_repr(char *out, double v);
/* the device's "%f" rounding of v[0 .. n) into units of 1e-6 and the negative-zero flag (test hook: must equal the host's,
 * sa_f6_units); returns SA_EUNSUPPORTED in rc_out[i] for a value outside +-2^31 */
int sa_f6_units_device(const double *v, int64_t n, int64_t *units_out, int32_t *neg_zero_out, int32_t *rc_out, int device);
int sa_f6_units(double v, int64_t *units_out, int32_t *neg_zero_out);

/* Plans a whole batch on the host (no GPU needed) with `threads` planner threads (0 = as sa_batch_create would) and
 * returns aggregate geometry plus a 64-bit FNV-1a digest over every array that would be uploaded.  The digest must
 * not depend on the number of threads: the CPU test-suite checks exactly that. */
int sa_plan_digest(const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs, int64_t n_jobs,
                   const char *const *ambig256, unsigned flags, int threads, sa_plan_info_t *info, uint64_t *digest);

/* ---- host-side helpers that signalMachine needs around the seam --------------------------------- */
/* signalUtils_guideAlignmentToRebasedAnchorPairs (impl/signalMachineUtils.c:142-164). op types:
 * 0 = match, 1 = reference-only (PAIRWISE_INDEL_X), 2 = read-only (PAIRWISE_INDEL_Y). */
int64_t sa_guide_to_anchors(int64_t start1, int64_t end1, int strand1, int64_t start2, const int32_t *op_type,
                            const int64_t *op_len, int64_t n_ops, int64_t trim, int64_t *ax, int64_t *ay,
                            int64_t cap);
/* signalUtils_getRemappedAnchorPairs (impl/signalMachineUtils.c:166-170) */
int64_t sa_remap_anchors(const int64_t *ax, const int64_t *ay, int64_t n, const int64_t *event_map,
                         int64_t map_offset, int64_t *ox, int64_t *oy);
/* signalUtils_estimateNanoporeParams (impl/signalMachineUtils.c:186-225): events (4 doubles each) are
 * drift-corrected in place, table5 noise columns rescaled; out7 = scale shift var drift scale_sd var_sd shift_sd */
int sa_estimate_params(const sa_model_t *m, double *table5_inout, const int64_t *strand_event_map, double *events4,
                       int64_t n_events, const char *strand_read, int64_t read_len, double *out7);

/* ---- guide alignment: a basecalled read against its reference window (what the reference's driver asks bwa mem for,
 * src/signalalign/signalAlignment.py:262-305) ------------------------------------------------------------------------------
 * Local alignment with affine gaps inside a Suzuki-Kasahara adaptive band, integer scores, one wave per read on the GPU.  The
 * rules (band geometry, steering, recurrence, tie-breaks, end cell, traceback) are written down in DESIGN.md and restated in
 * tests/guide_ref.py; the device's answer equals that restatement bit for bit.  Operation types are sa_guide_to_anchors':
 * 0 match, 1 reference-only, 2 read-only -- a result goes straight into sa_guide_to_anchors. */
typedef struct sa_guide_job {
    const char *read;  int64_t read_len;   /* nucleotides, any case */
    const char *ref;   int64_t ref_len;    /* the window, already in the orientation the read is aligned in */
    int64_t diag;                          /* reference index that read base 0 is expected at (sa_guide_seed); 0: window starts at the read */
} sa_guide_job_t;
typedef struct sa_guide_params {
    int32_t match, mismatch;               /* scores of a pair of equal / different letters of ACGT (2, -4) */
    int32_t gap_open, gap_extend;          /* a gap of length L costs gap_open + L * gap_extend (4, 2) */
    int32_t ambiguous;                     /* score of any letter outside ACGT against anything (-1) */
    int32_t band;                          /* cells per anti-diagonal: 64, 128, 192 or 256 (128) */
    double min_read_fraction;              /* SA_GUIDE_SHORT unless the aligned read span reaches this share of the read (0.5) */
} sa_guide_params_t;
#define SA_GUIDE_NO_ALIGNMENT 1            /* no positive-scoring alignment: zero operations */
#define SA_GUIDE_SHORT 2                   /* aligned read span < min_read_fraction * read_len */
#define SA_GUIDE_BAND_EDGE 4               /* the path touched the first or last band offset: it may be clipped by the band (a warning) */
#define SA_GUIDE_EMPTY 8                   /* read_len == 0 or ref_len == 0 */
#define SA_GUIDE_TRACE 16                  /* the traceback left the band or the job's bands: the operations are not to be used */
typedef struct sa_guide_result {
    int32_t status;                        /* 0 or SA_GUIDE_* bits */
    int64_t score, read_start, read_end, ref_start, ref_end;   /* half-open, in the job's coordinates */
    int64_t op_first, n_ops;               /* run-length operations, read order, in the arrays below */
} sa_guide_result_t;
/* params NULL: the defaults above.  diag is clamped to [0, ref_len].  *op_type_out / *op_len_out (malloc'd, sa_free) hold every
 * job's operations back to back.  SA_EINVAL (checked before any device use): a NULL array, n_jobs < 0, a length above 2^24, a band
 * that is no multiple of 64 in 64..256, a score beyond +-1000, gap_extend < 1, gap_open < 0; then SA_ENODEVICE without a GPU (there
 * is no CPU fallback).  The batch is cut into slices whose trace (band / 2 bytes per anti-diagonal) fits the device's free memory;
 * SA_ENOMEM when one job's does not.  kernel_ms_out (may be NULL): HIP-event time of the kernels. */
int sa_guide_align_batch(const sa_guide_job_t *jobs, int64_t n_jobs, const sa_guide_params_t *params, int device, unsigned flags,
                         sa_guide_result_t *results_out, int32_t **op_type_out, int64_t **op_len_out, double *kernel_ms_out);
/* sa_guide_align_batch keeps its device and pinned-host scratch between calls (grow only); this returns it */
void sa_guide_release(void);
/* Places a read inside a window that is longer than the band can absorb (host only).  Exact 15-mer matches between the read's
 * first 2000 bases and the window (with try_both_strands also its reverse complement) vote on the diagonal (window index minus
 * read index) in bins of 32; *diag_out is the median diagonal of the votes in the modal bin and its two neighbours, *reverse_out
 * 1 when the reverse complement got more votes, *votes_out those votes, *hits_out all 15-mer hits of that strand.  Fewer than 8
 * votes: no seed -- *diag_out = 0, *reverse_out = 0, and the return value is 1 (0 with a seed; SA_EINVAL for a NULL argument).
 * The diagonal of a reversed seed counts in the reverse-complemented window.  The caller crops the window to band / 2 before
 * the diagonal. */
int sa_guide_seed(const char *read, int64_t read_len, const char *window, int64_t window_len, int try_both_strands,
                  int64_t *diag_out, int *reverse_out, int64_t *votes_out, int64_t *hits_out);
/* The exonerate line of a guide alignment as the reference's driver writes it (src/signalalign/__init__.py:25-64):
 *   cigar: <label> <qstart> <qend> + <contig> <rstart> <rend> <+|-> <score> (M|D|I n)*
 * ref_start / ref_end are contig coordinates of the aligned interval on the forward strand; on the minus strand the line carries
 * them swapped (start > end) and the operations stay in read order.  Returns the length written (without the NUL), or the length
 * needed when cap is too small (nothing is written then); SA_EINVAL for a NULL argument or an unknown operation. */
int64_t sa_guide_format_cigar(const char *label, int64_t read_start, int64_t read_end, const char *contig, int64_t ref_start,
                              int64_t ref_end, int forward, int64_t score, const int32_t *op_type, const int64_t *op_len,
                              int64_t n_ops, char *out, int64_t cap);

/* ---- locating a read in a whole reference (what `bwa mem` finds for the reference's driver before it aligns: the locus) --------
 * A 15-mer index over every contig of a reference, resident on the GPU, and a batch kernel that votes each read's contig, strand
 * and diagonal out of it; sa_locate_window turns an answer into the window that sa_guide_seed / sa_guide_align_batch take.  The
 * index layout and the rules are written down in DESIGN.md ("Locating a read in a whole reference") and restated in
 * tests/locate_ref.py; the library's index equals that restatement's bit for bit, the device's answer field for field.
 *
 * The index: contigs concatenated in the order given, positions global int32.  Every position whose 15 letters are all of ACGT
 * (either case) and lie inside one contig gives an entry (code, pos), the code 2 bits per base, first base highest (sa_guide_seed's
 * encoding); entries sorted by (code, pos); a prefix table of 2^q + 1 offsets over the top q bits of the 30-bit code, q even, the
 * smallest with 2^q >= n_entries, clamped to [16, 26].  Built on the host (a stable LSD radix sort), uploaded once, resident until
 * sa_ref_index_destroy.  device < 0: built and kept on the host only.  SA_EINVAL: a NULL pointer, n_contigs == 0, a negative
 * length; SA_EUNSUPPORTED: 2^31 - 2^16 bases or more in all (checked on the lengths, before a sequence is read). */
typedef struct sa_ref_index sa_ref_index_t;
int sa_ref_index_build(sa_ref_index_t **out, const char *const *names, const char *const *seqs, const int64_t *lens,
                       int64_t n_contigs, int device);
/* every record of a FASTA in file order (a name ends at the first white space); SA_EIO when it cannot be read */
int sa_ref_index_build_fasta(sa_ref_index_t **out, const char *fasta_path, int device);
typedef struct sa_ref_index_info {
    int64_t n_contigs, total_bases, n_entries;
    int32_t q, device;                     /* table bits; the device the index lives on, -1 host only */
    int64_t host_bytes, device_bytes;      /* of the four arrays below */
    double build_seconds;                  /* host time of the build, the upload included */
} sa_ref_index_info_t;
int sa_ref_index_info(const sa_ref_index_t *idx, sa_ref_index_info_t *info);
/* views of the host arrays, valid until the index is destroyed: n_entries codes and positions, 2^q + 1 offsets,
 * n_contigs + 1 contig starts (the last one the total); any pointer may be NULL */
int sa_ref_index_entries(const sa_ref_index_t *idx, const uint32_t **codes, const int32_t **pos, const int32_t **table,
                         const int64_t **contig_start);
int sa_ref_index_contig(const sa_ref_index_t *idx, int64_t i, const char **name, int64_t *start, int64_t *len);
void sa_ref_index_destroy(sa_ref_index_t *idx);

typedef struct sa_locate_params {
    int32_t read_bases;                    /* seeds come from the read's first read_bases bases: 15..2048 (2000) */
    int32_t max_occ;                       /* a seed with more occurrences on a strand gives no hit there: 1..65536 (32) */
    int32_t span;                          /* width of the vote's window of keys: 1..8192 (128) */
    int32_t min_votes;                     /* SA_LOCATE_NONE below: >= 1 (8) */
    int32_t max_hits;                      /* hits kept per strand: a power of two in 1024..8192 (8192) */
} sa_locate_params_t;
#define SA_LOCATE_NONE 1                   /* votes < min_votes: contig -1, pos 0 */
#define SA_LOCATE_AMBIGUOUS 2              /* located, but 4 * second_votes >= 3 * votes: another locus is nearly as good (a warning) */
#define SA_LOCATE_OVERFLOW 4               /* a strand had more than max_hits hits: the later ones did not vote (a warning) */
#define SA_LOCATE_EMPTY 8                  /* read_len < 15: every other field 0, contig -1 */
typedef struct sa_locate_result {
    int32_t status, contig, reverse;
    int64_t pos;                           /* contig coordinate at which read base 0 is expected (may be < 0 or >= the contig's length);
                                              on the reverse strand read base i is expected at pos - i */
    int64_t key;                           /* the voted key, global: r - p forward, r + p reverse (r entry position, p seed position) */
    int64_t votes, second_votes;           /* keys in [keys[best], + span); the best count clear of that window */
    int64_t hits, seeds, repetitive;       /* kept hits of the chosen strand; the read's seeds; seeds above max_occ on that strand */
} sa_locate_result_t;
/* One workgroup per read.  params NULL: the defaults above.  SA_EINVAL (checked before any device use): a NULL array or read,
 * n_reads < 0, a read length above 2^24 or below 0, a parameter outside its range; then SA_ENODEVICE without a GPU or for an index
 * built with device < 0 (there is no CPU fallback).  The work happens on the index's device.  kernel_ms_out (may be NULL):
 * HIP-event time of the kernel. */
int sa_guide_locate_batch(const sa_ref_index_t *idx, const char *const *reads, const int64_t *read_lens, int64_t n_reads,
                          const sa_locate_params_t *params, unsigned flags, sa_locate_result_t *out, double *kernel_ms_out);
/* sa_guide_locate_batch keeps its device and pinned-host scratch between calls (grow only); this returns it */
void sa_locate_release(void);
/* The window to hand to the guide stage, [*start, *end) in the contig's coordinates, clipped to the contig: forward
 * [pos - band, pos + read_len + read_len / 4 + band), reverse the mirror [pos + 1 - read_len - read_len / 4 - band, pos + 1 + band).
 * SA_EINVAL: a NULL pointer, a result without a contig (SA_LOCATE_NONE, SA_LOCATE_EMPTY), read_len or band < 0, or a window that
 * the clipping leaves empty. */
int sa_locate_window(const sa_ref_index_t *idx, const sa_locate_result_t *r, int64_t read_len, int32_t band, int64_t *start,
                     int64_t *end);

/* ---- HDP rebuild, the deterministic pieces --------------------------------------------------------
 * The state of a serialised NanoporeHDP as the reference's Gibbs sampler leaves it, and what is computed FROM a state without
 * random numbers.  The sampling sweep itself (sample_dp_factors / gibbs_factor_iteration, impl/hdp.c:2110-2260, rand()-driven)
 * is not part of this library.
 *   sa_hdp_state_load / _write   deserialize_nhdp + deserialize_hdp / serialize_nhdp + serialize_hdp
 *                                (impl/nanopore_hdp.c:1077-1115, impl/hdp.c:2868-3322): host code; a file the reference wrote
 *                                goes through load + write byte for byte
 *   sa_hdp_state_distr_sample    take_distr_sample (impl/hdp.c:2067-2092): what ONE sample of the state adds to every observed
 *                                DP's collector -- the posterior predictive of every base factor on the sampling grid
 *                                (evaluate_posterior_predictive :530-562), the prior's (evaluate_prior_predictive :564-585),
 *                                mixed with the weights of cache_base_factor_weight / cache_prior_contribution (:2001-2044).
 *                                Grid evaluation and mixing run on the GPU (observed DPs x grid points x factors).
 *   sa_hdp_finalize_distributions  finalize_distributions (impl/hdp.c:2551-2584): collector / samples, then the slopes of the
 *                                natural cubic spline through it (spline_knot_slopes, impl/hdp_math_utils.c:402-442), one DP
 *                                per GPU thread, the reference's elimination order (bit-identical slopes for the densities of a
 *                                file the reference wrote).
 * Errors: SA_EIO (unreadable / malformed file), SA_ESTATE (a state without data has no factors), SA_ENODEVICE, SA_ENOMEM. */
typedef struct sa_hdp_state sa_hdp_state_t;
typedef struct sa_hdp_state_info {
    int64_t num_dps, depth, grid_length, n_data, n_factors, n_base_factors, n_observed, base_dp, alphabet_size, kmer_length;
    double mu, nu, alpha, beta, grid_start, grid_stop;
    int splines_finalized, has_data, sample_gamma;
    /* views into the state (valid until sa_hdp_state_free) */
    const double *data;                 /* n_data                                                        */
    const int64_t *data_dp;             /* n_data: the leaf DP of every data point                       */
    const double *gamma;                /* depth: concentration by depth of the DP                       */
    const double *grid;                 /* grid_length (linspace, impl/hdp_math_utils.c:497-510)         */
    const int64_t *dp_parent;           /* num_dps, -1 for the base DP                                   */
    const int64_t *dp_num_factor_children, *dp_depth;
    const uint8_t *observed;            /* num_dps (mark_observed_dps, impl/hdp.c:1132-1160)             */
    const int64_t *row_of_dp;           /* num_dps: row of an observed DP in post / slope, -1 otherwise  */
    const double *post, *slope;         /* n_observed x grid_length                                      */
    const int64_t *f_type, *f_parent;   /* n_factors, tree order: 0 base / 1 middle / 2 data point       */
    const int64_t *f_ref;               /* the factor's DP, or its data index for a data point           */
    const double *f_params;             /* 5 per factor (base factors): mu nu two_alpha beta log-term    */
    const int64_t *f_n_children;
} sa_hdp_state_info_t;
int sa_hdp_state_load(sa_hdp_state_t **out, const char *nhdp_path);
int sa_hdp_state_write(const sa_hdp_state_t *s, const char *nhdp_path);
int sa_hdp_state_info(const sa_hdp_state_t *s, sa_hdp_state_info_t *info);
void sa_hdp_state_free(sa_hdp_state_t *s);
/* out: n_observed x grid_length (rows as sa_hdp_state_info_t.row_of_dp), overwritten */
int sa_hdp_state_distr_sample(const sa_hdp_state_t *s, int device, double *out);
/* The host half of sa_hdp_state_distr_sample on its own: the weights of one sample as CSR over the observed DPs' rows --
 * row r holds entries [row_start[r], row_start[r + 1]) of (col, w); col < n_base_factors names a base factor (in tree order),
 * col == n_base_factors the prior; entries of a row are in the order the reference adds them.  The three arrays are the
 * library's (sa_free). */
int sa_hdp_state_sample_weights(const sa_hdp_state_t *s, int64_t **row_start, int64_t **col, double **w, int64_t *nnz);
/* sum: n_rows x grid_length collectors after `samples` samples; y_out = sum / samples, slope_out the spline slopes (both n_rows x
 * grid_length; y_out may be NULL) */
int sa_hdp_finalize_distributions(const double *grid, int64_t grid_length, const double *sum, int64_t n_rows, int64_t samples,
                                  int device, double *y_out, double *slope_out);

/* ---- the expectations objects of the EM loop, host only -----------------------------------------
 * Hmm / ContinuousPairHmm / HdpHmm (inc/stateMachine.h:64-83, inc/continuousHmm.h:8-75, impl/continuousHmm.c): what
 * getExpectationsUsingAnchors accumulates into, the .expectations files trainModels.py exchanges, and the M-step.
 *   sa_hmm_create            hmmContinuous_getExpectationsHmm (:841-856): an empty accumulator that "fits" the model -- its event
 *                            model loaded (hmmContinuous_loadEventModel), transitions at the transition pseudocount, and for
 *                            SA_HMM_GAUSSIAN (continuousPairHmm_construct :83-144) k-mer posteriors at the emission pseudocount;
 *                            SA_HMM_HDP (hdpHmm_constructEmpty :522-569) carries the assignment threshold and the assignment lists
 *   sa_hmm_add_expectations  adds one read's transition sums and likelihood -- sa_expect_batch's trans9_out / likelihood_out --
 *                            as hmm_addToTransitionsExpectation (:147) and `hmm->likelihood +=` do cell by cell
 *   sa_hmm_add_emission_expectation  continuousPairHmm_addToEmissionExpectation (:159-168)
 *   sa_hmm_add_assignment    hdpHmm_addToAssignment (:510-514): `kmer` points at k characters (not terminated)
 *   sa_hmm_write             continuousPairHmm_writeToFile (:353-407) / hdpHmm_writeToFile (:571-628), byte for byte; a NaN
 *                            transition leaves an empty file (hmmContinuous_checkTransitions)
 *   sa_hmm_load              continuousPairHmm_loadFromFile (:409-507) / hdpHmm_loadFromFile (:630-785): header, transitions and
 *                            likelihood, event model (the reference reads no further for a ContinuousPairHmm: the accumulators of
 *                            a loaded object are empty, at the pseudocounts), and for SA_HMM_HDP the two assignment lines.  What the
 *                            reference answers with st_errAbort is SA_EIO here
 *   sa_hmm_add_expectations_file  HMM.add_expectations_file (src/signalalign/hiddenMarkovModel.py:424-486), trainModels.py's accumulating
 *                            reader: a read's .expectations file added to this object -- transitions and likelihood, and all of a
 *                            ContinuousPairHmm file's accumulator lines (expectations and posteriors summed, the mask or-ed) or an
 *                            HdpHmm file's assignments; an empty or malformed file adds nothing (SA_EIO)
 *   sa_hmm_normalize         continuousPairHmm_normalize (:282-308) = hmmDiscrete_normalizeTransitions (impl/discreteHmm.c:125-137)
 *                            + the event model of every observed k-mer from its expectations; SA_HMM_HDP: the transitions
 *   sa_hmm_load_into_model   the M-step, continuousPairHmm_loadTransitionsIntoStateMachine (:320-338) and (SA_HMM_GAUSSIAN, Gaussian
 *                            model) continuousPairHmm_loadEmissionsIntoStateMachine (:340-351).  gapY -> gapX stays at log 0 as in a
 *                            machine loaded from a .model file, and the gapY table stays 1.75 x the match sd (the reference's :347
 *                            writes it to the wrong index): signalalign_amd/csrc/sa_hmm.c says why.  No batch created from `m`
 *                            may be alive across the call.
 * Views stay valid until the next call that adds an assignment or destroys the object. */
typedef struct sa_hmm sa_hmm_t;
#define SA_HMM_GAUSSIAN 0   /* ContinuousPairHmm, StateMachineType threeState    */
#define SA_HMM_HDP 1        /* HdpHmm, threeStateHdp                             */
typedef struct sa_hmm_view {
    int type, n_states, n_alpha, k;
    char alphabet[64];
    int64_t n_kmers;
    double *transitions;            /* 9: from * 3 + to (match, gapX, gapY), linear space        */
    double *likelihood;
    double *event_model;            /* 5 per k-mer                                               */
    double *event_expectations;     /* SA_HMM_GAUSSIAN: 2 per k-mer                              */
    double *posteriors;             /* SA_HMM_GAUSSIAN: per k-mer                                */
    uint8_t *observed;              /* SA_HMM_GAUSSIAN: per k-mer                                */
    double threshold;               /* SA_HMM_HDP                                                */
    int64_t n_assignments;          /* SA_HMM_HDP                                                */
    const double *assignment_events;
    const char *assignment_kmers;   /* k characters per assignment, not terminated               */
    int has_model;
} sa_hmm_view_t;
int sa_hmm_create(sa_hmm_t **out, const sa_model_t *m, int type, double threshold, double transitions_pseudocount,
                  double emissions_pseudocount);
void sa_hmm_destroy(sa_hmm_t *h);
int sa_hmm_view(sa_hmm_t *h, sa_hmm_view_t *v);
int sa_hmm_set_event_model(sa_hmm_t *h, const double *table5);
int sa_hmm_add_expectations(sa_hmm_t *h, const double *trans9, double likelihood);
int sa_hmm_add_emission_expectation(sa_hmm_t *h, int64_t kmer_index, double mean, double p);
int sa_hmm_add_assignment(sa_hmm_t *h, const char *kmer, double event_mean);
int sa_hmm_write(const sa_hmm_t *h, const char *path);
int sa_hmm_load(sa_hmm_t **out, const char *path, int type, double transitions_pseudocount, double emissions_pseudocount);
int sa_hmm_add_expectations_file(sa_hmm_t *h, const char *path);
int sa_hmm_normalize(sa_hmm_t *h);
int sa_hmm_load_into_model(sa_model_t *m, const sa_hmm_t *h);
/* the model's transitions as the ten tokens of a .model file's second line (linear space; tokens 5, 7 and 9 are 0) */
int sa_model_transitions10(const sa_model_t *m, double *out10);

/* ---- HDP rebuild: model construction, data, the Gibbs sweeps ----------------------------------------
 * What buildHdpUtil (impl/buildHdpUtil.c) and updateHdpFromAssignments (impl/signalMachine.c:384-397) do around the pieces above.
 * The sweep itself is sequential, random-number-driven host code (signalalign_amd/csrc/sa_hdpgibbs.c); every kept sample's
 * take_distr_sample and the finalisation run on the GPU.  PARITY UNPINNED by construction: the reference draws from rand() / ranlib
 * and walks pointer-hashed sets; here one seeded generator and insertion-ordered lists -- its tests of this code are properties
 * (tests/hdpTests.c:109-233, tests/nanoporeHdpTests.c:272-480), checked in tests/test_gpu_hdp_rebuild.py.
 *   sa_hdp_state_new       a NanoporeHDP without data: new_hier_dir_proc / new_hier_dir_proc_2 (impl/hdp.c:879-995) + one of the tree
 *                          layouts of impl/nanopore_hdp.c:489-1060 + finalize_hdp_structure.  `gamma` (depth values: 2 for the flat
 *                          layout, 3 otherwise) fixes the concentration parameters; gamma == NULL takes a Gamma prior on them
 *                          (gamma_alpha, gamma_beta per depth) and the sweeps sample them.  `groups`: per letter of `alphabet` (as
 *                          given, unsorted) -- SA_HDP_LAYOUT_COMPOSITION: non-zero = purine; SA_HDP_LAYOUT_GROUP_MULTISET: group number
 *   sa_hdp_nig_params_from_table  normal_inverse_gamma_params_from_minION (impl/nanopore_hdp.c:122-176): mu, nu, alpha, beta by maximum
 *                          likelihood from a lookup table's level means and level sds
 *   sa_hdp_state_pass_data / _pass_assignments / _pass_assignment_file   reset_hdp_data + pass_data_to_hdp (impl/hdp.c:1549-1660:
 *                          observed DPs marked, one chain of factors per observed DP under one base factor); from (k-mer, event)
 *                          assignments as hdpHmm_loadFromFile hands them on (impl/continuousHmm.c:722-780: sa_hmm_view's arrays);
 *                          from an assignments / alignment table (update_nhdp_from_alignment_with_filter, impl/nanopore_hdp.c:206-297;
 *                          strand_filter NULL: every row).  A k-mer outside the alphabet: SA_EALPHABET (the reference exits)
 *   sa_hdp_state_gibbs     execute_gibbs_sampling (impl/hdp.c:2486-2549): num_samples distribution samples, one per `thinning`
 *                          iterations behind `burn_in`; the collectors are ADDED to the state's (several calls continue one run)
 *   sa_hdp_state_finalize  finalize_distributions (:2551-2584); afterwards sa_hdp_state_write gives a .nhdp the aligner loads
 * SA_ESTATE: sampling without data or after finalisation, finalising without samples. */
#define SA_HDP_LAYOUT_FLAT 0            /* flat_hdp_model: every k-mer under the base DP (singleLevel*)        */
#define SA_HDP_LAYOUT_MULTISET 1        /* multiset_hdp_model: k-mers grouped by their multiset of letters     */
#define SA_HDP_LAYOUT_MIDDLE_NTS 2      /* middle_2_nts_hdp_model: by their two middle letters                 */
#define SA_HDP_LAYOUT_COMPOSITION 3     /* purine_composition_hdp_model: by their number of purines            */
#define SA_HDP_LAYOUT_GROUP_MULTISET 4  /* group_multiset_hdp_model: by the multiset of their letters' groups  */
int sa_hdp_state_new(sa_hdp_state_t **out, int layout, const char *alphabet, int64_t kmer_length, const int64_t *groups,
                     const double *gamma, const double *gamma_alpha, const double *gamma_beta, double grid_start, double grid_stop,
                     int64_t grid_length, double mu, double nu, double alpha, double beta);
/* the same over any tree of Dirichlet processes (set_dir_proc_parent for every DP, parents[base] = -1, every leaf at depth - 1): a
 * plain HierarchicalDirichletProcess, what the reference's own HDP tests build (tests/nanoporeHdpTests.c:272-345) */
int sa_hdp_state_new_tree(sa_hdp_state_t **out, int64_t num_dps, int64_t depth, const int64_t *parents, const double *gamma,
                          const double *gamma_alpha, const double *gamma_beta, double grid_start, double grid_stop, int64_t grid_length,
                          double mu, double nu, double alpha, double beta);
int sa_hdp_nig_params_from_table(const double *table5, int64_t n_kmers, double *mu_out, double *nu_out, double *alpha_out,
                                 double *beta_out);
int sa_hdp_state_pass_data(sa_hdp_state_t *s, const double *data, const int64_t *dp_ids, int64_t n);
int sa_hdp_state_pass_assignments(sa_hdp_state_t *s, const char *kmers /* k characters each */, const double *events, int64_t n);
int sa_hdp_state_pass_assignment_file(sa_hdp_state_t *s, const char *path, const char *strand_filter, int64_t *n_out);
int sa_hdp_state_kmer_dp(const sa_hdp_state_t *s, const char *kmer);   /* kmer_id (impl/nanopore_hdp.c:405-410), -1 outside the alphabet */
int sa_hdp_state_gibbs(sa_hdp_state_t *s, int64_t num_samples, int64_t burn_in, int64_t thinning, uint64_t seed, int device, int verbose);
int sa_hdp_state_finalize(sa_hdp_state_t *s, int device);
int64_t sa_hdp_state_samples_taken(const sa_hdp_state_t *s);
double sa_hdp_digamma(double x);    /* test hooks: the two special functions of the maximum-likelihood alpha (x > 0) */
double sa_hdp_trigamma(double x);

/* ---- HDP distribution distances ---------------------------------------------------------------
 * How far apart are the distributions of two Dirichlet processes: DistributionMetricMemo (inc/hdp.h:82-106, impl/hdp.c:2614-2866)
 * and its k-mer wrappers (inc/nanopore_hdp.h:77-97, impl/nanopore_hdp.c:431-483).  The reference fills its memo lazily, a pair at a
 * time; here the whole triangle is one GPU pass (signalalign_amd/csrc/sa_hdpdist.hip), a thread per pair, the reference's
 * expressions term for term in its summation order -- no clamping: a zero density is a NaN for KL and Shannon-Jensen, an integral
 * above one a NaN for Hellinger, two bit-identical rows give exactly 0 for KL, Shannon-Jensen and L2.
 * Argument checks come before any device use (SA_EINVAL: grid_length < 2, n_rows < 1, an unknown metric, a NULL array; n_rows == 1
 * succeeds and writes nothing), then SA_ENODEVICE without a GPU.  The state-level calls: SA_ESTATE unless the splines are
 * finalised, SA_EINVAL for an id outside [0, num_dps); an unobserved DP stands for its nearest observed ancestor (:2651-2658,
 * :2600-2602).  kernel_ms_out (may be NULL): HIP-event time of the kernels alone. */
#define SA_HDP_METRIC_KL 0              /* kl_divergence          impl/hdp.c:2666-2683 (symmetrised) */
#define SA_HDP_METRIC_HELLINGER 1       /* hellinger_distance     :2693-2710 */
#define SA_HDP_METRIC_L2 2              /* l2_distance            :2720-2738 */
#define SA_HDP_METRIC_SHANNON_JENSEN 3  /* shannon_jensen_distance :2748-2767 */
/* all pairs among n_rows distributions sampled on one grid: tri_out[(i - 1) * i / 2 + j] for i > j
 * (the memo's index, impl/hdp.c:2629); n_rows * (n_rows - 1) / 2 doubles in ordinary host memory */
int sa_hdp_distances(const double *grid, int64_t grid_length, const double *rows, int64_t n_rows, int metric,
                     int device, double *tri_out, double *kernel_ms_out);
/* returns the device and pinned scratch sa_hdp_distances keeps between calls */
void sa_hdp_distances_release(void);
/* n pairs: a[i * grid_length ..] against b[i * grid_length ..] */
int sa_hdp_distances_paired(const double *grid, int64_t grid_length, const double *a, const double *b, int64_t n,
                            int metric, int device, double *out, double *kernel_ms_out);
/* dir_proc_density (:2588-2612) for n_dps DP ids x n_x query points, out[d * n_x + q]; on the device.  grid_spline_interp
 * (impl/hdp_math_utils.c:471-495) operation for operation; its left knot index is kept within the arrays */
int sa_hdp_state_densities(const sa_hdp_state_t *s, const int64_t *dp_ids, int64_t n_dps, const double *x, int64_t n_x,
                           int device, double *out);
/* the full memo over the state's observed DPs (rows as sa_hdp_state_info_t.row_of_dp) */
int sa_hdp_state_distances(const sa_hdp_state_t *s, int metric, int device, double *tri_out, double *kernel_ms_out);
/* get_dir_proc_distance (:2614-2636) for n pairs of DP ids: 0.0 for dp1[i] == dp2[i] without evaluating; two different ids that
 * resolve to one row are evaluated */
int sa_hdp_state_distance_pairs(const sa_hdp_state_t *s, int metric, const int64_t *dp1, const int64_t *dp2, int64_t n,
                                int device, double *out);
/* compare_hdp_distrs (:2809-2842): s1's grid is the master, s2's densities are interpolated on it (no shortcut for equal ids) */
int sa_hdp_state_compare(const sa_hdp_state_t *s1, const int64_t *dp1, const sa_hdp_state_t *s2, const int64_t *dp2,
                         int64_t n, int metric, int device, double *out);
/* An HDP's distributions against a Gaussian table (get_kl_divergence / get_hellinger_distance / get_median_delta /
 * compare_distributions, src/signalalign/hiddenMarkovModel.py:775-837).  Per entry p is the DP's stored posterior row on the state's
 * own grid g and q = exp(-((g - mean) / sd)^2 / 2) / sqrt(2 pi) / sd (scipy's norm.pdf):
 *   kl_bits     scipy.stats.entropy(pk=p, qk=q, base=2): p and q divided by their sums, sum of rel_entr, divided by log 2;
 *               rel_entr(a, b) = a log1p((a - b) / b) for 0.5 < a / b < 2, a log(a / b) while the quotient is a normal number,
 *               a (log a - log b) when it under- or overflows; 0 for a = 0, b >= 0; +inf otherwise (a > 0, b = 0)
 *   hellinger   hellinger2 (:1119-1120): ||sqrt(p) - sqrt(q)||_2 / sqrt(2) on the values as they are (not normalised)
 *   mode_delta  |g[first argmax p] - mean|
 *   status      0: kl_bits is finite; 1: the DP is not observed (the Python reads an empty row and returns None; no ancestor stands
 *               in; the fields are 0); 2: kl_bits is not finite (left in place; the other two fields are valid)
 * One wave per entry on the device; every sum is one accumulator over the grid points in grid order.  Checked first -- SA_EINVAL:
 * a NULL array, n < 0, an id outside [0, num_dps), a mean that is not finite, an sd that is not finite or <= 0; then SA_ESTATE
 * unless the splines are finalised; n == 0 succeeds and writes nothing; then SA_ENODEVICE without a GPU. */
typedef struct sa_hdp_gauss_cmp { double kl_bits, hellinger, mode_delta; int32_t status, pad; } sa_hdp_gauss_cmp_t;
int sa_hdp_state_vs_gaussian(const sa_hdp_state_t *s, const int64_t *dp_ids, int64_t n, const double *mean, const double *sd,
                             int device, sa_hdp_gauss_cmp_t *out, double *kernel_ms_out);
/* get_nanopore_hdp_alphabet (impl/nanopore_hdp.c): the model's alphabet, NUL-terminated, into at least 64 bytes; k-mer ids count
 * in its order (sa_hdp_state_kmer_dp) */
int sa_hdp_state_alphabet(const sa_hdp_state_t *s, char *alphabet_out);

int sa_device_count(void);
/* HBM of `device`: bytes free (what the library's caching allocator holds counts as free) and in total; a caller that keeps
 * several batches in flight sizes its pipeline with this (sa_batch_stats_t.f_bytes is the bulk of a batch) */
int sa_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes);
const char *sa_strerror(int code);
const char *sa_version(void);
void sa_free(void *p);

#ifdef __cplusplus
}
#endif
#endif
