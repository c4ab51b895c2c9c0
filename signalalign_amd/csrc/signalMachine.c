/* signalMachine -- drop-in replacement of signalAlign's per-read aligner executable (impl/signalMachine.c).
 *
 * Same argv (getopt table impl/signalMachine.c:514-543), same input files (.model, .nhdp, .npRead, exonerate
 * cigar, indexed FASTA), same outputs: the three TSV renderings appended to -u / -i, the summary line on
 * stdout and the "SUCCESS" line on stderr that signalAlignment.py keys on (src/signalalign/signalAlignment.py:480).
 * The banded pair-HMM itself runs on the MI355X through libsignalalign_hip.so; there is no CPU fallback.
 *
 * Expectations mode (-t/-c) runs sa_expect_batch and writes the .expectations files of impl/continuousHmm.c.
 *
 * Batch front door (not in the reference): --batch <manifest> aligns many reads in ONE
 * process and ONE GPU batch per strand model -- models are parsed once, HIP is initialised once, and the reads run
 * side by side on the device.  Manifest: one read per line, tab separated, '#' comments,
 *     label  npRead  cigar_file  posteriors_out  [posteriors_out2|-]  [sequence_name|-]  [template_expectations|-]  [complement_expectations|-]
 * Everything else (models, references, thresholds, output format) comes from the usual options; --device <n> picks the
 * GPU (one process per GPU, each with its share of the manifest: reads are independent).  Per read the same
 * files, stdout summary line and stderr SUCCESS line are produced as by one single-read invocation.
 *
 * Guide alignment on the GPU (not in the reference either): --guide-window <contig>:<start>-<end>[:+|:-] instead of -p, or a
 * manifest's cigar column written as @<contig>:<start>-<end>[:+|:-], names the stretch of the -f reference the read lies in
 * (0-based, half-open, as a cigar's own coordinates); the read is then aligned to it by sa_guide_align_batch, all such reads of
 * a slice in one call, and the result stands in for the cigar file.
 *
 * Without a window: --guide-locate instead of -p, or a manifest's cigar column of exactly @.  The -f reference is indexed once per
 * process (sa_ref_index_build_fasta), all such reads of a slice are located by one sa_guide_locate_batch call, and each gets the
 * window sa_locate_window names -- from there on it is a read with a guide window.
 *
 * Reads from raw current (not in the reference binary, which starts from the .npRead its Python writes): -q, or a manifest's read
 * column, may name a raw-read file (sa_io.h; recognised by its magic).  All such reads of a slice go through one
 * sa_npread_from_raw_batch call ahead of the guide stages (raw_stage) and come out as 1D reads; --npread-out keeps the .npRead.
 */
#define _GNU_SOURCE
#include <ctype.h>
#include <getopt.h>
#include <inttypes.h>
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <errno.h>
#include <sys/stat.h>
#include <unistd.h>

#include "sa_io.h"
#include "signalalign_hip.h"

#define PROB_1 10000000.0

static void die(const char *fmt, const char *a) { /* st_errAbort: message to stderr, non-zero exit */
    fprintf(stderr, fmt, a ? a : "");
    fputc('\n', stderr);
    exit(1);
}

/* the one allocator of this file: n elements (a zero count becomes one), zeroed on request; never NULL */
static void *xalloc(int64_t n, size_t size, int zeroed) {
    const size_t count = (size_t) (n > 0 ? n : 1);
    void *p = zeroed ? calloc(count, size) : malloc(count * size);
    if (!p) die("signalMachine: out of memory%s", "");
    return p;
}

static void usage(void) {
    fprintf(stderr, "\n\tsignalMachine - Align ONT ionic current to a reference sequence\n\n");
    fprintf(stderr, "--help: Display this super useful message and exit\n");
    fprintf(stderr, "--sm3Hdp, -d: Flag, enable HMM-HDP model\n");
    fprintf(stderr, "--twoD, -e: Flag, use 2D workflow (enables complement alignment)\n");
    fprintf(stderr, "-s: Output format, 0=full, 1=variantCaller, 2=assignments\n");
    fprintf(stderr, "-o: Degernate, 0=C/E, 1=C/E/O, 2=A/I, 3=A/C/G/T, 4=J/T, 5=A/F");
    fprintf(stderr, "-T: Template HMM model\n");
    fprintf(stderr, "-C: Complement HMM model\n");
    fprintf(stderr, "-L: Read (output) label\n");
    fprintf(stderr, "-q: NanoporeRead (in npRead format)\n");
    fprintf(stderr, "-f: Forward reference to align to as a flat file\n");
    fprintf(stderr, "-b: Backward reference to align to as a flat file\n");
    fprintf(stderr, "-p: Guide alignment file, containing CIGARs in EXONERATE format\n");
    fprintf(stderr, "-u: Posteriors (output) file path, place to put the output\n");
    fprintf(stderr, "-v: TemplateHDP file\n");
    fprintf(stderr, "-w: Complement HDP file\n");
    fprintf(stderr, "-t: Template expectations (HMM transitions) output location\n");
    fprintf(stderr, "-c: Complement expectations (HMM transitions) output location\n");
    fprintf(stderr, "-x: Diagonal expansion, how much to expand the dynamic programming envelope\n");
    fprintf(stderr, "-D: Posterior probability threshold, keep aligned pairs with posterior prob >= this\n");
    fprintf(stderr, "-m: Constranint trim, how much to trim the guide alignment anchors by\n");
    fprintf(stderr, "-g: traceBackDiagonals, how many backward diagonals to calculate during traceback\n");
    fprintf(stderr, "-r: boolean option if read is RNA\n");
    fprintf(stderr, "--batch <manifest>: align many reads in one process (one GPU batch per strand model)\n");
    fprintf(stderr, "--batch-reads <n>: reads per GPU batch of a manifest (default 2048)\n");
    fprintf(stderr, "--emission <meanOnly|twoDist>: match emission of a Gaussian model (default meanOnly, what the reference's\n"
                    "                  signalMachine installs; twoDist adds the inverse Gaussian on the event noise, every read with its own\n"
                    "                  noise scaling -- with --batch too; Gaussian models, not with -t / -c)\n");
    fprintf(stderr, "--device <n>: GPU to use\n");
    fprintf(stderr, "--guide-window <contig>:<start>-<end>[:+|:-]: instead of -p: compute the guide alignment on the GPU, the read (2-D read\n"
                    "                  with --twoD, else the template read) against that stretch of the -f reference (0-based, half-open);\n"
                    "                  without a strand both are tried.  In a manifest: @<contig>:<start>-<end>[:+|:-] in the cigar column.\n"
                    "                  Not with --rna\n");
    fprintf(stderr, "--guide-locate: instead of -p or --guide-window: find the read's contig, strand and place in the whole -f reference on\n"
                    "                  the GPU, then go on as with the --guide-window that names them.  In a manifest: @ alone in the cigar\n"
                    "                  column.  Needs no -n.  Not with --rna\n");
    fprintf(stderr, "-q <raw-read file> (also a manifest's read column): a read given as raw current and basecalled sequence (recognised by its\n"
                    "                  magic; signalalign_amd/rawio.py writes one): events are detected, aligned to the sequence and mapped to\n"
                    "                  its bases on the GPU, which stands in for the .npRead of a 1D read.  DNA with a Gaussian -T model: not with\n"
                    "                  --twoD, -C, --rna or an .nhdp\n"
                    "--npread-out <dir>: write <dir>/<label>.npRead for every raw read (usable with -q); --signal-labels <dir>: write <dir>/<label>.labels.tsv for every raw read, made on the GPU: raw_start, raw_length, reference_index, posterior_probability, kmer per event on the MEA path (alignedsignal.py add_mea_labels); --signal-labels-kmer-index <n> (2): the labelled base of the k-mer; --signal-labels-full, -bands, -samples: also <label>.full.tsv (every row), .bands.tsv (reference_index, raw_start, raw_length, n_records per position), .samples.i64 (per raw sample the reference_index of its MEA segment or -1, little-endian int64).  Not with --twoD, -t/-c, --snp-step or --snp-sites\n"
                    "--raw-detector <w1,w2,t1,t2,peak>: the event detector's two window lengths, two thresholds and peak height\n"
                    "                  (default 3,6,1.4,9.0,0.2)\n");
    fprintf(stderr, "--guide-band <n>: band width of that alignment: 64, 128 (default), 192 or 256\n");
    fprintf(stderr, "--guide-cigars-out <dir>: write every computed guide alignment to <dir>/<label>.cigar (exonerate format, usable with -p)\n");
    fprintf(stderr, "--mea: also write <posteriors file>.mea, the rows of the full output on the maximum expected accuracy path\n");
    fprintf(stderr, "--site-calls: also write <posteriors file>.calls, per read and ambiguous site the normalised probability of\n"
                    "                  each of its letters (variantCaller.py MarginalizeFullVariants)\n");
    fprintf(stderr, "--site-calls-aggregate <file>: write the per-site calls averaged over all reads of the run to <file>\n"
                    "                  (AggregateOverReadsFull); a manifest's posteriors file may then be '-' (no TSV for that read)\n");
    fprintf(stderr, "--site-calls-accuracy <file>: score the run's site calls against known truth on the GPU: per level (0 per site per\n"
                    "                  read, 1 per read, 2 per genomic site), strand (t, c, all) and letter n_pos, n_neg, auc, the confusion\n"
                    "                  counts at the threshold, accuracy, precision and recall (plot_variant_accuracy.py).  Implies the site\n"
                    "                  tables and the over-reads aggregation; needs one of the two truth options\n"
                    "--site-calls-truth <positions.tsv>: contig, position, strand, change_from, change_to per line (the positions file)\n"
                    "--site-calls-truth-reads <labels.tsv>: read label, true letter per line; such a read is labelled as a whole\n"
                    "--site-calls-accuracy-curves <file>: per row and grid point threshold, tp_ge, fp_ge, tpr, fpr, precision\n"
                    "--site-calls-accuracy-bins <n>: grid points k / n, k = 0 .. n (default 1000)\n"
                    "--site-calls-accuracy-threshold <t>: the confusion counts' threshold (default 0.500000001); --site-calls-accuracy-quality <file> (raw reads, 1-D): per read an R line (label strand status n_calls n_correct n_unlabelled n_other_sites n_outside sum_abs_delta2 max_abs_delta2 max_reference_index n_path n_gaps sum_gap max_gap: calls against the distance of their band from the guide, plot_accuracy_vs_alignment_deviation.py; breaks of the MEA path, plot_breaks_in_alignments.py), a G line per gap (label strand event_before event_after gap), at the end an H line per histogram slot (bin_lo or under / over, wrong, correct); -quality-calls <file>: one line per call (label strand reference_index raw_start raw_length guide_event delta true_letter prob correct outside); -quality-bins lo,width,n (-10000,100,200); -quality-min-gap n (30)\n");
    fprintf(stderr, "--snp-step <N> --snp-dir <dir>: single-nucleotide probabilities: every read is aligned N times, with X at the\n"
                    "                  reference positions = s (mod N) in run s; <dir>/<label>.tsv gets pA pC pG pT per covered position\n"
                    "                  (singleNucleotideProbabilities.py); no posteriors file: no -u, a manifest's posteriors column '-'\n");
    fprintf(stderr, "--snp-marginals <file> (with --snp-step): the probabilities summed over all reads of the run on the GPU, one line per\n"
                    "                  covered site: contig, site, depth, pA pC pG pT, called base, reference base, delta\n"
                    "                  (variantCallingLib.py call_sites_with_marginal_probs); --snp-dir becomes optional: without it no\n"
                    "                  per-read call leaves the GPU.  1-D runs only (not with --twoD)\n"
                    "--snp-proposals <file> (with --snp-marginals): contig, site, delta of the sites whose called base differs from the\n"
                    "                  reference, thinned per contig to the largest delta of each run of sites less than 6 apart\n"
                    "                  (jamison.py group_sites_in_window; a trailing lone site is kept)\n"
                    "--snp-sites <file> (lines contig<TAB>site; with --snp-marginals, not with --snp-step): the second pass: every read\n"
                    "                  is aligned once, with X at the listed sites inside its window, and the same table comes out\n"
                    "--snp-reference-out <fasta> (with --snp-sites): the -f reference with the called base written in at every site\n"
                    "                  whose call differs from it, records and line width as in -f\n");
    fprintf(stderr, "--guide-deviation <file>: how far every read's alignment lies from its guide, made on the GPU from the records of\n"
                    "                  every batch (validateSignalAlignment.py): per read strand an R line (label, strand, status,\n"
                    "                  n_aligned, n_flagged, n_on_mea, mean_abs, max_abs, max_abs_mea, max_event, n_sets), an H line (the\n"
                    "                  histogram of |best position - guide position| in buckets of 5) and an S line per run of events\n"
                    "                  that lie farther than the threshold from the guide; a T line with the summed histogram at the\n"
                    "                  end.  Single reads and --batch; the posteriors file may be '-'.  The MEA paths are computed as\n"
                    "                  with --mea.  Not with -t/-c, --train-*, --snp-step or --snp-sites\n");
    fprintf(stderr, "--guide-deviation-threshold <n>: an event is flagged when it lies more than n positions from the guide (default 10)\n");
    fprintf(stderr, "--guide-deviation-events <file> (with --guide-deviation): one row per aligned event: label, strand, event_index,\n"
                    "                  reference_index, guide_reference_index, diff, on_mea, flagged\n");
    fprintf(stderr, "--position-profile <file> (with --batch): the pile-up of all reads' template alignments per position of the -f\n"
                    "                  reference, summed on the GPU and written at the end of the run: contig, position, reference letter,\n"
                    "                  entropy of the covering posteriors, k-mer rows and reads covering it, and the share of posterior\n"
                    "                  mass on each letter seen (multipleAlignmentAnalysis.py); a manifest's posteriors column may be '-'.\n"
                    "                  1-D DNA runs with -s 0 / 2 / 3 only: not with --twoD, --rna, -s 1, --snp-step or --snp-sites\n");
    fprintf(stderr, "--train-assignments <file>: write the top-N assignments table of the run (buildAlignment: kmer, strand, descaled\n"
                    "                  mean, posterior; what buildHdpUtil -l reads), selected on the GPU\n"
                    "--train-template-model <file> / --train-complement-model <file>: write the -T / -C model with its Gaussian event\n"
                    "                  means and SDs retrained on that table (trainModels.py train_normal_emmissions)\n"
                    "--train-min-prob <p> (0.8), --train-max-assignments <n> (10), --train-weight <w> (100), --train-min-sd <s> (0),\n"
                    "--train-median, --train-mod-only, --train-kmers <file> (one k-mer per line: only those are trained), --train-positions <positions.tsv> (only rows whose k-mer covers a labelled position; not with --rna), --train-positions-coverage <file> (offered rows per position)\n"
                    "                  with any --train-* output, a manifest's posteriors file may be '-' as well\n"
                    "--train-mixture-motifs <canonical:modified,...> (e.g. CCAGG:CEAGG,CCTGG:CETGG) with --train-mixture-template-model\n"
                    "                  <file> / --train-mixture-complement-model <file> / --train-mixture-distances <file>: every\n"
                    "                  canonical k-mer over a motif's modified position gets a two-component Gaussian mixture fitted\n"
                    "                  to its rows of that table on the GPU; the component farther from the -T / -C level mean\n"
                    "                  becomes the modified k-mer's mean and SD in the model written (mixture_model.py), the\n"
                    "                  distances file lists both components per k-mer\n\n");
}
static void usage_die(const char *fmt, const char *a) { usage(); die(fmt, a); }   /* a refusal after the usage text */

typedef struct {
    sa_model_t *model;
    double *table;          /* EMISSION_MATCH_MATRIX as the DP uses it (HDP expected means once they are set)  */
    double *table_orig;     /* as loaded: what the per-read parameter estimation starts from                  */
    sa_model_t *model_two;  /* --batch --emission twoDist: the same model with the two-distribution emission, the base of
                             * sa_batch_create_noise_scaled (every read's noise scaling is applied inside the batch) */
    char alphabet[64];
    int n_alpha, k;
} strand_model_t;

static void kmer_string(const strand_model_t *sm, int32_t id, char *out) {
    for (int i = sm->k - 1; i >= 0; i--) {
        out[i] = sm->alphabet[id % sm->n_alpha];
        id /= sm->n_alpha;
    }
    out[sm->k] = 0;
}

/* adjustReferenceCoordinate, impl/signalMachine.c:54-62 */
static int64_t adjust_ref(int64_t x, int64_t off, int64_t len_kmers, int64_t len, int is_template, int forward) {
    if ((is_template && forward) || (!is_template && !forward)) return x + off;
    return len_kmers - (x + (len - off));
}

typedef struct {
    const char *label, *contig;
    const strand_model_t *sm;
    sa_strand_params_t npp;
    const double *events;   /* all events of the strand, 4 doubles each */
    const char *target;
    int forward, is_template, rna;
    int64_t event_offset, ref_offset;
    const sa_pair_t *pairs;
    int64_t n_pairs;
    double score;
} out_ctx_t;

static int load_strand_model(strand_model_t *sm, const char *model_path, const char *nhdp_path) {
    int rc = sa_model_load(&sm->model, model_path, nhdp_path);
    if (rc) return rc;
    sa_model_alphabet(sm->model, sm->alphabet, &sm->n_alpha, &sm->k);
    int64_t n = 5;
    for (int i = 0; i < sm->k; i++) n *= sm->n_alpha;
    sm->table = malloc(sizeof(double) * (size_t) n);
    sm->table_orig = malloc(sizeof(double) * (size_t) n);
    memcpy(sm->table, sa_model_table5(sm->model), sizeof(double) * (size_t) n);
    memcpy(sm->table_orig, sm->table, sizeof(double) * (size_t) n);
    return SA_OK;
}

/* one read: its inputs, the two alignment jobs, where its outputs go */
typedef struct {
    char *label, *npread_path, *cigar_path, *post_path, *post_path2, *seq_name;
    char *expect[2];      /* [strand]: where -t / -c write the strand's expectations */
    char *guide_window;   /* <contig>:<start>-<end>[:+|:-] instead of a cigar file: the guide alignment is computed (guide_stage) */
    int guide_locate;     /* neither a cigar file nor a window: locate_stage writes guide_window */
    int raw;              /* npread_path names a raw-read file (sa_rawread_is): raw_stage fills np */
    int64_t *raw_start, *raw_length, n_raw_samples;   /* a raw read's events in samples, per template event (--signal-labels) */
    sa_cigar_t *pA;
    sa_npread_t *np;
    char *forward_seq, *backward_seq;
    struct {
        const char *target;   /* the window the strand is aligned to: forward_seq or backward_seq */
        int64_t lo, hi;       /* the strand's events inside the guide alignment */
        int64_t r_shift;      /* reference coordinate shift of the strand's rows */
    } st[2];
    int64_t n_guide;
    int64_t win_lo;       /* contig coordinate of forward_seq[0] (backward_seq[i] lies at win_lo + len - 1 - i) */
    int forward;
    int64_t *ax[2], *ay[2];
    sa_job_t jobs[2];
    sa_model_t *model[2]; /* --emission twoDist, single read: the strand models with this read's noise scaling */
    int failed;
    char err[512];
} read_t;

/* sa_npread_t names its strands; everything here indexes them */
static sa_strand_params_t *np_params(sa_npread_t *np, int s) { return s == 0 ? &np->template_params : &np->complement_params; }
static double *np_events(sa_npread_t *np, int s) { return s == 0 ? np->template_events : np->complement_events; }
static int64_t np_n_events(const sa_npread_t *np, int s) { return s == 0 ? np->n_template_events : np->n_complement_events; }
static const char *np_read(const sa_npread_t *np, int s) { return s == 0 ? np->template_read : np->complement_read; }
static int64_t np_read_length(const sa_npread_t *np, int s) { return s == 0 ? np->template_read_length : np->complement_read_length; }
static const int64_t *np_strand_map(const sa_npread_t *np, int s) {
    return s == 0 ? np->template_strand_event_map : np->complement_strand_event_map;
}
/* base of the aligned read -> event of the strand: per base of the 2D read with --twoD, of the template read without */
static const int64_t *np_event_map(const sa_npread_t *np, int s, int two_d) {
    return s == 0 ? (two_d ? np->template_event_map : np->template_strand_event_map) : np->complement_event_map;
}

typedef struct output output_t;   /* a run-wide output (signalMachine_outputs.inc) */

/* one run: its options as parsed, its models and reference records, its run-wide outputs */
typedef struct {
    int hdp, two_d, rna, expect_mode;
    int mea; /* --mea: also write the maximum-expected-accuracy path of every read (not in the reference binary) */
    int site_calls;         /* --site-calls: also write <posteriors>.calls (not in the reference binary) */
    char *agg_path;   /* --site-calls-aggregate: the over-reads table, written at the end of the run */
    /* --site-calls-accuracy: the run's calls scored against known truth on the GPU (sa_call_scores_t), written at the end; it
     * needs the over-reads table too (want_agg) */
    char *acc_path, *acc_curves_path, *acc_truth_path, *acc_reads_path;
    int acc_bins, acc_opts, want_agg;   /* acc_opts: --site-calls-accuracy-bins, -threshold or a -quality option was given */
    double acc_threshold;
    /* --site-calls-accuracy-quality: every template batch's calls against their distance from the guide, and the breaks of the MEA
     * paths (sa_batch_call_quality), written read by read; cq_calls_path: one line per call */
    char *cq_path, *cq_calls_path;
    sa_callq_params_t cq_params;
    int cq_opts;                        /* a -quality sub-option was given */
    /* --train-*: the top-N assignments of the whole run in k-mer tables on the GPU (one per strand), written at the end */
    char *train_assign, *train_model[2], *train_kmers;
    char *train_pos, *train_pos_cov;   /* --train-positions: only the rows that cover a line of the positions file; --train-positions-coverage */
    int want_train;         /* any of --train-assignments / --train-template-model / --train-complement-model / --train-mixture-* */
    double train_min_prob, train_weight, train_min_sd;
    int64_t train_n;
    int train_median, train_mod_only;
    /* --train-mixture-*: the modified k-mers of motif pairs get the other component of a two-component mixture (mixture_model.py) */
    char *mix_motifs, *mix_model[2], *mix_dist;
    int two_dist; /* --emission twoDist: the two-distribution emission (not an option of the reference binary: it is what its
                   * state machine carried when the reference's shipped output files were written).  A single read is aligned with
                   * a model of its own (read_t.model); the reads of a manifest share one batch on the strand's model_two and
                   * hand over their noise scalings (sa_batch_create_noise_scaled) */
    char *manifest;               /* --batch */
    int batch_mode;
    int64_t batch_reads;          /* --batch-reads */
    read_t one;                   /* the read -L -q -p -u -i -n -t -c --guide-window --guide-locate describe (-n: a manifest's default too) */
    int device;                   /* --device: which GPU of the node (one process per GPU; reads shard across processes) */
    int guide_band;               /* --guide-band */
    char *guide_cigars_out; /* --guide-cigars-out */
    char *npread_out;       /* --npread-out: where raw_stage writes <label>.npRead of every raw read */
    int raw_detector_set;         /* --raw-detector */
    sa_detector_params_t raw_detector;
    int64_t out_fmt, constraint_trim;
    int snp_set;            /* --snp-step was given */
    int64_t snp_step;       /* --snp-step N: single-nucleotide probabilities, N substituted copies of every read's reference */
    char *snp_dir;    /* --snp-dir: where <label>.tsv goes */
    char *snp_marg, *snp_prop;             /* --snp-marginals / --snp-proposals: the over-reads table on the GPU */
    char *snp_sites_path, *snp_ref_out;    /* --snp-sites, --snp-reference-out */
    char *prof_path;                       /* --position-profile: the per-position profile of the run's template batches, on the GPU */
    char *dev_path, *dev_events_path;   /* --guide-deviation: every strand batch's deviation from its guide, written read by read */
    sa_deviation_params_t dev_params;
    /* --signal-labels: every template batch's labelled signal (sa_batch_signal_labels), <dir>/<label>.labels.tsv and the files of the sub-options */
    char *lab_dir;
    int lab_full, lab_bands, lab_samples, lab_kmer_index, lab_kmer_index_set;
    char *model_path[2], *hdp_path[2], *ambig_path;   /* -T -C, -v -w, -a */
    char *fwd_ref, *bwd_ref;
    sa_params_t p;
    strand_model_t sm[2];   /* [strand]: 0 template, 1 complement (--twoD only) */
    const char *ambig[256];
    /* the records of -f, for the outputs that lay a table over them (load_ref_records), and per record the sites of --snp-sites, ascending */
    char **ref_names, **ref_seqs;
    int64_t *ref_lens, n_refs, **sites, *n_sites;
    const read_t *reads0;   /* the run's first read (a read's run ordinal is its place in the manifest) */
    output_t *out[8];       /* the run-wide outputs this run has, in the order they are opened, added to and finished */
    int n_out;
} run_t;

static int n_strands(const run_t *R) { return R->two_d ? 2 : 1; }
static int snp_mode(const run_t *R) { return R->snp_step > 0 || R->snp_sites_path != NULL; }
static const char *strand_name(int s) { return s == 0 ? "template" : "complement"; }

/* single-read mode keeps the reference's abort-with-message behaviour; in batch mode a bad read is reported and skipped */
static int fail(read_t *rd, int fatal, const char *fmt, const char *a) {
    if (fatal) die(fmt, a);
    snprintf(rd->err, sizeof(rd->err), fmt, a ? a : "");
    rd->failed = 1;
    return -1;
}

/* SA_CLI_TIMING=1: wall time of the three stages of every slice and the thread-seconds spent inside the host stage, printed
 * at the end of the run (probes/batch_cli_timing.sh; INTEGRATION.md quotes them) */
static double g_t_prep, g_t_gpu, g_t_render;                 /* wall seconds, summed over slices */
static double g_ts_parse, g_ts_fetch, g_ts_estimate;         /* thread-seconds inside the host stage */
static pthread_mutex_t g_t_mu = PTHREAD_MUTEX_INITIALIZER;
static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double) ts.tv_sec + 1e-9 * (double) ts.tv_nsec;
}
static void t_add(double *acc, double dt) {
    pthread_mutex_lock(&g_t_mu);
    *acc += dt;
    pthread_mutex_unlock(&g_t_mu);
}

static void set_hdp_expected(strand_model_t *sm) { /* stateMachine3_setModelToHdpExpectedValues, once per run */
    sa_model_set_to_hdp_expected_values(sm->model);
    int64_t n = 5;
    for (int i = 0; i < sm->k; i++) n *= sm->n_alpha;
    const double *mt = sa_model_table5(sm->model);
    for (int64_t i = 0; i < n; i += 5) { sm->table[i] = mt[i]; sm->table[i + 1] = mt[i + 1]; }
}

/* host work per read (parsing, parameter estimation, TSV rendering) is independent: a small pthread parallel-for */
typedef struct {
    void (*fn)(int64_t i, void *ctx);
    void *ctx;
    int64_t n;
    int64_t next;
    pthread_mutex_t mu;
} pfor_t;

static void *pfor_worker(void *arg) {
    pfor_t *pf = arg;
    for (;;) {
        pthread_mutex_lock(&pf->mu);
        int64_t i = pf->next++;
        pthread_mutex_unlock(&pf->mu);
        if (i >= pf->n) return NULL;
        pf->fn(i, pf->ctx);
    }
}

static void parallel_for(int64_t n, void (*fn)(int64_t, void *), void *ctx) {
    const char *e = getenv("SA_HOST_THREADS");
    long t = e ? atol(e) : sysconf(_SC_NPROCESSORS_ONLN);
    if (!e) {   /* a container's CPU quota (cgroup v2 cpu.max): more runnable threads than that only get the whole group throttled */
        static long quota = -1;
        if (quota < 0) {
            quota = 0;
            FILE *fq = fopen("/sys/fs/cgroup/cpu.max", "r");
            if (fq) {
                char a[32];
                long per = 0;
                if (fscanf(fq, "%31s %ld", a, &per) == 2 && strcmp(a, "max") != 0 && per > 0) quota = (atol(a) + per - 1) / per;
                fclose(fq);
            }
        }
        if (quota > 0 && t > quota) t = quota;
    }
    if (t > 32) t = 32;
    if (t > n) t = n;
    if (t <= 1) {
        for (int64_t i = 0; i < n; i++) fn(i, ctx);
        return;
    }
    pfor_t pf = {fn, ctx, n, 0, PTHREAD_MUTEX_INITIALIZER};
    pthread_t th[32];
    int started[32];
    for (long k = 0; k < t; k++) started[k] = pthread_create(&th[k], NULL, pfor_worker, &pf) == 0;
    if (!started[0]) pfor_worker(&pf); /* no threads at all: do the work here */
    for (long k = 0; k < t; k++)
        if (started[k]) pthread_join(th[k], NULL);
}

/* What one strand's batch of an alignment slice leaves for the rendering, [job] each.  Without --mea the batch stays alive and
 * pairs[job] is NULL: a job's rows are expanded from the batch's packed records by the thread that renders the job. */
typedef struct {
    sa_pair_t **pairs;
    int64_t *n_pairs;
    sa_mea_pair_t **mea;        /* --mea only */
    int64_t *n_mea;
    sa_batch_t *batch;
    int64_t *all_n, *all_sum;   /* -s 1 only (SA_FLAG_VC_ROWS): number and prob_e7 sum of ALL pairs of the job -- the rows the
                                 * variant-caller output does not print were dropped on the device */
    int p8;                     /* the batch holds 8-byte records (SA_FLAG_PAIRS8): path 0, the reference's k-mer at x */
    sa_site_call_t **calls;     /* --site-calls / --site-calls-aggregate only */
    int64_t *n_calls;
    /* --guide-deviation only: [job] summaries and histogram rows, all jobs' sets, and (--guide-deviation-events) all jobs' events
     * back to back, job j's from dev_ev_first[j] on */
    sa_deviation_read_t *dev_reads;
    sa_deviation_set_t *dev_sets;
    int32_t *dev_hist;
    sa_deviation_event_t *dev_events;
    int64_t *dev_ev_first;
    /* --signal-labels only: [job] records, and all jobs' MEA segments, full set, bands and per-sample maps back to back */
    /* --site-calls-accuracy-quality only: [job] summaries and histogram rows, all jobs' calls and gaps back to back */
    sa_callq_read_t *cq_reads;
    sa_callq_call_t *cq_calls;
    sa_callq_gap_t *cq_gaps;
    int64_t *cq_hist;
    sa_label_read_t *lab_reads;
    sa_label_segment_t *lab_mea, *lab_full;
    sa_label_band_t *lab_bands;
    int32_t *lab_samples;
} strand_result_t;

typedef struct {   /* what one strand's batch of a --snp-step / --snp-sites slice leaves, [read * N + step] each */
    sa_position_call_t **calls;
    int64_t *n_calls;
    int32_t *x_min, *x_max;
    int64_t *n_pairs, *sum_e7;
} snp_result_t;

/* One slice of the run's reads: host side of every read, one GPU batch per strand model, outputs.  (The whole manifest used to
 * be one batch: fine for thousands of reads, not for a flow cell.) */
typedef struct {
    run_t *R;
    read_t *reads;
    int64_t n_reads;
    int64_t *who, n_ok;   /* the reads that are still in: reads[who[0 .. n_ok)] */
    int validated;        /* the reads' jobs have been planned one by one (drop_refused_reads) */
    int64_t per_read;     /* jobs per read and strand: 1; N with --snp-step N, the substituted copies */
    sa_job_t *jobs[2];    /* [strand][place in who * per_read + copy] */
    char **tgt[2];        /* --snp-step, --snp-sites: the substituted targets those jobs point to, owned here, indexed alike */
    int64_t n_slots;      /* per strand, as the slice started */
    strand_result_t sr[2];       /* alignment mode */
    snp_result_t snp[2];         /* --snp-step, --snp-sites */
    double (*score)[2];          /* [job][strand], while an alignment slice is rendered */
    unsigned char *tmpl_amb;     /* [job], --twoD with site calls: the template strand has a row on an ambiguous k-mer (order_calls) */
} slice_t;

#include "signalMachine_rows.inc"
#include "signalMachine_reads.inc"
#include "signalMachine_outputs.inc"
#include "signalMachine_slices.inc"

/* ---- the steps of main ---- */
static void parse_options(run_t *R, int argc, char **argv) {
    read_t *one = &R->one;
    R->dev_params = (sa_deviation_params_t) {10, 5, 64};
    R->train_min_prob = 0.8; R->train_n = 10; R->train_weight = 100.0;   /* probability_threshold, number_of_kmer_assignments, og_model_weight (trainModels.py) */
    R->batch_reads = 2048; R->constraint_trim = 14; R->guide_band = 128; R->lab_kmer_index = 2;
    R->acc_bins = 1000; R->acc_threshold = 0.500000001;
    R->cq_params = (sa_callq_params_t) {-10000, 100, 200, 30};
    R->p = (sa_params_t) {.threshold = 0.01, .diagonal_expansion = 50, .trace_back_diagonals = 50, .min_diags_between_trace_back = 1000,
                          .split_matrix_bigger_than_this = (int64_t) 3000 * 3000};
    const int N = no_argument, Y = required_argument, O = optional_argument;
    const struct option long_options[] = {
        {"help", N, 0, 'h'}, {"sm3Hdp", N, 0, 'd'}, {"sparse_output", N, 0, 's'}, {"twoD", N, 0, 'e'}, {"rna", N, 0, 'r'},
        {"templateModel", Y, 0, 'T'}, {"complementModel", Y, 0, 'C'}, {"readLabel", Y, 0, 'L'}, {"npRead", Y, 0, 'q'},
        {"exonerate_cigar_file", Y, 0, 'p'}, {"posteriors", Y, 0, 'u'}, {"templateHdp", Y, 0, 'v'}, {"complementHdp", Y, 0, 'w'},
        {"templateExpectations", Y, 0, 't'}, {"complementExpectations", Y, 0, 'c'}, {"diagonalExpansion", Y, 0, 'x'}, {"threshold", Y, 0, 'D'},
        {"constraintTrim", Y, 0, 'm'}, {"forward_reference_path", Y, 0, 'f'}, {"backward_reference_path", O, 0, 'b'}, {"sequence_name", Y, 0, 'n'},
        {"traceBackDiagonals", O, 0, 'g'}, {"posteriorProbsFile2", O, 0, 'i'}, {"ambig_model", O, 0, 'a'},
        {"batch", Y, 0, 1000}, {"device", Y, 0, 1001}, {"mea", N, 0, 1002}, {"batch-reads", Y, 0, 1003}, {"emission", Y, 0, 1004},
        {"site-calls", N, 0, 1005}, {"site-calls-aggregate", Y, 0, 1006}, {"site-calls-accuracy", Y, 0, 1070}, {"site-calls-accuracy-curves", Y, 0, 1071},
        {"site-calls-accuracy-bins", Y, 0, 1072}, {"site-calls-accuracy-threshold", Y, 0, 1073}, {"site-calls-truth", Y, 0, 1074},
        {"site-calls-truth-reads", Y, 0, 1075}, {"site-calls-accuracy-quality", Y, 0, 1076}, {"site-calls-accuracy-quality-calls", Y, 0, 1077},
        {"site-calls-accuracy-quality-bins", Y, 0, 1078}, {"site-calls-accuracy-quality-min-gap", Y, 0, 1079},
        {"train-assignments", Y, 0, 1010}, {"train-template-model", Y, 0, 1011}, {"train-complement-model", Y, 0, 1012}, {"train-min-prob", Y, 0, 1013},
        {"train-max-assignments", Y, 0, 1014}, {"train-weight", Y, 0, 1015}, {"train-min-sd", Y, 0, 1016}, {"train-median", N, 0, 1017},
        {"train-mod-only", N, 0, 1018}, {"train-kmers", Y, 0, 1019}, {"train-mixture-motifs", Y, 0, 1040}, {"train-mixture-template-model", Y, 0, 1041},
        {"train-mixture-complement-model", Y, 0, 1042}, {"train-mixture-distances", Y, 0, 1043},
        {"train-positions", Y, 0, 1044}, {"train-positions-coverage", Y, 0, 1045},
        {"snp-step", Y, 0, 1020}, {"snp-dir", Y, 0, 1021}, {"snp-marginals", Y, 0, 1022}, {"snp-proposals", Y, 0, 1023}, {"snp-sites", Y, 0, 1024},
        {"snp-reference-out", Y, 0, 1025}, {"position-profile", Y, 0, 1026},
        {"guide-deviation", Y, 0, 1060}, {"guide-deviation-threshold", Y, 0, 1061}, {"guide-deviation-events", Y, 0, 1062},
        {"guide-window", Y, 0, 1050}, {"guide-locate", N, 0, 1053}, {"guide-band", Y, 0, 1051}, {"guide-cigars-out", Y, 0, 1052},
        {"npread-out", Y, 0, 1080}, {"raw-detector", Y, 0, 1081},
        {"signal-labels", Y, 0, 1090}, {"signal-labels-kmer-index", Y, 0, 1091}, {"signal-labels-full", N, 0, 1092},
        {"signal-labels-bands", N, 0, 1093}, {"signal-labels-samples", N, 0, 1094}, {0, 0, 0, 0}};
    /* the options that name a file or another string, and the flags */
    const struct { int key; char **to; } strings[] = {
        {'a', &R->ambig_path}, {'T', &R->model_path[0]}, {'C', &R->model_path[1]}, {'L', &one->label}, {'q', &one->npread_path}, {'p', &one->cigar_path},
        {'u', &one->post_path}, {'t', &one->expect[0]}, {'c', &one->expect[1]}, {'v', &R->hdp_path[0]}, {'w', &R->hdp_path[1]}, {'f', &R->fwd_ref},
        {'b', &R->bwd_ref}, {'n', &one->seq_name}, {'i', &one->post_path2}, {1000, &R->manifest}, {1006, &R->agg_path}, {1070, &R->acc_path},
        {1071, &R->acc_curves_path}, {1074, &R->acc_truth_path}, {1075, &R->acc_reads_path}, {1076, &R->cq_path}, {1077, &R->cq_calls_path}, {1010, &R->train_assign}, {1011, &R->train_model[0]},
        {1012, &R->train_model[1]}, {1019, &R->train_kmers}, {1040, &R->mix_motifs}, {1041, &R->mix_model[0]}, {1042, &R->mix_model[1]},
        {1043, &R->mix_dist}, {1044, &R->train_pos}, {1045, &R->train_pos_cov}, {1021, &R->snp_dir}, {1022, &R->snp_marg}, {1023, &R->snp_prop}, {1024, &R->snp_sites_path}, {1025, &R->snp_ref_out},
        {1026, &R->prof_path}, {1060, &R->dev_path}, {1062, &R->dev_events_path}, {1050, &one->guide_window}, {1052, &R->guide_cigars_out},
        {1080, &R->npread_out}, {1090, &R->lab_dir}};
    const struct { int key; int *flag; } flags[] = {{'e', &R->two_d}, {'r', &R->rna}, {'d', &R->hdp}, {1002, &R->mea}, {1005, &R->site_calls},
                                                    {1017, &R->train_median}, {1018, &R->train_mod_only}, {1053, &one->guide_locate},
                                                    {1092, &R->lab_full}, {1093, &R->lab_bands}, {1094, &R->lab_samples}};
    for (;;) {
        int idx = 0, known = 0;
        int key = getopt_long(argc, argv, "h:d:e:s:r:o:a:T:C:a:L:q:f:b:g:i:p:u:v:w:t:c:x:D:m:n:", long_options, &idx);
        if (key == -1) break;
        for (size_t i = 0; i < sizeof(strings) / sizeof(strings[0]) && !known; i++)
            if ((known = strings[i].key == key)) *strings[i].to = optarg ? strdup(optarg) : NULL;
        for (size_t i = 0; i < sizeof(flags) / sizeof(flags[0]) && !known; i++)
            if ((known = flags[i].key == key)) *flags[i].flag = 1;
        if (known) continue;
        switch (key) {
            case 's': if (optarg) sscanf(optarg, "%" SCNd64, &R->out_fmt); break;
            case 'x': sscanf(optarg, "%" SCNd64, &R->p.diagonal_expansion); break;
            case 'D': sscanf(optarg, "%lf", &R->p.threshold); break;
            case 'm': sscanf(optarg, "%" SCNd64, &R->constraint_trim); break;
            case 'g': if (optarg) sscanf(optarg, "%" SCNd64, &R->p.trace_back_diagonals); break;
            case 1001: R->device = atoi(optarg); break;
            case 1072: R->acc_bins = atoi(optarg); R->acc_opts = 1; break;
            case 1073: R->acc_threshold = atof(optarg); R->acc_opts = 1; break;
            case 1078: {
                long long lo = 0, width = 0;
                int n = 0;
                char tail = 0;
                if (sscanf(optarg, "%lld,%lld,%d%c", &lo, &width, &n, &tail) != 3) width = 0;   /* (refused with the other bad grids) */
                R->cq_params.bin_lo = lo; R->cq_params.bin_width = width; R->cq_params.n_bins = n;
                R->cq_opts = 1;
                break;
            }
            case 1079: R->cq_params.min_gap = atoi(optarg); R->cq_opts = 1; break;
            case 1013: R->train_min_prob = atof(optarg); break;
            case 1014: R->train_n = atoll(optarg); break;
            case 1015: R->train_weight = atof(optarg); break;
            case 1016: R->train_min_sd = atof(optarg); break;
            case 1020:
                R->snp_set = 1;
                if (sscanf(optarg, "%" SCNd64, &R->snp_step) != 1) R->snp_step = 0;
                break;
            case 1061: R->dev_params.threshold = atoi(optarg); break;
            case 1051: R->guide_band = atoi(optarg); break;
            case 1091: R->lab_kmer_index = atoi(optarg); R->lab_kmer_index_set = 1; break;
            case 1081: {
                sa_detector_params_t *d = &R->raw_detector;
                char tail = 0;
                if (sscanf(optarg, "%d,%d,%f,%f,%f%c", &d->window_length1, &d->window_length2, &d->threshold1, &d->threshold2, &d->peak_height,
                           &tail) != 5 || d->window_length1 < 1 || d->window_length2 < 1)
                    die("signalMachine: --raw-detector takes w1,w2,t1,t2,peak with window lengths >= 1, not %s", optarg);
                R->raw_detector_set = 1;
                break;
            }
            case 1003: R->batch_reads = atoll(optarg) > 0 ? atoll(optarg) : R->batch_reads; break;
            case 1004:
                if (!strcmp(optarg, "twoDist")) R->two_dist = 1;
                else if (strcmp(optarg, "meanOnly")) die("signalMachine: --emission takes meanOnly or twoDist, not %s", optarg);
                break;
            default: usage(); exit(1);   /* (--help among them) */
        }
    }
    if (!one->label) one->label = strdup("");
    if (R->p.diagonal_expansion % 2 != 0) R->p.diagonal_expansion++;
    R->batch_mode = R->manifest != NULL;
    R->want_train = R->train_assign || R->train_model[0] || R->train_model[1] || R->mix_motifs;
    R->want_agg = R->agg_path != NULL || R->acc_path != NULL;
    if (R->cq_calls_path) R->cq_opts = 1;
    if (R->cq_path || R->cq_opts) R->acc_opts = 1;
}

/* A table of refusals: the first row that is refused ends the run with its message, after the usage text where the row says so.
 * The rows stand in the order the checks have always been made in, so a command line that breaks two rules gets the same answer. */
typedef struct { int refused, usage; const char *fmt, *arg; } refusal_t;
static void refuse_first(const refusal_t *rows, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (rows[i].refused) (rows[i].usage ? usage_die : die)(rows[i].fmt, rows[i].arg);
}
#define REFUSE(rows) refuse_first(rows, sizeof(rows) / sizeof((rows)[0]))

/* what the options alone decide, before the reads are looked at */
static void check_options(const run_t *R) {
    const read_t *one = &R->one;
    const int guide = one->cigar_path != NULL || one->guide_window != NULL;
    const refusal_t rows[] = {
        {R->prof_path && !R->batch_mode, 1, "signalMachine: --position-profile needs --batch <manifest>%s", ""},
        {R->model_path[0] == NULL || (R->model_path[1] == NULL && R->two_d), 0, "Missing model files, exiting", NULL},
        {R->out_fmt == 3 && one->post_path2 == NULL && !R->batch_mode, 0, "Must pass in posteriorProbsFile2 if using 'both' outFmt", NULL},
        {one->cigar_path != NULL && one->guide_window != NULL, 0, "signalMachine: -p and --guide-window exclude each other%s", ""},
        {one->guide_locate && guide, 0, "signalMachine: --guide-locate excludes -p and --guide-window%s", ""},
        {one->guide_locate && R->batch_mode, 0, "signalMachine: --guide-locate is for a single read; in a manifest write @ in the cigar column%s", ""},
        {!guide && !one->guide_locate && !R->batch_mode, 0, "[signalMachine]ERROR: Need to provide input guide alignments, exiting", NULL},
        {R->guide_band < 64 || R->guide_band > 256 || R->guide_band % 64 != 0, 0, "signalMachine: --guide-band takes 64, 128, 192 or 256%s", ""},
    };
    REFUSE(rows);
}

/* the reads of this run: the manifest's, or the one the options describe.  What is refused here needs the manifest or a file. */
static int64_t load_reads(run_t *R, read_t **out) {
    const read_t *one = &R->one;
    read_t *reads = NULL;
    int64_t n_reads = 1;
    if (R->batch_mode) {
        n_reads = load_manifest(R->manifest, &reads);
        if (n_reads < 0) die("[signalMachine]ERROR: cannot read the batch manifest %s", R->manifest);
        for (int64_t i = 0; i < n_reads; i++) {
            if (reads[i].seq_name == NULL && one->seq_name != NULL) reads[i].seq_name = strdup(one->seq_name);
            if (reads[i].expect[0] != NULL || reads[i].expect[1] != NULL) R->expect_mode = 1;
        }
        for (int64_t i = 0; i < n_reads && R->expect_mode; i++)
            if (reads[i].expect[0] == NULL && reads[i].expect[1] == NULL)
                die("[signalMachine]ERROR: batch manifest mixes expectation and alignment reads (%s)", reads[i].label);
    } else {
        reads = xalloc(1, sizeof(read_t), 1);
        reads[0] = *one;
        R->expect_mode = one->expect[0] != NULL || one->expect[1] != NULL;
        if (one->guide_window != NULL || one->guide_locate) {
            if (R->fwd_ref == NULL) die(one->guide_locate ? "[signalMachine] ERROR: --guide-locate needs -f <fasta>" : "[signalMachine] ERROR: --guide-window needs -f <fasta>", NULL);
        } else if (R->fwd_ref == NULL || one->seq_name == NULL) {
            /* the reference needs -n; kept after the cigar check so that the error order matches (impl/signalMachine.c:642-663) */
            sa_cigar_t *probe = NULL;
            if (sa_cigar_load(one->cigar_path, &probe) != SA_OK)
                die("[signalMachine]ERROR: Didn't find input alignment file, looked %s", one->cigar_path);
            sa_cigar_free(probe);
            die("[signalMachine] ERROR: need -f <fasta> and -n <sequence name>", NULL);
        }
    }
    *out = reads;
    return n_reads;
}

/* ... and what the reads themselves rule out, before anything runs */
static void check_reads(const run_t *R, read_t *reads, int64_t n_reads) {
    for (int64_t i = 0; i < n_reads; i++) {   /* guide windows */
        if (reads[i].guide_locate && R->rna) die("signalMachine: --guide-locate (@ in a manifest) cannot be combined with --rna: RNA reads need a cigar file%s", "");
        if (reads[i].guide_window == NULL) continue;
        if (R->rna) die("signalMachine: a guide window (%s) cannot be combined with --rna: RNA reads need a cigar file", reads[i].guide_window);
        char *contig = NULL;
        int64_t a, b;
        int strand;
        if (parse_guide_window(reads[i].guide_window, &contig, &a, &b, &strand) != 0)
            die("signalMachine: cannot read the guide window %s (want <contig>:<start>-<end>[:+|:-])", reads[i].guide_window);
        free(contig);
    }
    for (int64_t i = 0; i < n_reads; i++) {   /* reads given as raw current: DNA, template strand, Gaussian event alignment */
        reads[i].raw = reads[i].npread_path != NULL && sa_rawread_is(reads[i].npread_path);
        if (!reads[i].raw) continue;
        if (R->two_d || R->model_path[1] != NULL) die("signalMachine: a raw read (%s) is a 1D read: not with --twoD or a complement model", reads[i].npread_path);
        if (R->rna) die("signalMachine: a raw read (%s) cannot be combined with --rna: RNA reads need a .npRead", reads[i].npread_path);
        if (R->hdp || R->hdp_path[0] != NULL) die("signalMachine: a raw read (%s) needs a Gaussian template model for its event alignment: not with an .nhdp", reads[i].npread_path);
    }
    if (R->npread_out && mkdir(R->npread_out, 0777) != 0 && errno != EEXIST) die("signalMachine: cannot create %s", R->npread_out);
    if (R->guide_cigars_out && mkdir(R->guide_cigars_out, 0777) != 0 && errno != EEXIST) die("signalMachine: cannot create %s", R->guide_cigars_out);
}

/* the modes against each other: what the options decide once the reads have said whether this is an expectations run */
static void check_modes(const run_t *R, const read_t *reads, int64_t n_reads) {
    const int U = 1, expect = R->expect_mode, snp = R->snp_set || R->snp_sites_path != NULL, snp_any = snp || R->snp_dir != NULL;
    const int calls = R->site_calls || R->want_agg, prof = R->prof_path != NULL, dev = R->dev_path != NULL, lab = R->lab_dir != NULL;
    const int cq = R->cq_path != NULL;
    const sa_callq_params_t *cp = &R->cq_params;
    const char *opt = R->snp_sites_path ? "--snp-sites" : "--snp-step";
    const refusal_t rows[] = {
        /* (the expectation pass keeps the reference-ordered kernels and the model's own noise; an HDP model has no such emission) */
        {R->two_dist && (R->hdp || R->hdp_path[0] || R->hdp_path[1] || expect || R->one.expect[0] || R->one.expect[1]), 0,
         "signalMachine: --emission twoDist aligns reads with a Gaussian model: not with an .nhdp, not with -t / -c%s", ""},
        {(R->mix_motifs != NULL) != (R->mix_model[0] || R->mix_model[1] || R->mix_dist), U,
         "signalMachine: --train-mixture-motifs goes with --train-mixture-template-model / -complement-model / -distances%s", ""},
        {R->want_train && (expect || R->mea), 0, "signalMachine: --train-* needs the alignment mode without --mea%s", ""},
        {R->want_train && (R->train_model[1] || R->mix_model[1]) && !R->two_d, 0, "signalMachine: --train-complement-model needs a 2-D run%s", ""},
        {R->want_train && (R->train_n < 1 || !(R->train_min_prob >= 0 && R->train_min_prob <= 1)), 0, "signalMachine: bad --train-max-assignments / --train-min-prob%s", ""},
        {R->train_pos && !R->want_train, U, "signalMachine: --train-positions needs a --train-* output%s", ""},
        {R->train_pos_cov && !R->train_pos, U, "signalMachine: --train-positions-coverage needs --train-positions <file>%s", ""},
        {R->train_pos && R->rna, U, "signalMachine: --train-positions does not take --rna runs%s", ""},
        {!R->acc_path && (R->acc_curves_path || R->acc_truth_path || R->acc_reads_path || R->acc_opts), U,
         "signalMachine: --site-calls-truth* and --site-calls-accuracy-* need --site-calls-accuracy <file>%s", ""},
        {R->acc_path && !R->acc_truth_path && !R->acc_reads_path, U, "signalMachine: --site-calls-accuracy needs --site-calls-truth <file> or --site-calls-truth-reads <file>%s", ""},
        {R->acc_path && (R->acc_bins < 1 || R->acc_threshold != R->acc_threshold), U, "signalMachine: --site-calls-accuracy-bins takes n >= 1, --site-calls-accuracy-threshold a number%s", ""},
        {R->acc_path && R->two_d && (R->mea || dev), U, "signalMachine: --site-calls-accuracy on a --twoD run cannot be combined with --mea / --guide-deviation%s", ""},
        {expect && calls, U, "signalMachine: --site-calls / --site-calls-aggregate / --site-calls-accuracy need the alignment mode, not -t/-c%s", ""},
        /* --site-calls-accuracy-quality: 1-D accuracy runs of raw reads */
        {!cq && R->cq_opts, U, "signalMachine: --site-calls-accuracy-quality-* need --site-calls-accuracy-quality <file>%s", ""},
        {cq && (cp->bin_width < 1 || cp->bin_width > (1ll << 40) || cp->bin_lo < -(1ll << 40) || cp->bin_lo > (1ll << 40) || cp->n_bins < 1 ||
                cp->n_bins > SA_CQ_MAX_BINS || cp->min_gap < 0), U,
         "signalMachine: --site-calls-accuracy-quality-bins takes lo,width,n with width >= 1 and 1 <= n <= 1024, -min-gap n >= 0%s", ""},
        {cq && R->two_d, U, "signalMachine: --site-calls-accuracy-quality does not take --twoD runs%s", ""},
        {cq && !R->batch_mode && !reads[0].raw, U, "signalMachine: --site-calls-accuracy-quality needs a read given as raw current: an .npRead has no raw starts%s", ""},
        {R->snp_prop && !R->snp_marg, U, "signalMachine: --snp-proposals needs --snp-marginals <file>%s", ""},
        {R->snp_sites_path && R->snp_set, U, "signalMachine: --snp-sites cannot be combined with --snp-step%s", ""},
        {R->snp_ref_out && !R->snp_sites_path, U, "signalMachine: --snp-reference-out needs --snp-sites <file>%s", ""},
        {R->snp_sites_path && !R->snp_marg, U, "signalMachine: --snp-sites needs --snp-marginals <file>%s", ""},
        {R->snp_sites_path && R->snp_dir, U, "signalMachine: --snp-sites writes no per-read files: --snp-dir not allowed%s", ""},
        {R->snp_marg && !snp, U, "signalMachine: --snp-marginals needs --snp-step <N> or --snp-sites <file>%s", ""},
        /* --position-profile: 1-D DNA runs of a manifest that keep every row and every path k-mer */
        {prof && R->two_d, U, "signalMachine: --position-profile does not take --twoD runs%s", ""},
        {prof && R->rna, U, "signalMachine: --position-profile does not take --rna runs%s", ""},
        {prof && R->out_fmt == 1, U, "signalMachine: --position-profile cannot be combined with -s 1 (it drops rows)%s", ""},
        {prof && snp, U, "signalMachine: --position-profile cannot be combined with --snp-step / --snp-sites%s", ""},
        {prof && expect, U, "signalMachine: --position-profile needs the alignment mode, not -t/-c%s", ""},
        {prof && R->fwd_ref == NULL, U, "signalMachine: --position-profile needs -f <fasta>%s", ""},
        /* --guide-deviation: alignment runs that keep every row */
        {R->dev_events_path && !dev, U, "signalMachine: --guide-deviation-events needs --guide-deviation <file>%s", ""},
        {dev && R->dev_params.threshold < 0, U, "signalMachine: --guide-deviation-threshold takes n >= 0%s", ""},
        {dev && expect, U, "signalMachine: --guide-deviation needs the alignment mode, not -t/-c%s", ""},
        {dev && R->want_train, U, "signalMachine: --guide-deviation cannot be combined with --train-*%s", ""},
        {dev && snp_any, U, "signalMachine: --guide-deviation cannot be combined with --snp-step / --snp-sites%s", ""},
        /* --signal-labels: 1-D alignment runs of raw reads */
        {!lab && (R->lab_full || R->lab_bands || R->lab_samples || R->lab_kmer_index_set), U, "signalMachine: --signal-labels-* need --signal-labels <dir>%s", ""},
        {lab && R->two_d, U, "signalMachine: --signal-labels does not take --twoD runs%s", ""},
        {lab && expect, U, "signalMachine: --signal-labels needs the alignment mode, not -t/-c%s", ""},
        {lab && snp_any, U, "signalMachine: --signal-labels cannot be combined with --snp-step / --snp-sites%s", ""},
        {lab && !R->batch_mode && !reads[0].raw, U, "signalMachine: --signal-labels needs a read given as raw current: an .npRead has no raw starts%s", ""},
        /* --snp-step / --snp-sites: their own outputs only */
        {snp_any && !R->snp_sites_path && (!R->snp_set || R->snp_step < 1), U, "signalMachine: --snp-step takes a step N >= 1%s", ""},
        {snp_any && !R->snp_dir && !R->snp_marg, U, "signalMachine: --snp-step needs --snp-dir <directory>%s", ""},
        {snp_any && R->snp_marg && R->two_d, U, "signalMachine: --snp-marginals does not take --twoD runs%s", ""},
        {snp_any && expect, U, "signalMachine: %s cannot be combined with -t/-c", opt},
        {snp_any && R->mea, U, "signalMachine: %s cannot be combined with --mea", opt},
        {snp_any && calls, U, "signalMachine: %s cannot be combined with --site-calls / --site-calls-aggregate / --site-calls-accuracy", opt},
        {snp_any && R->want_train, U, "signalMachine: %s cannot be combined with --train-*", opt},
    };
    REFUSE(rows);
    for (int64_t i = 0; i < n_reads && snp_any; i++) {   /* (this one needs the manifest) */
        if (!reads[i].post_path && !reads[i].post_path2) continue;
        if (R->snp_sites_path) usage_die("signalMachine: --snp-sites writes no posteriors file: no -u / -i, a manifest's posteriors column '-'%s", "");
        usage_die(R->batch_mode ? "signalMachine: --snp-step writes no posteriors file: the manifest's posteriors column of %s must be '-'"
                                : "signalMachine: --snp-step writes no posteriors file: -u / -i not allowed%s", R->batch_mode ? reads[i].label : "");
    }
}

static void load_models(run_t *R) {
    char *const *hdp = R->hdp_path;
    if (hdp[0] != NULL || hdp[1] != NULL) {
        if (hdp[0] == NULL || (hdp[1] == NULL && R->two_d)) die("Need to have template and complement HDPs", NULL);
        if (!R->hdp) {
            R->hdp = 1;
            fprintf(stderr, "[signalAlign] - Using threeStateHdp stateMachine since you pass in an HDP file\n");
        } else {
            fprintf(stderr, "[signalAlign] - using NanoporeHDPs\n");
        }
    }
    if (R->hdp && hdp[0] == NULL) die("signalAlign - ERROR: --sm3Hdp needs -v <template .nhdp>", NULL);
    for (int s = 0; s < n_strands(R); s++)
        if (load_strand_model(&R->sm[s], R->model_path[s], R->hdp ? hdp[s] : NULL) != SA_OK)
            die("signalAlign - ERROR: couldn't find model file here: %s", R->model_path[s]);
    for (int s = 0; s < n_strands(R) && R->two_dist && R->batch_mode; s++) {   /* the base of the slices' noise-scaled batches */
        strand_model_t *sm = &R->sm[s];
        if (sa_model_clone_with_table(&sm->model_two, sm->model, sm->table_orig) != SA_OK ||
            sa_model_set_emission(sm->model_two, SA_EMISSION_TWO_DIST) != SA_OK)
            die("signalMachine: --emission twoDist: could not set up the two-distribution model%s", "");
    }
    for (int s = 0; s < n_strands(R) && R->mix_motifs; s++) {   /* parsed once here, so that a bad list stops the run before it starts */
        mix_pair_t *probe = NULL;
        mixture_pairs(R, s, &probe);
        free(probe);
    }
    if (R->lab_dir && (R->lab_kmer_index < 0 || R->lab_kmer_index >= R->sm[0].k)) {
        char k[16];
        snprintf(k, sizeof(k), "%d", R->sm[0].k);
        die("signalMachine: --signal-labels-kmer-index takes an index inside the model's k-mer: 0 <= n < %s", k);
    }
    if (!R->ambig_path) {
        sa_default_ambig(R->ambig);
    } else if (sa_load_ambig(R->ambig_path, R->ambig) != SA_OK) {
        printf("Couldn't open %s for reading\n", R->ambig_path);
        exit(1);
    }
    /* the alignment branch sets the HDP expected values (impl/signalMachine.c:861-863), the expectation branch does not */
    for (int s = 0; s < n_strands(R) && R->hdp && !R->expect_mode; s++) set_hdp_expected(&R->sm[s]);
}

/* The reads go through in slices of --batch-reads (default 2048): bounded host and device memory for any manifest.
 * Two slices are in the air: while the GPU stage and the rendering of slice k run here, a second thread does the host side
 * of slice k+1 (10 000 short reads: host stage 0.39 s, GPU 0.28 s, rendering 0.25 s, one after the other before).  Rendering
 * stays on this thread, slice after slice, so the summary lines stay in read order: the front door is bound by host CPU
 * time -- text parsing and TSV rendering -- not by the order of its stages.  Returns the reads that failed. */
static int64_t run_slices(run_t *R, read_t *reads, int64_t n_reads) {
    const int64_t per = R->batch_reads;
    int64_t n_failed = 0;
    slice_t cur = {.R = R, .reads = reads, .n_reads = n_reads < per ? n_reads : per}, nxt;
    slice_prepare(&cur);
    for (int64_t off = 0; off < n_reads; off += per) {
        const int64_t n = n_reads - off < per ? n_reads - off : per;
        pthread_t th;
        int started = 0;
        if (off + n < n_reads) {
            nxt = (slice_t) {.R = R, .reads = reads + off + n, .n_reads = n_reads - off - n < per ? n_reads - off - n : per};
            started = pthread_create(&th, NULL, slice_prepare, &nxt) == 0;
            if (!started) slice_prepare(&nxt);
        }
        n_failed += run_slice(R, reads + off, n);
        if (started) pthread_join(th, NULL);
    }
    return n_failed;
}

int main(int argc, char **argv) {
    run_t R;
    memset(&R, 0, sizeof(R));
    parse_options(&R, argc, argv);
    check_options(&R);
    read_t *reads = NULL;
    const int64_t n_reads = load_reads(&R, &reads);
    R.reads0 = reads;
    check_reads(&R, reads, n_reads);
    check_modes(&R, reads, n_reads);
    load_models(&R);
    if (R.lab_dir && mkdir(R.lab_dir, 0777) != 0 && errno != EEXIST) die("signalMachine: cannot create %s", R.lab_dir);
    if (R.snp_step > 0) {   /* a slice holds at most --batch-reads jobs: N per read and strand */
        R.batch_reads = R.batch_reads / R.snp_step < 1 ? 1 : R.batch_reads / R.snp_step;
        if (R.snp_dir && mkdir(R.snp_dir, 0777) != 0 && errno != EEXIST) die("signalMachine: cannot create %s", R.snp_dir);
    }
    outputs_open(&R);
    const int64_t n_failed = run_slices(&R, reads, n_reads);
    outputs_finish(&R);
    if (R.batch_mode)
        fprintf(stderr, "[signalMachine] batch: %" PRId64 " of %" PRId64 " reads aligned\n", n_reads - n_failed, n_reads);
    if (getenv("SA_CLI_TIMING"))
        fprintf(stderr, "[signalMachine] timing: host stage %.3f s wall (thread-seconds: npRead+cigar parse %.3f, reference fetch "
                        "%.3f, parameter estimation+anchors %.3f), GPU stage %.3f s wall, render+write %.3f s wall\n",
                g_t_prep, g_ts_parse, g_ts_fetch, g_ts_estimate, g_t_gpu, g_t_render);
    sa_ref_index_destroy(g_ref_index);
    return n_failed == 0 ? 0 : 1;
}
