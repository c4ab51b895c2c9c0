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
 */
#define _GNU_SOURCE
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
    fprintf(stderr, "--mea: also write <posteriors file>.mea, the rows of the full output on the maximum expected accuracy path\n");
    fprintf(stderr, "--site-calls: also write <posteriors file>.calls, per read and ambiguous site the normalised probability of\n"
                    "                  each of its letters (variantCaller.py MarginalizeFullVariants)\n");
    fprintf(stderr, "--site-calls-aggregate <file>: write the per-site calls averaged over all reads of the run to <file>\n"
                    "                  (AggregateOverReadsFull); a manifest's posteriors file may then be '-' (no TSV for that read)\n");
    fprintf(stderr, "--snp-step <N> --snp-dir <dir>: single-nucleotide probabilities: every read is aligned N times, with X at the\n"
                    "                  reference positions = s (mod N) in run s; <dir>/<label>.tsv gets pA pC pG pT per covered position\n"
                    "                  (singleNucleotideProbabilities.py); no posteriors file: no -u, a manifest's posteriors column '-'\n");
    fprintf(stderr, "--train-assignments <file>: write the top-N assignments table of the run (buildAlignment: kmer, strand, descaled\n"
                    "                  mean, posterior; what buildHdpUtil -l reads), selected on the GPU\n"
                    "--train-template-model <file> / --train-complement-model <file>: write the -T / -C model with its Gaussian event\n"
                    "                  means and SDs retrained on that table (trainModels.py train_normal_emmissions)\n"
                    "--train-min-prob <p> (0.8), --train-max-assignments <n> (10), --train-weight <w> (100), --train-min-sd <s> (0),\n"
                    "--train-median, --train-mod-only, --train-kmers <file> (one k-mer per line: only those are trained)\n"
                    "                  with any --train-* output, a manifest's posteriors file may be '-' as well\n\n");
}

static double descale(double e, double level, double scale, double shift, double var) {
    return (e + var * level - scale * level - shift) / var;
}

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

/* Rows are put together in a line buffer and handed to stdio as bytes: "%f" through sa_format_f6 (the same characters as
 * printf, tests/test_host_ambig.py), integers and strings by hand.  With fprintf a row of the full format cost 0.8 us of
 * formatter on every one of 11 million rows of a 1000-read batch; rendering was the largest stage of the front door. */
static char *put_s(char *p, const char *s) {
    while (*s) *p++ = *s++;
    return p;
}
static char *put_i64(char *p, int64_t v) {
    char t[24];
    int n = 0;
    uint64_t u = v < 0 ? (uint64_t) 0 - (uint64_t) v : (uint64_t) v;
    if (v < 0) *p++ = '-';
    do { t[n++] = (char) ('0' + u % 10); u /= 10; } while (u);
    while (n) *p++ = t[--n];
    return p;
}
static char *put_f(char *p, double v) { return p + sa_format_f6(p, v); }
static void reverse_complement_into(const char *s, int k, char *out) {   /* sa_reverse_complement of a k-mer, no allocation */
    for (int i = 0; i < k; i++) {
        const char c = s[k - 1 - i];
        out[i] = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C'
               : c == 'a' ? 't' : c == 't' ? 'a' : c == 'c' ? 'g' : c == 'g' ? 'c' : c;
    }
    out[k] = 0;
}
static FILE *open_rows(const char *path) {
    FILE *fh = fopen(path, "a");
    if (!fh) die("signalMachine: cannot open output %s", path);
    setvbuf(fh, NULL, _IOFBF, 1 << 20);
    return fh;
}

/* writePosteriorProbsFull, impl/signalMachine.c:89-159 */
static void write_full(const char *path, const out_ctx_t *o) {
    FILE *fh = open_rows(path);
    const size_t fixed = strlen(o->contig) + strlen(o->label);
    char *line = (char *) malloc(fixed + 640);   /* nine "%f" of at most 320 characters... in theory; 24 for sane values */
    if (!line) die("signalMachine: out of memory%s", "");
    const int k = o->sm->k;
    int64_t ref_len = (int64_t) strlen(o->target), ref_len_kmers = ref_len - k;
    char k_i[16], path_kmer[16];
    for (int64_t i = 0; i < o->n_pairs; i++) {
        const sa_pair_t *p = &o->pairs[i];
        int64_t x_adj = adjust_ref(p->x, o->ref_offset, ref_len_kmers, ref_len, o->is_template, o->forward);
        int64_t y = p->y + o->event_offset;
        double prob = ((double) p->prob_e7) / PROB_1;
        double ev_mean = o->events[y * 4], ev_noise = o->events[y * 4 + 1], ev_dur = o->events[y * 4 + 2];
        memcpy(k_i, o->target + p->x, k);
        k_i[k] = 0;
        kmer_string(o->sm, p->kmer_id, path_kmer);
        double E_mean = o->sm->table[(int64_t) p->kmer_id * 5];
        /* emissions_signal_scaleNoise (impl/stateMachine.c:721-741) rescales the table per read; applied on the fly here */
        double E_noise = o->sm->table[(int64_t) p->kmer_id * 5 + 2] * o->npp.scale_sd;
        double scaled_Emean = E_mean * o->npp.scale + o->npp.shift;
        double scaled_Enoise = E_noise * o->npp.scale_sd;
        double descaled = descale(ev_mean, E_mean, o->npp.scale, o->npp.shift, o->npp.var);
        char ref_kmer[16], tmp[16];
        if ((o->is_template && o->forward) || (!o->is_template && !o->forward)) memcpy(ref_kmer, k_i, (size_t) k + 1);
        else reverse_complement_into(k_i, k, ref_kmer);
        if (o->rna) {
            reverse_complement_into(ref_kmer, k, tmp);
            memcpy(ref_kmer, tmp, (size_t) k + 1);
        }
        const double vals[9] = {ev_mean, ev_noise, ev_dur, scaled_Emean, scaled_Enoise, prob, descaled, E_mean, 0.0};
        int wide = 0;   /* a value the 24-character budget does not hold: the formatter's own path */
        for (int q = 0; q < 8; q++) wide |= !(fabs(vals[q]) < 9.0e15);
        if (wide) {
            fprintf(fh, "%s\t%" PRId64 "\t%s\t%s\t%s\t%" PRId64 "\t%f\t%f\t%f\t%s\t%f\t%f\t%f\t%f\t%f\t%s\n", o->contig, x_adj,
                    ref_kmer, o->label, o->is_template ? "t" : "c", y, ev_mean, ev_noise, ev_dur, k_i, scaled_Emean,
                    scaled_Enoise, prob, descaled, E_mean, path_kmer);
            continue;
        }
        char *w = line;
        w = put_s(w, o->contig); *w++ = '\t';
        w = put_i64(w, x_adj); *w++ = '\t';
        w = put_s(w, ref_kmer); *w++ = '\t';
        w = put_s(w, o->label); *w++ = '\t';
        *w++ = o->is_template ? 't' : 'c'; *w++ = '\t';
        w = put_i64(w, y); *w++ = '\t';
        w = put_f(w, ev_mean); *w++ = '\t';
        w = put_f(w, ev_noise); *w++ = '\t';
        w = put_f(w, ev_dur); *w++ = '\t';
        w = put_s(w, k_i); *w++ = '\t';
        w = put_f(w, scaled_Emean); *w++ = '\t';
        w = put_f(w, scaled_Enoise); *w++ = '\t';
        w = put_f(w, prob); *w++ = '\t';
        w = put_f(w, descaled); *w++ = '\t';
        w = put_f(w, E_mean); *w++ = '\t';
        w = put_s(w, path_kmer); *w++ = '\n';
        fwrite(line, 1, (size_t) (w - line), fh);
    }
    free(line);
    fclose(fh);
}

/* writePosteriorProbsVC, impl/signalMachine.c:161-232: only k-mers holding the internal ambiguity letter X */
static void write_vc(const char *path, const out_ctx_t *o) {
    int forward = o->forward;
    int label_forward = (o->rna || !o->is_template) ? !forward : forward;
    FILE *fh = open_rows(path);
    char *line = (char *) malloc(strlen(o->contig) + strlen(o->label) + 768);
    if (!line) die("signalMachine: out of memory%s", "");
    const int k = o->sm->k;
    int64_t ref_len = (int64_t) strlen(o->target), ref_len_kmers = ref_len - k;
    char k_i[16], path_kmer[16];
    for (int64_t i = 0; i < o->n_pairs; i++) {
        const sa_pair_t *p = &o->pairs[i];
        memcpy(k_i, o->target + p->x, k);
        k_i[k] = 0;
        int same = (o->is_template && forward) || (!o->is_template && !forward);
        char ref_kmer[16];
        if (same) memcpy(ref_kmer, k_i, (size_t) k + 1);
        else reverse_complement_into(k_i, k, ref_kmer);
        if (!strchr(ref_kmer, 'X')) continue;
        int64_t x_adj = adjust_ref(p->x, o->ref_offset, ref_len_kmers, ref_len, o->is_template, forward);
        int64_t y = p->y + o->event_offset;
        double prob = ((double) p->prob_e7) / PROB_1;
        kmer_string(o->sm, p->kmer_id, path_kmer);
        for (int q = 0; q < k; q++) {
            if (ref_kmer[q] != 'X') continue;
            int qp = same ? q : (k - 1) - q; /* adjustQueryPosition :81-87 */
            char *w = line;
            w = put_i64(w, y); *w++ = '\t';
            w = put_i64(w, x_adj + q); *w++ = '\t';
            *w++ = path_kmer[qp]; *w++ = '\t';
            w = put_f(w, prob); *w++ = '\t';
            *w++ = o->is_template ? 't' : 'c'; *w++ = '\t';
            w = put_s(w, label_forward ? "forward" : "backward"); *w++ = '\t';
            w = put_s(w, o->label); *w++ = '\t';
            w = put_f(w, o->score); *w++ = '\t';
            w = put_s(w, o->contig); *w++ = '\n';
            fwrite(line, 1, (size_t) (w - line), fh);
        }
    }
    free(line);
    fclose(fh);
}

/* writeAssignments, impl/signalMachine.c:234-270 */
static void write_assignments(const char *path, const out_ctx_t *o) {
    FILE *fh = open_rows(path);
    char path_kmer[16], line[704];
    for (int64_t i = 0; i < o->n_pairs; i++) {
        const sa_pair_t *p = &o->pairs[i];
        int64_t y = p->y + o->event_offset;
        double prob = ((double) p->prob_e7) / PROB_1;
        kmer_string(o->sm, p->kmer_id, path_kmer);
        double E_mean = o->sm->table[(int64_t) p->kmer_id * 5];
        double descaled = descale(o->events[y * 4], E_mean, o->npp.scale, o->npp.shift, o->npp.var);
        char *w = line;
        w = put_s(w, path_kmer); *w++ = '\t';
        *w++ = o->is_template ? 't' : 'c'; *w++ = '\t';
        w = put_f(w, descaled); *w++ = '\t';
        w = put_f(w, prob); *w++ = '\n';
        fwrite(line, 1, (size_t) (w - line), fh);
    }
    fclose(fh);
}

static void output_alignment(int64_t fmt, const char *f1, const char *f2, const out_ctx_t *o) {
    switch (fmt) {
        case 0: write_full(f1, o); break;
        case 1: write_vc(f1, o); break;
        case 2: write_assignments(f1, o); break;
        case 3: write_full(f1, o); write_vc(f2, o); break;
        default: fprintf(stderr, "signalAlign - No valid output format provided\n");
    }
}

/* continuousPairHmm_writeToFile (impl/continuousHmm.c:352-408) / hdpHmm_writeToFile (:572-623): the library's Hmm object
 * (sa_hmm_*), filled with what sa_expect_batch returned for the read.  `trans` already holds the transition pseudocount. */
static void write_expectations(const char *path, const strand_model_t *sm, const sa_strand_params_t *npp, int hdp, double threshold,
                               const double *trans, double lik, const sa_job_t *job, const sa_assignment_t *as,
                               int64_t n_as) {
    sa_hmm_t *h = NULL;
    int rc = sa_hmm_create(&h, sm->model, hdp ? SA_HMM_HDP : SA_HMM_GAUSSIAN, threshold, 0.0, 0.001 /* emissionsPseudocount, :785 */);
    if (rc != SA_OK) die("signalMachine: cannot build the expectations object: %s", sa_strerror(rc));
    int64_t n_kmers = 1;
    for (int i = 0; i < sm->k; i++) n_kmers *= sm->n_alpha;
    /* the event model is the state machine's table after this read's emissions_signal_scaleNoise
     * (impl/stateMachine.c:721-741: noise_mean *= scale_sd, noise_lambda *= var_sd, noise_sd = sqrt(mean^3 / lambda)) */
    double *em = malloc(sizeof(double) * 5 * (size_t) n_kmers);
    if (!em) die("signalMachine: out of memory%s", "");
    for (int64_t i = 0; i < n_kmers * 5; i += 5) {
        const double nm = sm->table[i + 2] * npp->scale_sd, nl = sm->table[i + 4] * npp->var_sd;
        em[i] = sm->table[i]; em[i + 1] = sm->table[i + 1]; em[i + 2] = nm; em[i + 3] = sqrt(pow(nm, 3.0) / nl); em[i + 4] = nl;
    }
    sa_hmm_set_event_model(h, em);
    free(em);
    sa_hmm_add_expectations(h, trans, lik);
    for (int64_t i = 0; hdp && i < n_as; i++)
        sa_hmm_add_assignment(h, job->ref + as[i].ref_pos, job->events[as[i].event * job->event_stride]);
    rc = sa_hmm_write(h, path);
    sa_hmm_destroy(h);
    if (rc != SA_OK) die("signalMachine: cannot open %s for writing", path);
}

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

/* options shared by every read of a run */
typedef struct {
    int hdp, two_d, rna, expect_mode;
    int mea; /* --mea: also write the maximum-expected-accuracy path of every read (not in the reference binary) */
    int site_calls;         /* --site-calls: also write <posteriors>.calls (not in the reference binary) */
    const char *agg_path;   /* --site-calls-aggregate: the over-reads table, written at the end of the run */
    /* --train-*: the top-N assignments of the whole run in k-mer tables on the GPU (one per strand), written at the end */
    const char *train_assign, *train_model[2], *train_kmers;
    double train_min_prob, train_weight, train_min_sd;
    int64_t train_n;
    int train_median, train_mod_only;
    sa_kmer_table_t *train_tab[2];
    int two_dist; /* --emission twoDist: the two-distribution emission (not an option of the reference binary: it is what its
                   * state machine carried when the reference's shipped output files were written).  A single read is aligned with
                   * a model of its own (read_t.model); the reads of a manifest share one batch on the strand's model_two and
                   * hand over their noise scalings (sa_batch_create_noise_scaled) */
    int batch_mode;
    int64_t out_fmt, constraint_trim;
    int64_t snp_step;       /* --snp-step N: single-nucleotide probabilities, N substituted copies of every read's reference */
    const char *snp_dir;    /* --snp-dir: where <label>.tsv goes */
    const char *fwd_ref, *bwd_ref;
    sa_params_t p;
    strand_model_t smt, smc;
    const char *ambig[256];
} run_t;

/* one read: its inputs, the two alignment jobs, where its outputs go */
typedef struct {
    char *label, *npread_path, *cigar_path, *post_path, *post_path2, *seq_name, *t_expect, *c_expect;
    sa_cigar_t *pA;
    sa_npread_t *np;
    char *forward_seq, *backward_seq;
    const char *template_target, *complement_target;
    int64_t t_lo, t_hi, c_lo, c_hi, r_shift_t, r_shift_c, n_guide;
    int64_t win_lo;       /* contig coordinate of forward_seq[0] (backward_seq[i] lies at win_lo + len - 1 - i) */
    int forward;
    int64_t *ax[2], *ay[2];
    sa_job_t jobs[2];
    sa_model_t *model[2]; /* --emission twoDist, single read: the strand models with this read's noise scaling */
    int failed;
    char err[512];
} read_t;

/* single-read mode keeps the reference's abort-with-message behaviour; in batch mode a bad read is reported and skipped */
static int fail(read_t *rd, int fatal, const char *fmt, const char *a) {
    if (fatal) die(fmt, a);
    snprintf(rd->err, sizeof(rd->err), fmt, a ? a : "");
    rd->failed = 1;
    return -1;
}

static int estimate_strand(const strand_model_t *sm, const int64_t *strand_map, double *events, int64_t n_events,
                           const char *read, int64_t read_len, sa_strand_params_t *out, sa_model_t **read_model) {
    int64_t n = 5;
    for (int i = 0; i < sm->k; i++) n *= sm->n_alpha;
    double *scratch = malloc(sizeof(double) * (size_t) n); /* the estimation rescales the noise columns in place */
    if (!scratch) return SA_ENOMEM;
    memcpy(scratch, sm->table_orig, sizeof(double) * (size_t) n);
    double est[7];
    int rc = sa_estimate_params(sm->model, scratch, strand_map, events, n_events, read, read_len, est);
    if (rc == SA_OK && read_model) {   /* the model this read is aligned with: the rescaled noise columns, two-distribution emission */
        rc = sa_model_clone_with_table(read_model, sm->model, scratch);
        if (rc == SA_OK) rc = sa_model_set_emission(*read_model, SA_EMISSION_TWO_DIST);
    }
    free(scratch);
    if (rc != SA_OK) return rc;
    out->scale = est[0]; out->shift = est[1]; out->var = est[2]; out->drift = est[3];
    out->scale_sd = est[4]; out->var_sd = est[5]; out->shift_sd = est[6];
    return SA_OK;
}

/* everything of impl/signalMachine.c:main between option parsing and performSignalAlignment, for one read */
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

static int validate_read(const run_t *R, read_t *rd);
static int prepare_read(const run_t *R, read_t *rd, int fatal) {
    const double tp0 = now_s();
    if (rd->cigar_path == NULL) return fail(rd, fatal, "[signalMachine]ERROR: Need to provide input guide alignments, exiting", NULL);
    if (sa_cigar_load(rd->cigar_path, &rd->pA) != SA_OK)
        return fail(rd, fatal, "[signalMachine]ERROR: Didn't find input alignment file, looked %s", rd->cigar_path);
    fprintf(stderr, "[signalMachine]NOTICE: Using guide alignments from %s\n", rd->cigar_path);
    sa_cigar_t *pA = rd->pA;
    if (rd->npread_path == NULL || sa_npread_load(rd->npread_path, &rd->np) != SA_OK)
        return fail(rd, fatal, "signalMachine: could not load the nanopore read %s", rd->npread_path);
    sa_npread_t *np = rd->np;
    if (pA->start2 < 0 || pA->end2 <= pA->start2 || pA->end2 > (R->two_d ? np->read_length : np->template_read_length))
        return fail(rd, fatal, "signalMachine: guide alignment of %s does not fit the read", rd->label);
    if (R->rna) {
        int64_t tmp = pA->start2;
        pA->start2 = np->template_read_length - pA->end2;
        pA->end2 = np->template_read_length - tmp;
    }
    const double tp1 = now_s();
    t_add(&g_ts_parse, tp1 - tp0);
    const char *seq_name = rd->seq_name ? rd->seq_name : pA->contig1;
    if (R->fwd_ref == NULL || seq_name == NULL)
        return fail(rd, fatal, "[signalMachine] ERROR: need -f <fasta> and -n <sequence name>", NULL);

    /* fastaHandler_ReferenceSequenceConstructFull, impl/fasta_handler.c:47-102 */
    if (R->rna) { /* listReverse(pA->operationList) */
        for (int64_t i = 0, j = pA->n_ops - 1; i < j; i++, j--) {
            int32_t t = pA->op_type[i]; pA->op_type[i] = pA->op_type[j]; pA->op_type[j] = t;
            int64_t l = pA->op_len[i]; pA->op_len[i] = pA->op_len[j]; pA->op_len[j] = l;
        }
    }
    int ferr = 0;
    rd->forward_seq = pA->strand1 ? sa_fasta_fetch(R->fwd_ref, seq_name, pA->start1, pA->end1 - 1, &ferr)
                                  : sa_fasta_fetch(R->fwd_ref, seq_name, pA->end1, pA->start1 - 1, &ferr);
    if (ferr == -2) {
        fprintf(stderr, "[signalMachine] ERROR %d: sequence name: %s is not in reference fasta: %s \n", ferr, seq_name, R->fwd_ref);
        if (fatal) exit(1);
        return fail(rd, 0, "sequence name %s is not in the reference fasta", seq_name);
    }
    if (rd->forward_seq == NULL) return fail(rd, fatal, "[signalMachine] ERROR: Unable to fetch reference sequence.  ", NULL);
    rd->win_lo = pA->strand1 ? pA->start1 : pA->end1;
    if (R->bwd_ref) {
        rd->backward_seq = pA->strand1 ? sa_fasta_fetch(R->bwd_ref, seq_name, pA->start1, pA->end1 - 1, &ferr)
                                       : sa_fasta_fetch(R->bwd_ref, seq_name, pA->end1, pA->start1 - 1, &ferr);
        if (rd->backward_seq == NULL) return fail(rd, fatal, "[signalMachine] ERROR: Unable to fetch reference sequence.  ", NULL);
        sa_reverse_in_place(rd->backward_seq);
    } else {
        rd->backward_seq = sa_complement(rd->forward_seq);
        sa_reverse_in_place(rd->backward_seq);
    }
    int strand1 = pA->strand1;
    if (R->rna) {
        char *tmp = rd->backward_seq;
        rd->backward_seq = strdup(rd->forward_seq);
        sa_reverse_in_place(rd->backward_seq);
        free(rd->forward_seq);
        rd->forward_seq = tmp;
        sa_reverse_in_place(rd->forward_seq);
        int64_t t2 = pA->start1;
        pA->start1 = pA->end1;
        pA->end1 = t2;
        pA->strand1 = !pA->strand1;
        strand1 = pA->strand1;
    }
    rd->template_target = strand1 ? rd->forward_seq : rd->backward_seq;
    rd->complement_target = strand1 ? rd->backward_seq : rd->forward_seq;

    /* event slices and coordinate shifts (impl/signalMachine.c:726-750) */
    const int64_t *t_map = R->two_d ? np->template_event_map : np->template_strand_event_map;
    rd->t_lo = t_map[pA->start2];
    rd->t_hi = t_map[pA->end2 - 1];
    if (R->two_d) { rd->c_lo = np->complement_event_map[pA->start2]; rd->c_hi = np->complement_event_map[pA->end2 - 1]; }
    rd->r_shift_t = pA->start1;
    rd->r_shift_c = R->two_d ? pA->end1 : 0;
    rd->forward = pA->strand1;

    const double tp2 = now_s();
    t_add(&g_ts_fetch, tp2 - tp1);
    /* anchors from the guide alignment (pA is rebased inside, impl/signalMachineUtils.c:142-164) */
    int64_t cap = 0;
    for (int64_t i = 0; i < pA->n_ops; i++) cap += pA->op_len[i];
    int64_t *gx = malloc(sizeof(int64_t) * (size_t) (cap + 1)), *gy = malloc(sizeof(int64_t) * (size_t) (cap + 1));
    rd->n_guide = sa_guide_to_anchors(pA->start1, pA->end1, pA->strand1, pA->start2, pA->op_type, pA->op_len, pA->n_ops,
                                      R->constraint_trim, gx, gy, cap + 1);
    if (rd->n_guide < 0) { free(gx); free(gy); return fail(rd, fatal, "signalMachine: could not convert the guide alignment", NULL); }

    /* per-strand: estimate the read's parameters (signalUtils_estimateNanoporeParams), build the job */
    if (estimate_strand(&R->smt, np->template_strand_event_map, np->template_events, np->n_template_events,
                        np->template_read, np->template_read_length, &np->template_params,
                        R->two_dist && !R->batch_mode ? &rd->model[0] : NULL) != SA_OK) {
        free(gx); free(gy);
        return fail(rd, fatal, "Cannot get scale params with no assignments", NULL);
    }
    memset(rd->jobs, 0, sizeof(rd->jobs));
    rd->ax[0] = malloc(sizeof(int64_t) * (size_t) (rd->n_guide + 1));
    rd->ay[0] = malloc(sizeof(int64_t) * (size_t) (rd->n_guide + 1));
    int64_t na0 = sa_remap_anchors(gx, gy, rd->n_guide, t_map, pA->start2, rd->ax[0], rd->ay[0]);
    rd->jobs[0].ref = rd->template_target;
    rd->jobs[0].ref_len = (int64_t) strlen(rd->template_target);
    rd->jobs[0].events = np->template_events + 4 * rd->t_lo;
    rd->jobs[0].event_stride = 4;
    rd->jobs[0].n_events = rd->t_hi - rd->t_lo;
    rd->jobs[0].anchor_x = rd->ax[0]; rd->jobs[0].anchor_y = rd->ay[0]; rd->jobs[0].n_anchors = na0;
    rd->jobs[0].scale = np->template_params.scale; rd->jobs[0].shift = np->template_params.shift;
    rd->jobs[0].var = np->template_params.var;
    if (R->two_d) {
        if (estimate_strand(&R->smc, np->complement_strand_event_map, np->complement_events, np->n_complement_events,
                            np->complement_read, np->complement_read_length, &np->complement_params,
                            R->two_dist && !R->batch_mode ? &rd->model[1] : NULL) != SA_OK) {
            free(gx); free(gy);
            return fail(rd, fatal, "Cannot get scale params with no assignments", NULL);
        }
        rd->ax[1] = malloc(sizeof(int64_t) * (size_t) (rd->n_guide + 1));
        rd->ay[1] = malloc(sizeof(int64_t) * (size_t) (rd->n_guide + 1));
        int64_t na1 = sa_remap_anchors(gx, gy, rd->n_guide, np->complement_event_map, pA->start2, rd->ax[1], rd->ay[1]);
        rd->jobs[1].ref = rd->complement_target;
        rd->jobs[1].ref_len = (int64_t) strlen(rd->complement_target);
        rd->jobs[1].events = np->complement_events + 4 * rd->c_lo;
        rd->jobs[1].event_stride = 4;
        rd->jobs[1].n_events = rd->c_hi - rd->c_lo;
        rd->jobs[1].anchor_x = rd->ax[1]; rd->jobs[1].anchor_y = rd->ay[1]; rd->jobs[1].n_anchors = na1;
        rd->jobs[1].scale = np->complement_params.scale; rd->jobs[1].shift = np->complement_params.shift;
        rd->jobs[1].var = np->complement_params.var;
    }
    free(gx);
    free(gy);
    t_add(&g_ts_estimate, now_s() - tp2);
    /* batch mode: the reads of a slice share one GPU batch, and the planner rejects a whole batch for one bad job (a
     * reference window with a letter outside the alphabet, anchors that give an invalid diagonal).  The reference runs one
     * process per read, so only that read may fail.  Alignment runs find the offender when -- and only when -- a batch is
     * turned down (validate_reads below); the expectation routine writes files strand by strand and cannot be re-run, so
     * its jobs are planned alone on the host here (integer geometry only, no GPU). */
    if (!fatal && R->expect_mode) return validate_read(R, rd);
    return 0;
}

/* plans every job of the read alone on the host; marks the read failed when the planner rejects one */
static int validate_read(const run_t *R, read_t *rd) {
    for (int s = 0; s < (R->two_d ? 2 : 1); s++) {
        int rc = sa_plan_describe(s == 0 ? R->smt.model : R->smc.model, &R->p, &rd->jobs[s], R->ambig, 0, NULL, NULL, 0, NULL, 0,
                                  NULL, 0);
        if (rc != SA_OK) return fail(rd, 0, "alignment job rejected: %s", sa_strerror(rc));
    }
    return 0;
}

typedef struct { const run_t *R; read_t *reads; const int64_t *who; } validate_ctx_t;
static void validate_one(int64_t j, void *ctx) {
    validate_ctx_t *v = ctx;
    read_t *rd = &v->reads[v->who[j]];
    if (validate_read(v->R, rd) != 0)
        fprintf(stderr, "[signalMachine] ERROR: read %s skipped: %s\n", rd->label, rd->err);
}

static void set_hdp_expected(strand_model_t *sm) { /* stateMachine3_setModelToHdpExpectedValues, once per run */
    sa_model_set_to_hdp_expected_values(sm->model);
    int64_t n = 5;
    for (int i = 0; i < sm->k; i++) n *= sm->n_alpha;
    const double *mt = sa_model_table5(sm->model);
    for (int64_t i = 0; i < n; i += 5) { sm->table[i] = mt[i]; sm->table[i + 1] = mt[i + 1]; }
}

static char *dup_field(const char *s) { return (s == NULL || s[0] == 0 || strcmp(s, "-") == 0) ? NULL : strdup(s); }

/* manifest of --batch: label, npRead, cigar, posteriors [, posteriors2, sequence_name, template expectations, complement expectations] */
static int64_t load_manifest(const char *path, read_t **out) {
    FILE *fh = fopen(path, "r");
    if (!fh) return -1;
    int64_t n = 0, cap = 0;
    read_t *reads = NULL;
    char *line = NULL;
    size_t lcap = 0;
    while (getline(&line, &lcap, fh) >= 0) {
        size_t len = strlen(line);
        while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
        if (len == 0 || line[0] == '#') continue;
        char *f[8] = {0};
        int nf = 0;
        for (char *tok = line; tok && nf < 8;) {
            char *tab = strchr(tok, '\t');
            if (tab) *tab = 0;
            f[nf++] = tok;
            tok = tab ? tab + 1 : NULL;
        }
        if (nf < 4) { fprintf(stderr, "[signalMachine] batch manifest: line with %d fields ignored (need at least 4)\n", nf); continue; }
        if (n == cap) {
            cap = cap ? cap * 2 : 64;
            reads = realloc(reads, sizeof(read_t) * (size_t) cap);
        }
        read_t *rd = &reads[n++];
        memset(rd, 0, sizeof(*rd));
        rd->label = strdup(f[0]);
        rd->npread_path = dup_field(f[1]);
        rd->cigar_path = dup_field(f[2]);
        rd->post_path = dup_field(f[3]);
        rd->post_path2 = dup_field(f[4]);
        rd->seq_name = dup_field(f[5]);
        rd->t_expect = dup_field(f[6]);
        rd->c_expect = dup_field(f[7]);
    }
    free(line);
    fclose(fh);
    *out = reads;
    return n;
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

typedef struct {
    const run_t *R;
    read_t *reads;
    int fatal;
} prep_ctx_t;

static void prep_one(int64_t i, void *ctx) {
    prep_ctx_t *c = ctx;
    if (prepare_read(c->R, &c->reads[i], c->fatal) != 0)
        fprintf(stderr, "[signalMachine] ERROR: read %s skipped: %s\n", c->reads[i].label, c->reads[i].err);
}

typedef struct {
    const run_t *R;
    read_t *reads;
    const int64_t *who;
    sa_pair_t ***pairs;   /* [strand][job] */
    int64_t **n_pairs;
    double (*score)[2];
    sa_mea_pair_t ***mea; /* [strand][job], --mea only */
    int64_t **n_mea;
    sa_batch_t *const *batch;   /* [strand]: the batch is still alive and pairs[strand][job] is NULL -- a job's rows are expanded
                                 * from the batch's packed records (sa_batch_pairs16) by the thread that renders the job */
    int64_t *const *all_n;      /* [strand][job], -s 1 only (SA_FLAG_VC_ROWS): number and prob_e7 sum of ALL pairs of the job -- the */
    int64_t *const *all_sum;    /* rows the variant-caller output does not print were dropped on the device                        */
    const int *p8;              /* [strand]: the batch holds 8-byte records (SA_FLAG_PAIRS8): path 0, the reference's k-mer at x          */
    sa_site_call_t ***calls;    /* [strand][job], --site-calls / --site-calls-aggregate only */
    int64_t **n_calls;
    unsigned char *tmpl_amb;    /* [job], the same with --twoD: the template strand has a row on an ambiguous k-mer (order_calls) */
} out_job_t;

/* kmer_id of the k letters at s (sorted alphabet, first letter most significant), -1 for a letter outside it */
static int32_t kmer_id_of(const strand_model_t *sm, const char *s) {
    int32_t id = 0;
    for (int i = 0; i < sm->k; i++) {
        const char *q = memchr(sm->alphabet, s[i], (size_t) sm->n_alpha);
        if (!q || !s[i]) return -1;
        id = id * sm->n_alpha + (int32_t) (q - sm->alphabet);
    }
    return id;
}

/* The rows of the full output that lie on the maximum-expected-accuracy path -- what mea_alignment_from_signal_align
 * (src/signalalign/mea_algorithm.py:323-341) returns as its final event table, here as a TSV next to the posteriors file.
 * The path holds one (x, y) per event; where several rows share a cell (ambiguous positions) the row with the lowest
 * posterior is the one the reference's matrix keeps (get_mea_params_from_events :305-318). */
static void write_mea(const char *post_path, const out_ctx_t *o, const sa_mea_pair_t *path, int64_t n_path) {
    char *out_path = malloc(strlen(post_path) + 8);
    sprintf(out_path, "%s.mea", post_path);
    int64_t y_max = -1;
    for (int64_t i = 0; i < n_path; i++) y_max = path[i].event_idx > y_max ? path[i].event_idx : y_max;
    int64_t *x_of = malloc(sizeof(int64_t) * (size_t) (y_max + 2)), *best = malloc(sizeof(int64_t) * (size_t) (y_max + 2));
    for (int64_t y = 0; y <= y_max; y++) { x_of[y] = -1; best[y] = -1; }
    for (int64_t i = 0; i < n_path; i++) x_of[path[i].event_idx] = path[i].ref_idx;
    for (int64_t i = 0; i < o->n_pairs; i++) {
        const sa_pair_t *p = &o->pairs[i];
        if (p->y > y_max || x_of[p->y] != p->x) continue;
        if (best[p->y] < 0 || p->prob_e7 < o->pairs[best[p->y]].prob_e7) best[p->y] = i;
    }
    sa_pair_t *rows = malloc(sizeof(sa_pair_t) * (size_t) (n_path > 0 ? n_path : 1));
    int64_t n = 0;
    for (int64_t i = 0; i < o->n_pairs; i++) {   /* output order of the posteriors file */
        const sa_pair_t *p = &o->pairs[i];
        if (p->y <= y_max && best[p->y] == i) rows[n++] = *p;
    }
    out_ctx_t m = *o;
    m.pairs = rows;
    m.n_pairs = n;
    write_full(out_path, &m);
    free(rows); free(x_of); free(best); free(out_path);
}

/* ---- --site-calls / --site-calls-aggregate: MarginalizeFullVariants.get_data and AggregateOverReadsFull
 * (src/signalalign/variantCaller.py:92-187, :393-410) over the calls sa_batch_site_calls made on the device ---- */
typedef struct { int64_t pos, i; } call_pos_t;
/* does any of the strand's pairs sit on a reference k-mer that holds an ambiguity letter (a variant_data row of get_data, :112)? */
static int has_ambiguous_rows(const char *const *ambig, const char *target, int k, const sa_pair_t *pairs, int64_t n) {
    const int64_t len = (int64_t) strlen(target);
    int64_t *last = malloc(sizeof(int64_t) * (size_t) (len + 1));   /* last[i]: the last ambiguous position below i, -1 none */
    int64_t prev = -1;
    for (int64_t i = 0; i <= len; i++) {
        last[i] = prev;
        if (i < len && ambig[(unsigned char) target[i]]) prev = i;
    }
    int found = 0;
    for (int64_t i = 0; i < n && !found; i++) {
        const int64_t end = (int64_t) pairs[i].x + k;
        found = end <= len && last[end] >= pairs[i].x;
    }
    free(last);
    return found;
}
static int cmp_call_pos(const void *a, const void *b) {
    const int64_t x = ((const call_pos_t *) a)->pos, y = ((const call_pos_t *) b)->pos;
    return x < y ? -1 : x > y;
}
/* The calls of one strand of a read in the order get_data walks them (:141-144): by the reference_index the TSV prints for the
 * site's k-mer (adjust_ref), ascending, reversed when the strand's mapping strand is '-'.  The mapping strand (:128-131, :179):
 * mapping_strands[mapping_index], where the index starts at 0 and moves on after every read strand that has variant_data rows --
 * rows whose reference k-mer holds an ambiguity letter (:112), whether or not one of them is a site.  So the complement gets
 * mapping_strands[1] exactly when the template has such a row (`tmpl_amb`, template_has_ambiguous_rows). */
static call_pos_t *order_calls(const read_t *rd, int s, int tmpl_amb, const sa_site_call_t *calls, int64_t n, int k, char *mapped) {
    const int idx = (s == 1 && tmpl_amb) ? 1 : 0;
    *mapped = (idx == 0) == (rd->forward != 0) ? '+' : '-';
    const char *target = s == 0 ? rd->template_target : rd->complement_target;
    const int64_t ref_len = (int64_t) strlen(target), ref_len_kmers = ref_len - k, off = s == 0 ? rd->r_shift_t : rd->r_shift_c;
    call_pos_t *v = malloc(sizeof(call_pos_t) * (size_t) (n > 0 ? n : 1));
    for (int64_t i = 0; i < n; i++) {
        v[i].pos = adjust_ref(calls[i].x, off, ref_len_kmers, ref_len, s == 0, rd->forward);
        v[i].i = i;
    }
    qsort(v, (size_t) n, sizeof(call_pos_t), cmp_call_pos);
    if (*mapped == '-')
        for (int64_t a = 0, b = n - 1; a < b; a++, b--) { call_pos_t t = v[a]; v[a] = v[b]; v[b] = t; }
    return v;
}
/* <posteriors>.calls: label contig position strand forward_mapped letters p_1 .. p_n (one row per reported site) */
static void write_calls(const char *post_path, const read_t *rd, int s, int tmpl_amb, const sa_site_call_t *calls, int64_t n, int k) {
    char *out_path = malloc(strlen(post_path) + 8);
    sprintf(out_path, "%s.calls", post_path);
    FILE *fh = open_rows(out_path);
    char mapped;
    call_pos_t *v = order_calls(rd, s, tmpl_amb, calls, n, k, &mapped);
    char *line = malloc(strlen(rd->label) + strlen(rd->pA->contig1) + 512);
    for (int64_t q = 0; q < n; q++) {
        const sa_site_call_t *c = &calls[v[q].i];
        char *w = line;
        w = put_s(w, rd->label); *w++ = '\t';
        w = put_s(w, rd->pA->contig1); *w++ = '\t';
        w = put_i64(w, v[q].pos); *w++ = '\t';
        *w++ = s == 0 ? 't' : 'c'; *w++ = '\t';
        *w++ = mapped; *w++ = '\t';
        for (int l = 0; l < c->n_letters; l++) *w++ = c->letters[l];
        for (int l = 0; l < c->n_letters; l++) { *w++ = '\t'; w = put_f(w, c->prob[l]); }
        *w++ = '\n';
        fwrite(line, 1, (size_t) (w - line), fh);
    }
    free(line); free(v); free(out_path);
    fclose(fh);
}

/* The over-reads table (_normalize_all_data :393-407): per (contig, position, strand, forward_mapped) and letter the per-read
 * probabilities summed in read order; written at the end of the run. */
#define AGG_MAX_LETTERS 16
typedef struct {
    int64_t pos;
    int contig, n;
    char strand, mapped, used;
    char letter[AGG_MAX_LETTERS];
    double sum[AGG_MAX_LETTERS];
} agg_entry_t;
static struct {
    agg_entry_t *tab;
    size_t cap, n;
    char **contigs;
    int n_contigs;
} g_agg;
static uint64_t agg_hash(int contig, int64_t pos, char strand, char mapped) {
    uint64_t h = (uint64_t) pos * 0x9E3779B97F4A7C15ull ^ ((uint64_t) (unsigned) contig << 17) ^ ((uint64_t) (unsigned char) strand << 8) ^
                 (uint64_t) (unsigned char) mapped;
    h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    return h;
}
static agg_entry_t *agg_slot(int contig, int64_t pos, char strand, char mapped) {
    if (2 * (g_agg.n + 1) > g_agg.cap) {   /* grow: rehash into twice the room */
        const size_t ncap = g_agg.cap ? 2 * g_agg.cap : 1 << 16;
        agg_entry_t *nt = calloc(ncap, sizeof(agg_entry_t));
        if (!nt) die("signalMachine: out of memory%s", "");
        for (size_t i = 0; i < g_agg.cap; i++) {
            const agg_entry_t *e = &g_agg.tab[i];
            if (!e->used) continue;
            size_t h = (size_t) agg_hash(e->contig, e->pos, e->strand, e->mapped) & (ncap - 1);
            while (nt[h].used) h = (h + 1) & (ncap - 1);
            nt[h] = *e;
        }
        free(g_agg.tab);
        g_agg.tab = nt;
        g_agg.cap = ncap;
    }
    size_t h = (size_t) agg_hash(contig, pos, strand, mapped) & (g_agg.cap - 1);
    for (;; h = (h + 1) & (g_agg.cap - 1)) {
        agg_entry_t *e = &g_agg.tab[h];
        if (!e->used) {
            e->used = 1; e->contig = contig; e->pos = pos; e->strand = strand; e->mapped = mapped;
            g_agg.n++;
            return e;
        }
        if (e->contig == contig && e->pos == pos && e->strand == strand && e->mapped == mapped) return e;
    }
}
static void agg_add_read(const read_t *rd, int s, int tmpl_amb, const sa_site_call_t *calls, int64_t n, int k) {
    if (n <= 0) return;
    int ci = 0;
    while (ci < g_agg.n_contigs && strcmp(g_agg.contigs[ci], rd->pA->contig1) != 0) ci++;
    if (ci == g_agg.n_contigs) {
        g_agg.contigs = realloc(g_agg.contigs, sizeof(char *) * (size_t) (g_agg.n_contigs + 1));
        g_agg.contigs[g_agg.n_contigs++] = strdup(rd->pA->contig1);
    }
    char mapped;
    call_pos_t *v = order_calls(rd, s, tmpl_amb, calls, n, k, &mapped);
    for (int64_t q = 0; q < n; q++) {
        const sa_site_call_t *c = &calls[v[q].i];
        agg_entry_t *e = agg_slot(ci, v[q].pos, s == 0 ? 't' : 'c', mapped);
        for (int l = 0; l < c->n_letters; l++) {
            int t = 0;
            while (t < e->n && e->letter[t] != c->letters[l]) t++;
            if (t == e->n) {
                if (e->n == AGG_MAX_LETTERS) die("signalMachine: --site-calls-aggregate: more than 16 letters at one site%s", "");
                e->letter[e->n] = c->letters[l]; e->sum[e->n] = 0.0; e->n++;
            }
            e->sum[t] += c->prob[l];
        }
    }
    free(v);
}
static int cmp_agg(const void *a, const void *b) {
    const agg_entry_t *x = *(const agg_entry_t *const *) a, *y = *(const agg_entry_t *const *) b;
    const int c = strcmp(g_agg.contigs[x->contig], g_agg.contigs[y->contig]);
    if (c) return c;
    if (x->strand != y->strand) return x->strand < y->strand ? -1 : 1;
    if (x->mapped != y->mapped) return x->mapped < y->mapped ? -1 : 1;
    return x->pos < y->pos ? -1 : x->pos > y->pos;
}
/* write_data (:409-411): header, then the rows as pandas prints them -- np.round(sum / total, 6) through repr.  Columns: the sorted
 * union of the letters; a letter a site does not have counts 0. */
static void write_aggregate(const char *path) {
    int have[256] = {0};
    agg_entry_t **rows = malloc(sizeof(agg_entry_t *) * (g_agg.n ? g_agg.n : 1));
    size_t n = 0;
    for (size_t i = 0; i < g_agg.cap; i++)
        if (g_agg.tab[i].used) {
            rows[n++] = &g_agg.tab[i];
            for (int t = 0; t < g_agg.tab[i].n; t++) have[(unsigned char) g_agg.tab[i].letter[t]] = 1;
        }
    qsort(rows, n, sizeof(agg_entry_t *), cmp_agg);
    FILE *fh = fopen(path, "w");
    if (!fh) die("signalMachine: cannot open output %s", path);
    setvbuf(fh, NULL, _IOFBF, 1 << 20);
    char cols[256];
    int nc = 0;
    for (int ch = 0; ch < 256; ch++)
        if (have[ch]) cols[nc++] = (char) ch;
    fprintf(fh, "contig\tposition\tstrand\tforward_mapped");
    for (int c = 0; c < nc; c++) fprintf(fh, "\t%c", cols[c]);
    fputc('\n', fh);
    char num[40];
    for (size_t r = 0; r < n; r++) {
        const agg_entry_t *e = rows[r];
        double total = 0.0;   /* sum over the letters in column order, as the reference's generator adds them */
        for (int c = 0; c < nc; c++)
            for (int t = 0; t < e->n; t++)
                if (e->letter[t] == cols[c]) total += e->sum[t];
        fprintf(fh, "%s\t%" PRId64 "\t%c\t%c", g_agg.contigs[e->contig], e->pos, e->strand, e->mapped);
        for (int c = 0; c < nc; c++) {
            double v = 0.0;
            for (int t = 0; t < e->n; t++)
                if (e->letter[t] == cols[c]) v = e->sum[t];
            sa_format_py_round6(num, v / total);
            fprintf(fh, "\t%s", num);
        }
        fputc('\n', fh);
    }
    fclose(fh);
    free(rows);
}

static void output_one(int64_t j, void *ctx) {
    out_job_t *c = ctx;
    const run_t *R = c->R;
    read_t *rd = &c->reads[c->who[j]];
    const int n_strands = R->two_d ? 2 : 1;
    if (R->out_fmt == 3 && rd->post_path2 == NULL) {
        fprintf(stderr, "[signalMachine] ERROR: read %s: 'both' output format needs a second output file\n", rd->label);
        rd->failed = 1;
        return;
    }
    /* The rows are expanded here, job by job on the rendering threads, from the packed records the batch holds in page-locked
     * memory: the GPU stage does not expand every job's pairs into freshly allocated sa_pair_t arrays on the main thread (523 MB
     * per slice of 2048 long reads). */
    sa_pair_t *mine[2] = {NULL, NULL};
    const sa_pair_t *pp[2] = {NULL, NULL};
    for (int s = 0; s < n_strands; s++) {
        pp[s] = c->pairs[s][j];
        if (pp[s] == NULL && c->batch && c->batch[s] && c->p8 && c->p8[s]) {
            /* 8-byte records (round 6: -s 0 / 2 on reads without ambiguity letters -- half the bytes over PCIe where the pairs outweigh
             * the kernels, e.g. --sm3Hdp -D 0.01): x, y, probability; the pair's k-mer is the reference's at x, its path 0 */
            const sa_pair8_t *pk8 = NULL;
            int64_t n = 0;
            const strand_model_t *sm = s == 0 ? &R->smt : &R->smc;
            const char *target = s == 0 ? rd->template_target : rd->complement_target;
            if (sa_batch_pairs8(c->batch[s], j, &pk8, &n) != SA_OK || n != c->n_pairs[s][j]) {
                fprintf(stderr, "[signalMachine] ERROR: read %s: results of the batch are not readable\n", rd->label);
                rd->failed = 1;
                free(mine[0]);
                return;
            }
            mine[s] = malloc(sizeof(sa_pair_t) * (size_t) (n > 0 ? n : 1));
            int bad_kmer = 0;
            for (int64_t i = 0; i < n; i++) {
                sa_pair_t *q = &mine[s][i];
                sa_pair8_unpack(pk8[i], &q->prob_e7, &q->x, &q->y);
                q->path = 0;
                q->kmer_id = kmer_id_of(sm, target + q->x);
                bad_kmer |= q->kmer_id < 0;
            }
            if (bad_kmer) {   /* (cannot happen: the planner refuses a reference with a letter outside the model's alphabet) */
                fprintf(stderr, "[signalMachine] ERROR: read %s: a pair names a k-mer outside the model's alphabet\n", rd->label);
                rd->failed = 1;
                free(mine[0]); free(mine[1]);
                return;
            }
            pp[s] = mine[s];
        } else if (pp[s] == NULL && c->batch && c->batch[s]) {
            const sa_pair16_t *pk = NULL;
            int64_t n = 0;
            if (sa_batch_pairs16(c->batch[s], j, &pk, &n) != SA_OK || n != c->n_pairs[s][j]) {
                fprintf(stderr, "[signalMachine] ERROR: read %s: results of the batch are not readable\n", rd->label);
                rd->failed = 1;
                free(mine[0]);
                return;
            }
            mine[s] = malloc(sizeof(sa_pair_t) * (size_t) (n > 0 ? n : 1));
            for (int64_t i = 0; i < n; i++) mine[s][i] = sa_pair16_unpack(pk[i]);
            pp[s] = mine[s];
        }
    }
    for (int s = 0; s < n_strands; s++) {
        double tot = 0.0;
        int64_t n_all = c->n_pairs[s][j];
        if (c->all_n && c->all_n[s]) {   /* (prob_e7 sums are integers below 2^53: the same double as the loop below gives) */
            n_all = c->all_n[s][j];
            tot = (double) c->all_sum[s][j];
        } else {
            for (int64_t i = 0; i < c->n_pairs[s][j]; i++) tot += (double) pp[s][i].prob_e7;
        }
        c->score[j][s] = 100.0 * tot / ((double) n_all * PROB_1); /* scoreByPosteriorProbabilityIgnoringGaps :407-412 */
    }
    const int tmpl_amb = c->tmpl_amb && has_ambiguous_rows(R->ambig, rd->template_target, R->smt.k, pp[0], c->n_pairs[0][j]);
    if (c->tmpl_amb) c->tmpl_amb[j] = (unsigned char) tmpl_amb;
    if (rd->post_path != NULL) {
        out_ctx_t o;
        o.label = rd->label; o.contig = rd->pA->contig1; o.sm = &R->smt; o.npp = rd->np->template_params;
        o.events = rd->np->template_events; o.target = rd->template_target; o.forward = rd->forward; o.is_template = 1;
        o.rna = R->rna; o.event_offset = rd->t_lo; o.ref_offset = rd->r_shift_t; o.pairs = pp[0];
        o.n_pairs = c->n_pairs[0][j]; o.score = c->score[j][0];
        output_alignment(R->out_fmt, rd->post_path, rd->post_path2, &o);
        if (R->mea) write_mea(rd->post_path, &o, c->mea[0][j], c->n_mea[0][j]);
        if (R->site_calls) write_calls(rd->post_path, rd, 0, tmpl_amb, c->calls[0][j], c->n_calls[0][j], R->smt.k);
        if (R->two_d) {
            o.sm = &R->smc; o.npp = rd->np->complement_params; o.events = rd->np->complement_events;
            o.target = rd->complement_target; o.is_template = 0; o.event_offset = rd->c_lo; o.ref_offset = rd->r_shift_c;
            o.pairs = pp[1]; o.n_pairs = c->n_pairs[1][j]; o.score = c->score[j][1];
            output_alignment(R->out_fmt, rd->post_path, rd->post_path2, &o);
            if (R->mea) write_mea(rd->post_path, &o, c->mea[1][j], c->n_mea[1][j]);
            if (R->site_calls) write_calls(rd->post_path, rd, 1, tmpl_amb, c->calls[1][j], c->n_calls[1][j], R->smc.k);
        }
    }
    free(mine[0]); free(mine[1]);
}

static int cmp_str(const void *a, const void *b) { return strcmp(*(const char *const *) a, *(const char *const *) b); }

/* appending from several threads is only safe when no two reads share an output file */
static int outputs_distinct(const read_t *reads, const int64_t *who, int64_t n) {
    const char **v = malloc(sizeof(char *) * (size_t) (2 * n + 1));
    int64_t m = 0;
    for (int64_t j = 0; j < n; j++) {
        if (reads[who[j]].post_path) v[m++] = reads[who[j]].post_path;
        if (reads[who[j]].post_path2) v[m++] = reads[who[j]].post_path2;
    }
    qsort(v, (size_t) m, sizeof(char *), cmp_str);
    int ok = 1;
    for (int64_t i = 1; i < m && ok; i++) ok = strcmp(v[i], v[i - 1]) != 0;
    free(v);
    return ok;
}

/* One slice of the run's reads: host side of every read, one GPU batch per strand model, outputs.  Returns the number
 * of reads that failed.  (The whole manifest used to be one batch: fine for thousands of reads, not for a flow cell.) */
/* host side of every read of a slice (files, parameter estimation, anchors): all host threads */
typedef struct { const run_t *R; read_t *reads; int64_t n; int batch_mode; } slice_prep_t;
static void *slice_prepare(void *arg) {
    slice_prep_t *sp = arg;
    const double ts0 = now_s();
    prep_ctx_t pc = {sp->R, sp->reads, !sp->batch_mode};
    parallel_for(sp->n, prep_one, &pc);
    t_add(&g_t_prep, now_s() - ts0);
    return NULL;
}

/* What the GPU stage of a slice leaves for its rendering */
static void release_read(read_t *rd);
typedef struct {
    run_t *Rp;
    read_t *reads;
    int64_t n_reads, n_ok;
    int64_t *who;
    sa_job_t *bj;
    sa_pair_t **pairs_s[2];
    int64_t *n_pairs_s[2];
    sa_mea_pair_t **mea_s[2];
    int64_t *n_mea_s[2];
    sa_batch_t *batch[2];  /* alive until the slice is rendered (their packed records are what the rendering reads) */
    int64_t *all_n_s[2], *all_sum_s[2];   /* -s 1: see out_job_t */
    int p8_s[2];          /* see out_job_t */
    sa_site_call_t **calls_s[2];   /* see out_job_t */
    int64_t *n_calls_s[2];
} render_job_t;
static int64_t render_slice(render_job_t *job);

/* GPU stage of a slice; returns the rendering job (NULL: nothing left to render -- the expectations mode writes its files
 * here -- with the number of failed reads in *n_failed_now) */
/* --train-*: the assignments table (generate_top_n_kmers_from_sa_output) and the retrained models (train_normal_emmissions:
 * the prior is the -T / -C file as written on disk) */
static void write_training(run_t *R, const char *t_model, const char *c_model, int device) {
    const int n_strands = R->two_d ? 2 : 1;
    if (!(R->train_assign || R->train_model[0] || R->train_model[1])) return;
    for (int s = 0; s < n_strands; s++)   /* (a run without a read that aligned: empty tables) */
        if (!R->train_tab[s] && sa_kmer_table_create(&R->train_tab[s], (s ? &R->smc : &R->smt)->model, R->train_n, R->train_min_prob, device) != SA_OK)
            die("signalMachine: --train-*: no k-mer table%s", "");
    if (R->train_assign) {   /* the template table's 't' rows, then the complement table's 'c' rows */
        for (int s = 0; s < n_strands; s++)
            if (sa_kmer_table_write(R->train_tab[s], s, R->train_assign, s > 0) != SA_OK) die("signalMachine: cannot write %s", R->train_assign);
    }
    for (int s = 0; s < n_strands; s++) {
        if (!R->train_model[s]) continue;
        const strand_model_t *sm = s ? &R->smc : &R->smt;
        int64_t nk = 1;
        for (int i = 0; i < sm->k; i++) nk *= sm->n_alpha;
        sa_kmer_stat_t *st = calloc((size_t) nk, sizeof(sa_kmer_stat_t));
        uint8_t *mask = NULL;
        if (R->train_kmers) {   /* load_training_kmers (trainModels.py:704-719): a duplicate line is an error */
            FILE *f = fopen(R->train_kmers, "r");
            if (!f) die("signalMachine: cannot read %s", R->train_kmers);
            mask = calloc((size_t) nk, 1);
            char line[256];
            while (fgets(line, sizeof line, f)) {
                line[strcspn(line, "\r\n")] = 0;
                const int64_t id = (int64_t) strlen(line) == sm->k ? sa_kmer_id(sm->model, line) : -1;
                if (id < 0 || id >= nk) continue;   /* (a k-mer outside the model never matches, as in the reference) */
                if (mask[id]) die("signalMachine: --train-kmers: duplicate k-mer %s", line);
                mask[id] = 1;
            }
            fclose(f);
        }
        if (!st || sa_kmer_table_stats(R->train_tab[s], s, R->train_median, st, NULL) != SA_OK)
            die("signalMachine: --train-*: statistics failed%s", "");
        if (sa_model_write_trained(s ? c_model : t_model, st, R->train_weight, R->train_min_sd, R->train_mod_only, mask, R->train_model[s]) != SA_OK)
            die("signalMachine: cannot write %s", R->train_model[s]);
        free(st);
        free(mask);
    }
    for (int s = 0; s < 2; s++) { sa_kmer_table_destroy(R->train_tab[s]); R->train_tab[s] = NULL; }
}

/* One strand's batch of a slice.  jobs[i] belongs to reads[who[i / per_read]] (per_read > 1: --snp-step's substituted copies).
 * --emission twoDist: a single read brings its own model; the reads of a manifest share the strand's two-distribution model and
 * each job gets the scale_sd / var_sd its read's parameter estimation left (emissions_signal_scaleNoise, applied inside the batch:
 * SA_FLAG_TWO_DIST_ALL_KERNELS, whatever kernel family a read's regions take). */
static int create_strand_batch(sa_batch_t **b, const run_t *R, const strand_model_t *sm, const read_t *reads, const int64_t *who,
                               int strand, const sa_job_t *jobs, int64_t n_jobs, int64_t per_read, int device, unsigned flags) {
    if (!R->two_dist) return sa_batch_create(b, sm->model, &R->p, jobs, n_jobs, R->ambig, device, flags);
    if (!R->batch_mode) return sa_batch_create(b, reads[who[0]].model[strand], &R->p, jobs, n_jobs, R->ambig, device, flags);
    sa_noise_scale_t *nz = malloc(sizeof(sa_noise_scale_t) * (size_t) (n_jobs > 0 ? n_jobs : 1));
    if (!nz) return SA_ENOMEM;
    for (int64_t i = 0; i < n_jobs; i++) {
        const sa_npread_t *np = reads[who[i / per_read]].np;
        const sa_strand_params_t *pp = strand == 0 ? &np->template_params : &np->complement_params;
        nz[i].scale_sd = pp->scale_sd;
        nz[i].var_sd = pp->var_sd;
    }
    const int rc = sa_batch_create_noise_scaled(b, sm->model_two, &R->p, jobs, nz, n_jobs, R->ambig, device,
                                                flags | SA_FLAG_TWO_DIST_ALL_KERNELS);
    free(nz);
    return rc;
}

static render_job_t *run_slice(run_t *Rp, read_t *reads, int64_t n_reads, int batch_mode, int device, int64_t *n_failed_now) {
#define R (*Rp)
    *n_failed_now = 0;
    /* (the host side of the slice's reads has run: slice_prepare, a slice ahead of this function) */
    int64_t n_ok = 0;
    for (int64_t i = 0; i < n_reads; i++) n_ok += reads[i].failed ? 0 : 1;
    const double ts1 = now_s();
    const strand_model_t *sms[2] = {&R.smt, &R.smc};
    const int n_strands = R.two_d ? 2 : 1;

    /* ---- the pair-HMM on the GPU: one batch per strand model, all reads side by side ---- */
    sa_job_t *bj = malloc(sizeof(sa_job_t) * (size_t) (n_ok > 0 ? n_ok : 1));
    int64_t *who = malloc(sizeof(int64_t) * (size_t) (n_ok > 0 ? n_ok : 1));
    int64_t k = 0;
    for (int64_t i = 0; i < n_reads; i++)
        if (!reads[i].failed) who[k++] = i;

    if (R.expect_mode) { /* impl/signalMachine.c:772-848 */
        if (n_ok > 0) fprintf(stderr, "Starting expectations routine\n");
        for (int s = 0; s < n_strands && n_ok > 0; s++) {
            fprintf(stderr, "signalAlign - getting expectations for %s\n", s == 0 ? "template" : "complement");
            for (int64_t j = 0; j < n_ok; j++) bj[j] = reads[who[j]].jobs[s];
            double *trans = malloc(sizeof(double) * 9 * (size_t) n_ok), *lik = calloc((size_t) n_ok, sizeof(double));
            for (int64_t j = 0; j < 9 * n_ok; j++) trans[j] = 0.001; /* transitionsPseudocount, :785 */
            sa_assignment_t **as = calloc((size_t) n_ok, sizeof(*as));
            int64_t *n_as = calloc((size_t) n_ok, sizeof(int64_t));
            int rc = sa_expect_batch(sms[s]->model, &R.p, bj, n_ok, R.ambig, device, 0, trans, lik, as, n_as);
            if (rc != SA_OK) {
                fprintf(stderr, "signalMachine: expectations failed: %s\n", sa_strerror(rc));
                exit(1);
            }
            for (int64_t j = 0; j < n_ok; j++) {
                read_t *rd = &reads[who[j]];
                const char *path = s == 0 ? rd->t_expect : rd->c_expect;
                if (R.hdp)
                    fprintf(stderr, s == 0 ? "signalAlign - got %" PRId64 " template HDP assignments\n"
                                           : "signalAlign - got %" PRId64 "complement HDP assignments\n", n_as[j]);
                if (path != NULL) {
                    fprintf(stderr, "signalAlign - writing expectations to file: %s\n", path);
                    write_expectations(path, sms[s], s == 0 ? &rd->np->template_params : &rd->np->complement_params, R.hdp,
                                       R.p.threshold, trans + 9 * j, lik[j], &rd->jobs[s], as[j], n_as[j]);
                }
                sa_free(as[j]);
            }
            free(trans); free(lik); free(as); free(n_as);
        }
        for (int64_t j = 0; j < n_ok; j++)
            fprintf(stderr, "signalAlign - SUCCESS: finished alignment of query %s, exiting\n", reads[who[j]].label);
        free(bj); free(who);
        *n_failed_now = n_reads - n_ok;
        for (int64_t i = 0; i < n_reads; i++) release_read(&reads[i]);
        return NULL;
    }

    sa_pair_t **pairs_s[2] = {NULL, NULL};
    int64_t *n_pairs_s[2] = {NULL, NULL};
    sa_pair_t ***pairs = pairs_s;
    int64_t **n_pairs = n_pairs_s;
    sa_mea_pair_t **mea_s[2] = {NULL, NULL};
    int64_t *n_mea_s[2] = {NULL, NULL};
    sa_mea_pair_t ***mea = mea_s;
    int64_t **n_mea = n_mea_s;
    int validated = !batch_mode;   /* a single-read run has nobody to isolate a bad job from */
    sa_batch_t *batches[2] = {NULL, NULL};
    int64_t *all_n[2] = {NULL, NULL}, *all_sum[2] = {NULL, NULL};
    /* -s 1 prints only the rows whose reference k-mer holds an X: the others stay on the device (SA_FLAG_VC_ROWS), the run's pair
     * count and score come from the totals the device kept */
    /* --site-calls / --site-calls-aggregate: every batch records its sites (SA_FLAG_SITE_CALLS) and keeps every row (the calls are
     * made of the rows SA_FLAG_VC_ROWS would drop; -s 1 then filters on the host, write_vc) */
    const int want_calls = R.site_calls || R.agg_path != NULL;
    const unsigned calls_flag = want_calls ? SA_FLAG_SITE_CALLS : 0u;
    const int want_train = R.train_assign || R.train_model[0] || R.train_model[1];
    const unsigned vc_flag = (R.out_fmt == 1 && !R.mea && !want_calls && !want_train && !getenv("SA_CLI_VC_ON_HOST")) ? SA_FLAG_VC_ROWS : 0u;
    sa_site_call_t **calls_s[2] = {NULL, NULL};
    int64_t *n_calls_s[2] = {NULL, NULL};
    /* -s 0 / -s 2 without --mea: 8-byte result records where the batch allows them (one path per cell: no ambiguity letter in any
     * read's reference; fewer than 2^20 positions and events per read) -- the planner says SA_EUNSUPPORTED otherwise and the strand's
     * batch is made again with 16-byte records.  SA_CLI_PAIRS16=1: always 16-byte records (the test's checker). */
    const unsigned p8_want = ((R.out_fmt == 0 || R.out_fmt == 2) && !R.mea && !want_calls && !getenv("SA_CLI_PAIRS16")) ? SA_FLAG_PAIRS8 : 0u;
    int p8_used[2] = {0, 0};
    /* --train-*: each strand's rows go into the run's k-mer table right after its batch ran, while the records are still in HBM;
     * the tables are checkpointed here, so that the retry below (a read the planner refuses) can take the slice's rows back */
    for (int s = 0; s < n_strands && want_train; s++) {
        int rc = R.train_tab[s] ? SA_OK : sa_kmer_table_create(&R.train_tab[s], sms[s]->model, R.train_n, R.train_min_prob, device);
        if (rc == SA_OK) rc = sa_kmer_table_checkpoint(R.train_tab[s]);
        if (rc != SA_OK) {
            fprintf(stderr, "signalMachine: --train-*: %s\n", sa_strerror(rc));
            exit(1);
        }
    }
    for (int s = 0; s < n_strands; s++) {
        pairs[s] = calloc((size_t) (n_ok > 0 ? n_ok : 1), sizeof(sa_pair_t *));
        n_pairs[s] = calloc((size_t) (n_ok > 0 ? n_ok : 1), sizeof(int64_t));
        if (n_ok == 0) continue;
        fprintf(stderr, s == 0 ? "signalAlign - starting template alignment\n" : "signalAlign - starting complement alignment\n");
        for (int64_t j = 0; j < n_ok; j++) bj[j] = reads[who[j]].jobs[s];
        if (want_calls) {
            calls_s[s] = calloc((size_t) n_ok, sizeof(sa_site_call_t *));
            n_calls_s[s] = calloc((size_t) n_ok, sizeof(int64_t));
        }
        int rc;
        if (!R.mea) {   /* the batch stays alive for the rendering, which expands its packed records job by job */
            sa_batch_t *b = NULL;
            rc = create_strand_batch(&b, &R, sms[s], reads, who, s, bj, n_ok, 1, device, vc_flag | p8_want | calls_flag);
            p8_used[s] = rc == SA_OK && p8_want != 0;
            if (rc == SA_EUNSUPPORTED && p8_want)
                rc = create_strand_batch(&b, &R, sms[s], reads, who, s, bj, n_ok, 1, device, vc_flag);
            if (rc == SA_OK) rc = sa_batch_run(b);
            if (rc == SA_OK && want_calls) rc = sa_batch_site_calls(b, 0, calls_s[s], n_calls_s[s], NULL);
            if (rc == SA_OK && want_train) {
                rc = sa_kmer_table_add_batch(R.train_tab[s], b, bj, n_ok, s, NULL);
                if (rc != SA_OK) {   /* (a batch that ran: nothing a retry without some reads would change) */
                    fprintf(stderr, "signalMachine: --train-*: %s\n", sa_strerror(rc));
                    exit(1);
                }
            }
            for (int64_t j = 0; j < n_ok && rc == SA_OK; j++) rc = sa_batch_n_pairs(b, j, &n_pairs[s][j]);
            if (vc_flag && rc == SA_OK) {
                free(all_n[s]); free(all_sum[s]);
                all_n[s] = calloc((size_t) n_ok, sizeof(int64_t));
                all_sum[s] = calloc((size_t) n_ok, sizeof(int64_t));
                for (int64_t j = 0; j < n_ok && rc == SA_OK; j++) rc = sa_batch_all_pairs_summary(b, j, &all_n[s][j], &all_sum[s][j]);
            }
            /* only the packed pairs (pinned host memory) are read from here on: the batch's HBM goes back now, so that the
             * complement strand's batch plans into the whole card */
            if (rc == SA_OK) rc = sa_batch_release_device(b);
            if (rc == SA_OK) batches[s] = b;
            else sa_batch_destroy(b);
        } else { /* the same batch, kept alive for the path step: its pairs are still on the device */
            sa_batch_t *b = NULL;
            mea[s] = calloc((size_t) n_ok, sizeof(sa_mea_pair_t *));
            n_mea[s] = calloc((size_t) n_ok, sizeof(int64_t));
            rc = create_strand_batch(&b, &R, sms[s], reads, who, s, bj, n_ok, 1, device, calls_flag);
            if (rc == SA_OK) rc = sa_batch_run(b);
            if (rc == SA_OK && want_calls) rc = sa_batch_site_calls(b, 0, calls_s[s], n_calls_s[s], NULL);
            for (int64_t j = 0; j < n_ok && rc == SA_OK; j++) {
                sa_batch_n_pairs(b, j, &n_pairs[s][j]);
                pairs[s][j] = malloc(sizeof(sa_pair_t) * (size_t) (n_pairs[s][j] > 0 ? n_pairs[s][j] : 1));
                rc = sa_batch_pairs(b, j, pairs[s][j], n_pairs[s][j]);
            }
            if (rc == SA_OK) rc = sa_batch_mea(b, 0, mea[s], n_mea[s], NULL, NULL, NULL);
            sa_batch_destroy(b);
        }
        if (!validated && rc != SA_OK && rc != SA_ENODEVICE && rc != SA_ENOMEM) {
            /* the planner turned the batch down (a letter outside the alphabet, anchors that give no band, a cell of more paths
             * or a matrix larger than the result records can name -- SA_EUNSUPPORTED --, ...): find the reads whose jobs it
             * rejects (each planned alone on the host, all host threads), let them fail alone as the reference's
             * one-process-per-read runs would, and start over.  Only when no read is to blame does the run end below. */
            validated = 1;
            validate_ctx_t vc = {&R, reads, who};
            parallel_for(n_ok, validate_one, &vc);
            int64_t k2 = 0;
            for (int64_t j = 0; j < n_ok; j++)
                if (!reads[who[j]].failed) who[k2++] = who[j];
            if (k2 < n_ok) {
                for (int q = 0; q < n_strands && want_train; q++)
                    if (sa_kmer_table_rollback(R.train_tab[q]) != SA_OK) die("signalMachine: --train-*: rollback failed%s", "");
                for (int q = 0; q <= s; q++) {
                    sa_batch_destroy(batches[q]);
                    batches[q] = NULL;
                    for (int64_t j = 0; j < n_ok; j++) { sa_free(pairs[q][j]); if (R.mea && mea[q]) sa_free(mea[q][j]); }
                    free(pairs[q]); free(n_pairs[q]);
                    if (R.mea) { free(mea[q]); free(n_mea[q]); mea[q] = NULL; n_mea[q] = NULL; }
                    if (calls_s[q]) {
                        for (int64_t j = 0; j < n_ok; j++) sa_free(calls_s[q][j]);
                        free(calls_s[q]); free(n_calls_s[q]); calls_s[q] = NULL; n_calls_s[q] = NULL;
                    }
                    pairs[q] = NULL; n_pairs[q] = NULL;
                }
                n_ok = k2;
                s = -1;   /* both strands again, without the offenders */
                continue;
            }
        }
        if (rc != SA_OK) {
            fprintf(stderr, "signalMachine: alignment failed: %s\n", sa_strerror(rc));
            exit(1);
        }
    }

    /* ---- outputs: rendered in parallel (one file per read), summary lines in read order ---- */
    g_t_gpu += now_s() - ts1;
    render_job_t *job = calloc(1, sizeof(*job));
    job->Rp = Rp; job->reads = reads; job->n_reads = n_reads; job->n_ok = n_ok; job->who = who; job->bj = bj;
    for (int s = 0; s < 2; s++) { job->pairs_s[s] = pairs[s]; job->n_pairs_s[s] = n_pairs[s]; job->mea_s[s] = mea[s]; job->n_mea_s[s] = n_mea[s]; job->batch[s] = batches[s]; job->all_n_s[s] = all_n[s]; job->all_sum_s[s] = all_sum[s]; job->p8_s[s] = p8_used[s];
                              job->calls_s[s] = calls_s[s]; job->n_calls_s[s] = n_calls_s[s]; }
    return job;
#undef R
}

/* rendering of a slice (one file per read, in parallel), summary lines in read order, then the reads' memory goes back;
 * returns the number of the slice's reads that failed */
static int64_t render_slice(render_job_t *job) {
    run_t *Rp = job->Rp;
#define R (*Rp)
    read_t *reads = job->reads;
    const int64_t n_reads = job->n_reads, n_ok = job->n_ok;
    int64_t *who = job->who;
    sa_job_t *bj = job->bj;
    sa_pair_t ***pairs = job->pairs_s;
    int64_t **n_pairs = job->n_pairs_s;
    sa_mea_pair_t ***mea = job->mea_s;
    int64_t **n_mea = job->n_mea_s;
    const int n_strands = R.two_d ? 2 : 1;
    const double ts2 = now_s();
    double (*score)[2] = calloc((size_t) (n_ok > 0 ? n_ok : 1), sizeof(*score));
    unsigned char *tmpl_amb = (R.two_d && job->calls_s[1]) ? calloc((size_t) (n_ok > 0 ? n_ok : 1), 1) : NULL;
    {
        out_job_t oc = {&R, reads, who, pairs, n_pairs, score, mea, n_mea, job->batch, job->all_n_s, job->all_sum_s, job->p8_s,
                        job->calls_s, job->n_calls_s, tmpl_amb};
        if (outputs_distinct(reads, who, n_ok)) parallel_for(n_ok, output_one, &oc);
        else for (int64_t j = 0; j < n_ok; j++) output_one(j, &oc);
    }
    for (int s = 0; s < 2; s++) { sa_batch_destroy(job->batch[s]); job->batch[s] = NULL; }
    if (R.agg_path)   /* (in read order: the sums over reads do not depend on the rendering threads) */
        for (int64_t j = 0; j < n_ok; j++)
            for (int s = 0; s < n_strands && !reads[who[j]].failed; s++)
                agg_add_read(&reads[who[j]], s, tmpl_amb && tmpl_amb[j], job->calls_s[s][j], job->n_calls_s[s][j],
                             s == 0 ? R.smt.k : R.smc.k);
    for (int64_t j = 0; j < n_ok; j++) {
        read_t *rd = &reads[who[j]];
        if (rd->failed) continue;
        fprintf(stdout, "%s %" PRId64 "\t%" PRId64 "(%f)\t", rd->label, rd->n_guide, job->all_n_s[0] ? job->all_n_s[0][j] : n_pairs[0][j], score[j][0]);
        if (R.two_d) fprintf(stdout, "%" PRId64 "(%f)\n", job->all_n_s[1] ? job->all_n_s[1][j] : n_pairs[1][j], score[j][1]);
        else fprintf(stdout, "\n");
        fprintf(stderr, "signalAlign - SUCCESS: finished alignment of query %s, exiting\n", rd->label);
        for (int s = 0; s < n_strands; s++) {
            sa_free(pairs[s][j]);
            if (R.mea) sa_free(mea[s][j]);
        }
    }
    free(tmpl_amb);
    for (int s = 0; s < n_strands; s++)
        if (job->calls_s[s]) {
            for (int64_t j = 0; j < n_ok; j++) sa_free(job->calls_s[s][j]);
            free(job->calls_s[s]); free(job->n_calls_s[s]);
        }
    t_add(&g_t_render, now_s() - ts2);
    int64_t n_failed = 0;
    for (int64_t i = 0; i < n_reads; i++) n_failed += reads[i].failed ? 1 : 0;
    for (int s = 0; s < n_strands; s++) { free(pairs[s]); free(n_pairs[s]); free(job->all_n_s[s]); free(job->all_sum_s[s]); if (R.mea) { free(mea[s]); free(n_mea[s]); } }
    free(score); free(bj); free(who);
    for (int64_t i = 0; i < n_reads; i++) release_read(&reads[i]);
    return n_failed;
#undef R
}

/* what a read holds once its outputs are written */
static void release_read(read_t *rd) {
    if (rd->pA) sa_cigar_free(rd->pA);
    if (rd->np) sa_npread_free(rd->np);
    free(rd->forward_seq); free(rd->backward_seq);
    for (int s = 0; s < 2; s++) { free(rd->ax[s]); free(rd->ay[s]); rd->ax[s] = rd->ay[s] = NULL; }
    for (int s = 0; s < 2; s++) { if (rd->model[s]) sa_model_destroy(rd->model[s]); rd->model[s] = NULL; }
    rd->pA = NULL; rd->np = NULL; rd->forward_seq = rd->backward_seq = NULL;
}

/* ---- --snp-step N --snp-dir DIR: single-nucleotide probabilities (singleNucleotideProbabilities.py:551-723) ----
 * Every read strand becomes N jobs in one batch: job s aligns the read to its window with X at the contig positions = s (mod N)
 * (replace_periodic_reference_positions; the default ambiguity table makes X the four bases).  sa_batch_position_calls folds
 * the rows of every X position on the device (CallMethylation.call_methyls); the N step files of a read are merged into
 * DIR/<label>.tsv (discover_single_nucleotide_probabilities).  fast5_input names the .npRead: the one deliberate difference. */
typedef struct {
    const run_t *run;
    read_t *reads;
    const int64_t *who;
    int64_t N;
    sa_position_call_t **calls[2];   /* [strand][read * N + step] */
    int64_t *n_calls[2];
    int32_t *x_min[2], *x_max[2];
} snp_out_t;

/* contig coordinate of index t of a strand's target (the TSV's reference_index of a k-mer at t covers t .. t + k - 1) */
static int64_t snp_contig_pos(const read_t *rd, int s, int64_t t) {
    const int64_t off = s == 0 ? rd->r_shift_t : rd->r_shift_c;
    const int same = (s == 0 && rd->forward) || (s == 1 && !rd->forward);
    return same ? off + t : off - 1 - t;
}

static void snp_output_one(int64_t j, void *ctx) {
    snp_out_t *c = ctx;
    const run_t *R = c->run;
    read_t *rd = &c->reads[c->who[j]];
    const int n_strands = R->two_d ? 2 : 1;
    int64_t cap = 0;
    for (int64_t s = 0; s < c->N; s++)
        for (int q = 0; q < n_strands; q++) cap += c->n_calls[q][j * c->N + s];
    sa_snp_site_t *sites = malloc(sizeof(sa_snp_site_t) * (size_t) (cap > 0 ? cap : 1));
    if (!sites) die("signalMachine: out of memory%s", "");
    int64_t n = 0;
    for (int64_t s = 0; s < c->N; s++) {   /* one step file after the other */
        const int64_t js = j * c->N + s;
        /* the window of call_methyls (:160-169) over the reference_index of every row of the step's file, both strands */
        int64_t lo_ref = INT64_MAX, hi_ref = INT64_MIN;
        for (int q = 0; q < n_strands; q++) {
            if (c->x_min[q][js] < 0) continue;
            const int k = q == 0 ? R->smt.k : R->smc.k;
            const char *target = q == 0 ? rd->template_target : rd->complement_target;
            const int64_t len = (int64_t) strlen(target), off = q == 0 ? rd->r_shift_t : rd->r_shift_c;
            const int64_t a = adjust_ref(c->x_min[q][js], off, len - k, len, q == 0, rd->forward);
            const int64_t b = adjust_ref(c->x_max[q][js], off, len - k, len, q == 0, rd->forward);
            lo_ref = a < lo_ref ? a : lo_ref; lo_ref = b < lo_ref ? b : lo_ref;
            hi_ref = a > hi_ref ? a : hi_ref; hi_ref = b > hi_ref ? b : hi_ref;
        }
        if (lo_ref > hi_ref) continue;   /* no row at all: the reference's step file cannot be parsed and is missing */
        int64_t w_lo = 0, w_hi = 0;
        sa_snp_site_window(lo_ref, hi_ref, c->N, &w_lo, &w_hi);
        for (int q = 0; q < n_strands; q++) {   /* template sites, then complement sites, each ascending */
            const sa_position_call_t *pc = c->calls[q][js];
            const int64_t m = c->n_calls[q][js];
            const int same = (q == 0 && rd->forward) || (q == 1 && !rd->forward);
            for (int64_t i0 = 0; i0 < m; i0++) {
                const sa_position_call_t *p = &pc[same ? i0 : m - 1 - i0];
                const int64_t pos = snp_contig_pos(rd, q, p->p);
                if (pos < w_lo || pos >= w_hi) continue;
                sa_snp_site_t *o = &sites[n++];
                o->pos = pos;
                o->strand = q;
                o->pad = 0;
                for (int l = 0; l < 4; l++) {
                    o->p[l] = 0.0;
                    for (int e = 0; e < p->n_letters; e++)
                        if (p->letters[e] == "ACGT"[l]) o->p[l] = p->prob[e];
                }
            }
        }
    }
    const char *np_name = strrchr(rd->npread_path, '/') ? strrchr(rd->npread_path, '/') + 1 : rd->npread_path;
    char *path = malloc(strlen(R->snp_dir) + strlen(rd->label) + 8);
    sprintf(path, "%s/%s.tsv", R->snp_dir, rd->label);
    if (sa_snp_write_read(path, np_name, rd->label, rd->pA->contig1, !rd->forward, sites, n) != SA_OK)
        die("signalMachine: cannot write %s", path);
    free(path);
    free(sites);
}

/* plans every substituted job of a read alone on the host (validate_read for the N copies) */
typedef struct { const run_t *R; read_t *reads; const int64_t *who; sa_job_t *const *jobs; int64_t N; } snp_validate_t;
static void snp_validate_one(int64_t j, void *ctx) {
    snp_validate_t *v = ctx;
    read_t *rd = &v->reads[v->who[j]];
    for (int q = 0; q < (v->R->two_d ? 2 : 1) && !rd->failed; q++)
        for (int64_t s = 0; s < v->N && !rd->failed; s++) {
            const int rc = sa_plan_describe(q == 0 ? v->R->smt.model : v->R->smc.model, &v->R->p, &v->jobs[q][j * v->N + s], v->R->ambig,
                                            0, NULL, NULL, 0, NULL, 0, NULL, 0);
            if (rc != SA_OK) fail(rd, 0, "alignment job rejected: %s", sa_strerror(rc));
        }
    if (rd->failed) fprintf(stderr, "[signalMachine] ERROR: read %s skipped: %s\n", rd->label, rd->err);
}

/* GPU stage and outputs of a slice in --snp-step mode; returns the number of the slice's reads that failed */
static int64_t run_slice_snp(run_t *Rp, read_t *reads, int64_t n_reads, int batch_mode, int device) {
#define R (*Rp)
    const int n_strands = R.two_d ? 2 : 1;
    const int64_t N = R.snp_step;
    const strand_model_t *sms[2] = {&R.smt, &R.smc};
    const double ts1 = now_s();
    int64_t *who = malloc(sizeof(int64_t) * (size_t) (n_reads > 0 ? n_reads : 1));
    int64_t n_ok = 0;
    for (int64_t i = 0; i < n_reads; i++)
        if (!reads[i].failed) who[n_ok++] = i;
    /* the substituted targets: read j, step s, strand q at tgt[q][j * N + s] */
    char **tgt[2] = {NULL, NULL};
    sa_job_t *jobs[2] = {NULL, NULL};
    const size_t nj_all = (size_t) (n_ok > 0 ? n_ok : 1) * (size_t) N;
    for (int q = 0; q < n_strands; q++) {
        tgt[q] = calloc(nj_all, sizeof(char *));
        jobs[q] = calloc(nj_all, sizeof(sa_job_t));
        if (!tgt[q] || !jobs[q]) die("signalMachine: out of memory%s", "");
    }
    for (int64_t j = 0; j < n_ok; j++) {
        read_t *rd = &reads[who[j]];
        const int64_t hi = rd->win_lo + (int64_t) strlen(rd->forward_seq) - 1;
        for (int q = 0; q < n_strands; q++) {
            const char *t = q == 0 ? rd->template_target : rd->complement_target;
            const int from_fwd = t == rd->forward_seq;   /* forward_seq[i] at win_lo + i, backward_seq[i] at hi - i */
            const int64_t len = (int64_t) strlen(t);
            for (int64_t s = 0; s < N; s++) {
                char *o = malloc((size_t) len + 1);
                if (!o) die("signalMachine: out of memory%s", "");
                sa_snp_substitute(t, len, from_fwd ? rd->win_lo : hi, !from_fwd, N, s, 'X', o);
                tgt[q][j * N + s] = o;
                jobs[q][j * N + s] = rd->jobs[q];
                jobs[q][j * N + s].ref = o;
            }
        }
    }
    snp_out_t oc;
    memset(&oc, 0, sizeof(oc));
    oc.run = Rp; oc.reads = reads; oc.who = who; oc.N = N;
    int64_t *n_pairs[2] = {NULL, NULL}, *sum_e7[2] = {NULL, NULL};
    int validated = !batch_mode;
    for (int q = 0; q < n_strands; q++) {
        const int64_t nj = n_ok * N;
        oc.calls[q] = calloc(nj_all, sizeof(sa_position_call_t *));
        oc.n_calls[q] = calloc(nj_all, sizeof(int64_t));
        oc.x_min[q] = calloc(nj_all, sizeof(int32_t));
        oc.x_max[q] = calloc(nj_all, sizeof(int32_t));
        n_pairs[q] = calloc(nj_all, sizeof(int64_t));
        sum_e7[q] = calloc(nj_all, sizeof(int64_t));
        if (nj == 0) continue;
        fprintf(stderr, q == 0 ? "signalAlign - starting template alignment\n" : "signalAlign - starting complement alignment\n");
        sa_batch_t *b = NULL;
        int rc = create_strand_batch(&b, &R, sms[q], reads, who, q, jobs[q], nj, N, device, SA_FLAG_POSITION_CALLS);
        if (rc == SA_OK) rc = sa_batch_run(b);
        if (rc == SA_OK) rc = sa_batch_position_calls(b, 0, oc.calls[q], oc.n_calls[q], oc.x_min[q], oc.x_max[q], NULL);
        for (int64_t i = 0; i < nj && rc == SA_OK; i++) rc = sa_batch_all_pairs_summary(b, i, &n_pairs[q][i], &sum_e7[q][i]);
        sa_batch_destroy(b);
        if (!validated && rc != SA_OK && rc != SA_ENODEVICE && rc != SA_ENOMEM) {
            /* the planner turned the batch down: the reads whose substituted jobs it rejects fail alone, the rest start over */
            validated = 1;
            snp_validate_t vc = {&R, reads, who, jobs, N};
            parallel_for(n_ok, snp_validate_one, &vc);
            /* the slice closes up: a refused read's targets are freed, a kept read's move down to its new place and leave
             * their old slots empty, so that every target is owned by exactly one slot of tgt */
            int64_t k2 = 0;
            for (int64_t j = 0; j < n_ok; j++) {
                const int refused = reads[who[j]].failed;
                for (int q2 = 0; q2 < n_strands; q2++)
                    for (int64_t s = 0; s < N; s++) {
                        char **src = &tgt[q2][j * N + s];
                        if (refused) {
                            free(*src);
                            *src = NULL;
                        } else if (k2 != j) {
                            tgt[q2][k2 * N + s] = *src;
                            jobs[q2][k2 * N + s] = jobs[q2][j * N + s];
                            *src = NULL;
                        }
                    }
                if (!refused) who[k2++] = who[j];
            }
            if (k2 < n_ok) {
                for (int q2 = 0; q2 <= q; q2++) {
                    for (size_t i = 0; i < nj_all; i++) sa_free(oc.calls[q2][i]);
                    free(oc.calls[q2]); free(oc.n_calls[q2]); free(oc.x_min[q2]); free(oc.x_max[q2]);
                    free(n_pairs[q2]); free(sum_e7[q2]);
                    oc.calls[q2] = NULL; oc.n_calls[q2] = NULL; oc.x_min[q2] = oc.x_max[q2] = NULL;
                    n_pairs[q2] = sum_e7[q2] = NULL;
                }
                n_ok = k2;
                q = -1;   /* both strands again, without the offenders */
                continue;
            }
        }
        if (rc != SA_OK) {
            fprintf(stderr, "signalMachine: alignment failed: %s\n", sa_strerror(rc));
            exit(1);
        }
    }
    g_t_gpu += now_s() - ts1;
    const double ts2 = now_s();
    parallel_for(n_ok, snp_output_one, &oc);
    /* the summary lines of the N -s 0 runs of every read, step after step */
    for (int64_t j = 0; j < n_ok; j++) {
        read_t *rd = &reads[who[j]];
        for (int64_t s = 0; s < N; s++) {
            const int64_t js = j * N + s;
            double score[2];
            for (int q = 0; q < n_strands; q++)
                score[q] = 100.0 * (double) sum_e7[q][js] / ((double) n_pairs[q][js] * PROB_1);
            fprintf(stdout, "%s %" PRId64 "\t%" PRId64 "(%f)\t", rd->label, rd->n_guide, n_pairs[0][js], score[0]);
            if (R.two_d) fprintf(stdout, "%" PRId64 "(%f)\n", n_pairs[1][js], score[1]);
            else fprintf(stdout, "\n");
            fprintf(stderr, "signalAlign - SUCCESS: finished alignment of query %s, exiting\n", rd->label);
        }
    }
    t_add(&g_t_render, now_s() - ts2);
    for (int q = 0; q < n_strands; q++) {
        for (size_t i = 0; i < nj_all; i++) { sa_free(oc.calls[q] ? oc.calls[q][i] : NULL); free(tgt[q][i]); }
        free(oc.calls[q]); free(oc.n_calls[q]); free(oc.x_min[q]); free(oc.x_max[q]);
        free(n_pairs[q]); free(sum_e7[q]); free(tgt[q]); free(jobs[q]);
    }
    free(who);
    int64_t n_failed = 0;
    for (int64_t i = 0; i < n_reads; i++) n_failed += reads[i].failed ? 1 : 0;
    for (int64_t i = 0; i < n_reads; i++) release_read(&reads[i]);
    return n_failed;
#undef R
}

int main(int argc, char **argv) {
    run_t R;
    memset(&R, 0, sizeof(R));
    R.train_min_prob = 0.8;   /* probability_threshold, number_of_kmer_assignments, og_model_weight (trainModels.py) */
    R.train_n = 10;
    R.train_weight = 100.0;
    int64_t diag_expansion = 50, trace_back = 50, batch_reads = 2048;
    double threshold = 0.01;
    int device = 0; /* --device: which GPU of the node (one process per GPU; reads shard across processes) */
    int snp_set = 0;
    R.constraint_trim = 14;
    char *t_model = NULL, *c_model = NULL, *label = NULL, *npread_path = NULL, *cigar_path = NULL, *post_path = NULL;
    char *t_expect = NULL, *c_expect = NULL, *t_hdp = NULL, *c_hdp = NULL, *fwd_ref = NULL, *bwd_ref = NULL,
         *post_path2 = NULL, *seq_name = NULL, *ambig_model = NULL, *manifest = NULL;
    static struct option long_options[] = {{"help", no_argument, 0, 'h'},
                                           {"sm3Hdp", no_argument, 0, 'd'},
                                           {"sparse_output", no_argument, 0, 's'},
                                           {"twoD", no_argument, 0, 'e'},
                                           {"rna", no_argument, 0, 'r'},
                                           {"templateModel", required_argument, 0, 'T'},
                                           {"complementModel", required_argument, 0, 'C'},
                                           {"readLabel", required_argument, 0, 'L'},
                                           {"npRead", required_argument, 0, 'q'},
                                           {"exonerate_cigar_file", required_argument, 0, 'p'},
                                           {"posteriors", required_argument, 0, 'u'},
                                           {"templateHdp", required_argument, 0, 'v'},
                                           {"complementHdp", required_argument, 0, 'w'},
                                           {"templateExpectations", required_argument, 0, 't'},
                                           {"complementExpectations", required_argument, 0, 'c'},
                                           {"diagonalExpansion", required_argument, 0, 'x'},
                                           {"threshold", required_argument, 0, 'D'},
                                           {"constraintTrim", required_argument, 0, 'm'},
                                           {"forward_reference_path", required_argument, 0, 'f'},
                                           {"backward_reference_path", optional_argument, 0, 'b'},
                                           {"sequence_name", required_argument, 0, 'n'},
                                           {"traceBackDiagonals", optional_argument, 0, 'g'},
                                           {"posteriorProbsFile2", optional_argument, 0, 'i'},
                                           {"ambig_model", optional_argument, 0, 'a'},
                                           {"batch", required_argument, 0, 1000},
                                           {"device", required_argument, 0, 1001},
                                           {"mea", no_argument, 0, 1002},
                                           {"batch-reads", required_argument, 0, 1003},
                                           {"emission", required_argument, 0, 1004},
                                           {"site-calls", no_argument, 0, 1005},
                                           {"site-calls-aggregate", required_argument, 0, 1006},
                                           {"train-assignments", required_argument, 0, 1010},
                                           {"train-template-model", required_argument, 0, 1011},
                                           {"train-complement-model", required_argument, 0, 1012},
                                           {"train-min-prob", required_argument, 0, 1013},
                                           {"train-max-assignments", required_argument, 0, 1014},
                                           {"train-weight", required_argument, 0, 1015},
                                           {"train-min-sd", required_argument, 0, 1016},
                                           {"train-median", no_argument, 0, 1017},
                                           {"train-mod-only", no_argument, 0, 1018},
                                           {"train-kmers", required_argument, 0, 1019},
                                           {"snp-step", required_argument, 0, 1020},
                                           {"snp-dir", required_argument, 0, 1021},
                                           {0, 0, 0, 0}};
    for (;;) {
        int idx = 0;
        int key = getopt_long(argc, argv, "h:d:e:s:r:o:a:T:C:a:L:q:f:b:g:i:p:u:v:w:t:c:x:D:m:n:", long_options, &idx);
        if (key == -1) break;
        switch (key) {
            case 'h': usage(); return 1;
            case 's': if (optarg) sscanf(optarg, "%" SCNd64, &R.out_fmt); break;
            case 'e': R.two_d = 1; break;
            case 'a': ambig_model = optarg ? strdup(optarg) : NULL; break;
            case 'r': R.rna = 1; break;
            case 'd': R.hdp = 1; break;
            case 'T': t_model = strdup(optarg); break;
            case 'C': c_model = strdup(optarg); break;
            case 'L': label = strdup(optarg); break;
            case 'q': npread_path = strdup(optarg); break;
            case 'p': cigar_path = strdup(optarg); break;
            case 'u': post_path = strdup(optarg); break;
            case 't': t_expect = strdup(optarg); break;
            case 'c': c_expect = strdup(optarg); break;
            case 'v': t_hdp = strdup(optarg); break;
            case 'w': c_hdp = strdup(optarg); break;
            case 'x': sscanf(optarg, "%" SCNd64, &diag_expansion); break;
            case 'D': sscanf(optarg, "%lf", &threshold); break;
            case 'm': sscanf(optarg, "%" SCNd64, &R.constraint_trim); break;
            case 'f': fwd_ref = strdup(optarg); break;
            case 'b': bwd_ref = optarg ? strdup(optarg) : NULL; break;
            case 'n': seq_name = strdup(optarg); break;
            case 'g': if (optarg) sscanf(optarg, "%" SCNd64, &trace_back); break;
            case 'i': post_path2 = optarg ? strdup(optarg) : NULL; break;
            case 1000: manifest = strdup(optarg); break;
            case 1001: device = atoi(optarg); break;
            case 1002: R.mea = 1; break;
            case 1005: R.site_calls = 1; break;
            case 1006: R.agg_path = strdup(optarg); break;
            case 1010: R.train_assign = strdup(optarg); break;
            case 1011: R.train_model[0] = strdup(optarg); break;
            case 1012: R.train_model[1] = strdup(optarg); break;
            case 1013: R.train_min_prob = atof(optarg); break;
            case 1014: R.train_n = atoll(optarg); break;
            case 1015: R.train_weight = atof(optarg); break;
            case 1016: R.train_min_sd = atof(optarg); break;
            case 1017: R.train_median = 1; break;
            case 1018: R.train_mod_only = 1; break;
            case 1019: R.train_kmers = strdup(optarg); break;
            case 1020:
                snp_set = 1;
                if (sscanf(optarg, "%" SCNd64, &R.snp_step) != 1) R.snp_step = 0;
                break;
            case 1021: R.snp_dir = strdup(optarg); break;
            case 1003: batch_reads = atoll(optarg) > 0 ? atoll(optarg) : batch_reads; break;
            case 1004:
                if (!strcmp(optarg, "twoDist")) R.two_dist = 1;
                else if (strcmp(optarg, "meanOnly")) die("signalMachine: --emission takes meanOnly or twoDist, not %s", optarg);
                break;
            default: usage(); return 1;
        }
    }
    if (!label) label = strdup("");
    if (t_model == NULL || (c_model == NULL && R.two_d)) die("Missing model files, exiting", NULL);
    if (R.out_fmt == 3 && post_path2 == NULL && manifest == NULL) die("Must pass in posteriorProbsFile2 if using 'both' outFmt", NULL);
    if (cigar_path == NULL && manifest == NULL) die("[signalMachine]ERROR: Need to provide input guide alignments, exiting", NULL);
    R.fwd_ref = fwd_ref;
    R.bwd_ref = bwd_ref;

    /* the reads of this run */
    read_t *reads = NULL;
    int64_t n_reads = 0;
    const int batch_mode = manifest != NULL;
    R.batch_mode = batch_mode;
    if (batch_mode) {
        n_reads = load_manifest(manifest, &reads);
        if (n_reads < 0) die("[signalMachine]ERROR: cannot read the batch manifest %s", manifest);
        for (int64_t i = 0; i < n_reads; i++) {
            if (reads[i].seq_name == NULL && seq_name != NULL) reads[i].seq_name = strdup(seq_name);
            if (reads[i].t_expect != NULL || reads[i].c_expect != NULL) R.expect_mode = 1;
        }
        if (R.expect_mode)
            for (int64_t i = 0; i < n_reads; i++)
                if (reads[i].t_expect == NULL && reads[i].c_expect == NULL)
                    die("[signalMachine]ERROR: batch manifest mixes expectation and alignment reads (%s)", reads[i].label);
    } else {
        reads = calloc(1, sizeof(read_t));
        n_reads = 1;
        reads[0].label = label; reads[0].npread_path = npread_path; reads[0].cigar_path = cigar_path;
        reads[0].post_path = post_path; reads[0].post_path2 = post_path2; reads[0].seq_name = seq_name;
        reads[0].t_expect = t_expect; reads[0].c_expect = c_expect;
        R.expect_mode = t_expect != NULL || c_expect != NULL;
        if (fwd_ref == NULL || seq_name == NULL) {
            /* the reference needs -n; kept after the cigar check so that the error order matches (impl/signalMachine.c:642-663) */
            sa_cigar_t *probe = NULL;
            if (sa_cigar_load(cigar_path, &probe) != SA_OK)
                die("[signalMachine]ERROR: Didn't find input alignment file, looked %s", cigar_path);
            sa_cigar_free(probe);
            die("[signalMachine] ERROR: need -f <fasta> and -n <sequence name>", NULL);
        }
    }
    /* (the expectation pass keeps the reference-ordered kernels and the model's own noise; an HDP model has no such emission) */
    if (R.two_dist && (R.hdp || t_hdp != NULL || c_hdp != NULL || R.expect_mode || t_expect != NULL || c_expect != NULL))
        die("signalMachine: --emission twoDist aligns reads with a Gaussian model: not with an .nhdp, not with -t / -c%s", "");

    if (R.train_assign || R.train_model[0] || R.train_model[1]) {
        if (R.expect_mode || R.mea) die("signalMachine: --train-* needs the alignment mode without --mea%s", "");
        if (R.train_model[1] && !R.two_d) die("signalMachine: --train-complement-model needs a 2-D run%s", "");
        if (R.train_n < 1 || !(R.train_min_prob >= 0 && R.train_min_prob <= 1)) die("signalMachine: bad --train-max-assignments / --train-min-prob%s", "");
    }
    if (R.expect_mode && (R.site_calls || R.agg_path)) { usage(); die("signalMachine: --site-calls / --site-calls-aggregate need the alignment mode, not -t/-c%s", ""); }
    if (snp_set || R.snp_dir) {   /* --snp-step: its own outputs only */
        if (!snp_set || R.snp_step < 1) { usage(); die("signalMachine: --snp-step takes a step N >= 1%s", ""); }
        if (!R.snp_dir) { usage(); die("signalMachine: --snp-step needs --snp-dir <directory>%s", ""); }
        if (R.expect_mode) { usage(); die("signalMachine: --snp-step cannot be combined with -t/-c%s", ""); }
        if (R.mea) { usage(); die("signalMachine: --snp-step cannot be combined with --mea%s", ""); }
        if (R.site_calls || R.agg_path) { usage(); die("signalMachine: --snp-step cannot be combined with --site-calls / --site-calls-aggregate%s", ""); }
        if (R.train_assign || R.train_model[0] || R.train_model[1]) { usage(); die("signalMachine: --snp-step cannot be combined with --train-*%s", ""); }
        for (int64_t i = 0; i < n_reads; i++)
            if (reads[i].post_path || reads[i].post_path2) {
                usage();
                die(batch_mode ? "signalMachine: --snp-step writes no posteriors file: the manifest's posteriors column of %s must be '-'"
                               : "signalMachine: --snp-step writes no posteriors file: -u / -i not allowed%s", batch_mode ? reads[i].label : "");
            }
    }

    R.p.threshold = threshold;
    R.p.diagonal_expansion = diag_expansion % 2 == 0 ? diag_expansion : diag_expansion + 1;
    R.p.trace_back_diagonals = trace_back;
    R.p.min_diags_between_trace_back = 1000;
    R.p.split_matrix_bigger_than_this = (int64_t) 3000 * 3000;

    if (t_hdp != NULL || c_hdp != NULL) {
        if (t_hdp == NULL || (c_hdp == NULL && R.two_d)) die("Need to have template and complement HDPs", NULL);
        if (!R.hdp) {
            R.hdp = 1;
            fprintf(stderr, "[signalAlign] - Using threeStateHdp stateMachine since you pass in an HDP file\n");
        } else {
            fprintf(stderr, "[signalAlign] - using NanoporeHDPs\n");
        }
    }
    if (R.hdp && t_hdp == NULL) die("signalAlign - ERROR: --sm3Hdp needs -v <template .nhdp>", NULL);

    if (load_strand_model(&R.smt, t_model, R.hdp ? t_hdp : NULL) != SA_OK)
        die("signalAlign - ERROR: couldn't find model file here: %s", t_model);
    if (R.two_d && load_strand_model(&R.smc, c_model, R.hdp ? c_hdp : NULL) != SA_OK)
        die("signalAlign - ERROR: couldn't find model file here: %s", c_model);
    for (int s = 0; s < (R.two_d ? 2 : 1) && R.two_dist && batch_mode; s++) {   /* the base of the slices' noise-scaled batches */
        strand_model_t *sm = s == 0 ? &R.smt : &R.smc;
        if (sa_model_clone_with_table(&sm->model_two, sm->model, sm->table_orig) != SA_OK ||
            sa_model_set_emission(sm->model_two, SA_EMISSION_TWO_DIST) != SA_OK)
            die("signalMachine: --emission twoDist: could not set up the two-distribution model%s", "");
    }
    if (ambig_model) {
        if (sa_load_ambig(ambig_model, R.ambig) != SA_OK) {
            printf("Couldn't open %s for reading\n", ambig_model);
            return 1;
        }
    } else {
        sa_default_ambig(R.ambig);
    }

    if (R.hdp && !R.expect_mode) { /* the alignment branch sets the HDP expected values (impl/signalMachine.c:861-863), the expectation branch does not */
        set_hdp_expected(&R.smt);
        if (R.two_d) set_hdp_expected(&R.smc);
    }
    /* the reads go through in slices of --batch-reads (default 2048): bounded host and device memory for any manifest */
    /* Two slices are in the air: while the GPU stage and the rendering of slice k run here, a second thread does the host side
     * of slice k+1 (10 000 short reads: host stage 0.39 s, GPU 0.28 s, rendering 0.25 s, one after the other before).  Rendering
     * stays on this thread, slice after slice, so the summary lines stay in read order: the front door is bound by host CPU
     * time -- text parsing and TSV rendering -- not by the order of its stages. */
    int64_t n_failed = 0;
    if (R.snp_step > 0) {   /* a slice holds at most --batch-reads jobs: N per read and strand */
        batch_reads = batch_reads / R.snp_step > 0 ? batch_reads / R.snp_step : 1;
        if (mkdir(R.snp_dir, 0777) != 0 && errno != EEXIST) die("signalMachine: cannot create %s", R.snp_dir);
    }
    slice_prep_t cur = {&R, reads, n_reads < batch_reads ? n_reads : batch_reads, batch_mode}, nxt;
    slice_prepare(&cur);
    for (int64_t off = 0; off < n_reads; off += batch_reads) {
        const int64_t n = n_reads - off < batch_reads ? n_reads - off : batch_reads;
        pthread_t th;
        int started = 0;
        if (off + n < n_reads) {
            const int64_t n2 = n_reads - off - n < batch_reads ? n_reads - off - n : batch_reads;
            nxt = (slice_prep_t) {&R, reads + off + n, n2, batch_mode};
            started = pthread_create(&th, NULL, slice_prepare, &nxt) == 0;
            if (!started) slice_prepare(&nxt);
        }
        int64_t failed_now = 0;
        if (R.snp_step > 0) {
            n_failed += run_slice_snp(&R, reads + off, n, batch_mode, device);
            if (started) pthread_join(th, NULL);
            continue;
        }
        render_job_t *job = run_slice(&R, reads + off, n, batch_mode, device, &failed_now);
        n_failed += failed_now;
        if (job) { n_failed += render_slice(job); free(job); }
        if (started) pthread_join(th, NULL);
    }
    if (R.agg_path) write_aggregate(R.agg_path);
    write_training(&R, t_model, c_model, device);
    if (batch_mode)
        fprintf(stderr, "[signalMachine] batch: %" PRId64 " of %" PRId64 " reads aligned\n", n_reads - n_failed, n_reads);
    if (getenv("SA_CLI_TIMING"))
        fprintf(stderr, "[signalMachine] timing: host stage %.3f s wall (thread-seconds: npRead+cigar parse %.3f, reference fetch "
                        "%.3f, parameter estimation+anchors %.3f), GPU stage %.3f s wall, render+write %.3f s wall\n",
                g_t_prep, g_ts_parse, g_ts_fetch, g_ts_estimate, g_t_gpu, g_t_render);
    return n_failed == 0 ? 0 : 1;
}
