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
                    "--npread-out <dir>: write <dir>/<label>.npRead for every raw read (usable with -q)\n"
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
                    "--site-calls-accuracy-threshold <t>: the confusion counts' threshold (default 0.500000001)\n");
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
                    "--train-median, --train-mod-only, --train-kmers <file> (one k-mer per line: only those are trained)\n"
                    "                  with any --train-* output, a manifest's posteriors file may be '-' as well\n"
                    "--train-mixture-motifs <canonical:modified,...> (e.g. CCAGG:CEAGG,CCTGG:CETGG) with --train-mixture-template-model\n"
                    "                  <file> / --train-mixture-complement-model <file> / --train-mixture-distances <file>: every\n"
                    "                  canonical k-mer over a motif's modified position gets a two-component Gaussian mixture fitted\n"
                    "                  to its rows of that table on the GPU; the component farther from the -T / -C level mean\n"
                    "                  becomes the modified k-mer's mean and SD in the model written (mixture_model.py), the\n"
                    "                  distances file lists both components per k-mer\n\n");
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
    /* --site-calls-accuracy: the run's calls scored against known truth on the GPU (sa_call_scores_t), written at the end; it
     * needs the over-reads table too (want_agg) */
    const char *acc_path, *acc_curves_path, *acc_truth_path, *acc_reads_path;
    int acc_bins, want_agg;
    double acc_threshold;
    /* --train-*: the top-N assignments of the whole run in k-mer tables on the GPU (one per strand), written at the end */
    const char *train_assign, *train_model[2], *train_kmers;
    int want_train;         /* any of --train-assignments / --train-template-model / --train-complement-model / --train-mixture-* */
    double train_min_prob, train_weight, train_min_sd;
    int64_t train_n;
    int train_median, train_mod_only;
    /* --train-mixture-*: the modified k-mers of motif pairs get the other component of a two-component mixture (mixture_model.py) */
    const char *mix_motifs, *mix_model[2], *mix_dist;
    sa_kmer_table_t *train_tab[2];
    int two_dist; /* --emission twoDist: the two-distribution emission (not an option of the reference binary: it is what its
                   * state machine carried when the reference's shipped output files were written).  A single read is aligned with
                   * a model of its own (read_t.model); the reads of a manifest share one batch on the strand's model_two and
                   * hand over their noise scalings (sa_batch_create_noise_scaled) */
    int batch_mode;
    int device;                   /* --device, for the stage that runs ahead of a slice's GPU stage (the guide alignment) */
    int guide_band;               /* --guide-band */
    const char *guide_cigars_out; /* --guide-cigars-out */
    const char *npread_out;       /* --npread-out: where raw_stage writes <label>.npRead of every raw read */
    int raw_detector_set;         /* --raw-detector */
    sa_detector_params_t raw_detector;
    int64_t out_fmt, constraint_trim;
    int64_t snp_step;       /* --snp-step N: single-nucleotide probabilities, N substituted copies of every read's reference */
    const char *snp_dir;    /* --snp-dir: where <label>.tsv goes */
    /* --snp-marginals / --snp-proposals: the over-reads table on the GPU, the -f reference's records it is laid over, and the
     * run's first read (a read's run ordinal is its place in the manifest) */
    const char *snp_marg, *snp_prop;
    /* --snp-sites: the listed sites per record of the -f reference, ascending; --snp-reference-out */
    const char *snp_sites_path, *snp_ref_out;
    int64_t **snp_sites, *snp_n_sites;
    sa_snp_marginals_t *snp_tab;
    char **snp_names, **snp_seqs;   /* (the records of -f: --position-profile lays its table over them too) */
    int64_t *snp_lens, snp_n_contigs;
    const char *prof_path;          /* --position-profile: the per-position profile of the run's template batches, on the GPU */
    sa_position_profile_t *prof_tab;
    /* --guide-deviation: every strand batch's deviation from its guide (sa_batch_guide_deviation), written read by read */
    const char *dev_path, *dev_events_path;
    FILE *dev_fh, *dev_events_fh;
    sa_deviation_params_t dev_params;
    int64_t dev_total[SA_DEV_MAX_BUCKETS];   /* the H lines written so far, summed: the T line */
    const void *reads0;
    const char *fwd_ref, *bwd_ref;
    sa_params_t p;
    strand_model_t sm[2];   /* [strand]: 0 template, 1 complement (--twoD only) */
    const char *ambig[256];
} run_t;

static int n_strands(const run_t *R) { return R->two_d ? 2 : 1; }
static const char *strand_name(int s) { return s == 0 ? "template" : "complement"; }

/* one read: its inputs, the two alignment jobs, where its outputs go */
typedef struct {
    char *label, *npread_path, *cigar_path, *post_path, *post_path2, *seq_name;
    char *expect[2];      /* [strand]: where -t / -c write the strand's expectations */
    char *guide_window;   /* <contig>:<start>-<end>[:+|:-] instead of a cigar file: the guide alignment is computed (guide_stage) */
    int guide_locate;     /* neither a cigar file nor a window: locate_stage writes guide_window */
    int raw;              /* npread_path names a raw-read file (sa_rawread_is): raw_stage fills np */
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

/* plans `per_read` jobs per strand alone on the host (integer geometry only, no GPU); marks the read failed when the planner
 * rejects one */
static int validate_read(const run_t *R, read_t *rd, const sa_job_t *const jobs[2], int64_t per_read) {
    for (int s = 0; s < n_strands(R); s++)
        for (int64_t i = 0; i < per_read; i++) {
            int rc = sa_plan_describe(R->sm[s].model, &R->p, &jobs[s][i], R->ambig, 0, NULL, NULL, 0, NULL, 0, NULL, 0);
            if (rc != SA_OK) return fail(rd, 0, "alignment job rejected: %s", sa_strerror(rc));
        }
    return 0;
}

/* one strand of a read: estimate the read's parameters (signalUtils_estimateNanoporeParams), build the job from the guide
 * alignment's anchors */
static int build_strand_job(const run_t *R, read_t *rd, int s, const int64_t *gx, const int64_t *gy) {
    sa_npread_t *np = rd->np;
    sa_strand_params_t *pp = np_params(np, s);
    if (estimate_strand(&R->sm[s], np_strand_map(np, s), np_events(np, s), np_n_events(np, s), np_read(np, s), np_read_length(np, s), pp,
                        R->two_dist && !R->batch_mode ? &rd->model[s] : NULL) != SA_OK)
        return -1;
    sa_job_t *job = &rd->jobs[s];
    rd->ax[s] = xalloc(rd->n_guide + 1, sizeof(int64_t), 0);
    rd->ay[s] = xalloc(rd->n_guide + 1, sizeof(int64_t), 0);
    job->n_anchors = sa_remap_anchors(gx, gy, rd->n_guide, np_event_map(np, s, R->two_d), rd->pA->start2, rd->ax[s], rd->ay[s]);
    job->anchor_x = rd->ax[s]; job->anchor_y = rd->ay[s];
    job->ref = rd->st[s].target;
    job->ref_len = (int64_t) strlen(rd->st[s].target);
    job->events = np_events(np, s) + 4 * rd->st[s].lo;
    job->event_stride = 4;
    job->n_events = rd->st[s].hi - rd->st[s].lo;
    job->scale = pp->scale; job->shift = pp->shift; job->var = pp->var;
    return 0;
}

/* everything of impl/signalMachine.c:main between option parsing and performSignalAlignment, for one read */
static int prepare_read(const run_t *R, read_t *rd, int fatal) {
    const double tp0 = now_s();
    if (rd->failed) return -1;   /* the guide stage gave up on it */
    if (rd->pA == NULL) {        /* (a read with a guide window has its alignment, and its .npRead, from guide_stage) */
        if (rd->cigar_path == NULL) return fail(rd, fatal, "[signalMachine]ERROR: Need to provide input guide alignments, exiting", NULL);
        if (sa_cigar_load(rd->cigar_path, &rd->pA) != SA_OK)
            return fail(rd, fatal, "[signalMachine]ERROR: Didn't find input alignment file, looked %s", rd->cigar_path);
        fprintf(stderr, "[signalMachine]NOTICE: Using guide alignments from %s\n", rd->cigar_path);
    }
    sa_cigar_t *pA = rd->pA;
    if (rd->np == NULL && (rd->npread_path == NULL || sa_npread_load(rd->npread_path, &rd->np) != SA_OK))
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
    rd->st[0].target = strand1 ? rd->forward_seq : rd->backward_seq;
    rd->st[1].target = strand1 ? rd->backward_seq : rd->forward_seq;

    /* event slices and coordinate shifts (impl/signalMachine.c:726-750) */
    for (int s = 0; s < n_strands(R); s++) {
        const int64_t *map = np_event_map(np, s, R->two_d);
        rd->st[s].lo = map[pA->start2];
        rd->st[s].hi = map[pA->end2 - 1];
    }
    rd->st[0].r_shift = pA->start1;
    rd->st[1].r_shift = R->two_d ? pA->end1 : 0;
    rd->forward = pA->strand1;

    const double tp2 = now_s();
    t_add(&g_ts_fetch, tp2 - tp1);
    /* anchors from the guide alignment (pA is rebased inside, impl/signalMachineUtils.c:142-164) */
    int64_t cap = 0;
    for (int64_t i = 0; i < pA->n_ops; i++) cap += pA->op_len[i];
    int64_t *gx = xalloc(cap + 1, sizeof(int64_t), 0), *gy = xalloc(cap + 1, sizeof(int64_t), 0);
    rd->n_guide = sa_guide_to_anchors(pA->start1, pA->end1, pA->strand1, pA->start2, pA->op_type, pA->op_len, pA->n_ops,
                                      R->constraint_trim, gx, gy, cap + 1);
    int built = rd->n_guide < 0 ? -1 : 0;
    memset(rd->jobs, 0, sizeof(rd->jobs));
    for (int s = 0; s < n_strands(R) && built == 0; s++) built = build_strand_job(R, rd, s, gx, gy);
    free(gx);
    free(gy);
    if (rd->n_guide < 0) return fail(rd, fatal, "signalMachine: could not convert the guide alignment", NULL);
    if (built != 0) return fail(rd, fatal, "Cannot get scale params with no assignments", NULL);
    t_add(&g_ts_estimate, now_s() - tp2);
    /* batch mode: the reads of a slice share one GPU batch, and the planner rejects a whole batch for one bad job (a
     * reference window with a letter outside the alphabet, anchors that give an invalid diagonal).  The reference runs one
     * process per read, so only that read may fail.  Alignment runs find the offender when -- and only when -- a batch is
     * turned down (drop_refused_reads below); the expectation routine writes files strand by strand and cannot be re-run, so
     * its jobs are planned alone on the host here. */
    if (!fatal && R->expect_mode) {
        const sa_job_t *const own[2] = {&rd->jobs[0], &rd->jobs[1]};
        return validate_read(R, rd, own, 1);
    }
    return 0;
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
        if (rd->cigar_path && rd->cigar_path[0] == '@') {   /* @<contig>:<start>-<end>[:+|:-]: computed, not read; @ alone: located first */
            if (rd->cigar_path[1] == 0) rd->guide_locate = 1;
            else rd->guide_window = strdup(rd->cigar_path + 1);
            free(rd->cigar_path);
            rd->cigar_path = NULL;
        }
        rd->post_path = dup_field(f[3]);
        rd->post_path2 = dup_field(f[4]);
        rd->seq_name = dup_field(f[5]);
        rd->expect[0] = dup_field(f[6]);
        rd->expect[1] = dup_field(f[7]);
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


/* ---- reads given as raw current --------------------------------------------------------------------------------------------- */
/* The reads of a slice whose -q / manifest file is a raw-read file (sa_io.h): ONE sa_npread_from_raw_batch call -- event detection,
 * MoM scalings, event alignment and the base-to-event map on the GPU -- gives each the sa_npread_t that sa_npread_load would have
 * read from the .npRead the reference's Python writes for a 1D read: template read, strand event map, events, the default
 * parameters (estimate_strand replaces them).  From there on it is a read like any other.  A read the chain rejects fails as a
 * read with an unreadable .npRead does. */
static void raw_stage(const run_t *R, read_t *reads, int64_t n_reads) {
    int64_t n = 0;
    for (int64_t i = 0; i < n_reads; i++) n += reads[i].raw && !reads[i].failed;
    if (n == 0) return;
    const int fatal = !R->batch_mode;
    read_t **rd = xalloc(n, sizeof(read_t *), 0);
    sa_rawread_t **rr = xalloc(n, sizeof(sa_rawread_t *), 1);
    sa_raw_job_t *jobs = xalloc(n, sizeof(sa_raw_job_t), 1);
    const char **seq = xalloc(n, sizeof(char *), 0);
    n = 0;
    for (int64_t i = 0; i < n_reads; i++) {
        read_t *r = &reads[i];
        if (!r->raw || r->failed) continue;
        sa_rawread_t *w = NULL;
        const int rc = sa_rawread_load(r->npread_path, &w);
        if (rc != SA_OK) { fail(r, fatal, "signalMachine: could not load the raw read %s", r->npread_path); continue; }
        if (w->seq_len < R->sm[0].k) {
            sa_rawread_free(w);
            fail(r, fatal, "signalMachine: the sequence of the raw read %s is shorter than the model's k-mers", r->npread_path);
            continue;
        }
        rd[n] = r;
        rr[n] = w;
        jobs[n] = (sa_raw_job_t) {w->samples, w->n_samples, w->digitisation, w->offset, w->range, w->sample_rate, w->start_time};
        seq[n++] = w->sequence;
    }
    sa_raw_npread_t *out = xalloc(n, sizeof(sa_raw_npread_t), 1);
    const int rc = n > 0 ? sa_npread_from_raw_batch(R->sm[0].model, jobs, seq, n, R->raw_detector_set ? &R->raw_detector : NULL, R->device, 0,
                                                    out, NULL) : SA_OK;
    for (int64_t q = 0; q < n; q++) {
        read_t *r = rd[q];
        const sa_raw_npread_t *o = &out[q];
        if (rc != SA_OK) { fail(r, fatal, "signalMachine: the raw reads could not be turned into events: %s", sa_strerror(rc)); continue; }
        if (o->status != 0) {
            char what[160];
            snprintf(what, sizeof(what), "%s (status %d)", (o->status & SA_RAW_MAP_LENGTH) ? "Read and event map lengths do not match"
                     : (o->status & SA_RAW_NO_PEAK) ? "the event detector found no event boundary"
                     : "its events do not align to its sequence", (int) o->status);
            fail(r, fatal, "signalMachine: no event table for the raw read: %s", what);
            continue;
        }
        if (R->npread_out) {
            char *path = xalloc((int64_t) (strlen(R->npread_out) + strlen(r->label) + 16), 1, 0);
            sprintf(path, "%s/%s.npRead", R->npread_out, r->label);
            if (sa_raw_npread_write(o, seq[q], R->sm[0].model, path) != SA_OK) fprintf(stderr, "[signalMachine]WARNING: cannot write %s\n", path);
            free(path);
        }
        sa_npread_t *np = xalloc(1, sizeof(sa_npread_t), 1);
        np->template_params = np->complement_params = (sa_strand_params_t) {1, 1, 1, 1, 1, 0, 0};   /* the .npRead's 1 1 1 1 1 0 */
        np->n_template_events = o->n_events;
        np->template_read_length = o->read_len;
        np->two_d_read = strdup("");
        np->complement_read = strdup("");
        np->template_read = strdup(seq[q]);
        np->template_strand_event_map = xalloc(o->read_len, sizeof(int64_t), 0);
        memcpy(np->template_strand_event_map, o->strand_event_map, sizeof(int64_t) * (size_t) o->read_len);
        np->template_events = xalloc(4 * o->n_events, sizeof(double), 0);
        memcpy(np->template_events, o->events4, sizeof(double) * 4 * (size_t) o->n_events);
        r->np = np;
        fprintf(stderr, "[signalMachine]NOTICE: %s from raw current: %" PRId64 " samples, %" PRId64 " events on %" PRId64 " bases (shift %f, scale %f)\n",
                r->label, rr[q]->n_samples, o->n_events, o->read_len, o->mom_shift, o->mom_scale);
    }
    sa_raw_npread_free(out, n);
    for (int64_t q = 0; q < n; q++) sa_rawread_free(rr[q]);
    free(out); free(seq); free(jobs); free(rr); free(rd);
}

/* ---- guide alignment on the GPU --------------------------------------------------------------------------------------------- */
/* <contig>:<start>-<end>[:+|:-], read from the right (a contig name may hold colons); strand: 1 '+', 0 '-', -1 not given */
static int parse_guide_window(const char *spec, char **contig, int64_t *start, int64_t *end, int *strand) {
    size_t len = strlen(spec);
    *strand = -1;
    if (len >= 2 && spec[len - 2] == ':' && (spec[len - 1] == '+' || spec[len - 1] == '-')) {
        *strand = spec[len - 1] == '+';
        len -= 2;
    }
    size_t colon = len;
    while (colon > 0 && spec[colon - 1] != ':') colon--;
    if (colon < 2) return -1;   /* no colon, or an empty contig name */
    char range[64];
    if (len - colon == 0 || len - colon >= sizeof(range)) return -1;
    memcpy(range, spec + colon, len - colon);
    range[len - colon] = 0;
    char *dash = NULL, *stop = NULL;
    if (!isdigit((unsigned char) range[0])) return -1;
    const long long a = strtoll(range, &dash, 10);
    if (*dash != '-' || !isdigit((unsigned char) dash[1])) return -1;
    const long long b = strtoll(dash + 1, &stop, 10);
    if (*stop != 0 || b <= a) return -1;
    *contig = strndup(spec, colon - 1);
    *start = a;
    *end = b;
    return 0;
}

typedef struct {
    read_t *rd;
    char *contig, *oriented;   /* the window as the read is aligned to it: forward or reverse complement */
    int64_t w_start, w_len, crop;
    int reverse;
    sa_guide_job_t job;
} guide_item_t;

typedef struct {
    const run_t *R;
    guide_item_t *items;
} guide_ctx_t;

/* host side of one read: the .npRead, the window, the seed */
static void guide_prepare_one(int64_t i, void *ctx) {
    const guide_ctx_t *g = ctx;
    const run_t *R = g->R;
    guide_item_t *it = &g->items[i];
    read_t *rd = it->rd;
    const int fatal = !R->batch_mode;
    int64_t w_end = 0;
    if (rd->failed) return;   /* the raw stage gave up on it */
    int strand = -1;
    if (parse_guide_window(rd->guide_window, &it->contig, &it->w_start, &w_end, &strand) != 0) {
        fail(rd, fatal, "signalMachine: cannot read the guide window %s (want <contig>:<start>-<end>[:+|:-])", rd->guide_window);
        return;
    }
    if (R->fwd_ref == NULL) { fail(rd, fatal, "[signalMachine] ERROR: a guide window needs -f <fasta>", NULL); return; }
    if (rd->np == NULL && (rd->npread_path == NULL || sa_npread_load(rd->npread_path, &rd->np) != SA_OK)) {   /* (locate_stage loads it too) */
        fail(rd, fatal, "signalMachine: could not load the nanopore read %s", rd->npread_path);
        return;
    }
    const char *read = R->two_d ? rd->np->two_d_read : rd->np->template_read;
    const int64_t read_len = R->two_d ? rd->np->read_length : rd->np->template_read_length;
    int ferr = 0;
    char *window = sa_fasta_fetch(R->fwd_ref, it->contig, it->w_start, w_end - 1, &ferr);
    if (window == NULL) {
        fail(rd, fatal, ferr == -2 ? "sequence name %s is not in the reference fasta" : "[signalMachine] ERROR: Unable to fetch the guide window %s",
             ferr == -2 ? it->contig : rd->guide_window);
        return;
    }
    it->w_len = (int64_t) strlen(window);
    int64_t diag = 0, votes = 0, hits = 0;
    int reverse = 0, seeded;
    if (strand == 0) {   /* told: minus */
        it->oriented = sa_reverse_complement(window);
        free(window);
        seeded = sa_guide_seed(read, read_len, it->oriented, it->w_len, 0, &diag, &reverse, &votes, &hits) == 0;
        reverse = 1;
    } else {
        seeded = sa_guide_seed(read, read_len, window, it->w_len, strand < 0, &diag, &reverse, &votes, &hits) == 0;
        if (seeded && reverse) {
            it->oriented = sa_reverse_complement(window);
            free(window);
        } else {
            it->oriented = window;
            reverse = 0;
        }
    }
    if (!seeded) diag = 0;
    it->reverse = reverse;
    /* the band absorbs what lies within it of the seed's diagonal: the window starts band / 2 before */
    it->crop = seeded && diag > R->guide_band / 2 ? diag - R->guide_band / 2 : 0;
    it->job.read = read;
    it->job.read_len = read_len;
    it->job.ref = it->oriented + it->crop;
    it->job.ref_len = it->w_len - it->crop;
    it->job.diag = diag - it->crop;
}

/* The -f reference's index: built on first need, once per process, resident on the device until the process ends */
static sa_ref_index_t *g_ref_index = NULL;
static int g_ref_index_rc = SA_OK, g_ref_index_tried = 0;
static pthread_mutex_t g_ref_index_mu = PTHREAD_MUTEX_INITIALIZER;

static int ref_index_get(const run_t *R, sa_ref_index_t **out) {
    pthread_mutex_lock(&g_ref_index_mu);
    if (!g_ref_index_tried) {
        g_ref_index_tried = 1;
        g_ref_index_rc = sa_ref_index_build_fasta(&g_ref_index, R->fwd_ref, R->device);
        sa_ref_index_info_t info;
        if (g_ref_index_rc == SA_OK && sa_ref_index_info(g_ref_index, &info) == SA_OK)
            fprintf(stderr, "[signalMachine]NOTICE: Indexed %s: %" PRId64 " contigs, %" PRId64 " bases, %" PRId64 " 15-mers, %.2f s\n", R->fwd_ref,
                    info.n_contigs, info.total_bases, info.n_entries, info.build_seconds);
    }
    *out = g_ref_index;
    const int rc = g_ref_index_rc;
    pthread_mutex_unlock(&g_ref_index_mu);
    return rc;
}

typedef struct {
    const run_t *R;
    read_t **rd;
} locate_ctx_t;

static void locate_load_one(int64_t i, void *ctx) {
    const locate_ctx_t *c = ctx;
    read_t *rd = c->rd[i];
    if (rd->np == NULL && (rd->npread_path == NULL || sa_npread_load(rd->npread_path, &rd->np) != SA_OK))   /* (raw_stage fills it too) */
        fail(rd, !c->R->batch_mode, "signalMachine: could not load the nanopore read %s", rd->npread_path);
}

/* The reads of a slice that name neither a cigar file nor a window: ONE sa_guide_locate_batch call against the index of the whole
 * -f reference; a located read gets the window spec that sa_locate_window gives and is a read with a guide window from there on.
 * A read without a location fails as a read with an unreadable cigar file does. */
static void locate_stage(const run_t *R, read_t *reads, int64_t n_reads) {
    int64_t n = 0;
    for (int64_t i = 0; i < n_reads; i++) n += reads[i].guide_locate && reads[i].guide_window == NULL && !reads[i].failed;
    if (n == 0) return;
    const int fatal = !R->batch_mode;
    read_t **rd = xalloc(n, sizeof(read_t *), 0);
    n = 0;
    for (int64_t i = 0; i < n_reads; i++)
        if (reads[i].guide_locate && reads[i].guide_window == NULL && !reads[i].failed) rd[n++] = &reads[i];
    sa_ref_index_t *idx = NULL;
    int rc = R->fwd_ref == NULL ? SA_EINVAL : ref_index_get(R, &idx);
    if (rc != SA_OK) {
        for (int64_t i = 0; i < n; i++)
            fail(rd[i], fatal, R->fwd_ref == NULL ? "[signalMachine] ERROR: --guide-locate needs -f <fasta>%s"
                 : "signalMachine: the reference could not be indexed: %s", R->fwd_ref == NULL ? "" : sa_strerror(rc));
        free(rd);
        return;
    }
    locate_ctx_t ctx = {R, rd};
    parallel_for(n, locate_load_one, &ctx);
    const char **seq = xalloc(n, sizeof(char *), 0);
    int64_t *len = xalloc(n, sizeof(int64_t), 0), *who = xalloc(n, sizeof(int64_t), 0), n_live = 0;
    for (int64_t i = 0; i < n; i++) {
        if (rd[i]->failed) continue;
        seq[n_live] = R->two_d ? rd[i]->np->two_d_read : rd[i]->np->template_read;
        len[n_live] = R->two_d ? rd[i]->np->read_length : rd[i]->np->template_read_length;
        who[n_live++] = i;
    }
    sa_locate_result_t *res = xalloc(n_live, sizeof(sa_locate_result_t), 1);
    rc = n_live > 0 ? sa_guide_locate_batch(idx, seq, len, n_live, NULL, 0, res, NULL) : SA_OK;
    for (int64_t q = 0; q < n_live; q++) {
        read_t *r = rd[who[q]];
        const sa_locate_result_t *l = &res[q];
        if (rc != SA_OK) { fail(r, fatal, "signalMachine: the read could not be located: %s", sa_strerror(rc)); continue; }
        int64_t start = 0, end = 0;
        const char *contig = NULL;
        if ((l->status & (SA_LOCATE_NONE | SA_LOCATE_EMPTY)) || sa_locate_window(idx, l, len[q], R->guide_band, &start, &end) != SA_OK ||
            sa_ref_index_contig(idx, l->contig, &contig, NULL, NULL) != SA_OK) {
            fail(r, fatal, "signalMachine: no location for the read in %s", R->fwd_ref);
            continue;
        }
        r->guide_window = xalloc((int64_t) strlen(contig) + 64, 1, 0);
        sprintf(r->guide_window, "%s:%" PRId64 "-%" PRId64 ":%c", contig, start, end, l->reverse ? '-' : '+');
        fprintf(stderr, "[signalMachine]NOTICE: Read located at %s (%" PRId64 " votes, next %" PRId64 ")\n", r->guide_window, l->votes,
                l->second_votes);
        if (l->status & SA_LOCATE_AMBIGUOUS)
            fprintf(stderr, "[signalMachine]WARNING: the location of %s is ambiguous: another locus has %" PRId64 " votes against %" PRId64 "\n",
                    r->label, l->second_votes, l->votes);
        if (l->status & SA_LOCATE_OVERFLOW)
            fprintf(stderr, "[signalMachine]WARNING: %s has more 15-mer hits than the vote keeps (overflow): the later ones did not vote\n", r->label);
    }
    free(res); free(who); free(len); free(seq); free(rd);
}

/* The reads of a slice that name a window instead of a cigar file: ONE sa_guide_align_batch call, ahead of prepare_read's
 * remaining work; the result becomes the read's sa_cigar_t.  A read whose alignment is unusable fails as a read with an unusable
 * cigar file does. */
static void guide_stage(const run_t *R, read_t *reads, int64_t n_reads) {
    int64_t n = 0;
    for (int64_t i = 0; i < n_reads; i++) n += reads[i].guide_window != NULL;
    if (n == 0) return;
    const int fatal = !R->batch_mode;
    guide_item_t *items = xalloc(n, sizeof(guide_item_t), 1);
    n = 0;
    for (int64_t i = 0; i < n_reads; i++)
        if (reads[i].guide_window != NULL) items[n++].rd = &reads[i];
    guide_ctx_t ctx = {R, items};
    parallel_for(n, guide_prepare_one, &ctx);
    sa_guide_job_t *jobs = xalloc(n, sizeof(sa_guide_job_t), 1);
    int64_t *who = xalloc(n, sizeof(int64_t), 0), n_jobs = 0;
    for (int64_t i = 0; i < n; i++)
        if (!items[i].rd->failed) { jobs[n_jobs] = items[i].job; who[n_jobs++] = i; }
    sa_guide_result_t *res = xalloc(n_jobs, sizeof(sa_guide_result_t), 1);
    int32_t *op_type = NULL;
    int64_t *op_len = NULL;
    sa_guide_params_t prm = {2, -4, 4, 2, -1, R->guide_band, 0.5};
    int rc = n_jobs > 0 ? sa_guide_align_batch(jobs, n_jobs, &prm, R->device, 0, res, &op_type, &op_len, NULL) : SA_OK;
    for (int64_t q = 0; q < n_jobs; q++) {
        guide_item_t *it = &items[who[q]];
        read_t *rd = it->rd;
        if (rc != SA_OK) { fail(rd, fatal, "signalMachine: the guide alignment could not be computed: %s", sa_strerror(rc)); continue; }
        const sa_guide_result_t *r = &res[q];
        if (r->status & ~SA_GUIDE_BAND_EDGE) {
            fail(rd, fatal, r->status & (SA_GUIDE_NO_ALIGNMENT | SA_GUIDE_EMPTY) ? "signalMachine: no guide alignment of the read inside %s"
                 : r->status & SA_GUIDE_SHORT ? "signalMachine: the guide alignment inside %s covers less than half of the read"
                 : "signalMachine: the guide alignment inside %s could not be traced", rd->guide_window);
            continue;
        }
        if (r->status & SA_GUIDE_BAND_EDGE)
            fprintf(stderr, "[signalMachine]WARNING: the guide alignment of %s touches the edge of its band (--guide-band %d): it may be clipped\n",
                    rd->label, R->guide_band);
        /* window coordinates of the aligned stretch in the orientation it was aligned in, then forward contig coordinates */
        const int64_t a = it->crop + r->ref_start, b = it->crop + r->ref_end;
        const int64_t fs = it->w_start + (it->reverse ? it->w_len - b : a), fe = it->w_start + (it->reverse ? it->w_len - a : b);
        sa_cigar_t *c = xalloc(1, sizeof(sa_cigar_t), 1);
        c->contig1 = strdup(it->contig);
        c->contig2 = strdup(rd->label);
        c->start2 = r->read_start; c->end2 = r->read_end; c->strand2 = 1;
        c->start1 = it->reverse ? fe : fs; c->end1 = it->reverse ? fs : fe; c->strand1 = !it->reverse;
        c->score = (double) r->score;
        c->n_ops = r->n_ops;
        c->op_type = xalloc(r->n_ops, sizeof(int32_t), 0);
        c->op_len = xalloc(r->n_ops, sizeof(int64_t), 0);
        memcpy(c->op_type, op_type + r->op_first, sizeof(int32_t) * (size_t) r->n_ops);
        memcpy(c->op_len, op_len + r->op_first, sizeof(int64_t) * (size_t) r->n_ops);
        rd->pA = c;
        rd->seq_name = strdup(it->contig);   /* the window names the contig, whatever -n says */
        fprintf(stderr, "[signalMachine]NOTICE: Guide alignment computed on the GPU inside %s: read %" PRId64 "-%" PRId64 " on %s %" PRId64 "-%" PRId64
                        " %c, score %" PRId64 "\n", rd->guide_window, c->start2, c->end2, c->contig1, fs, fe, it->reverse ? '-' : '+', r->score);
        if (R->guide_cigars_out) {
            const int64_t need = sa_guide_format_cigar(rd->label, c->start2, c->end2, c->contig1, fs, fe, !it->reverse, r->score, c->op_type,
                                                       c->op_len, c->n_ops, NULL, 0);
            char *line = xalloc(need + 1, 1, 0);
            sa_guide_format_cigar(rd->label, c->start2, c->end2, c->contig1, fs, fe, !it->reverse, r->score, c->op_type, c->op_len, c->n_ops,
                                  line, need + 1);
            char *path = xalloc((int64_t) (strlen(R->guide_cigars_out) + strlen(rd->label) + 16), 1, 0);
            sprintf(path, "%s/%s.cigar", R->guide_cigars_out, rd->label);
            FILE *fh = fopen(path, "w");
            if (fh) { fprintf(fh, "%s\n", line); fclose(fh); }
            else fprintf(stderr, "[signalMachine]WARNING: cannot write %s\n", path);
            free(path);
            free(line);
        }
    }
    sa_free(op_type);
    sa_free(op_len);
    for (int64_t i = 0; i < n; i++) { free(items[i].contig); free(items[i].oriented); }
    free(res); free(who); free(jobs); free(items);
}

/* One slice of the run's reads: host side of every read, one GPU batch per strand model, outputs.  (The whole manifest used to
 * be one batch: fine for thousands of reads, not for a flow cell.) */
typedef struct {
    run_t *R;
    read_t *reads;
    int64_t n_reads;
    int device;
    int64_t *who, n_ok;   /* the reads that are still in: reads[who[0 .. n_ok)] */
    int validated;        /* the reads' jobs have been planned one by one (drop_refused_reads) */
} slice_t;

static void prep_one(int64_t i, void *ctx) {
    const slice_t *sl = ctx;
    read_t *rd = &sl->reads[i];
    if (prepare_read(sl->R, rd, !sl->R->batch_mode) != 0)
        fprintf(stderr, "[signalMachine] ERROR: read %s skipped: %s\n", rd->label, rd->err);
}

/* host side of every read of a slice (files, parameter estimation, anchors): all host threads */
static void *slice_prepare(void *arg) {
    slice_t *sl = arg;
    const double ts0 = now_s();
    raw_stage(sl->R, sl->reads, sl->n_reads);
    locate_stage(sl->R, sl->reads, sl->n_reads);
    guide_stage(sl->R, sl->reads, sl->n_reads);
    parallel_for(sl->n_reads, prep_one, sl);
    t_add(&g_t_prep, now_s() - ts0);
    return NULL;
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

/* the GPU stage of a slice starts here: who[0 .. n_ok) are the reads whose host side went through */
static void slice_open(slice_t *sl, run_t *R, read_t *reads, int64_t n_reads, int device) {
    memset(sl, 0, sizeof(*sl));
    sl->R = R; sl->reads = reads; sl->n_reads = n_reads; sl->device = device;
    sl->validated = !R->batch_mode;   /* a single-read run has nobody to isolate a bad job from */
    sl->who = xalloc(n_reads, sizeof(int64_t), 0);
    for (int64_t i = 0; i < n_reads; i++)
        if (!reads[i].failed) sl->who[sl->n_ok++] = i;
}

/* ... and ends here: the reads' memory goes back; returns the number of the slice's reads that failed */
static int64_t slice_close(slice_t *sl) {
    int64_t n_failed = 0;
    for (int64_t i = 0; i < sl->n_reads; i++) n_failed += sl->reads[i].failed ? 1 : 0;
    for (int64_t i = 0; i < sl->n_reads; i++) release_read(&sl->reads[i]);
    free(sl->who);
    return n_failed;
}

/* the summary line on stdout (n == NULL: none, the expectations mode) and the SUCCESS line on stderr of one alignment of a read */
static void report_read(const run_t *R, const read_t *rd, const int64_t *n, const double *score) {
    if (n) {
        fprintf(stdout, "%s %" PRId64 "\t%" PRId64 "(%f)\t", rd->label, rd->n_guide, n[0], score[0]);
        if (R->two_d) fprintf(stdout, "%" PRId64 "(%f)\n", n[1], score[1]);
        else fprintf(stdout, "\n");
    }
    fprintf(stderr, "signalAlign - SUCCESS: finished alignment of query %s, exiting\n", rd->label);
}

/* The planner turned a strand's batch down with `rc` (a letter outside the alphabet, anchors that give no band, a cell of more
 * paths or a matrix larger than the result records can name -- SA_EUNSUPPORTED --, ...): find the reads whose jobs it rejects
 * (each planned alone on the host, all host threads) and let them fail alone, as the reference's one-process-per-read runs
 * would.  jobs[strand] holds per_read jobs for every read of who (NULL: the reads' own jobs).  Once per slice, never for a
 * single read, nor when the device or its memory is what is missing.  Returns 1 when reads were dropped: who and n_ok are closed
 * up (kept_from[k], if asked for, is the place the read now at k had before) and the caller starts both strands over; on 0 the
 * caller ends the run when rc is an error, for no read is to blame. */
typedef struct { const slice_t *sl; sa_job_t *const *jobs; int64_t per_read; } validate_ctx_t;
static void validate_one(int64_t j, void *ctx) {
    validate_ctx_t *v = ctx;
    read_t *rd = &v->sl->reads[v->sl->who[j]];
    const sa_job_t *jobs[2];
    for (int s = 0; s < 2; s++) jobs[s] = !v->jobs ? &rd->jobs[s] : v->jobs[s] ? v->jobs[s] + j * v->per_read : NULL;
    if (validate_read(v->sl->R, rd, jobs, v->per_read) != 0)
        fprintf(stderr, "[signalMachine] ERROR: read %s skipped: %s\n", rd->label, rd->err);
}
static int drop_refused_reads(slice_t *sl, int rc, sa_job_t *const *jobs, int64_t per_read, int64_t *kept_from) {
    if (sl->validated || rc == SA_OK || rc == SA_ENODEVICE || rc == SA_ENOMEM) return 0;
    sl->validated = 1;
    validate_ctx_t vc = {sl, jobs, per_read};
    parallel_for(sl->n_ok, validate_one, &vc);
    int64_t k = 0;
    for (int64_t j = 0; j < sl->n_ok; j++)
        if (!sl->reads[sl->who[j]].failed) {
            if (kept_from) kept_from[k] = j;
            sl->who[k++] = sl->who[j];
        }
    const int dropped = k < sl->n_ok;
    sl->n_ok = k;
    return dropped;
}

/* What one strand's batch of a slice leaves for the rendering, [job] each.  Without --mea the batch stays alive and pairs[job]
 * is NULL: a job's rows are expanded from the batch's packed records by the thread that renders the job. */
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
} strand_result_t;

/* a result of n_jobs jobs, filled as far as its batch got */
static void strand_result_free(strand_result_t *sr, int64_t n_jobs) {
    sa_batch_destroy(sr->batch);
    for (int64_t j = 0; j < n_jobs; j++) {
        if (sr->pairs) sa_free(sr->pairs[j]);
        if (sr->mea) sa_free(sr->mea[j]);
        if (sr->calls) sa_free(sr->calls[j]);
    }
    free(sr->pairs); free(sr->n_pairs); free(sr->mea); free(sr->n_mea); free(sr->all_n); free(sr->all_sum);
    free(sr->calls); free(sr->n_calls);
    free(sr->dev_reads); free(sr->dev_hist); free(sr->dev_ev_first);
    sa_free(sr->dev_sets); sa_free(sr->dev_events);
    memset(sr, 0, sizeof(*sr));
}

/* an alignment slice between its GPU stage and its rendering */
typedef struct {
    slice_t sl;
    sa_job_t *bj;              /* [job]: the jobs of the strand whose batch is being made */
    strand_result_t sr[2];
    double (*score)[2];        /* [job][strand] */
    unsigned char *tmpl_amb;   /* [job], --twoD with site calls: the template strand has a row on an ambiguous k-mer (order_calls) */
} align_slice_t;

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
    sa_pair_t *rows = xalloc(n_path, sizeof(sa_pair_t), 0);
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
    const int64_t ref_len = (int64_t) strlen(rd->st[s].target), ref_len_kmers = ref_len - k, off = rd->st[s].r_shift;
    call_pos_t *v = xalloc(n, sizeof(call_pos_t), 0);
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
    agg_entry_t **rows = xalloc((int64_t) g_agg.n, sizeof(agg_entry_t *), 0);
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

/* ---- --site-calls-accuracy: the calls scored against known truth (plot_variant_accuracy.py:44-175) in one sa_call_scores_t.
 * Levels 0 and 1 are added batch by batch while the batch's records lie in HBM (acc_add_batch), level 2 at the end of the run from
 * the over-reads table, in the six decimals it prints (acc_add_aggregate).  The accumulator's letters are those of the run's first
 * call, so it is made when that call is there.  A read named in --site-calls-truth-reads is labelled as a whole (generate_labels2),
 * every other site by the positions file (generate_labels); level 2 takes the positions file only. ---- */
typedef struct { int contig, strand; int64_t pos, line; char letter; } acc_truth_t;
typedef struct { char *label; char letter; } acc_label_t;
static struct {
    sa_call_scores_t *acc;
    int device, ck;                      /* ck: the accumulator was there, and checkpointed, when the slice began */
    char letters[SA_SITE_MAX_LETTERS + 1];
    char **contigs;                      /* a contig's index is its place here: the positions file's names first */
    int n_contigs;
    acc_truth_t *truth;                  /* sorted by (contig, pos, strand, line) */
    int64_t n_truth;
    acc_label_t *labels;                 /* sorted by label */
    int64_t n_labels;
} g_acc;
static int acc_contig(const char *name) {
    int ci = 0;
    while (ci < g_acc.n_contigs && strcmp(g_acc.contigs[ci], name) != 0) ci++;
    if (ci == g_acc.n_contigs) {
        g_acc.contigs = realloc(g_acc.contigs, sizeof(char *) * (size_t) (g_acc.n_contigs + 1));
        g_acc.contigs[g_acc.n_contigs++] = strdup(name);
    }
    return ci;
}
static int cmp_acc_truth(const void *a, const void *b) {
    const acc_truth_t *x = a, *y = b;
    if (x->contig != y->contig) return x->contig < y->contig ? -1 : 1;
    if (x->pos != y->pos) return x->pos < y->pos ? -1 : 1;
    if (x->strand != y->strand) return x->strand < y->strand ? -1 : 1;
    return x->line < y->line ? -1 : x->line > y->line;
}
static int cmp_acc_label(const void *a, const void *b) { return strcmp(((const acc_label_t *) a)->label, ((const acc_label_t *) b)->label); }
/* the two truth files, read before the run starts so that a bad one stops it */
static void acc_load(const run_t *R) {
    char line[4096], a[1024], st[64], from[64], to[64];
    if (R->acc_truth_path) {
        FILE *fh = fopen(R->acc_truth_path, "r");
        if (!fh) die("signalMachine: --site-calls-truth: cannot read %s", R->acc_truth_path);
        int64_t cap = 0, pos = 0;
        while (fgets(line, sizeof line, fh)) {
            if (line[0] == '\n' || line[0] == '#') continue;
            if (sscanf(line, "%1023s %" SCNd64 " %63s %63s %63s", a, &pos, st, from, to) != 5 || (strcmp(st, "+") && strcmp(st, "-")) || strlen(to) != 1)
                die("signalMachine: --site-calls-truth: not 'contig position +|- change_from change_to': %s", line);
            if (g_acc.n_truth == cap) g_acc.truth = realloc(g_acc.truth, sizeof(acc_truth_t) * (size_t) (cap = cap ? 2 * cap : 1024));
            g_acc.truth[g_acc.n_truth] = (acc_truth_t) {acc_contig(a), st[0] == '-', pos, g_acc.n_truth, to[0]};
            g_acc.n_truth++;
        }
        fclose(fh);
        qsort(g_acc.truth, (size_t) g_acc.n_truth, sizeof(acc_truth_t), cmp_acc_truth);
    }
    if (R->acc_reads_path) {
        FILE *fh = fopen(R->acc_reads_path, "r");
        if (!fh) die("signalMachine: --site-calls-truth-reads: cannot read %s", R->acc_reads_path);
        int64_t cap = 0;
        while (fgets(line, sizeof line, fh)) {
            if (line[0] == '\n' || line[0] == '#') continue;
            if (sscanf(line, "%1023s %63s", a, to) != 2 || strlen(to) != 1) die("signalMachine: --site-calls-truth-reads: not 'label letter': %s", line);
            if (g_acc.n_labels == cap) g_acc.labels = realloc(g_acc.labels, sizeof(acc_label_t) * (size_t) (cap = cap ? 2 * cap : 1024));
            g_acc.labels[g_acc.n_labels++] = (acc_label_t) {strdup(a), to[0]};
        }
        fclose(fh);
        qsort(g_acc.labels, (size_t) g_acc.n_labels, sizeof(acc_label_t), cmp_acc_label);
    }
}
/* index of the read's label letter in the accumulator's letters, -1 for a read without a label */
static int acc_read_letter(const char *label) {
    const acc_label_t key = {(char *) label, 0};
    const acc_label_t *e = g_acc.n_labels ? bsearch(&key, g_acc.labels, (size_t) g_acc.n_labels, sizeof(acc_label_t), cmp_acc_label) : NULL;
    if (!e) return -1;
    const char *at = strchr(g_acc.letters, e->letter);
    if (!at) die("signalMachine: --site-calls-truth-reads: the letter of read %s is not one of the sites' letters", label);
    return (int) (at - g_acc.letters);
}
/* the first line of the positions file that names (contig, pos, mapped strand): its change_to, 0 when none does */
static char acc_truth_letter(int contig, int64_t pos, int strand) {
    int64_t lo = 0, hi = g_acc.n_truth;
    const acc_truth_t key = {contig, strand, pos, -1, 0};
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (cmp_acc_truth(&g_acc.truth[mid], &key) < 0) lo = mid + 1; else hi = mid;
    }
    const acc_truth_t *e = lo < g_acc.n_truth ? &g_acc.truth[lo] : NULL;
    return e && e->contig == contig && e->pos == pos && e->strand == strand ? e->letter : 0;
}
/* the accumulator, made when the run has its first call: its letters are that call's */
static void acc_create(const run_t *R, const strand_result_t *sr, int64_t n) {
    for (int64_t j = 0; j < n && !g_acc.acc; j++) {
        if (sr->n_calls[j] <= 0) continue;
        const sa_site_call_t *c = &sr->calls[j][0];
        memcpy(g_acc.letters, c->letters, (size_t) c->n_letters);
        g_acc.letters[c->n_letters] = 0;
        sa_truth_site_t *t = xalloc(g_acc.n_truth, sizeof(*t), 1);
        for (int64_t i = 0; i < g_acc.n_truth; i++) {
            t[i].contig = g_acc.truth[i].contig; t[i].mapped_strand = g_acc.truth[i].strand; t[i].pos = g_acc.truth[i].pos;
            t[i].change_to = g_acc.truth[i].letter;
        }
        const int rc = sa_call_scores_create(&g_acc.acc, g_acc.letters, R->acc_bins, R->acc_threshold, t, g_acc.n_truth, g_acc.device);
        free(t);
        if (rc == SA_EINVAL) die("signalMachine: --site-calls-truth: a change_to letter is not one of the sites' letters %s, or a position is negative", g_acc.letters);
        if (rc != SA_OK) die("signalMachine: --site-calls-accuracy: %s", sa_strerror(rc));
    }
}
/* levels 0 and 1 of the slice's finished batch of strand s.  The mapping strand of a job is the one order_calls gives its calls. */
static int acc_add_batch(const align_slice_t *c, int s, sa_batch_t *b) {
    const run_t *R = c->sl.R;
    const int64_t nj = c->sl.n_ok;
    acc_create(R, &c->sr[s], nj);
    if (!g_acc.acc) return SA_OK;   /* (no call so far: nothing to score) */
    sa_score_job_map_t *map = xalloc(nj, sizeof(*map), 1);
    for (int64_t j = 0; j < nj; j++) {
        const read_t *rd = &c->sl.reads[c->sl.who[j]];
        const int idx = (s == 1 && c->tmpl_amb && c->tmpl_amb[j]) ? 1 : 0;
        const int along = (s == 0 && rd->forward) || (s == 1 && !rd->forward);   /* adjust_ref as x0 + x_sign * x */
        map[j].contig = acc_contig(rd->pA->contig1);
        map[j].x_sign = along ? 1 : -1;
        map[j].x0 = along ? rd->st[s].r_shift : rd->st[s].r_shift - R->sm[s].k;
        map[j].strand = s;
        map[j].mapped_strand = (idx == 0) == (rd->forward != 0) ? 0 : 1;
        map[j].true_letter = acc_read_letter(rd->label);
    }
    const int rc = sa_call_scores_add_batch(g_acc.acc, b, map, nj, NULL);
    free(map);
    return rc;
}
/* level 2: every row of the over-reads table whose letters are the accumulator's and whose site the positions file names, with
 * the values write_aggregate prints */
static void acc_add_aggregate(void) {
    const size_t nl = strlen(g_acc.letters);
    for (int strand = 0; strand < 2 && g_acc.acc; strand++) {
        double *prob = xalloc((int64_t) (g_agg.n * nl), sizeof(double), 0);
        int8_t *tl = xalloc((int64_t) g_agg.n, 1, 0);
        int64_t n = 0;
        for (size_t i = 0; i < g_agg.cap; i++) {
            const agg_entry_t *e = &g_agg.tab[i];
            if (!e->used || (e->strand == 't') != (strand == 0) || (size_t) e->n != nl) continue;
            double v[SA_SITE_MAX_LETTERS], total = 0.0;
            int ok = 1;
            for (size_t l = 0; l < nl && ok; l++) {   /* (the accumulator's letters are sorted: the table's column order) */
                int t = 0;
                while (t < e->n && e->letter[t] != g_acc.letters[l]) t++;
                ok = t < e->n;
                if (ok) { v[l] = e->sum[t]; total += v[l]; }
            }
            const char letter = ok ? acc_truth_letter(acc_contig(g_agg.contigs[e->contig]), e->pos, e->mapped == '-') : 0;
            const char *at = letter ? strchr(g_acc.letters, letter) : NULL;
            if (!at) continue;
            char num[40];
            for (size_t l = 0; l < nl; l++) {
                sa_format_py_round6(num, v[l] / total);
                prob[(size_t) n * nl + l] = strtod(num, NULL);
            }
            tl[n++] = (int8_t) (at - g_acc.letters);
        }
        const int rc = sa_call_scores_add_records(g_acc.acc, 2, strand, prob, tl, n);
        if (rc != SA_OK) die("signalMachine: --site-calls-accuracy: %s", sa_strerror(rc));
        free(prob); free(tl);
    }
}
static void write_accuracy(const run_t *R) {
    if (!R->acc_path) return;
    sa_call_score_row_t *rows = NULL;
    int64_t n_rows = 0, *curves = NULL;
    sa_call_scores_counts_t counts = {0, 0};
    if (g_acc.acc) {
        acc_add_aggregate();
        const int rc = sa_call_scores_finish(g_acc.acc, &rows, &n_rows, &curves, &counts, NULL);
        if (rc != SA_OK) die("signalMachine: --site-calls-accuracy: %s", sa_strerror(rc));
    }
    if (sa_call_scores_write(R->acc_path, R->acc_curves_path, R->acc_bins, rows, n_rows, curves) != SA_OK)
        die("signalMachine: cannot write %s", R->acc_path);
    fprintf(stderr, "[signalMachine] accuracy: %" PRId64 " rows; %" PRId64 " calls without truth dropped, %" PRId64 " sites of other letters skipped\n",
            n_rows, counts.unlabelled, counts.other_sites);
    sa_free(rows); sa_free(curves);
    sa_call_scores_destroy(g_acc.acc);
    g_acc.acc = NULL;
}

static out_ctx_t out_ctx_for(const run_t *R, const read_t *rd, int s, const sa_pair_t *pairs, int64_t n_pairs, double score) {
    out_ctx_t o;
    o.label = rd->label; o.contig = rd->pA->contig1; o.sm = &R->sm[s]; o.npp = *np_params(rd->np, s);
    o.events = np_events(rd->np, s); o.target = rd->st[s].target; o.forward = rd->forward; o.is_template = s == 0;
    o.rna = R->rna; o.event_offset = rd->st[s].lo; o.ref_offset = rd->st[s].r_shift; o.pairs = pairs;
    o.n_pairs = n_pairs; o.score = score;
    return o;
}

/* The rows of job j, expanded from the packed records the strand's batch holds in page-locked memory.  This runs job by job on
 * the rendering threads: the GPU stage does not expand every job's pairs into freshly allocated sa_pair_t arrays on the main
 * thread (523 MB per slice of 2048 long reads).  NULL, and the read marked failed, when the records cannot be had.
 * 8-byte records (-s 0 / 2 on reads without ambiguity letters -- half the bytes over PCIe where the pairs outweigh the kernels,
 * e.g. --sm3Hdp -D 0.01) hold x, y and the probability; the pair's k-mer is the reference's at x, its path 0. */
static sa_pair_t *expand_job_pairs(const run_t *R, read_t *rd, int s, const strand_result_t *sr, int64_t j) {
    const sa_pair8_t *pk8 = NULL;
    const sa_pair16_t *pk16 = NULL;
    int64_t n = 0;
    const int rc = sr->p8 ? sa_batch_pairs8(sr->batch, j, &pk8, &n) : sa_batch_pairs16(sr->batch, j, &pk16, &n);
    if (rc != SA_OK || n != sr->n_pairs[j]) {
        fprintf(stderr, "[signalMachine] ERROR: read %s: results of the batch are not readable\n", rd->label);
        rd->failed = 1;
        return NULL;
    }
    sa_pair_t *rows = xalloc(n, sizeof(sa_pair_t), 0);
    if (!sr->p8) {
        for (int64_t i = 0; i < n; i++) rows[i] = sa_pair16_unpack(pk16[i]);
        return rows;
    }
    int bad_kmer = 0;
    for (int64_t i = 0; i < n; i++) {
        sa_pair_t *q = &rows[i];
        sa_pair8_unpack(pk8[i], &q->prob_e7, &q->x, &q->y);
        q->path = 0;
        q->kmer_id = kmer_id_of(&R->sm[s], rd->st[s].target + q->x);
        bad_kmer |= q->kmer_id < 0;
    }
    if (bad_kmer) {   /* (cannot happen: the planner refuses a reference with a letter outside the model's alphabet) */
        fprintf(stderr, "[signalMachine] ERROR: read %s: a pair names a k-mer outside the model's alphabet\n", rd->label);
        rd->failed = 1;
        free(rows);
        return NULL;
    }
    return rows;
}

static void output_one(int64_t j, void *ctx) {
    align_slice_t *c = ctx;
    const run_t *R = c->sl.R;
    read_t *rd = &c->sl.reads[c->sl.who[j]];
    if (R->out_fmt == 3 && rd->post_path2 == NULL) {
        fprintf(stderr, "[signalMachine] ERROR: read %s: 'both' output format needs a second output file\n", rd->label);
        rd->failed = 1;
        return;
    }
    sa_pair_t *mine[2] = {NULL, NULL};
    const sa_pair_t *pp[2] = {NULL, NULL};
    for (int s = 0; s < n_strands(R); s++) {
        const strand_result_t *sr = &c->sr[s];
        pp[s] = sr->pairs[j];
        if (pp[s] != NULL || sr->batch == NULL) continue;
        pp[s] = mine[s] = expand_job_pairs(R, rd, s, sr, j);
        if (mine[s] == NULL) {
            free(mine[0]);
            return;
        }
    }
    for (int s = 0; s < n_strands(R); s++) {
        const strand_result_t *sr = &c->sr[s];
        double tot = 0.0;
        int64_t n_all = sr->n_pairs[j];
        if (sr->all_n) {   /* (prob_e7 sums are integers below 2^53: the same double as the loop below gives) */
            n_all = sr->all_n[j];
            tot = (double) sr->all_sum[j];
        } else {
            for (int64_t i = 0; i < sr->n_pairs[j]; i++) tot += (double) pp[s][i].prob_e7;
        }
        c->score[j][s] = 100.0 * tot / ((double) n_all * PROB_1); /* scoreByPosteriorProbabilityIgnoringGaps :407-412 */
    }
    const int tmpl_amb = c->tmpl_amb && has_ambiguous_rows(R->ambig, rd->st[0].target, R->sm[0].k, pp[0], c->sr[0].n_pairs[j]);
    if (c->tmpl_amb) c->tmpl_amb[j] = (unsigned char) tmpl_amb;
    for (int s = 0; s < n_strands(R) && rd->post_path != NULL; s++) {
        const strand_result_t *sr = &c->sr[s];
        const out_ctx_t o = out_ctx_for(R, rd, s, pp[s], sr->n_pairs[j], c->score[j][s]);
        output_alignment(R->out_fmt, rd->post_path, rd->post_path2, &o);
        if (R->mea) write_mea(rd->post_path, &o, sr->mea[j], sr->n_mea[j]);
        if (R->site_calls) write_calls(rd->post_path, rd, s, tmpl_amb, sr->calls[j], sr->n_calls[j], R->sm[s].k);
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

/* --train-mixture-motifs: the (canonical, modified) k-mer ids of every motif pair of the list, for the model of strand s:
 * get_motif_kmer_pairs with the reference's flanks (A, T, G, C), the pairs of all motifs as one sorted set (mixture_model.py
 * main(): a set union).  A malformed list or a letter outside the model's alphabet ends the run with the usage text. */
typedef struct {
    int32_t canonical, modified;
    char name[2][24];
} mix_pair_t;

static int cmp_mix_pair(const void *a, const void *b) {
    const mix_pair_t *x = a, *y = b;
    const int c = strcmp(x->name[0], y->name[0]);
    return c ? c : strcmp(x->name[1], y->name[1]);
}

static int64_t mixture_pairs(const run_t *R, int s, mix_pair_t **out) {
    const strand_model_t *sm = &R->sm[s];
    char *list = strdup(R->mix_motifs), *save = NULL;
    mix_pair_t *v = NULL;
    int64_t n = 0;
    if (R->mix_motifs[0] == 0 || R->mix_motifs[strlen(R->mix_motifs) - 1] == ',' || strstr(R->mix_motifs, ",,")) {
        usage();
        die("signalMachine: --train-mixture-motifs: malformed list %s", R->mix_motifs);
    }
    for (char *item = strtok_r(list, ",", &save); item; item = strtok_r(NULL, ",", &save)) {
        char *colon = strchr(item, ':');
        if (!colon || colon == item || colon[1] == 0 || strchr(colon + 1, ':')) {
            usage();
            die("signalMachine: --train-mixture-motifs: expected <canonical>:<modified>, got %s", item);
        }
        *colon = 0;
        for (const char *m = item; m; m = m == item ? colon + 1 : NULL)
            for (const char *c = m; *c; c++)
                if (!memchr(sm->alphabet, toupper((unsigned char) *c), (size_t) sm->n_alpha)) {
                    usage();
                    die("signalMachine: --train-mixture-motifs: a letter of %s is not in the model's alphabet", m);
                }
        char *pairs = NULL;
        int64_t np = 0;
        if (sm->k >= (int) sizeof(v->name[0]) || sa_motif_kmer_pairs(sm->k, item, colon + 1, NULL, &pairs, &np) != SA_OK) {
            usage();
            die("signalMachine: --train-mixture-motifs: %s and its partner must differ in one letter, the first of them made of A, C, G, T", item);
        }
        v = realloc(v, (size_t) (n + np + 1) * sizeof(mix_pair_t));
        if (!v) die("signalMachine: out of memory%s", "");
        for (int64_t i = 0; i < np; i++) {
            mix_pair_t *q = &v[n];
            snprintf(q->name[0], sizeof q->name[0], "%s", pairs + (2 * i) * (sm->k + 1));
            snprintf(q->name[1], sizeof q->name[1], "%s", pairs + (2 * i + 1) * (sm->k + 1));
            q->canonical = (int32_t) sa_kmer_id(sm->model, q->name[0]);
            q->modified = (int32_t) sa_kmer_id(sm->model, q->name[1]);
            if (q->canonical >= 0 && q->modified >= 0) n++;
        }
        sa_free(pairs);
    }
    free(list);
    if (n) qsort(v, (size_t) n, sizeof(mix_pair_t), cmp_mix_pair);
    int64_t m = 0;
    for (int64_t i = 0; i < n; i++)
        if (m == 0 || cmp_mix_pair(&v[m - 1], &v[i]) != 0) v[m++] = v[i];
    *out = v;
    return m;
}

typedef struct {
    const char *kmer;
    double v[7];            /* canonical model mean, sd; canonical mixture mean, sd; modified mixture mean, sd; distance */
    int strand;
} mix_row_t;

static int cmp_mix_row(const void *a, const void *b) {   /* distance descending, then k-mer, then strand */
    const mix_row_t *x = a, *y = b;
    if (x->v[6] != y->v[6]) return x->v[6] > y->v[6] ? -1 : 1;
    const int c = strcmp(x->kmer, y->kmer);
    return c ? c : x->strand - y->strand;
}

/* generate_gaussian_mixture_model_for_motifs (mixture_model.py:122-186) per strand: K = 2 with sklearn's defaults on the rows of
 * every pair's canonical k-mer, closest_to_canonical against the -T / -C file's level mean, the other component into the
 * modified k-mer's row ({n = 1, m, s} at weight 0 gives m and s back exactly, and the mean^3 / sd^2 lambda of
 * set_kmer_event_mean_params).  The distances of all strands go into one file. */
static void write_mixture(run_t *R, const char *t_model, const char *c_model) {
    if (!R->mix_motifs) return;
    mix_row_t *rows = NULL;
    mix_pair_t *pairs[2] = {NULL, NULL};
    int64_t n_rows = 0;
    for (int s = 0; s < n_strands(R); s++) {
        if (!R->mix_model[s] && !R->mix_dist) continue;
        const strand_model_t *sm = &R->sm[s];
        int64_t nk = 1;
        for (int i = 0; i < sm->k; i++) nk *= sm->n_alpha;
        const int64_t np = mixture_pairs(R, s, &pairs[s]);
        int32_t *ids = xalloc(np, sizeof(int32_t), 1);
        sa_mixture_fit_t *fit = xalloc(np, sizeof(sa_mixture_fit_t), 1);
        sa_kmer_stat_t *st = xalloc(nk, sizeof(sa_kmer_stat_t), 1);
        uint8_t *mask = xalloc(nk, 1, 1);
        for (int64_t i = 0; i < np; i++) ids[i] = pairs[s][i].canonical;
        const sa_mixture_params_t mp = {2, 100, 1e-3, 1e-6};
        if (np > 0 && sa_kmer_table_mixture(R->train_tab[s], s, ids, np, &mp, NULL, fit, NULL) != SA_OK)
            die("signalMachine: --train-mixture-*: the fit failed%s", "");
        rows = realloc(rows, (size_t) (n_rows + np + 1) * sizeof(mix_row_t));
        if (!rows) die("signalMachine: out of memory%s", "");
        for (int64_t i = 0; i < np; i++) {
            const mix_pair_t *q = &pairs[s][i];
            int32_t match = 0, other = 1;
            double distance = 0;
            if (fit[i].status != 0 || sa_mixture_assign(&fit[i], sm->table_orig[5 * q->canonical], &match, &other, &distance) != SA_OK) {
                fprintf(stderr, "No alignments found for kmer: %s\n", q->name[0]);
                continue;
            }
            st[q->modified].n = 1;
            st[q->modified].m = fit[i].mean[other];
            st[q->modified].s = fit[i].sd[other];
            mask[q->modified] = 1;
            mix_row_t *r = &rows[n_rows++];
            r->kmer = q->name[0];
            r->strand = s;
            r->v[0] = sm->table_orig[5 * q->canonical]; r->v[1] = sm->table_orig[5 * q->canonical + 1];
            r->v[2] = fit[i].mean[match]; r->v[3] = fit[i].sd[match];
            r->v[4] = fit[i].mean[other]; r->v[5] = fit[i].sd[other];
            r->v[6] = distance;
        }
        if (R->mix_model[s] && sa_model_write_trained(s ? c_model : t_model, st, 0.0, 0.0, 0, mask, R->mix_model[s]) != SA_OK)
            die("signalMachine: cannot write %s", R->mix_model[s]);
        free(ids);
        free(fit);
        free(st);
        free(mask);
    }
    if (R->mix_dist) {
        FILE *f = fopen(R->mix_dist, "w");
        if (!f) die("signalMachine: cannot write %s", R->mix_dist);
        if (n_rows) qsort(rows, (size_t) n_rows, sizeof(mix_row_t), cmp_mix_row);
        fprintf(f, "kmer\tcanonical_model_mean\tcanonical_model_sd\tcanonical_mixture_mean\tcanonical_mixture_sd\tmodified_mixture_mean\t"
                   "modified_mixture_sd\tdistance\tstrand\n");
        for (int64_t i = 0; i < n_rows; i++) {
            fputs(rows[i].kmer, f);
            for (int q = 0; q < 7; q++) {
                char num[40];
                sa_format_py_repr(num, rows[i].v[q]);
                fprintf(f, "\t%s", num);
            }
            fprintf(f, "\t%c\n", rows[i].strand ? 'c' : 't');
        }
        if (fclose(f) != 0) die("signalMachine: cannot write %s", R->mix_dist);
    }
    free(rows);
    free(pairs[0]);
    free(pairs[1]);
}

/* --train-*: the assignments table (generate_top_n_kmers_from_sa_output) and the retrained models (train_normal_emmissions:
 * the prior is the -T / -C file as written on disk) */
static void write_training(run_t *R, const char *t_model, const char *c_model, int device) {
    if (!R->want_train) return;
    for (int s = 0; s < n_strands(R); s++)   /* (a run without a read that aligned: empty tables) */
        if (!R->train_tab[s] && sa_kmer_table_create(&R->train_tab[s], R->sm[s].model, R->train_n, R->train_min_prob, device) != SA_OK)
            die("signalMachine: --train-*: no k-mer table%s", "");
    if (R->train_assign) {   /* the template table's 't' rows, then the complement table's 'c' rows */
        for (int s = 0; s < n_strands(R); s++)
            if (sa_kmer_table_write(R->train_tab[s], s, R->train_assign, s > 0) != SA_OK) die("signalMachine: cannot write %s", R->train_assign);
    }
    for (int s = 0; s < n_strands(R); s++) {
        if (!R->train_model[s]) continue;
        const strand_model_t *sm = &R->sm[s];
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
    write_mixture(R, t_model, c_model);
    for (int s = 0; s < 2; s++) { sa_kmer_table_destroy(R->train_tab[s]); R->train_tab[s] = NULL; }
}

/* One strand's batch of a slice.  jobs[i] belongs to reads[who[i / per_read]] (per_read > 1: --snp-step's substituted copies).
 * --emission twoDist: a single read brings its own model; the reads of a manifest share the strand's two-distribution model and
 * each job gets the scale_sd / var_sd its read's parameter estimation left (emissions_signal_scaleNoise, applied inside the batch:
 * SA_FLAG_TWO_DIST_ALL_KERNELS, whatever kernel family a read's regions take). */
static int create_strand_batch(sa_batch_t **b, const slice_t *sl, int strand, const sa_job_t *jobs, int64_t n_jobs, int64_t per_read,
                               unsigned flags) {
    const run_t *R = sl->R;
    const strand_model_t *sm = &R->sm[strand];
    if (!R->two_dist) return sa_batch_create(b, sm->model, &R->p, jobs, n_jobs, R->ambig, sl->device, flags);
    if (!R->batch_mode) return sa_batch_create(b, sl->reads[sl->who[0]].model[strand], &R->p, jobs, n_jobs, R->ambig, sl->device, flags);
    sa_noise_scale_t *nz = xalloc(n_jobs, sizeof(sa_noise_scale_t), 0);
    for (int64_t i = 0; i < n_jobs; i++) {
        const sa_strand_params_t *pp = np_params(sl->reads[sl->who[i / per_read]].np, strand);
        nz[i].scale_sd = pp->scale_sd;
        nz[i].var_sd = pp->var_sd;
    }
    const int rc = sa_batch_create_noise_scaled(b, sm->model_two, &R->p, jobs, nz, n_jobs, R->ambig, sl->device,
                                                flags | SA_FLAG_TWO_DIST_ALL_KERNELS);
    free(nz);
    return rc;
}

/* Expectations mode (-t / -c, impl/signalMachine.c:772-848): sa_expect_batch per strand, the .expectations file of every read */
static int64_t run_slice_expect(run_t *R, read_t *reads, int64_t n_reads, int device) {
    slice_t sl;
    slice_open(&sl, R, reads, n_reads, device);
    const int64_t n_ok = sl.n_ok;
    sa_job_t *bj = xalloc(n_ok, sizeof(sa_job_t), 0);
    if (n_ok > 0) fprintf(stderr, "Starting expectations routine\n");
    for (int s = 0; s < n_strands(R) && n_ok > 0; s++) {
        fprintf(stderr, "signalAlign - getting expectations for %s\n", strand_name(s));
        for (int64_t j = 0; j < n_ok; j++) bj[j] = reads[sl.who[j]].jobs[s];
        double *trans = xalloc(9 * n_ok, sizeof(double), 0), *lik = xalloc(n_ok, sizeof(double), 1);
        for (int64_t j = 0; j < 9 * n_ok; j++) trans[j] = 0.001; /* transitionsPseudocount, :785 */
        sa_assignment_t **as = xalloc(n_ok, sizeof(*as), 1);
        int64_t *n_as = xalloc(n_ok, sizeof(int64_t), 1);
        int rc = sa_expect_batch(R->sm[s].model, &R->p, bj, n_ok, R->ambig, device, 0, trans, lik, as, n_as);
        if (rc != SA_OK) die("signalMachine: expectations failed: %s", sa_strerror(rc));
        for (int64_t j = 0; j < n_ok; j++) {
            read_t *rd = &reads[sl.who[j]];
            if (R->hdp)
                fprintf(stderr, s == 0 ? "signalAlign - got %" PRId64 " template HDP assignments\n"
                                       : "signalAlign - got %" PRId64 "complement HDP assignments\n", n_as[j]);
            if (rd->expect[s] != NULL) {
                fprintf(stderr, "signalAlign - writing expectations to file: %s\n", rd->expect[s]);
                write_expectations(rd->expect[s], &R->sm[s], np_params(rd->np, s), R->hdp, R->p.threshold, trans + 9 * j, lik[j],
                                   &rd->jobs[s], as[j], n_as[j]);
            }
            sa_free(as[j]);
        }
        free(trans); free(lik); free(as); free(n_as);
    }
    for (int64_t j = 0; j < n_ok; j++) report_read(R, &reads[sl.who[j]], NULL, NULL);
    free(bj);
    return slice_close(&sl);
}

static int snp_contig_pos_is_forward(const read_t *rd, int s);
static int64_t snp_contig_index(const run_t *R, const read_t *rd);

/* --position-profile: the slice's finished template batch added to the run's table.  Job j is read j's template strand, and where
 * its target lies on the contig is snp_contig_pos written as an affine map, as snp_add_to_marginals does */
static int profile_add_batch(const align_slice_t *c, sa_batch_t *b) {
    const run_t *R = c->sl.R;
    const int64_t nj = c->sl.n_ok;
    sa_profile_job_map_t *map = xalloc(nj, sizeof(*map), 1);
    for (int64_t j = 0; j < nj; j++) {
        const read_t *rd = &c->sl.reads[c->sl.who[j]];
        const int same = snp_contig_pos_is_forward(rd, 0);
        map[j].contig = (int32_t) snp_contig_index(R, rd);
        map[j].pos_sign = same ? 1 : -1;
        map[j].pos0 = same ? rd->st[0].r_shift : rd->st[0].r_shift - 1;
    }
    const int rc = sa_position_profile_add_batch(R->prof_tab, b, map, nj, 0, NULL);
    free(map);
    return rc;
}

/* --guide-deviation: the finished batch of strand s against its own jobs' anchors, with the MEA paths just made of it */
static int deviation_of_batch(align_slice_t *c, int s, sa_batch_t *b) {
    const run_t *R = c->sl.R;
    strand_result_t *sr = &c->sr[s];
    const int64_t n = c->sl.n_ok;
    sa_deviation_job_t *dj = xalloc(n, sizeof(*dj), 1);
    sr->dev_ev_first = xalloc(n + 1, sizeof(int64_t), 1);
    for (int64_t j = 0; j < n; j++) {
        const sa_job_t *q = &c->bj[j];
        dj[j] = (sa_deviation_job_t) {q->anchor_x, q->anchor_y, q->n_anchors, q->n_events};
        sr->dev_ev_first[j + 1] = sr->dev_ev_first[j] + q->n_events;
    }
    sr->dev_reads = xalloc(n, sizeof(sa_deviation_read_t), 1);
    sr->dev_hist = xalloc(n * R->dev_params.n_buckets, sizeof(int32_t), 1);
    int64_t n_sets = 0;
    const int rc = sa_batch_guide_deviation(b, dj, n, (const sa_mea_pair_t *const *) sr->mea, sr->n_mea, &R->dev_params,
                                            R->dev_events_path ? SA_DEV_EVENTS : 0u, sr->dev_reads, &sr->dev_sets, &n_sets, sr->dev_hist, NULL,
                                            R->dev_events_path ? &sr->dev_events : NULL, NULL);
    free(dj);
    return rc;
}

/* ... and the lines of job j's strand s, in read order (render_slice).  Events are printed as the TSV's event_index column prints
 * them, positions as its reference_index maps x; diff stays in the job's coordinates. */
static void write_deviation(run_t *R, const read_t *rd, int s, const strand_result_t *sr, int64_t j) {
    const sa_deviation_read_t *r = &sr->dev_reads[j];
    const int nb = R->dev_params.n_buckets;
    const int64_t lo = rd->st[s].lo;
    const char *strand = s == 0 ? "t" : "c";
    char mean[400];
    mean[sa_format_f6(mean, r->n_aligned ? (double) r->sum_abs / (double) r->n_aligned : 0.0)] = 0;
    fprintf(R->dev_fh, "R\t%s\t%s\t%d\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%s\t%d\t%d\t%" PRId64 "\t%d\n", rd->label, strand, r->status,
            r->n_aligned, r->n_flagged, r->n_on_mea, mean, r->max_abs, r->max_abs_mea, r->n_aligned ? lo + r->max_event : (int64_t) -1, r->n_sets);
    fprintf(R->dev_fh, "H\t%s\t%s", rd->label, strand);
    for (int q = 0; q < nb; q++) {
        fprintf(R->dev_fh, "\t%d", sr->dev_hist[j * nb + q]);
        R->dev_total[q] += sr->dev_hist[j * nb + q];
    }
    fputc('\n', R->dev_fh);
    for (int64_t i = 0; i < r->n_sets; i++) {
        const sa_deviation_set_t *t = &sr->dev_sets[r->set_first + i];
        fprintf(R->dev_fh, "S\t%s\t%s\t%" PRId64 "\t%" PRId64 "\t%d\t%d\t%d\t%" PRId64 "\t%d\n", rd->label, strand, lo + t->first_event,
                lo + t->last_event, t->count, t->peak, t->mea_peak, lo + t->center_event, t->open_end);
    }
    if (!R->dev_events_fh) return;
    const int64_t ref_len = (int64_t) strlen(rd->st[s].target), ref_len_kmers = ref_len - R->sm[s].k, off = rd->st[s].r_shift;
    const sa_deviation_event_t *ev = sr->dev_events + sr->dev_ev_first[j];
    for (int64_t y = 0; y < sr->dev_ev_first[j + 1] - sr->dev_ev_first[j]; y++) {
        if (!(ev[y].flags & 1u)) continue;
        fprintf(R->dev_events_fh, "%s\t%s\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%d\t%d\t%d\n", rd->label, strand, lo + y,
                adjust_ref(ev[y].best_x, off, ref_len_kmers, ref_len, s == 0, rd->forward),
                adjust_ref(ev[y].guide, off, ref_len_kmers, ref_len, s == 0, rd->forward), ev[y].diff, (int) ((ev[y].flags >> 1) & 1u),
                (int) ((ev[y].flags >> 2) & 1u));
    }
}

/* Creates, runs and harvests the batch of strand s of an alignment slice into c->sr[s]; whatever it returns, the result is one
 * strand_result_free can take.
 * -s 1 prints only the rows whose reference k-mer holds an X: the others stay on the device (SA_FLAG_VC_ROWS), the run's pair
 * count and score come from the totals the device kept.
 * --site-calls / --site-calls-aggregate: every batch records its sites (SA_FLAG_SITE_CALLS) and keeps every row (the calls are
 * made of the rows SA_FLAG_VC_ROWS would drop; -s 1 then filters on the host, write_vc).
 * -s 0 / -s 2 without --mea: 8-byte result records where the batch allows them (one path per cell: no ambiguity letter in any
 * read's reference; fewer than 2^20 positions and events per read) -- the planner says SA_EUNSUPPORTED otherwise and the strand's
 * batch is made again with 16-byte records.  SA_CLI_PAIRS16=1: always 16-byte records (the test's checker).
 * --train-*: the strand's rows go into the run's k-mer table right after its batch ran, while the records are still in HBM.
 * --mea: the pairs are copied out while the batch still has them on the device for the path step; the batch ends here.
 * --guide-deviation: the batch is made and harvested as with --mea, and its deviation from the guide follows the paths.
 * Otherwise the batch stays alive for the rendering, which expands its packed records job by job. */
static int run_strand_batch(align_slice_t *c, int s) {
    const slice_t *sl = &c->sl;
    run_t *R = sl->R;
    strand_result_t *sr = &c->sr[s];
    const int64_t n = sl->n_ok;
    const int want_calls = R->site_calls || R->want_agg;
    const int want_mea = R->mea || R->dev_path != NULL;
    unsigned flags = want_calls ? SA_FLAG_SITE_CALLS : 0u, p8 = 0u;
    if (!want_mea && !want_calls) {
        if (R->out_fmt == 1 && !R->want_train && !getenv("SA_CLI_VC_ON_HOST")) flags |= SA_FLAG_VC_ROWS;
        if ((R->out_fmt == 0 || R->out_fmt == 2) && !getenv("SA_CLI_PAIRS16") && !R->prof_tab) p8 = SA_FLAG_PAIRS8;   /* (the profile reads path k-mers) */
    }
    for (int64_t j = 0; j < n; j++) c->bj[j] = sl->reads[sl->who[j]].jobs[s];
    sr->pairs = xalloc(n, sizeof(sa_pair_t *), 1);
    sr->n_pairs = xalloc(n, sizeof(int64_t), 1);
    if (want_calls) {
        sr->calls = xalloc(n, sizeof(sa_site_call_t *), 1);
        sr->n_calls = xalloc(n, sizeof(int64_t), 1);
    }
    if (want_mea) {
        sr->mea = xalloc(n, sizeof(sa_mea_pair_t *), 1);
        sr->n_mea = xalloc(n, sizeof(int64_t), 1);
    }
    sa_batch_t *b = NULL;
    int rc = create_strand_batch(&b, sl, s, c->bj, n, 1, flags | p8);
    sr->p8 = rc == SA_OK && p8 != 0;
    if (rc == SA_EUNSUPPORTED && p8) rc = create_strand_batch(&b, sl, s, c->bj, n, 1, flags);
    if (rc == SA_OK) rc = sa_batch_run(b);
    if (rc == SA_OK && want_calls) rc = sa_batch_site_calls(b, 0, sr->calls, sr->n_calls, NULL);
    /* --site-calls-accuracy: scored while the records are in HBM.  (A 2-D run's complement waits for the rendering, which finds out
     * the mapping strand of its calls: render_slice.) */
    if (rc == SA_OK && R->acc_path && !(s == 1 && R->two_d)) {
        rc = acc_add_batch(c, s, b);
        if (rc != SA_OK) die("signalMachine: --site-calls-accuracy: %s", sa_strerror(rc));
    }
    if (rc == SA_OK && R->want_train) {   /* (a batch that ran: nothing a retry without some reads would change) */
        rc = sa_kmer_table_add_batch(R->train_tab[s], b, c->bj, n, s, NULL);
        if (rc != SA_OK) die("signalMachine: --train-*: %s", sa_strerror(rc));
    }
    if (rc == SA_OK && R->prof_tab && s == 0) {
        rc = profile_add_batch(c, b);
        if (rc != SA_OK) die("signalMachine: --position-profile: %s", sa_strerror(rc));
    }
    if (want_mea) {
        for (int64_t j = 0; j < n && rc == SA_OK; j++) {
            sa_batch_n_pairs(b, j, &sr->n_pairs[j]);
            sr->pairs[j] = xalloc(sr->n_pairs[j], sizeof(sa_pair_t), 0);
            rc = sa_batch_pairs(b, j, sr->pairs[j], sr->n_pairs[j]);
        }
        if (rc == SA_OK) rc = sa_batch_mea(b, 0, sr->mea, sr->n_mea, NULL, NULL, NULL);
        if (rc == SA_OK && R->dev_path) {
            rc = deviation_of_batch(c, s, b);
            if (rc != SA_OK) die("signalMachine: --guide-deviation: %s", sa_strerror(rc));
        }
        sa_batch_destroy(b);
        return rc;
    }
    for (int64_t j = 0; j < n && rc == SA_OK; j++) rc = sa_batch_n_pairs(b, j, &sr->n_pairs[j]);
    if ((flags & SA_FLAG_VC_ROWS) && rc == SA_OK) {
        sr->all_n = xalloc(n, sizeof(int64_t), 1);
        sr->all_sum = xalloc(n, sizeof(int64_t), 1);
        for (int64_t j = 0; j < n && rc == SA_OK; j++) rc = sa_batch_all_pairs_summary(b, j, &sr->all_n[j], &sr->all_sum[j]);
    }
    /* only the packed pairs (pinned host memory) are read from here on: the batch's HBM goes back now, so that the
     * complement strand's batch plans into the whole card */
    if (rc == SA_OK) rc = sa_batch_release_device(b);
    if (rc == SA_OK) sr->batch = b;
    else sa_batch_destroy(b);
    return rc;
}

/* rendering of an alignment slice (one file per read, in parallel), summary lines in read order */
static void render_slice(align_slice_t *c) {
    const slice_t *sl = &c->sl;
    const run_t *R = sl->R;
    const double ts2 = now_s();
    c->score = xalloc(sl->n_ok, sizeof(*c->score), 1);
    c->tmpl_amb = (R->two_d && c->sr[1].calls) ? xalloc(sl->n_ok, 1, 1) : NULL;
    if (outputs_distinct(sl->reads, sl->who, sl->n_ok)) parallel_for(sl->n_ok, output_one, c);
    else for (int64_t j = 0; j < sl->n_ok; j++) output_one(j, c);
    for (int64_t j = 0; j < sl->n_ok; j++) {
        const read_t *rd = &sl->reads[sl->who[j]];
        if (rd->failed) continue;
        int64_t n_all[2] = {0, 0};
        for (int s = 0; s < n_strands(R); s++) {
            const strand_result_t *sr = &c->sr[s];
            n_all[s] = sr->all_n ? sr->all_n[j] : sr->n_pairs[j];
            /* (the aggregate's sums over reads are taken here, in read order: they do not depend on the rendering threads) */
            if (R->want_agg) agg_add_read(rd, s, c->tmpl_amb && c->tmpl_amb[j], sr->calls[j], sr->n_calls[j], R->sm[s].k);
        }
        report_read(R, rd, n_all, c->score[j]);
        for (int s = 0; s < n_strands(R) && R->dev_path; s++) write_deviation(sl->R, rd, s, &c->sr[s], j);
    }
    if (R->acc_path && R->two_d && c->sr[1].batch && sl->n_ok > 0) {   /* (the records go up again from the batch's host copy) */
        const int rc = acc_add_batch(c, 1, c->sr[1].batch);
        if (rc != SA_OK) die("signalMachine: --site-calls-accuracy: %s", sa_strerror(rc));
    }
    free(c->tmpl_amb);
    free(c->score);
    for (int s = 0; s < 2; s++) strand_result_free(&c->sr[s], sl->n_ok);
    t_add(&g_t_render, now_s() - ts2);
}

/* Alignment mode: the pair-HMM on the GPU, one batch per strand model with all reads side by side, then the outputs */
static int64_t run_slice_align(run_t *R, read_t *reads, int64_t n_reads, int device) {
    align_slice_t c;
    memset(&c, 0, sizeof(c));
    slice_t *sl = &c.sl;
    /* (the host side of the slice's reads has run: slice_prepare, a slice ahead of this function) */
    slice_open(sl, R, reads, n_reads, device);
    const double ts1 = now_s();
    c.bj = xalloc(sl->n_ok, sizeof(sa_job_t), 0);
    /* --train-*: the tables are checkpointed here, so that the retry below (a read the planner refuses) can take the slice's
     * rows back */
    for (int s = 0; s < n_strands(R) && R->want_train; s++) {
        int rc = R->train_tab[s] ? SA_OK : sa_kmer_table_create(&R->train_tab[s], R->sm[s].model, R->train_n, R->train_min_prob, device);
        if (rc == SA_OK) rc = sa_kmer_table_checkpoint(R->train_tab[s]);
        if (rc != SA_OK) die("signalMachine: --train-*: %s", sa_strerror(rc));
    }
    /* --position-profile: the same for its table */
    if (R->prof_tab && sa_position_profile_checkpoint(R->prof_tab) != SA_OK) die("signalMachine: --position-profile: checkpoint failed%s", "");
    /* --site-calls-accuracy: the same; an accumulator that this slice makes is given up instead */
    g_acc.ck = g_acc.acc != NULL;
    if (g_acc.ck && sa_call_scores_checkpoint(g_acc.acc) != SA_OK) die("signalMachine: --site-calls-accuracy: checkpoint failed%s", "");
    for (int s = 0; s < n_strands(R) && sl->n_ok > 0; s++) {
        fprintf(stderr, "signalAlign - starting %s alignment\n", strand_name(s));
        const int64_t n_jobs = sl->n_ok;
        const int rc = run_strand_batch(&c, s);
        if (drop_refused_reads(sl, rc, NULL, 1, NULL)) {
            for (int q = 0; q < n_strands(R) && R->want_train; q++)
                if (sa_kmer_table_rollback(R->train_tab[q]) != SA_OK) die("signalMachine: --train-*: rollback failed%s", "");
            if (R->prof_tab && sa_position_profile_rollback(R->prof_tab) != SA_OK) die("signalMachine: --position-profile: rollback failed%s", "");
            if (g_acc.acc && g_acc.ck && sa_call_scores_rollback(g_acc.acc) != SA_OK) die("signalMachine: --site-calls-accuracy: rollback failed%s", "");
            if (g_acc.acc && !g_acc.ck) { sa_call_scores_destroy(g_acc.acc); g_acc.acc = NULL; }
            for (int q = 0; q <= s; q++) strand_result_free(&c.sr[q], n_jobs);
            s = -1;   /* both strands again, without the offenders */
            continue;
        }
        if (rc != SA_OK) die("signalMachine: alignment failed: %s", sa_strerror(rc));
    }
    g_t_gpu += now_s() - ts1;
    render_slice(&c);
    free(c.bj);
    return slice_close(sl);
}

/* ---- --snp-step N --snp-dir DIR: single-nucleotide probabilities (singleNucleotideProbabilities.py:551-723) ----
 * Every read strand becomes N jobs in one batch: job s aligns the read to its window with X at the contig positions = s (mod N)
 * (replace_periodic_reference_positions; the default ambiguity table makes X the four bases).  sa_batch_position_calls folds
 * the rows of every X position on the device (CallMethylation.call_methyls); the N step files of a read are merged into
 * DIR/<label>.tsv (discover_single_nucleotide_probabilities).  fast5_input names the .npRead: the one deliberate difference.
 * --snp-marginals: every batch is also added to one over-reads table on the device (sa_snp_marginals_add_batch), written at the
 * end of the run; --snp-sites: the same with one copy per read, X at the listed sites only (1-D runs). */
typedef struct {   /* what one strand's batch leaves, [read * N + step] each */
    sa_position_call_t **calls;
    int64_t *n_calls;
    int32_t *x_min, *x_max;
    int64_t *n_pairs, *sum_e7;
} snp_result_t;

static void snp_result_free(snp_result_t *r, int64_t n_jobs) {
    for (int64_t i = 0; i < n_jobs && r->calls; i++) sa_free(r->calls[i]);
    free(r->calls); free(r->n_calls); free(r->x_min); free(r->x_max); free(r->n_pairs); free(r->sum_e7);
    memset(r, 0, sizeof(*r));
}

typedef struct {
    slice_t sl;
    int64_t N, n_slots;   /* n_slots: the reads the slice started with, times N */
    char **tgt[2];        /* the substituted targets: read j, step s, strand q at tgt[q][j * N + s] */
    sa_job_t *jobs[2];
    snp_result_t sr[2];
} snp_slice_t;

/* contig coordinate of index t of a strand's target (the TSV's reference_index of a k-mer at t covers t .. t + k - 1) */
static int snp_contig_pos_is_forward(const read_t *rd, int s) { return (s == 0 && rd->forward) || (s == 1 && !rd->forward); }
static int64_t snp_contig_pos(const read_t *rd, int s, int64_t t) {
    const int64_t off = rd->st[s].r_shift;
    return snp_contig_pos_is_forward(rd, s) ? off + t : off - 1 - t;
}

/* --snp-marginals, --position-profile: which record of the -f reference a read lies on */
static int64_t snp_contig_index(const run_t *R, const read_t *rd) {
    const char *name = rd->seq_name ? rd->seq_name : rd->pA->contig1;
    int64_t ci = 0;
    while (ci < R->snp_n_contigs && strcmp(R->snp_names[ci], name) != 0) ci++;
    if (ci == R->snp_n_contigs) die("signalMachine: %s is no record of the -f reference", name);
    return ci;
}

static void snp_output_one(int64_t j, void *ctx) {
    snp_slice_t *c = ctx;
    const run_t *R = c->sl.R;
    read_t *rd = &c->sl.reads[c->sl.who[j]];
    int64_t cap = 0;
    for (int64_t s = 0; s < c->N; s++)
        for (int q = 0; q < n_strands(R); q++) cap += c->sr[q].n_calls[j * c->N + s];
    sa_snp_site_t *sites = xalloc(cap, sizeof(sa_snp_site_t), 0);
    int64_t n = 0;
    for (int64_t s = 0; s < c->N; s++) {   /* one step file after the other */
        const int64_t js = j * c->N + s;
        /* the window of call_methyls (:160-169) over the reference_index of every row of the step's file, both strands */
        int64_t lo_ref = INT64_MAX, hi_ref = INT64_MIN;
        for (int q = 0; q < n_strands(R); q++) {
            if (c->sr[q].x_min[js] < 0) continue;
            const int k = R->sm[q].k;
            const int64_t len = (int64_t) strlen(rd->st[q].target), off = rd->st[q].r_shift;
            const int64_t a = adjust_ref(c->sr[q].x_min[js], off, len - k, len, q == 0, rd->forward);
            const int64_t b = adjust_ref(c->sr[q].x_max[js], off, len - k, len, q == 0, rd->forward);
            lo_ref = a < lo_ref ? a : lo_ref; lo_ref = b < lo_ref ? b : lo_ref;
            hi_ref = a > hi_ref ? a : hi_ref; hi_ref = b > hi_ref ? b : hi_ref;
        }
        if (lo_ref > hi_ref) continue;   /* no row at all: the reference's step file cannot be parsed and is missing */
        int64_t w_lo = 0, w_hi = 0;
        sa_snp_site_window(lo_ref, hi_ref, c->N, &w_lo, &w_hi);
        for (int q = 0; q < n_strands(R); q++) {   /* template sites, then complement sites, each ascending */
            const sa_position_call_t *pc = c->sr[q].calls[js];
            const int64_t m = c->sr[q].n_calls[js];
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

/* the substituted copies of every read's jobs */
static void snp_build_jobs(snp_slice_t *c) {
    const slice_t *sl = &c->sl;
    const int64_t N = c->N;
    c->n_slots = sl->n_ok * N;
    for (int q = 0; q < n_strands(sl->R); q++) {
        c->tgt[q] = xalloc(c->n_slots, sizeof(char *), 1);
        c->jobs[q] = xalloc(c->n_slots, sizeof(sa_job_t), 1);
    }
    for (int64_t j = 0; j < sl->n_ok; j++) {
        const read_t *rd = &sl->reads[sl->who[j]];
        const int64_t hi = rd->win_lo + (int64_t) strlen(rd->forward_seq) - 1;
        for (int q = 0; q < n_strands(sl->R); q++) {
            const char *t = rd->st[q].target;
            const int from_fwd = t == rd->forward_seq;   /* forward_seq[i] at win_lo + i, backward_seq[i] at hi - i */
            const int64_t len = (int64_t) strlen(t);
            for (int64_t s = 0; s < N; s++) {
                char *o = xalloc(len + 1, 1, 0);
                if (sl->R->snp_sites) {   /* --snp-sites: X at the listed sites of the read's contig */
                    const int64_t ci = snp_contig_index(sl->R, rd);
                    sa_snp_substitute_sites(t, len, from_fwd ? rd->win_lo : hi, !from_fwd, sl->R->snp_sites[ci], sl->R->snp_n_sites[ci], 'X', o);
                } else {
                    sa_snp_substitute(t, len, from_fwd ? rd->win_lo : hi, !from_fwd, N, s, 'X', o);
                }
                c->tgt[q][j * N + s] = o;
                c->jobs[q][j * N + s] = rd->jobs[q];
                c->jobs[q][j * N + s].ref = o;
            }
        }
    }
}

/* The slice closes up after drop_refused_reads: the read now at k was at kept_from[k].  A refused read's targets are freed, a
 * kept read's move down to its new place and leave their old slots empty, so that every target is owned by exactly one slot. */
static void snp_close_up(snp_slice_t *c, int64_t n_before, const int64_t *kept_from) {
    const int64_t N = c->N;
    for (int64_t j = 0, k = 0; j < n_before; j++) {
        const int kept = k < c->sl.n_ok && kept_from[k] == j;
        for (int q = 0; q < n_strands(c->sl.R); q++)
            for (int64_t s = 0; s < N; s++) {
                char **src = &c->tgt[q][j * N + s];
                if (!kept) {
                    free(*src);
                    *src = NULL;
                } else if (k != j) {
                    c->tgt[q][k * N + s] = *src;
                    c->jobs[q][k * N + s] = c->jobs[q][j * N + s];
                    *src = NULL;
                }
            }
        k += kept;
    }
}

/* --snp-marginals: the finished batch of strand q added to the run's table.  Job j * N + s is read j's copy s: where its target
 * lies on the contig (snp_contig_pos), the reference_index of its records (adjust_ref), its direction, the read's place in the
 * manifest as run ordinal, and one window per (read, step) */
static int snp_add_to_marginals(snp_slice_t *c, int q, sa_batch_t *b) {
    const run_t *R = c->sl.R;
    const int64_t N = c->N, nj = c->sl.n_ok * N;
    sa_snp_job_map_t *map = xalloc(nj, sizeof(*map), 1);
    for (int64_t j = 0; j < c->sl.n_ok; j++) {
        const read_t *rd = &c->sl.reads[c->sl.who[j]];
        const int64_t ci = snp_contig_index(R, rd);
        const int same = (q == 0 && rd->forward) || (q == 1 && !rd->forward);
        const int64_t off = rd->st[q].r_shift, run = (int64_t) (rd - (const read_t *) R->reads0);
        for (int64_t s = 0; s < N; s++) {
            sa_snp_job_map_t *m = &map[j * N + s];
            m->contig = (int32_t) ci;
            m->pos_sign = m->x_sign = same ? 1 : -1;
            m->pos0 = same ? off : off - 1;
            m->x0 = same ? off : off - R->sm[q].k;   /* adjust_ref: len_kmers - (x + (len - off)) with len_kmers = len - k */
            m->strand = q;
            m->direction = same;
            m->run = run;
            m->group = run * N + s;
        }
    }
    const int rc = sa_snp_marginals_add_batch(R->snp_tab, b, map, nj, NULL);
    free(map);
    return rc;
}

/* creates, runs and harvests the batch of strand q of a --snp-step slice into c->sr[q] */
static int snp_run_strand_batch(snp_slice_t *c, int q) {
    snp_result_t *r = &c->sr[q];
    const int64_t nj = c->sl.n_ok * c->N;
    r->calls = xalloc(nj, sizeof(sa_position_call_t *), 1);
    r->n_calls = xalloc(nj, sizeof(int64_t), 1);
    r->x_min = xalloc(nj, sizeof(int32_t), 1);
    r->x_max = xalloc(nj, sizeof(int32_t), 1);
    r->n_pairs = xalloc(nj, sizeof(int64_t), 1);
    r->sum_e7 = xalloc(nj, sizeof(int64_t), 1);
    sa_batch_t *b = NULL;
    int rc = create_strand_batch(&b, &c->sl, q, c->jobs[q], nj, c->N, SA_FLAG_POSITION_CALLS);
    if (rc == SA_OK) rc = sa_batch_run(b);
    if (rc == SA_OK && c->sl.R->snp_dir) rc = sa_batch_position_calls(b, 0, r->calls, r->n_calls, r->x_min, r->x_max, NULL);
    if (rc == SA_OK && c->sl.R->snp_tab) rc = snp_add_to_marginals(c, q, b);
    for (int64_t i = 0; i < nj && rc == SA_OK; i++) rc = sa_batch_all_pairs_summary(b, i, &r->n_pairs[i], &r->sum_e7[i]);
    sa_batch_destroy(b);
    return rc;
}

/* --snp-step mode: GPU stage and outputs of a slice */
static int64_t run_slice_snp(run_t *R, read_t *reads, int64_t n_reads, int device) {
    snp_slice_t c;
    memset(&c, 0, sizeof(c));
    slice_t *sl = &c.sl;
    const int64_t N = c.N = R->snp_step > 0 ? R->snp_step : 1;   /* (--snp-sites: one copy per read) */
    const double ts1 = now_s();
    slice_open(sl, R, reads, n_reads, device);
    snp_build_jobs(&c);
    int64_t *kept_from = xalloc(sl->n_ok, sizeof(int64_t), 0);
    /* --snp-marginals: the table is checkpointed here, so that the retry below takes the slice's rows out again */
    if (R->snp_tab && sa_snp_marginals_checkpoint(R->snp_tab) != SA_OK) die("signalMachine: --snp-marginals: checkpoint failed%s", "");
    for (int q = 0; q < n_strands(R) && sl->n_ok > 0; q++) {
        fprintf(stderr, "signalAlign - starting %s alignment\n", strand_name(q));
        const int64_t n_before = sl->n_ok;
        const int rc = snp_run_strand_batch(&c, q);
        if (drop_refused_reads(sl, rc, c.jobs, N, kept_from)) {
            if (R->snp_tab && sa_snp_marginals_rollback(R->snp_tab) != SA_OK) die("signalMachine: --snp-marginals: rollback failed%s", "");
            snp_close_up(&c, n_before, kept_from);
            for (int q2 = 0; q2 <= q; q2++) snp_result_free(&c.sr[q2], n_before * N);
            q = -1;   /* both strands again, without the offenders */
            continue;
        }
        if (rc != SA_OK) die("signalMachine: alignment failed: %s", sa_strerror(rc));
    }
    free(kept_from);
    g_t_gpu += now_s() - ts1;
    const double ts2 = now_s();
    if (R->snp_dir) parallel_for(sl->n_ok, snp_output_one, &c);
    /* the summary lines of the N -s 0 runs of every read, step after step */
    for (int64_t j = 0; j < sl->n_ok; j++)
        for (int64_t s = 0; s < N; s++) {
            const int64_t js = j * N + s;
            int64_t n[2] = {0, 0};
            double score[2] = {0.0, 0.0};
            for (int q = 0; q < n_strands(R); q++) {
                n[q] = c.sr[q].n_pairs[js];
                score[q] = 100.0 * (double) c.sr[q].sum_e7[js] / ((double) n[q] * PROB_1);
            }
            report_read(R, &reads[sl->who[j]], n, score);
        }
    t_add(&g_t_render, now_s() - ts2);
    for (int q = 0; q < n_strands(R); q++) {
        snp_result_free(&c.sr[q], sl->n_ok * N);
        for (int64_t i = 0; i < c.n_slots; i++) free(c.tgt[q][i]);
        free(c.tgt[q]); free(c.jobs[q]);
    }
    return slice_close(sl);
}

static int cmp_i64(const void *a, const void *b) {
    const int64_t x = *(const int64_t *) a, y = *(const int64_t *) b;
    return x < y ? -1 : x > y;
}

/* --snp-sites: lines "contig<TAB>site[<TAB>...]" (a --snp-proposals file among them) into ascending lists per record */
static void load_snp_sites(run_t *R) {
    FILE *fh = fopen(R->snp_sites_path, "r");
    if (!fh) die("signalMachine: cannot read %s", R->snp_sites_path);
    R->snp_sites = xalloc(R->snp_n_contigs, sizeof(int64_t *), 1);
    R->snp_n_sites = xalloc(R->snp_n_contigs, sizeof(int64_t), 1);
    char line[4096], name[2048];
    while (fgets(line, sizeof line, fh)) {
        int64_t site = 0;
        if (line[0] == '\n' || line[0] == '#') continue;
        if (sscanf(line, "%2047[^\t]\t%" SCNd64, name, &site) != 2) die("signalMachine: --snp-sites: cannot parse a line of %s", R->snp_sites_path);
        int64_t ci = 0;
        while (ci < R->snp_n_contigs && strcmp(R->snp_names[ci], name) != 0) ci++;
        if (ci == R->snp_n_contigs || site < 0 || site >= R->snp_lens[ci]) die("signalMachine: --snp-sites: a site of %s is not in the -f reference", name);
        R->snp_sites[ci] = realloc(R->snp_sites[ci], sizeof(int64_t) * (size_t) (R->snp_n_sites[ci] + 1));
        if (!R->snp_sites[ci]) die("signalMachine: out of memory%s", "");
        R->snp_sites[ci][R->snp_n_sites[ci]++] = site;
    }
    fclose(fh);
    for (int64_t c = 0; c < R->snp_n_contigs; c++)
        if (R->snp_n_sites[c]) qsort(R->snp_sites[c], (size_t) R->snp_n_sites[c], sizeof(int64_t), cmp_i64);
}

/* --snp-reference-out: every record of -f with the calls applied, lines as wide as the input's first sequence line */
static void write_snp_reference(const run_t *R, const sa_snp_marginal_t *m, int64_t n) {
    int64_t width = 60;
    FILE *in = fopen(R->fwd_ref, "r");
    if (in) {
        char *buf = NULL;
        size_t cap = 0;
        ssize_t got;
        while ((got = getline(&buf, &cap, in)) >= 0)
            if (got > 0 && buf[0] != '>') {
                while (got > 0 && (buf[got - 1] == '\n' || buf[got - 1] == '\r')) got--;
                if (got > 0) width = (int64_t) got;
                break;
            }
        free(buf);
        fclose(in);
    }
    FILE *fh = fopen(R->snp_ref_out, "w");
    if (!fh) die("signalMachine: cannot write %s", R->snp_ref_out);
    for (int64_t c = 0; c < R->snp_n_contigs; c++) {
        char *out = xalloc(R->snp_lens[c] + 1, 1, 0);
        if (sa_snp_apply_calls(R->snp_seqs[c], R->snp_lens[c], m, n, (int32_t) c, out) != SA_OK) die("signalMachine: --snp-reference-out failed%s", "");
        fprintf(fh, ">%s\n", R->snp_names[c]);
        for (int64_t i = 0; i < R->snp_lens[c]; i += width)
            fprintf(fh, "%.*s\n", (int) (R->snp_lens[c] - i < width ? R->snp_lens[c] - i : width), out + i);
        free(out);
    }
    if (fclose(fh) != 0) die("signalMachine: cannot write %s", R->snp_ref_out);
}

/* --snp-marginals / --snp-proposals at the end of the run: finish on the device, the table, the thinned proposals per contig */
static void write_snp_marginals(run_t *R) {
    if (!R->snp_tab) return;
    sa_snp_marginal_t *m = NULL;
    int64_t n = 0;
    if (sa_snp_marginals_finish(R->snp_tab, 1, (const char *const *) R->snp_seqs, &m, &n, NULL) != SA_OK)
        die("signalMachine: --snp-marginals: the final step failed%s", "");
    if (sa_snp_write_marginals(R->snp_marg, (const char *const *) R->snp_names, m, n) != SA_OK) die("signalMachine: cannot write %s", R->snp_marg);
    if (R->snp_prop) {
        FILE *fh = fopen(R->snp_prop, "w");
        if (!fh) die("signalMachine: cannot write %s", R->snp_prop);
        int64_t *pos = xalloc(n, sizeof(int64_t), 0), *keep = xalloc(n, sizeof(int64_t), 0);
        double *delta = xalloc(n, sizeof(double), 0);
        for (int64_t a = 0; a < n;) {   /* the sites come in (contig, position) order: one contig after the other */
            int64_t e = a, np = 0, nk = 0;
            for (; e < n && m[e].contig == m[a].contig; e++)
                if (m[e].is_proposal) { pos[np] = m[e].pos; delta[np] = m[e].delta; np++; }
            if (sa_snp_group_sites(pos, delta, np, 6, 1, keep, &nk) != SA_OK) die("signalMachine: --snp-proposals failed%s", "");
            for (int64_t i = 0, j = 0; i < nk; i++) {   /* keep[] ascends, and so does pos[] */
                while (pos[j] != keep[i]) j++;
                char num[40];
                sa_format_py_repr(num, delta[j]);
                fprintf(fh, "%s\t%" PRId64 "\t%s\n", R->snp_names[m[a].contig], keep[i], num);
            }
            a = e;
        }
        free(pos); free(keep); free(delta);
        if (fclose(fh) != 0) die("signalMachine: cannot write %s", R->snp_prop);
    }
    if (R->snp_ref_out) write_snp_reference(R, m, n);
    sa_free(m);
    sa_snp_marginals_destroy(R->snp_tab);
    R->snp_tab = NULL;
}

/* --position-profile at the end of the run: finish on the device, the script's file */
static void write_position_profile(run_t *R) {
    if (!R->prof_tab) return;
    sa_profile_site_t *sites = NULL;
    int64_t n = 0;
    uint32_t seen = 0;
    if (sa_position_profile_finish(R->prof_tab, (const char *const *) R->snp_seqs, &sites, &n, &seen, NULL) != SA_OK)
        die("signalMachine: --position-profile: the final step failed%s", "");
    if (sa_position_profile_write(R->prof_path, R->sm[0].alphabet, seen, (const char *const *) R->snp_names, sites, n) != SA_OK)
        die("signalMachine: cannot write %s", R->prof_path);
    sa_free(sites);
    sa_position_profile_destroy(R->prof_tab);
    R->prof_tab = NULL;
}

int main(int argc, char **argv) {
    run_t R;
    memset(&R, 0, sizeof(R));
    R.dev_params = (sa_deviation_params_t) {10, 5, 64};
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
         *post_path2 = NULL, *seq_name = NULL, *ambig_model = NULL, *manifest = NULL, *guide_window = NULL;
    int guide_locate = 0, acc_opts = 0;
    R.guide_band = 128;
    R.acc_bins = 1000;
    R.acc_threshold = 0.500000001;
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
                                           {"site-calls-accuracy", required_argument, 0, 1070},
                                           {"site-calls-accuracy-curves", required_argument, 0, 1071},
                                           {"site-calls-accuracy-bins", required_argument, 0, 1072},
                                           {"site-calls-accuracy-threshold", required_argument, 0, 1073},
                                           {"site-calls-truth", required_argument, 0, 1074},
                                           {"site-calls-truth-reads", required_argument, 0, 1075},
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
                                           {"train-mixture-motifs", required_argument, 0, 1040},
                                           {"train-mixture-template-model", required_argument, 0, 1041},
                                           {"train-mixture-complement-model", required_argument, 0, 1042},
                                           {"train-mixture-distances", required_argument, 0, 1043},
                                           {"snp-step", required_argument, 0, 1020},
                                           {"snp-dir", required_argument, 0, 1021},
                                           {"snp-marginals", required_argument, 0, 1022},
                                           {"snp-proposals", required_argument, 0, 1023},
                                           {"snp-sites", required_argument, 0, 1024},
                                           {"snp-reference-out", required_argument, 0, 1025},
                                           {"position-profile", required_argument, 0, 1026},
                                           {"guide-deviation", required_argument, 0, 1060},
                                           {"guide-deviation-threshold", required_argument, 0, 1061},
                                           {"guide-deviation-events", required_argument, 0, 1062},
                                           {"guide-window", required_argument, 0, 1050},
                                           {"guide-locate", no_argument, 0, 1053},
                                           {"guide-band", required_argument, 0, 1051},
                                           {"guide-cigars-out", required_argument, 0, 1052},
                                           {"npread-out", required_argument, 0, 1080},
                                           {"raw-detector", required_argument, 0, 1081},
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
            case 1070: R.acc_path = strdup(optarg); break;
            case 1071: R.acc_curves_path = strdup(optarg); break;
            case 1072: R.acc_bins = atoi(optarg); acc_opts = 1; break;
            case 1073: R.acc_threshold = atof(optarg); acc_opts = 1; break;
            case 1074: R.acc_truth_path = strdup(optarg); break;
            case 1075: R.acc_reads_path = strdup(optarg); break;
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
            case 1040: R.mix_motifs = strdup(optarg); break;
            case 1041: R.mix_model[0] = strdup(optarg); break;
            case 1042: R.mix_model[1] = strdup(optarg); break;
            case 1043: R.mix_dist = strdup(optarg); break;
            case 1020:
                snp_set = 1;
                if (sscanf(optarg, "%" SCNd64, &R.snp_step) != 1) R.snp_step = 0;
                break;
            case 1021: R.snp_dir = strdup(optarg); break;
            case 1022: R.snp_marg = strdup(optarg); break;
            case 1023: R.snp_prop = strdup(optarg); break;
            case 1024: R.snp_sites_path = strdup(optarg); break;
            case 1025: R.snp_ref_out = strdup(optarg); break;
            case 1026: R.prof_path = strdup(optarg); break;
            case 1060: R.dev_path = strdup(optarg); break;
            case 1061: R.dev_params.threshold = atoi(optarg); break;
            case 1062: R.dev_events_path = strdup(optarg); break;
            case 1050: guide_window = strdup(optarg); break;
            case 1051: R.guide_band = atoi(optarg); break;
            case 1053: guide_locate = 1; break;
            case 1052: R.guide_cigars_out = strdup(optarg); break;
            case 1080: R.npread_out = strdup(optarg); break;
            case 1081: {
                sa_detector_params_t *d = &R.raw_detector;
                char tail = 0;
                if (sscanf(optarg, "%d,%d,%f,%f,%f%c", &d->window_length1, &d->window_length2, &d->threshold1, &d->threshold2, &d->peak_height,
                           &tail) != 5 || d->window_length1 < 1 || d->window_length2 < 1)
                    die("signalMachine: --raw-detector takes w1,w2,t1,t2,peak with window lengths >= 1, not %s", optarg);
                R.raw_detector_set = 1;
                break;
            }
            case 1003: batch_reads = atoll(optarg) > 0 ? atoll(optarg) : batch_reads; break;
            case 1004:
                if (!strcmp(optarg, "twoDist")) R.two_dist = 1;
                else if (strcmp(optarg, "meanOnly")) die("signalMachine: --emission takes meanOnly or twoDist, not %s", optarg);
                break;
            default: usage(); return 1;
        }
    }
    if (!label) label = strdup("");
    if (R.prof_path && manifest == NULL) { usage(); die("signalMachine: --position-profile needs --batch <manifest>%s", ""); }
    if (t_model == NULL || (c_model == NULL && R.two_d)) die("Missing model files, exiting", NULL);
    if (R.out_fmt == 3 && post_path2 == NULL && manifest == NULL) die("Must pass in posteriorProbsFile2 if using 'both' outFmt", NULL);
    if (cigar_path != NULL && guide_window != NULL) die("signalMachine: -p and --guide-window exclude each other%s", "");
    if (guide_locate && (cigar_path != NULL || guide_window != NULL)) die("signalMachine: --guide-locate excludes -p and --guide-window%s", "");
    if (guide_locate && manifest != NULL) die("signalMachine: --guide-locate is for a single read; in a manifest write @ in the cigar column%s", "");
    if (cigar_path == NULL && guide_window == NULL && !guide_locate && manifest == NULL)
        die("[signalMachine]ERROR: Need to provide input guide alignments, exiting", NULL);
    if (R.guide_band < 64 || R.guide_band > 256 || R.guide_band % 64 != 0) die("signalMachine: --guide-band takes 64, 128, 192 or 256%s", "");
    R.device = device;
    R.fwd_ref = fwd_ref;
    R.bwd_ref = bwd_ref;

    /* the reads of this run */
    read_t *reads = NULL;
    int64_t n_reads = 0;
    R.batch_mode = manifest != NULL;
    if (R.batch_mode) {
        n_reads = load_manifest(manifest, &reads);
        if (n_reads < 0) die("[signalMachine]ERROR: cannot read the batch manifest %s", manifest);
        for (int64_t i = 0; i < n_reads; i++) {
            if (reads[i].seq_name == NULL && seq_name != NULL) reads[i].seq_name = strdup(seq_name);
            if (reads[i].expect[0] != NULL || reads[i].expect[1] != NULL) R.expect_mode = 1;
        }
        if (R.expect_mode)
            for (int64_t i = 0; i < n_reads; i++)
                if (reads[i].expect[0] == NULL && reads[i].expect[1] == NULL)
                    die("[signalMachine]ERROR: batch manifest mixes expectation and alignment reads (%s)", reads[i].label);
    } else {
        reads = calloc(1, sizeof(read_t));
        n_reads = 1;
        reads[0].label = label; reads[0].npread_path = npread_path; reads[0].cigar_path = cigar_path;
        reads[0].post_path = post_path; reads[0].post_path2 = post_path2; reads[0].seq_name = seq_name;
        reads[0].expect[0] = t_expect; reads[0].expect[1] = c_expect;
        reads[0].guide_window = guide_window;
        reads[0].guide_locate = guide_locate;
        R.expect_mode = t_expect != NULL || c_expect != NULL;
        if (guide_window != NULL || guide_locate) {
            if (fwd_ref == NULL) die(guide_locate ? "[signalMachine] ERROR: --guide-locate needs -f <fasta>" : "[signalMachine] ERROR: --guide-window needs -f <fasta>", NULL);
        } else if (fwd_ref == NULL || seq_name == NULL) {
            /* the reference needs -n; kept after the cigar check so that the error order matches (impl/signalMachine.c:642-663) */
            sa_cigar_t *probe = NULL;
            if (sa_cigar_load(cigar_path, &probe) != SA_OK)
                die("[signalMachine]ERROR: Didn't find input alignment file, looked %s", cigar_path);
            sa_cigar_free(probe);
            die("[signalMachine] ERROR: need -f <fasta> and -n <sequence name>", NULL);
        }
    }
    for (int64_t i = 0; i < n_reads; i++) {   /* guide windows: refused before anything runs */
        if (reads[i].guide_locate && R.rna) die("signalMachine: --guide-locate (@ in a manifest) cannot be combined with --rna: RNA reads need a cigar file%s", "");
        if (reads[i].guide_window == NULL) continue;
        if (R.rna) die("signalMachine: a guide window (%s) cannot be combined with --rna: RNA reads need a cigar file", reads[i].guide_window);
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
        if (R.two_d || c_model != NULL) die("signalMachine: a raw read (%s) is a 1D read: not with --twoD or a complement model", reads[i].npread_path);
        if (R.rna) die("signalMachine: a raw read (%s) cannot be combined with --rna: RNA reads need a .npRead", reads[i].npread_path);
        if (R.hdp || t_hdp != NULL) die("signalMachine: a raw read (%s) needs a Gaussian template model for its event alignment: not with an .nhdp", reads[i].npread_path);
    }
    if (R.npread_out && mkdir(R.npread_out, 0777) != 0 && errno != EEXIST) die("signalMachine: cannot create %s", R.npread_out);
    if (R.guide_cigars_out && mkdir(R.guide_cigars_out, 0777) != 0 && errno != EEXIST) die("signalMachine: cannot create %s", R.guide_cigars_out);
    /* (the expectation pass keeps the reference-ordered kernels and the model's own noise; an HDP model has no such emission) */
    if (R.two_dist && (R.hdp || t_hdp != NULL || c_hdp != NULL || R.expect_mode || t_expect != NULL || c_expect != NULL))
        die("signalMachine: --emission twoDist aligns reads with a Gaussian model: not with an .nhdp, not with -t / -c%s", "");

    const int mix_out = R.mix_model[0] || R.mix_model[1] || R.mix_dist;
    if ((R.mix_motifs != NULL) != (mix_out != 0)) {
        usage();
        die("signalMachine: --train-mixture-motifs goes with --train-mixture-template-model / -complement-model / -distances%s", "");
    }
    R.want_train = R.train_assign || R.train_model[0] || R.train_model[1] || R.mix_motifs;
    if (R.want_train) {
        if (R.expect_mode || R.mea) die("signalMachine: --train-* needs the alignment mode without --mea%s", "");
        if ((R.train_model[1] || R.mix_model[1]) && !R.two_d) die("signalMachine: --train-complement-model needs a 2-D run%s", "");
        if (R.train_n < 1 || !(R.train_min_prob >= 0 && R.train_min_prob <= 1)) die("signalMachine: bad --train-max-assignments / --train-min-prob%s", "");
    }
    if (!R.acc_path && (R.acc_curves_path || R.acc_truth_path || R.acc_reads_path || acc_opts)) {
        usage();
        die("signalMachine: --site-calls-truth* and --site-calls-accuracy-* need --site-calls-accuracy <file>%s", "");
    }
    if (R.acc_path && !R.acc_truth_path && !R.acc_reads_path) { usage(); die("signalMachine: --site-calls-accuracy needs --site-calls-truth <file> or --site-calls-truth-reads <file>%s", ""); }
    if (R.acc_path && (R.acc_bins < 1 || R.acc_threshold != R.acc_threshold)) { usage(); die("signalMachine: --site-calls-accuracy-bins takes n >= 1, --site-calls-accuracy-threshold a number%s", ""); }
    if (R.acc_path && R.two_d && (R.mea || R.dev_path)) { usage(); die("signalMachine: --site-calls-accuracy on a --twoD run cannot be combined with --mea / --guide-deviation%s", ""); }
    R.want_agg = R.agg_path != NULL || R.acc_path != NULL;
    if (R.expect_mode && (R.site_calls || R.want_agg)) { usage(); die("signalMachine: --site-calls / --site-calls-aggregate / --site-calls-accuracy need the alignment mode, not -t/-c%s", ""); }
    if (R.snp_prop && !R.snp_marg) { usage(); die("signalMachine: --snp-proposals needs --snp-marginals <file>%s", ""); }
    if (R.snp_sites_path && snp_set) { usage(); die("signalMachine: --snp-sites cannot be combined with --snp-step%s", ""); }
    if (R.snp_ref_out && !R.snp_sites_path) { usage(); die("signalMachine: --snp-reference-out needs --snp-sites <file>%s", ""); }
    if (R.snp_sites_path && !R.snp_marg) { usage(); die("signalMachine: --snp-sites needs --snp-marginals <file>%s", ""); }
    if (R.snp_sites_path && R.snp_dir) { usage(); die("signalMachine: --snp-sites writes no per-read files: --snp-dir not allowed%s", ""); }
    if (R.snp_marg && !snp_set && !R.snp_sites_path) { usage(); die("signalMachine: --snp-marginals needs --snp-step <N> or --snp-sites <file>%s", ""); }
    if (R.prof_path) {   /* --position-profile: 1-D DNA runs of a manifest that keep every row and every path k-mer */
        if (R.two_d) { usage(); die("signalMachine: --position-profile does not take --twoD runs%s", ""); }
        if (R.rna) { usage(); die("signalMachine: --position-profile does not take --rna runs%s", ""); }
        if (R.out_fmt == 1) { usage(); die("signalMachine: --position-profile cannot be combined with -s 1 (it drops rows)%s", ""); }
        if (snp_set || R.snp_sites_path) { usage(); die("signalMachine: --position-profile cannot be combined with --snp-step / --snp-sites%s", ""); }
        if (R.expect_mode) { usage(); die("signalMachine: --position-profile needs the alignment mode, not -t/-c%s", ""); }
        if (fwd_ref == NULL) { usage(); die("signalMachine: --position-profile needs -f <fasta>%s", ""); }
    }
    if (R.dev_events_path && !R.dev_path) { usage(); die("signalMachine: --guide-deviation-events needs --guide-deviation <file>%s", ""); }
    if (R.dev_path) {   /* --guide-deviation: alignment runs that keep every row */
        if (R.dev_params.threshold < 0) { usage(); die("signalMachine: --guide-deviation-threshold takes n >= 0%s", ""); }
        if (R.expect_mode) { usage(); die("signalMachine: --guide-deviation needs the alignment mode, not -t/-c%s", ""); }
        if (R.want_train) { usage(); die("signalMachine: --guide-deviation cannot be combined with --train-*%s", ""); }
        if (snp_set || R.snp_dir || R.snp_sites_path) { usage(); die("signalMachine: --guide-deviation cannot be combined with --snp-step / --snp-sites%s", ""); }
    }
    if (snp_set || R.snp_dir || R.snp_sites_path) {   /* --snp-step / --snp-sites: their own outputs only */
        const char *opt = R.snp_sites_path ? "--snp-sites" : "--snp-step";
        if (!R.snp_sites_path && (!snp_set || R.snp_step < 1)) { usage(); die("signalMachine: --snp-step takes a step N >= 1%s", ""); }
        if (!R.snp_dir && !R.snp_marg) { usage(); die("signalMachine: --snp-step needs --snp-dir <directory>%s", ""); }
        if (R.snp_marg && R.two_d) { usage(); die("signalMachine: --snp-marginals does not take --twoD runs%s", ""); }
        if (R.expect_mode) { usage(); die("signalMachine: %s cannot be combined with -t/-c", opt); }
        if (R.mea) { usage(); die("signalMachine: %s cannot be combined with --mea", opt); }
        if (R.site_calls || R.want_agg) { usage(); die("signalMachine: %s cannot be combined with --site-calls / --site-calls-aggregate / --site-calls-accuracy", opt); }
        if (R.want_train) { usage(); die("signalMachine: %s cannot be combined with --train-*", opt); }
        for (int64_t i = 0; i < n_reads; i++)
            if (reads[i].post_path || reads[i].post_path2) {
                usage();
                if (R.snp_sites_path) die("signalMachine: --snp-sites writes no posteriors file: no -u / -i, a manifest's posteriors column '-'%s", "");
                die(R.batch_mode ? "signalMachine: --snp-step writes no posteriors file: the manifest's posteriors column of %s must be '-'"
                                 : "signalMachine: --snp-step writes no posteriors file: -u / -i not allowed%s", R.batch_mode ? reads[i].label : "");
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

    if (load_strand_model(&R.sm[0], t_model, R.hdp ? t_hdp : NULL) != SA_OK)
        die("signalAlign - ERROR: couldn't find model file here: %s", t_model);
    if (R.two_d && load_strand_model(&R.sm[1], c_model, R.hdp ? c_hdp : NULL) != SA_OK)
        die("signalAlign - ERROR: couldn't find model file here: %s", c_model);
    for (int s = 0; s < n_strands(&R) && R.two_dist && R.batch_mode; s++) {   /* the base of the slices' noise-scaled batches */
        strand_model_t *sm = &R.sm[s];
        if (sa_model_clone_with_table(&sm->model_two, sm->model, sm->table_orig) != SA_OK ||
            sa_model_set_emission(sm->model_two, SA_EMISSION_TWO_DIST) != SA_OK)
            die("signalMachine: --emission twoDist: could not set up the two-distribution model%s", "");
    }
    if (R.mix_motifs) {   /* parsed once here, so that a bad list stops the run before it starts */
        mix_pair_t *probe = NULL;
        for (int s = 0; s < n_strands(&R); s++) {
            mixture_pairs(&R, s, &probe);
            free(probe);
        }
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
        for (int s = 0; s < n_strands(&R); s++) set_hdp_expected(&R.sm[s]);
    }
    /* the reads go through in slices of --batch-reads (default 2048): bounded host and device memory for any manifest */
    /* Two slices are in the air: while the GPU stage and the rendering of slice k run here, a second thread does the host side
     * of slice k+1 (10 000 short reads: host stage 0.39 s, GPU 0.28 s, rendering 0.25 s, one after the other before).  Rendering
     * stays on this thread, slice after slice, so the summary lines stay in read order: the front door is bound by host CPU
     * time -- text parsing and TSV rendering -- not by the order of its stages. */
    int64_t n_failed = 0;
    if (R.snp_step > 0) {   /* a slice holds at most --batch-reads jobs: N per read and strand */
        batch_reads /= R.snp_step;
        if (batch_reads < 1) batch_reads = 1;
        if (R.snp_dir && mkdir(R.snp_dir, 0777) != 0 && errno != EEXIST) die("signalMachine: cannot create %s", R.snp_dir);
    }
    if (R.snp_marg) {   /* the table lies over every record of the -f reference */
        if (sa_fasta_read_all(R.fwd_ref, &R.snp_names, &R.snp_seqs, &R.snp_lens, &R.snp_n_contigs) != SA_OK)
            die("signalMachine: --snp-marginals: cannot read %s", R.fwd_ref);
        const int rc = sa_snp_marginals_create(&R.snp_tab, R.snp_lens, R.snp_n_contigs, R.snp_step, device);
        if (rc != SA_OK) die("signalMachine: --snp-marginals: %s", sa_strerror(rc));
        R.reads0 = reads;
        if (R.snp_sites_path) load_snp_sites(&R);
    }
    if (R.prof_path) {   /* the table lies over every record of the -f reference */
        if (sa_fasta_read_all(R.fwd_ref, &R.snp_names, &R.snp_seqs, &R.snp_lens, &R.snp_n_contigs) != SA_OK)
            die("signalMachine: --position-profile: cannot read %s", R.fwd_ref);
        const int rc = sa_position_profile_create(&R.prof_tab, R.sm[0].model, R.snp_lens, R.snp_n_contigs, device);
        if (rc != SA_OK) die("signalMachine: --position-profile: %s", sa_strerror(rc));
    }
    if (R.acc_path) {
        g_acc.device = device;
        acc_load(&R);
    }
    if (R.dev_path) {
        if (!(R.dev_fh = fopen(R.dev_path, "w"))) die("signalMachine: cannot open output %s", R.dev_path);
        fprintf(R.dev_fh, "#guide-deviation threshold=%d bucket_size=%d n_buckets=%d; R label strand status n_aligned n_flagged n_on_mea mean_abs "
                          "max_abs max_abs_mea max_event n_sets; H label strand counts; S label strand first_event last_event count peak "
                          "mea_peak center_event open_end; T counts\n", R.dev_params.threshold, R.dev_params.bucket_size, R.dev_params.n_buckets);
        if (R.dev_events_path) {
            if (!(R.dev_events_fh = fopen(R.dev_events_path, "w"))) die("signalMachine: cannot open output %s", R.dev_events_path);
            fprintf(R.dev_events_fh, "#label\tstrand\tevent_index\treference_index\tguide_reference_index\tdiff\ton_mea\tflagged\n");
        }
    }
    int64_t (*const run_slice)(run_t *, read_t *, int64_t, int) = R.expect_mode ? run_slice_expect : (R.snp_step > 0 || R.snp_sites_path) ? run_slice_snp : run_slice_align;
    slice_t cur = {.R = &R, .reads = reads, .n_reads = n_reads < batch_reads ? n_reads : batch_reads}, nxt;
    slice_prepare(&cur);
    for (int64_t off = 0; off < n_reads; off += batch_reads) {
        const int64_t n = n_reads - off < batch_reads ? n_reads - off : batch_reads;
        pthread_t th;
        int started = 0;
        if (off + n < n_reads) {
            const int64_t n2 = n_reads - off - n < batch_reads ? n_reads - off - n : batch_reads;
            nxt = (slice_t) {.R = &R, .reads = reads + off + n, .n_reads = n2};
            started = pthread_create(&th, NULL, slice_prepare, &nxt) == 0;
            if (!started) slice_prepare(&nxt);
        }
        n_failed += run_slice(&R, reads + off, n, device);
        if (started) pthread_join(th, NULL);
    }
    if (R.agg_path) write_aggregate(R.agg_path);
    write_accuracy(&R);
    write_training(&R, t_model, c_model, device);
    write_snp_marginals(&R);
    write_position_profile(&R);
    if (R.dev_fh) {   /* --guide-deviation: the histogram summed over the reads written */
        fprintf(R.dev_fh, "T");
        for (int q = 0; q < R.dev_params.n_buckets; q++) fprintf(R.dev_fh, "\t%" PRId64, R.dev_total[q]);
        fputc('\n', R.dev_fh);
        if (fclose(R.dev_fh) != 0 || (R.dev_events_fh && fclose(R.dev_events_fh) != 0)) die("signalMachine: cannot write %s", R.dev_path);
    }
    if (R.batch_mode)
        fprintf(stderr, "[signalMachine] batch: %" PRId64 " of %" PRId64 " reads aligned\n", n_reads - n_failed, n_reads);
    if (getenv("SA_CLI_TIMING"))
        fprintf(stderr, "[signalMachine] timing: host stage %.3f s wall (thread-seconds: npRead+cigar parse %.3f, reference fetch "
                        "%.3f, parameter estimation+anchors %.3f), GPU stage %.3f s wall, render+write %.3f s wall\n",
                g_t_prep, g_ts_parse, g_ts_fetch, g_ts_estimate, g_t_gpu, g_t_render);
    sa_ref_index_destroy(g_ref_index);
    return n_failed == 0 ? 0 : 1;
}
