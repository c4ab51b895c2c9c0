/* compareDistributions -- drop-in for the reference's executable of the same name (impl/compareDistributions.c): dumps the
 * density of every k-mer of a NanoporeHDP (.nhdp) on linspace(30, 90, 600) into <dir>/x_vals.txt and <dir>/<kmer>_distr.txt, which
 * visualization/compare_trained_models.py reads.  Argument order, the usage line, the two notices and the file formats follow the
 * reference; the densities are the library's (sa_hdp_state_densities: dir_proc_density on the GPU, k-mers in chunks).
 *
 * Beside the reference's two arguments: --kmers FILE (dump only the k-mers listed there, one per line), --distances
 * kl|hellinger|l2|shannonJensen --out FILE (kmer_i <tab> kmer_j <tab> distance for every pair i > j of the listed k-mers, or of all
 * k-mers: get_kmer_distr_distance, impl/nanopore_hdp.c:431-434, through sa_hdp_state_distance_pairs) and --device <n>.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "signalalign_hip.h"

#define GRID_START 30.0
#define GRID_STOP 90.0
#define GRID_LENGTH 600
#define KMER_CHUNK 1024
#define PAIR_CHUNK (1 << 20)

static void die(const char *what, const char *detail) {
    fprintf(stderr, "[compareDistributions] ERROR: %s%s%s\n", what, detail ? ": " : "", detail ? detail : "");
    exit(1);
}

static void usage(void) {
    fprintf(stderr, "USAGE_NEW: compareDistributions [NanoporeHDP_file] [distribution_directory]\n");
    exit(EXIT_FAILURE);
}

static void *must(void *p) {
    if (!p) die("out of memory", NULL);
    return p;
}

static FILE *open_in_dir(const char *dir, const char *name, const char *suffix) {
    const size_t len = strlen(dir) + strlen(name) + strlen(suffix) + 2;
    char *path = must(malloc(len));
    snprintf(path, len, "%s/%s%s", dir, name, suffix);
    FILE *f = fopen(path, "w");
    if (!f) die("cannot write", path);
    free(path);
    return f;
}

typedef struct {
    sa_hdp_state_t *s;
    int metric, device;
    const char *kmers;
    int64_t stride, n, *dp_i, *dp_j, *i, *j;
    double *d;
    FILE *f;
} pair_writer_t;

static void flush_pairs(pair_writer_t *w) {
    if (w->n < 1) return;
    const int rc = sa_hdp_state_distance_pairs(w->s, w->metric, w->dp_i, w->dp_j, w->n, w->device, w->d);
    if (rc != SA_OK) die("cannot evaluate the distances", sa_strerror(rc));
    for (int64_t q = 0; q < w->n; q++)
        fprintf(w->f, "%s\t%s\t%.17g\n", w->kmers + w->i[q] * w->stride, w->kmers + w->j[q] * w->stride, w->d[q]);
    w->n = 0;
}

int main(int argc, char *argv[]) {
    const char *positional[2] = {NULL, NULL}, *kmer_file = NULL, *metric_name = NULL, *out_file = NULL;
    int n_positional = 0, device = 0;
    for (int i = 1; i < argc; i++) {
        const char **value = NULL;
        if (strcmp(argv[i], "--kmers") == 0) value = &kmer_file;
        else if (strcmp(argv[i], "--distances") == 0) value = &metric_name;
        else if (strcmp(argv[i], "--out") == 0) value = &out_file;
        if (value || strcmp(argv[i], "--device") == 0) {
            if (i + 1 >= argc) usage();
            if (value) *value = argv[++i];
            else device = atoi(argv[++i]);
        } else {
            if (n_positional < 2) positional[n_positional] = argv[i];
            n_positional++;
        }
    }
    if (n_positional != 2) usage();
    int metric = -1;
    if (metric_name) {
        static const char *const names[4] = {"kl", "hellinger", "l2", "shannonJensen"};   /* SA_HDP_METRIC_* */
        for (int m = 0; m < 4; m++)
            if (strcmp(metric_name, names[m]) == 0) metric = m;
        if (metric < 0) die("--distances takes kl, hellinger, l2 or shannonJensen, not", metric_name);
        if (!out_file) die("--distances needs --out FILE", NULL);
    } else if (out_file) {
        die("--out needs --distances", NULL);
    }

    const char *model_file = positional[0], *dir = positional[1];
    fprintf(stderr, "[compareDistributions] NOTICE: Loading NanoporeHDP from %s\n", model_file);
    fprintf(stderr, "[compareDistributions] NOTICE: Putting distributions in %s\n", dir);
    sa_hdp_state_t *s = NULL;
    if (sa_hdp_state_load(&s, model_file) != SA_OK) die("cannot read the NanoporeHDP", model_file);
    sa_hdp_state_info_t info;
    char alphabet[64];
    if (sa_hdp_state_info(s, &info) != SA_OK || sa_hdp_state_alphabet(s, alphabet) != SA_OK || info.alphabet_size < 1 || info.kmer_length < 1)
        die("not a NanoporeHDP", model_file);
    if (!info.splines_finalized) die("Must finalize distributions before querying densities", model_file);
    const int64_t k = info.kmer_length;

    /* the k-mers to dump: the listed ones, or all of the alphabet in k-mer index order */
    int64_t n_kmers = 0;
    char *kmers = NULL;   /* k + 1 bytes each */
    int64_t *dps = NULL;
    if (kmer_file) {
        FILE *f = fopen(kmer_file, "r");
        if (!f) die("cannot read", kmer_file);
        char line[256];
        int64_t cap = 0;
        while (fgets(line, sizeof(line), f)) {
            line[strcspn(line, " \t\r\n")] = 0;
            if (!line[0]) continue;
            if (n_kmers == cap) {
                cap = cap ? 2 * cap : 64;
                kmers = must(realloc(kmers, (size_t) (cap * (k + 1))));
                dps = must(realloc(dps, sizeof(int64_t) * (size_t) cap));
            }
            const int dp = (int64_t) strlen(line) == k ? sa_hdp_state_kmer_dp(s, line) : -1;
            if (dp < 0) die("K-mer contains character outside alphabet or has the wrong length", line);
            memcpy(kmers + n_kmers * (k + 1), line, (size_t) (k + 1));
            dps[n_kmers++] = dp;
        }
        fclose(f);
        if (n_kmers < 1) die("no k-mer in", kmer_file);
    } else {
        n_kmers = 1;
        for (int64_t i = 0; i < k; i++) n_kmers *= info.alphabet_size;
        kmers = must(malloc((size_t) (n_kmers * (k + 1))));
        dps = must(malloc(sizeof(int64_t) * (size_t) n_kmers));
        for (int64_t id = 0; id < n_kmers; id++) {
            char *kmer = kmers + id * (k + 1);
            int64_t rest = id;
            kmer[k] = 0;
            for (int64_t i = k - 1; i >= 0; i--) {
                kmer[i] = alphabet[rest % info.alphabet_size];
                rest /= info.alphabet_size;
            }
            dps[id] = sa_hdp_state_kmer_dp(s, kmer);
        }
    }

    /* linspace (impl/hdp_math_utils.c:497-510) */
    double x[GRID_LENGTH];
    const double dx = (GRID_STOP - GRID_START) / ((double) (GRID_LENGTH - 1));
    for (int i = 0; i < GRID_LENGTH - 1; i++) x[i] = GRID_START + i * dx;
    x[GRID_LENGTH - 1] = GRID_STOP;
    FILE *xf = open_in_dir(dir, "x_vals", ".txt");
    for (int i = 0; i < GRID_LENGTH - 1; i++) fprintf(xf, "%.17lg\n", x[i]);
    fprintf(xf, "%.17lg", x[GRID_LENGTH - 1]);
    fclose(xf);

    double *dens = must(malloc(sizeof(double) * KMER_CHUNK * GRID_LENGTH));
    for (int64_t first = 0; first < n_kmers; first += KMER_CHUNK) {
        const int64_t n = n_kmers - first < KMER_CHUNK ? n_kmers - first : KMER_CHUNK;
        const int rc = sa_hdp_state_densities(s, dps + first, n, x, GRID_LENGTH, device, dens);
        if (rc != SA_OK) die("cannot evaluate the densities", sa_strerror(rc));
        for (int64_t i = 0; i < n; i++) {
            FILE *f = open_in_dir(dir, kmers + (first + i) * (k + 1), "_distr.txt");
            for (int g = 0; g < GRID_LENGTH; g++) fprintf(f, "%.17lg\n", dens[i * GRID_LENGTH + g]);
            fclose(f);
        }
    }
    free(dens);

    if (metric >= 0) {
        pair_writer_t w;
        w.s = s; w.metric = metric; w.device = device; w.kmers = kmers; w.stride = k + 1; w.n = 0;
        w.f = fopen(out_file, "w");
        if (!w.f) die("cannot write", out_file);
        w.dp_i = must(malloc(sizeof(int64_t) * PAIR_CHUNK)); w.dp_j = must(malloc(sizeof(int64_t) * PAIR_CHUNK));
        w.i = must(malloc(sizeof(int64_t) * PAIR_CHUNK)); w.j = must(malloc(sizeof(int64_t) * PAIR_CHUNK));
        w.d = must(malloc(sizeof(double) * PAIR_CHUNK));
        for (int64_t i = 1; i < n_kmers; i++)
            for (int64_t j = 0; j < i; j++) {
                w.i[w.n] = i; w.j[w.n] = j; w.dp_i[w.n] = dps[i]; w.dp_j[w.n] = dps[j];
                if (++w.n == PAIR_CHUNK) flush_pairs(&w);
            }
        flush_pairs(&w);
        free(w.dp_i); free(w.dp_j); free(w.i); free(w.j); free(w.d);
        fclose(w.f);
    }
    free(kmers);
    free(dps);
    sa_hdp_state_free(s);
    return 0;
}
