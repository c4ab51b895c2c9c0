/* compareDistributions -- drop-in for the reference's executable of the same name (impl/compareDistributions.c): dumps the
 * density of every k-mer of a NanoporeHDP (.nhdp) on linspace(30, 90, 600) into <dir>/x_vals.txt and <dir>/<kmer>_distr.txt, which
 * visualization/compare_trained_models.py reads.  Argument order, the usage line, the two notices and the file formats follow the
 * reference; the densities are the library's (sa_hdp_state_densities: dir_proc_density on the GPU, k-mers in chunks).
 *
 * Beside the reference's two arguments: --kmers FILE (dump only the k-mers listed there, one per line), --distances
 * kl|hellinger|l2|shannonJensen --out FILE (kmer_i <tab> kmer_j <tab> distance for every pair i > j of the listed k-mers, or of all
 * k-mers: get_kmer_distr_distance, impl/nanopore_hdp.c:431-434, through sa_hdp_state_distance_pairs) and --device <n>.
 *
 * --model FILE.model --compare OUT.tsv: the HDP against the Gaussian table it stands beside (compare_distributions,
 * src/signalalign/hiddenMarkovModel.py:775-837, through sa_hdp_state_vs_gaussian): one line per dumped k-mer,
 * kmer <tab> status <tab> kl_bits <tab> hellinger <tab> mode_delta, the normal density being the model's level mean and sd.  With
 * --assignments TABLE.tsv [--strand t|c] [--bandwidth H] (the four-column table sa_kmer_table_write writes) also the data: a Gaussian
 * kernel density estimate of every k-mer's event means (plot_kmer_distribution, :654-773, through sa_kmer_table_kde) goes to
 * <dir>/<kmer>_kde.txt in the format of <kmer>_distr.txt, and n_rows <tab> kde_vs_hdp <tab> kde_vs_gaussian are appended to each
 * line: the metric --distances names (hellinger if none) between the three curves on the x_vals grid (sa_hdp_distances_paired).
 */
#include <inttypes.h>
#include <math.h>
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

/* the rows of an assignments table (kmer, strand, descaled mean, posterior) of one strand into a k-mer table that drops none */
static sa_kmer_table_t *table_from_assignments(const char *path, const sa_model_t *m, int64_t k, char strand, int device) {
    FILE *f = fopen(path, "r");
    if (!f) die("cannot read", path);
    int64_t n = 0, cap = 0;
    int32_t *ids = NULL;
    double *mean = NULL, *prob = NULL;
    char line[512], kmer[256], st[16];
    while (fgets(line, sizeof(line), f)) {
        double v, pr;
        const int got = sscanf(line, "%255s %15s %lf %lf", kmer, st, &v, &pr);
        if (got <= 0) continue;
        if (got != 4) die("not a four-column assignments table", path);
        if (st[0] != strand || st[1]) continue;
        const int64_t id = (int64_t) strlen(kmer) == k ? sa_kmer_id(m, kmer) : -1;
        if (id < 0) die("K-mer contains character outside alphabet or has the wrong length", kmer);
        if (n == cap) {
            cap = cap ? 2 * cap : 4096;
            ids = must(realloc(ids, sizeof(int32_t) * (size_t) cap));
            mean = must(realloc(mean, sizeof(double) * (size_t) cap));
            prob = must(realloc(prob, sizeof(double) * (size_t) cap));
        }
        ids[n] = (int32_t) id; mean[n] = v; prob[n] = pr;
        n++;
    }
    fclose(f);
    sa_kmer_table_t *t = NULL;
    int rc = sa_kmer_table_create(&t, m, n > 0 ? n : 1, 0.0, device);
    if (rc == SA_OK) rc = sa_kmer_table_add_rows(t, 0, ids, mean, prob, n);
    if (rc != SA_OK) die("cannot build the k-mer table", sa_strerror(rc));
    free(ids); free(mean); free(prob);
    return t;
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
    const char *gauss_file = NULL, *compare_file = NULL, *assignments_file = NULL, *strand_name = NULL, *bandwidth_text = NULL;
    int n_positional = 0, device = 0;
    for (int i = 1; i < argc; i++) {
        const char **value = NULL;
        if (strcmp(argv[i], "--kmers") == 0) value = &kmer_file;
        else if (strcmp(argv[i], "--distances") == 0) value = &metric_name;
        else if (strcmp(argv[i], "--out") == 0) value = &out_file;
        else if (strcmp(argv[i], "--model") == 0) value = &gauss_file;
        else if (strcmp(argv[i], "--compare") == 0) value = &compare_file;
        else if (strcmp(argv[i], "--assignments") == 0) value = &assignments_file;
        else if (strcmp(argv[i], "--strand") == 0) value = &strand_name;
        else if (strcmp(argv[i], "--bandwidth") == 0) value = &bandwidth_text;
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
        if (!out_file && !compare_file) die("--distances needs --out FILE", NULL);
    } else if (out_file) {
        die("--out needs --distances", NULL);
    }
    if (!gauss_file != !compare_file) die("--model FILE.model and --compare OUT.tsv go together", NULL);
    if ((assignments_file || strand_name || bandwidth_text) && !compare_file) die("--assignments, --strand and --bandwidth need --compare", NULL);
    if ((strand_name || bandwidth_text) && !assignments_file) die("--strand and --bandwidth need --assignments", NULL);
    if (strand_name && strcmp(strand_name, "t") != 0 && strcmp(strand_name, "c") != 0) die("--strand takes t or c, not", strand_name);
    double bandwidth = 0.5;
    if (bandwidth_text) {
        char *end = NULL;
        bandwidth = strtod(bandwidth_text, &end);
        if (!end || *end || !(bandwidth > 0) || !isfinite(bandwidth)) die("--bandwidth takes a positive number, not", bandwidth_text);
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

    /* the Gaussian table the HDP is compared with: same alphabet, same k */
    sa_model_t *gauss = NULL;
    if (gauss_file) {
        char m_alphabet[64];
        int m_n_alpha = 0, m_k = 0;
        if (sa_model_load(&gauss, gauss_file, NULL) != SA_OK || sa_model_alphabet(gauss, m_alphabet, &m_n_alpha, &m_k) != SA_OK)
            die("cannot read the model", gauss_file);
        if (m_k != k || m_n_alpha != info.alphabet_size || strncmp(m_alphabet, alphabet, (size_t) m_n_alpha) != 0)
            die("the model's alphabet and k-mer length are not the NanoporeHDP's", gauss_file);
    }

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

    FILE *cf = NULL;
    sa_kmer_table_t *table = NULL;
    sa_hdp_gauss_cmp_t *cmp = NULL;
    double *mu = NULL, *sd = NULL, *kde = NULL, *normal = NULL, *d_hdp = NULL, *d_gauss = NULL;
    int32_t *ids = NULL;
    int64_t *n_rows = NULL;
    if (compare_file) {
        cf = fopen(compare_file, "w");
        if (!cf) die("cannot write", compare_file);
        cmp = must(malloc(sizeof(sa_hdp_gauss_cmp_t) * KMER_CHUNK));
        mu = must(malloc(sizeof(double) * KMER_CHUNK)); sd = must(malloc(sizeof(double) * KMER_CHUNK));
        ids = must(malloc(sizeof(int32_t) * KMER_CHUNK));
        if (assignments_file) {
            table = table_from_assignments(assignments_file, gauss, k, strand_name ? strand_name[0] : 't', device);
            kde = must(malloc(sizeof(double) * KMER_CHUNK * GRID_LENGTH)); normal = must(malloc(sizeof(double) * KMER_CHUNK * GRID_LENGTH));
            d_hdp = must(malloc(sizeof(double) * KMER_CHUNK)); d_gauss = must(malloc(sizeof(double) * KMER_CHUNK));
            n_rows = must(malloc(sizeof(int64_t) * KMER_CHUNK));
        }
    }
    double *dens = must(malloc(sizeof(double) * KMER_CHUNK * GRID_LENGTH));
    for (int64_t first = 0; first < n_kmers; first += KMER_CHUNK) {
        const int64_t n = n_kmers - first < KMER_CHUNK ? n_kmers - first : KMER_CHUNK;
        int rc = sa_hdp_state_densities(s, dps + first, n, x, GRID_LENGTH, device, dens);
        if (rc != SA_OK) die("cannot evaluate the densities", sa_strerror(rc));
        for (int64_t i = 0; i < n; i++) {
            FILE *f = open_in_dir(dir, kmers + (first + i) * (k + 1), "_distr.txt");
            for (int g = 0; g < GRID_LENGTH; g++) fprintf(f, "%.17lg\n", dens[i * GRID_LENGTH + g]);
            fclose(f);
        }
        if (!cf) continue;
        const double *table5 = sa_model_table5(gauss);
        for (int64_t i = 0; i < n; i++) {
            const int64_t id = sa_kmer_id(gauss, kmers + (first + i) * (k + 1));
            if (id < 0) die("K-mer contains character outside alphabet", kmers + (first + i) * (k + 1));
            ids[i] = (int32_t) id;
            mu[i] = table5[5 * id];
            sd[i] = table5[5 * id + 1];
        }
        rc = sa_hdp_state_vs_gaussian(s, dps + first, n, mu, sd, device, cmp, NULL);
        if (rc != SA_OK) die("cannot compare with the model", sa_strerror(rc));
        if (table) {
            rc = sa_kmer_table_kde(table, 0, ids, n, x, GRID_LENGTH, bandwidth, kde, n_rows, NULL);
            if (rc != SA_OK) die("cannot evaluate the kernel density estimates", sa_strerror(rc));
            for (int64_t i = 0; i < n; i++) {
                FILE *f = open_in_dir(dir, kmers + (first + i) * (k + 1), "_kde.txt");
                for (int g = 0; g < GRID_LENGTH; g++) {
                    const double z = (x[g] - mu[i]) / sd[i];
                    kde[i * GRID_LENGTH + g] = exp(kde[i * GRID_LENGTH + g]);
                    normal[i * GRID_LENGTH + g] = exp(-(z * z) / 2.0) / 2.5066282746310002 / sd[i];   /* scipy's norm.pdf */
                    fprintf(f, "%.17lg\n", kde[i * GRID_LENGTH + g]);
                }
                fclose(f);
            }
            const int m = metric >= 0 ? metric : SA_HDP_METRIC_HELLINGER;
            if ((rc = sa_hdp_distances_paired(x, GRID_LENGTH, kde, dens, n, m, device, d_hdp, NULL)) != SA_OK ||
                (rc = sa_hdp_distances_paired(x, GRID_LENGTH, kde, normal, n, m, device, d_gauss, NULL)) != SA_OK)
                die("cannot evaluate the distances", sa_strerror(rc));
        }
        for (int64_t i = 0; i < n; i++) {
            fprintf(cf, "%s\t%d\t%.17g\t%.17g\t%.17g", kmers + (first + i) * (k + 1), (int) cmp[i].status, cmp[i].kl_bits, cmp[i].hellinger,
                    cmp[i].mode_delta);
            if (table) fprintf(cf, "\t%" PRId64 "\t%.17g\t%.17g", n_rows[i], d_hdp[i], d_gauss[i]);
            fputc('\n', cf);
        }
    }
    free(dens);
    if (cf && fclose(cf) != 0) die("cannot write", compare_file);
    if (table) sa_kmer_table_destroy(table);
    if (gauss) sa_model_destroy(gauss);
    free(cmp); free(mu); free(sd); free(ids); free(kde); free(normal); free(d_hdp); free(d_gauss); free(n_rows);

    if (metric >= 0 && out_file) {
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
