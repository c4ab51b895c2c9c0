/* Host half of the per-position profile (sa_profile.hip): the entropy term, the argument checks that run before anything is
 * added, and the file multipleAlignmentAnalysis.py writes (src/signalalign/scripts/multipleAlignmentAnalysis.py:203-242).
 * Nothing here touches the device, so that it can be built and run on its own. */
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "sa_internal.h"

/* shannon_entropy's summand (:101) of a printed posterior of u millionths, in units of 2^-40.  1 - q is taken as (10^6 - u) / 10^6,
 * so that the two products swap under u <-> 10^6 - u and the term is symmetric to the bit. */
int64_t sa_profile_entropy_term(int64_t units) {
    if (units <= 0 || units >= SA_PROFILE_UNITS_1) return 0;
    const double q = (double) units / 1e6, p = (double) (SA_PROFILE_UNITS_1 - units) / 1e6;
    return (int64_t) llrint((q * log2(q) + p * log2(p)) * 1099511627776.0);
}

int sa_profile_check_map(const sa_profile_job_map_t *map, int64_t n_jobs, int64_t n_contigs) {
    if (n_jobs < 0 || (n_jobs > 0 && !map)) return SA_EINVAL;
    for (int64_t j = 0; j < n_jobs; j++)
        if (map[j].contig < 0 || map[j].contig >= n_contigs || (map[j].pos_sign != 1 && map[j].pos_sign != -1)) return SA_EINVAL;
    return SA_OK;
}

int sa_profile_check_records(int64_t n_jobs, const int64_t *first, const int32_t *x, const int32_t *kmer_id, const int64_t *prob_e7,
                             int64_t n_kmers) {
    if (n_jobs < 0 || !first || first[0] != 0) return SA_EINVAL;
    for (int64_t j = 0; j < n_jobs; j++)
        if (first[j + 1] < first[j]) return SA_EINVAL;
    const int64_t n = first[n_jobs];
    if (n > 0 && (!x || !kmer_id || !prob_e7)) return SA_EINVAL;
    for (int64_t i = 0; i < n; i++)
        if (x[i] < 0 || x[i] >= SA_PAIR16_MAX_COORD || kmer_id[i] < 0 || kmer_id[i] >= n_kmers || prob_e7[i] < 0 ||
            prob_e7[i] > (int64_t) SA_PROB_1)
            return SA_EINVAL;
    return SA_OK;
}

/* the contig positions of the job's indices x_min .. x_max + k - 1, both ends inside [0, contig_len) */
int sa_profile_span(const sa_profile_job_map_t *m, int64_t contig_len, int64_t x_min, int64_t x_max, int k, int64_t *lo, int64_t *hi) {
    const int64_t far = (int64_t) 1 << 42;   /* (a contig has at most 2^40 positions, an index is below 2^28 + k) */
    if (x_min < 0 || x_max < x_min || m->pos0 < -far || m->pos0 > far) return SA_EINVAL;
    const int64_t a = m->pos0 + (int64_t) m->pos_sign * x_min, b = m->pos0 + (int64_t) m->pos_sign * (x_max + k - 1);
    *lo = a < b ? a : b;
    *hi = a < b ? b : a;
    return (*lo < 0 || *hi >= contig_len) ? SA_EINVAL : SA_OK;
}

int sa_position_profile_write(const char *path, const char *alphabet, uint32_t letters_seen, const char *const *contig_names,
                              const sa_profile_site_t *sites, int64_t n) {
    if (!path || !alphabet || !contig_names || n < 0 || (n > 0 && !sites)) return SA_EINVAL;
    const int n_alpha = (int) strlen(alphabet);
    if (n_alpha > SA_SITE_MAX_LETTERS || (n_alpha < 32 && (letters_seen >> n_alpha) != 0)) return SA_EINVAL;
    int order[SA_SITE_MAX_LETTERS], n_seen = 0;   /* the seen letters, sorted as the script sorts all_characters */
    for (int l = 0; l < n_alpha; l++)
        if (letters_seen >> l & 1u) {
            int at = n_seen++;
            while (at > 0 && (unsigned char) alphabet[order[at - 1]] > (unsigned char) alphabet[l]) { order[at] = order[at - 1]; at--; }
            order[at] = l;
        }
    FILE *fh = fopen(path, "w");
    if (!fh) return SA_EIO;
    setvbuf(fh, NULL, _IOFBF, 1 << 16);
    fputs("#contig\tposition\tref_char\tshannon_entropy\tkmer_aln_count\tread_aln_count", fh);
    for (int q = 0; q < n_seen; q++) fprintf(fh, "\tp%c", alphabet[order[q]]);
    fputc('\n', fh);
    char num[40];
    for (int64_t i = 0; i < n; i++) {
        const sa_profile_site_t *s = &sites[i];
        const char ref[2] = {s->ref, 0};
        sa_format_py_repr(num, s->entropy);
        fprintf(fh, "%s\t%" PRId64 "\t%s\t%s\t%" PRId64 "\t%d", contig_names[s->contig], s->pos, ref, num, s->kmer_count, (int) s->read_count);
        for (int q = 0; q < n_seen; q++) {
            sa_format_py_repr(num, s->prob[order[q]]);
            fprintf(fh, "\t%s", num);
        }
        fputc('\n', fh);
    }
    return fclose(fh) == 0 ? SA_OK : SA_EIO;
}
