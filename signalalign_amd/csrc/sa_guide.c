/* sa_guide.c -- host pieces of the guide-alignment stage (sa_guide.hip): placing a read inside its window by a k-mer vote, and
 * the exonerate line of a finished alignment.  Plain C, no device. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sa_io.h"
#include "signalalign_hip.h"

#define SEED_K 15
#define SEED_READ_BASES 2000
#define SEED_BIN 32
#define SEED_MIN_VOTES 8

typedef struct { uint32_t kmer; int32_t pos; } seed_kmer_t;

static int seed_cmp(const void *a, const void *b) {
    const seed_kmer_t *x = a, *y = b;
    if (x->kmer != y->kmer) return x->kmer < y->kmer ? -1 : 1;
    return x->pos < y->pos ? -1 : (x->pos > y->pos ? 1 : 0);
}
static int cmp_i64(const void *a, const void *b) {
    const int64_t x = *(const int64_t *) a, y = *(const int64_t *) b;
    return x < y ? -1 : (x > y ? 1 : 0);
}

/* the vote of one strand: returns the votes of the modal bin and its neighbours; *diag the median diagonal of those votes */
static int64_t seed_vote(const seed_kmer_t *rk, int64_t n_rk, int64_t read_bases, const char *win, int64_t win_len, int64_t *diag,
                         int64_t *hits_out) {
    *diag = 0;
    *hits_out = 0;
    if (n_rk == 0 || win_len < SEED_K) return 0;
    const int64_t n_bins = (win_len + read_bases) / SEED_BIN + 2;
    int64_t *bins = calloc((size_t) n_bins, sizeof(int64_t));
    int64_t cap = 1024, n_hits = 0;
    int64_t *hits = malloc(sizeof(int64_t) * (size_t) cap);
    if (!bins || !hits) { free(bins); free(hits); return -1; }
    uint32_t kmer = 0;
    int64_t run = 0;   /* letters of ACGT in a row ending here */
    const uint32_t mask = (1u << (2 * SEED_K)) - 1u;
    for (int64_t i = 0; i < win_len; i++) {
        const int c = sa_base_code(win[i]);
        if (c > 3) { run = 0; kmer = 0; continue; }
        kmer = ((kmer << 2) | (uint32_t) c) & mask;
        if (++run < SEED_K) continue;
        const int64_t wpos = i - (SEED_K - 1);
        int64_t lo = 0, hi = n_rk;   /* first entry with this k-mer */
        while (lo < hi) {
            const int64_t mid = (lo + hi) / 2;
            if (rk[mid].kmer < kmer) lo = mid + 1; else hi = mid;
        }
        for (; lo < n_rk && rk[lo].kmer == kmer; lo++) {
            const int64_t d = wpos - rk[lo].pos;
            if (n_hits == cap) {
                cap *= 2;
                int64_t *bigger = realloc(hits, sizeof(int64_t) * (size_t) cap);
                if (!bigger) { free(bins); free(hits); return -1; }
                hits = bigger;
            }
            hits[n_hits++] = d;
            bins[(d + read_bases) / SEED_BIN]++;
        }
    }
    int64_t modal = 0;
    for (int64_t b = 1; b < n_bins; b++)
        if (bins[b] > bins[modal]) modal = b;
    int64_t votes = 0;
    if (n_hits > 0) {
        for (int64_t h = 0; h < n_hits; h++) {
            const int64_t b = (hits[h] + read_bases) / SEED_BIN;
            if (b >= modal - 1 && b <= modal + 1) hits[votes++] = hits[h];
        }
        qsort(hits, (size_t) votes, sizeof(int64_t), cmp_i64);
        *diag = hits[(votes - 1) / 2];
    }
    *hits_out = n_hits;
    free(bins);
    free(hits);
    return votes;
}

int sa_guide_seed(const char *read, int64_t read_len, const char *window, int64_t window_len, int try_both_strands,
                  int64_t *diag_out, int *reverse_out, int64_t *votes_out, int64_t *hits_out) {
    if (!read || !window || !diag_out || !reverse_out || read_len < 0 || window_len < 0) return SA_EINVAL;
    *diag_out = 0;
    *reverse_out = 0;
    if (votes_out) *votes_out = 0;
    if (hits_out) *hits_out = 0;
    const int64_t bases = read_len < SEED_READ_BASES ? read_len : SEED_READ_BASES;
    seed_kmer_t *rk = malloc(sizeof(seed_kmer_t) * (size_t) (bases > 0 ? bases : 1));
    if (!rk) return SA_ENOMEM;
    int64_t n_rk = 0, run = 0;
    uint32_t kmer = 0;
    const uint32_t mask = (1u << (2 * SEED_K)) - 1u;
    for (int64_t i = 0; i < bases; i++) {
        const int c = sa_base_code(read[i]);
        if (c > 3) { run = 0; kmer = 0; continue; }
        kmer = ((kmer << 2) | (uint32_t) c) & mask;
        if (++run < SEED_K) continue;
        rk[n_rk].kmer = kmer;
        rk[n_rk].pos = (int32_t) (i - (SEED_K - 1));
        n_rk++;
    }
    qsort(rk, (size_t) n_rk, sizeof(seed_kmer_t), seed_cmp);
    int64_t diag[2] = {0, 0}, votes[2] = {0, 0}, hits[2] = {0, 0};
    votes[0] = seed_vote(rk, n_rk, bases, window, window_len, &diag[0], &hits[0]);
    int rc = votes[0] < 0 ? SA_ENOMEM : SA_OK;
    if (rc == SA_OK && try_both_strands) {
        char *tmp = malloc((size_t) window_len + 1);
        if (!tmp) rc = SA_ENOMEM;
        else {
            memcpy(tmp, window, (size_t) window_len);
            tmp[window_len] = 0;
            char *rcw = sa_reverse_complement(tmp);
            free(tmp);
            if (!rcw) rc = SA_ENOMEM;
            else {
                votes[1] = seed_vote(rk, n_rk, bases, rcw, window_len, &diag[1], &hits[1]);
                if (votes[1] < 0) rc = SA_ENOMEM;
                free(rcw);
            }
        }
    }
    free(rk);
    if (rc != SA_OK) return rc;
    const int s = votes[1] > votes[0] ? 1 : 0;
    if (votes_out) *votes_out = votes[s];
    if (hits_out) *hits_out = hits[s];
    if (votes[s] < SEED_MIN_VOTES) return 1;   /* no seed */
    *diag_out = diag[s];
    *reverse_out = s;
    return 0;
}

int64_t sa_guide_format_cigar(const char *label, int64_t read_start, int64_t read_end, const char *contig, int64_t ref_start,
                              int64_t ref_end, int forward, int64_t score, const int32_t *op_type, const int64_t *op_len,
                              int64_t n_ops, char *out, int64_t cap) {
    if (!label || !contig || n_ops < 0 || (n_ops > 0 && (!op_type || !op_len)) || (cap > 0 && !out)) return SA_EINVAL;
    for (int64_t i = 0; i < n_ops; i++)
        if (op_type[i] < 0 || op_type[i] > 2 || op_len[i] < 0) return SA_EINVAL;
    static const char letter[3] = {'M', 'D', 'I'};
    int64_t need = 0;
    for (int pass = 0; pass < 2; pass++) {
        char *dst = pass ? out : NULL;
        size_t room = pass ? (size_t) cap : 0;
        int64_t at = snprintf(dst, room, "cigar: %s %lld %lld + %s %lld %lld %c %lld", label, (long long) read_start, (long long) read_end,
                              contig, (long long) (forward ? ref_start : ref_end), (long long) (forward ? ref_end : ref_start),
                              forward ? '+' : '-', (long long) score);
        for (int64_t i = 0; i < n_ops; i++)
            at += snprintf(pass ? out + at : NULL, pass ? (size_t) (cap - at) : 0, " %c %lld", letter[op_type[i]], (long long) op_len[i]);
        need = at;
        if (pass == 0 && need + 1 > cap) return need;
    }
    return need;
}
