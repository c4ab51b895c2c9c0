/* sa_locate.c -- the reference index of the locate stage (sa_locate.hip): every 15-mer of ACGT of every contig, sorted by
 * (code, position), under a prefix table over the code's top bits.  Built here on the host, once per reference; plain C, the
 * upload is sa_locate.hip's.  The layout is restated in tests/locate_ref.py (build_index). */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "sa_io.h"
#include "sa_locate.h"

#define K SA_LOCATE_K
#define MAX_TOTAL (((int64_t) 1 << 31) - ((int64_t) 1 << 16))

static double now_seconds(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double) ts.tv_sec + 1e-9 * (double) ts.tv_nsec;
}

/* entries of one contig in position order, written at codes + at / pos + at (both NULL: counted only) */
static int64_t contig_entries(const char *seq, int64_t len, int64_t start, uint32_t *codes, int32_t *pos, int64_t at) {
    const uint32_t mask = (1u << (2 * K)) - 1u;
    uint32_t kmer = 0;
    int64_t run = 0, n = 0;
    for (int64_t i = 0; i < len; i++) {
        const int c = sa_base_code(seq[i]);
        if (c > 3) { run = 0; kmer = 0; continue; }
        kmer = ((kmer << 2) | (uint32_t) c) & mask;
        if (++run < K) continue;
        if (codes) { codes[at + n] = kmer; pos[at + n] = (int32_t) (start + i - (K - 1)); }
        n++;
    }
    return n;
}

/* stable LSD radix sort by the 30-bit code, three passes of ten bits: equal codes keep their order, i.e. ascending positions */
static int radix_sort(uint32_t *codes, int32_t *pos, int64_t n) {
    uint32_t *c2 = malloc(sizeof(uint32_t) * (size_t) (n ? n : 1));
    int32_t *p2 = malloc(sizeof(int32_t) * (size_t) (n ? n : 1));
    int64_t *count = malloc(sizeof(int64_t) * 1025);
    if (!c2 || !p2 || !count) { free(c2); free(p2); free(count); return SA_ENOMEM; }
    uint32_t *src_c = codes, *dst_c = c2;
    int32_t *src_p = pos, *dst_p = p2;
    for (int pass = 0; pass < 3; pass++) {
        const int shift = 10 * pass;
        memset(count, 0, sizeof(int64_t) * 1025);
        for (int64_t i = 0; i < n; i++) count[((src_c[i] >> shift) & 1023u) + 1]++;
        for (int b = 0; b < 1024; b++) count[b + 1] += count[b];
        for (int64_t i = 0; i < n; i++) {
            const int64_t to = count[(src_c[i] >> shift) & 1023u]++;
            dst_c[to] = src_c[i];
            dst_p[to] = src_p[i];
        }
        uint32_t *tc = src_c; src_c = dst_c; dst_c = tc;
        int32_t *tp = src_p; src_p = dst_p; dst_p = tp;
    }
    /* three passes: the sorted entries are in the scratch arrays */
    memcpy(codes, src_c, sizeof(uint32_t) * (size_t) n);
    memcpy(pos, src_p, sizeof(int32_t) * (size_t) n);
    free(c2); free(p2); free(count);
    return SA_OK;
}

void sa_ref_index_destroy(sa_ref_index_t *idx) {
    if (!idx) return;
    sa_locate_drop_device(idx);
    if (idx->names)
        for (int64_t i = 0; i < idx->n_contigs; i++) free(idx->names[i]);
    free(idx->names); free(idx->starts); free(idx->codes); free(idx->pos); free(idx->table);
    free(idx);
}

int sa_ref_index_build(sa_ref_index_t **out, const char *const *names, const char *const *seqs, const int64_t *lens,
                       int64_t n_contigs, int device) {
    if (!out || !names || !seqs || !lens || n_contigs <= 0) return SA_EINVAL;
    *out = NULL;
    int64_t total = 0;
    for (int64_t i = 0; i < n_contigs; i++) {
        if (!names[i] || lens[i] < 0 || (lens[i] > 0 && !seqs[i])) return SA_EINVAL;
        if (lens[i] >= MAX_TOTAL || (total += lens[i]) >= MAX_TOTAL) return SA_EUNSUPPORTED;
    }
    const double t0 = now_seconds();
    sa_ref_index_t *idx = calloc(1, sizeof(*idx));
    if (!idx) return SA_ENOMEM;
    idx->device = -1;
    idx->n_contigs = n_contigs;
    idx->total = total;
    idx->names = calloc((size_t) n_contigs, sizeof(char *));
    idx->starts = malloc(sizeof(int64_t) * (size_t) (n_contigs + 1));
    int rc = idx->names && idx->starts ? SA_OK : SA_ENOMEM;
    int64_t n = 0;
    for (int64_t i = 0; i < n_contigs && rc == SA_OK; i++) {
        if (!(idx->names[i] = strdup(names[i]))) rc = SA_ENOMEM;
        idx->starts[i] = i == 0 ? 0 : idx->starts[i - 1] + lens[i - 1];
        n += contig_entries(seqs[i], lens[i], 0, NULL, NULL, 0);
    }
    if (rc == SA_OK) {
        idx->starts[n_contigs] = total;
        idx->n_entries = n;
        idx->codes = malloc(sizeof(uint32_t) * (size_t) (n ? n : 1));
        idx->pos = malloc(sizeof(int32_t) * (size_t) (n ? n : 1));
        if (!idx->codes || !idx->pos) rc = SA_ENOMEM;
    }
    if (rc == SA_OK) {
        int64_t at = 0;
        for (int64_t i = 0; i < n_contigs; i++) at += contig_entries(seqs[i], lens[i], idx->starts[i], idx->codes, idx->pos, at);
        rc = radix_sort(idx->codes, idx->pos, n);
    }
    if (rc == SA_OK) {
        int q = 16;
        while (q < 26 && ((int64_t) 1 << q) < n) q += 2;
        idx->q = q;
        const int64_t n_buckets = (int64_t) 1 << q;
        idx->table = malloc(sizeof(int32_t) * (size_t) (n_buckets + 1));
        if (!idx->table) rc = SA_ENOMEM;
        else {   /* table[b]: entries whose bucket is below b */
            int64_t e = 0;
            for (int64_t b = 0; b <= n_buckets; b++) {
                while (e < n && (int64_t) (idx->codes[e] >> (2 * K - q)) < b) e++;
                idx->table[b] = (int32_t) e;
            }
        }
    }
    if (rc == SA_OK && device >= 0) {
        idx->device = device;
        rc = sa_locate_upload(idx);
    }
    if (rc != SA_OK) { sa_ref_index_destroy(idx); return rc; }
    idx->build_seconds = now_seconds() - t0;
    *out = idx;
    return SA_OK;
}

int sa_ref_index_build_fasta(sa_ref_index_t **out, const char *fasta_path, int device) {
    if (!out || !fasta_path) return SA_EINVAL;
    *out = NULL;
    char **names = NULL, **seqs = NULL;
    int64_t *lens = NULL, n = 0;
    const double t0 = now_seconds();
    int rc = sa_fasta_read_all(fasta_path, &names, &seqs, &lens, &n);
    if (rc != SA_OK) return rc;
    rc = sa_ref_index_build(out, (const char *const *) names, (const char *const *) seqs, lens, n, device);
    sa_fasta_records_free(names, seqs, lens, n);
    if (rc == SA_OK) (*out)->build_seconds = now_seconds() - t0;   /* reading the file is part of it */
    return rc;
}

int sa_ref_index_info(const sa_ref_index_t *idx, sa_ref_index_info_t *info) {
    if (!idx || !info) return SA_EINVAL;
    memset(info, 0, sizeof(*info));
    info->n_contigs = idx->n_contigs;
    info->total_bases = idx->total;
    info->n_entries = idx->n_entries;
    info->q = idx->q;
    info->device = idx->device;
    info->host_bytes = 8 * idx->n_entries + 4 * (((int64_t) 1 << idx->q) + 1) + 8 * (idx->n_contigs + 1);
    info->device_bytes = idx->device_bytes;
    info->build_seconds = idx->build_seconds;
    return SA_OK;
}

int sa_ref_index_entries(const sa_ref_index_t *idx, const uint32_t **codes, const int32_t **pos, const int32_t **table,
                         const int64_t **contig_start) {
    if (!idx) return SA_EINVAL;
    if (codes) *codes = idx->codes;
    if (pos) *pos = idx->pos;
    if (table) *table = idx->table;
    if (contig_start) *contig_start = idx->starts;
    return SA_OK;
}

int sa_ref_index_contig(const sa_ref_index_t *idx, int64_t i, const char **name, int64_t *start, int64_t *len) {
    if (!idx || i < 0 || i >= idx->n_contigs) return SA_EINVAL;
    if (name) *name = idx->names[i];
    if (start) *start = idx->starts[i];
    if (len) *len = idx->starts[i + 1] - idx->starts[i];
    return SA_OK;
}

int sa_locate_window(const sa_ref_index_t *idx, const sa_locate_result_t *r, int64_t read_len, int32_t band, int64_t *start,
                     int64_t *end) {
    if (!idx || !r || !start || !end || read_len < 0 || band < 0 || r->contig < 0 || r->contig >= idx->n_contigs) return SA_EINVAL;
    const int64_t len = idx->starts[r->contig + 1] - idx->starts[r->contig], ext = read_len + read_len / 4 + band;
    int64_t lo = r->reverse ? r->pos + 1 - ext : r->pos - band, hi = r->reverse ? r->pos + 1 + band : r->pos + ext;
    if (lo < 0) lo = 0;
    if (hi > len) hi = len;
    if (lo >= hi) return SA_EINVAL;
    *start = lo;
    *end = hi;
    return SA_OK;
}
