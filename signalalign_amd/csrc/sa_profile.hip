// Per-position profile of all reads' posteriors on gfx950 -- multipleAlignmentAnalysis.py (src/signalalign/scripts/
// multipleAlignmentAnalysis.py:52-69, :118-242) over the records of finished batches, kept in HBM across batches
// (include/signalalign_hip.h has the semantics and the three deliberate differences from the script; sa_profile.c the host half).
//
// The accumulator is a table over contig positions (sa_contig_acc.h has the layout, the life cycle and the compaction of finish;
// here are the sums and their kernels) in which every contig has one slot more than positions, where the difference array of its
// spans takes the -1 of a span that ends on the last position.  Its store is [acc | diff | seen], per slot g, with S = 2 + letters
// of the alphabet: acc[g * S + 0] the contributions, acc[g * S + 1] the entropy units, acc[g * S + 2 + l] the printed units of
// letter l (64-bit integers), diff[g] the spans' difference array (int32); one word more holds the seen letters.  A checkpoint
// covers all of it.
//
// Kernels of an add:
//   k_pf_range        one block per chunk of a job's records: the job's smallest and largest x (LDS, then one global atomic min /
//                     max per block), and a flag for a k-mer id or a posterior the table cannot take.  The host maps the two ends
//                     of every job and refuses the call before anything is added (sa_profile_span).
//   k_pf_spans        one thread per job with records: +1 / -1 into the difference array
//   k_pf_accumulate   one block per chunk (SaRecChunk, at most SA_CHAIN_CHUNK records of one alignment), in tiles of W records.  A
//                     tile's records are consecutive along an alignment and touch a narrow run of indices: the block takes the
//                     tile's smallest x as the base of a window of W indices in LDS (W * S 64-bit words: the count, the entropy
//                     units and the letters' units of every index), adds with LDS atomics, and flushes the non-zero words with one
//                     64-bit global atomic each.  A contribution outside the window goes straight to a global atomic, so the
//                     result never depends on the window; SA_PROFILE_DIRECT sends every contribution that way.  The entropy term
//                     is looked up once per record in the table of the 1 000 001 terms (the host function's values, built once
//                     per process, one device copy per table).
// Kernels of finish, between which sa_acc_finish scans the blocks' counts:
//   k_pf_block_sums   one block per 2048 slots: the sum of its differences, scanned over the blocks (k_acc_scan) before
//   k_pf_mark         read_count of every slot from the scanned sums; how many slots of the block are reported
//   k_pf_emit         the sites, compacted in (contig, position) order
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "sa_internal.h"
#include "sa_contig_acc.h"

#define PF_THREADS 256
#define PF_LDS_WORDS 6144   // 48 KiB of window: three blocks per CU
#define PF_ERR_RECORD 1

struct PfJob {
    long long g0;          // slot of index 0 of the job's ref
    long long d_lo, d_hi;  // the span's slots (a job with records)
    int sign, has;
};

struct PfArgs {
    const sa_pair16_t *recs;
    const SaRecChunk *chunks;
    const PfJob *jobs;
    const long long *term;          // SA_PROFILE_UNITS_1 + 1 entries
    unsigned long long *acc;
    unsigned *seen;
    long long n_slots;
    int k, n_alpha, S, W;
    unsigned char comp[SA_SITE_MAX_LETTERS];
};

// poisoned: an add failed after its spans went in, and part of the call may be in the table
struct sa_position_profile : SaContigAcc {
    int k = 0, n_alpha = 0, S = 0;
    long long n_kmers = 0;
    char alphabet[SA_SITE_MAX_LETTERS + 1] = {0};
    unsigned char comp[SA_SITE_MAX_LETTERS] = {0};
    long long *d_term = nullptr;
    size_t o_diff = 0, o_seen = 0;   // of the store's [acc | diff | seen]
    unsigned long long *acc() const { return (unsigned long long *) d_store; }
    int *diff() const { return (int *) (d_store + o_diff); }
    unsigned *seen() const { return (unsigned *) (d_store + o_seen); }
};

// the 1 000 001 terms of sa_profile_entropy_term, made once per process
static const std::vector<long long> &pf_terms() {
    static std::vector<long long> tab;
    static std::once_flag once;
    std::call_once(once, [] {
        tab.resize((size_t) SA_PROFILE_UNITS_1 + 1);
        for (long long u = 0; u <= SA_PROFILE_UNITS_1; u++) tab[(size_t) u] = sa_profile_entropy_term(u);
    });
    return tab;
}

__device__ __forceinline__ void pf_rec(const sa_pair16_t r, int *x, unsigned *kmer, long long *pe7) {
    *x = (int) (r.a & 0xfffffffull);
    *kmer = (unsigned) (r.b & 0xffffffffull);
    *pe7 = (long long) ((r.b >> 32) & 0xffffffull);
}

__global__ __launch_bounds__(PF_THREADS) void k_pf_range(const sa_pair16_t *__restrict__ recs, const SaRecChunk *__restrict__ chunks,
                                                         long long n_kmers, int *__restrict__ xmin, int *__restrict__ xmax,
                                                         unsigned *__restrict__ err) {
    __shared__ int s_lo, s_hi;
    if (threadIdx.x == 0) { s_lo = INT_MAX; s_hi = -1; }
    __syncthreads();
    const SaRecChunk C = chunks[blockIdx.x];
    int lo = INT_MAX, hi = -1;
    bool bad = false;
    for (int i = threadIdx.x; i < C.n; i += PF_THREADS) {
        int x;
        unsigned kmer;
        long long pe7;
        pf_rec(recs[C.first + i], &x, &kmer, &pe7);
        lo = min(lo, x);
        hi = max(hi, x);
        bad |= (long long) kmer >= n_kmers || pe7 > (long long) SA_PROB_1;
    }
    if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    if (bad) atomicOr(err, (unsigned) PF_ERR_RECORD);
    __syncthreads();
    if (threadIdx.x == 0 && s_hi >= 0) { atomicMin(&xmin[C.job], s_lo); atomicMax(&xmax[C.job], s_hi); }
}

__global__ __launch_bounds__(PF_THREADS) void k_pf_spans(const PfJob *__restrict__ jobs, int nj, int *__restrict__ diff) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nj || !jobs[j].has) return;
    atomicAdd(&diff[jobs[j].d_lo], 1);
    atomicAdd(&diff[jobs[j].d_hi + 1], -1);
}

template <bool DIRECT>
__global__ __launch_bounds__(PF_THREADS) void k_pf_accumulate(const PfArgs A) {
    __shared__ unsigned long long win[DIRECT ? 1 : PF_LDS_WORDS];
    __shared__ int s_base;
    __shared__ unsigned s_seen;
    const SaRecChunk C = A.chunks[blockIdx.x];
    const PfJob J = A.jobs[C.job];
    const int S = A.S, W = A.W;
    unsigned seen = 0;
    if (threadIdx.x == 0) s_seen = 0;
    for (int t0 = 0; t0 < C.n; t0 += W) {
        const int tn = min(W, C.n - t0);
        int base = 0;
        if (!DIRECT) {
            if (threadIdx.x == 0) s_base = INT_MAX;
            for (int e = threadIdx.x; e < W * S; e += PF_THREADS) win[e] = 0;
            __syncthreads();
            int lo = INT_MAX;
            for (int i = threadIdx.x; i < tn; i += PF_THREADS) lo = min(lo, (int) (A.recs[C.first + t0 + i].a & 0xfffffffull));
            if (lo != INT_MAX) atomicMin(&s_base, lo);
            __syncthreads();
            base = s_base;
        }
        for (int i = threadIdx.x; i < tn; i += PF_THREADS) {
            int x;
            unsigned kmer;
            long long pe7;
            pf_rec(A.recs[C.first + t0 + i], &x, &kmer, &pe7);
            const long long u = sa_printed_units(pe7);
            if (u < 0 || u > SA_PROFILE_UNITS_1) continue;   // (k_pf_range refused the call: not reached)
            const unsigned long long units = (unsigned long long) u, term = (unsigned long long) A.term[u];
            for (int d = A.k - 1; d >= 0; d--) {   // digit d of the k-mer id, the last letter first
                const unsigned dg = kmer % (unsigned) A.n_alpha;
                kmer /= (unsigned) A.n_alpha;
                const int letter = J.sign < 0 ? (int) A.comp[dg] : (int) dg;
                seen |= 1u << letter;
                const int p = x + d;
                const unsigned w = (unsigned) (p - base);
                if (!DIRECT && w < (unsigned) W) {
                    unsigned long long *e = win + (size_t) w * S;
                    atomicAdd(&e[0], 1ull);
                    if (term) atomicAdd(&e[1], term);
                    if (units) atomicAdd(&e[2 + letter], units);
                } else {
                    const long long g = J.g0 + (long long) J.sign * p;
                    if (g < 0 || g >= A.n_slots) continue;   // (the host checked the job's ends: not reached)
                    unsigned long long *e = A.acc + (size_t) g * S;
                    atomicAdd(&e[0], 1ull);
                    if (term) atomicAdd(&e[1], term);
                    if (units) atomicAdd(&e[2 + letter], units);
                }
            }
        }
        if (!DIRECT) {
            __syncthreads();
            for (int e = threadIdx.x; e < W * S; e += PF_THREADS) {
                const unsigned long long v = win[e];
                if (!v) continue;
                const int w = e / S;
                const long long g = J.g0 + (long long) J.sign * (base + w);
                if (g < 0 || g >= A.n_slots) continue;
                atomicAdd(&A.acc[(size_t) g * S + (e - w * S)], v);
            }
            __syncthreads();
        }
    }
    __syncthreads();   // (s_seen's clearing, when the chunk had no tile to synchronise on)
    if (seen) atomicOr(&s_seen, seen);
    __syncthreads();
    if (threadIdx.x == 0 && s_seen) atomicOr(A.seen, s_seen);
}

extern "C" int sa_position_profile_create(sa_position_profile_t **out, const sa_model_t *m, const int64_t *contig_lens, int64_t n_contigs,
                                          int device) {
    if (!out || !m) return SA_EINVAL;
    *out = nullptr;
    sa_position_profile *t = new (std::nothrow) sa_position_profile();
    if (!t) return SA_ENOMEM;
    int rc = sa_acc_layout(t, contig_lens, n_contigs, /* pad */ 1);
    if (rc == SA_OK && (m->n_alpha > SA_SITE_MAX_LETTERS || m->n_alpha < 1 || m->k < 1 || m->n_kmers > (int64_t) INT32_MAX)) rc = SA_EUNSUPPORTED;
    for (int l = 0; rc == SA_OK && l < m->n_alpha; l++) {
        const char c = m->alphabet[l];
        const char want = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
        const char *hit = (const char *) memchr(m->alphabet, want, (size_t) m->n_alpha);
        if (!hit) rc = SA_EUNSUPPORTED;
        else t->comp[l] = (unsigned char) (hit - m->alphabet);
    }
    if (rc != SA_OK) { delete t; return rc; }
    t->k = m->k;
    t->n_alpha = m->n_alpha;
    t->S = 2 + m->n_alpha;
    t->n_kmers = m->n_kmers;
    memcpy(t->alphabet, m->alphabet, (size_t) m->n_alpha);
    SaLayout L;
    (void) L.add(8 * (size_t) t->S * (size_t) t->n_slots);
    t->o_diff = L.add(4 * (size_t) t->n_slots);
    t->o_seen = L.add(4);
    const std::vector<long long> &terms = pf_terms();
    rc = sa_acc_alloc(t, device, L.end, L.end);
    if (rc != SA_OK) goto done;
    SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &t->d_term, 8 * terms.size(), device));
    SA_HIP_GOTO_DONE(hipMemcpy(t->d_term, terms.data(), 8 * terms.size(), hipMemcpyHostToDevice));
done:
    if (rc != SA_OK) { sa_position_profile_destroy(t); return rc; }
    *out = t;
    return SA_OK;
}

extern "C" void sa_position_profile_destroy(sa_position_profile_t *t) {
    if (!t) return;
    sa_acc_free(t);
    g_sa_pool.put(SaPool::DEVICE, t->d_term);
    delete t;
}

// the records `recs` (on the device; job j's are V.first[j] .. + V.count[j]) added; the caller holds t->mu, the map's contigs and
// signs are checked and the device is set
static int pf_add(sa_position_profile *t, const sa_pair16_t *recs, const SaBatchView &V, const sa_profile_job_map_t *map, unsigned flags,
                  double *kernel_ms_out) {
    const size_t nj = V.count.size();
    const std::vector<SaRecChunk> chunks = sa_view_chunks(V, SA_CHAIN_CHUNK, SA_ORDINAL_PER_JOB);
    const size_t nc = chunks.size();
    if (nc == 0) return SA_OK;
    if (nc > (size_t) INT32_MAX || nj > (size_t) INT32_MAX) return SA_EUNSUPPORTED;
    int rc = SA_OK;
    bool adding = false;
    SaLayout L;   // [chunks | smallest x, largest x of every job | err | jobs]
    const size_t o_ch = L.add(sizeof(SaRecChunk) * nc), o_x = L.add(4 * 2 * nj), o_err = L.add(4), o_jobs = L.add(sizeof(PfJob) * nj);
    char *d = nullptr;
    std::vector<int> hx(2 * nj);
    std::vector<PfJob> jobs(nj);
    unsigned h_err = 0;
    float ms0 = 0, ms1 = 0;
    if (g_sa_pool.get(SaPool::DEVICE, (void **) &d, L.end, t->device) != hipSuccess) return SA_ENOMEM;
    {
        int *xmin = (int *) (d + o_x), *xmax = xmin + nj;
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_ch, chunks.data(), sizeof(SaRecChunk) * nc, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemsetAsync(xmin, 0x7f, 4 * nj, 0));   // (0x7f7f7f7f: above every x)
        SA_HIP_GOTO_DONE(hipMemsetAsync(xmax, 0xff, 4 * nj, 0));   // (-1)
        SA_HIP_GOTO_DONE(hipMemsetAsync(d + o_err, 0, 4, 0));
        SA_HIP_GOTO_DONE(hipEventRecord(t->e0, 0));
        hipLaunchKernelGGL(k_pf_range, dim3((unsigned) nc), dim3(PF_THREADS), 0, 0, recs, (const SaRecChunk *) (d + o_ch), t->n_kmers, xmin, xmax,
                           (unsigned *) (d + o_err));
        SA_HIP_GOTO_DONE(hipEventRecord(t->e1, 0));
        SA_HIP_GOTO_DONE(hipGetLastError());
        SA_HIP_GOTO_DONE(hipMemcpy(hx.data(), xmin, 4 * 2 * nj, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(hipMemcpy(&h_err, d + o_err, 4, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(hipEventElapsedTime(&ms0, t->e0, t->e1));
        if (h_err) { rc = SA_EINVAL; goto done; }
        for (size_t j = 0; j < nj; j++) {   // every job's two ends on its contig, before anything is added
            PfJob &J = jobs[j];
            const size_t c = (size_t) map[j].contig;
            J.sign = map[j].pos_sign;
            J.has = V.count[j] > 0;
            J.g0 = J.d_lo = J.d_hi = 0;
            if (!J.has) continue;
            int64_t lo = 0, hi = 0;
            if (sa_profile_span(&map[j], t->clen[c], hx[j], hx[nj + j], t->k, &lo, &hi) != SA_OK) { rc = SA_EINVAL; goto done; }
            J.g0 = t->coff[c] + map[j].pos0;
            J.d_lo = t->coff[c] + lo;
            J.d_hi = t->coff[c] + hi;
        }
        PfArgs A;
        A.recs = recs;
        A.chunks = (const SaRecChunk *) (d + o_ch);
        A.jobs = (const PfJob *) (d + o_jobs);
        A.term = t->d_term;
        A.acc = t->acc();
        A.seen = t->seen();
        A.n_slots = t->n_slots;
        A.k = t->k; A.n_alpha = t->n_alpha; A.S = t->S;
        A.W = PF_LDS_WORDS / t->S;
        memcpy(A.comp, t->comp, sizeof A.comp);
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_jobs, jobs.data(), sizeof(PfJob) * nj, hipMemcpyHostToDevice, 0));
        adding = true;
        SA_HIP_GOTO_DONE(hipEventRecord(t->e0, 0));
        hipLaunchKernelGGL(k_pf_spans, dim3((unsigned) ((nj + PF_THREADS - 1) / PF_THREADS)), dim3(PF_THREADS), 0, 0, A.jobs, (int) nj, t->diff());
        if (flags & SA_PROFILE_DIRECT) hipLaunchKernelGGL(k_pf_accumulate<true>, dim3((unsigned) nc), dim3(PF_THREADS), 0, 0, A);
        else hipLaunchKernelGGL(k_pf_accumulate<false>, dim3((unsigned) nc), dim3(PF_THREADS), 0, 0, A);
        SA_HIP_GOTO_DONE(hipEventRecord(t->e1, 0));
        SA_HIP_GOTO_DONE(hipGetLastError());
        SA_HIP_GOTO_DONE(hipEventSynchronize(t->e1));
        SA_HIP_GOTO_DONE(hipEventElapsedTime(&ms1, t->e0, t->e1));
        if (kernel_ms_out) *kernel_ms_out = (double) ms0 + (double) ms1;
    }
done:
    if (rc != SA_OK) {
        (void) hipStreamSynchronize(0);
        if (adding) t->poisoned = true;   // (part of the call may be in the table)
    }
    g_sa_pool.put(SaPool::DEVICE, d);
    return rc;
}

extern "C" int sa_position_profile_add_batch(sa_position_profile_t *t, sa_batch_t *b, const sa_profile_job_map_t *map, int64_t n_jobs,
                                             unsigned flags, double *kernel_ms_out) {
    if (!t || !b || n_jobs < 0 || (n_jobs > 0 && !map) || (flags & ~SA_PROFILE_DIRECT)) return SA_EINVAL;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    SaAccEnter in(t);
    if (in.rc) return in.rc;
    SaBatchView V;
    const int rc = sa_batch_view(b, &V);
    if (V.batch_flags & SA_FLAG_VC_ROWS) return SA_EINVAL;       // (it dropped rows; refused before the batch's state is looked at)
    if (V.p8) return SA_EUNSUPPORTED;                            // (an 8-byte record names no path k-mer)
    if (rc) return rc;
    if (V.batch_flags & SA_FLAG_EXPECT_INTERNAL) return SA_ESTATE;
    if ((int64_t) V.count.size() != n_jobs || V.device != t->device || V.k != t->k || V.n_alpha != t->n_alpha) return SA_EINVAL;
    if (sa_profile_check_map(map, n_jobs, t->n_contigs) != SA_OK) return SA_EINVAL;
    if (hipSetDevice(t->device) != hipSuccess) return SA_ENODEVICE;   // (the view may have bound the batch's, the same one)
    return pf_add(t, (const sa_pair16_t *) V.recs, V, map, flags, kernel_ms_out);
}

extern "C" int sa_position_profile_add_records(sa_position_profile_t *t, const sa_profile_job_map_t *map, int64_t n_jobs, const int64_t *first,
                                               const int32_t *x, const int32_t *kmer_id, const int64_t *prob_e7, unsigned flags,
                                               double *kernel_ms_out) {
    if (!t || (flags & ~SA_PROFILE_DIRECT)) return SA_EINVAL;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (sa_profile_check_map(map, n_jobs, t->n_contigs) != SA_OK) return SA_EINVAL;
    if (sa_profile_check_records(n_jobs, first, x, kmer_id, prob_e7, t->n_kmers) != SA_OK) return SA_EINVAL;
    const size_t n = (size_t) first[n_jobs];
    SaBatchView V;
    V.first.assign(first, first + n_jobs);
    V.count.resize((size_t) n_jobs);
    for (int64_t j = 0; j < n_jobs; j++) V.count[(size_t) j] = first[j + 1] - first[j];
    std::vector<sa_pair16_t> recs(n);
    for (size_t i = 0; i < n; i++) recs[i] = sa_pair16_pack(prob_e7[i], x[i], 0, 0, kmer_id[i]);
    SaAccEnter in(t);
    if (in.rc) return in.rc;
    if (n == 0) return SA_OK;
    int rc = SA_OK;
    sa_pair16_t *d_recs = nullptr;
    if (g_sa_pool.get(SaPool::DEVICE, (void **) &d_recs, sizeof(sa_pair16_t) * n, t->device) != hipSuccess) return SA_ENOMEM;
    SA_HIP_GOTO_DONE(hipMemcpy(d_recs, recs.data(), sizeof(sa_pair16_t) * n, hipMemcpyHostToDevice));
    rc = pf_add(t, d_recs, V, map, flags, kernel_ms_out);
done:
    g_sa_pool.put(SaPool::DEVICE, d_recs);
    return rc;
}

extern "C" int sa_position_profile_checkpoint(sa_position_profile_t *t) { return sa_acc_checkpoint(t); }
extern "C" int sa_position_profile_rollback(sa_position_profile_t *t) { return sa_acc_rollback(t); }

// ---- finish ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SA_ACC_THREADS) void k_pf_block_sums(const int *__restrict__ diff, long long n_slots, long long *__restrict__ blk_sum) {
    __shared__ long long total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const long long g0 = sa_acc_first_slot();
    long long mine = 0;
    for (int q = 0; q < SA_ACC_PER_THREAD; q++)
        if (g0 + q < n_slots) mine += diff[g0 + q];
    if (mine) atomicAdd((unsigned long long *) &total, (unsigned long long) mine);
    __syncthreads();
    if (threadIdx.x == 0) blk_sum[blockIdx.x] = total;
}

// read_count of the thread's SA_ACC_PER_THREAD slots from g0 on: the differences before the block (before), then inside it
__device__ __forceinline__ void pf_read_counts(const int *__restrict__ diff, long long n_slots, long long g0, long long before, long long *rc) {
    long long mine = 0;
    for (int q = 0; q < SA_ACC_PER_THREAD; q++)
        if (g0 + q < n_slots) mine += diff[g0 + q];
    long long run = sa_acc_place(mine, before);
    for (int q = 0; q < SA_ACC_PER_THREAD; q++) {
        if (g0 + q < n_slots) run += diff[g0 + q];
        rc[q] = run;
    }
    __syncthreads();
}

__global__ __launch_bounds__(SA_ACC_THREADS) void k_pf_mark(const int *__restrict__ diff, const unsigned long long *__restrict__ acc, int S,
                                                           long long n_slots, const long long *__restrict__ blk_before,
                                                           long long *__restrict__ blk_cnt) {
    const long long g0 = sa_acc_first_slot();
    long long rc[SA_ACC_PER_THREAD];
    pf_read_counts(diff, n_slots, g0, blk_before[blockIdx.x], rc);
    sa_acc_block_count(sa_acc_count(g0, n_slots, [&](long long g, int q) { return rc[q] > 0 || acc[(size_t) g * S] > 0; }), blk_cnt);
}

__global__ __launch_bounds__(SA_ACC_THREADS) void k_pf_emit(const int *__restrict__ diff, const unsigned long long *__restrict__ acc, int S,
                                                           int n_alpha, long long n_slots, const long long *__restrict__ blk_before,
                                                           const long long *__restrict__ blk_off, const long long *__restrict__ coff,
                                                           int n_contigs, const char *__restrict__ ref, sa_profile_site_t *__restrict__ out) {
    const long long g0 = sa_acc_first_slot();
    long long rc[SA_ACC_PER_THREAD];
    pf_read_counts(diff, n_slots, g0, blk_before[blockIdx.x], rc);
    const int mine = sa_acc_count(g0, n_slots, [&](long long g, int q) { return rc[q] > 0 || acc[(size_t) g * S] > 0; });
    long long w = sa_acc_place(mine, blk_off[blockIdx.x]);
    for (int q = 0; q < SA_ACC_PER_THREAD && mine; q++) {
        const long long g = g0 + q;
        if (g >= n_slots) continue;
        const unsigned long long *a = acc + (size_t) g * S;
        const long long kc = (long long) a[0], eu = (long long) a[1];
        if (!(rc[q] > 0 || kc > 0)) continue;
        const int c = sa_acc_contig_of(coff, n_contigs, g);
        sa_profile_site_t o;
        o.pos = g - coff[c];
        o.contig = c;
        o.read_count = (int32_t) rc[q];
        o.kmer_count = kc;
        o.entropy_units = eu;
        long long total = 0;
        for (int l = 0; l < SA_SITE_MAX_LETTERS; l++) {
            o.units[l] = l < n_alpha ? (long long) a[2 + l] : 0;
            total += o.units[l];
        }
        for (int l = 0; l < SA_SITE_MAX_LETTERS; l++) o.prob[l] = total > 0 ? (double) o.units[l] / (double) total : 0.0;
        o.entropy = eu == 0 ? 0.0 : ((double) eu * 9.094947017729282e-13 / (double) kc) / -2.0;   // (2^-40)
        o.ref = kc > 0 ? sa_acc_ref_letter(ref, g) : (char) 0;
        for (int q2 = 0; q2 < 7; q2++) o.pad[q2] = 0;
        out[w++] = o;
    }
}

extern "C" int sa_position_profile_finish(sa_position_profile_t *t, const char *const *ref_by_contig, sa_profile_site_t **sites_out,
                                          int64_t *n_out, uint32_t *letters_seen_out, double *kernel_ms_out) {
    if (letters_seen_out) *letters_seen_out = 0;
    if (const int rc = sa_acc_finish_args(t, ref_by_contig, sites_out, n_out, kernel_ms_out)) return rc;
    SaAccEnter in(t);
    if (in.rc) return in.rc;
    unsigned seen = 0;
    if (hipMemcpy(&seen, t->seen(), 4, hipMemcpyDeviceToHost) != hipSuccess) return SA_ENODEVICE;
    const size_t nb = sa_acc_blocks(t), o_before = sa_up256(8 * nb);   // the call's own scratch: [block sums | sums before each block]
    const int *diff = t->diff();
    const unsigned long long *acc = t->acc();
    const int rc = sa_acc_finish(
        t, ref_by_contig, o_before + 8 * (nb + 1),
        [&](unsigned grid, char *own, long long *blk_cnt) {
            long long *blk_sum = (long long *) own, *blk_before = (long long *) (own + o_before);
            hipLaunchKernelGGL(k_pf_block_sums, dim3(grid), dim3(SA_ACC_THREADS), 0, 0, diff, t->n_slots, blk_sum);
            hipLaunchKernelGGL(k_acc_scan, dim3(1), dim3(SA_SCAN_THREADS), 0, 0, (const long long *) blk_sum, blk_before, (long long) grid);
            hipLaunchKernelGGL(k_pf_mark, dim3(grid), dim3(SA_ACC_THREADS), 0, 0, diff, acc, t->S, t->n_slots, (const long long *) blk_before, blk_cnt);
        },
        [&](unsigned grid, char *own, const long long *blk_off, const char *ref, sa_profile_site_t *d_out) {
            hipLaunchKernelGGL(k_pf_emit, dim3(grid), dim3(SA_ACC_THREADS), 0, 0, diff, acc, t->S, t->n_alpha, t->n_slots,
                               (const long long *) (own + o_before), blk_off, (const long long *) t->d_coff, (int) t->n_contigs, ref, d_out);
        },
        sites_out, n_out, kernel_ms_out);
    if (rc == SA_OK && letters_seen_out) *letters_seen_out = seen;
    return rc;
}
