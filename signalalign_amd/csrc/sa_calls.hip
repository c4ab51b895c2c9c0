// Per-site variant / methylation calls on gfx950 -- MarginalizeFullVariants.get_data (src/signalalign/variantCaller.py:92-187),
// chained onto a finished batch as sa_batch_mea is: the pairs are read where sa_batch_run left them in HBM and only the calls
// come back.
//
// A site is a k-mer index x whose last letter is an ambiguity letter; its call sums, per letter l of that ambiguity letter, the
// printed posterior of the pairs at x whose path k-mer ends in l, and normalises over the letters.  The sums are integers of
// 1e-6 (sa_printed_units): exact, so the result does not depend on the order in which the pairs arrive.
//
// Tables (built on the host at sa_batch_create, uploaded on the first call): one bit per k-mer index of every job, set at a
// site, and per 64-bit word the index of its first site -- a pair finds its site slot with one word, one prefix and a popcount.
// Per site its x and its kind (which ambiguity letter), per kind and alphabet digit the letter's index (-1: not a letter of it).
//
// Kernels:
//   k_site_accum    one thread per 16-byte record, blocks over chunks of a job's records: unpack x, kmer_id, prob_e7; bit test;
//                   one 64-bit integer atomic add into units[site * stride + letter].  Reads 16 B per record, writes nothing else.
//   k_site_final    one wave per job: totals, probabilities (in place beside the units), kept sites counted by ballot
//   k_site_scan     one block of 1024 threads: exclusive scan of the per-job counts
//   k_site_compact  one wave per job: the kept sites written, in x order, to the job's place in the compact output
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "sa_internal.h"
#include "sa_chain.h"

// The table of a batch's ambiguity letters, shared by the site calls and the position calls (sa_chain.h)
struct SaAmbigTab {
    int n_alpha = 0, k = 0, stride = 0;                // stride: most letters of any kind in the batch
    long long n_sites = 0;
    std::vector<long long> site_off;                   // n_jobs + 1: job j's sites are [site_off[j], site_off[j + 1])
    std::vector<long long> word_off;                   // n_jobs + 1: job j's bitmap words
    std::vector<unsigned long long> bits;              // bit i of job j: i is a site
    std::vector<int> pre;                              // per word: global index of the first site at or after its first bit
    std::vector<int> x;                                // per site: its index i
    std::vector<unsigned char> kind;                   // per site
    std::vector<std::string> letters;                  // per kind: distinct options, sorted
    std::vector<signed char> slot;                     // kind * n_alpha + digit: index into letters[kind], -1 none
    // device copy of the tables, one block from the caching allocator: [bits | pre | word_off | site_off | kind | nl | slot]
    char *d = nullptr;
    int device = -1;
    size_t o_pre = 0, o_woff = 0, o_soff = 0, o_kind = 0, o_nl = 0, o_slot = 0;
};

static int ambig_tab_build(SaAmbigTab *S, const sa_model_t *m, const sa_job_t *jobs, int64_t n_jobs, const char *const *ambig, int tail) {
    S->n_alpha = m->n_alpha;
    S->k = m->k;
    int kind_of[256];
    for (int c = 0; c < 256; c++) kind_of[c] = -1;
    S->site_off.assign((size_t) n_jobs + 1, 0);
    S->word_off.assign((size_t) n_jobs + 1, 0);
    for (int64_t j = 0; j < n_jobs; j++) {
        const long long lx = jobs[j].ref_len - tail;
        S->word_off[(size_t) j + 1] = S->word_off[(size_t) j] + (lx > 0 ? (lx + 63) / 64 : 0);
    }
    S->bits.assign((size_t) S->word_off[(size_t) n_jobs], 0ull);
    S->pre.assign(S->bits.size(), 0);
    for (int64_t j = 0; j < n_jobs; j++) {
        const char *ref = jobs[j].ref;
        const long long lx = jobs[j].ref_len - tail;
        const long long w0 = S->word_off[(size_t) j];
        for (long long x = 0; x < lx; x++) {
            if ((x & 63) == 0) S->pre[(size_t) (w0 + (x >> 6))] = (int) S->x.size();
            const unsigned char c = (unsigned char) ref[x + tail];
            const char *opts = ambig ? ambig[c] : nullptr;
            if (!opts) continue;
            if (kind_of[c] < 0) {
                std::string l(opts);
                std::sort(l.begin(), l.end());
                l.erase(std::unique(l.begin(), l.end()), l.end());
                if (l.size() > SA_SITE_MAX_LETTERS || S->letters.size() >= 256) return SA_EUNSUPPORTED;
                kind_of[c] = (int) S->letters.size();
                S->letters.push_back(l);
                S->stride = std::max(S->stride, (int) l.size());
            }
            S->bits[(size_t) (w0 + (x >> 6))] |= 1ull << (x & 63);
            S->x.push_back((int) x);
            S->kind.push_back((unsigned char) kind_of[c]);
            if (S->x.size() >= (size_t) INT32_MAX) return SA_EUNSUPPORTED;
        }
        S->site_off[(size_t) j + 1] = (long long) S->x.size();
    }
    S->n_sites = (long long) S->x.size();
    S->slot.assign(S->letters.size() * (size_t) S->n_alpha, (signed char) -1);
    for (size_t kd = 0; kd < S->letters.size(); kd++)
        for (size_t i = 0; i < S->letters[kd].size(); i++)
            for (int a = 0; a < S->n_alpha; a++)
                if (m->alphabet[a] == S->letters[kd][i]) S->slot[kd * (size_t) S->n_alpha + (size_t) a] = (signed char) i;
    return SA_OK;
}

int sa_ambig_build(const sa_model_t *m, const sa_job_t *jobs, int64_t n_jobs, const char *const *ambig, int tail, SaAmbigTab **out) {
    *out = nullptr;
    SaAmbigTab *S = new (std::nothrow) SaAmbigTab();
    if (!S) return SA_ENOMEM;
    const int rc = ambig_tab_build(S, m, jobs, n_jobs, ambig, tail);
    if (rc != SA_OK) { delete S; return rc; }
    *out = S;
    return SA_OK;
}

long long sa_ambig_count(const SaAmbigTab *s) { return s ? s->n_sites : 0; }
void sa_ambig_release_device(SaAmbigTab *s) {
    if (!s || !s->d) return;
    g_sa_pool.put(SaPool::DEVICE, s->d);
    s->d = nullptr;
    s->device = -1;
}
void sa_ambig_free(SaAmbigTab *s) {
    sa_ambig_release_device(s);
    delete s;
}

struct SiteTabs {
    const unsigned long long *bits;
    const int *pre;
    const long long *word_off, *site_off;
    const unsigned char *kind;
    const int *nl;            // per kind: number of letters
    const signed char *slot;
    int n_alpha, k, stride;
};
static SiteTabs sites_tabs(const SaAmbigTab *S) {
    SiteTabs T;
    T.bits = (const unsigned long long *) S->d;
    T.pre = (const int *) (S->d + S->o_pre);
    T.word_off = (const long long *) (S->d + S->o_woff);
    T.site_off = (const long long *) (S->d + S->o_soff);
    T.kind = (const unsigned char *) (S->d + S->o_kind);
    T.nl = (const int *) (S->d + S->o_nl);
    T.slot = (const signed char *) (S->d + S->o_slot);
    T.n_alpha = S->n_alpha;
    T.k = S->k;
    T.stride = S->stride;
    return T;
}

static int sites_upload(SaAmbigTab *S, int device) {
    if (S->d && S->device == device) return SA_OK;
    sa_ambig_release_device(S);
    const size_t nw = S->bits.size(), nj1 = S->word_off.size(), ns = (size_t) S->n_sites, nk = S->letters.size();
    std::vector<int> nl(nk);
    for (size_t kd = 0; kd < nk; kd++) nl[kd] = (int) S->letters[kd].size();
    SaLayout L;
    L.add(8 * nw);   // (the bitmap, at 0)
    S->o_pre = L.add(4 * nw);
    S->o_woff = L.add(8 * nj1);
    S->o_soff = L.add(8 * nj1);
    S->o_kind = L.add(ns);
    S->o_nl = L.add(4 * nk);
    S->o_slot = L.add(S->slot.size() + 1);
    const size_t bytes = L.end;
    if (g_sa_pool.get(SaPool::DEVICE, (void **) &S->d, bytes, device) != hipSuccess) { S->d = nullptr; return SA_ENOMEM; }
    S->device = device;
    const struct { size_t off; const void *src; size_t n; } up[] = {
        {0, S->bits.data(), 8 * nw}, {S->o_pre, S->pre.data(), 4 * nw}, {S->o_woff, S->word_off.data(), 8 * nj1},
        {S->o_soff, S->site_off.data(), 8 * nj1}, {S->o_kind, S->kind.data(), ns}, {S->o_nl, nl.data(), 4 * nk},
        {S->o_slot, S->slot.data(), S->slot.size()}};
    for (const auto &u : up)
        if (u.n && hipMemcpy(S->d + u.off, u.src, u.n, hipMemcpyHostToDevice) != hipSuccess) {
            sa_ambig_release_device(S);
            return SA_ENODEVICE;
        }
    return SA_OK;
}

// units[site * stride + letter] += printed units of every record of the chunk that sits at a site
__global__ __launch_bounds__(256) void k_site_accum(const sa_pair16_t *__restrict__ pairs, const SaRecChunk *__restrict__ chunks,
                                                    SiteTabs T, unsigned long long *__restrict__ units) {
    const SaRecChunk C = chunks[blockIdx.x];
    const long long w0 = T.word_off[C.job], w1 = T.word_off[C.job + 1];
    for (int i = threadIdx.x; i < C.n; i += blockDim.x) {
        const sa_pair16_t r = pairs[C.first + i];
        const long long x = (long long) (r.a & 0xfffffffull);
        const long long w = w0 + (x >> 6);
        if (w >= w1) continue;   // (x beyond the job's k-mers: not a record of this job's matrix; cannot happen)
        const unsigned long long word = T.bits[w];
        if (!((word >> (x & 63)) & 1ull)) continue;
        const int site = T.pre[w] + __popcll(word & ((1ull << (x & 63)) - 1ull));
        const unsigned kmer_id = (unsigned) (r.b & 0xffffffffull);
        const int l = T.slot[(int) T.kind[site] * T.n_alpha + (int) (kmer_id % (unsigned) T.n_alpha)];
        if (l < 0) continue;
        const long long u = sa_printed_units((long long) ((r.b >> 32) & 0xffffffull));
        if (u) atomicAdd(&units[(size_t) site * (size_t) T.stride + (size_t) l], (unsigned long long) u);
    }
}

// job blockIdx.x: every site's total and probabilities; count[j] = its sites with a non-zero total
__global__ __launch_bounds__(64) void k_site_final(SiteTabs T, const unsigned long long *__restrict__ units, double *__restrict__ prob,
                                                   int *__restrict__ count) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const long long s0 = T.site_off[j], s1 = T.site_off[j + 1];
    int kept = 0;
    for (long long base = s0; base < s1; base += 64) {
        const long long s = base + lane;
        bool keep = false;
        if (s < s1) {
            const int nl = T.nl[T.kind[s]];
            const unsigned long long *u = units + (size_t) s * (size_t) T.stride;
            unsigned long long tot = 0;
            for (int l = 0; l < nl; l++) tot += u[l];
            keep = tot != 0;
            double *p = prob + (size_t) s * (size_t) T.stride;
            for (int l = 0; l < nl; l++) p[l] = keep ? (double) u[l] / (double) tot : 0.0;
        }
        kept += __popcll(__ballot(keep));
    }
    if (lane == 0) count[j] = kept;
}

// exclusive scan of count[0 .. n) into off[0 .. n], one block
__global__ __launch_bounds__(SA_SCAN_THREADS) void k_site_scan(const int *__restrict__ count, long long *__restrict__ off, int n) {
    sa_block_excl_scan([count](int i) { return (long long) count[i]; }, off, n);
}

// job blockIdx.x: its kept sites, in x order, from off[j] on -- site index, units and probabilities (stride per site)
__global__ __launch_bounds__(64) void k_site_compact(SiteTabs T, const unsigned long long *__restrict__ units, const double *__restrict__ prob,
                                                     const long long *__restrict__ off, int *__restrict__ o_site,
                                                     unsigned long long *__restrict__ o_units, double *__restrict__ o_prob) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const long long s0 = T.site_off[j], s1 = T.site_off[j + 1];
    const size_t st = (size_t) T.stride;
    long long w = off[j];
    for (long long base = s0; base < s1; base += 64) {
        const long long s = base + lane;
        bool keep = false;
        int nl = 0;
        if (s < s1) {
            nl = T.nl[T.kind[s]];
            for (int l = 0; l < nl; l++) keep = keep || units[(size_t) s * st + (size_t) l] != 0;
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const size_t dst = (size_t) (w + __popcll(mask & ((1ull << lane) - 1ull)));
            o_site[dst] = (int) s;
            for (int l = 0; l < nl; l++) {
                o_units[dst * st + (size_t) l] = units[(size_t) s * st + (size_t) l];
                o_prob[dst * st + (size_t) l] = prob[(size_t) s * st + (size_t) l];
            }
        }
        w += __popcll(mask);
    }
}

// the timing events and the lock around them; the call's device and pinned storage comes from the caching allocator and goes
// back to it at the end of the call (sa_pool_release / the pool's bounds reach it)
static SaScratch g_site_ws;

// the records of a call that brings its own (sa_*_calls_records), up into a block of the caching allocator; the caller holds
// the scratch's lock and has bound it to `device`
static int fold_records_upload(const std::vector<sa_pair16_t> &recs, int device, char **d_recs) {
    const size_t bytes = sizeof(sa_pair16_t) * recs.size();
    if (g_sa_pool.get(SaPool::DEVICE, (void **) d_recs, bytes, device) != hipSuccess) { *d_recs = nullptr; return SA_ENOMEM; }
    if (bytes && hipMemcpy(*d_recs, recs.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return SA_ENODEVICE;
    return SA_OK;
}

// what the table alone says of a site fold: the host half of SaSiteFold
static void site_fold_init(const SaAmbigTab *S, size_t nj, SaSiteFold *F) {
    F->nj = nj;
    F->stride = (size_t) S->stride;
    F->ns = (size_t) S->n_sites;
    F->kernel_ms = 0.0;
    F->h_x = S->x.data();
    F->h_site_off = S->site_off.data();
    F->letters = S->letters;
}

// The site fold of table S (n_sites > 0) over the 16-byte records of view V: V.recs on V.device, or -- h_recs -- the host
// records that go up first.  What sa_site_fold_run promises of the lock and the timed region holds here.
static int site_fold_records(SaAmbigTab *S, const SaBatchView &V, const std::vector<sa_pair16_t> *h_recs, SaSiteFold *F) {
    int rc = SA_OK;
    const size_t nj = F->nj, stride = F->stride, ns = F->ns;
    const sa_pair16_t *d_pairs = (const sa_pair16_t *) V.recs;
    const int device = F->device = V.device;
    const std::vector<SaRecChunk> chunks = sa_view_chunks(V, SA_CHAIN_CHUNK, SA_ORDINAL_PER_JOB);   // (ordinals unused)
    const size_t nc = chunks.size();
    SaLayout L;   // device: [units | prob | chunks | count]
    const size_t o_units = L.add(8 * ns * stride), o_prob = L.add(8 * ns * stride), o_chunks = L.add(sizeof(SaRecChunk) * nc),
                 o_count = L.add(4 * nj);
    SaScratch &W = g_site_ws;
    F->ws = &W;
    F->guard = std::unique_lock<std::mutex>(W.mu);
    char *&d = F->d;
    SiteTabs T;
    if ((rc = W.rebind(device)) != SA_OK || (rc = sites_upload(S, device)) != SA_OK) return rc;
    if (h_recs) {
        if ((rc = fold_records_upload(*h_recs, device, &F->d_recs)) != SA_OK) return rc;
        d_pairs = (const sa_pair16_t *) F->d_recs;
    }
    if (g_sa_pool.get(SaPool::DEVICE, (void **) &d, L.end, device) != hipSuccess) { d = nullptr; return SA_ENOMEM; }
    T = sites_tabs(S);
    if (nc) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_chunks, chunks.data(), sizeof(SaRecChunk) * nc, hipMemcpyHostToDevice, 0));
    SA_HIP_GOTO_DONE(hipMemsetAsync(d + o_units, 0, 8 * ns * stride, 0));
    SA_HIP_GOTO_DONE(W.time_begin());
    if (nc) hipLaunchKernelGGL(k_site_accum, dim3((unsigned) nc), dim3(256), 0, 0, d_pairs, (const SaRecChunk *) (d + o_chunks), T,
                               (unsigned long long *) (d + o_units));
    hipLaunchKernelGGL(k_site_final, dim3((unsigned) nj), dim3(64), 0, 0, T, (const unsigned long long *) (d + o_units),
                       (double *) (d + o_prob), (int *) (d + o_count));
    F->units = (const unsigned long long *) (d + o_units);
    F->prob = (const double *) (d + o_prob);
    F->count = (const int *) (d + o_count);
    F->site_off = T.site_off;
    F->kind = T.kind;
done:
    return rc;
}

// the accumulate-and-normalise half of the site calls of a finished batch, left on the device (SaSiteFold, sa_chain.h)
int sa_site_fold_run(sa_batch_t *b, SaSiteFold *F) {
    SaAmbigTab *S = nullptr;
    int64_t nj64 = 0;
    int rc = sa_batch_ambig(b, SA_TAB_SITES, &S, &nj64);
    if (rc) return rc;
    site_fold_init(S, (size_t) nj64, F);
    if (F->ns == 0) return SA_OK;   // (a batch without sites -- a SA_FLAG_PAIRS8 one among them -- has nothing to read on the device)
    SaBatchView V;
    if ((rc = sa_batch_view(b, &V)) != SA_OK) return rc;
    if (V.p8 || (V.batch_flags & SA_FLAG_VC_ROWS)) return SA_ESTATE;   // (such records name no k-mer / are not all the rows)
    return site_fold_records(S, V, nullptr, F);
}

void sa_site_fold_release(SaSiteFold *F, bool failed) {
    if (failed && (F->d || F->d_recs)) (void) hipStreamSynchronize(0);   // (a failed call may have left work queued on its blocks)
    if (F->d) g_sa_pool.put(SaPool::DEVICE, F->d);
    if (F->d_recs) g_sa_pool.put(SaPool::DEVICE, F->d_recs);
    F->d = F->d_recs = nullptr;
    if (F->guard.owns_lock()) F->guard.unlock();
}

// The second half of the site calls: fold F of table S (run, when the table has sites) compacted and copied out into the
// cleared calls_out / n_out, one entry per job; the fold is released.
static int site_calls_out(const SaAmbigTab *S, SaSiteFold &F, sa_site_call_t **calls_out, int64_t *n_out, double *kernel_ms_out) {
    int rc = SA_OK;
    const size_t nj = F.nj, stride = (size_t) S->stride, ns = (size_t) S->n_sites;
    std::vector<long long> h_off(nj + 1, 0);
    const int *h_site = nullptr;
    const unsigned long long *h_units = nullptr;
    const double *h_prob = nullptr;
    char *d = nullptr, *h = nullptr;   // this call's device and pinned blocks (g_sa_pool), beside the fold's
    if (ns > 0) {
        SaScratch &W = *F.ws;
        const int device = F.device;
        const SiteTabs T = sites_tabs(S);
        SaLayout L;   // device: [off | out site | out units | out prob]
        const size_t o_off = L.add(8 * (nj + 1)), o_osite = L.add(4 * ns), o_ounits = L.add(8 * ns * stride),
                     o_oprob = L.add(8 * ns * stride), dev_bytes = L.end;
        float kms = 0;
        size_t n_kept = 0, o_hunits = 0, o_hprob = 0;
        if (g_sa_pool.get(SaPool::DEVICE, (void **) &d, dev_bytes, device) != hipSuccess) { d = nullptr; rc = SA_ENOMEM; goto done; }
        hipLaunchKernelGGL(k_site_scan, dim3(1), dim3(SA_SCAN_THREADS), 0, 0, F.count, (long long *) (d + o_off), (int) nj);
        hipLaunchKernelGGL(k_site_compact, dim3((unsigned) nj), dim3(64), 0, 0, T, F.units, F.prob, (const long long *) (d + o_off),
                           (int *) (d + o_osite), (unsigned long long *) (d + o_ounits), (double *) (d + o_oprob));
        SA_HIP_GOTO_DONE(W.time_end());
        SA_HIP_GOTO_DONE(hipMemcpy(h_off.data(), d + o_off, 8 * (nj + 1), hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(W.time_ms(&kms));
        if (kernel_ms_out) *kernel_ms_out = (double) kms;
        // only the kept calls cross PCIe
        n_kept = (size_t) h_off[nj];
        o_hunits = sa_up256(4 * n_kept);
        o_hprob = o_hunits + 8 * n_kept * stride;
        if (g_sa_pool.get(SaPool::PINNED, (void **) &h, o_hprob + 8 * n_kept * stride + 256, device) != hipSuccess) {
            h = nullptr;
            rc = SA_ENOMEM;
            goto done;
        }
        if (n_kept) {
            SA_HIP_GOTO_DONE(hipMemcpyAsync(h, d + o_osite, 4 * n_kept, hipMemcpyDeviceToHost, 0));
            SA_HIP_GOTO_DONE(hipMemcpyAsync(h + o_hunits, d + o_ounits, 8 * n_kept * stride, hipMemcpyDeviceToHost, 0));
            SA_HIP_GOTO_DONE(hipMemcpyAsync(h + o_hprob, d + o_oprob, 8 * n_kept * stride, hipMemcpyDeviceToHost, 0));
            SA_HIP_GOTO_DONE(hipStreamSynchronize(0));
        }
        h_site = (const int *) h;
        h_units = (const unsigned long long *) (h + o_hunits);
        h_prob = (const double *) (h + o_hprob);
    }
    {
        std::atomic<bool> oom(false);
        sa_parallel_for(nj, [&](size_t j) {
            const long long a = h_off[j], n = h_off[j + 1] - h_off[j];
            n_out[j] = n;
            calls_out[j] = (sa_site_call_t *) calloc((size_t) (n > 0 ? n : 1), sizeof(sa_site_call_t));
            if (!calls_out[j]) { oom = true; return; }
            for (long long i = 0; i < n; i++) {
                sa_site_call_t &c = calls_out[j][i];
                const size_t s = (size_t) h_site[a + i], r = (size_t) (a + i) * stride;
                const std::string &l = S->letters[S->kind[s]];
                c.x = S->x[s];
                c.n_letters = (int32_t) l.size();
                memcpy(c.letters, l.data(), l.size());
                for (size_t q = 0; q < l.size(); q++) {
                    c.units[q] = (int64_t) h_units[r + q];
                    c.prob[q] = h_prob[r + q];
                }
            }
        });
        if (oom) rc = SA_ENOMEM;
    }
done:
    if (rc != SA_OK && (d || F.d)) (void) hipStreamSynchronize(0);   // (a failed call may have left work queued on its blocks)
    if (d) g_sa_pool.put(SaPool::DEVICE, d);   // (every kernel and copy of the call has completed: synchronous copies above)
    if (h) g_sa_pool.put(SaPool::PINNED, h);
    sa_site_fold_release(&F, false);
    if (rc != SA_OK)
        for (size_t j = 0; j < nj; j++) { free(calls_out[j]); calls_out[j] = nullptr; n_out[j] = 0; }
    return rc;
}

extern "C" int sa_batch_site_calls(sa_batch_t *b, unsigned flags, sa_site_call_t **calls_out, int64_t *n_out, double *kernel_ms_out) {
    (void) flags;
    if (!b || !calls_out || !n_out) return SA_EINVAL;
    SaAmbigTab *S = nullptr;
    int64_t nj64 = 0;
    int rc = sa_batch_ambig(b, SA_TAB_SITES, &S, &nj64);
    if (rc) return rc;
    for (int64_t j = 0; j < nj64; j++) { calls_out[j] = nullptr; n_out[j] = 0; }
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    SaSiteFold F;
    if ((rc = sa_site_fold_run(b, &F)) != SA_OK) { sa_site_fold_release(&F, true); return rc; }
    return site_calls_out(S, F, calls_out, n_out, kernel_ms_out);
}

// What sa_site_calls_records and sa_position_calls_records check before the device, and the records packed as a batch leaves
// them: job j's are first[j] .. first[j + 1), each with x a k-mer index of the job's reference.  The view gets the jobs' ranges.
static int calls_records_pack(const sa_model_t *m, const sa_job_t *jobs, int64_t n_jobs, const int64_t *first, const int32_t *x,
                              const int32_t *kmer_id, const int64_t *prob_e7, std::vector<sa_pair16_t> *recs, SaBatchView *V) {
    if (!m || n_jobs < 0 || (n_jobs > 0 && !jobs) || !first || first[0] != 0) return SA_EINVAL;
    for (int64_t j = 0; j < n_jobs; j++)
        if (first[j + 1] < first[j] || jobs[j].ref_len < 0 || (jobs[j].ref_len > 0 && !jobs[j].ref)) return SA_EINVAL;
    const int64_t n = first[n_jobs];
    if (n > 0 && (!x || !kmer_id || !prob_e7)) return SA_EINVAL;
    for (int64_t j = 0; j < n_jobs; j++) {
        const int64_t lx = jobs[j].ref_len - (m->k - 1);   // the job's k-mers
        if (lx > SA_PAIR16_MAX_COORD) return SA_EUNSUPPORTED;   // (as the planners refuse such a matrix)
        for (int64_t i = first[j]; i < first[j + 1]; i++)
            if (x[i] < 0 || x[i] >= lx || kmer_id[i] < 0 || kmer_id[i] >= m->n_kmers || prob_e7[i] < 0 || prob_e7[i] > (int64_t) SA_PROB_1)
                return SA_EINVAL;
    }
    try {   // (every record is valid: only now is there anything to hold them)
        recs->resize((size_t) n);
        V->first.assign(first, first + n_jobs);
        V->count.resize((size_t) n_jobs);
    } catch (const std::bad_alloc &) {
        return SA_ENOMEM;
    }
    for (int64_t i = 0; i < n; i++) (*recs)[(size_t) i] = sa_pair16_pack(prob_e7[i], x[i], 0, 0, kmer_id[i]);
    for (int64_t j = 0; j < n_jobs; j++) V->count[(size_t) j] = first[j + 1] - first[j];
    V->k = m->k;
    V->n_alpha = m->n_alpha;
    return SA_OK;
}

extern "C" int sa_site_calls_records(const sa_model_t *m, const sa_job_t *jobs, int64_t n_jobs, const char *const *ambig, const int64_t *first,
                                     const int32_t *x, const int32_t *kmer_id, const int64_t *prob_e7, int device,
                                     sa_site_call_t **calls_out, int64_t *n_out, double *kernel_ms_out) {
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (!calls_out || !n_out) return SA_EINVAL;
    std::vector<sa_pair16_t> recs;
    SaBatchView V;
    int rc = calls_records_pack(m, jobs, n_jobs, first, x, kmer_id, prob_e7, &recs, &V);
    if (rc) return rc;
    SaAmbigTab *S = nullptr;
    if ((rc = sa_ambig_build(m, jobs, n_jobs, ambig, m->k - 1, &S)) != SA_OK) return rc;
    for (int64_t j = 0; j < n_jobs; j++) { calls_out[j] = nullptr; n_out[j] = 0; }
    SaSiteFold F;
    site_fold_init(S, (size_t) n_jobs, &F);
    if (F.ns > 0) {   // (as for a batch, a call without sites has nothing to do on the device)
        V.device = device;
        if ((rc = sa_device_check(device)) == SA_OK) rc = site_fold_records(S, V, &recs, &F);
    }
    if (rc != SA_OK) sa_site_fold_release(&F, true);
    else rc = site_calls_out(S, F, calls_out, n_out, kernel_ms_out);
    sa_ambig_free(S);   // (its device copy goes back with it)
    return rc;
}

// ---- Per-position marginals (sa_batch_position_calls): CallMethylation.call_methyls (alignmentAnalysisLib.py:159-247) ----
// A position is an index p of a job's reference that holds an ambiguity letter; every record with x <= p <= x + k - 1 adds its
// printed posterior to the letter that its path k-mer has at p.  The reference adds floating-point values serially in TSV row
// order, so the sums are made in that order: the rows of each position are gathered into a bucket, the bucket is put in row
// order and folded by one lane.  A position whose rows all print 0.000000 has total 0, where the reference divides by zero
// (alignmentAnalysisLib.py:230-233): it is reported with its rows, every sum and every probability 0.0.
//
// Tables (built at sa_batch_create with SA_FLAG_POSITION_CALLS): the sites' tables (ambig_tab_build) with tail 0, i.e. one bit
// per reference position of every job, set at an ambiguous one; a "site" of that table is a position, its slot below.
//
// Kernels:
//   k_pos_count     one thread per record: x_min / x_max of the job (wave reduction, one integer atomic per wave); per covered
//                   ambiguous position one integer atomic increment of the slot's row count
//   k_pos_job_scan  one wave per job: exclusive scan of its slots' counts (bucket offsets inside the job), the job's total
//   k_site_scan     the jobs' totals into the jobs' bucket bases
//   k_pos_scatter   one thread per record: per covered ambiguous position one 8-byte entry (row ordinal << 24 | letter << 20 |
//                   printed units) at the slot's next free place (integer atomic)
//   k_pos_fold      one lane per slot: insertion sort of its bucket (the keys are unique: a record has one entry per slot), the
//                   serial fold, total and probabilities; per job the number of non-empty slots
//   k_site_scan     those counts into output offsets
//   k_pos_compact   one wave per job: the non-empty slots in position order
// the digits of kmer_id, first letter first
__device__ static inline void pos_digits(unsigned id, int n_alpha, int k, unsigned char *dig) {
    for (int i = k - 1; i >= 0; i--) {
        dig[i] = (unsigned char) (id % (unsigned) n_alpha);
        id /= (unsigned) n_alpha;
    }
}

// fn(slot, l) for every ambiguous position p = x + d (d ascending) that record r of a job with bitmap words [w0, w1) covers and
// whose letter in r's path k-mer is letter l of the position's kind; the k-mer's digits are made at the first such position
template <class F>
__device__ __forceinline__ void pos_for_each_covered(const SiteTabs &T, long long w0, long long w1, const sa_pair16_t &r, F fn) {
    const int x = (int) (r.a & 0xfffffffull);
    unsigned char dig[SA_POS_MAX_K];
    bool have = false;
    for (int d = 0; d < T.k; d++) {
        const long long p = (long long) x + d, w = w0 + (p >> 6);
        if (w >= w1) break;   // (past the job's reference: cannot happen for a record of its matrix)
        const unsigned long long word = T.bits[w];
        if (!((word >> (p & 63)) & 1ull)) continue;
        if (!have) { pos_digits((unsigned) (r.b & 0xffffffffull), T.n_alpha, T.k, dig); have = true; }
        const int slot = T.pre[w] + __popcll(word & ((1ull << (p & 63)) - 1ull));
        const int l = T.slot[(int) T.kind[slot] * T.n_alpha + (int) dig[d]];
        if (l < 0) continue;
        fn(slot, l);
    }
}

__global__ __launch_bounds__(256) void k_pos_count(const sa_pair16_t *__restrict__ pairs, const SaRecChunk *__restrict__ chunks, SiteTabs T,
                                                   unsigned *__restrict__ cnt, int *__restrict__ xmin, int *__restrict__ xmax) {
    const SaRecChunk C = chunks[blockIdx.x];
    const long long w0 = T.word_off[C.job], w1 = T.word_off[C.job + 1];
    int lo = INT_MAX, hi = -1;
    for (int i = threadIdx.x; i < C.n; i += blockDim.x) {
        const sa_pair16_t r = pairs[C.first + i];
        const int x = (int) (r.a & 0xfffffffull);
        lo = min(lo, x);
        hi = max(hi, x);
        pos_for_each_covered(T, w0, w1, r, [&](int slot, int) { atomicAdd(&cnt[slot], 1u); });
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
    }
    if ((threadIdx.x & 63) == 0 && hi >= 0) {
        atomicMin(&xmin[C.job], lo);
        atomicMax(&xmax[C.job], hi);
    }
}

// job blockIdx.x (one wave): loc[s] = rows of the job's slots before s; tot[j] = the job's rows over all its slots
__global__ __launch_bounds__(64) void k_pos_job_scan(SiteTabs T, const unsigned *__restrict__ cnt, unsigned *__restrict__ loc,
                                                     int *__restrict__ tot) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const long long s0 = T.site_off[j], s1 = T.site_off[j + 1];
    unsigned carry = 0;
    for (long long base = s0; base < s1; base += 64) {
        const long long s = base + lane;
        const unsigned v = s < s1 ? cnt[s] : 0u;
        const unsigned incl = sa_wave_incl_scan(v, lane);
        if (s < s1) loc[s] = carry + incl - v;
        carry += __shfl(incl, 63);
    }
    if (lane == 0) tot[j] = (int) carry;
}

__global__ __launch_bounds__(256) void k_pos_scatter(const sa_pair16_t *__restrict__ pairs, const SaRecChunk *__restrict__ chunks, SiteTabs T,
                                                     const unsigned *__restrict__ loc, const long long *__restrict__ base,
                                                     unsigned *__restrict__ fill, unsigned long long *__restrict__ ent) {
    const SaRecChunk C = chunks[blockIdx.x];
    const long long w0 = T.word_off[C.job], w1 = T.word_off[C.job + 1], b0 = base[C.job];
    for (int i = threadIdx.x; i < C.n; i += blockDim.x) {
        const sa_pair16_t r = pairs[C.first + i];
        pos_for_each_covered(T, w0, w1, r, [&](int slot, int l) {
            const unsigned long long units = (unsigned long long) sa_printed_units((long long) ((r.b >> 32) & 0xffffffull));
            const unsigned q = atomicAdd(&fill[slot], 1u);
            ent[b0 + (long long) loc[slot] + q] = ((unsigned long long) (C.local + i) << 24) | ((unsigned long long) l << 20) | units;
        });
    }
}

// job blockIdx.x: every slot's bucket in row order, folded; kept[j] = the job's slots with rows
__global__ __launch_bounds__(256) void k_pos_fold(SiteTabs T, const unsigned *__restrict__ cnt, const unsigned *__restrict__ loc,
                                                  const long long *__restrict__ base, unsigned long long *__restrict__ ent,
                                                  double *__restrict__ sum, double *__restrict__ prob, int *__restrict__ kept) {
    __shared__ int n_kept;
    const int j = blockIdx.x;
    if (threadIdx.x == 0) n_kept = 0;
    __syncthreads();
    const long long s0 = T.site_off[j], s1 = T.site_off[j + 1];
    for (long long s = s0 + threadIdx.x; s < s1; s += blockDim.x) {
        const unsigned n = cnt[s];
        if (n == 0) continue;
        unsigned long long *e = ent + base[j] + loc[s];
        for (unsigned a = 1; a < n; a++) {   // insertion sort: buckets hold tens of entries
            const unsigned long long v = e[a];
            unsigned b = a;
            while (b > 0 && e[b - 1] > v) { e[b] = e[b - 1]; b--; }
            e[b] = v;
        }
        double acc[SA_SITE_MAX_LETTERS];
        const int nl = T.nl[T.kind[s]];
        for (int l = 0; l < SA_SITE_MAX_LETTERS; l++) acc[l] = 0.0;
        for (unsigned a = 0; a < n; a++) {
            const unsigned long long v = e[a];
            const int l = (int) ((v >> 20) & 0xfull);
            const double u = (double) (long long) (v & 0xfffffull) / 1e6;   // the double "%f" reads back as
#pragma unroll
            for (int q = 0; q < SA_SITE_MAX_LETTERS; q++)
                if (q == l) acc[q] += u;
        }
        double total = 0.0;
        for (int l = 0; l < nl; l++) total += acc[l];
        double *ps = sum + (size_t) s * (size_t) T.stride, *pp = prob + (size_t) s * (size_t) T.stride;
        for (int l = 0; l < nl; l++) {
            ps[l] = acc[l];
            pp[l] = total != 0.0 ? acc[l] / total : 0.0;   // (every row printed 0.000000: the site fold's rule for a zero sum)
        }
        atomicAdd(&n_kept, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) kept[j] = n_kept;
}

// job blockIdx.x: its non-empty slots, in position order, from off[j] on -- slot index, row count, sums and probabilities
__global__ __launch_bounds__(64) void k_pos_compact(SiteTabs T, const unsigned *__restrict__ cnt, const double *__restrict__ sum,
                                                    const double *__restrict__ prob, const long long *__restrict__ off,
                                                    int *__restrict__ o_slot, unsigned *__restrict__ o_n, double *__restrict__ o_sum,
                                                    double *__restrict__ o_prob) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const long long s0 = T.site_off[j], s1 = T.site_off[j + 1];
    const size_t st = (size_t) T.stride;
    long long w = off[j];
    for (long long b = s0; b < s1; b += 64) {
        const long long s = b + lane;
        const bool keep = s < s1 && cnt[s] != 0;
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const size_t dst = (size_t) (w + __popcll(mask & ((1ull << lane) - 1ull)));
            const int nl = T.nl[T.kind[s]];
            o_slot[dst] = (int) s;
            o_n[dst] = cnt[s];
            for (int l = 0; l < nl; l++) {
                o_sum[dst * st + (size_t) l] = sum[(size_t) s * st + (size_t) l];
                o_prob[dst * st + (size_t) l] = prob[(size_t) s * st + (size_t) l];
            }
        }
        w += __popcll(mask);
    }
}

static SaScratch g_pos_ws;

// what the table alone says of a position fold
static void pos_fold_init(SaAmbigTab *P, size_t nj, SaPosFold *F) {
    F->nj = nj;
    F->tab = P;
    F->n_kept = 0;
    F->kernel_ms = 0.0;
    F->h_off.assign(nj + 1, 0);
    F->stride = (size_t) (P->stride > 0 ? P->stride : 1);
}

// The position fold of table P (nj > 0 jobs) over the 16-byte records of view V: V.recs on V.device, or -- h_recs -- the host
// records that go up first.  What sa_pos_fold_run promises of the lock holds here.
static int pos_fold_records(SaAmbigTab *P, const SaBatchView &V, const std::vector<sa_pair16_t> *h_recs, SaPosFold *F) {
    int rc = SA_OK;
    const size_t nj = F->nj, stride = F->stride, ns = (size_t) P->n_sites;
    const sa_pair16_t *d_pairs = (const sa_pair16_t *) V.recs;
    const int device = F->device = V.device;
    F->count = V.count;
    const std::vector<long long> &count = F->count;
    for (size_t j = 0; j < nj; j++)   // (a job's bucket entries, at most k per record, are counted in 32 bits)
        if ((long long) P->k * count[j] >= (long long) INT32_MAX) return SA_EUNSUPPORTED;
    const std::vector<SaRecChunk> chunks = sa_view_chunks(V, SA_CHAIN_CHUNK, SA_ORDINAL_PER_JOB);
    const size_t nc = chunks.size(), ns1 = ns ? ns : 1;
    // device: [cnt, fill | loc | sum | prob | chunks | tot | base | kept | off | xmin | xmax | out slot | out n | out sum |
    // out prob]; cnt and fill are one entry (one memset clears both); the entries in a block of their own, sized once the
    // counts are known
    SaLayout L;
    const size_t o_cnt = L.add(2 * 4 * ns1), o_fill = o_cnt + 4 * ns1, o_loc = L.add(4 * ns1), o_sum = L.add(8 * ns1 * stride),
                 o_prob = L.add(8 * ns1 * stride), o_chunks = L.add(sizeof(SaRecChunk) * nc), o_tot = L.add(4 * nj),
                 o_base = L.add(8 * (nj + 1)), o_kept = L.add(4 * nj), o_off = L.add(8 * (nj + 1)), o_xmin = L.add(4 * nj),
                 o_xmax = L.add(4 * nj), o_oslot = L.add(4 * ns1), o_on = L.add(4 * ns1), o_osum = L.add(8 * ns1 * stride),
                 o_oprob = L.add(8 * ns1 * stride), dev_bytes = L.end;
    std::vector<long long> h_base(nj + 1, 0);
    std::vector<long long> &h_off = F->h_off;
    char *&d = F->d;
    unsigned long long *&d_ent = F->d_ent;
    SaScratch &W = g_pos_ws;
    F->guard = std::unique_lock<std::mutex>(W.mu);
    float kms0 = 0, kms1 = 0;
    SiteTabs T;
    if ((rc = W.rebind(device)) != SA_OK || (rc = sites_upload(P, device)) != SA_OK) return rc;
    if (h_recs) {
        if ((rc = fold_records_upload(*h_recs, device, &F->d_recs)) != SA_OK) return rc;
        d_pairs = (const sa_pair16_t *) F->d_recs;
    }
    if (g_sa_pool.get(SaPool::DEVICE, (void **) &d, dev_bytes, device) != hipSuccess) { d = nullptr; return SA_ENOMEM; }
    T = sites_tabs(P);
    if (nc) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_chunks, chunks.data(), sizeof(SaRecChunk) * nc, hipMemcpyHostToDevice, 0));
    SA_HIP_GOTO_DONE(hipMemsetAsync(d + o_cnt, 0, 2 * 4 * ns1, 0));   // (cnt and fill)
    SA_HIP_GOTO_DONE(hipMemsetAsync(d + o_xmin, 0x7f, 4 * nj, 0));
    SA_HIP_GOTO_DONE(hipMemsetAsync(d + o_xmax, 0xff, 4 * nj, 0));
    SA_HIP_GOTO_DONE(W.time_begin());
    if (nc) hipLaunchKernelGGL(k_pos_count, dim3((unsigned) nc), dim3(256), 0, 0, d_pairs, (const SaRecChunk *) (d + o_chunks), T,
                               (unsigned *) (d + o_cnt), (int *) (d + o_xmin), (int *) (d + o_xmax));
    hipLaunchKernelGGL(k_pos_job_scan, dim3((unsigned) nj), dim3(64), 0, 0, T, (const unsigned *) (d + o_cnt), (unsigned *) (d + o_loc),
                       (int *) (d + o_tot));
    hipLaunchKernelGGL(k_site_scan, dim3(1), dim3(SA_SCAN_THREADS), 0, 0, (const int *) (d + o_tot), (long long *) (d + o_base), (int) nj);
    SA_HIP_GOTO_DONE(W.time_end());
    SA_HIP_GOTO_DONE(hipMemcpy(h_base.data(), d + o_base, 8 * (nj + 1), hipMemcpyDeviceToHost));
    SA_HIP_GOTO_DONE(W.time_ms(&kms0));
    {   // the buckets: 8 bytes per (record, covered ambiguous position)
        const size_t n_ent = (size_t) h_base[nj];
        if (g_sa_pool.get(SaPool::DEVICE, (void **) &d_ent, 8 * (n_ent ? n_ent : 1), device) != hipSuccess) {
            d_ent = nullptr;
            rc = SA_ENOMEM;
            goto done;
        }
    }
    SA_HIP_GOTO_DONE(W.time_begin());
    if (nc) hipLaunchKernelGGL(k_pos_scatter, dim3((unsigned) nc), dim3(256), 0, 0, d_pairs, (const SaRecChunk *) (d + o_chunks), T,
                               (const unsigned *) (d + o_loc), (const long long *) (d + o_base), (unsigned *) (d + o_fill), d_ent);
    hipLaunchKernelGGL(k_pos_fold, dim3((unsigned) nj), dim3(256), 0, 0, T, (const unsigned *) (d + o_cnt), (const unsigned *) (d + o_loc),
                       (const long long *) (d + o_base), d_ent, (double *) (d + o_sum), (double *) (d + o_prob), (int *) (d + o_kept));
    hipLaunchKernelGGL(k_site_scan, dim3(1), dim3(SA_SCAN_THREADS), 0, 0, (const int *) (d + o_kept), (long long *) (d + o_off), (int) nj);
    hipLaunchKernelGGL(k_pos_compact, dim3((unsigned) nj), dim3(64), 0, 0, T, (const unsigned *) (d + o_cnt), (const double *) (d + o_sum),
                       (const double *) (d + o_prob), (const long long *) (d + o_off), (int *) (d + o_oslot), (unsigned *) (d + o_on),
                       (double *) (d + o_osum), (double *) (d + o_oprob));
    SA_HIP_GOTO_DONE(W.time_end());
    SA_HIP_GOTO_DONE(hipMemcpy(h_off.data(), d + o_off, 8 * (nj + 1), hipMemcpyDeviceToHost));
    SA_HIP_GOTO_DONE(W.time_ms(&kms1));
    F->kernel_ms = (double) kms0 + (double) kms1;
    F->n_kept = (size_t) h_off[nj];
    F->off = (const long long *) (d + o_off);
    F->slot = (const int *) (d + o_oslot);
    F->n_rows = (const unsigned *) (d + o_on);
    F->sum = (const double *) (d + o_osum);
    F->prob = (const double *) (d + o_oprob);
    F->xmin = (const int *) (d + o_xmin);
    F->xmax = (const int *) (d + o_xmax);
    F->kind = T.kind;
    F->h_x = P->x.data();
    F->acgt.assign(P->letters.size() * 4, (signed char) -1);
    for (size_t kd = 0; kd < P->letters.size(); kd++)
        for (int l = 0; l < 4; l++) {
            const size_t e = P->letters[kd].find("ACGT"[l]);
            if (e != std::string::npos) F->acgt[kd * 4 + (size_t) l] = (signed char) e;
        }
done:
    return rc;
}

// the position fold of a finished batch, left on the device (SaPosFold, sa_chain.h)
int sa_pos_fold_run(sa_batch_t *b, SaPosFold *F) {
    SaAmbigTab *P = nullptr;
    int64_t nj64 = 0;
    int rc = sa_batch_ambig(b, SA_TAB_POSITIONS, &P, &nj64);
    if (rc) return rc;
    pos_fold_init(P, (size_t) nj64, F);
    if (nj64 == 0) return SA_OK;
    SaBatchView V;
    if ((rc = sa_batch_view(b, &V)) != SA_OK) return rc;
    if (V.p8 || (V.batch_flags & SA_FLAG_VC_ROWS)) return SA_ESTATE;   // (such records name no k-mer / are not all the rows)
    return pos_fold_records(P, V, nullptr, F);
}

void sa_pos_fold_release(SaPosFold *F, bool failed) {
    if (failed && (F->d || F->d_recs)) (void) hipStreamSynchronize(0);   // (a failed call may have left work queued on its blocks)
    if (F->d) g_sa_pool.put(SaPool::DEVICE, F->d);
    if (F->d_ent) g_sa_pool.put(SaPool::DEVICE, F->d_ent);
    if (F->d_recs) g_sa_pool.put(SaPool::DEVICE, F->d_recs);
    F->d = F->d_recs = nullptr;
    F->d_ent = nullptr;
    if (F->guard.owns_lock()) F->guard.unlock();
}

// The second half of the position calls: fold F (of at least one job; fold_rc is what its run returned) copied out into the
// cleared calls_out / n_out, one entry per job; the fold is released.
static int pos_calls_out(SaPosFold &F, int fold_rc, sa_position_call_t **calls_out, int64_t *n_out, int32_t *x_min_out, int32_t *x_max_out,
                         double *kernel_ms_out) {
    int rc = fold_rc;
    const size_t nj = F.nj, stride = F.stride, n_kept = F.n_kept;
    const SaAmbigTab *P = F.tab;
    const std::vector<long long> &count = F.count, &h_off = F.h_off;
    std::vector<int> h_xmin(nj), h_xmax(nj);
    std::vector<int> h_slot;
    std::vector<unsigned> h_cnt;
    std::vector<double> h_sum, h_prob;
    if (rc != SA_OK) goto done;
    if (kernel_ms_out) *kernel_ms_out = F.kernel_ms;
    SA_HIP_GOTO_DONE(hipMemcpy(h_xmin.data(), F.xmin, 4 * nj, hipMemcpyDeviceToHost));
    SA_HIP_GOTO_DONE(hipMemcpy(h_xmax.data(), F.xmax, 4 * nj, hipMemcpyDeviceToHost));
    if (n_kept) {   // only the kept positions cross PCIe
        h_slot.resize(n_kept);
        h_cnt.resize(n_kept);
        h_sum.resize(n_kept * stride);
        h_prob.resize(n_kept * stride);
        SA_HIP_GOTO_DONE(hipMemcpy(h_slot.data(), F.slot, 4 * n_kept, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(hipMemcpy(h_cnt.data(), F.n_rows, 4 * n_kept, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(hipMemcpy(h_sum.data(), F.sum, 8 * n_kept * stride, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(hipMemcpy(h_prob.data(), F.prob, 8 * n_kept * stride, hipMemcpyDeviceToHost));
    }
    for (size_t j = 0; j < nj; j++) {
        const bool any = count[j] > 0;
        if (x_min_out) x_min_out[j] = any ? (int32_t) h_xmin[j] : -1;
        if (x_max_out) x_max_out[j] = any ? (int32_t) h_xmax[j] : -1;
    }
    {
        std::atomic<bool> oom(false);
        sa_parallel_for(nj, [&](size_t j) {
            const long long a = h_off[j], n = h_off[j + 1] - h_off[j];
            n_out[j] = n;
            calls_out[j] = (sa_position_call_t *) calloc((size_t) (n > 0 ? n : 1), sizeof(sa_position_call_t));
            if (!calls_out[j]) { oom = true; return; }
            for (long long i = 0; i < n; i++) {
                sa_position_call_t &c = calls_out[j][i];
                const size_t r = (size_t) (a + i), s = (size_t) h_slot[r];
                const std::string &l = P->letters[P->kind[s]];
                c.p = P->x[s];
                c.n_rows = (int32_t) h_cnt[r];
                c.n_letters = (int32_t) l.size();
                memcpy(c.letters, l.data(), l.size());
                for (size_t q = 0; q < l.size(); q++) {
                    c.sum[q] = h_sum[r * stride + q];
                    c.prob[q] = h_prob[r * stride + q];
                }
            }
        });
        if (oom) rc = SA_ENOMEM;
    }
done:
    sa_pos_fold_release(&F, rc != SA_OK);
    if (rc != SA_OK)
        for (size_t j = 0; j < nj; j++) { free(calls_out[j]); calls_out[j] = nullptr; n_out[j] = 0; }
    return rc;
}

extern "C" int sa_batch_position_calls(sa_batch_t *b, unsigned flags, sa_position_call_t **calls_out, int64_t *n_out,
                                       int32_t *x_min_out, int32_t *x_max_out, double *kernel_ms_out) {
    (void) flags;
    if (!b || !calls_out || !n_out) return SA_EINVAL;
    SaPosFold F;
    {   // (the entries of the outputs are cleared before anything can fail, for a batch whose table exists)
        SaAmbigTab *P0 = nullptr;
        int64_t nj0 = 0;
        const int rc0 = sa_batch_ambig(b, SA_TAB_POSITIONS, &P0, &nj0);
        if (rc0) return rc0;
        for (int64_t j = 0; j < nj0; j++) { calls_out[j] = nullptr; n_out[j] = 0; }
        if (kernel_ms_out) *kernel_ms_out = 0.0;
        if (nj0 == 0) return SA_OK;
    }
    return pos_calls_out(F, sa_pos_fold_run(b, &F), calls_out, n_out, x_min_out, x_max_out, kernel_ms_out);
}

extern "C" int sa_position_calls_records(const sa_model_t *m, const sa_job_t *jobs, int64_t n_jobs, const char *const *ambig,
                                         const int64_t *first, const int32_t *x, const int32_t *kmer_id, const int64_t *prob_e7, int device,
                                         sa_position_call_t **calls_out, int64_t *n_out, int32_t *x_min_out, int32_t *x_max_out,
                                         double *kernel_ms_out) {
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (!calls_out || !n_out) return SA_EINVAL;
    std::vector<sa_pair16_t> recs;
    SaBatchView V;
    int rc = calls_records_pack(m, jobs, n_jobs, first, x, kmer_id, prob_e7, &recs, &V);
    if (rc) return rc;
    SaAmbigTab *P = nullptr;
    if ((rc = m->k > SA_POS_MAX_K ? SA_EUNSUPPORTED : sa_ambig_build(m, jobs, n_jobs, ambig, 0, &P)) != SA_OK) return rc;
    for (int64_t j = 0; j < n_jobs; j++) { calls_out[j] = nullptr; n_out[j] = 0; }
    if (n_jobs > 0 && (rc = sa_device_check(device)) == SA_OK) {
        SaPosFold F;
        pos_fold_init(P, (size_t) n_jobs, &F);
        V.device = device;
        rc = pos_calls_out(F, pos_fold_records(P, V, &recs, &F), calls_out, n_out, x_min_out, x_max_out, kernel_ms_out);
    }
    sa_ambig_free(P);   // (its device copy goes back with it)
    return rc;
}
