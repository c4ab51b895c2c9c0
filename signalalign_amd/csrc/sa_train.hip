// Gaussian k-mer emission training on gfx950 -- trainModels.train_normal_emmissions (src/signalalign/train/trainModels.py:735-828)
// without the assignments files: generate_top_n_kmers_from_sa_output (build_alignments.py:76-275) keeps, per strand and path
// k-mer, the N rows of largest printed posterior among those >= min_prob; the model's event means and SDs are then blended
// with the statistics of those rows.  The rows are read where a finished batch left them in HBM; the kept ones stay in HBM
// across batches (sa_kmer_table_t), and only per-k-mer statistics -- or the rows, when the table file is asked for -- come back.
//
// Selection key of a row: printed posterior (20 bits) << 40 | (2^40 - 1 - run ordinal).  Keys are unique, so "the N largest
// keys of a k-mer" is the reference's top N with ties broken by run order, whatever order the rows arrive in.  It is found by
// radix selection, 10 bits per level from the top: a level histograms the candidates of every k-mer that is not settled yet
// and whose key matches the k-mer's prefix so far, and a cut picks the digit holding the N-th largest key.  Most k-mers settle
// after one or two levels (the posterior alone); only k-mers with more rows tied at the cutoff posterior than they still need
// go on to the run-order levels, which read a copy of those tied rows only.  Candidates are the table's rows (earlier batches)
// and the new batch's records.  The histograms are global (n_kmers x 1024 counters): a block's records spread over all k-mers.
//
// Kernels:
//   k_kt_hist_rows / k_kt_hist_rec<P8>   one thread per row / record: filter, key, one 32-bit integer atomic into
//                                        hist[kmer * 1024 + digit] (16- or 8-byte records; the k-mer of an 8-byte record is the
//                                        job's reference k-mer at x)
//   k_kt_cut                             one wave per k-mer: suffix sums of its 1024 bins, the digit of the N-th largest key
//   k_kt_tie_rows / k_kt_tie_rec<P8>     after the two posterior levels, only if some k-mer is still open: its rows at the cutoff
//                                        posterior into one buffer, which the run-order levels then read instead of all candidates
//   k_kt_scan                            one block of 1024 threads: exclusive scan of the kept counts into the new table's offsets
//   k_kt_compact_rows / _rec<P8>         the rows at or above the k-mer's threshold into the k-mer's segment of the new table;
//                                        for records the descaled mean is computed and rounded as "%f" prints it
//   k_kt_cover / k_kt_cover_count<P8>    a table with positions (trainModels.py:161-286, the rows that cover labelled positions):
//                                        one bit per (job, reference position) from one search of the sorted position keys, which
//                                        the record kernels above test; and per add one pass that counts the offered rows per key
//   k_kt_stats                           one block per k-mer: exact integer sums (S, and Q in two words), radix selection (8 bits
//                                        per pass) of the median and of the median absolute deviation
//   k_kt_mixture<K> / k_kt_mix_gather    one block per (k-mer, K): a K-component Gaussian mixture by EM over the k-mer's rows
//                                        (mixture_model.py:42-186; see the section further down)
//   k_kt_kde<SKIP> / k_kt_kde_gather     one block per (k-mer, tile of 512 query points): the log density of a Gaussian kernel density
//                                        estimate over the k-mer's rows (hiddenMarkovModel.py:654-773; see the section further down)
// Within a k-mer's segment rows lie in arrival order; the keys are unique, so sa_kmer_table_rows sorts them on the host and
// every statistic is independent of the order.  Scratch comes from the library's caching allocator.
#include <hip/hip_runtime.h>

#include <ctype.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "sa_internal.h"
#include "sa_chain.h"

#define KT_BINS 1024                     // 10 bits per selection level
#define KT_RUN_BITS 40
#define KT_RUN_MASK ((1ull << KT_RUN_BITS) - 1ull)
#define KT_UNITS_LIMIT 2147483648.0      // descaled values beyond +-2^31 are refused (their "%f" is not computed here)
#define KT_DESC_LIMIT 2147.483648        // a table row's descaled value is below this in magnitude: |units| <= 2^31 (k_kt_stats squares them)
#define KT_ERR_RANGE 1                   // err word bits
#define KT_ERR_BOUNDS 2

// "%f" of v as glibc prints it: the exact binary value rounded to six decimals, ties to even.  floor(v * 1e6) is found exactly
// with the sign of one fma against an integer (exact in sign), the rounding with the sign against the half point.
__host__ __device__ static inline int kt_f6_units(double v, long long *units, int *neg_zero) {
    if (!(fabs(v) < KT_UNITS_LIMIT)) return SA_EUNSUPPORTED;
    double f = floor(v * 1e6);
    if (fma(v, 1e6, -f) < 0) f -= 1.0;
    else if (fma(v, 1e6, -(f + 1.0)) >= 0) f += 1.0;
    const double d = fma(v, 1e6, -(f + 0.5));
    double r = f;
    if (d > 0) r = f + 1.0;
    else if (d == 0) r = fmod(f, 2.0) == 0 ? f : f + 1.0;
    *units = (long long) r;
    *neg_zero = (signbit(v) && *units == 0) ? 1 : 0;
    return SA_OK;
}
// a row's descaled value: only what k_kt_stats can square in 64 bits is taken into a table
__host__ __device__ static inline int kt_desc_units(double v, long long *units, int *neg_zero) {
    if (!(fabs(v) < KT_DESC_LIMIT)) return SA_EUNSUPPORTED;
    return kt_f6_units(v, units, neg_zero);
}

struct KtRow {                  // a kept row in HBM (24 bytes)
    unsigned long long key;
    long long desc;             // descaled units
    int kmer, neg_zero;
};
struct KtState {                // per k-mer selection state
    unsigned long long prefix, thr;
    long long need, keep;
    int done, pad;
};
struct KtJob {                  // per job of a batch
    long long ev_off, n_ev, x_off, n_x;
    double scale, shift, var;
    // a table with positions (sa_kmer_table_add_batch_at): the job's words of the cover mask, its reference positions, and where
    // they lie: reference_index = x0 + x_sign * x on `contig`, paired with site strand `site_strand`
    long long m_off, m_nx, x0;
    int contig, x_sign, site_strand, pad;
};
struct KtRecs {
    const void *recs;
    const SaRecChunk *chunks;
    const KtJob *jobs;
    const double *ev;           // event means of every job, dense
    const int *xk;              // 8-byte records: k-mer id of every reference position of every job
    const double *level;        // level mean per k-mer
    long long min_units, n_kmers;
    const unsigned long long *mask;   // the cover mask (k_kt_cover), bit x of job j at word jobs[j].m_off; NULL: every row is offered
};

__device__ static inline bool kt_rec(const KtRecs &R, bool p8, const SaRecChunk &C, int i, int *kmer, unsigned long long *key, long long *y,
                                     int *xo, unsigned *err) {
    long long pe7;
    int x;
    if (p8) {
        const sa_pair8_t r = ((const sa_pair8_t *) R.recs)[C.first + i];
        x = (int) (r & 0xfffffull);
        *y = (long long) ((r >> 20) & 0xfffffull);
        pe7 = (long long) (r >> 40);
        const KtJob J = R.jobs[C.job];
        if (x >= J.n_x) { atomicOr(err, KT_ERR_BOUNDS); return false; }
        *kmer = R.xk[J.x_off + x];
    } else {
        const sa_pair16_t r = ((const sa_pair16_t *) R.recs)[C.first + i];
        x = (int) (r.a & 0xfffffffull);
        *y = (long long) ((r.a >> 28) & 0xfffffffull);
        *kmer = (int) (unsigned) (r.b & 0xffffffffull);
        pe7 = (long long) ((r.b >> 32) & 0xffffffull);
    }
    *xo = x;
    if (*kmer < 0 || *kmer >= R.n_kmers) { atomicOr(err, KT_ERR_BOUNDS); return false; }
    const long long u = sa_printed_units(pe7);
    if (u < R.min_units) return false;
    if (R.mask) {   // a table with positions: only a row that covers one is offered
        const long long m_nx = R.jobs[C.job].m_nx, m_off = R.jobs[C.job].m_off;
        if (x >= m_nx) { atomicOr(err, KT_ERR_BOUNDS); return false; }
        if (!((R.mask[m_off + (x >> 6)] >> (x & 63)) & 1ull)) return false;
    }
    *key = ((unsigned long long) u << KT_RUN_BITS) | (KT_RUN_MASK - (unsigned long long) (C.local + i));
    return true;
}

__device__ static inline void kt_count(const KtState *st, unsigned *hist, int kmer, unsigned long long key, int shift) {
    const KtState &s = st[kmer];
    if (s.done) return;
    if (shift < 50 && (key >> (shift + 10)) != s.prefix) return;
    atomicAdd(&hist[(size_t) kmer * KT_BINS + ((key >> shift) & (KT_BINS - 1))], 1u);
}

__global__ __launch_bounds__(256) void k_kt_hist_rows(const KtRow *__restrict__ rows, long long n, const KtState *__restrict__ st,
                                                      unsigned *__restrict__ hist, int shift) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const KtRow r = rows[i];
    kt_count(st, hist, r.kmer, r.key, shift);
}

template <bool P8>
__global__ __launch_bounds__(256) void k_kt_hist_rec(KtRecs R, const KtState *__restrict__ st, unsigned *__restrict__ hist, int shift,
                                                     unsigned *__restrict__ err) {
    const SaRecChunk C = R.chunks[blockIdx.x];
    for (int i = threadIdx.x; i < C.n; i += blockDim.x) {
        int kmer, x;
        unsigned long long key;
        long long y;
        if (kt_rec(R, P8, C, i, &kmer, &key, &y, &x, err)) kt_count(st, hist, kmer, key, shift);
    }
}

// k-mer blockIdx.x (one wave): lane l holds bins [16 l, 16 l + 16); suffix sums from the top bin down find the digit of the
// need-th largest key.  Level 0 (shift 50) also settles every k-mer with at most N candidates (all of them are kept).
__global__ __launch_bounds__(64) void k_kt_cut(KtState *__restrict__ st, const unsigned *__restrict__ hist, int shift,
                                               unsigned *__restrict__ active, unsigned long long *__restrict__ tied) {
    const long long km = blockIdx.x;
    const int lane = threadIdx.x;
    KtState s = st[km];
    if (s.done) return;
    const unsigned *h = hist + (size_t) km * KT_BINS + (size_t) lane * 16;
    long long mine = 0;
    for (int q = 0; q < 16; q++) mine += h[q];
    long long incl = mine;   // sum over lanes >= lane
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_down(incl, o);
        if (lane + o < 64) incl += u;
    }
    const long long total = __shfl(incl, 0);
    if (shift == 50 && total <= s.need) {   // (s.need is N at level 0)
        if (lane == 0) { s.done = 1; s.thr = 0; s.keep = total; st[km] = s; }
        return;
    }
    if (shift == 50) s.keep = s.need;
    const long long above = incl - mine;   // keys in bins of higher lanes
    const bool mine_holds = above < s.need && incl >= s.need;
    const unsigned long long owner = __ballot(mine_holds);
    const int ol = owner ? (int) __ffsll((long long) owner) - 1 : -1;
    if (lane != ol) {
        if (lane == 0 && ol < 0) atomicAdd(active, 0x10000u);   // (cannot happen: the counts hold at least `need` keys)
        return;
    }
    long long acc = above;
    int digit = lane * 16 + 15;
    for (; digit >= lane * 16; digit--) {
        const long long c = h[digit - lane * 16];
        if (acc + c >= s.need) break;
        acc += c;
    }
    const long long c = h[digit - lane * 16];
    s.need -= acc;
    s.prefix = (s.prefix << 10) | (unsigned long long) digit;
    if (c == s.need || shift == 0) {
        s.done = 1;
        s.thr = s.prefix << shift;
    } else {
        atomicAdd(active, 1u);
        if (shift == 40) atomicAdd(tied, (unsigned long long) c);   // (the rows at the cutoff posterior: the run-order levels' input)
    }
    st[km] = s;
}

// The run-order levels read only the rows tied at the cutoff posterior of a k-mer still open after the two posterior levels:
// these copy them (key and k-mer) into one buffer, in any order (the keys are unique).
__device__ static inline void kt_tie(const KtState *st, int kmer, unsigned long long key, KtRow *tie, unsigned long long *n_tie,
                                     unsigned long long cap, unsigned *err) {
    const KtState &s = st[kmer];
    if (s.done || (key >> 40) != s.prefix) return;
    const unsigned long long slot = atomicAdd(n_tie, 1ull);
    if (slot >= cap) { atomicOr(err, KT_ERR_BOUNDS); return; }
    KtRow r;
    r.key = key; r.desc = 0; r.kmer = kmer; r.neg_zero = 0;
    tie[slot] = r;
}
__global__ __launch_bounds__(256) void k_kt_tie_rows(const KtRow *__restrict__ rows, long long n, const KtState *__restrict__ st,
                                                     KtRow *__restrict__ tie, unsigned long long *__restrict__ n_tie, unsigned long long cap,
                                                     unsigned *__restrict__ err) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) kt_tie(st, rows[i].kmer, rows[i].key, tie, n_tie, cap, err);
}
template <bool P8>
__global__ __launch_bounds__(256) void k_kt_tie_rec(KtRecs R, const KtState *__restrict__ st, KtRow *__restrict__ tie,
                                                    unsigned long long *__restrict__ n_tie, unsigned long long cap, unsigned *__restrict__ err) {
    const SaRecChunk C = R.chunks[blockIdx.x];
    for (int i = threadIdx.x; i < C.n; i += blockDim.x) {
        int kmer, x;
        unsigned long long key;
        long long y;
        if (kt_rec(R, P8, C, i, &kmer, &key, &y, &x, err)) kt_tie(st, kmer, key, tie, n_tie, cap, err);
    }
}

// exclusive scan of keep[0 .. n) into off[0 .. n], one block
__global__ __launch_bounds__(SA_SCAN_THREADS) void k_kt_scan(const KtState *__restrict__ st, long long *__restrict__ off, long long n) {
    sa_block_excl_scan([st](long long i) { return st[i].keep; }, off, n);
}

__device__ static inline void kt_put(const KtState *st, const long long *off, unsigned long long *fill, KtRow *out, const KtRow &r,
                                     unsigned *err) {
    const KtState &s = st[r.kmer];
    if (r.key < s.thr) return;
    const long long slot = off[r.kmer] + (long long) atomicAdd(&fill[r.kmer], 1ull);
    if (slot >= off[r.kmer + 1]) { atomicOr(err, KT_ERR_BOUNDS); return; }
    out[slot] = r;
}

__global__ __launch_bounds__(256) void k_kt_compact_rows(const KtRow *__restrict__ rows, long long n, const KtState *__restrict__ st,
                                                         const long long *__restrict__ off, unsigned long long *__restrict__ fill,
                                                         KtRow *__restrict__ out, unsigned *__restrict__ err) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) kt_put(st, off, fill, out, rows[i], err);
}

template <bool P8>
__global__ __launch_bounds__(256) void k_kt_compact_rec(KtRecs R, const KtState *__restrict__ st, const long long *__restrict__ off,
                                                        unsigned long long *__restrict__ fill, KtRow *__restrict__ out,
                                                        unsigned *__restrict__ err) {
    const SaRecChunk C = R.chunks[blockIdx.x];
    const KtJob J = R.jobs[C.job];
    for (int i = threadIdx.x; i < C.n; i += blockDim.x) {
        KtRow r;
        long long y;
        int x;
        if (!kt_rec(R, P8, C, i, &r.kmer, &r.key, &y, &x, err)) continue;
        if (r.key < st[r.kmer].thr) continue;
        if (y >= J.n_ev) { atomicOr(err, KT_ERR_BOUNDS); continue; }
        const double e = R.ev[J.ev_off + y], level = R.level[r.kmer];
        const double desc = (e + J.var * level - J.scale * level - J.shift) / J.var;   // signalMachine.c descale(); no contraction
        if (kt_desc_units(desc, &r.desc, &r.neg_zero) != SA_OK) { atomicOr(err, KT_ERR_RANGE); continue; }
        kt_put(st, off, fill, out, r, err);
    }
}

// ---- a table with positions: the cover mask and the coverage counts ------------------------------------------------------------
// A positions line as a key: (contig, site strand, position), so the lines a row can cover are one run of the sorted keys.
#define KT_POS_MAX_CONTIG (1ll << 21)
#define KT_POS_MAX_POS (1ll << 41)
#define KT_POS_MAX_X0 (1ll << 42)
__host__ __device__ static inline unsigned long long kt_pos_key(long long contig, int strand, long long pos) {
    return ((unsigned long long) contig << 42) | ((unsigned long long) strand << 41) | (unsigned long long) pos;
}
// the first index of a[0 .. n) whose entry is >= key
__device__ __forceinline__ long long kt_lower_bound(const unsigned long long *__restrict__ a, long long n, unsigned long long key) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// The keys a row at reference_index ri of job J covers are those in [*lo, *hi]: positions ri .. ri + k - 1 (p - (k - 1) <= ri <= p).
// false: the window lies outside the positions a key can have.
__device__ static inline bool kt_window(const KtJob &J, long long ri, int k, unsigned long long *lo, unsigned long long *hi) {
    const long long a = ri < 0 ? 0 : ri, b = ri + k - 1 < KT_POS_MAX_POS ? ri + k - 1 : KT_POS_MAX_POS - 1;
    if (b < a) return false;
    *lo = kt_pos_key(J.contig, J.site_strand, a);
    *hi = kt_pos_key(J.contig, J.site_strand, b);
    return true;
}

// The cover mask: one thread per (job, x), a wave per 64-bit word (a job's bits start at a word of their own, woff[j]); one
// lower-bound search of the sorted keys answers "is there a key of this contig and site strand in [ri, ri + k - 1]", and the
// wave's ballot is the word.  The selection's passes (kt_rec) then test one bit per record.
__global__ __launch_bounds__(256) void k_kt_cover(const KtJob *__restrict__ jobs, const long long *__restrict__ woff, long long n_jobs,
                                                  long long n_words, const unsigned long long *__restrict__ keys, long long n_keys, int k,
                                                  unsigned long long *__restrict__ mask) {
    const long long gid = (long long) blockIdx.x * blockDim.x + threadIdx.x, w = gid >> 6;
    if (w >= n_words) return;   // (a whole wave: the ballot below sees full waves only)
    long long lo = 0, hi = n_jobs;   // the job whose words hold w: the last j with woff[j] <= w
    while (hi - lo > 1) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (woff[mid] <= w) lo = mid; else hi = mid;
    }
    const KtJob J = jobs[lo];
    const long long x = ((w - J.m_off) << 6) + (threadIdx.x & 63);
    bool covered = false;
    unsigned long long k_lo, k_hi;
    if (x < J.m_nx && kt_window(J, J.x0 + (long long) J.x_sign * x, k, &k_lo, &k_hi)) {
        const long long at = kt_lower_bound(keys, n_keys, k_lo);
        covered = at < n_keys && keys[at] <= k_hi;
    }
    const unsigned long long word = __ballot(covered);
    if ((threadIdx.x & 63) == 0) mask[w] = word;
}

// The coverage counts, once per add: an offered record (kt_rec: posterior and mask bit) walks the at most k keys of its window
// and adds one to each, a 64-bit integer atomic per key straight into HBM (no LDS stage: DESIGN.md, "Training from labelled positions").
template <bool P8>
__global__ __launch_bounds__(256) void k_kt_cover_count(KtRecs R, const unsigned long long *__restrict__ keys, long long n_keys, int k,
                                                        unsigned long long *__restrict__ cnt, unsigned *__restrict__ err) {
    const SaRecChunk C = R.chunks[blockIdx.x];
    const KtJob J = R.jobs[C.job];
    for (int i = threadIdx.x; i < C.n; i += blockDim.x) {
        int kmer, x;
        unsigned long long key, k_lo, k_hi;
        long long y;
        if (!kt_rec(R, P8, C, i, &kmer, &key, &y, &x, err)) continue;
        if (!kt_window(J, J.x0 + (long long) J.x_sign * x, k, &k_lo, &k_hi)) continue;
        for (long long at = kt_lower_bound(keys, n_keys, k_lo); at < n_keys && keys[at] <= k_hi; at++) atomicAdd(&cnt[at], 1ull);
    }
}

struct KtRaw {                  // per k-mer result of k_kt_stats
    long long n, S;
    unsigned long long q_lo, q_hi;
    long long med2;             // median in half units (sum of the two middle values)
    unsigned long long mad4;    // MAD in quarter units (sum of the two middle |2 x - med2|)
};

// value of rank r (ascending) among f(0 .. n), unsigned 64-bit, 8 bits per pass; every thread of the block gets it
template <class F>
__device__ static unsigned long long kt_select(F f, long long n, long long r, unsigned *hist, unsigned long long *sh) {
    unsigned long long prefix = 0;
    for (int s = 56; s >= 0; s -= 8) {
        for (int t = threadIdx.x; t < 256; t += blockDim.x) hist[t] = 0;
        __syncthreads();
        for (long long i = threadIdx.x; i < n; i += blockDim.x) {
            const unsigned long long v = f(i);
            if (s == 56 || (v >> (s + 8)) == prefix) atomicAdd(&hist[(v >> s) & 255], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            long long c = 0;
            int d = 0;
            for (; d < 255; d++) {
                if (r < c + (long long) hist[d]) break;
                c += hist[d];
            }
            sh[0] = (prefix << 8) | (unsigned long long) d;
            sh[1] = (unsigned long long) (r - c);
        }
        __syncthreads();
        prefix = sh[0];
        r = (long long) sh[1];
        __syncthreads();
    }
    return prefix;
}

#define KT_STATS_THREADS 256
__global__ __launch_bounds__(KT_STATS_THREADS) void k_kt_stats(const KtRow *__restrict__ rows, const long long *__restrict__ off, int median,
                                                               KtRaw *__restrict__ out) {
    __shared__ long long s_S[KT_STATS_THREADS];
    __shared__ unsigned long long s_lo[KT_STATS_THREADS], s_hi[KT_STATS_THREADS];
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sh[2];
    const long long km = blockIdx.x, a = off[km], n = off[km + 1] - a;
    const int t = threadIdx.x;
    long long S = 0;
    unsigned long long lo = 0, hi = 0;
    for (long long i = t; i < n; i += KT_STATS_THREADS) {
        const long long v = rows[a + i].desc;
        S += v;
        const unsigned long long u = (unsigned long long) (v < 0 ? -v : v), sq = u * u;   // |v| <= 2^31 (KT_DESC_LIMIT): u^2 <= 2^62
        lo += sq;
        hi += lo < sq ? 1ull : 0ull;
    }
    s_S[t] = S; s_lo[t] = lo; s_hi[t] = hi;
    __syncthreads();
    for (int w = KT_STATS_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) {
            s_S[t] += s_S[t + w];
            const unsigned long long l = s_lo[t] + s_lo[t + w];
            s_hi[t] += s_hi[t + w] + (l < s_lo[t] ? 1ull : 0ull);
            s_lo[t] = l;
        }
        __syncthreads();
    }
    KtRaw R;
    R.n = n; R.S = s_S[0]; R.q_lo = s_lo[0]; R.q_hi = s_hi[0]; R.med2 = 0; R.mad4 = 0;
    if (median && n > 0) {
        const unsigned long long bias = 1ull << 63;
        auto val = [&](long long i) { return (unsigned long long) rows[a + i].desc ^ bias; };
        const long long lo_m = (long long) (kt_select(val, n, (n - 1) / 2, hist, sh) ^ bias);
        const long long hi_m = (long long) (kt_select(val, n, n / 2, hist, sh) ^ bias);
        const long long med2 = lo_m + hi_m;
        auto dev = [&](long long i) {
            const long long d = 2 * rows[a + i].desc - med2;
            return (unsigned long long) (d < 0 ? -d : d);
        };
        R.med2 = med2;
        R.mad4 = kt_select(dev, n, (n - 1) / 2, hist, sh) + kt_select(dev, n, n / 2, hist, sh);
    }
    if (t == 0) out[km] = R;
}

// ---- the table ---------------------------------------------------------------------------------------------------------------
struct KtSide {
    KtRow *d_rows = nullptr;          // n_rows rows, k-mer segments at off[]
    long long n_rows = 0;
    long long *d_off = nullptr;       // n_kmers + 1
};
struct sa_kmer_table {
    int n_alpha = 0, k = 0, device = 0;
    char alphabet[64] = {0};
    long long n_kmers = 0, N = 0, min_units = 0;
    unsigned long long run_next = 0;  // run ordinal of the next row
    double *d_level = nullptr;
    KtSide side[2];
    // sa_kmer_table_checkpoint: the state to go back to; the arrays a side had then are kept (not returned to the pool) when the
    // side first changes after the checkpoint
    bool ck = false;
    unsigned long long ck_run = 0;
    KtSide ck_side[2];
    bool ck_taken[2] = {false, false};
    // sa_kmer_table_set_positions: the distinct lines as sorted keys (kt_pos_key), and per key the offered rows that cover it:
    // d_pcnt holds n_pkey live counts and then n_pkey more, their values at the checkpoint
    bool has_pos = false;
    std::vector<unsigned long long> h_pkey;
    unsigned long long *d_pkey = nullptr, *d_pcnt = nullptr;
    double at_ms[2] = {0.0, 0.0};     // the last add's cover mask and counts pass
    std::mutex mu;
    hipEvent_t e0 = nullptr, e1 = nullptr;
};

extern "C" int sa_kmer_table_create(sa_kmer_table_t **out, const sa_model_t *m, int64_t max_per_kmer, double min_prob, int device) {
    if (!out || !m || max_per_kmer < 1 || !(min_prob >= 0.0 && min_prob <= 1.0)) return SA_EINVAL;
    *out = nullptr;
    if (const int rc = sa_device_check(device, /* quiet */ true)) return rc;
    if (hipSetDevice(device) != hipSuccess) return SA_ENODEVICE;
    sa_kmer_table *t = new (std::nothrow) sa_kmer_table();
    if (!t) return SA_ENOMEM;
    t->n_alpha = m->n_alpha; t->k = m->k; t->device = device;
    memcpy(t->alphabet, m->alphabet, sizeof(t->alphabet));
    t->n_kmers = m->n_kmers;
    t->N = max_per_kmer;
    // float(printed) >= min_prob: the smallest printed value that passes (the parse of "%f" is units / 1e6, correctly rounded)
    long long u = 0;
    while (u <= 1000000 && !((double) u / 1e6 >= min_prob)) u++;
    t->min_units = u;
    std::vector<double> level((size_t) t->n_kmers);
    for (long long i = 0; i < t->n_kmers; i++) level[(size_t) i] = m->table5[5 * i];
    int rc = SA_OK;
    std::vector<long long> zero((size_t) t->n_kmers + 1, 0);
    SA_HIP_GOTO_DONE(hipEventCreate(&t->e0));
    SA_HIP_GOTO_DONE(hipEventCreate(&t->e1));
    SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &t->d_level, sizeof(double) * (size_t) t->n_kmers, device));
    SA_HIP_GOTO_DONE(hipMemcpy(t->d_level, level.data(), sizeof(double) * (size_t) t->n_kmers, hipMemcpyHostToDevice));
    for (int s = 0; s < 2; s++) {
        SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &t->side[s].d_off, sizeof(long long) * zero.size(), device));
        SA_HIP_GOTO_DONE(hipMemcpy(t->side[s].d_off, zero.data(), sizeof(long long) * zero.size(), hipMemcpyHostToDevice));
    }
done:
    if (rc != SA_OK) { sa_kmer_table_destroy(t); return rc; }
    *out = t;
    return SA_OK;
}

extern "C" void sa_kmer_table_destroy(sa_kmer_table_t *t) {
    if (!t) return;
    (void) hipSetDevice(t->device);
    for (int s = 0; s < 2; s++) {
        g_sa_pool.put(SaPool::DEVICE, t->side[s].d_rows);
        g_sa_pool.put(SaPool::DEVICE, t->side[s].d_off);
        if (t->ck_taken[s]) {
            g_sa_pool.put(SaPool::DEVICE, t->ck_side[s].d_rows);
            g_sa_pool.put(SaPool::DEVICE, t->ck_side[s].d_off);
        }
    }
    g_sa_pool.put(SaPool::DEVICE, t->d_level);
    g_sa_pool.put(SaPool::DEVICE, t->d_pkey);
    g_sa_pool.put(SaPool::DEVICE, t->d_pcnt);
    if (t->e0) (void) hipEventDestroy(t->e0);
    if (t->e1) (void) hipEventDestroy(t->e1);
    delete t;
}

// The selection over the table's rows of `side` and a set of new candidates, and the new table.  `rec` (records of a batch,
// nc chunks) or `rows` (n_new rows already in table form) are the new candidates.  Levels 1-2 (the posterior) histogram every
// candidate; if a k-mer is still open then, its rows at the cutoff posterior are copied out once (k_kt_tie_*) and levels 3-6
// (the run ordinal) histogram only that copy.  *kms_out: HIP-event time of the device work, summed over the stretches between
// the host's reads of the level counters (the waits for those reads are not in it).
static int kt_merge(sa_kmer_table *t, int side, const KtRecs *rec, bool p8, long long nc, const KtRow *new_rows, long long n_new,
                    double *kms_out) {
    KtSide &S = t->side[side];
    const long long nk = t->n_kmers;
    const int dev = t->device;
    int rc = SA_OK;
    char *d = nullptr;
    KtRow *d_new = nullptr, *d_tie = nullptr;
    long long *d_off_new = nullptr;
    long long total = 0;
    unsigned h_err = 0, h_active = 0;
    unsigned long long h_tied = 0;
    double kms = 0;
    float seg = 0;
    // scratch: [state | hist | off | fill | err, active | tied, n_tie]; each pair of words is one entry (one memset clears both)
    SaLayout L;
    const size_t o_st = L.add(sizeof(KtState) * (size_t) nk), o_hist = L.add(4 * (size_t) nk * KT_BINS), o_off = L.add(8 * (size_t) (nk + 1)),
                 o_fill = L.add(8 * (size_t) nk), o_err = L.add(2 * 4), o_tied = L.add(2 * 8), bytes = L.end;
    std::vector<KtState> st0((size_t) nk);
    for (KtState &q : st0) { q.prefix = 0; q.thr = 0; q.need = t->N; q.keep = 0; q.done = 0; q.pad = 0; }
    SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &d, bytes, dev));
    {
        KtState *st = (KtState *) (d + o_st);
        unsigned *hist = (unsigned *) (d + o_hist), *err = (unsigned *) (d + o_err), *active = err + 1;
        unsigned long long *tied = (unsigned long long *) (d + o_tied), *n_tie = tied + 1;
        long long *off = (long long *) (d + o_off);
        unsigned long long *fill = (unsigned long long *) (d + o_fill);
        SA_HIP_GOTO_DONE(hipMemcpyAsync(st, st0.data(), sizeof(KtState) * (size_t) nk, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemsetAsync(err, 0, 8, 0));
        SA_HIP_GOTO_DONE(hipMemsetAsync(tied, 0, 16, 0));
        for (int shift = 50; shift >= 0; shift -= 10) {
            SA_HIP_GOTO_DONE(hipEventRecord(t->e0, 0));
            SA_HIP_GOTO_DONE(hipMemsetAsync(hist, 0, 4 * (size_t) nk * KT_BINS, 0));
            SA_HIP_GOTO_DONE(hipMemsetAsync(active, 0, 4, 0));
            if (shift >= 40) {   // the posterior levels: every candidate
                if (S.n_rows)
                    hipLaunchKernelGGL(k_kt_hist_rows, dim3((unsigned) ((S.n_rows + 255) / 256)), dim3(256), 0, 0, S.d_rows, S.n_rows, st, hist, shift);
                if (n_new)
                    hipLaunchKernelGGL(k_kt_hist_rows, dim3((unsigned) ((n_new + 255) / 256)), dim3(256), 0, 0, new_rows, n_new, st, hist, shift);
                if (nc) {
                    if (p8) hipLaunchKernelGGL(k_kt_hist_rec<true>, dim3((unsigned) nc), dim3(256), 0, 0, *rec, st, hist, shift, err);
                    else hipLaunchKernelGGL(k_kt_hist_rec<false>, dim3((unsigned) nc), dim3(256), 0, 0, *rec, st, hist, shift, err);
                }
            } else if (h_tied) {   // the run-order levels: the tied rows only
                hipLaunchKernelGGL(k_kt_hist_rows, dim3((unsigned) ((h_tied + 255) / 256)), dim3(256), 0, 0, d_tie, (long long) h_tied, st, hist, shift);
            }
            hipLaunchKernelGGL(k_kt_cut, dim3((unsigned) nk), dim3(64), 0, 0, st, hist, shift, active, tied);
            SA_HIP_GOTO_DONE(hipEventRecord(t->e1, 0));
            SA_HIP_GOTO_DONE(hipGetLastError());
            SA_HIP_GOTO_DONE(hipMemcpy(&h_active, active, 4, hipMemcpyDeviceToHost));
            SA_HIP_GOTO_DONE(hipEventElapsedTime(&seg, t->e0, t->e1));
            kms += seg;
            if (h_active >= 0x10000u) { rc = SA_ENODEVICE; goto done; }   // (a cut found fewer keys than it counted before)
            if (h_active == 0) break;
            if (shift == 40) {   // k-mers still open: copy their rows at the cutoff posterior out once
                SA_HIP_GOTO_DONE(hipMemcpy(&h_tied, tied, 8, hipMemcpyDeviceToHost));
                SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &d_tie, sizeof(KtRow) * (size_t) (h_tied ? h_tied : 1), dev));
                SA_HIP_GOTO_DONE(hipEventRecord(t->e0, 0));
                if (S.n_rows)
                    hipLaunchKernelGGL(k_kt_tie_rows, dim3((unsigned) ((S.n_rows + 255) / 256)), dim3(256), 0, 0, S.d_rows, S.n_rows, st, d_tie, n_tie, h_tied, err);
                if (n_new)
                    hipLaunchKernelGGL(k_kt_tie_rows, dim3((unsigned) ((n_new + 255) / 256)), dim3(256), 0, 0, new_rows, n_new, st, d_tie, n_tie, h_tied, err);
                if (nc) {
                    if (p8) hipLaunchKernelGGL(k_kt_tie_rec<true>, dim3((unsigned) nc), dim3(256), 0, 0, *rec, st, d_tie, n_tie, h_tied, err);
                    else hipLaunchKernelGGL(k_kt_tie_rec<false>, dim3((unsigned) nc), dim3(256), 0, 0, *rec, st, d_tie, n_tie, h_tied, err);
                }
                SA_HIP_GOTO_DONE(hipEventRecord(t->e1, 0));
                SA_HIP_GOTO_DONE(hipGetLastError());
                SA_HIP_GOTO_DONE(hipEventSynchronize(t->e1));
                SA_HIP_GOTO_DONE(hipEventElapsedTime(&seg, t->e0, t->e1));
                kms += seg;
            }
        }
        SA_HIP_GOTO_DONE(hipEventRecord(t->e0, 0));
        hipLaunchKernelGGL(k_kt_scan, dim3(1), dim3(SA_SCAN_THREADS), 0, 0, st, off, nk);
        SA_HIP_GOTO_DONE(hipEventRecord(t->e1, 0));
        SA_HIP_GOTO_DONE(hipMemcpy(&total, off + nk, 8, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(hipEventElapsedTime(&seg, t->e0, t->e1));
        kms += seg;
        SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &d_new, sizeof(KtRow) * (size_t) (total > 0 ? total : 1), dev));
        SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &d_off_new, 8 * (size_t) (nk + 1), dev));
        SA_HIP_GOTO_DONE(hipEventRecord(t->e0, 0));
        SA_HIP_GOTO_DONE(hipMemsetAsync(fill, 0, 8 * (size_t) nk, 0));
        if (S.n_rows)
            hipLaunchKernelGGL(k_kt_compact_rows, dim3((unsigned) ((S.n_rows + 255) / 256)), dim3(256), 0, 0, S.d_rows, S.n_rows, st, off, fill, d_new, err);
        if (n_new)
            hipLaunchKernelGGL(k_kt_compact_rows, dim3((unsigned) ((n_new + 255) / 256)), dim3(256), 0, 0, new_rows, n_new, st, off, fill, d_new, err);
        if (nc) {
            if (p8) hipLaunchKernelGGL(k_kt_compact_rec<true>, dim3((unsigned) nc), dim3(256), 0, 0, *rec, st, off, fill, d_new, err);
            else hipLaunchKernelGGL(k_kt_compact_rec<false>, dim3((unsigned) nc), dim3(256), 0, 0, *rec, st, off, fill, d_new, err);
        }
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d_off_new, off, 8 * (size_t) (nk + 1), hipMemcpyDeviceToDevice, 0));
        SA_HIP_GOTO_DONE(hipEventRecord(t->e1, 0));
        SA_HIP_GOTO_DONE(hipGetLastError());
        SA_HIP_GOTO_DONE(hipMemcpy(&h_err, err, 4, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(hipEventElapsedTime(&seg, t->e0, t->e1));
        kms += seg;
        if (h_err & KT_ERR_BOUNDS) { rc = SA_EINVAL; goto done; }
        if (h_err & KT_ERR_RANGE) { rc = SA_EUNSUPPORTED; goto done; }
        if (t->ck && !t->ck_taken[side]) {   // the first change since the checkpoint: keep what the side had
            t->ck_side[side] = S;
            t->ck_taken[side] = true;
        } else {
            g_sa_pool.put(SaPool::DEVICE, S.d_rows);
            g_sa_pool.put(SaPool::DEVICE, S.d_off);
        }
        S.d_rows = d_new;
        S.d_off = d_off_new;
        S.n_rows = total;
        d_new = nullptr;
        d_off_new = nullptr;
        if (kms_out) *kms_out = kms;
    }
done:
    if (rc != SA_OK) (void) hipDeviceSynchronize();
    g_sa_pool.put(SaPool::DEVICE, d_new);
    g_sa_pool.put(SaPool::DEVICE, d_off_new);
    g_sa_pool.put(SaPool::DEVICE, d_tie);
    g_sa_pool.put(SaPool::DEVICE, d);
    return rc;
}

extern "C" int sa_kmer_table_checkpoint(sa_kmer_table_t *t) {
    if (!t) return SA_EINVAL;
    std::lock_guard<std::mutex> g(t->mu);
    (void) hipSetDevice(t->device);
    for (int s = 0; s < 2; s++)
        if (t->ck_taken[s]) {
            g_sa_pool.put(SaPool::DEVICE, t->ck_side[s].d_rows);
            g_sa_pool.put(SaPool::DEVICE, t->ck_side[s].d_off);
            t->ck_side[s] = KtSide();
            t->ck_taken[s] = false;
        }
    if (!t->h_pkey.empty() &&
        hipMemcpy(t->d_pcnt + t->h_pkey.size(), t->d_pcnt, 8 * t->h_pkey.size(), hipMemcpyDeviceToDevice) != hipSuccess)
        return SA_ENODEVICE;
    t->ck = true;
    t->ck_run = t->run_next;
    return SA_OK;
}

extern "C" int sa_kmer_table_rollback(sa_kmer_table_t *t) {
    if (!t) return SA_EINVAL;
    std::lock_guard<std::mutex> g(t->mu);
    if (!t->ck) return SA_ESTATE;
    (void) hipSetDevice(t->device);
    for (int s = 0; s < 2; s++)
        if (t->ck_taken[s]) {
            g_sa_pool.put(SaPool::DEVICE, t->side[s].d_rows);
            g_sa_pool.put(SaPool::DEVICE, t->side[s].d_off);
            t->side[s] = t->ck_side[s];
            t->ck_side[s] = KtSide();
            t->ck_taken[s] = false;
        }
    t->run_next = t->ck_run;
    if (!t->h_pkey.empty() &&
        hipMemcpy(t->d_pcnt, t->d_pcnt + t->h_pkey.size(), 8 * t->h_pkey.size(), hipMemcpyDeviceToDevice) != hipSuccess)
        return SA_ENODEVICE;
    return SA_OK;
}

static int kt_kmer_ids(const sa_kmer_table *t, const char *ref, long long n_x, int *out) {
    int digit[256];
    for (int c = 0; c < 256; c++) digit[c] = -1;
    for (int a = 0; a < t->n_alpha; a++) digit[(unsigned char) t->alphabet[a]] = a;
    for (long long x = 0; x < n_x; x++) {
        long long id = 0;
        for (int i = 0; i < t->k; i++) {
            const int dg = digit[(unsigned char) ref[x + i]];
            if (dg < 0) return SA_EALPHABET;
            id = id * t->n_alpha + dg;
        }
        out[x] = (int) id;
    }
    return SA_OK;
}

// sa_kmer_table_add_batch (map NULL) and sa_kmer_table_add_batch_at (map[j] places job j on a table with positions)
static int kt_add_batch(sa_kmer_table_t *t, sa_batch_t *b, const sa_job_t *jobs, int64_t n_jobs, int strand, const sa_train_job_map_t *map,
                        bool at, double *kernel_ms_out) {
    if (!t || !b || (n_jobs > 0 && !jobs) || n_jobs < 0 || (strand != 0 && strand != 1) || (at && n_jobs > 0 && !map)) return SA_EINVAL;
    std::lock_guard<std::mutex> g(t->mu);
    if (at != t->has_pos) return SA_ESTATE;   // (rows without coordinates on a table with positions, or the reverse)
    SaBatchView V;
    int rc = sa_batch_view(b, &V);
    if (V.batch_flags & SA_FLAG_VC_ROWS) return SA_EINVAL;   // (it dropped rows; refused before the batch's state is looked at)
    if (rc) return rc;
    if (V.batch_flags & SA_FLAG_EXPECT_INTERNAL) return SA_ESTATE;
    if ((int64_t) V.count.size() != n_jobs || V.device != t->device) return SA_EINVAL;
    const bool p8 = V.p8;   // (either record size is read)
    const std::vector<long long> &count = V.count;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    const size_t nj = (size_t) n_jobs;
    long long n_total = 0;
    for (size_t j = 0; j < nj; j++) n_total += count[j];
    if (t->run_next + (unsigned long long) n_total > KT_RUN_MASK) return SA_EUNSUPPORTED;
    // per job: events (dense means), for 8-byte records the k-mer id of every reference position, and with positions the job's
    // words of the cover mask
    std::vector<KtJob> kj(nj);
    std::vector<long long> woff(nj + 1, 0);
    long long n_ev = 0, n_x = 0, n_words = 0;
    for (size_t j = 0; j < nj; j++) {
        const sa_job_t &J = jobs[j];
        if (J.n_events < 0 || (J.n_events > 0 && (!J.events || J.event_stride < 1)) || !(J.var != 0)) return SA_EINVAL;
        kj[j].ev_off = n_ev; kj[j].n_ev = J.n_events;
        kj[j].scale = J.scale; kj[j].shift = J.shift; kj[j].var = J.var;
        n_ev += J.n_events;
        const long long positions = std::max<long long>(0, J.ref_len - t->k + 1), lx = p8 ? positions : 0;
        if (p8 && lx > 0 && !J.ref) return SA_EINVAL;
        kj[j].x_off = n_x; kj[j].n_x = lx;
        n_x += lx;
        kj[j].m_off = n_words; kj[j].m_nx = 0; kj[j].x0 = 0;
        kj[j].contig = 0; kj[j].x_sign = 1; kj[j].site_strand = 0; kj[j].pad = 0;
        if (at) {
            const sa_train_job_map_t &m = map[j];
            if (m.contig < 0 || m.contig >= KT_POS_MAX_CONTIG || (m.x_sign != 1 && m.x_sign != -1) ||
                (m.site_strand != 0 && m.site_strand != 1) || m.x0 <= -KT_POS_MAX_X0 || m.x0 >= KT_POS_MAX_X0)
                return SA_EINVAL;
            kj[j].m_nx = positions; kj[j].x0 = m.x0;
            kj[j].contig = m.contig; kj[j].x_sign = m.x_sign; kj[j].site_strand = m.site_strand;
            n_words += (positions + 63) / 64;
        }
        woff[j + 1] = n_words;
    }
    const std::vector<SaRecChunk> chunks = sa_view_chunks(V, SA_CHAIN_CHUNK, (long long) t->run_next);   // (run ordinals)
    const long long nc = (long long) chunks.size();
    // one pinned staging block and one device block: [jobs | chunks | events | k-mer ids | mask word offsets]; the device block
    // has the cover mask behind that
    SaLayout L;
    const size_t o_jobs = L.add(sizeof(KtJob) * nj), o_ch = L.add(sizeof(SaRecChunk) * (size_t) nc), o_ev = L.add(8 * (size_t) n_ev),
                 o_xk = L.add(4 * (size_t) n_x + 4), o_woff = L.add(8 * (nj + 1)), bytes = L.end, o_mask = L.add(8 * (size_t) n_words + 8),
                 o_cerr = L.add(8), d_bytes = L.end;
    char *h = nullptr, *d = nullptr;
    if (hipSetDevice(t->device) != hipSuccess) return SA_ENODEVICE;
    if (g_sa_pool.get(SaPool::PINNED, (void **) &h, bytes, t->device) != hipSuccess) return SA_ENOMEM;
    {
        memcpy(h + o_jobs, kj.data(), sizeof(KtJob) * nj);
        if (nc) memcpy(h + o_ch, chunks.data(), sizeof(SaRecChunk) * (size_t) nc);
        memcpy(h + o_woff, woff.data(), 8 * (nj + 1));
        double *ev = (double *) (h + o_ev);
        int *xk = (int *) (h + o_xk);
        std::vector<int> bad(nj, SA_OK);
        sa_parallel_for(nj, [&](size_t j) {
            const sa_job_t &J = jobs[j];
            double *e = ev + kj[j].ev_off;
            for (long long y = 0; y < J.n_events; y++) e[y] = J.events[y * J.event_stride];
            if (p8) bad[j] = kt_kmer_ids(t, J.ref, kj[j].n_x, xk + kj[j].x_off);
        });
        for (size_t j = 0; j < nj; j++)
            if (bad[j] != SA_OK) { rc = bad[j]; goto done; }
        SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &d, d_bytes, t->device));
        SA_HIP_GOTO_DONE(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
        KtRecs R;
        R.recs = V.recs;
        R.chunks = (const SaRecChunk *) (d + o_ch);
        R.jobs = (const KtJob *) (d + o_jobs);
        R.ev = (const double *) (d + o_ev);
        R.xk = (const int *) (d + o_xk);
        R.level = t->d_level;
        R.min_units = t->min_units;
        R.n_kmers = t->n_kmers;
        R.mask = nullptr;
        const long long n_keys = (long long) t->h_pkey.size();
        double merge_ms = 0.0;
        float seg = 0;
        if (at) {   // the cover mask, once for the three passes of the selection and the counts pass
            R.mask = (const unsigned long long *) (d + o_mask);
            t->at_ms[0] = t->at_ms[1] = 0.0;
            if (n_words) {
                SA_HIP_GOTO_DONE(hipEventRecord(t->e0, 0));
                hipLaunchKernelGGL(k_kt_cover, dim3((unsigned) ((n_words * 64 + 255) / 256)), dim3(256), 0, 0, R.jobs,
                                   (const long long *) (d + o_woff), (long long) nj, n_words, t->d_pkey, n_keys, t->k,
                                   (unsigned long long *) (d + o_mask));
                SA_HIP_GOTO_DONE(hipEventRecord(t->e1, 0));
                SA_HIP_GOTO_DONE(hipGetLastError());
                SA_HIP_GOTO_DONE(hipEventSynchronize(t->e1));
                SA_HIP_GOTO_DONE(hipEventElapsedTime(&seg, t->e0, t->e1));
                t->at_ms[0] = seg;
            }
        }
        rc = kt_merge(t, strand, &R, p8, nc, nullptr, 0, &merge_ms);
        if (rc != SA_OK) goto done;
        t->run_next += (unsigned long long) n_total;
        if (at && nc && n_keys) {   // the coverage counts of the offered records
            unsigned h_err = 0;
            unsigned *cerr = (unsigned *) (d + o_cerr);
            SA_HIP_GOTO_DONE(hipMemsetAsync(cerr, 0, 8, 0));
            SA_HIP_GOTO_DONE(hipEventRecord(t->e0, 0));
            if (p8) hipLaunchKernelGGL(k_kt_cover_count<true>, dim3((unsigned) nc), dim3(256), 0, 0, R, t->d_pkey, n_keys, t->k, t->d_pcnt, cerr);
            else hipLaunchKernelGGL(k_kt_cover_count<false>, dim3((unsigned) nc), dim3(256), 0, 0, R, t->d_pkey, n_keys, t->k, t->d_pcnt, cerr);
            SA_HIP_GOTO_DONE(hipEventRecord(t->e1, 0));
            SA_HIP_GOTO_DONE(hipGetLastError());
            SA_HIP_GOTO_DONE(hipMemcpy(&h_err, cerr, 4, hipMemcpyDeviceToHost));
            SA_HIP_GOTO_DONE(hipEventElapsedTime(&seg, t->e0, t->e1));
            t->at_ms[1] = seg;
            if (h_err) { rc = SA_EINVAL; goto done; }   // (cannot happen: the selection read the same records)
        }
        if (kernel_ms_out) *kernel_ms_out = merge_ms + (at ? t->at_ms[0] + t->at_ms[1] : 0.0);
    }
done:
    g_sa_pool.put(SaPool::DEVICE, d);
    g_sa_pool.put(SaPool::PINNED, h);
    return rc;
}

extern "C" int sa_kmer_table_add_batch(sa_kmer_table_t *t, sa_batch_t *b, const sa_job_t *jobs, int64_t n_jobs, int strand,
                                       double *kernel_ms_out) {
    return kt_add_batch(t, b, jobs, n_jobs, strand, nullptr, false, kernel_ms_out);
}

extern "C" int sa_kmer_table_add_batch_at(sa_kmer_table_t *t, sa_batch_t *b, const sa_job_t *jobs, int64_t n_jobs, int strand,
                                          const sa_train_job_map_t *map, double *kernel_ms_out) {
    return kt_add_batch(t, b, jobs, n_jobs, strand, map, true, kernel_ms_out);
}

extern "C" int sa_kmer_table_set_positions(sa_kmer_table_t *t, const sa_train_site_t *sites, int64_t n) {
    if (!t || n < 0 || (n > 0 && !sites)) return SA_EINVAL;
    std::vector<unsigned long long> keys((size_t) n);
    for (int64_t i = 0; i < n; i++) {
        const sa_train_site_t &s = sites[i];
        if (s.contig < 0 || s.contig >= KT_POS_MAX_CONTIG || s.pos < 0 || s.pos >= KT_POS_MAX_POS || (s.mapped_strand != 0 && s.mapped_strand != 1))
            return SA_EINVAL;
        keys[(size_t) i] = kt_pos_key(s.contig, s.mapped_strand, s.pos);
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    std::lock_guard<std::mutex> g(t->mu);
    if (t->run_next != 0 || t->side[0].n_rows != 0 || t->side[1].n_rows != 0) return SA_ESTATE;
    int rc = SA_OK;
    unsigned long long *d_key = nullptr, *d_cnt = nullptr;
    const size_t nk = keys.size();
    if (hipSetDevice(t->device) != hipSuccess) return SA_ENODEVICE;
    SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &d_key, 8 * (nk ? nk : 1), t->device));
    SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &d_cnt, 16 * (nk ? nk : 1), t->device));
    if (nk) SA_HIP_GOTO_DONE(hipMemcpy(d_key, keys.data(), 8 * nk, hipMemcpyHostToDevice));
    SA_HIP_GOTO_DONE(hipMemset(d_cnt, 0, 16 * (nk ? nk : 1)));   // (an empty table's counts, live and at a checkpoint)
    g_sa_pool.put(SaPool::DEVICE, t->d_pkey);
    g_sa_pool.put(SaPool::DEVICE, t->d_pcnt);
    t->d_pkey = d_key;
    t->d_pcnt = d_cnt;
    d_key = d_cnt = nullptr;
    t->h_pkey.swap(keys);
    t->has_pos = true;
done:
    g_sa_pool.put(SaPool::DEVICE, d_key);
    g_sa_pool.put(SaPool::DEVICE, d_cnt);
    return rc;
}

extern "C" int sa_kmer_table_position_counts(const sa_kmer_table_t *t, sa_train_site_t **sites_out, int64_t **counts_out, int64_t *n_out) {
    if (!t || !sites_out || !counts_out || !n_out) return SA_EINVAL;
    *sites_out = nullptr;
    *counts_out = nullptr;
    *n_out = 0;
    std::lock_guard<std::mutex> g(const_cast<sa_kmer_table *>(t)->mu);
    if (!t->has_pos) return SA_ESTATE;
    const size_t nk = t->h_pkey.size();
    sa_train_site_t *s = (sa_train_site_t *) calloc(nk ? nk : 1, sizeof(sa_train_site_t));
    int64_t *c = (int64_t *) calloc(nk ? nk : 1, sizeof(int64_t));
    if (!s || !c) { free(s); free(c); return SA_ENOMEM; }
    if (nk && (hipSetDevice(t->device) != hipSuccess || hipMemcpy(c, t->d_pcnt, 8 * nk, hipMemcpyDeviceToHost) != hipSuccess)) {
        free(s); free(c);
        return SA_ENODEVICE;
    }
    for (size_t i = 0; i < nk; i++) {
        const unsigned long long key = t->h_pkey[i];
        s[i].contig = (int32_t) (key >> 42);
        s[i].mapped_strand = (int32_t) ((key >> 41) & 1ull);
        s[i].pos = (int64_t) (key & ((1ull << 41) - 1ull));
    }
    *sites_out = s;
    *counts_out = c;
    *n_out = (int64_t) nk;
    return SA_OK;
}

extern "C" int sa_kmer_table_add_at_times(const sa_kmer_table_t *t, double ms_out[2]) {
    if (!t || !ms_out) return SA_EINVAL;
    std::lock_guard<std::mutex> g(const_cast<sa_kmer_table *>(t)->mu);
    ms_out[0] = t->at_ms[0];
    ms_out[1] = t->at_ms[1];
    return SA_OK;
}

extern "C" int sa_kmer_table_add_rows(sa_kmer_table_t *t, int strand, const int32_t *kmer_ids, const double *descaled, const double *prob,
                                      int64_t n) {
    if (!t || n < 0 || (n > 0 && (!kmer_ids || !descaled || !prob)) || (strand != 0 && strand != 1)) return SA_EINVAL;
    std::lock_guard<std::mutex> g(t->mu);
    if (t->has_pos) return SA_ESTATE;   // (rows without coordinates)
    if (t->run_next + (unsigned long long) n > KT_RUN_MASK) return SA_EUNSUPPORTED;
    std::vector<KtRow> rows;
    rows.reserve((size_t) n);
    for (int64_t i = 0; i < n; i++) {
        if (kmer_ids[i] < 0 || kmer_ids[i] >= t->n_kmers || !(prob[i] >= 0.0 && prob[i] <= 1.0)) return SA_EINVAL;
        long long pu;
        int nz;
        if (kt_f6_units(prob[i], &pu, &nz) != SA_OK) return SA_EINVAL;
        if (pu < t->min_units) continue;
        KtRow r;
        r.kmer = kmer_ids[i];
        r.key = ((unsigned long long) pu << KT_RUN_BITS) | (KT_RUN_MASK - (t->run_next + (unsigned long long) i));
        if (kt_desc_units(descaled[i], &r.desc, &r.neg_zero) != SA_OK) return SA_EUNSUPPORTED;
        rows.push_back(r);
    }
    int rc = SA_OK;
    KtRow *d = nullptr;
    if (hipSetDevice(t->device) != hipSuccess) return SA_ENODEVICE;
    SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &d, sizeof(KtRow) * (rows.size() ? rows.size() : 1), t->device));
    if (!rows.empty()) SA_HIP_GOTO_DONE(hipMemcpy(d, rows.data(), sizeof(KtRow) * rows.size(), hipMemcpyHostToDevice));
    rc = kt_merge(t, strand, nullptr, false, 0, d, (long long) rows.size(), nullptr);
    if (rc == SA_OK) t->run_next += (unsigned long long) n;
done:
    g_sa_pool.put(SaPool::DEVICE, d);
    return rc;
}

// the rows of a strand and their k-mer offsets, on the host, each k-mer's rows sorted by key (posterior, then run order)
static int kt_fetch(const sa_kmer_table *t, int strand, std::vector<KtRow> *rows, std::vector<long long> *off) {
    const KtSide &S = t->side[strand];
    rows->resize((size_t) S.n_rows);
    off->resize((size_t) t->n_kmers + 1);
    if (hipSetDevice(t->device) != hipSuccess) return SA_ENODEVICE;
    if (S.n_rows && hipMemcpy(rows->data(), S.d_rows, sizeof(KtRow) * (size_t) S.n_rows, hipMemcpyDeviceToHost) != hipSuccess) return SA_ENODEVICE;
    if (hipMemcpy(off->data(), S.d_off, 8 * off->size(), hipMemcpyDeviceToHost) != hipSuccess) return SA_ENODEVICE;
    for (long long km = 0; km < t->n_kmers; km++)
        std::sort(rows->begin() + (*off)[(size_t) km], rows->begin() + (*off)[(size_t) km + 1],
                  [](const KtRow &a, const KtRow &b) { return a.key > b.key; });
    return SA_OK;
}

extern "C" int sa_kmer_table_rows(const sa_kmer_table_t *t, int strand, sa_kmer_row_t **rows_out, int64_t *n_out) {
    if (!t || !rows_out || !n_out || (strand != 0 && strand != 1)) return SA_EINVAL;
    *rows_out = nullptr;
    *n_out = 0;
    std::lock_guard<std::mutex> g(const_cast<sa_kmer_table *>(t)->mu);
    std::vector<KtRow> rows;
    std::vector<long long> off;
    int rc = kt_fetch(t, strand, &rows, &off);
    if (rc) return rc;
    sa_kmer_row_t *o = (sa_kmer_row_t *) calloc(rows.size() ? rows.size() : 1, sizeof(sa_kmer_row_t));
    if (!o) return SA_ENOMEM;
    for (size_t i = 0; i < rows.size(); i++) {
        o[i].descaled_units = rows[i].desc;
        o[i].run = (int64_t) (KT_RUN_MASK - (rows[i].key & KT_RUN_MASK));
        o[i].kmer_id = rows[i].kmer;
        o[i].prob_units = (int32_t) (rows[i].key >> KT_RUN_BITS);
        o[i].neg_zero = rows[i].neg_zero;
    }
    *rows_out = o;
    *n_out = (int64_t) rows.size();
    return SA_OK;
}

static char *kt_put_units(char *w, long long u, int neg_zero) {   // "%f" of u / 1e6 as printf prints the double it came from
    if (u < 0 || neg_zero) *w++ = '-';
    unsigned long long a = (unsigned long long) (u < 0 ? -u : u);
    char tmp[24];
    int n = 0;
    unsigned long long ip = a / 1000000ull;
    do { tmp[n++] = (char) ('0' + ip % 10); ip /= 10; } while (ip);
    while (n) *w++ = tmp[--n];
    *w++ = '.';
    unsigned long long fp = a % 1000000ull;
    for (int q = 5; q >= 0; q--) { w[q] = (char) ('0' + fp % 10); fp /= 10; }
    return w + 6;
}

extern "C" int sa_kmer_table_write(const sa_kmer_table_t *t, int strand, const char *path, int append) {
    if (!t || !path || strand < -1 || strand > 1) return SA_EINVAL;
    FILE *f = fopen(path, append ? "a" : "w");
    if (!f) return SA_EIO;
    std::lock_guard<std::mutex> g(const_cast<sa_kmer_table *>(t)->mu);
    int rc = SA_OK;
    std::vector<char> buf(128);
    for (int s = 0; s < 2 && rc == SA_OK; s++) {
        if (strand >= 0 && s != strand) continue;
        std::vector<KtRow> rows;
        std::vector<long long> off;
        if ((rc = kt_fetch(t, s, &rows, &off)) != SA_OK) break;
        for (const KtRow &r : rows) {
            char *w = buf.data();
            long long id = r.kmer;
            for (int i = t->k - 1; i >= 0; i--) { w[i] = t->alphabet[id % t->n_alpha]; id /= t->n_alpha; }
            w += t->k;
            *w++ = '\t';
            *w++ = s ? 'c' : 't';
            *w++ = '\t';
            w = kt_put_units(w, r.desc, r.neg_zero);
            *w++ = '\t';
            w = kt_put_units(w, (long long) (r.key >> KT_RUN_BITS), 0);
            *w++ = '\n';
            if (fwrite(buf.data(), 1, (size_t) (w - buf.data()), f) != (size_t) (w - buf.data())) { rc = SA_EIO; break; }
        }
    }
    if (fclose(f) != 0 && rc == SA_OK) rc = SA_EIO;
    return rc;
}

// the double nearest num / den (den > 0), by long division: 64 significant bits and a sticky bit, rounded to 53 bits, ties to even
static double kt_ratio(unsigned __int128 num, unsigned __int128 den) {
    if (num == 0) return 0.0;
    unsigned __int128 q = num / den, r = num % den;
    int e = 0;   // value = q * 2^-e + r / den * 2^-e
    while (q < ((unsigned __int128) 1 << 64)) {   // (at least 65 significant bits in q)
        q <<= 1;
        r <<= 1;
        if (r >= den) { q |= 1; r -= den; }
        e++;
    }
    int nb = 0;
    for (unsigned __int128 z = q; z; z >>= 1) nb++;
    const int drop = nb - 53;
    unsigned __int128 mant = q >> drop;
    const unsigned __int128 rest = q & (((unsigned __int128) 1 << drop) - 1), half = (unsigned __int128) 1 << (drop - 1);
    const bool sticky = r != 0;
    if (rest > half || (rest == half && (sticky || (mant & 1)))) mant++;
    return ldexp((double) (unsigned long long) mant, drop - e);
}

extern "C" int sa_kmer_table_stats(const sa_kmer_table_t *t, int strand, int use_median, sa_kmer_stat_t *out, double *kernel_ms_out) {
    if (!t || !out || (strand != 0 && strand != 1)) return SA_EINVAL;
    sa_kmer_table *T = const_cast<sa_kmer_table *>(t);
    std::lock_guard<std::mutex> g(T->mu);
    const long long nk = t->n_kmers;
    std::vector<KtRaw> raw((size_t) nk);
    int rc = SA_OK;
    KtRaw *d = nullptr;
    float kms = 0;
    if (hipSetDevice(t->device) != hipSuccess) return SA_ENODEVICE;
    SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &d, sizeof(KtRaw) * (size_t) nk, t->device));
    SA_HIP_GOTO_DONE(hipEventRecord(T->e0, 0));
    hipLaunchKernelGGL(k_kt_stats, dim3((unsigned) nk), dim3(KT_STATS_THREADS), 0, 0, t->side[strand].d_rows, t->side[strand].d_off,
                       use_median ? 1 : 0, d);
    SA_HIP_GOTO_DONE(hipEventRecord(T->e1, 0));
    SA_HIP_GOTO_DONE(hipGetLastError());
    SA_HIP_GOTO_DONE(hipMemcpy(raw.data(), d, sizeof(KtRaw) * (size_t) nk, hipMemcpyDeviceToHost));
    SA_HIP_GOTO_DONE(hipEventElapsedTime(&kms, T->e0, T->e1));
    if (kernel_ms_out) *kernel_ms_out = (double) kms;
    for (long long km = 0; km < nk; km++) {
        const KtRaw &R = raw[(size_t) km];
        sa_kmer_stat_t &o = out[km];
        o.n = R.n;
        o.m = o.s = 0.0;
        if (R.n == 0) continue;
        if (use_median) {
            o.m = (double) R.med2 / 2e6;
            o.s = ((double) R.mad4 / 4e6) / 0.6744897501960817;
        } else {
            o.m = (double) R.S / ((double) R.n * 1e6);
            const unsigned __int128 Q = ((unsigned __int128) R.q_hi << 64) | R.q_lo;
            const unsigned __int128 aS = (unsigned __int128) (R.S < 0 ? -(__int128) R.S : (__int128) R.S);
            const unsigned __int128 V = (unsigned __int128) R.n * Q - aS * aS;   // >= 0 (Cauchy-Schwarz)
            const unsigned __int128 D = (unsigned __int128) R.n * (unsigned __int128) R.n * (unsigned __int128) 1000000000000ull;
            o.s = sqrt(kt_ratio(V, D));
        }
    }
done:
    g_sa_pool.put(SaPool::DEVICE, d);
    return rc;
}

// ---- Gaussian mixtures over a k-mer's descaled event means (mixture_model.py:42-186) ---------------------------------------------
// fit_model_to_kmer_dist / get_nanopore_gauss_mixture fit sklearn's GaussianMixture to the rows of one k-mer; here the same EM
// (sklearn's fit with n_init = 1: E-step, M-step, |change of the mean log-likelihood| < tol) runs on the device from a
// deterministic start, one work-group per job, the loop and its convergence test included.  x_i = units_i / 1e6.
//   order      a fit must be a function of the table's contents only, but a segment lies in arrival order (atomics).  Every
//              fitted segment is therefore put into key order first (keys are unique): a bitonic sort in LDS for a segment of
//              at most KT_MIX_LDS_ROWS rows, rocPRIM's segmented radix sort into a copy in HBM for the others
//   sums       thread t adds rows t, t + 256, ... in that order; a wave's 64 partial sums are added by a shuffle tree and the
//              four waves' sums as (w0 + w1) + (w2 + w3): the same rows give the same bits
//   centring   rows are held as (units - c) / 1e6 with c the midpoint of the k-mer's smallest and largest units (an integer).
//              An iteration is one pass: the E-step's t = x - mean_c is also what the M-step sums (R = sum r, S1 = sum r t,
//              S2 = sum r t^2), so the new mean is the old one plus d = (S1 - 10 eps mean) / nk and the new variance
//              (S2 - 2 d S1 + d^2 R) / nk: sum r x / nk and sum r (x - mean)^2 / nk written out.  Shifting by the component's own
//              mean, not by a constant of the k-mer, keeps the rounding of the variance relative to the variance: a
//              component that has shrunk onto one row has var = reg_covar = 1e-6, and a constant shift leaves an error of
//              eps (x - c)^2 ~ 1e-14 there, 1e-8 of it
//   LDS        KT_MIX_LDS_ROWS = 2048 rows: 16 KiB of keys and 16 KiB of values per work-group, four work-groups of 256
//              threads per CU (160 KiB); a larger segment is read from its sorted copy in HBM once per iteration
//   start      hard labels min(K - 1, floor(K (x - lo) / (hi - lo))) and one M-step on them, or the caller's weights, means
//              and sds; either way the loop starts from (weight, mean, sd) in the caller's units, so that the default start
//              handed back in as an explicit one gives the same bits
#define KT_MIX_THREADS 256
#define KT_MIX_LDS_ROWS 2048
#define KT_MIX_MAXK 4
#define KT_MIX_EPS10 (10.0 * 2.220446049250313e-16)

struct KtMixJob {
    long long a, n;             // the k-mer's segment of the table
    long long so;               // n > KT_MIX_LDS_ROWS: where its sorted units lie in the copy
    int kmer, pad;
};

// sums of v[0 .. NV) over the block, in every thread (fixed tree; s_red: 4 x NV doubles)
template <int NV>
__device__ static inline void kt_mix_sum(double (&v)[NV], double *s_red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; q++) {
        double x = v[q];
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
        v[q] = x;
    }
    __syncthreads();   // (the readers of the previous sums are done)
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NV; q++) s_red[wave * NV + q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; q++) v[q] = (s_red[q] + s_red[NV + q]) + (s_red[2 * NV + q] + s_red[3 * NV + q]);
}

// M-step from R_c = sum r, S1_c = sum r t, S2_c = sum r t^2 with t = x - m_c (the component's mean before the step, centred;
// cd: the centre).  sum r x / nk moves the mean by d = (S1 - 10 eps (m + cd)) / nk, and sum r (x - mean)^2 = S2 - 2 d S1 + d^2 R.
template <int K>
__device__ static inline void kt_mix_mstep(const double *v, double reg, double cd, double *w, double *m, double *sd) {
    double nk[K], tot = 0;
#pragma unroll
    for (int c = 0; c < K; c++) {
        const double R = v[3 * c], S1 = v[3 * c + 1], S2 = v[3 * c + 2];
        nk[c] = R + KT_MIX_EPS10;
        const double d = (S1 - KT_MIX_EPS10 * (m[c] + cd)) / nk[c];
        double var = (S2 - 2.0 * d * S1 + d * d * R) / nk[c];
        if (var < 0) var = 0;   // (rounding, when every row of the component has one value)
        m[c] += d;
        sd[c] = sqrt(var + reg);
        tot += nk[c];
    }
#pragma unroll
    for (int c = 0; c < K; c++) w[c] = nk[c] / tot;
}

__global__ __launch_bounds__(KT_MIX_THREADS) void k_kt_mix_gather(const KtRow *__restrict__ rows, const KtMixJob *__restrict__ jobs,
                                                                  const int *__restrict__ large, unsigned long long *__restrict__ keys,
                                                                  long long *__restrict__ units) {
    const KtMixJob J = jobs[large[blockIdx.x]];
    for (long long i = threadIdx.x; i < J.n; i += KT_MIX_THREADS) {
        const KtRow r = rows[J.a + i];
        keys[J.so + i] = r.key;
        units[J.so + i] = r.desc;
    }
}

// job blockIdx.x.  init: n_jobs x 3K doubles (weights, means, sds) or null.  start_out (n_jobs x 3K, or null): the start is
// written there and nothing is fitted.
template <int K>
__global__ __launch_bounds__(KT_MIX_THREADS) void k_kt_mixture(const KtRow *__restrict__ rows, const long long *__restrict__ sorted,
                                                               const KtMixJob *__restrict__ jobs, sa_mixture_params_t P,
                                                               const double *__restrict__ init, double *__restrict__ start_out,
                                                               sa_mixture_fit_t *__restrict__ out) {
    constexpr int NV = 3 * K + 1;
    __shared__ unsigned long long s_key[KT_MIX_LDS_ROWS];
    __shared__ long long s_val[KT_MIX_LDS_ROWS];   // units, then the bits of the centred doubles
    __shared__ double s_red[4 * NV];
    __shared__ long long s_mm[8];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const KtMixJob J = jobs[blockIdx.x];
    const long long n = J.n;
    sa_mixture_fit_t F;
    memset(&F, 0, sizeof F);
    F.n = n;
    F.kmer_id = J.kmer;
    if (n < K) {
        F.status = 1;
        if (t == 0) out[blockIdx.x] = F;
        return;
    }
    const bool lds = n <= KT_MIX_LDS_ROWS;
    const long long *src = sorted + (lds ? 0 : J.so);
    if (lds) {   // key order: bitonic sort, descending, of (key + 1, units); the padding (key 0) ends up behind the rows
        int p2 = 1;
        while (p2 < n) p2 <<= 1;
        for (int i = t; i < p2; i += KT_MIX_THREADS) {
            if (i < n) {
                const KtRow r = rows[J.a + i];
                s_key[i] = r.key + 1ull;
                s_val[i] = r.desc;
            } else {
                s_key[i] = 0;
                s_val[i] = 0;
            }
        }
        __syncthreads();
        for (int k2 = 2; k2 <= p2; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int i = t; i < p2; i += KT_MIX_THREADS) {
                    const int p = i ^ j;
                    if (p <= i) continue;
                    const unsigned long long ki = s_key[i], kp = s_key[p];
                    if ((i & k2) == 0 ? ki < kp : ki > kp) {
                        s_key[i] = kp; s_key[p] = ki;
                        const long long u = s_val[i];
                        s_val[i] = s_val[p]; s_val[p] = u;
                    }
                }
                __syncthreads();
            }
    }
    // smallest and largest units (integers: any order gives the same)
    long long lo = 0x7fffffffffffffffll, hi = -0x7fffffffffffffffll - 1;
    for (long long i = t; i < n; i += KT_MIX_THREADS) {
        const long long u = lds ? s_val[i] : src[i];
        lo = u < lo ? u : lo;
        hi = u > hi ? u : hi;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const long long a = __shfl_down(lo, o), b = __shfl_down(hi, o);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if (lane == 0) { s_mm[2 * wave] = lo; s_mm[2 * wave + 1] = hi; }
    __syncthreads();
    lo = s_mm[0]; hi = s_mm[1];
    for (int q = 1; q < 4; q++) {
        lo = s_mm[2 * q] < lo ? s_mm[2 * q] : lo;
        hi = s_mm[2 * q + 1] > hi ? s_mm[2 * q + 1] : hi;
    }
    const long long cu = lo + (hi - lo) / 2;
    const double cd = (double) cu / 1e6;
    double w[K], m[K], sd[K], v[NV];
    if (init) {
#pragma unroll
        for (int c = 0; c < K; c++) {
            w[c] = init[(size_t) blockIdx.x * 3 * K + c];
            m[c] = init[(size_t) blockIdx.x * 3 * K + K + c];
            sd[c] = init[(size_t) blockIdx.x * 3 * K + 2 * K + c];
        }
    } else {
        // the labels' M-step as it is written, in two passes: means first, then the squares about them
        const double xlo = (double) lo / 1e6, xhi = (double) hi / 1e6;
        auto label_of = [&](long long u) {
            if (hi == lo) return 0;
            const double f = floor((double) K * ((double) u / 1e6 - xlo) / (xhi - xlo));
            return f < (double) (K - 1) ? (int) f : K - 1;
        };
#pragma unroll
        for (int q = 0; q < NV; q++) v[q] = 0;
        for (long long i = t; i < n; i += KT_MIX_THREADS) {
            const long long u = lds ? s_val[i] : src[i];
            const int label = label_of(u);
            const double xc = (double) (u - cu) / 1e6;
#pragma unroll
            for (int c = 0; c < K; c++) {
                const double r = label == c ? 1.0 : 0.0;
                v[3 * c] += r;
                v[3 * c + 1] += r * xc;
            }
        }
        kt_mix_sum<NV>(v, s_red);
        double nk[K], tot = 0;
#pragma unroll
        for (int c = 0; c < K; c++) {
            nk[c] = v[3 * c] + KT_MIX_EPS10;
            m[c] = (v[3 * c + 1] - KT_MIX_EPS10 * cd) / nk[c];
            tot += nk[c];
        }
#pragma unroll
        for (int q = 0; q < NV; q++) v[q] = 0;
        for (long long i = t; i < n; i += KT_MIX_THREADS) {
            const long long u = lds ? s_val[i] : src[i];
            const int label = label_of(u);
            const double xc = (double) (u - cu) / 1e6;
#pragma unroll
            for (int c = 0; c < K; c++) v[c] += label == c ? (xc - m[c]) * (xc - m[c]) : 0.0;
        }
        kt_mix_sum<NV>(v, s_red);
#pragma unroll
        for (int c = 0; c < K; c++) {
            w[c] = nk[c] / tot;
            sd[c] = sqrt(v[c] / nk[c] + P.reg_covar);
            m[c] += cd;
        }
    }
    if (start_out) {
        if (t == 0)
            for (int c = 0; c < K; c++) {
                start_out[(size_t) blockIdx.x * 3 * K + c] = w[c];
                start_out[(size_t) blockIdx.x * 3 * K + K + c] = m[c];
                start_out[(size_t) blockIdx.x * 3 * K + 2 * K + c] = sd[c];
            }
        return;
    }
#pragma unroll
    for (int c = 0; c < K; c++) m[c] -= cd;
    if (lds) {   // the rows as centred doubles, once
        __syncthreads();
        for (int i = t; i < n; i += KT_MIX_THREADS) s_val[i] = __double_as_longlong((double) (s_val[i] - cu) / 1e6);
        __syncthreads();
    }
    double lb = -INFINITY;
    int it = 0, converged = 0;
    while (it < P.max_iter) {
        it++;
        const double prev = lb;
        double off[K];
#pragma unroll
        for (int c = 0; c < K; c++) off[c] = log(w[c]) - log(sd[c]);
#pragma unroll
        for (int q = 0; q < NV; q++) v[q] = 0;
        for (long long i = t; i < n; i += KT_MIX_THREADS) {
            const double x = lds ? __longlong_as_double(s_val[i]) : (double) (src[i] - cu) / 1e6;
            double lp[K], tc[K], mx = -INFINITY;
#pragma unroll
            for (int c = 0; c < K; c++) {
                tc[c] = x - m[c];
                const double z = tc[c] / sd[c];
                lp[c] = -0.5 * (1.8378770664093453 + z * z) + off[c];
                mx = lp[c] > mx ? lp[c] : mx;
            }
            double s = 0;
#pragma unroll
            for (int c = 0; c < K; c++) s += exp(lp[c] - mx);
            const double norm = mx + log(s);
#pragma unroll
            for (int c = 0; c < K; c++) {
                const double r = exp(lp[c] - norm);
                v[3 * c] += r;
                v[3 * c + 1] += r * tc[c];
                v[3 * c + 2] += r * tc[c] * tc[c];
            }
            v[3 * K] += norm;
        }
        kt_mix_sum<NV>(v, s_red);
        lb = v[3 * K] / (double) n;
        kt_mix_mstep<K>(v, P.reg_covar, cd, w, m, sd);
        if (fabs(lb - prev) < P.tol) { converged = 1; break; }
    }
    F.n_iter = it;
    F.converged = converged;
    F.lower_bound = lb;
#pragma unroll
    for (int c = 0; c < K; c++) { F.weight[c] = w[c]; F.mean[c] = m[c] + cd; F.sd[c] = sd[c]; }
    if (t == 0) out[blockIdx.x] = F;
}

template <int K>
static void kt_mix_launch(long long nj, const KtRow *rows, const long long *sorted, const KtMixJob *jobs, const sa_mixture_params_t &P,
                          const double *init, double *start_out, sa_mixture_fit_t *out) {
    hipLaunchKernelGGL(k_kt_mixture<K>, dim3((unsigned) nj), dim3(KT_MIX_THREADS), 0, 0, rows, sorted, jobs, P, init, start_out, out);
}

// the fits (out) or, with start_out, only the start of every job (n_jobs x 3K doubles; a job with fewer rows than components: zeros)
static int kt_mixture(const sa_kmer_table_t *t, int strand, const int32_t *kmer_ids, int64_t n_jobs, const sa_mixture_params_t *p,
                      const double *init, sa_mixture_fit_t *out, double *start_out, double *kernel_ms_out) {
    if (!t || !p || (!out && !start_out) || (strand != 0 && strand != 1) || n_jobs < 0) return SA_EINVAL;
    if (p->n_components < 1 || p->n_components > KT_MIX_MAXK || p->max_iter < 1 || !(p->tol >= 0) || !isfinite(p->tol) ||
        !(p->reg_covar >= 0) || !isfinite(p->reg_covar))
        return SA_EINVAL;
    const int K = p->n_components;
    const long long nj = kmer_ids ? (long long) n_jobs : t->n_kmers;
    if (nj > 0x7fffffffll) return SA_EUNSUPPORTED;
    for (long long j = 0; kmer_ids && j < nj; j++)
        if (kmer_ids[j] < 0 || kmer_ids[j] >= t->n_kmers) return SA_EINVAL;
    for (long long q = 0; init && q < nj * 3 * K; q++) {
        const bool is_mean = (q % (3 * K)) / K == 1;
        if (!isfinite(init[q]) || (!is_mean && !(init[q] > 0))) return SA_EINVAL;
    }
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (nj == 0) return SA_OK;
    sa_kmer_table *T = const_cast<sa_kmer_table *>(t);
    std::lock_guard<std::mutex> g(T->mu);
    const KtSide &S = t->side[strand];
    if (hipSetDevice(t->device) != hipSuccess) return SA_ENODEVICE;
    std::vector<long long> off((size_t) t->n_kmers + 1);
    if (hipMemcpy(off.data(), S.d_off, 8 * off.size(), hipMemcpyDeviceToHost) != hipSuccess) return SA_ENODEVICE;
    // jobs; those above the LDS cap get a place in the sorted copy
    std::vector<KtMixJob> jobs((size_t) nj);
    std::vector<int> large;
    std::vector<unsigned> seg_begin, seg_end;
    long long n_large = 0;
    for (long long j = 0; j < nj; j++) {
        const long long km = kmer_ids ? kmer_ids[j] : j;
        KtMixJob &J = jobs[(size_t) j];
        J.a = off[(size_t) km]; J.n = off[(size_t) km + 1] - J.a; J.so = 0; J.kmer = (int) km; J.pad = 0;
        if (J.n > KT_MIX_LDS_ROWS && J.n >= K) {
            J.so = n_large;
            large.push_back((int) j);
            seg_begin.push_back((unsigned) n_large);
            n_large += J.n;
            if (n_large > 0xffffffffll) return SA_EUNSUPPORTED;   // (the segmented sort counts rows in 32 bits)
            seg_end.push_back((unsigned) n_large);
        }
    }
    const size_t nl = large.size(), n_init = init ? (size_t) nj * 3 * K : 0, n_start = start_out ? (size_t) nj * 3 * K : 0;
    SaLayout L;
    const size_t o_jobs = L.add(sizeof(KtMixJob) * (size_t) nj), o_large = L.add(4 * nl), o_beg = L.add(4 * nl), o_end = L.add(4 * nl),
                 o_init = L.add(8 * n_init), o_up = L.end, o_out = L.add(sizeof(sa_mixture_fit_t) * (size_t) nj), o_start = L.add(8 * n_start),
                 o_k0 = L.add(8 * (size_t) n_large), o_k1 = L.add(8 * (size_t) n_large), o_u0 = L.add(8 * (size_t) n_large),
                 o_u1 = L.add(8 * (size_t) n_large), bytes = L.end;
    int rc = SA_OK;
    char *h = nullptr, *d = nullptr;
    void *d_tmp = nullptr;
    size_t tmp_bytes = 0;
    float kms = 0;
    if (g_sa_pool.get(SaPool::PINNED, (void **) &h, o_up, t->device) != hipSuccess) return SA_ENOMEM;
    {
        memcpy(h + o_jobs, jobs.data(), sizeof(KtMixJob) * (size_t) nj);
        if (nl) {
            memcpy(h + o_large, large.data(), 4 * nl);
            memcpy(h + o_beg, seg_begin.data(), 4 * nl);
            memcpy(h + o_end, seg_end.data(), 4 * nl);
        }
        if (n_init) memcpy(h + o_init, init, 8 * n_init);
        SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &d, bytes, t->device));
        SA_HIP_GOTO_DONE(hipMemcpy(d, h, o_up, hipMemcpyHostToDevice));
        const KtMixJob *dj = (const KtMixJob *) (d + o_jobs);
        unsigned long long *k0 = (unsigned long long *) (d + o_k0), *k1 = (unsigned long long *) (d + o_k1);
        long long *u0 = (long long *) (d + o_u0), *u1 = (long long *) (d + o_u1);
        const unsigned *beg = (const unsigned *) (d + o_beg), *end = (const unsigned *) (d + o_end);
        if (nl) {
            SA_HIP_GOTO_DONE(rocprim::segmented_radix_sort_pairs_desc(nullptr, tmp_bytes, k0, k1, u0, u1, (unsigned) n_large, (unsigned) nl, beg,
                                                                      end, 0, 64 - 4, (hipStream_t) 0));
            SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, &d_tmp, tmp_bytes, t->device));
        }
        SA_HIP_GOTO_DONE(hipEventRecord(T->e0, 0));
        if (nl) {
            hipLaunchKernelGGL(k_kt_mix_gather, dim3((unsigned) nl), dim3(KT_MIX_THREADS), 0, 0, S.d_rows, dj, (const int *) (d + o_large), k0, u0);
            SA_HIP_GOTO_DONE(rocprim::segmented_radix_sort_pairs_desc(d_tmp, tmp_bytes, k0, k1, u0, u1, (unsigned) n_large, (unsigned) nl, beg,
                                                                      end, 0, 64 - 4, (hipStream_t) 0));
        }
        const double *d_init = n_init ? (const double *) (d + o_init) : nullptr;
        double *d_start = n_start ? (double *) (d + o_start) : nullptr;
        sa_mixture_fit_t *d_out = (sa_mixture_fit_t *) (d + o_out);
        if (n_start) SA_HIP_GOTO_DONE(hipMemsetAsync(d_start, 0, 8 * n_start, 0));
        switch (K) {
            case 1: kt_mix_launch<1>(nj, S.d_rows, u1, dj, *p, d_init, d_start, d_out); break;
            case 2: kt_mix_launch<2>(nj, S.d_rows, u1, dj, *p, d_init, d_start, d_out); break;
            case 3: kt_mix_launch<3>(nj, S.d_rows, u1, dj, *p, d_init, d_start, d_out); break;
            default: kt_mix_launch<4>(nj, S.d_rows, u1, dj, *p, d_init, d_start, d_out); break;
        }
        SA_HIP_GOTO_DONE(hipEventRecord(T->e1, 0));
        SA_HIP_GOTO_DONE(hipGetLastError());
        if (start_out) SA_HIP_GOTO_DONE(hipMemcpy(start_out, d_start, 8 * n_start, hipMemcpyDeviceToHost));
        else SA_HIP_GOTO_DONE(hipMemcpy(out, d_out, sizeof(sa_mixture_fit_t) * (size_t) nj, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(hipEventElapsedTime(&kms, T->e0, T->e1));
        if (kernel_ms_out) *kernel_ms_out = (double) kms;
    }
done:
    if (rc != SA_OK) (void) hipDeviceSynchronize();
    g_sa_pool.put(SaPool::DEVICE, d_tmp);
    g_sa_pool.put(SaPool::DEVICE, d);
    g_sa_pool.put(SaPool::PINNED, h);
    return rc;
}

extern "C" int sa_kmer_table_mixture(const sa_kmer_table_t *t, int strand, const int32_t *kmer_ids, int64_t n_jobs,
                                     const sa_mixture_params_t *p, const double *init, sa_mixture_fit_t *out, double *kernel_ms_out) {
    if (!out) return SA_EINVAL;
    return kt_mixture(t, strand, kmer_ids, n_jobs, p, init, out, nullptr, kernel_ms_out);
}

extern "C" int sa_kmer_table_mixture_start(const sa_kmer_table_t *t, int strand, const int32_t *kmer_ids, int64_t n_jobs,
                                           const sa_mixture_params_t *p, double *init_out) {
    if (!init_out) return SA_EINVAL;
    return kt_mixture(t, strand, kmer_ids, n_jobs, p, nullptr, nullptr, init_out, nullptr);
}

// closest_to_canonical (mixture_model.py:92-104) for two components: strict < against 1000, the first minimal index
extern "C" int sa_mixture_assign(const sa_mixture_fit_t *fit, double canonical_mean, int32_t *match_out, int32_t *other_out,
                                 double *distance_out) {
    if (!fit || fit->status != 0) return SA_EINVAL;
    int min_index = 0;
    double min_distance = 1000;
    for (int i = 0; i < 2; i++) {
        const double distance = fabs(fit->mean[i] - canonical_mean);
        if (distance < min_distance) { min_index = i; min_distance = distance; }
    }
    if (match_out) *match_out = min_index;
    if (other_out) *other_out = 1 - min_index;
    if (distance_out) *distance_out = min_distance;
    return SA_OK;
}

// get_motif_kmer_pairs (mixture_model.py:189-200) over get_motif_kmers (utils/sequenceTools.py:332-374): every window of k
// letters that covers the modified position of the motif, the positions outside the motif filled with every letter of
// `alphabet`; the canonical k-mer has the FIRST occurrence of the new letter replaced (so a flank that holds the new letter
// gives a pair whose canonical half still carries one: the reference's behaviour, kept)
extern "C" int sa_motif_kmer_pairs(int k, const char *canonical_motif, const char *modified_motif, const char *alphabet, char **pairs_out,
                                   int64_t *n_out) {
    if (!canonical_motif || !modified_motif || !pairs_out || !n_out || k < 1 || k > 16) return SA_EINVAL;
    *pairs_out = nullptr;
    *n_out = 0;
    std::string can(canonical_motif), mod(modified_motif), alpha(alphabet ? alphabet : "ATGC");
    for (char &c : can) c = (char) toupper((unsigned char) c);
    for (char &c : mod) c = (char) toupper((unsigned char) c);
    if (can.size() != mod.size() || can.empty() || alpha.empty()) return SA_EINVAL;
    const int len = (int) can.size();
    int pos = -1, n_diff = 0;
    for (int i = 0; i < len; i++) {
        if (!strchr("ATGC", can[(size_t) i])) return SA_EINVAL;
        if (can[(size_t) i] != mod[(size_t) i]) { pos = i; n_diff++; }
    }
    if (n_diff != 1) return SA_EINVAL;
    const char old_c = can[(size_t) pos], new_c = mod[(size_t) pos];
    std::vector<std::pair<std::string, std::string>> pairs;
    for (int i = 0; i < k; i++) {
        const int s = pos + i - k + 1, nf = s < 0 ? -s : 0, nb = s + k > len ? s + k - len : 0;
        const std::string core = mod.substr((size_t) (s < 0 ? 0 : s), (size_t) (k - nf - nb));
        double combos = 1;
        for (int q = 0; q < nf + nb; q++) combos *= (double) alpha.size();
        if (combos * k > 1e7) return SA_EUNSUPPORTED;
        std::vector<int> digit((size_t) (nf + nb), 0);
        for (;;) {
            std::string km;
            for (int q = 0; q < nf; q++) km.push_back(alpha[(size_t) digit[(size_t) q]]);
            km += core;
            for (int q = 0; q < nb; q++) km.push_back(alpha[(size_t) digit[(size_t) (nf + q)]]);
            std::string old_km = km;
            old_km[old_km.find(new_c)] = old_c;
            pairs.emplace_back(old_km, km);
            int q = nf + nb - 1;
            while (q >= 0 && ++digit[(size_t) q] == (int) alpha.size()) digit[(size_t) q--] = 0;
            if (q < 0) break;
        }
    }
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    char *o = (char *) calloc(pairs.size() * 2 * (size_t) (k + 1) + 1, 1);
    if (!o) return SA_ENOMEM;
    for (size_t i = 0; i < pairs.size(); i++) {
        memcpy(o + (2 * i) * (size_t) (k + 1), pairs[i].first.c_str(), (size_t) k);
        memcpy(o + (2 * i + 1) * (size_t) (k + 1), pairs[i].second.c_str(), (size_t) k);
    }
    *pairs_out = o;
    *n_out = (int64_t) pairs.size();
    return SA_OK;
}

// ---- Gaussian kernel density estimate over a k-mer's descaled event means (hiddenMarkovModel.py:654-773) -------------------------
// plot_kmer_distribution fits sklearn's KernelDensity(kernel="gaussian", bandwidth=h) to the rows of one k-mer and draws
// exp(score_samples(x)); here score_samples (rtol = atol = 0) for any set of jobs and query points, in fp64.  x_i = units_i / 1e6.
//   definition r = 1 / h (one correctly rounded division); for a query point q: d_i = q - x_i, z_i = d_i r, e_i = -0.5 (z_i z_i);
//              E = the largest e_i (the nearest row's, found as min |d_i|: every operation is monotone in |d_i|);
//              S = sum of exp(e_i - E) over the rows with e_i - E >= -KT_KDE_CUT;
//              log density = (E + log S) - ((log n + log h) + log(2 pi) / 2)
//   order      S is ONE accumulator per query point, started at 0.0, the rows added in ascending order of their units (equal units
//              give equal terms, so ties need no rule).  A segment lies in arrival order, so every job's units are first copied and
//              sorted (rocPRIM's segmented radix sort); the value of a (k-mer, q, h) is therefore a function of the table's contents
//              only: not of the other jobs or points of the call, of the chunking, or of how the table was filled
//   cut        a row further than KT_KDE_CUT = 64 below the largest exponent is not added; it is part of the definition and is
//              tested per (row, point), so it does not depend on tiling.  What it leaves out is less than n exp(-64) of a sum that
//              is at least 1: below 7e-19 for the n < 2^32 a job may have, less than a hundredth of an ulp.  The test is also what
//              makes the kernel fast: the loop is bound by fp64 exp, and a wave whose 64 adjacent points all fail it for a row
//              branches around the exp (SA_KDE_NO_SKIP=1, a measurement hook, evaluates every exp and multiplies by 0 or 1: same bits)
//   finite     E is subtracted before exp, so the result is finite for every q for which ((q - x) r)^2 does not overflow
//   shape      one work-group of 256 threads per (job, tile of 512 query points); a thread owns points t and t + 256 of the tile in
//              registers, so each of its two slots is 64 adjacent points per wave.  The sorted rows go through LDS as doubles in
//              chunks of KT_KDE_LDS_ROWS (16 KiB) and are read as broadcasts; two sweeps: min |d|, then the sum
//   output     jobs are taken in chunks whose n_jobs x n_x block fits a device slab (8 M doubles; SA_KDE_SLAB: a test and
//              measurement hook); each chunk is gathered, sorted, evaluated and copied to the caller's ordinary host memory
#define KT_KDE_THREADS 256
#define KT_KDE_PTS 2
#define KT_KDE_TILE (KT_KDE_THREADS * KT_KDE_PTS)
#define KT_KDE_LDS_ROWS 2048
#define KT_KDE_CUT 64.0
#define KT_KDE_HALF_LOG_2PI 0.9189385332046727
#define KT_KDE_CHUNK_ROWS (1ll << 28)

struct KtKdeJob {
    long long a, n;             // the k-mer's segment of the table
    long long so;               // where its units lie in the chunk's copy
};

__global__ __launch_bounds__(KT_KDE_THREADS) void k_kt_kde_gather(const KtRow *__restrict__ rows, const KtKdeJob *__restrict__ jobs,
                                                                  long long *__restrict__ units) {
    const KtKdeJob J = jobs[blockIdx.x];
    for (long long i = threadIdx.x; i < J.n; i += KT_KDE_THREADS) units[J.so + i] = rows[J.a + i].desc;
}

// block b: job b / n_tiles, tile b % n_tiles.  out: n_jobs x n_x
template <bool SKIP>
__global__ __launch_bounds__(KT_KDE_THREADS) void k_kt_kde(const long long *__restrict__ sorted, const KtKdeJob *__restrict__ jobs,
                                                           const double *__restrict__ x, long long n_x, long long n_tiles, double inv_h,
                                                           double log_h, double *__restrict__ out) {
    __shared__ double s_x[KT_KDE_LDS_ROWS];
    const long long job = (long long) blockIdx.x / n_tiles, tile = (long long) blockIdx.x % n_tiles;
    const int t = threadIdx.x;
    const KtKdeJob J = jobs[job];
    long long qi[KT_KDE_PTS];
    bool ok[KT_KDE_PTS];
    double q[KT_KDE_PTS], dmin[KT_KDE_PTS], emax[KT_KDE_PTS], s[KT_KDE_PTS];
#pragma unroll
    for (int p = 0; p < KT_KDE_PTS; p++) {
        qi[p] = tile * KT_KDE_TILE + (long long) p * KT_KDE_THREADS + t;
        ok[p] = qi[p] < n_x;
        q[p] = ok[p] ? x[qi[p]] : 0.0;
        dmin[p] = INFINITY;
        emax[p] = 0.0;
        s[p] = 0.0;
    }
    if (J.n == 0) {
#pragma unroll
        for (int p = 0; p < KT_KDE_PTS; p++)
            if (ok[p]) out[(size_t) job * (size_t) n_x + (size_t) qi[p]] = -INFINITY;
        return;
    }
    const long long *src = sorted + J.so;
    for (int sweep = 0; sweep < 2; sweep++) {
        if (sweep == 1) {
#pragma unroll
            for (int p = 0; p < KT_KDE_PTS; p++) {
                const double z = dmin[p] * inv_h;
                emax[p] = -0.5 * (z * z);
            }
        }
        for (long long base = 0; base < J.n; base += KT_KDE_LDS_ROWS) {
            const int c = (int) (J.n - base < KT_KDE_LDS_ROWS ? J.n - base : KT_KDE_LDS_ROWS);
            __syncthreads();   // (the readers of the previous chunk are done)
            for (int i = t; i < c; i += KT_KDE_THREADS) s_x[i] = (double) src[base + i] / 1e6;
            __syncthreads();
            if (sweep == 0) {
                for (int i = 0; i < c; i++) {
                    const double xi = s_x[i];
#pragma unroll
                    for (int p = 0; p < KT_KDE_PTS; p++) {
                        const double d = fabs(q[p] - xi);
                        dmin[p] = d < dmin[p] ? d : dmin[p];
                    }
                }
            } else {
                for (int i = 0; i < c; i++) {
                    const double xi = s_x[i];
#pragma unroll
                    for (int p = 0; p < KT_KDE_PTS; p++) {
                        const double z = (q[p] - xi) * inv_h;
                        const double e = -0.5 * (z * z) - emax[p];
                        const bool in = ok[p] && e >= -KT_KDE_CUT;
                        if (SKIP) {
                            if (in) s[p] += exp(e);
                        } else {
                            s[p] += exp(in ? e : -KT_KDE_CUT) * (in ? 1.0 : 0.0);
                        }
                    }
                }
            }
        }
    }
    const double norm = (log((double) J.n) + log_h) + KT_KDE_HALF_LOG_2PI;
#pragma unroll
    for (int p = 0; p < KT_KDE_PTS; p++)
        if (ok[p]) out[(size_t) job * (size_t) n_x + (size_t) qi[p]] = (emax[p] + log(s[p])) - norm;
}

// Slab size in doubles (see "output" above).  A chunk holds at least one job whatever the size.
static size_t kt_kde_slab_doubles() {
    if (const char *e = getenv("SA_KDE_SLAB")) {
        const long long v = atoll(e);
        if (v > 0) return (size_t) v;
    }
    return (size_t) 8 << 20;
}

extern "C" int sa_kmer_table_kde(const sa_kmer_table_t *t, int strand, const int32_t *kmer_ids, int64_t n_jobs, const double *x, int64_t n_x,
                                 double bandwidth, double *log_density_out, int64_t *n_rows_out, double *kernel_ms_out) {
    if (!t || !x || !log_density_out || (strand != 0 && strand != 1) || n_jobs < 0 || n_x < 1 || !isfinite(bandwidth) || !(bandwidth > 0))
        return SA_EINVAL;
    for (int64_t i = 0; i < n_x; i++)
        if (!isfinite(x[i])) return SA_EINVAL;
    const long long nj = kmer_ids ? (long long) n_jobs : t->n_kmers;
    for (long long j = 0; kmer_ids && j < nj; j++)
        if (kmer_ids[j] < 0 || kmer_ids[j] >= t->n_kmers) return SA_EINVAL;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (nj == 0) return SA_OK;
    const long long n_tiles = ((long long) n_x + KT_KDE_TILE - 1) / KT_KDE_TILE;
    if (n_tiles > 0x7fffffffll) return SA_EUNSUPPORTED;
    sa_kmer_table *T = const_cast<sa_kmer_table *>(t);
    std::lock_guard<std::mutex> g(T->mu);
    const KtSide &S = t->side[strand];
    if (hipSetDevice(t->device) != hipSuccess) return SA_ENODEVICE;
    std::vector<long long> off((size_t) t->n_kmers + 1);
    if (hipMemcpy(off.data(), S.d_off, 8 * off.size(), hipMemcpyDeviceToHost) != hipSuccess) return SA_ENODEVICE;
    // chunks of jobs: the output block within the slab, the rows within what one sort takes, the grid within 2^31 blocks
    const size_t slab = kt_kde_slab_doubles();
    const long long jobs_per_launch = 0x7fffffffll / n_tiles;
    std::vector<long long> chunk_first(1, 0);
    size_t max_jobs = 0, max_rows = 0;
    {
        long long rows = 0, first = 0;
        for (long long j = 0; j < nj; j++) {
            const long long km = kmer_ids ? kmer_ids[j] : j, n = off[(size_t) km + 1] - off[(size_t) km];
            if (n > 0xffffffffll) return SA_EUNSUPPORTED;   // (the segmented sort counts rows in 32 bits)
            if (j > first && ((size_t) (j - first + 1) * (size_t) n_x > slab || rows + n > KT_KDE_CHUNK_ROWS || j - first >= jobs_per_launch)) {
                chunk_first.push_back(j);
                first = j;
                rows = 0;
            }
            rows += n;
            max_jobs = std::max(max_jobs, (size_t) (j - first + 1));
            max_rows = std::max(max_rows, (size_t) rows);
            if (n_rows_out) n_rows_out[j] = n;
        }
        chunk_first.push_back(nj);
    }
    const double inv_h = 1.0 / bandwidth, log_h = log(bandwidth);
    const bool skip = !(getenv("SA_KDE_NO_SKIP") && atoi(getenv("SA_KDE_NO_SKIP")) != 0);
    SaLayout L;
    const size_t o_jobs = L.add(sizeof(KtKdeJob) * max_jobs), o_beg = L.add(4 * max_jobs), o_end = L.add(4 * max_jobs), o_up = L.end,
                 o_x = L.add(8 * (size_t) n_x), o_u0 = L.add(8 * max_rows), o_u1 = L.add(8 * max_rows),
                 o_out = L.add(8 * max_jobs * (size_t) n_x), bytes = L.end;
    int rc = SA_OK;
    char *h = nullptr, *d = nullptr;
    void *d_tmp = nullptr;
    size_t tmp_cap = 0;
    double kms = 0;
    if (g_sa_pool.get(SaPool::PINNED, (void **) &h, o_up, t->device) != hipSuccess) return SA_ENOMEM;
    {
        SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &d, bytes, t->device));
        SA_HIP_GOTO_DONE(hipMemcpy(d + o_x, x, 8 * (size_t) n_x, hipMemcpyHostToDevice));
        KtKdeJob *hj = (KtKdeJob *) (h + o_jobs);
        unsigned *hb = (unsigned *) (h + o_beg), *he = (unsigned *) (h + o_end);
        const KtKdeJob *dj = (const KtKdeJob *) (d + o_jobs);
        const unsigned *beg = (const unsigned *) (d + o_beg), *end = (const unsigned *) (d + o_end);
        long long *u0 = (long long *) (d + o_u0), *u1 = (long long *) (d + o_u1);
        double *d_out = (double *) (d + o_out);
        for (size_t c = 0; c + 1 < chunk_first.size(); c++) {
            const long long j0 = chunk_first[c], cj = chunk_first[c + 1] - j0;
            long long rows = 0;
            for (long long j = 0; j < cj; j++) {
                const long long km = kmer_ids ? kmer_ids[j0 + j] : j0 + j;
                hj[j].a = off[(size_t) km]; hj[j].n = off[(size_t) km + 1] - hj[j].a; hj[j].so = rows;
                hb[j] = (unsigned) rows;
                rows += hj[j].n;
                he[j] = (unsigned) rows;
            }
            SA_HIP_GOTO_DONE(hipMemcpy(d, h, o_up, hipMemcpyHostToDevice));
            if (rows) {
                size_t need = 0;
                SA_HIP_GOTO_DONE(rocprim::segmented_radix_sort_keys(nullptr, need, u0, u1, (unsigned) rows, (unsigned) cj, beg, end, 0, 64,
                                                                    (hipStream_t) 0));
                if (need > tmp_cap) {
                    g_sa_pool.put(SaPool::DEVICE, d_tmp);
                    d_tmp = nullptr;
                    tmp_cap = 0;
                    SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, &d_tmp, need, t->device));
                    tmp_cap = need;
                }
            }
            SA_HIP_GOTO_DONE(hipEventRecord(T->e0, 0));
            if (rows) {
                size_t need = tmp_cap;
                hipLaunchKernelGGL(k_kt_kde_gather, dim3((unsigned) cj), dim3(KT_KDE_THREADS), 0, 0, S.d_rows, dj, u0);
                SA_HIP_GOTO_DONE(rocprim::segmented_radix_sort_keys(d_tmp, need, u0, u1, (unsigned) rows, (unsigned) cj, beg, end, 0, 64,
                                                                    (hipStream_t) 0));
            }
            if (skip)
                hipLaunchKernelGGL(k_kt_kde<true>, dim3((unsigned) (cj * n_tiles)), dim3(KT_KDE_THREADS), 0, 0, u1, dj, (const double *) (d + o_x),
                                   (long long) n_x, n_tiles, inv_h, log_h, d_out);
            else
                hipLaunchKernelGGL(k_kt_kde<false>, dim3((unsigned) (cj * n_tiles)), dim3(KT_KDE_THREADS), 0, 0, u1, dj, (const double *) (d + o_x),
                                   (long long) n_x, n_tiles, inv_h, log_h, d_out);
            SA_HIP_GOTO_DONE(hipEventRecord(T->e1, 0));
            SA_HIP_GOTO_DONE(hipGetLastError());
            SA_HIP_GOTO_DONE(hipMemcpy(log_density_out + (size_t) j0 * (size_t) n_x, d_out, 8 * (size_t) cj * (size_t) n_x, hipMemcpyDeviceToHost));
            float seg = 0;
            SA_HIP_GOTO_DONE(hipEventElapsedTime(&seg, T->e0, T->e1));
            kms += (double) seg;
        }
        if (kernel_ms_out) *kernel_ms_out = kms;
    }
done:
    if (rc != SA_OK) (void) hipDeviceSynchronize();
    g_sa_pool.put(SaPool::DEVICE, d_tmp);
    g_sa_pool.put(SaPool::DEVICE, d);
    g_sa_pool.put(SaPool::PINNED, h);
    return rc;
}

// ---- host: Python's repr, the "%f" units, the model writer ----------------------------------------------------------------------
extern "C" int sa_format_py_repr(char *out, double v) {
    if (isnan(v)) return sprintf(out, "nan");
    if (isinf(v)) return sprintf(out, v < 0 ? "-inf" : "inf");
    if (v == 0) return sprintf(out, signbit(v) ? "-0.0" : "0.0");
    // shortest digit string that reads back as v: the correctly rounded one of each length, or its neighbour in the last digit
    // (near a power of two the round-trip interval is lopsided, and the nearest string of a length may miss it while the next
    // one up or down does not)
    char buf[64];
    unsigned long long M = 0;
    int E = 0, P = 0;
    bool found = false;
    for (int p = 0; p <= 16 && !found; p++) {
        snprintf(buf, sizeof buf, "%.*e", p, fabs(v));
        char *ep = strchr(buf, 'e');
        const int ex = atoi(ep + 1);
        unsigned long long m = 0;
        for (char *c = buf; c < ep; c++)
            if (*c >= '0' && *c <= '9') m = m * 10 + (unsigned long long) (*c - '0');
        const unsigned long long cand[3] = {m, m - 1, m + 1};
        for (int q = 0; q < 3 && !found; q++) {
            if (cand[q] == 0) continue;
            snprintf(buf, sizeof buf, "%llue%d", cand[q], ex - p);
            if (strtod(buf, nullptr) == fabs(v)) { M = cand[q]; E = ex - p; P = p; found = true; }
        }
    }
    if (!found) {   // (17 significant digits always read back)
        snprintf(buf, sizeof buf, "%.16e", fabs(v));
        char *ep = strchr(buf, 'e');
        M = 0;
        for (char *c = buf; c < ep; c++)
            if (*c >= '0' && *c <= '9') M = M * 10 + (unsigned long long) (*c - '0');
        E = atoi(ep + 1) - 16;
    }
    (void) P;
    while (M % 10 == 0) { M /= 10; E++; }
    char dg[24];
    const int nd = snprintf(dg, sizeof dg, "%llu", M);
    const int decpt = nd + E;   // value = 0.d1d2... * 10^decpt
    char *w = out;
    if (v < 0) *w++ = '-';
    if (decpt > -4 && decpt <= 16) {   // float_repr_style 'short', format code 'r'
        if (decpt <= 0) {
            *w++ = '0'; *w++ = '.';
            for (int i = 0; i < -decpt; i++) *w++ = '0';
            memcpy(w, dg, (size_t) nd); w += nd;
        } else if (decpt >= nd) {
            memcpy(w, dg, (size_t) nd); w += nd;
            for (int i = nd; i < decpt; i++) *w++ = '0';
            *w++ = '.'; *w++ = '0';
        } else {
            memcpy(w, dg, (size_t) decpt); w += decpt;
            *w++ = '.';
            memcpy(w, dg + decpt, (size_t) (nd - decpt)); w += nd - decpt;
        }
    } else {
        *w++ = dg[0];
        if (nd > 1) { *w++ = '.'; memcpy(w, dg + 1, (size_t) (nd - 1)); w += nd - 1; }
        const int x = decpt - 1;
        w += sprintf(w, "e%c%02d", x < 0 ? '-' : '+', x < 0 ? -x : x);
    }
    *w = 0;
    return (int) (w - out);
}

extern "C" int sa_f6_units(double v, int64_t *units_out, int32_t *neg_zero_out) {
    long long u = 0;
    int nz = 0;
    const int rc = kt_f6_units(v, &u, &nz);
    if (units_out) *units_out = u;
    if (neg_zero_out) *neg_zero_out = nz;
    return rc;
}

__global__ void k_kt_f6(const double *v, long long n, long long *u, int *nz, int *rc) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long a = 0;
    int z = 0;
    rc[i] = kt_f6_units(v[i], &a, &z);
    u[i] = a;
    nz[i] = z;
}
extern "C" int sa_f6_units_device(const double *v, int64_t n, int64_t *units_out, int32_t *neg_zero_out, int32_t *rc_out, int device) {
    if (n < 0 || (n > 0 && (!v || !units_out || !neg_zero_out || !rc_out)) || n > (1ll << 31)) return SA_EINVAL;
    int rc = sa_device_check(device, /* quiet */ true);
    if (rc || n == 0) return rc;
    if (hipSetDevice(device) != hipSuccess) return SA_ENODEVICE;
    char *d = nullptr;
    const size_t o_u = sa_up256(8 * (size_t) n), o_z = sa_up256(o_u + 8 * (size_t) n), o_r = sa_up256(o_z + 4 * (size_t) n);
    if (hipMalloc((void **) &d, o_r + 4 * (size_t) n) != hipSuccess) return SA_ENOMEM;
    SA_HIP_GOTO_DONE(hipMemcpy(d, v, 8 * (size_t) n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_kt_f6, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, (const double *) d, (long long) n, (long long *) (d + o_u),
                       (int *) (d + o_z), (int *) (d + o_r));
    SA_HIP_GOTO_DONE(hipGetLastError());
    SA_HIP_GOTO_DONE(hipMemcpy(units_out, d + o_u, 8 * (size_t) n, hipMemcpyDeviceToHost));
    SA_HIP_GOTO_DONE(hipMemcpy(neg_zero_out, d + o_z, 4 * (size_t) n, hipMemcpyDeviceToHost));
    SA_HIP_GOTO_DONE(hipMemcpy(rc_out, d + o_r, 4 * (size_t) n, hipMemcpyDeviceToHost));
done:
    (void) hipFree(d);
    return rc;
}

static bool kt_read_line_tokens(FILE *f, std::vector<std::string> *tok) {
    tok->clear();
    std::string line;
    int c;
    while ((c = fgetc(f)) != EOF && c != '\n') line.push_back((char) c);
    if (c == EOF && line.empty()) return false;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && isspace((unsigned char) line[i])) i++;
        size_t j = i;
        while (j < line.size() && !isspace((unsigned char) line[j])) j++;
        if (j > i) tok->push_back(line.substr(i, j - i));
        i = j;
    }
    return true;
}

static bool kt_parse(const std::string &s, double *v) {
    char *end = nullptr;
    *v = strtod(s.c_str(), &end);
    return end && *end == 0 && !s.empty();
}

extern "C" int sa_model_write_trained(const char *prior_model_path, const sa_kmer_stat_t *stats, double weight, double min_sd, int mod_only,
                                      const uint8_t *kmer_mask, const char *out_path) {
    if (!prior_model_path || !stats || !out_path) return SA_EINVAL;
    FILE *f = fopen(prior_model_path, "r");
    if (!f) return SA_EIO;
    std::vector<std::string> head, trans, params;
    const bool ok = kt_read_line_tokens(f, &head) && kt_read_line_tokens(f, &trans) && kt_read_line_tokens(f, &params);
    fclose(f);
    if (!ok || head.size() != 4 || trans.size() != 10) return SA_EIO;
    const int n_alpha = atoi(head[1].c_str()), k = atoi(head[3].c_str());
    std::string alphabet = head[2];
    if (n_alpha < 1 || k < 1 || (int) alphabet.size() != n_alpha) return SA_EIO;
    long long nk = 1;
    for (int i = 0; i < k; i++) nk *= n_alpha;
    if ((long long) params.size() != 5 * nk) return SA_EIO;
    std::vector<double> tv(10), pv((size_t) (5 * nk));
    for (int i = 0; i < 10; i++)
        if (!kt_parse(trans[(size_t) i], &tv[(size_t) i])) return SA_EIO;
    for (size_t i = 0; i < pv.size(); i++)
        if (!kt_parse(params[i], &pv[i])) return SA_EIO;
    std::string sorted = alphabet;
    std::sort(sorted.begin(), sorted.end());
    for (long long km = 0; km < nk; km++) {
        const sa_kmer_stat_t &S = stats[km];
        if (S.n <= 0) continue;
        if (kmer_mask && !kmer_mask[km]) continue;
        if (mod_only) {   // k-mers made only of A, C, G, T keep their prior
            bool canonical = true;
            long long id = km;
            for (int i = 0; i < k; i++) {
                const char c = sorted[(size_t) (id % n_alpha)];
                id /= n_alpha;
                canonical = canonical && (c == 'A' || c == 'C' || c == 'G' || c == 'T');
            }
            if (canonical) continue;
        }
        const double n = (double) S.n;
        const double mean0 = pv[(size_t) (5 * km)] * weight, sd0 = pv[(size_t) (5 * km + 1)] * weight;
        const double mu = (S.m * n + mean0) / (n + weight);
        const double sd = std::max((S.s * n + sd0) / (n + weight), min_sd);   // (np.max([a, min_sd]): a NaN would win; none occurs)
        pv[(size_t) (5 * km)] = mu;
        pv[(size_t) (5 * km + 1)] = sd;
        // gaussian_param_to_inv_gaussian_param (hiddenMarkovModel.py:1149-1155): Python's ** is libm's pow, which the compiler would
        // otherwise turn into sd * sd (pow is not correctly rounded: they differ in the last bit now and then)
        volatile double three = 3.0, two = 2.0;
        pv[(size_t) (5 * km + 4)] = pow(mu, (double) three) / pow(sd, (double) two);
    }
    FILE *o = fopen(out_path, "w");
    if (!o) return SA_EIO;
    char num[40];
    fprintf(o, "3\t%d\t%s\t%d\n", n_alpha, alphabet.c_str(), k);
    for (int i = 0; i < 9; i++) {
        sa_format_py_repr(num, tv[(size_t) i]);
        fprintf(o, "%s\t", num);
    }
    sa_format_py_repr(num, tv[9]);
    fprintf(o, "%s\n", num);
    for (size_t i = 0; i < pv.size(); i++) {
        sa_format_py_repr(num, pv[i]);
        fputs(num, o);
        fputc('\t', o);
    }
    fputc('\n', o);
    return fclose(o) == 0 ? SA_OK : SA_EIO;
}
