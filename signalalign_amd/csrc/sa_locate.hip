// sa_locate.hip -- locating a basecalled read in a whole reference on the GPU: contig, strand and diagonal by a vote of exact
// 15-mer matches against a resident index (sa_locate.c builds it).
//
// What it replaces: the part of the `bwa mem` call of the reference's driver (src/signalalign/signalAlignment.py:262-305) that
// finds the locus; the guide stage (sa_guide.c, sa_guide.hip) places and aligns the read inside the window this stage names.
//
// The rules ("Locating a read in a whole reference"; restated in tests/locate_ref.py, and the device equals that field
// for field), all integer:
//   seeds     every 15-mer of ACGT in the read's first read_bases bases, at read position p
//   hits      forward: an entry with the seed's code at reference position r, key r - p; reverse: an entry with the code of the
//             seed's reverse complement, key r + p; a seed with more than max_occ entries on a strand gives none there
//   order     per strand seed by seed in read order, ascending r inside a seed; the first max_hits are kept
//   vote      keys sorted; c_i = keys in [key_i, key_i + span); best = first maximum; votes = c_best; key = keys[best + (votes-1)/2];
//             second_votes = max c_j over key_j < keys[best] - span or key_j >= keys[best] + 2 * span
//   strand    reverse only with strictly more votes
//   contig    the last contig that starts at or before the anchor: key + half forward, key + 14 - half reverse, half =
//             min(read_len, read_bases) / 2, clamped to the reference; pos = key (+ 14 reverse) - the contig's start
//
// Mapping: one workgroup of 256 threads per read.  The read's letter codes sit in LDS; thread t owns the eight seeds at read
// positions 8t .. 8t + 7, on both strands: sixteen independent lookups whose prefix-table loads, binary-search probes and entry
// loads are each issued for all sixteen before any is used (the lookups are dependent gathers: latency is the cost).  A strand's
// occurrence counts go through a block scan, which gives every seed its place in the LDS key buffer -- no atomics, so which hits
// survive the cap does not depend on timing.  The keys are sorted by a bitonic network in LDS, c_i is two binary searches per
// key, a block reduction finds the first maximum.  The strands run one after the other through the same buffer.
//
// Every range taken from the prefix table is clamped to [0, n_entries] before it addresses anything, every probe stays inside
// its range, every key offset is checked against max_hits: a damaged index gives a wrong answer, not an access outside the arrays.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "sa_io.h"
#include "sa_scratch.h"
#include "sa_locate.h"

#define LC_K SA_LOCATE_K
#define LC_THREADS 256
#define LC_SEEDS 8                             // per thread and strand
#define LC_MAX_BASES (LC_THREADS * LC_SEEDS)   // 2048
#define LC_MAX_HITS 8192
#define LC_MAX_LEN (1 << 24)
#define LC_PROBES 32                           // a binary search over fewer than 2^31 entries ends sooner

struct LcJob {
    int code_off, n;   // letter codes of the read's first n bases at codes + code_off
};
struct LcRes {
    int status, contig, reverse, key, votes, second_votes, hits, seeds, repetitive, pad;
    long long pos;
};
struct LcPlan {
    const LcJob *jobs;
    const unsigned char *codes;   // 0..3 = ACGT, 4 = anything else
    const unsigned int *ix_codes;
    const int *ix_pos, *ix_table, *ix_starts;
    LcRes *res;
    int n_entries, q, n_contigs, total;
    int max_occ, span, min_votes, max_hits;
};

struct LcVote {
    int votes, key, second, kept, repetitive, overflow;
};

// exclusive prefix sum of v over the block's threads in thread order; *total the sum.  `part` holds one int per wave.
__device__ __forceinline__ int lc_block_scan(int v, int *part, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    __syncthreads();   // `part` may still be read from the previous use
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < LC_THREADS / 64; w++) {
        const int s = part[w];
        before += w < wave ? s : 0;
        all += s;
    }
    *total = all;
    return before + inc - v;
}

// the largest v over the block (64-bit, unsigned); `part` holds one value per wave
__device__ __forceinline__ unsigned long long lc_block_max(unsigned long long v, unsigned long long *part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    __syncthreads();
    if (lane == 0) part[wave] = v;
    __syncthreads();
    unsigned long long m = part[0];
#pragma unroll
    for (int w = 1; w < LC_THREADS / 64; w++) m = part[w] > m ? part[w] : m;
    return m;
}

// first index in keys[0, n) whose key is >= v
__device__ __forceinline__ int lc_lower_bound(const int *keys, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One strand: first[] / occ[] are this thread's eight seeds' entry ranges (occ 0: no hit), sign -1 forward, +1 reverse.
__device__ LcVote lc_strand(const LcPlan &P, const int (&first)[LC_SEEDS], const int (&occ)[LC_SEEDS], int repetitive_mine, int sign,
                            int *keys, int *part, unsigned long long *part64) {
    const int tid = threadIdx.x, max_hits = P.max_hits, span = P.span;
    LcVote V;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < LC_SEEDS; k++) mine += occ[k];
    int total = 0, rep_total = 0;
    int off = lc_block_scan(mine, part, &total);
    (void) lc_block_scan(repetitive_mine, part, &rep_total);
    V.repetitive = rep_total;
    V.overflow = total > max_hits;
    const int kept = total < max_hits ? total : max_hits;
    V.kept = kept;
    V.votes = 0; V.key = 0; V.second = 0;
    if (kept == 0) return V;   // (uniform: every thread holds the same total)
    int n_pad = 1;
    while (n_pad < kept) n_pad <<= 1;
    for (int i = kept + tid; i < n_pad; i += LC_THREADS) keys[i] = INT_MAX;
    // the hits: round j loads entry j of each of the eight seeds before any key is stored
    int at[LC_SEEDS], most = 0;
#pragma unroll
    for (int k = 0; k < LC_SEEDS; k++) {
        at[k] = off;
        off += occ[k];
        int room = max_hits - at[k];
        room = room < 0 ? 0 : room;
        const int take = occ[k] < room ? occ[k] : room;
        most = take > most ? take : most;
    }
    for (int j = 0; j < most; j++) {
        int r[LC_SEEDS];
#pragma unroll
        for (int k = 0; k < LC_SEEDS; k++) {
            const bool on = j < occ[k] && at[k] + j < max_hits;
            r[k] = on ? P.ix_pos[first[k] + j] : 0;
        }
#pragma unroll
        for (int k = 0; k < LC_SEEDS; k++)
            if (j < occ[k] && at[k] + j < max_hits) keys[at[k] + j] = r[k] + sign * (tid * LC_SEEDS + k);
    }
    __syncthreads();
    // bitonic sort of keys[0, n_pad), ascending
    for (int size = 2; size <= n_pad; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (n_pad >> 1); t += LC_THREADS) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i | stride;
                const int a = keys[i], b = keys[j];
                const bool up = (i & size) == 0;
                if ((a > b) == up) { keys[i] = b; keys[j] = a; }
            }
            __syncthreads();
        }
    }
    // c_i and its first maximum: the count in the high half, the complement of i in the low half
    unsigned long long best = 0;
    for (int i = tid; i < kept; i += LC_THREADS) {
        const int key = keys[i];
        const int c = lc_lower_bound(keys, kept, key + span) - lc_lower_bound(keys, kept, key);
        const unsigned long long v = ((unsigned long long) (unsigned) c << 32) | (unsigned) (INT_MAX - i);
        best = v > best ? v : best;
    }
    best = lc_block_max(best, part64);
    int votes = (int) (best >> 32), bi = INT_MAX - (int) (best & 0xffffffffu);
    bi = bi < 0 ? 0 : (bi >= kept ? kept - 1 : bi);
    votes = votes < 1 ? 1 : (votes > kept - bi ? kept - bi : votes);
    const int kb = keys[bi];
    unsigned long long second = 0;
    for (int i = tid; i < kept; i += LC_THREADS) {
        const int key = keys[i];
        if (key < kb - span || key >= kb + 2 * span) {
            const int c = lc_lower_bound(keys, kept, key + span) - lc_lower_bound(keys, kept, key);
            second = (unsigned long long) c > second ? (unsigned long long) c : second;
        }
    }
    second = lc_block_max(second, part64);
    V.votes = votes;
    V.key = keys[bi + (votes - 1) / 2];
    V.second = (int) second;
    __syncthreads();   // the next strand writes the buffer
    return V;
}

__global__ __launch_bounds__(LC_THREADS) void k_guide_locate(LcPlan P, int n_jobs) {
    __shared__ int keys[LC_MAX_HITS];
    __shared__ unsigned char letters[LC_MAX_BASES + LC_K + LC_SEEDS];
    __shared__ int part[LC_THREADS / 64];
    __shared__ unsigned long long part64[LC_THREADS / 64];
    const int job = blockIdx.x;
    if (job >= n_jobs) return;
    const int tid = threadIdx.x;
    const LcJob J = P.jobs[job];
    const int n = J.n < 0 ? 0 : (J.n > LC_MAX_BASES ? LC_MAX_BASES : J.n);
    const unsigned char *rd = P.codes + J.code_off;
    for (int i = tid; i < (int) sizeof(letters); i += LC_THREADS) letters[i] = i < n ? rd[i] : 4;
    __syncthreads();
    // this thread's seeds: read positions 8 * tid + k; codes of both strands by rolling over 22 letters
    unsigned int code[2][LC_SEEDS];
    bool seed[LC_SEEDS];
    {
        const unsigned int mask = (1u << (2 * LC_K)) - 1u;
        unsigned int f = 0, r = 0;
        int run = 0;
#pragma unroll
        for (int i = 0; i < LC_SEEDS + LC_K - 1; i++) {
            const unsigned int c = letters[tid * LC_SEEDS + i];
            run = c > 3 ? 0 : run + 1;
            f = ((f << 2) | (c & 3u)) & mask;
            r = (r >> 2) | ((3u - (c & 3u)) << (2 * (LC_K - 1)));
            if (i >= LC_K - 1) {
                const int k = i - (LC_K - 1);
                seed[k] = run >= LC_K;   // (a letter past the read's end is 4: such a seed does not exist)
                code[0][k] = f;
                code[1][k] = r;
            }
        }
    }
    int n_seeds_mine = 0;
#pragma unroll
    for (int k = 0; k < LC_SEEDS; k++) n_seeds_mine += seed[k] ? 1 : 0;
    // sixteen lookups: bucket ranges first ...
    const int n_entries = P.n_entries, shift = 2 * LC_K - P.q;
    int lo[2][LC_SEEDS], hi[2][LC_SEEDS];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int k = 0; k < LC_SEEDS; k++) {
            const unsigned int b = code[s][k] >> shift;   // < 2^q: the code has 30 bits
            lo[s][k] = seed[k] ? P.ix_table[b] : 0;
            hi[s][k] = seed[k] ? P.ix_table[b + 1] : 0;
        }
    int l2[2][LC_SEEDS], h2[2][LC_SEEDS];   // the upper bound's search
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int k = 0; k < LC_SEEDS; k++) {
            int a = lo[s][k], z = hi[s][k];
            a = a < 0 ? 0 : (a > n_entries ? n_entries : a);
            z = z < a ? a : (z > n_entries ? n_entries : z);
            lo[s][k] = a; hi[s][k] = z;
            l2[s][k] = a; h2[s][k] = z;
        }
    // ... then the first entry with the code (lo) and the first above it (l2), one probe of every search per round
    for (int round = 0; round < LC_PROBES; round++) {
        bool open = false;
        unsigned int v[2][LC_SEEDS], w[2][LC_SEEDS];
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int k = 0; k < LC_SEEDS; k++) {
                v[s][k] = lo[s][k] < hi[s][k] ? P.ix_codes[(lo[s][k] + hi[s][k]) >> 1] : 0u;
                w[s][k] = l2[s][k] < h2[s][k] ? P.ix_codes[(l2[s][k] + h2[s][k]) >> 1] : 0u;
            }
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int k = 0; k < LC_SEEDS; k++) {
                if (lo[s][k] < hi[s][k]) {
                    const int mid = (lo[s][k] + hi[s][k]) >> 1;
                    if (v[s][k] < code[s][k]) lo[s][k] = mid + 1; else hi[s][k] = mid;
                }
                if (l2[s][k] < h2[s][k]) {
                    const int mid = (l2[s][k] + h2[s][k]) >> 1;
                    if (w[s][k] <= code[s][k]) l2[s][k] = mid + 1; else h2[s][k] = mid;
                }
                open = open || lo[s][k] < hi[s][k] || l2[s][k] < h2[s][k];
            }
        if (!open) break;
    }
    int occ[2][LC_SEEDS], rep[2] = {0, 0};
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int k = 0; k < LC_SEEDS; k++) {
            int o = l2[s][k] - lo[s][k];   // both inside the clamped bucket range
            o = o < 0 ? 0 : o;
            rep[s] += o > P.max_occ ? 1 : 0;
            occ[s][k] = o > P.max_occ ? 0 : o;
        }
    int n_seeds = 0;
    (void) lc_block_scan(n_seeds_mine, part, &n_seeds);
    const LcVote F = lc_strand(P, lo[0], occ[0], rep[0], -1, keys, part, part64);
    const LcVote R = lc_strand(P, lo[1], occ[1], rep[1], +1, keys, part, part64);
    if (tid != 0) return;
    const bool reverse = R.votes > F.votes;
    const LcVote V = reverse ? R : F;
    LcRes res;
    res.status = (F.overflow || R.overflow) ? SA_LOCATE_OVERFLOW : 0;
    res.contig = -1; res.reverse = reverse ? 1 : 0; res.key = V.key; res.votes = V.votes; res.second_votes = V.second;
    res.hits = V.kept; res.seeds = n_seeds; res.repetitive = V.repetitive; res.pad = 0; res.pos = 0;
    if (V.votes < P.min_votes) res.status |= SA_LOCATE_NONE;
    else {
        if (4ll * V.second >= 3ll * V.votes) res.status |= SA_LOCATE_AMBIGUOUS;
        const int half = n / 2;
        long long anchor = reverse ? (long long) V.key + (LC_K - 1) - half : (long long) V.key + half;
        anchor = anchor < 0 ? 0 : (anchor > (long long) P.total - 1 ? (long long) P.total - 1 : anchor);
        int a = 0, z = P.n_contigs;   // first contig that starts after the anchor
        while (a < z) {
            const int mid = (a + z) >> 1;
            if ((long long) P.ix_starts[mid] <= anchor) a = mid + 1; else z = mid;
        }
        const int contig = a > 0 ? a - 1 : 0;
        res.contig = contig;
        res.pos = (long long) V.key + (reverse ? LC_K - 1 : 0) - (long long) P.ix_starts[contig];
    }
    P.res[job] = res;
}

// ---- the index's device copy ---------------------------------------------------------------------------------------------------
extern "C" void sa_locate_drop_device(struct sa_ref_index *idx) {
    if (!idx || idx->device < 0 || !idx->d_codes) return;
    (void) hipSetDevice(idx->device);
    (void) hipFree(idx->d_codes); (void) hipFree(idx->d_pos); (void) hipFree(idx->d_table); (void) hipFree(idx->d_starts);
    idx->d_codes = idx->d_pos = idx->d_table = idx->d_starts = nullptr;
    idx->device_bytes = 0;
}

extern "C" int sa_locate_upload(struct sa_ref_index *idx) {
    int rc = sa_device_check(idx->device);
    if (rc != SA_OK) return rc;
    const size_t n = (size_t) idx->n_entries, nt = ((size_t) 1 << idx->q) + 1, nc = (size_t) idx->n_contigs + 1;
    std::vector<int> starts(nc);
    for (size_t i = 0; i < nc; i++) starts[i] = (int) idx->starts[i];
    SA_HIP_GOTO_DONE(hipSetDevice(idx->device));
    SA_HIP_GOTO_DONE(hipMalloc(&idx->d_codes, 4 * (n ? n : 1)));
    SA_HIP_GOTO_DONE(hipMalloc(&idx->d_pos, 4 * (n ? n : 1)));
    SA_HIP_GOTO_DONE(hipMalloc(&idx->d_table, 4 * nt));
    SA_HIP_GOTO_DONE(hipMalloc(&idx->d_starts, 4 * nc));
    if (n) {
        SA_HIP_GOTO_DONE(hipMemcpy(idx->d_codes, idx->codes, 4 * n, hipMemcpyHostToDevice));
        SA_HIP_GOTO_DONE(hipMemcpy(idx->d_pos, idx->pos, 4 * n, hipMemcpyHostToDevice));
    }
    SA_HIP_GOTO_DONE(hipMemcpy(idx->d_table, idx->table, 4 * nt, hipMemcpyHostToDevice));
    SA_HIP_GOTO_DONE(hipMemcpy(idx->d_starts, starts.data(), 4 * nc, hipMemcpyHostToDevice));
    idx->device_bytes = (int64_t) (8 * n + 4 * nt + 4 * nc);
done:
    if (rc != SA_OK) {
        (void) hipFree(idx->d_codes); (void) hipFree(idx->d_pos); (void) hipFree(idx->d_table); (void) hipFree(idx->d_starts);
        idx->d_codes = idx->d_pos = idx->d_table = idx->d_starts = nullptr;
    }
    return rc;
}

// ---- the batch call --------------------------------------------------------------------------------------------------------------
enum { LC_WS, LC_IN, LC_RES };
static SaScratch g_lc_ws;

extern "C" void sa_locate_release(void) {
    std::lock_guard<std::mutex> guard(g_lc_ws.mu);
    g_lc_ws.release();
}

extern "C" int sa_guide_locate_batch(const sa_ref_index_t *idx, const char *const *reads, const int64_t *read_lens, int64_t n_reads,
                                     const sa_locate_params_t *params, unsigned flags, sa_locate_result_t *out, double *kernel_ms_out) {
    (void) flags;
    if (!idx || n_reads < 0 || (n_reads > 0 && (!reads || !read_lens)) || !out) return SA_EINVAL;
    sa_locate_params_t prm = {2000, 32, 128, 8, LC_MAX_HITS};
    if (params) prm = *params;
    if (prm.read_bases < LC_K || prm.read_bases > LC_MAX_BASES || prm.max_occ < 1 || prm.max_occ > 65536 || prm.span < 1 ||
        prm.span > 8192 || prm.min_votes < 1 || prm.max_hits < 1024 || prm.max_hits > LC_MAX_HITS ||
        (prm.max_hits & (prm.max_hits - 1)) != 0)
        return SA_EINVAL;
    for (int64_t j = 0; j < n_reads; j++)
        if (read_lens[j] < 0 || read_lens[j] > LC_MAX_LEN || (read_lens[j] > 0 && !reads[j])) return SA_EINVAL;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (idx->device < 0) {
        fprintf(stderr, "[signalalign_hip] the reference index was built without a device; this library has no CPU fallback\n");
        return SA_ENODEVICE;
    }
    int rc = sa_device_check(idx->device);
    if (rc != SA_OK) return rc;
    std::vector<LcJob> jobs;
    std::vector<int64_t> who;   // the reads that reach the device: a read shorter than a seed is answered here
    size_t code_tot = 0;
    for (int64_t j = 0; j < n_reads; j++) {
        memset(&out[j], 0, sizeof(out[j]));
        out[j].contig = -1;
        if (read_lens[j] < LC_K) { out[j].status = SA_LOCATE_EMPTY; continue; }
        LcJob J;
        J.n = (int) (read_lens[j] < prm.read_bases ? read_lens[j] : prm.read_bases);
        J.code_off = (int) code_tot;
        code_tot += (size_t) J.n;
        if (code_tot > (size_t) INT_MAX) return SA_EUNSUPPORTED;   // (a million reads of 2048 bases; cut the batch)
        jobs.push_back(J);
        who.push_back(j);
    }
    const size_t nj = jobs.size();
    if (nj == 0) return SA_OK;
    SaScratch &W = g_lc_ws;
    std::lock_guard<std::mutex> guard(W.mu);
    // the upload image: [jobs, letter codes], ONE entry of the device workspace; the results behind it
    SaLayout L;
    const size_t o_codes = sa_up256(sizeof(LcJob) * nj), in_bytes = o_codes + code_tot, res_bytes = sizeof(LcRes) * nj;
    const size_t o_in = L.add(in_bytes), o_res = L.add(res_bytes);
    if ((rc = W.rebind(idx->device)) != SA_OK || (rc = W.pin(LC_IN, in_bytes)) != SA_OK) return rc;
    if ((rc = W.pin(LC_RES, res_bytes)) != SA_OK) return rc;
    if ((rc = W.dev(LC_WS, L.end)) != SA_OK) return rc;
    memcpy(W.at(LC_IN), jobs.data(), sizeof(LcJob) * nj);
    unsigned char *codes = (unsigned char *) W.at(LC_IN) + o_codes;
    sa_parallel_for(nj, [&](size_t k) {
        const char *src = reads[who[k]];
        unsigned char *dst = codes + jobs[k].code_off;
        for (int i = 0; i < jobs[k].n; i++) dst[i] = (unsigned char) sa_base_code(src[i]);
    });
    float kms = 0;
    {
        char *d = (char *) W.at(LC_WS);
        LcPlan P;
        memset(&P, 0, sizeof(P));
        P.jobs = (const LcJob *) (d + o_in);
        P.codes = (const unsigned char *) (d + o_in + o_codes);
        P.ix_codes = (const unsigned int *) idx->d_codes;
        P.ix_pos = (const int *) idx->d_pos;
        P.ix_table = (const int *) idx->d_table;
        P.ix_starts = (const int *) idx->d_starts;
        P.res = (LcRes *) (d + o_res);
        P.n_entries = (int) idx->n_entries; P.q = idx->q; P.n_contigs = (int) idx->n_contigs; P.total = (int) idx->total;
        P.max_occ = prm.max_occ; P.span = prm.span; P.min_votes = prm.min_votes; P.max_hits = prm.max_hits;
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_in, W.at(LC_IN), in_bytes, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(W.time_begin());
        hipLaunchKernelGGL(k_guide_locate, dim3((unsigned) nj), dim3(LC_THREADS), 0, 0, P, (int) nj);
        SA_HIP_GOTO_DONE(W.time_end());
        SA_HIP_GOTO_DONE(hipMemcpyAsync(W.at(LC_RES), d + o_res, res_bytes, hipMemcpyDeviceToHost, 0));
        SA_HIP_GOTO_DONE(hipStreamSynchronize(0));
        SA_HIP_GOTO_DONE(W.time_ms(&kms));
    }
    if (kernel_ms_out) *kernel_ms_out = (double) kms;
    for (size_t k = 0; k < nj; k++) {
        const LcRes &r = ((const LcRes *) W.at(LC_RES))[k];
        sa_locate_result_t &o = out[who[k]];
        o.status = r.status; o.contig = r.contig; o.reverse = r.reverse; o.pos = r.pos; o.key = r.key; o.votes = r.votes;
        o.second_votes = r.second_votes; o.hits = r.hits; o.seeds = r.seeds; o.repetitive = r.repetitive;
    }
done:
    return rc;
}
