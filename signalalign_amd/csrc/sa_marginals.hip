// Single-nucleotide probabilities marginalised over reads on gfx950 -- call_sites_with_marginal_probs and scan_for_proposals
// (src/signalalign/scripts/variantCallingLib.py:114-164, :226-271) over what --snp-step writes per read, kept in HBM across
// batches (include/signalalign_hip.h has the semantics and the two deliberate differences from the reference).
//
// The accumulator is a table over contig positions (sa_contig_acc.h has the layout, the life cycle and the compaction of finish;
// here are the sums and their kernels).  Its store is [sum | depth | tcnt | tloc], per position g: sum[g * 8 + 0..3] the forward
// sum of A, C, G, T, sum[g * 8 + 4..7] the backward sum, depth[g] the rows added so far, and two working arrays of an add,
// tcnt[g] and tloc[g].  A checkpoint covers [sum | depth]: tcnt is zero between calls and tloc is scratch.
//
// The reference adds doubles serially, row after row, so a site's rows of one add call are gathered into a bucket, the bucket
// is put in order and ONE lane folds it, starting from the sums the accumulator holds.  Every row of a call has a unique
// 32-bit ordinal (its rank in (run, strand, given order), made on the host), so a bucket's order does not depend on the
// order in which the atomics handed out its places.  The touched sites are listed, so an add never walks the contigs.
//
// Kernels of an add over n rows {site, ordinal, direction, p[4]}:
//   k_mg_count        one thread per row: ticket[i] = integer atomic increment of tcnt[site]
//   k_mg_alloc        the row with ticket 0 reserves its site's bucket (integer atomic on one cursor; a bucket above
//                     MG_SHORT rows gets a power of two of places) and appends the site to its tier's list
//   k_mg_scatter      one thread per row: entry (ordinal << 32 | row index) at the bucket's place `ticket`
//   k_mg_fold_short   buckets of at most MG_SHORT (16) rows: one lane per site, insertion sort in place, serial fold
//   k_mg_fold_lds     buckets of at most MG_MEDIUM (1024) rows: one wave per site, bitonic sort in LDS, the rows' values
//                     gathered 64 at a time by the wave, folded by lane 0
//   k_mg_fold_global  larger buckets: one block of 256 threads per site, the same bitonic network over the bucket in global
//                     memory (any depth: the bucket's places are a power of two, padded with the largest key), the same fold
// Each fold adds the bucket's rows to depth[] and clears tcnt[] of its site.
// Chained onto a batch (sa_snp_marginals_add_batch): after the position fold that sa_batch_position_calls shares (SaPosFold),
//   k_mg_window       one thread per job: reference_index of the job's smallest and largest x into its group's range
//   k_mg_batch_rows   one wave per job: every position call of the job becomes a row (contig position, window filter, the
//                     letters' probabilities in A, C, G, T order); a kept position outside its contig raises a flag
// Kernels of finish, between which sa_acc_finish scans the blocks' counts:
//   k_mg_mark         one block per 2048 positions: how many are reported
//   k_mg_emit         marginal, probabilities, called letter, proposal and delta of every reported position, compacted in
//                     (contig, position) order
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <numeric>
#include <unordered_map>
#include <vector>

#include "sa_internal.h"
#include "sa_contig_acc.h"

#define MG_SHORT 16u
#define MG_MEDIUM 1024u
#define MG_MAX_ROWS (1ll << 30)

struct MgRow {
    long long site;   // global position, -1: dropped
    unsigned ord;     // unique within the call
    int dir;          // 1: forward sum
    double p[4];
};

struct MgJob {   // sa_snp_job_map_t as the device reads it
    long long pos0, x0, coff, clen;
    int pos_sign, x_sign, dir, group;
    unsigned ord;
    int pad;
};

// poisoned: an add failed after its first kernel, and tcnt[] may hold counts
struct sa_snp_marginals : SaContigAcc {
    long long step = 0;
    double *d_sum = nullptr;   // the store's arrays
    unsigned *d_depth = nullptr, *d_tcnt = nullptr, *d_tloc = nullptr;
};

__device__ __forceinline__ unsigned mg_pow2ceil(unsigned c) { return c <= 1u ? 1u : 1u << (32 - __clz((int) (c - 1u))); }
__device__ __forceinline__ unsigned mg_places(unsigned c) { return c <= MG_SHORT ? c : mg_pow2ceil(c); }

__global__ __launch_bounds__(256) void k_mg_count(const MgRow *__restrict__ rows, unsigned n, unsigned *__restrict__ tcnt,
                                                  unsigned *__restrict__ ticket) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long site = rows[i].site;
    ticket[i] = site >= 0 ? atomicAdd(&tcnt[site], 1u) : 0xffffffffu;
}

// ctr: [0] the cursor over the entries, [1 + tier] the length of the tier's list
__global__ __launch_bounds__(256) void k_mg_alloc(const MgRow *__restrict__ rows, unsigned n, const unsigned *__restrict__ ticket,
                                                  const unsigned *__restrict__ tcnt, unsigned *__restrict__ tloc, unsigned *__restrict__ ctr,
                                                  long long *__restrict__ list_a, long long *__restrict__ list_b,
                                                  long long *__restrict__ list_c) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || ticket[i] != 0u) return;
    const long long site = rows[i].site;
    const unsigned c = tcnt[site];
    tloc[site] = atomicAdd(&ctr[0], mg_places(c));
    const int tier = c <= MG_SHORT ? 0 : c <= MG_MEDIUM ? 1 : 2;
    const unsigned at = atomicAdd(&ctr[1 + tier], 1u);
    (tier == 0 ? list_a : tier == 1 ? list_b : list_c)[at] = site;
}

__global__ __launch_bounds__(256) void k_mg_scatter(const MgRow *__restrict__ rows, unsigned n, const unsigned *__restrict__ ticket,
                                                    const unsigned *__restrict__ tloc, unsigned long long *__restrict__ ent) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long site = rows[i].site;
    if (site < 0) return;
    ent[(size_t) tloc[site] + ticket[i]] = ((unsigned long long) rows[i].ord << 32) | (unsigned long long) i;
}

__device__ __forceinline__ void mg_add_row(double *acc, const double *p, int dir) {
    if (dir) {
        acc[0] += p[0]; acc[1] += p[1]; acc[2] += p[2]; acc[3] += p[3];
    } else {
        acc[4] += p[0]; acc[5] += p[1]; acc[6] += p[2]; acc[7] += p[3];
    }
}

__global__ __launch_bounds__(256) void k_mg_fold_short(const long long *__restrict__ list, const unsigned *__restrict__ n_list,
                                                       unsigned *__restrict__ tcnt, const unsigned *__restrict__ tloc,
                                                       unsigned long long *__restrict__ ent, const MgRow *__restrict__ rows,
                                                       double *__restrict__ sum, unsigned *__restrict__ depth) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *n_list) return;
    const long long site = list[i];
    const unsigned c = tcnt[site];
    unsigned long long *e = ent + tloc[site];
    for (unsigned a = 1; a < c; a++) {   // at most MG_SHORT entries, unique keys
        const unsigned long long v = e[a];
        unsigned b = a;
        while (b > 0 && e[b - 1] > v) { e[b] = e[b - 1]; b--; }
        e[b] = v;
    }
    double acc[8];
    double *s = sum + (size_t) site * 8;
    for (int q = 0; q < 8; q++) acc[q] = s[q];
    for (unsigned a = 0; a < c; a++) {
        const MgRow &r = rows[(unsigned) (e[a] & 0xffffffffull)];
        mg_add_row(acc, r.p, r.dir);
    }
    for (int q = 0; q < 8; q++) s[q] = acc[q];
    depth[site] += c;
    tcnt[site] = 0;
}

// the bitonic network over m = 2^k keys (ascending), by the NT threads of the block; `s` in LDS or in global memory
template <int NT>
__device__ __forceinline__ void mg_bitonic(unsigned long long *s, unsigned m) {
    for (unsigned k = 2; k <= m; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned t = threadIdx.x; t < (m >> 1); t += NT) {
                const unsigned lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
                const unsigned long long a = s[lo], b = s[hi];
                if ((a > b) == ((lo & k) == 0u)) { s[lo] = b; s[hi] = a; }
            }
            __syncthreads();
        }
}

// the c sorted entries of a site folded into its sums: the block gathers the rows' values NT at a time, thread 0 adds them
template <int NT>
__device__ __forceinline__ void mg_fold_sorted(const unsigned long long *sorted, unsigned c, const MgRow *__restrict__ rows,
                                               double *__restrict__ s, double (*sv)[4], int *sd) {
    double acc[8];
    if (threadIdx.x == 0)
        for (int q = 0; q < 8; q++) acc[q] = s[q];
    for (unsigned base = 0; base < c; base += NT) {
        const unsigned q = base + threadIdx.x;
        if (q < c) {
            const MgRow &r = rows[(unsigned) (sorted[q] & 0xffffffffull)];
            sv[threadIdx.x][0] = r.p[0]; sv[threadIdx.x][1] = r.p[1]; sv[threadIdx.x][2] = r.p[2]; sv[threadIdx.x][3] = r.p[3];
            sd[threadIdx.x] = r.dir;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned m = min((unsigned) NT, c - base);
            for (unsigned a = 0; a < m; a++) mg_add_row(acc, sv[a], sd[a]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int q = 0; q < 8; q++) s[q] = acc[q];
}

__global__ __launch_bounds__(64) void k_mg_fold_lds(const long long *__restrict__ list, const unsigned *__restrict__ n_list,
                                                    unsigned *__restrict__ tcnt, const unsigned *__restrict__ tloc,
                                                    const unsigned long long *__restrict__ ent, const MgRow *__restrict__ rows,
                                                    double *__restrict__ sum, unsigned *__restrict__ depth) {
    __shared__ unsigned long long key[MG_MEDIUM];
    __shared__ double sv[64][4];
    __shared__ int sd[64];
    const unsigned n = *n_list;
    for (unsigned i = blockIdx.x; i < n; i += gridDim.x) {
        const long long site = list[i];
        const unsigned c = tcnt[site], m = mg_pow2ceil(c);   // MG_SHORT < c <= MG_MEDIUM
        const unsigned long long *e = ent + tloc[site];
        for (unsigned q = threadIdx.x; q < m; q += 64) key[q] = q < c ? e[q] : ~0ull;
        __syncthreads();
        mg_bitonic<64>(key, m);
        mg_fold_sorted<64>(key, c, rows, sum + (size_t) site * 8, sv, sd);
        if (threadIdx.x == 0) {
            depth[site] += c;
            tcnt[site] = 0;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_mg_fold_global(const long long *__restrict__ list, const unsigned *__restrict__ n_list,
                                                        unsigned *__restrict__ tcnt, const unsigned *__restrict__ tloc,
                                                        unsigned long long *ent, const MgRow *__restrict__ rows,
                                                        double *__restrict__ sum, unsigned *__restrict__ depth) {
    __shared__ double sv[256][4];
    __shared__ int sd[256];
    const unsigned n = *n_list;
    for (unsigned i = blockIdx.x; i < n; i += gridDim.x) {
        const long long site = list[i];
        const unsigned c = tcnt[site], m = mg_pow2ceil(c);   // c > MG_MEDIUM; the bucket has m places (k_mg_alloc)
        unsigned long long *e = ent + tloc[site];
        for (unsigned q = c + threadIdx.x; q < m; q += 256) e[q] = ~0ull;
        __syncthreads();
        mg_bitonic<256>(e, m);
        mg_fold_sorted<256>(e, c, rows, sum + (size_t) site * 8, sv, sd);
        if (threadIdx.x == 0) {
            depth[site] += c;
            tcnt[site] = 0;
        }
        __syncthreads();
    }
}

// the call's rows (n of them, on the device) added on stream 0; the caller holds t->mu and has set the device
static int mg_add_rows(sa_snp_marginals *t, const MgRow *d_rows, size_t n) {
    if (n == 0) return SA_OK;
    if ((long long) n > MG_MAX_ROWS) return SA_EUNSUPPORTED;
    int rc = SA_OK;
    const size_t cap_b = n / (MG_SHORT + 1) + 1, cap_c = n / (MG_MEDIUM + 1) + 1;
    SaLayout L;   // [ctr | ticket | entries (every bucket below twice its rows) | list a | list b | list c]
    const size_t o_ctr = L.add(4 * 4), o_ticket = L.add(4 * n), o_ent = L.add(8 * 2 * n), o_la = L.add(8 * n), o_lb = L.add(8 * cap_b),
                 o_lc = L.add(8 * cap_c);
    char *d = nullptr;
    if (g_sa_pool.get(SaPool::DEVICE, (void **) &d, L.end, t->device) != hipSuccess) return SA_ENOMEM;
    {
        unsigned *ctr = (unsigned *) (d + o_ctr), *ticket = (unsigned *) (d + o_ticket);
        unsigned long long *ent = (unsigned long long *) (d + o_ent);
        long long *la = (long long *) (d + o_la), *lb = (long long *) (d + o_lb), *lc = (long long *) (d + o_lc);
        const unsigned un = (unsigned) n, grid = (unsigned) ((n + 255) / 256);
        SA_HIP_GOTO_DONE(hipMemsetAsync(ctr, 0, 4 * 4, 0));
        hipLaunchKernelGGL(k_mg_count, dim3(grid), dim3(256), 0, 0, d_rows, un, t->d_tcnt, ticket);
        hipLaunchKernelGGL(k_mg_alloc, dim3(grid), dim3(256), 0, 0, d_rows, un, (const unsigned *) ticket, (const unsigned *) t->d_tcnt,
                           t->d_tloc, ctr, la, lb, lc);
        hipLaunchKernelGGL(k_mg_scatter, dim3(grid), dim3(256), 0, 0, d_rows, un, (const unsigned *) ticket, (const unsigned *) t->d_tloc, ent);
        hipLaunchKernelGGL(k_mg_fold_short, dim3(grid), dim3(256), 0, 0, (const long long *) la, (const unsigned *) (ctr + 1), t->d_tcnt,
                           (const unsigned *) t->d_tloc, ent, d_rows, t->d_sum, t->d_depth);
        if (n > MG_SHORT)
            hipLaunchKernelGGL(k_mg_fold_lds, dim3((unsigned) std::min(cap_b, (size_t) 4096)), dim3(64), 0, 0, (const long long *) lb,
                               (const unsigned *) (ctr + 2), t->d_tcnt, (const unsigned *) t->d_tloc, (const unsigned long long *) ent, d_rows,
                               t->d_sum, t->d_depth);
        if (n > MG_MEDIUM)
            hipLaunchKernelGGL(k_mg_fold_global, dim3((unsigned) std::min(cap_c, (size_t) 1024)), dim3(256), 0, 0, (const long long *) lc,
                               (const unsigned *) (ctr + 3), t->d_tcnt, (const unsigned *) t->d_tloc, ent, d_rows, t->d_sum, t->d_depth);
        SA_HIP_GOTO_DONE(hipGetLastError());
        SA_HIP_GOTO_DONE(hipStreamSynchronize(0));
    }
done:
    if (rc != SA_OK) {
        (void) hipStreamSynchronize(0);
        t->poisoned = true;   // (the working counts of the touched sites are not known to be zero any more)
    }
    g_sa_pool.put(SaPool::DEVICE, d);
    return rc;
}

extern "C" int sa_snp_marginals_create(sa_snp_marginals_t **out, const int64_t *contig_lens, int64_t n_contigs, int64_t step, int device) {
    if (!out || step < 0) return SA_EINVAL;
    *out = nullptr;
    sa_snp_marginals *t = new (std::nothrow) sa_snp_marginals();
    if (!t) return SA_ENOMEM;
    int rc = sa_acc_layout(t, contig_lens, n_contigs, /* pad */ 0);
    if (rc != SA_OK) { delete t; return rc; }
    t->step = step;
    const size_t np = (size_t) (t->n_slots > 0 ? t->n_slots : 1);
    SaLayout L;
    const size_t o_sum = L.add(8 * 8 * np), o_depth = L.add(4 * np), ck_bytes = L.end, o_tcnt = L.add(4 * np), o_tloc = L.add(4 * np);
    rc = sa_acc_alloc(t, device, L.end, ck_bytes);
    if (rc != SA_OK) { sa_snp_marginals_destroy(t); return rc; }
    t->d_sum = (double *) (t->d_store + o_sum);
    t->d_depth = (unsigned *) (t->d_store + o_depth);
    t->d_tcnt = (unsigned *) (t->d_store + o_tcnt);
    t->d_tloc = (unsigned *) (t->d_store + o_tloc);
    *out = t;
    return SA_OK;
}

extern "C" void sa_snp_marginals_destroy(sa_snp_marginals_t *t) {
    if (!t) return;
    sa_acc_free(t);
    delete t;
}

extern "C" int sa_snp_marginals_add_sites(sa_snp_marginals_t *t, int32_t contig, int64_t run, int direction, const sa_snp_site_t *sites,
                                          int64_t n) {
    (void) run;   // (every row of the call shares it: it orders nothing here)
    if (!t || n < 0 || (n > 0 && !sites) || contig < 0 || contig >= t->n_contigs) return SA_EINVAL;
    if (n > MG_MAX_ROWS) return SA_EUNSUPPORTED;
    if (n == 0) return SA_OK;
    const long long c0 = t->coff[(size_t) contig], len = t->coff[(size_t) contig + 1] - c0;
    size_t n_t = 0;
    for (int64_t i = 0; i < n; i++) {
        if (sites[i].pos < 0 || sites[i].pos >= len || (sites[i].strand != 0 && sites[i].strand != 1)) return SA_EINVAL;
        n_t += sites[i].strand == 0;
    }
    std::vector<MgRow> rows((size_t) n);
    unsigned next[2] = {0u, (unsigned) n_t};   // strand t before c, each in the order given
    for (int64_t i = 0; i < n; i++) {
        MgRow &r = rows[(size_t) i];
        r.site = c0 + sites[i].pos;
        r.ord = next[sites[i].strand]++;
        r.dir = direction ? 1 : 0;
        for (int l = 0; l < 4; l++) r.p[l] = sites[i].p[l];
    }
    SaAccEnter in(t);
    if (in.rc) return in.rc;
    int rc = SA_OK;
    MgRow *d_rows = nullptr;
    if (g_sa_pool.get(SaPool::DEVICE, (void **) &d_rows, sizeof(MgRow) * (size_t) n, t->device) != hipSuccess) return SA_ENOMEM;
    SA_HIP_GOTO_DONE(hipMemcpy(d_rows, rows.data(), sizeof(MgRow) * (size_t) n, hipMemcpyHostToDevice));
    rc = mg_add_rows(t, d_rows, (size_t) n);
done:
    g_sa_pool.put(SaPool::DEVICE, d_rows);
    return rc;
}

// order-preserving map of a signed 64-bit value onto an unsigned one (for the integer atomics of k_mg_window)
__host__ __device__ static inline unsigned long long mg_bias(long long v) { return (unsigned long long) v ^ (1ull << 63); }
__host__ __device__ static inline long long mg_unbias(unsigned long long u) { return (long long) (u ^ (1ull << 63)); }
__device__ static inline long long mg_floor_mult(long long v, long long m) { return v - (((v % m) + m) % m); }

__global__ __launch_bounds__(256) void k_mg_window(const MgJob *__restrict__ jobs, int nj, const int *__restrict__ xmin,
                                                   const int *__restrict__ xmax, const long long *__restrict__ count,
                                                   unsigned long long *__restrict__ glo, unsigned long long *__restrict__ ghi) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nj || count[j] <= 0) return;
    const MgJob J = jobs[j];
    const long long a = J.x0 + (long long) J.x_sign * xmin[j], b = J.x0 + (long long) J.x_sign * xmax[j];
    atomicMin(&glo[J.group], mg_bias(min(a, b)));
    atomicMax(&ghi[J.group], mg_bias(max(a, b)));
}

// job blockIdx.x: its position calls off[j] .. off[j + 1) as rows
__global__ __launch_bounds__(64) void k_mg_batch_rows(const MgJob *__restrict__ jobs, const long long *__restrict__ off,
                                                      const int *__restrict__ slot, const double *__restrict__ prob, int stride,
                                                      const unsigned char *__restrict__ kind, const int *__restrict__ x_of_slot,
                                                      const signed char *__restrict__ acgt, long long step,
                                                      const unsigned long long *__restrict__ glo, const unsigned long long *__restrict__ ghi,
                                                      MgRow *__restrict__ rows, int *__restrict__ err) {
    const int j = blockIdx.x;
    const MgJob J = jobs[j];
    long long w_lo = LLONG_MIN, w_hi = LLONG_MAX;
    if (off[j] == off[j + 1]) return;   // (a job without records has no calls, and its group may have no range)
    if (step >= 1) {   // sa_snp_site_window over the group's reference_index range
        const long long lo = mg_unbias(glo[J.group]), hi = mg_unbias(ghi[J.group]) + step;
        w_lo = mg_floor_mult(lo - step, step);
        w_hi = mg_floor_mult(hi, step) == hi ? hi : mg_floor_mult(hi, step) + step;
    }
    for (long long r = off[j] + threadIdx.x; r < off[j + 1]; r += 64) {
        const int s = slot[r];
        const long long pos = J.pos0 + (long long) J.pos_sign * x_of_slot[s];
        MgRow row;
        row.ord = J.ord;
        row.dir = J.dir;
        const signed char *e = acgt + 4 * (int) kind[s];
        for (int l = 0; l < 4; l++) row.p[l] = e[l] >= 0 ? prob[(size_t) r * (size_t) stride + (size_t) e[l]] : 0.0;
        if (pos < w_lo || pos >= w_hi) {
            row.site = -1;
        } else if (pos < 0 || pos >= J.clen) {
            row.site = -1;
            atomicOr(err, 1);
        } else {
            row.site = J.coff + pos;
        }
        rows[r] = row;
    }
}

extern "C" int sa_snp_marginals_add_batch(sa_snp_marginals_t *t, sa_batch_t *b, const sa_snp_job_map_t *map, int64_t n_jobs,
                                          double *kernel_ms_out) {
    if (!t || !b || n_jobs < 0 || (n_jobs > 0 && !map)) return SA_EINVAL;
    if (kernel_ms_out) kernel_ms_out[0] = kernel_ms_out[1] = 0.0;
    SaAccEnter in(t);
    if (in.rc) return in.rc;
    SaPosFold F;
    int rc = sa_pos_fold_run(b, &F);
    char *d = nullptr;
    const size_t nj = F.nj, n = F.n_kept;
    if (rc == SA_OK && ((size_t) n_jobs != nj || F.device != t->device)) rc = SA_EINVAL;
    if (rc == SA_OK && (long long) n > MG_MAX_ROWS) rc = SA_EUNSUPPORTED;
    if (rc != SA_OK || nj == 0 || n == 0) {
        sa_pos_fold_release(&F, rc != SA_OK);
        if (rc == SA_OK && kernel_ms_out) kernel_ms_out[0] = F.kernel_ms;
        return rc;
    }
    {
        // rows in (run, strand, job) order: the job's rank is its rows' ordinal (a job has one row per position at most)
        std::vector<MgJob> jobs(nj);
        std::vector<size_t> by(nj);
        std::iota(by.begin(), by.end(), (size_t) 0);
        std::unordered_map<long long, int> group_of;
        for (size_t j = 0; j < nj && rc == SA_OK; j++) {
            const sa_snp_job_map_t &m = map[j];
            if (m.contig < 0 || m.contig >= t->n_contigs || (m.pos_sign != 1 && m.pos_sign != -1) || (m.x_sign != 1 && m.x_sign != -1) ||
                (m.strand != 0 && m.strand != 1)) {
                rc = SA_EINVAL;
                break;
            }
            MgJob &J = jobs[j];
            J.pos0 = m.pos0; J.x0 = m.x0;
            J.coff = t->coff[(size_t) m.contig];
            J.clen = t->coff[(size_t) m.contig + 1] - J.coff;
            J.pos_sign = m.pos_sign; J.x_sign = m.x_sign;
            J.dir = m.direction ? 1 : 0;
            J.group = group_of.emplace((long long) m.group, (int) group_of.size()).first->second;
            J.ord = 0; J.pad = 0;
        }
        if (rc != SA_OK) { sa_pos_fold_release(&F, false); return rc; }
        std::sort(by.begin(), by.end(), [&](size_t a, size_t c) {
            if (map[a].run != map[c].run) return map[a].run < map[c].run;
            if (map[a].strand != map[c].strand) return map[a].strand < map[c].strand;
            return a < c;
        });
        for (size_t r = 0; r < nj; r++) jobs[by[r]].ord = (unsigned) r;
        const size_t ng = group_of.size(), ns = (size_t) sa_ambig_count(F.tab);
        SaLayout L;   // [jobs | count | glo, ghi | x of slot | acgt | err | rows]
        const size_t o_jobs = L.add(sizeof(MgJob) * nj), o_count = L.add(8 * nj), o_glo = L.add(8 * ng), o_ghi = L.add(8 * ng),
                     o_x = L.add(4 * (ns ? ns : 1)), o_acgt = L.add(F.acgt.size() + 1), o_err = L.add(4), o_rows = L.add(sizeof(MgRow) * n);
        float kms = 0;
        int h_err = 0;
        if (hipSetDevice(t->device) != hipSuccess) { rc = SA_ENODEVICE; goto done; }   // (the fold bound the batch's, the same one)
        if (g_sa_pool.get(SaPool::DEVICE, (void **) &d, L.end, t->device) != hipSuccess) { d = nullptr; rc = SA_ENOMEM; goto done; }
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_jobs, jobs.data(), sizeof(MgJob) * nj, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_count, F.count.data(), 8 * nj, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_x, F.h_x, 4 * ns, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_acgt, F.acgt.data(), F.acgt.size(), hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemsetAsync(d + o_glo, 0xff, 8 * ng, 0));   // (the largest biased value)
        SA_HIP_GOTO_DONE(hipMemsetAsync(d + o_ghi, 0, 8 * ng, 0));      // (the smallest)
        SA_HIP_GOTO_DONE(hipMemsetAsync(d + o_err, 0, 4, 0));
        SA_HIP_GOTO_DONE(hipEventRecord(t->e0, 0));
        hipLaunchKernelGGL(k_mg_window, dim3((unsigned) ((nj + 255) / 256)), dim3(256), 0, 0, (const MgJob *) (d + o_jobs), (int) nj, F.xmin,
                           F.xmax, (const long long *) (d + o_count), (unsigned long long *) (d + o_glo), (unsigned long long *) (d + o_ghi));
        hipLaunchKernelGGL(k_mg_batch_rows, dim3((unsigned) nj), dim3(64), 0, 0, (const MgJob *) (d + o_jobs), F.off, F.slot, F.prob,
                           (int) F.stride, F.kind, (const int *) (d + o_x), (const signed char *) (d + o_acgt), t->step,
                           (const unsigned long long *) (d + o_glo), (const unsigned long long *) (d + o_ghi), (MgRow *) (d + o_rows),
                           (int *) (d + o_err));
        SA_HIP_GOTO_DONE(hipGetLastError());
        SA_HIP_GOTO_DONE(hipMemcpy(&h_err, d + o_err, 4, hipMemcpyDeviceToHost));
        if (h_err) { rc = SA_EINVAL; goto done; }   // (nothing has been added yet)
        rc = mg_add_rows(t, (const MgRow *) (d + o_rows), n);
        if (rc != SA_OK) goto done;
        SA_HIP_GOTO_DONE(hipEventRecord(t->e1, 0));
        SA_HIP_GOTO_DONE(hipEventSynchronize(t->e1));
        SA_HIP_GOTO_DONE(hipEventElapsedTime(&kms, t->e0, t->e1));
        if (kernel_ms_out) { kernel_ms_out[0] = F.kernel_ms; kernel_ms_out[1] = (double) kms; }
    }
done:
    if (rc != SA_OK && d) (void) hipStreamSynchronize(0);
    if (d) g_sa_pool.put(SaPool::DEVICE, d);
    sa_pos_fold_release(&F, rc != SA_OK);
    return rc;
}

extern "C" int sa_snp_marginals_checkpoint(sa_snp_marginals_t *t) { return sa_acc_checkpoint(t); }
extern "C" int sa_snp_marginals_rollback(sa_snp_marginals_t *t) { return sa_acc_rollback(t); }

// ---- finish ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SA_ACC_THREADS) void k_mg_mark(const unsigned *__restrict__ depth, long long n_pos, unsigned min_depth,
                                                           long long *__restrict__ blk_cnt) {
    sa_acc_block_count(sa_acc_count(sa_acc_first_slot(), n_pos, [=](long long g, int) { return depth[g] >= min_depth; }), blk_cnt);
}

__device__ __forceinline__ int mg_letter_index(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

__global__ __launch_bounds__(SA_ACC_THREADS) void k_mg_emit(const unsigned *__restrict__ depth, const double *__restrict__ sum,
                                                           long long n_pos, unsigned min_depth, const long long *__restrict__ coff,
                                                           int n_contigs, const char *__restrict__ ref,
                                                           const long long *__restrict__ blk_off, sa_snp_marginal_t *__restrict__ out) {
    const long long g0 = sa_acc_first_slot();
    const int mine = sa_acc_count(g0, n_pos, [=](long long g, int) { return depth[g] >= min_depth; });
    long long w = sa_acc_place(mine, blk_off[blockIdx.x]);
    for (int q = 0; q < SA_ACC_PER_THREAD && mine; q++) {
        const long long g = g0 + q;
        if (g >= n_pos || depth[g] < min_depth) continue;
        const int c = sa_acc_contig_of(coff, n_contigs, g);
        sa_snp_marginal_t o;
        o.pos = g - coff[c];
        o.contig = c;
        o.depth = (int32_t) depth[g];
        const double *s = sum + (size_t) g * 8;
        for (int l = 0; l < 4; l++) { o.fwd[l] = s[l]; o.bwd[l] = s[4 + l]; }
        double m[4];
        for (int l = 0; l < 4; l++) m[l] = o.fwd[l] + o.bwd[3 - l];   // (rc_probs on the backward sum)
        const double total = ((m[0] + m[1]) + m[2]) + m[3];
        o.ref = sa_acc_ref_letter(ref, g);
        const int ri = mg_letter_index(o.ref);   // ('N' without a reference: none)
        for (int q2 = 0; q2 < 5; q2++) o.pad[q2] = 0;
        if (total == 0.0) {
            for (int l = 0; l < 4; l++) o.prob[l] = 0.0;
            o.called = 'N';
            o.is_proposal = 0;
            o.delta = 0.0;
        } else {
            int best = 0;
            for (int l = 0; l < 4; l++) o.prob[l] = m[l] / total;
            for (int l = 1; l < 4; l++)
                if (o.prob[l] > o.prob[best]) best = l;
            o.called = "ACGT"[best];
            o.is_proposal = (char) (ri >= 0 && ri != best);
            o.delta = ri >= 0 ? o.prob[best] - o.prob[ri] : 0.0;
        }
        out[w++] = o;
    }
}

extern "C" int sa_snp_marginals_finish(sa_snp_marginals_t *t, int64_t min_depth, const char *const *ref_by_contig,
                                       sa_snp_marginal_t **sites_out, int64_t *n_out, double *kernel_ms_out) {
    if (const int rc = sa_acc_finish_args(t, ref_by_contig, sites_out, n_out, kernel_ms_out)) return rc;
    const unsigned md = (unsigned) std::min<int64_t>(std::max<int64_t>(min_depth, 1), (int64_t) UINT32_MAX);
    SaAccEnter in(t);
    if (in.rc) return in.rc;
    return sa_acc_finish(
        t, ref_by_contig, 0,
        [&](unsigned nb, char *, long long *blk_cnt) {
            hipLaunchKernelGGL(k_mg_mark, dim3(nb), dim3(SA_ACC_THREADS), 0, 0, (const unsigned *) t->d_depth, t->n_slots, md, blk_cnt);
        },
        [&](unsigned nb, char *, const long long *blk_off, const char *ref, sa_snp_marginal_t *d_out) {
            hipLaunchKernelGGL(k_mg_emit, dim3(nb), dim3(SA_ACC_THREADS), 0, 0, (const unsigned *) t->d_depth, (const double *) t->d_sum,
                               t->n_slots, md, (const long long *) t->d_coff, (int) t->n_contigs, ref, blk_off, d_out);
        },
        sites_out, n_out, kernel_ms_out);
}
