// What a device-resident table over contig positions is, apart from what it sums (sa_marginals.hip, sa_profile.hip): the layout
// of the contigs' slots, the one device store with its checkpoint copy, the way into a call, and the compaction of finish.
//
// Slots: contig c's position q is slot coff[c] + q, the contigs one after the other, each with `pad` slots more than positions.
// Life cycle, the same for every such table:
//   - an add that fails once it has begun to change the store poisons the table; every later call but destroy is SA_ESTATE,
//     and SaAccEnter is the one place that says so;
//   - checkpoint copies the store's first ck_bytes aside (one copy; a second checkpoint overwrites the first), rollback copies
//     them back and keeps the checkpoint; a rollback without a checkpoint is SA_ESTATE;
//   - finish reports the kept slots compacted in (contig, position) order in a malloc'd array the caller frees; with nothing
//     kept -- an empty table included, for which nothing is launched -- that is a one-element array and *n_out = 0.
// Cost: create, checkpoint, rollback and finish are O(contig length) -- they zero, copy or scan every slot; an add is O(rows).
#ifndef SA_CONTIG_ACC_H
#define SA_CONTIG_ACC_H

#include <stdint.h>
#include <stdlib.h>

#include <mutex>
#include <vector>

#include "sa_chain.h"

// one block of finish: SA_ACC_THREADS threads, SA_ACC_PER_THREAD consecutive slots each
#define SA_ACC_THREADS 256
#define SA_ACC_PER_THREAD 8
#define SA_ACC_SPAN (SA_ACC_THREADS * SA_ACC_PER_THREAD)

struct SaContigAcc {
    int device = 0, pad = 0;
    long long n_contigs = 0, n_slots = 0;
    std::vector<long long> coff, clen;   // slot of position 0 of every contig (n_contigs + 1), and the lengths
    long long *d_coff = nullptr;
    char *d_store = nullptr, *ck_store = nullptr;   // the table's arrays in ONE block; what a checkpoint covers comes first
    size_t store_bytes = 0, ck_bytes = 0;
    bool poisoned = false, ck = false;
    std::mutex mu;
    hipEvent_t e0 = nullptr, e1 = nullptr;
};

// the contigs' slots: n_contigs in [1, INT32_MAX), every length in [0, 2^40]
static inline int sa_acc_layout(SaContigAcc *a, const int64_t *contig_lens, int64_t n_contigs, int pad) {
    if (n_contigs < 1 || n_contigs >= INT32_MAX || !contig_lens) return SA_EINVAL;
    for (int64_t c = 0; c < n_contigs; c++)
        if (contig_lens[c] < 0 || contig_lens[c] > (int64_t) 1 << 40) return SA_EINVAL;
    a->pad = pad;
    a->n_contigs = n_contigs;
    a->clen.assign(contig_lens, contig_lens + n_contigs);
    a->coff.assign((size_t) n_contigs + 1, 0);
    for (int64_t c = 0; c < n_contigs; c++) a->coff[(size_t) c + 1] = a->coff[(size_t) c] + contig_lens[c] + pad;
    a->n_slots = a->coff[(size_t) n_contigs];
    return SA_OK;
}

// the laid-out table on `device`: its events, the contigs' offsets, and the store, zeroed; what it got goes back in sa_acc_free
static inline int sa_acc_alloc(SaContigAcc *a, int device, size_t store_bytes, size_t ck_bytes) {
    if (const int rc = sa_device_check(device, /* quiet */ true)) return rc;
    if (hipSetDevice(device) != hipSuccess) return SA_ENODEVICE;
    a->device = device;
    a->store_bytes = store_bytes;
    a->ck_bytes = ck_bytes;
    int rc = SA_OK;
    SA_HIP_GOTO_DONE(hipEventCreate(&a->e0));
    SA_HIP_GOTO_DONE(hipEventCreate(&a->e1));
    SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &a->d_coff, 8 * a->coff.size(), device));
    SA_HIP_GOTO_DONE(g_sa_pool.get(SaPool::DEVICE, (void **) &a->d_store, store_bytes, device));
    SA_HIP_GOTO_DONE(hipMemcpy(a->d_coff, a->coff.data(), 8 * a->coff.size(), hipMemcpyHostToDevice));
    SA_HIP_GOTO_DONE(hipMemset(a->d_store, 0, store_bytes));   // (all bits zero is +0.0)
    SA_HIP_GOTO_DONE(hipDeviceSynchronize());
done:
    return rc;
}

static inline void sa_acc_free(SaContigAcc *a) {
    (void) hipSetDevice(a->device);
    void *blocks[] = {a->d_coff, a->d_store, a->ck_store};
    for (void *p : blocks) g_sa_pool.put(SaPool::DEVICE, p);
    if (a->e0) (void) hipEventDestroy(a->e0);
    if (a->e1) (void) hipEventDestroy(a->e1);
}

// The way into a call on a table: its lock, SA_ESTATE for a poisoned one, its device.  `if (in.rc) return in.rc;`
struct SaAccEnter {
    std::lock_guard<std::mutex> g;
    const int rc;
    explicit SaAccEnter(SaContigAcc *a)
        : g(a->mu), rc(a->poisoned ? SA_ESTATE : hipSetDevice(a->device) != hipSuccess ? SA_ENODEVICE : SA_OK) {}
};

static inline int sa_acc_checkpoint(SaContigAcc *a) {
    if (!a) return SA_EINVAL;
    SaAccEnter in(a);
    if (in.rc) return in.rc;
    int rc = SA_OK;
    if (!a->ck_store && g_sa_pool.get(SaPool::DEVICE, (void **) &a->ck_store, a->ck_bytes, a->device) != hipSuccess) {
        a->ck_store = nullptr;
        return SA_ENOMEM;
    }
    a->ck = false;
    SA_HIP_GOTO_DONE(hipMemcpy(a->ck_store, a->d_store, a->ck_bytes, hipMemcpyDeviceToDevice));
    SA_HIP_GOTO_DONE(hipDeviceSynchronize());
    a->ck = true;
done:
    return rc;
}

static inline int sa_acc_rollback(SaContigAcc *a) {
    if (!a) return SA_EINVAL;
    SaAccEnter in(a);
    if (in.rc) return in.rc;
    if (!a->ck) return SA_ESTATE;
    int rc = SA_OK;
    SA_HIP_GOTO_DONE(hipMemcpy(a->d_store, a->ck_store, a->ck_bytes, hipMemcpyDeviceToDevice));
    SA_HIP_GOTO_DONE(hipDeviceSynchronize());
done:
    return rc;
}

// A timed region on the table's events around launches on stream 0: begin, the launches, end (which also reports a launch that
// failed), the caller's blocking copy, then ms.  The copy stays outside the region.
static inline hipError_t sa_acc_time_begin(SaContigAcc *a) { return hipEventRecord(a->e0, 0); }
static inline hipError_t sa_acc_time_end(SaContigAcc *a) {
    const hipError_t e = hipEventRecord(a->e1, 0);
    return e != hipSuccess ? e : hipGetLastError();
}
static inline hipError_t sa_acc_time_ms(SaContigAcc *a, float *ms) { return hipEventElapsedTime(ms, a->e0, a->e1); }

// ---- finish: the device side ---------------------------------------------------------------------------------------------------
// slot of the thread's first of SA_ACC_PER_THREAD
__device__ __forceinline__ long long sa_acc_first_slot() {
    return (long long) blockIdx.x * SA_ACC_SPAN + (long long) threadIdx.x * SA_ACC_PER_THREAD;
}

// how many of the thread's slots from g0 on are reported: keep(g, q) of slot g = g0 + q < n_slots
template <class Keep>
__device__ __forceinline__ int sa_acc_count(long long g0, long long n_slots, Keep keep) {
    int mine = 0;
    for (int q = 0; q < SA_ACC_PER_THREAD; q++)
        if (g0 + q < n_slots && keep(g0 + q, q)) mine++;
    return mine;
}

// a mark kernel's end: the threads' counts summed into the block's
__device__ __forceinline__ void sa_acc_block_count(int mine, long long *__restrict__ blk_cnt) {
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// What lies before the thread's `mine`: `before` the block, the block's waves before this one (through LDS) and the wave's lanes
// before this one (wave scan).  With the block's entry of the scanned counts as `before`, that is the output index of the thread's
// first reported slot.  A kernel that asks twice with the same T puts a barrier between the two.
template <class T>
__device__ __forceinline__ long long sa_acc_place(T mine, long long before) {
    __shared__ T wave_tot[SA_ACC_THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const T incl = sa_wave_incl_scan(mine, lane);
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    long long w = before + incl - mine;
    for (int q = 0; q < wv; q++) w += wave_tot[q];
    return w;
}

// the contig of slot g: the last c with coff[c] <= g (contigs without a slot share an offset with the next)
__device__ __forceinline__ int sa_acc_contig_of(const long long *__restrict__ coff, int n_contigs, long long g) {
    int lo = 0, hi = n_contigs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (coff[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// the reference letter at slot g in upper case; 'N' without a reference
__device__ __forceinline__ char sa_acc_ref_letter(const char *__restrict__ ref, long long g) {
    if (!ref) return 'N';
    const char r = ref[g];
    return r >= 'a' && r <= 'z' ? (char) (r - 'a' + 'A') : r;
}

// exclusive scan of n blocks' values into off[0 .. n] (one block)
static __global__ __launch_bounds__(SA_SCAN_THREADS) void k_acc_scan(const long long *__restrict__ v, long long *__restrict__ off, long long n) {
    sa_block_excl_scan([v](long long i) { return v[i]; }, off, n);
}

// ---- finish: the host side -----------------------------------------------------------------------------------------------------
static inline size_t sa_acc_blocks(const SaContigAcc *a) { return ((size_t) a->n_slots + SA_ACC_SPAN - 1) / SA_ACC_SPAN; }

// before the lock is taken: the arguments, the outputs cleared, a reference for every contig or for none
template <class Site>
static int sa_acc_finish_args(const SaContigAcc *t, const char *const *ref_by_contig, Site **sites_out, int64_t *n_out, double *kernel_ms_out) {
    if (!t || !sites_out || !n_out) return SA_EINVAL;
    *sites_out = nullptr;
    *n_out = 0;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (ref_by_contig)
        for (long long c = 0; c < t->n_contigs; c++)
            if (!ref_by_contig[c]) return SA_EINVAL;
    return SA_OK;
}

// The compaction, by a caller that has entered (SaAccEnter).  With nb = sa_acc_blocks(a) and a scratch block of the caller's own
// (`own_bytes` of it):
//   mark(nb, own, blk_cnt)                 launches what leaves the count of block b's reported slots in blk_cnt[b]
//   emit(nb, own, blk_off, ref, d_out)     launches what writes the reported slots of block b from d_out[blk_off[b]] on; ref holds
//                                          the contigs' letters slot by slot, or is NULL
// *kernel_ms_out is the sum of the two timed regions, around mark and scan and around emit.
template <class Site, class Mark, class Emit>
static int sa_acc_finish(SaContigAcc *a, const char *const *ref_by_contig, size_t own_bytes, Mark mark, Emit emit, Site **sites_out,
                         int64_t *n_out, double *kernel_ms_out) {
    const size_t ns = (size_t) a->n_slots, nb = sa_acc_blocks(a);
    int rc = SA_OK;
    SaLayout L;   // [the caller's own | block counts | counts before each block | reference letters]
    const size_t o_own = L.add(own_bytes), o_cnt = L.add(8 * nb), o_off = L.add(8 * (nb + 1)), o_ref = L.add(ref_by_contig ? ns : 1);
    char *d = nullptr;
    Site *d_out = nullptr, *host = nullptr;
    long long n_kept = 0;
    float ms0 = 0, ms1 = 0;
    if (nb > 0) {   // (a table without a slot keeps nothing: the one place that decides it, and nothing is launched)
        if (g_sa_pool.get(SaPool::DEVICE, (void **) &d, L.end, a->device) != hipSuccess) return SA_ENOMEM;
        if (ref_by_contig)
            for (long long c = 0; c < a->n_contigs; c++) {
                const size_t len = (size_t) a->clen[(size_t) c];
                if (len) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_ref + a->coff[(size_t) c], ref_by_contig[c], len, hipMemcpyHostToDevice, 0));
            }
        SA_HIP_GOTO_DONE(sa_acc_time_begin(a));
        mark((unsigned) nb, d + o_own, (long long *) (d + o_cnt));
        hipLaunchKernelGGL(k_acc_scan, dim3(1), dim3(SA_SCAN_THREADS), 0, 0, (const long long *) (d + o_cnt), (long long *) (d + o_off), (long long) nb);
        SA_HIP_GOTO_DONE(sa_acc_time_end(a));
        SA_HIP_GOTO_DONE(hipMemcpy(&n_kept, d + o_off + 8 * nb, 8, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(sa_acc_time_ms(a, &ms0));
    }
    host = (Site *) calloc((size_t) (n_kept > 0 ? n_kept : 1), sizeof(Site));
    if (!host) { rc = SA_ENOMEM; goto done; }
    if (n_kept > 0) {
        if (g_sa_pool.get(SaPool::DEVICE, (void **) &d_out, sizeof(Site) * (size_t) n_kept, a->device) != hipSuccess) {
            d_out = nullptr;
            rc = SA_ENOMEM;
            goto done;
        }
        SA_HIP_GOTO_DONE(sa_acc_time_begin(a));
        emit((unsigned) nb, d + o_own, (const long long *) (d + o_off), ref_by_contig ? (const char *) (d + o_ref) : (const char *) nullptr, d_out);
        SA_HIP_GOTO_DONE(sa_acc_time_end(a));
        SA_HIP_GOTO_DONE(hipMemcpy(host, d_out, sizeof(Site) * (size_t) n_kept, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(sa_acc_time_ms(a, &ms1));
    }
    if (kernel_ms_out) *kernel_ms_out = (double) ms0 + (double) ms1;
    *sites_out = host;
    *n_out = n_kept;
    host = nullptr;
done:
    if (rc != SA_OK) (void) hipStreamSynchronize(0);
    g_sa_pool.put(SaPool::DEVICE, d);
    g_sa_pool.put(SaPool::DEVICE, d_out);
    free(host);
    return rc;
}

#endif
