// Deviation of every read's alignment from its guide on gfx950 -- validateSignalAlignment.py (analyze_event_skips,
// src/signalalign/visualization/plot_labelled_read.py:364-472; the histogram, validateSignalAlignment.py:178-192; flag_large_gaps,
// :103-142) over the records of a finished batch (include/signalalign_hip.h has the rules and the three deliberate differences).
//
// Every event of the call has one 64-bit slot, job j's from ev_first[j] on: bit 63 aligned, bit 62 on the MEA path, bits 28..51
// the largest prob_e7 of the event's records, bits 0..27 the largest x among those.  Kernels, all on stream 0:
//   k_dv_best     one block per chunk (SaRecChunk, at most SA_CHAIN_CHUNK records of one job), in tiles of DV_TILE records: a 64-bit
//                 atomic maximum of (1 << 63) | prob_e7 << 28 | x into the slot of the record's event.  A job's records are ordered
//                 by x + y, so a tile touches a narrow run of y: with SA_DEV_WINDOW the block takes the tile's smallest y as the
//                 base of a window of DV_WIN slots in LDS, takes the maxima there, and flushes the touched slots with one global
//                 atomic each; a record outside the window goes straight to a global atomic, so the result never depends on the
//                 window.  Without the flag every record goes that way (SA_DEV_DIRECT): a batch holds about one record per event,
//                 so the window saves few atomics, and measured on 2000 reads of 5000 events it saved no time
//                 (profiles/guide_deviation.json): the simpler path is the default.
//   k_dv_mea      one thread per pair of the MEA paths: bit 62 of the slot of its event
//   k_dv_events   one thread per event: its job (binary search of ev_first), the guide position (binary search of the job's
//                 anchor_y), the difference and the flags, as sa_deviation_event_t
//   k_dv_jobs     one wave per job, 64 events a step: the histogram in LDS (added to the summed one with integer atomics), the sums
//                 and maxima in the lanes' registers, the runs by ballots over the aligned and the flagged mask with the open run
//                 carried across steps.  Run once to count the sets and make everything else, and -- after k_dv_scan has scanned
//                 the counts over the jobs -- once more to write them.
// The host reads the number of sets once to size the sets' block, and the results once.  No host pass over events or records.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "sa_internal.h"
#include "sa_chain.h"
#include "sa_scratch.h"

#define DV_THREADS 256
#define DV_TILE 2048       // records of a tile
#define DV_WIN 2048        // slots of the window: 16 KiB of LDS
#define DV_BIT_ALIGNED (1ull << 63)
#define DV_BIT_MEA (1ull << 62)
#define DV_X_MASK 0xfffffffull
#define DV_MAX_COORD (1ll << 28)

struct DvJob {
    long long ev_first;    // the job's first slot
    long long anc_first;   // the job's first anchor in the call's anchor arrays
    int n_events, n_anchors;
};

enum { DV_WS = 0, DV_SETS, DV_RECS };
static SaScratch g_dv_ws;

extern "C" void sa_guide_deviation_release(void) {
    std::lock_guard<std::mutex> guard(g_dv_ws.mu);
    g_dv_ws.release();
}

template <bool P8>
__device__ __forceinline__ void dv_rec(const void *__restrict__ recs, long long i, int *x, int *y, unsigned long long *pe7) {
    if (P8) {
        const unsigned long long r = ((const unsigned long long *) recs)[i];
        *x = (int) (r & 0xfffffull);
        *y = (int) ((r >> 20) & 0xfffffull);
        *pe7 = r >> 40;
    } else {
        const sa_pair16_t r = ((const sa_pair16_t *) recs)[i];
        *x = (int) (r.a & 0xfffffffull);
        *y = (int) ((r.a >> 28) & 0xfffffffull);
        *pe7 = (r.b >> 32) & 0xffffffull;
    }
}

template <bool DIRECT, bool P8>
__global__ __launch_bounds__(DV_THREADS) void k_dv_best(const void *__restrict__ recs, const SaRecChunk *__restrict__ chunks,
                                                        const DvJob *__restrict__ jobs, unsigned long long *__restrict__ best) {
    __shared__ unsigned long long win[DIRECT ? 1 : DV_WIN];
    __shared__ int s_base;
    const SaRecChunk C = chunks[blockIdx.x];
    const DvJob J = jobs[C.job];
    unsigned long long *slot = best + J.ev_first;
    for (int t0 = 0; t0 < C.n; t0 += DV_TILE) {
        const int tn = min(DV_TILE, C.n - t0);
        int base = 0;
        if (!DIRECT) {
            if (threadIdx.x == 0) s_base = INT_MAX;
            for (int e = threadIdx.x; e < DV_WIN; e += DV_THREADS) win[e] = 0;
            __syncthreads();
            int lo = INT_MAX;
            for (int i = threadIdx.x; i < tn; i += DV_THREADS) {
                int x, y;
                unsigned long long pe7;
                dv_rec<P8>(recs, C.first + t0 + i, &x, &y, &pe7);
                lo = min(lo, y);
            }
            if (lo != INT_MAX) atomicMin(&s_base, lo);
            __syncthreads();
            base = s_base;
        }
        for (int i = threadIdx.x; i < tn; i += DV_THREADS) {
            int x, y;
            unsigned long long pe7;
            dv_rec<P8>(recs, C.first + t0 + i, &x, &y, &pe7);
            if ((unsigned) y >= (unsigned) J.n_events) continue;   // (the host checked the caller's records, the batch its own: not reached)
            const unsigned long long key = DV_BIT_ALIGNED | (pe7 << 28) | (unsigned long long) x;
            const unsigned w = (unsigned) (y - base);
            if (!DIRECT && w < (unsigned) DV_WIN) atomicMax(&win[w], key);
            else atomicMax(&slot[y], key);
        }
        if (!DIRECT) {
            __syncthreads();
            for (int e = threadIdx.x; e < DV_WIN; e += DV_THREADS) {
                const unsigned long long v = win[e];
                if (v) atomicMax(&slot[base + e], v);   // (a touched slot: base + e is the y of a record that passed the check)
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(DV_THREADS) void k_dv_mea(const unsigned *__restrict__ idx, long long n, long long n_slots,
                                                       unsigned long long *__restrict__ best) {
    const long long i = (long long) blockIdx.x * DV_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned s = idx[i];
    if ((long long) s < n_slots) atomicOr(&best[s], DV_BIT_MEA);
}

__global__ __launch_bounds__(DV_THREADS) void k_dv_events(const DvJob *__restrict__ jobs, int nj, long long n_slots, const int *__restrict__ ax,
                                                          const int *__restrict__ ay, const unsigned long long *__restrict__ best,
                                                          int threshold, sa_deviation_event_t *__restrict__ events) {
    const long long e = (long long) blockIdx.x * DV_THREADS + threadIdx.x;
    if (e >= n_slots) return;
    int lo = 0, hi = nj - 1;   // the last job whose first slot is <= e: jobs without events share a first slot with their successor
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].ev_first <= e) lo = mid;
        else hi = mid - 1;
    }
    const DvJob J = jobs[lo];
    const int y = (int) (e - J.ev_first);
    const unsigned long long v = best[e];
    sa_deviation_event_t o;
    o.best_x = o.guide = o.diff = 0;
    o.flags = 0;
    if ((v & DV_BIT_ALIGNED) && J.n_anchors > 0) {
        const int *jx = ax + J.anc_first, *jy = ay + J.anc_first;
        int a = 0, b = J.n_anchors;   // the first anchor with anchor_y >= y
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (jy[mid] < y) a = mid + 1;
            else b = mid;
        }
        int guide;
        if (a < J.n_anchors && jy[a] == y) guide = jx[a];
        else if (a == 0) guide = jx[0];
        else if (a == J.n_anchors) guide = jx[a - 1];
        else guide = (jx[a - 1] + jx[a]) / 2;
        o.best_x = (int) (v & DV_X_MASK);
        o.guide = guide;
        o.diff = o.best_x - guide;
        const int ab = o.diff < 0 ? -o.diff : o.diff;
        o.flags = 1u | ((v & DV_BIT_MEA) ? 2u : 0u) | (ab > threshold ? 4u : 0u);
    }
    events[e] = o;
}

__device__ __forceinline__ long long dv_wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long dv_wave_max(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o);
        v = u > v ? u : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long dv_below(int bit) { return bit >= 64 ? ~0ull : (1ull << bit) - 1ull; }   // bits [0, bit)

// the run that is open at the wave's place in the job (wave-uniform)
struct DvRun {
    int open, first, last, count, peak, mea_peak;
    long long sum_y;
};

template <bool WRITE>
__global__ __launch_bounds__(64) void k_dv_jobs(const DvJob *__restrict__ jobs, const long long *__restrict__ n_recs,
                                                const sa_deviation_event_t *__restrict__ events, int bucket_size, int n_buckets,
                                                sa_deviation_read_t *__restrict__ reads, int *__restrict__ hist,
                                                unsigned long long *__restrict__ total_hist, sa_deviation_set_t *__restrict__ sets) {
    __shared__ int s_hist[WRITE ? 1 : SA_DEV_MAX_BUCKETS];
    const int j = blockIdx.x, lane = threadIdx.x;
    const DvJob J = jobs[j];
    const sa_deviation_event_t *ev = events + J.ev_first;
    if (!WRITE) {
        for (int q = lane; q < n_buckets; q += 64) s_hist[q] = 0;
        __syncthreads();
    }
    long long n_aligned = 0, n_flagged = 0, n_on_mea = 0, sum_abs = 0;   // the first three wave-uniform, the rest the lane's own
    unsigned long long max_key = 0;                                      // abs << 32 | ~y: the largest abs at the smallest y
    int max_mea = 0, n_sets = 0;
    long long w = WRITE ? reads[j].set_first : 0;
    DvRun R = {0, 0, 0, 0, 0, 0, 0};
    auto emit = [&](int open_end) {
        if (WRITE && lane == 0) {
            sa_deviation_set_t s;
            s.first_event = R.first; s.last_event = R.last; s.count = R.count; s.peak = R.peak; s.mea_peak = R.mea_peak;
            s.center_event = (int) (R.sum_y / R.count);
            s.open_end = open_end; s.pad = 0;
            sets[w] = s;
        }
        w++;
        n_sets++;
        R.open = 0;
    };
    for (int y0 = 0; y0 < J.n_events; y0 += 64) {
        const int y = y0 + lane;
        sa_deviation_event_t o;
        o.best_x = o.guide = o.diff = 0;
        o.flags = 0;
        if (y < J.n_events) o = ev[y];
        const bool aligned = o.flags & 1u, on_mea = (o.flags & 2u) && aligned, flagged = (o.flags & 4u) && aligned;
        const int ab = o.diff < 0 ? -o.diff : o.diff;
        const unsigned long long A = __ballot(aligned), F = __ballot(flagged);
        if (!WRITE) {
            n_aligned += __popcll(A);
            n_flagged += __popcll(F);
            n_on_mea += __popcll(__ballot(on_mea));
            if (aligned) {
                sum_abs += ab;
                const unsigned long long key = ((unsigned long long) (unsigned) ab << 32) | (unsigned long long) (0xffffffffu - (unsigned) y);
                max_key = key > max_key ? key : max_key;
                if (on_mea) max_mea = max(max_mea, ab);
                atomicAdd(&s_hist[min(ab / bucket_size, n_buckets - 1)], 1);
            }
        }
        // the runs of this step, over the aligned events only: `cur` holds the aligned events not yet walked
        unsigned long long cur = A;
        while (cur) {
            const int at = __ffsll((long long) cur) - 1;
            if ((F >> at) & 1ull) {
                const unsigned long long U = cur & ~F;   // the aligned events from here on that are not flagged
                const int end = U ? __ffsll((long long) U) - 1 : 64;
                const unsigned long long seg = cur & dv_below(end);   // all of them flagged: a piece of one run
                const bool in = (seg >> lane) & 1ull;
                // the piece's peak (high half) and peak on the path (low half), and the sum of its lanes
                unsigned long long pk = in ? ((unsigned long long) (unsigned) ab << 32) | (unsigned long long) (on_mea ? (unsigned) ab : 0u) : 0ull;
                long long ls = in ? lane : 0;
                for (int q = 32; q > 0; q >>= 1) {
                    const unsigned long long u = __shfl_xor(pk, q);
                    const unsigned hi = max((unsigned) (pk >> 32), (unsigned) (u >> 32)), lo = max((unsigned) pk, (unsigned) u);
                    pk = ((unsigned long long) hi << 32) | lo;
                    ls += __shfl_xor(ls, q);
                }
                const int cnt = __popcll(seg);
                if (!R.open) {
                    R.open = 1; R.first = y0 + at; R.count = 0; R.peak = 0; R.mea_peak = 0; R.sum_y = 0;
                }
                R.last = y0 + 63 - __clzll((long long) seg);
                R.count += cnt;
                R.peak = max(R.peak, (int) (pk >> 32));
                R.mea_peak = max(R.mea_peak, (int) (unsigned) pk);
                R.sum_y += (long long) y0 * cnt + ls;
                if (end < 64) emit(0);   // (the unflagged event at `end` closes it)
                cur &= ~dv_below(end);
            } else {
                if (R.open) emit(0);     // (a run carried in from the step before)
                const unsigned long long N = cur & F;
                cur = N ? cur & ~dv_below(__ffsll((long long) N) - 1) : 0ull;
            }
        }
    }
    if (R.open) emit(1);   // still open when the read ends
    if (WRITE) return;
    __syncthreads();
    for (int q = lane; q < n_buckets; q += 64) {
        const int v = s_hist[q];
        hist[(size_t) j * n_buckets + q] = v;
        if (v) atomicAdd(&total_hist[q], (unsigned long long) v);
    }
    sum_abs = dv_wave_sum(sum_abs);
    max_key = dv_wave_max(max_key);
    max_mea = (int) dv_wave_max((unsigned long long) max_mea);
    if (lane == 0) {
        sa_deviation_read_t r;
        r.status = J.n_anchors == 0 ? SA_DEV_NO_GUIDE : (n_recs[j] == 0 ? SA_DEV_NO_RECORDS : 0);
        r.n_sets = n_sets;
        r.set_first = 0;
        r.n_aligned = n_aligned; r.n_flagged = n_flagged; r.n_on_mea = n_on_mea; r.sum_abs = sum_abs;
        r.max_abs = (int) (max_key >> 32);
        r.max_abs_mea = max_mea;
        r.max_event = n_aligned ? (int) (0xffffffffu - (unsigned) max_key) : 0;
        r.pad = 0;
        reads[j] = r;
    }
}

// every job's first set: the exclusive scan of the jobs' counts; set_off[nj] is the number of sets
__global__ __launch_bounds__(SA_SCAN_THREADS) void k_dv_scan(sa_deviation_read_t *__restrict__ reads, long long *__restrict__ set_off, int nj) {
    sa_block_excl_scan([&](int i) { return (long long) reads[i].n_sets; }, set_off, nj);
    __syncthreads();
    for (int i = threadIdx.x; i < nj; i += SA_SCAN_THREADS) reads[i].set_first = set_off[i];
}

static const sa_deviation_params_t DV_DEFAULT = {10, 5, 64};

// what both calls check of their arguments; `ev_first` (nj + 1), the anchors and the paths' slots are what goes up
struct DvInput {
    std::vector<DvJob> jobs;
    std::vector<int> ax, ay;
    std::vector<unsigned> mea;
    long long n_slots = 0;
};
static int dv_check(const sa_deviation_job_t *jobs, int64_t n_jobs, const sa_mea_pair_t *const *mea_path, const int64_t *n_mea,
                    const sa_deviation_params_t *p, unsigned flags, sa_deviation_read_t *reads_out, sa_deviation_set_t **sets_out,
                    int64_t *n_sets_out, sa_deviation_event_t **events_out, DvInput *in) {
    if (n_jobs < 0 || (n_jobs > 0 && (!jobs || !reads_out)) || !sets_out || !n_sets_out || (flags & ~(SA_DEV_DIRECT | SA_DEV_EVENTS | SA_DEV_WINDOW))) return SA_EINVAL;
    if ((flags & SA_DEV_DIRECT) && (flags & SA_DEV_WINDOW)) return SA_EINVAL;
    if ((flags & SA_DEV_EVENTS) && !events_out) return SA_EINVAL;
    if ((mea_path == nullptr) != (n_mea == nullptr)) return SA_EINVAL;
    if (p->threshold < 0 || p->bucket_size < 1 || p->n_buckets < 1 || p->n_buckets > SA_DEV_MAX_BUCKETS) return SA_EINVAL;
    if (n_jobs > (int64_t) INT32_MAX) return SA_EUNSUPPORTED;
    in->jobs.resize((size_t) n_jobs);
    long long n_slots = 0, n_anc = 0, n_path = 0;
    for (int64_t j = 0; j < n_jobs; j++) {
        const sa_deviation_job_t &q = jobs[j];
        if (q.n_events < 0 || q.n_events > DV_MAX_COORD || q.n_anchors < 0 || q.n_anchors > (int64_t) INT32_MAX) return SA_EINVAL;
        if (q.n_anchors > 0 && (!q.anchor_x || !q.anchor_y)) return SA_EINVAL;
        if (mea_path && (n_mea[j] < 0 || (n_mea[j] > 0 && !mea_path[j]))) return SA_EINVAL;
        DvJob &J = in->jobs[(size_t) j];
        J.ev_first = n_slots; J.anc_first = n_anc; J.n_events = (int) q.n_events; J.n_anchors = (int) q.n_anchors;
        n_slots += q.n_events;
        n_anc += q.n_anchors;
        if (mea_path) n_path += n_mea[j];
    }
    if (n_slots > (long long) INT32_MAX) return SA_EUNSUPPORTED;
    in->n_slots = n_slots;
    in->ax.resize((size_t) n_anc); in->ay.resize((size_t) n_anc); in->mea.resize((size_t) n_path);
    size_t ia = 0, im = 0;
    for (int64_t j = 0; j < n_jobs; j++) {
        const sa_deviation_job_t &q = jobs[j];
        for (int64_t i = 0; i < q.n_anchors; i++, ia++) {
            const int64_t x = q.anchor_x[i], y = q.anchor_y[i];
            if (x < 0 || x >= DV_MAX_COORD || y < 0 || y > (int64_t) INT32_MAX || (i > 0 && y <= q.anchor_y[i - 1])) return SA_EINVAL;
            in->ax[ia] = (int) x; in->ay[ia] = (int) y;
        }
        for (int64_t i = 0; mea_path && i < n_mea[j]; i++, im++) {
            const int64_t e = mea_path[j][i].event_idx;
            if (e < 0 || e >= q.n_events) return SA_EINVAL;
            in->mea[im] = (unsigned) (in->jobs[(size_t) j].ev_first + e);
        }
    }
    return SA_OK;
}

// the records `recs` (on W's device; job j's are V.first[j] .. + V.count[j]); the caller holds W.mu and has bound W to the device
static int dv_run(SaScratch &W, const void *recs, bool p8, const SaBatchView &V, const DvInput &in, const sa_deviation_params_t &P,
                  unsigned flags, sa_deviation_read_t *reads_out, sa_deviation_set_t **sets_out, int64_t *n_sets_out, int32_t *hist_out,
                  int64_t *total_hist_out, sa_deviation_event_t **events_out, double *kernel_ms_out) {
    const size_t nj = in.jobs.size(), nb = (size_t) P.n_buckets, ns = (size_t) in.n_slots, na = in.ax.size(), nm = in.mea.size();
    *sets_out = nullptr;
    *n_sets_out = 0;
    if (flags & SA_DEV_EVENTS) *events_out = nullptr;
    if (nj == 0) {
        for (size_t q = 0; total_hist_out && q < nb; q++) total_hist_out[q] = 0;
        *sets_out = (sa_deviation_set_t *) malloc(sizeof(sa_deviation_set_t));
        if (flags & SA_DEV_EVENTS) *events_out = (sa_deviation_event_t *) malloc(sizeof(sa_deviation_event_t));
        return *sets_out && (!(flags & SA_DEV_EVENTS) || *events_out) ? SA_OK : SA_ENOMEM;
    }
    const std::vector<SaRecChunk> chunks = sa_view_chunks(V, SA_CHAIN_CHUNK, SA_ORDINAL_PER_JOB);
    const size_t nc = chunks.size();
    if (nc > (size_t) INT32_MAX) return SA_EUNSUPPORTED;
    int rc = SA_OK;
    // [jobs | records per job | chunks | anchor_x | anchor_y | paths' slots | best | events | reads | hist | total hist | set_off]
    SaLayout L;
    const size_t o_jobs = L.add(sizeof(DvJob) * nj), o_nrec = L.add(8 * nj), o_ch = L.add(sizeof(SaRecChunk) * nc), o_ax = L.add(4 * na),
                 o_ay = L.add(4 * na), o_mea = L.add(4 * nm), o_best = L.add(8 * ns), o_ev = L.add(sizeof(sa_deviation_event_t) * ns),
                 o_reads = L.add(sizeof(sa_deviation_read_t) * nj), o_hist = L.add(4 * nj * nb), o_thist = L.add(8 * nb),
                 o_soff = L.add(8 * (nj + 1));
    float ms0 = 0, ms1 = 0;
    long long n_sets = 0;
    sa_deviation_set_t *h_sets = nullptr;
    sa_deviation_event_t *h_events = nullptr;
    if ((rc = W.dev(DV_WS, L.end)) != SA_OK) return rc;
    {
        char *d = (char *) W.at(DV_WS);
        const DvJob *d_jobs = (const DvJob *) (d + o_jobs);
        const long long *d_nrec = (const long long *) (d + o_nrec);
        unsigned long long *d_best = (unsigned long long *) (d + o_best);
        sa_deviation_event_t *d_ev = (sa_deviation_event_t *) (d + o_ev);
        sa_deviation_read_t *d_reads = (sa_deviation_read_t *) (d + o_reads);
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_jobs, in.jobs.data(), sizeof(DvJob) * nj, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_nrec, V.count.data(), 8 * nj, hipMemcpyHostToDevice, 0));
        if (nc) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_ch, chunks.data(), sizeof(SaRecChunk) * nc, hipMemcpyHostToDevice, 0));
        if (na) {
            SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_ax, in.ax.data(), 4 * na, hipMemcpyHostToDevice, 0));
            SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_ay, in.ay.data(), 4 * na, hipMemcpyHostToDevice, 0));
        }
        if (nm) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_mea, in.mea.data(), 4 * nm, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(W.time_begin());
        if (ns) SA_HIP_GOTO_DONE(hipMemsetAsync(d_best, 0, 8 * ns, 0));
        SA_HIP_GOTO_DONE(hipMemsetAsync(d + o_thist, 0, 8 * nb, 0));
        if (nc && ns) {
            const SaRecChunk *d_ch = (const SaRecChunk *) (d + o_ch);
            const dim3 grid((unsigned) nc), block(DV_THREADS);
            if (!(flags & SA_DEV_WINDOW)) {
                if (p8) hipLaunchKernelGGL((k_dv_best<true, true>), grid, block, 0, 0, recs, d_ch, d_jobs, d_best);
                else hipLaunchKernelGGL((k_dv_best<true, false>), grid, block, 0, 0, recs, d_ch, d_jobs, d_best);
            } else {
                if (p8) hipLaunchKernelGGL((k_dv_best<false, true>), grid, block, 0, 0, recs, d_ch, d_jobs, d_best);
                else hipLaunchKernelGGL((k_dv_best<false, false>), grid, block, 0, 0, recs, d_ch, d_jobs, d_best);
            }
        }
        if (nm && ns)
            hipLaunchKernelGGL(k_dv_mea, dim3((unsigned) ((nm + DV_THREADS - 1) / DV_THREADS)), dim3(DV_THREADS), 0, 0,
                               (const unsigned *) (d + o_mea), (long long) nm, (long long) ns, d_best);
        if (ns)
            hipLaunchKernelGGL(k_dv_events, dim3((unsigned) ((ns + DV_THREADS - 1) / DV_THREADS)), dim3(DV_THREADS), 0, 0, d_jobs, (int) nj,
                               (long long) ns, (const int *) (d + o_ax), (const int *) (d + o_ay), (const unsigned long long *) d_best,
                               (int) P.threshold, d_ev);
        hipLaunchKernelGGL(k_dv_jobs<false>, dim3((unsigned) nj), dim3(64), 0, 0, d_jobs, d_nrec, (const sa_deviation_event_t *) d_ev,
                           (int) P.bucket_size, (int) P.n_buckets, d_reads, (int *) (d + o_hist), (unsigned long long *) (d + o_thist),
                           (sa_deviation_set_t *) nullptr);
        hipLaunchKernelGGL(k_dv_scan, dim3(1), dim3(SA_SCAN_THREADS), 0, 0, d_reads, (long long *) (d + o_soff), (int) nj);
        SA_HIP_GOTO_DONE(W.time_end());
        SA_HIP_GOTO_DONE(hipMemcpy(&n_sets, d + o_soff + 8 * nj, 8, hipMemcpyDeviceToHost));   // the one readback of the counts
        SA_HIP_GOTO_DONE(W.time_ms(&ms0));
        h_sets = (sa_deviation_set_t *) malloc(sizeof(sa_deviation_set_t) * (size_t) (n_sets > 0 ? n_sets : 1));
        if (flags & SA_DEV_EVENTS) h_events = (sa_deviation_event_t *) malloc(sizeof(sa_deviation_event_t) * (ns ? ns : 1));
        if (!h_sets || ((flags & SA_DEV_EVENTS) && !h_events)) { rc = SA_ENOMEM; goto done; }
        if (n_sets > 0) {
            if ((rc = W.dev(DV_SETS, sizeof(sa_deviation_set_t) * (size_t) n_sets)) != SA_OK) goto done;
            SA_HIP_GOTO_DONE(W.time_begin());
            hipLaunchKernelGGL(k_dv_jobs<true>, dim3((unsigned) nj), dim3(64), 0, 0, d_jobs, d_nrec, (const sa_deviation_event_t *) d_ev,
                               (int) P.bucket_size, (int) P.n_buckets, d_reads, (int *) nullptr, (unsigned long long *) nullptr,
                               (sa_deviation_set_t *) W.at(DV_SETS));
            SA_HIP_GOTO_DONE(W.time_end());
            SA_HIP_GOTO_DONE(hipMemcpy(h_sets, W.at(DV_SETS), sizeof(sa_deviation_set_t) * (size_t) n_sets, hipMemcpyDeviceToHost));
            SA_HIP_GOTO_DONE(W.time_ms(&ms1));
        }
        SA_HIP_GOTO_DONE(hipMemcpy(reads_out, d_reads, sizeof(sa_deviation_read_t) * nj, hipMemcpyDeviceToHost));
        if (hist_out) SA_HIP_GOTO_DONE(hipMemcpy(hist_out, d + o_hist, 4 * nj * nb, hipMemcpyDeviceToHost));
        if (total_hist_out) SA_HIP_GOTO_DONE(hipMemcpy(total_hist_out, d + o_thist, 8 * nb, hipMemcpyDeviceToHost));
        if ((flags & SA_DEV_EVENTS) && ns) SA_HIP_GOTO_DONE(hipMemcpy(h_events, d_ev, sizeof(sa_deviation_event_t) * ns, hipMemcpyDeviceToHost));
    }
    if (kernel_ms_out) *kernel_ms_out = (double) ms0 + (double) ms1;
    *sets_out = h_sets;
    *n_sets_out = n_sets;
    if (flags & SA_DEV_EVENTS) *events_out = h_events;
    return SA_OK;
done:
    (void) hipStreamSynchronize(0);
    free(h_sets);
    free(h_events);
    return rc;
}

extern "C" int sa_batch_guide_deviation(sa_batch_t *b, const sa_deviation_job_t *jobs, int64_t n_jobs, const sa_mea_pair_t *const *mea_path,
                                        const int64_t *n_mea, const sa_deviation_params_t *p, unsigned flags, sa_deviation_read_t *reads_out,
                                        sa_deviation_set_t **sets_out, int64_t *n_sets_out, int32_t *hist_out, int64_t *total_hist_out,
                                        sa_deviation_event_t **events_out, double *kernel_ms_out) {
    if (!b) return SA_EINVAL;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    const sa_deviation_params_t P = p ? *p : DV_DEFAULT;
    DvInput in;
    int rc = dv_check(jobs, n_jobs, mea_path, n_mea, &P, flags, reads_out, sets_out, n_sets_out, events_out, &in);
    if (rc) return rc;
    SaScratch &W = g_dv_ws;
    std::lock_guard<std::mutex> guard(W.mu);
    SaBatchView V;
    rc = sa_batch_view(b, &V);
    if (V.batch_flags & SA_FLAG_VC_ROWS) return SA_EINVAL;   // (it dropped rows; refused before the batch's state is looked at)
    if (rc) return rc;
    if (V.batch_flags & SA_FLAG_EXPECT_INTERNAL) return SA_ESTATE;
    if ((int64_t) V.count.size() != n_jobs) return SA_EINVAL;
    for (int64_t j = 0; j < n_jobs; j++)
        if (V.n_events[(size_t) j] != jobs[j].n_events) return SA_EINVAL;
    if ((rc = W.rebind(V.device)) != SA_OK) return rc;
    return dv_run(W, V.recs, V.p8, V, in, P, flags, reads_out, sets_out, n_sets_out, hist_out, total_hist_out, events_out, kernel_ms_out);
}

extern "C" int sa_guide_deviation_records(const sa_deviation_job_t *jobs, int64_t n_jobs, const int64_t *first, const int32_t *x,
                                          const int32_t *y, const int64_t *prob_e7, const sa_mea_pair_t *const *mea_path, const int64_t *n_mea,
                                          const sa_deviation_params_t *p, int device, unsigned flags, sa_deviation_read_t *reads_out,
                                          sa_deviation_set_t **sets_out, int64_t *n_sets_out, int32_t *hist_out, int64_t *total_hist_out,
                                          sa_deviation_event_t **events_out, double *kernel_ms_out) {
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    const sa_deviation_params_t P = p ? *p : DV_DEFAULT;
    DvInput in;
    int rc = dv_check(jobs, n_jobs, mea_path, n_mea, &P, flags, reads_out, sets_out, n_sets_out, events_out, &in);
    if (rc) return rc;
    if (!first || first[0] != 0) return SA_EINVAL;
    for (int64_t j = 0; j < n_jobs; j++)
        if (first[j + 1] < first[j]) return SA_EINVAL;
    const size_t n = (size_t) first[n_jobs];
    if (n > 0 && (!x || !y || !prob_e7)) return SA_EINVAL;
    std::vector<sa_pair16_t> recs(n);
    for (int64_t j = 0; j < n_jobs; j++)
        for (int64_t i = first[j]; i < first[j + 1]; i++) {
            if (x[i] < 0 || x[i] >= DV_MAX_COORD || y[i] < 0 || y[i] >= jobs[j].n_events || prob_e7[i] < 0 || prob_e7[i] > (int64_t) SA_PROB_1)
                return SA_EINVAL;
            recs[(size_t) i] = sa_pair16_pack(prob_e7[i], x[i], y[i], 0, 0);
        }
    if ((rc = sa_device_check(device)) != SA_OK) return rc;
    SaBatchView V;
    V.first.assign(first, first + n_jobs);
    V.count.resize((size_t) n_jobs);
    for (int64_t j = 0; j < n_jobs; j++) V.count[(size_t) j] = first[j + 1] - first[j];
    SaScratch &W = g_dv_ws;
    std::lock_guard<std::mutex> guard(W.mu);
    if ((rc = W.rebind(device)) != SA_OK || (rc = W.dev(DV_RECS, sizeof(sa_pair16_t) * (n ? n : 1))) != SA_OK) return rc;
    if (n && hipMemcpy(W.at(DV_RECS), recs.data(), sizeof(sa_pair16_t) * n, hipMemcpyHostToDevice) != hipSuccess) return SA_ENODEVICE;
    return dv_run(W, W.at(DV_RECS), false, V, in, P, flags, reads_out, sets_out, n_sets_out, hist_out, total_hist_out, events_out, kernel_ms_out);
}
