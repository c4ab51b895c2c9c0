// Labelled signal on gfx950: which reference position, k-mer and posterior every stretch of raw current belongs to -- the label sets
// of src/signalalign/alignedsignal.py (CreateLabels.add_mea_labels, add_signal_align_predictions, fix_sa_reference_indexes,
// AlignedSignal.generate_label_mapping, match_ref_position_with_raw_start_band) and mea_algorithm.py (match_events_with_signalalign,
// create_label_from_events) over the records of a finished batch (include/signalalign_hip.h has the rules and the differences).
//
// Every event of the call has one slot, job j's from ev_first[j] + j on (one spare slot per job: the end of its scan).  Kernels, all
// on stream 0, in launch order:
//   k_lb_count      one block per chunk (SaRecChunk, at most SA_CHAIN_CHUNK records of one job): the records per event (integer
//                   atomics) and, for the bands, the job's smallest and largest x (wave minima, one atomic per wave)
//   k_lb_scan<EV>   one block per job: the exclusive scan of the counts over the job's events (sa_block_excl_scan)
//   k_lb_scatter    per chunk: every record's ordinal into a free place of its event's range (the atomic hands places out in
//                   arrival order) ...
//   k_lb_order      ... and one lane per event puts the ordinals of its range in ascending order by ranking them (a range of more
//                   than LB_SMALL ordinals is ranked by the whole wave): the records by event, equal events in record order.
//                   Ordinals are distinct, so the result does not depend on the arrival order.
//   k_lb_full       per chunk: the full set, gathered through that order
//   k_lb_find       one thread per pair of the MEA paths: the walk over the ordered range of the pair's event for the records
//                   of its x; the lowest prob_e7 wins, among equals the first in record order
//   k_lb_scan<PATH> one block per job: the exclusive scan of "has a record" over the job's path
//   k_lb_band_acc   per chunk: smallest and largest y and the count per x (integer atomics; the x slots are laid out on the host
//                   from the jobs' x ranges, the call's one readback before the results)
//   k_lb_scan<X>    one block per job: the exclusive scan of "has a record" over the job's x slots
//   k_lb_job_scan   one block: every job's first MEA segment and first band, into the per-read records
//   k_lb_mea_emit   one thread per path pair: its segment, and its raw_start in an int32 array for the fill
//   k_lb_band_emit  one thread per x slot
//   k_lb_reads      one wave per job over its MEA segments: the per-read record
//   k_lb_fill       one block per tile of SA_LABEL_SAMPLE_TILE samples of one read: the segments of the tile's first and last
//                   sample by binary search over the segment starts (wave-uniform), then per sample a search inside that range from
//                   the thread's previous segment on; consecutive lanes store consecutive samples.  A pure write stream: 4 bytes
//                   per sample; the starts it reads (4 bytes per 9 samples at 5000 events per 45 000 samples) stay in cache.
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

#define LB_THREADS 256
#define LB_SMALL 16                 // ordinals of one event that a single lane ranks
#define LB_MAX_COORD (1ll << 28)
#define LB_ALL_FLAGS (SA_LABEL_MEA | SA_LABEL_FULL | SA_LABEL_BANDS | SA_LABEL_SAMPLES | SA_LABEL_TIMES)

struct LbJob {
    long long ev_first;     // first event in the call's raw_start / raw_length; the job's slots start at ev_first + job
    long long rec_first;    // first record in the view's records
    long long out_first;    // first record in the ordered arrays and the full set
    long long path_first;   // first pair in the call's paths; the job's path scan starts at path_first + job
    long long samp_first;   // first sample in the per-sample map
    long long x_first;      // first x slot; the job's band scan starts at x_first + job
    long long ref_first;
    int n_events, n_rec, n_path, n_samples, x_min, n_x, ref_step, base_shift;
};
struct LbTile { int job, t0; };
struct LbPair { int x, y; };

enum { LB_WS = 0, LB_RECS, LB_X, LB_SAMPLES };
static SaScratch g_lb_ws;
// HIP events around every kernel of the last SA_LABEL_TIMES call (under g_lb_ws.mu)
static hipEvent_t g_lb_ev[2 * SA_LABEL_N_KERNELS];
static bool g_lb_ev_made = false;
static double g_lb_last_ms[SA_LABEL_N_KERNELS];

extern "C" void sa_signal_labels_release(void) {
    std::lock_guard<std::mutex> guard(g_lb_ws.mu);
    if (g_lb_ev_made) {
        if (g_lb_ws.device >= 0) (void) hipSetDevice(g_lb_ws.device);
        for (hipEvent_t &e : g_lb_ev) (void) hipEventDestroy(e);
        g_lb_ev_made = false;
    }
    g_lb_ws.release();
}

extern "C" int sa_signal_labels_last_kernel_ms(double *out, int32_t n) {
    if (!out || n < 0) return SA_EINVAL;
    std::lock_guard<std::mutex> guard(g_lb_ws.mu);
    for (int k = 0; k < n && k < SA_LABEL_N_KERNELS; k++) out[k] = g_lb_last_ms[k];
    return SA_LABEL_N_KERNELS;
}

__device__ __forceinline__ void lb_rec(const sa_pair16_t *__restrict__ recs, long long i, int *x, int *y, int *kmer, long long *pe7) {
    const sa_pair16_t r = recs[i];
    *x = (int) (r.a & 0xfffffffull);
    *y = (int) ((r.a >> 28) & 0xfffffffull);
    *kmer = (int) (unsigned) (r.b & 0xffffffffull);
    *pe7 = (long long) ((r.b >> 32) & 0xffffffull);
}

__device__ __forceinline__ sa_label_segment_t lb_segment(const LbJob &J, const long long *__restrict__ raw_start,
                                                         const long long *__restrict__ raw_length, int x, int y, int kmer, long long pe7) {
    sa_label_segment_t s;
    s.raw_start = raw_start[J.ev_first + y];
    s.raw_length = raw_length[J.ev_first + y];
    s.reference_index = J.ref_first + (long long) J.ref_step * x + J.base_shift;
    s.x = x; s.y = y; s.kmer_id = kmer;
    s.prob_units = (int) sa_printed_units(pe7);
    return s;
}

// the last job whose `first` is <= i (jobs without entries share a first with their successor)
template <class First>
__device__ __forceinline__ int lb_job_of(First first, int nj, long long i) {
    int lo = 0, hi = nj - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first(mid) <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <bool BANDS>
__global__ __launch_bounds__(LB_THREADS) void k_lb_count(const sa_pair16_t *__restrict__ recs, const SaRecChunk *__restrict__ chunks,
                                                         const LbJob *__restrict__ jobs, int *__restrict__ cnt, int *__restrict__ xr) {
    const SaRecChunk C = chunks[blockIdx.x];
    const LbJob J = jobs[C.job];
    int *slot = cnt + J.ev_first + C.job;
    int lo = INT_MAX, hi = -1;
    for (int i = threadIdx.x; i < C.n; i += LB_THREADS) {
        int x, y, kmer;
        long long pe7;
        lb_rec(recs, C.first + i, &x, &y, &kmer, &pe7);
        if ((unsigned) y >= (unsigned) J.n_events) continue;   // (the host checked the caller's records, the batch its own: not reached)
        atomicAdd(&slot[y], 1);
        lo = min(lo, x);
        hi = max(hi, x);
    }
    if (BANDS) {
        for (int o = 32; o > 0; o >>= 1) {
            lo = min(lo, __shfl_xor(lo, o));
            hi = max(hi, __shfl_xor(hi, o));
        }
        if ((threadIdx.x & 63) == 0 && hi >= 0) {
            atomicMin(&xr[2 * C.job], lo);
            atomicMax(&xr[2 * C.job + 1], hi);
        }
    }
}

enum { LB_SCAN_EVENTS = 0, LB_SCAN_PATH, LB_SCAN_X };
// off[base .. base + n] of job blockIdx.x: the exclusive scan of src's counts (events) or of "is set" (path: found >= 0, x: count > 0)
template <int WHAT>
__global__ __launch_bounds__(SA_SCAN_THREADS) void k_lb_scan(const LbJob *__restrict__ jobs, const int *__restrict__ src,
                                                             long long *__restrict__ off) {
    const int j = blockIdx.x;
    const LbJob J = jobs[j];
    if (WHAT == LB_SCAN_EVENTS) {
        const int *s = src + J.ev_first + j;
        sa_block_excl_scan([&](int i) { return (long long) s[i]; }, off + J.ev_first + j, J.n_events);
    } else if (WHAT == LB_SCAN_PATH) {
        const int *s = src + J.path_first;
        sa_block_excl_scan([&](int i) { return (long long) (s[i] >= 0); }, off + J.path_first + j, J.n_path);
    } else {
        const int *s = src + J.x_first;
        sa_block_excl_scan([&](int i) { return (long long) (s[i] > 0); }, off + J.x_first + j, J.n_x);
    }
}

__global__ __launch_bounds__(LB_THREADS) void k_lb_scatter(const sa_pair16_t *__restrict__ recs, const SaRecChunk *__restrict__ chunks,
                                                           const LbJob *__restrict__ jobs, int *__restrict__ cnt,
                                                           const long long *__restrict__ yoff, int *__restrict__ tmp) {
    const SaRecChunk C = chunks[blockIdx.x];
    const LbJob J = jobs[C.job];
    const long long base = J.ev_first + C.job;
    for (int i = threadIdx.x; i < C.n; i += LB_THREADS) {
        int x, y, kmer;
        long long pe7;
        lb_rec(recs, C.first + i, &x, &y, &kmer, &pe7);
        if ((unsigned) y >= (unsigned) J.n_events) continue;
        const int place = atomicSub(&cnt[base + y], 1) - 1;   // the event's count places, each handed out once
        tmp[J.out_first + yoff[base + y] + place] = (int) C.local + i;
    }
}

__global__ __launch_bounds__(LB_THREADS) void k_lb_order(const LbJob *__restrict__ jobs, int nj, long long n_slots,
                                                         const long long *__restrict__ yoff, const int *__restrict__ tmp,
                                                         int *__restrict__ perm) {
    const long long e = (long long) blockIdx.x * LB_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    long long first = 0;
    int n = 0;
    if (e < n_slots) {
        const int j = lb_job_of([&](int q) { return jobs[q].ev_first; }, nj, e);
        const LbJob J = jobs[j];
        const long long at = e + j;   // (e - J.ev_first is the event; its slot is ev_first + j + event)
        first = J.out_first + yoff[at];
        n = (int) (yoff[at + 1] - yoff[at]);
    }
    if (n <= LB_SMALL) {
        for (int i = 0; i < n; i++) {
            const int v = tmp[first + i];
            int r = 0;
            for (int q = 0; q < n; q++) r += tmp[first + q] < v;
            perm[first + r] = v;
        }
    }
    unsigned long long big = __ballot(n > LB_SMALL);
    while (big) {   // wave-uniform: one long range at a time, ranked by all 64 lanes
        const int src = __ffsll((long long) big) - 1;
        big &= big - 1;
        const long long f = __shfl(first, src);
        const int m = __shfl(n, src);
        for (int i = lane; i < m; i += 64) {
            const int v = tmp[f + i];
            int r = 0;
            for (int q = 0; q < m; q++) r += tmp[f + q] < v;
            perm[f + r] = v;
        }
    }
}

__global__ __launch_bounds__(LB_THREADS) void k_lb_full(const sa_pair16_t *__restrict__ recs, const SaRecChunk *__restrict__ chunks,
                                                        const LbJob *__restrict__ jobs, const int *__restrict__ perm,
                                                        const long long *__restrict__ raw_start, const long long *__restrict__ raw_length,
                                                        sa_label_segment_t *__restrict__ full) {
    const SaRecChunk C = chunks[blockIdx.x];
    const LbJob J = jobs[C.job];
    for (int i = threadIdx.x; i < C.n; i += LB_THREADS) {
        const long long o = J.out_first + C.local + i;
        const int ord = perm[o];
        if ((unsigned) ord >= (unsigned) J.n_rec) continue;   // (an ordinal of the job: not reached)
        int x, y, kmer;
        long long pe7;
        lb_rec(recs, J.rec_first + ord, &x, &y, &kmer, &pe7);
        full[o] = lb_segment(J, raw_start, raw_length, x, y, kmer, pe7);
    }
}

__global__ __launch_bounds__(LB_THREADS) void k_lb_find(const sa_pair16_t *__restrict__ recs, const LbJob *__restrict__ jobs, int nj,
                                                        long long n_path, const LbPair *__restrict__ path,
                                                        const long long *__restrict__ yoff, const int *__restrict__ perm,
                                                        int *__restrict__ found) {
    const long long p = (long long) blockIdx.x * LB_THREADS + threadIdx.x;
    if (p >= n_path) return;
    const int j = lb_job_of([&](int q) { return jobs[q].path_first; }, nj, p);
    const LbJob J = jobs[j];
    const LbPair P = path[p];
    const long long at = J.ev_first + j + P.y;   // (the host checked the path's events)
    const long long a = J.out_first + yoff[at], b = J.out_first + yoff[at + 1];
    int best = -1;
    long long best_pe7 = 0;
    for (long long q = a; q < b; q++) {
        const int ord = perm[q];
        int x, y, kmer;
        long long pe7;
        lb_rec(recs, J.rec_first + ord, &x, &y, &kmer, &pe7);
        if (x == P.x && (best < 0 || pe7 < best_pe7)) { best = ord; best_pe7 = pe7; }
    }
    found[p] = best;
}

__global__ __launch_bounds__(LB_THREADS) void k_lb_band_acc(const sa_pair16_t *__restrict__ recs, const SaRecChunk *__restrict__ chunks,
                                                            const LbJob *__restrict__ jobs, int *__restrict__ xcnt, int *__restrict__ ymin,
                                                            int *__restrict__ ymax) {
    const SaRecChunk C = chunks[blockIdx.x];
    const LbJob J = jobs[C.job];
    for (int i = threadIdx.x; i < C.n; i += LB_THREADS) {
        int x, y, kmer;
        long long pe7;
        lb_rec(recs, C.first + i, &x, &y, &kmer, &pe7);
        const unsigned s = (unsigned) (x - J.x_min);
        if (s >= (unsigned) J.n_x || (unsigned) y >= (unsigned) J.n_events) continue;   // (x_min and n_x span the job's records: not reached)
        atomicAdd(&xcnt[J.x_first + s], 1);
        atomicMin(&ymin[J.x_first + s], y);
        atomicMax(&ymax[J.x_first + s], y);
    }
}

// every job's first MEA segment and first band: the exclusive scans of the jobs' totals
__global__ __launch_bounds__(SA_SCAN_THREADS) void k_lb_job_scan(const LbJob *__restrict__ jobs, int nj, const long long *__restrict__ poff,
                                                                 const long long *__restrict__ boff, long long *__restrict__ jm_off,
                                                                 long long *__restrict__ jb_off, sa_label_read_t *__restrict__ reads) {
    auto n_mea = [&](int j) { return poff ? poff[jobs[j].path_first + j + jobs[j].n_path] : 0ll; };
    auto n_bands = [&](int j) { return boff ? boff[jobs[j].x_first + j + jobs[j].n_x] : 0ll; };
    sa_block_excl_scan(n_mea, jm_off, nj);
    __syncthreads();
    sa_block_excl_scan(n_bands, jb_off, nj);
    __syncthreads();
    for (int j = threadIdx.x; j < nj; j += SA_SCAN_THREADS) {
        sa_label_read_t r;
        memset(&r, 0, sizeof(r));
        r.mea_first = jm_off[j]; r.n_mea = n_mea(j);
        r.band_first = jb_off[j]; r.n_bands = n_bands(j);
        r.full_first = jobs[j].out_first; r.n_full = jobs[j].n_rec;
        r.sample_first = jobs[j].samp_first; r.n_samples = jobs[j].n_samples;
        reads[j] = r;
    }
}

__global__ __launch_bounds__(LB_THREADS) void k_lb_mea_emit(const sa_pair16_t *__restrict__ recs, const LbJob *__restrict__ jobs, int nj,
                                                            long long n_path, const int *__restrict__ found,
                                                            const long long *__restrict__ poff, const sa_label_read_t *__restrict__ reads,
                                                            const long long *__restrict__ raw_start, const long long *__restrict__ raw_length,
                                                            sa_label_segment_t *__restrict__ mea, int *__restrict__ seg_start) {
    const long long p = (long long) blockIdx.x * LB_THREADS + threadIdx.x;
    if (p >= n_path) return;
    const int ord = found[p];
    if (ord < 0) return;
    const int j = lb_job_of([&](int q) { return jobs[q].path_first; }, nj, p);
    const LbJob J = jobs[j];
    int x, y, kmer;
    long long pe7;
    lb_rec(recs, J.rec_first + ord, &x, &y, &kmer, &pe7);
    const long long o = reads[j].mea_first + poff[p + j];   // (below the number of path pairs: the size of both arrays)
    const sa_label_segment_t s = lb_segment(J, raw_start, raw_length, x, y, kmer, pe7);
    mea[o] = s;
    seg_start[o] = (int) s.raw_start;
}

__global__ __launch_bounds__(LB_THREADS) void k_lb_band_emit(const LbJob *__restrict__ jobs, int nj, long long n_x,
                                                             const int *__restrict__ xcnt, const int *__restrict__ ymin,
                                                             const int *__restrict__ ymax, const long long *__restrict__ boff,
                                                             const sa_label_read_t *__restrict__ reads,
                                                             const long long *__restrict__ raw_start, const long long *__restrict__ raw_length,
                                                             sa_label_band_t *__restrict__ bands) {
    const long long s = (long long) blockIdx.x * LB_THREADS + threadIdx.x;
    if (s >= n_x) return;
    const int c = xcnt[s];
    if (c <= 0) return;
    const int j = lb_job_of([&](int q) { return jobs[q].x_first; }, nj, s);
    const LbJob J = jobs[j];
    const int x = J.x_min + (int) (s - J.x_first);
    const long long lo = raw_start[J.ev_first + ymin[s]], hi = raw_start[J.ev_first + ymax[s]];
    sa_label_band_t b;
    b.raw_start = lo;
    b.raw_length = hi - lo + raw_length[J.ev_first + ymax[s]];
    b.reference_index = J.ref_first + (long long) J.ref_step * x + J.base_shift;
    b.x = x;
    b.n_records = c;
    bands[reads[j].band_first + boff[s + j]] = b;   // (below the number of x slots with a record: at most the array's size)
}

__device__ __forceinline__ long long lb_wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(64) void k_lb_reads(const LbJob *__restrict__ jobs, const sa_label_segment_t *__restrict__ mea, int have_mea,
                                                 sa_label_read_t *__restrict__ reads) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const LbJob J = jobs[j];
    sa_label_read_t R = reads[j];
    const sa_label_segment_t *seg = mea + R.mea_first;
    const long long n = R.n_mea;
    long long stay = 0, skipped = 0, changes = 0;
    int carry = 0;   // the x of the segment before this step's first
    for (long long i0 = 0; i0 < n; i0 += 64) {
        const long long i = i0 + lane;
        const int x = i < n ? seg[i].x : 0;
        int prev = __shfl_up(x, 1);
        if (lane == 0) prev = carry;
        if (i < n && i > 0) {
            const int dx = x - prev, ab = dx < 0 ? -dx : dx;
            stay += dx == 0;
            changes += dx != 0;
            skipped += ab > 1 ? ab - 1 : 0;
        }
        carry = __shfl(x, 63);
    }
    stay = lb_wave_sum(stay);
    skipped = lb_wave_sum(skipped);
    changes = lb_wave_sum(changes);
    if (lane != 0) return;
    R.status = J.n_rec == 0 ? SA_LABEL_NO_RECORDS : (have_mea && J.n_path == 0 ? SA_LABEL_NO_PATH : 0);
    R.mea_without_record = J.n_path - n;
    R.stay_events = stay;
    R.skipped_positions = skipped;
    R.n_positions = n > 0 ? changes + 1 : 0;
    if (n > 0) {
        const sa_label_segment_t a = seg[0], z = seg[n - 1];
        R.minus_strand = a.reference_index >= z.reference_index;
        R.first_sample = a.raw_start;
        R.end_sample = z.raw_start + z.raw_length;
        R.labelled_samples = R.end_sample - R.first_sample;
    }
    reads[j] = R;
}

// the last segment of starts[lo .. hi) that starts at or before t; lo - 1 when none does
__device__ __forceinline__ int lb_last_le(const int *__restrict__ starts, int lo, int hi, int t) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

__global__ __launch_bounds__(LB_THREADS) void k_lb_fill(const LbTile *__restrict__ tiles, const LbJob *__restrict__ jobs,
                                                        const sa_label_read_t *__restrict__ reads, const int *__restrict__ seg_start,
                                                        int *__restrict__ samples) {
    const LbTile T = tiles[blockIdx.x];
    const LbJob J = jobs[T.job];
    const int n_seg = (int) reads[T.job].n_mea;
    const int end_last = (int) reads[T.job].end_sample;
    const int *starts = seg_start + reads[T.job].mea_first;
    int *out = samples + J.samp_first;
    const long long t_end = min((long long) T.t0 + SA_LABEL_SAMPLE_TILE, (long long) J.n_samples);   // (64 bits: n_samples may be 2^31 - 1)
    // the tile's segments: those of its first and of its last sample (wave-uniform searches)
    int cur = lb_last_le(starts, 0, n_seg, T.t0);
    const int last = lb_last_le(starts, cur < 0 ? 0 : cur, n_seg, (int) (t_end - 1));
    for (long long t = (long long) T.t0 + threadIdx.x; t < t_end; t += LB_THREADS) {
        cur = lb_last_le(starts, cur < 0 ? 0 : cur, last + 1, (int) t);
        out[t] = (cur < 0 || (cur == n_seg - 1 && t >= end_last)) ? -1 : cur;
    }
}

// what both calls check of their arguments, and what goes up: the jobs, the raw starts and lengths, the paths
struct LbInput {
    std::vector<LbJob> jobs;
    std::vector<long long> raw;   // all raw_start, then all raw_length
    std::vector<LbPair> path;
    long long n_slots = 0, n_samples = 0;
};
static int lb_check(const sa_label_job_t *jobs, int64_t n_jobs, const sa_mea_pair_t *const *mea_path, const int64_t *n_mea, unsigned flags,
                    sa_label_read_t *reads_out, sa_label_segment_t **mea_out, sa_label_segment_t **full_out, sa_label_band_t **bands_out,
                    int32_t **samples_out, LbInput *in) {
    if (n_jobs < 0 || (n_jobs > 0 && (!jobs || !reads_out)) || (flags & ~LB_ALL_FLAGS)) return SA_EINVAL;
    if ((flags & SA_LABEL_SAMPLES) && !(flags & SA_LABEL_MEA)) return SA_EINVAL;
    if (((flags & SA_LABEL_MEA) && !mea_out) || ((flags & SA_LABEL_FULL) && !full_out) || ((flags & SA_LABEL_BANDS) && !bands_out) ||
        ((flags & SA_LABEL_SAMPLES) && !samples_out))
        return SA_EINVAL;
    if ((mea_path == nullptr) != (n_mea == nullptr)) return SA_EINVAL;
    if (n_jobs > (int64_t) INT32_MAX) return SA_EUNSUPPORTED;
    const bool use_path = (flags & SA_LABEL_MEA) && mea_path;
    in->jobs.resize((size_t) n_jobs);
    long long n_slots = 0, n_path = 0, n_samples = 0;
    for (int64_t j = 0; j < n_jobs; j++) {
        const sa_label_job_t &q = jobs[j];
        if (q.n_events < 0 || q.n_events > LB_MAX_COORD || q.n_samples < 0) return SA_EINVAL;
        if (q.n_events > 0 && (!q.raw_start || !q.raw_length)) return SA_EINVAL;
        if (q.ref_step != 1 && q.ref_step != -1) return SA_EINVAL;
        if (use_path && (n_mea[j] < 0 || (n_mea[j] > 0 && !mea_path[j]))) return SA_EINVAL;
        for (int64_t y = 0; y < q.n_events; y++) {
            if (q.raw_start[y] < 0 || q.raw_length[y] < 1 || (y > 0 && q.raw_start[y] <= q.raw_start[y - 1])) return SA_EINVAL;
            if (q.raw_start[y] > q.n_samples || q.raw_length[y] > q.n_samples - q.raw_start[y]) return SA_EINVAL;
        }
        if (q.n_samples > (int64_t) INT32_MAX || (use_path && n_mea[j] > (int64_t) INT32_MAX)) return SA_EUNSUPPORTED;
        LbJob &J = in->jobs[(size_t) j];
        memset(&J, 0, sizeof(J));
        J.ev_first = n_slots; J.path_first = n_path; J.samp_first = n_samples; J.ref_first = q.ref_first;
        J.n_events = (int) q.n_events; J.n_samples = (int) q.n_samples; J.n_path = use_path ? (int) n_mea[j] : 0;
        J.ref_step = q.ref_step; J.base_shift = q.base_shift;
        n_slots += q.n_events;
        n_samples += q.n_samples;
        n_path += J.n_path;
    }
    in->n_slots = n_slots;
    in->n_samples = n_samples;
    in->raw.resize((size_t) (2 * n_slots));
    in->path.resize((size_t) n_path);
    size_t ip = 0;
    for (int64_t j = 0; j < n_jobs; j++) {
        const sa_label_job_t &q = jobs[j];
        const LbJob &J = in->jobs[(size_t) j];
        for (int64_t y = 0; y < q.n_events; y++) {
            in->raw[(size_t) (J.ev_first + y)] = q.raw_start[y];
            in->raw[(size_t) (n_slots + J.ev_first + y)] = q.raw_length[y];
        }
        for (int64_t i = 0; i < J.n_path; i++, ip++) {
            const int64_t x = mea_path[j][i].ref_idx, e = mea_path[j][i].event_idx;
            if (e < 0 || e >= q.n_events || x < 0 || x >= LB_MAX_COORD) return SA_EINVAL;
            if (i > 0 && e <= mea_path[j][i - 1].event_idx) return SA_EINVAL;   // a path names an event once, in ascending order
            in->path[ip] = LbPair{(int) x, (int) e};
        }
    }
    if (n_slots > (long long) INT32_MAX || n_samples > (long long) INT32_MAX || n_path > (long long) INT32_MAX) return SA_EUNSUPPORTED;
    return SA_OK;
}

static inline unsigned lb_blocks(size_t n) { return (unsigned) ((n + LB_THREADS - 1) / LB_THREADS); }

// the records `recs` (on W's device; job j's are V.first[j] .. + V.count[j]); the caller holds W.mu and has bound W to the device
static int lb_run(SaScratch &W, const sa_pair16_t *recs, const SaBatchView &V, LbInput &in, unsigned flags, sa_label_read_t *reads_out,
                  sa_label_segment_t **mea_out, sa_label_segment_t **full_out, sa_label_band_t **bands_out, int32_t **samples_out,
                  double *kernel_ms_out) {
    const bool want_mea = flags & SA_LABEL_MEA, want_full = flags & SA_LABEL_FULL, want_bands = flags & SA_LABEL_BANDS,
               want_samples = flags & SA_LABEL_SAMPLES, times = flags & SA_LABEL_TIMES;
    const size_t nj = in.jobs.size(), ns = (size_t) in.n_slots, np = in.path.size(), nsamp = want_samples ? (size_t) in.n_samples : 0;
    if (want_mea) *mea_out = nullptr;
    if (want_full) *full_out = nullptr;
    if (want_bands) *bands_out = nullptr;
    if (want_samples) *samples_out = nullptr;
    long long n_rec = 0;
    for (size_t j = 0; j < nj; j++) {
        if (V.count[j] > (long long) INT32_MAX) return SA_EUNSUPPORTED;
        in.jobs[j].rec_first = V.first[j]; in.jobs[j].out_first = n_rec; in.jobs[j].n_rec = (int) V.count[j];
        n_rec += V.count[j];
    }
    if (n_rec > (long long) INT32_MAX) return SA_EUNSUPPORTED;
    const size_t nr = (size_t) n_rec;
    sa_label_segment_t *h_mea = nullptr, *h_full = nullptr;
    sa_label_band_t *h_bands = nullptr;
    int32_t *h_samples = nullptr;
    int rc = SA_OK;
    float ms0 = 0, ms1 = 0;
    long long n_x = 0, n_mea_all = 0, n_bands_all = 0;
    for (double &v : g_lb_last_ms) v = 0.0;
    if (nj == 0) {
        if (want_mea) h_mea = (sa_label_segment_t *) malloc(sizeof(sa_label_segment_t));
        if (want_full) h_full = (sa_label_segment_t *) malloc(sizeof(sa_label_segment_t));
        if (want_bands) h_bands = (sa_label_band_t *) malloc(sizeof(sa_label_band_t));
        if (want_samples) h_samples = (int32_t *) malloc(sizeof(int32_t));
        if ((want_mea && !h_mea) || (want_full && !h_full) || (want_bands && !h_bands) || (want_samples && !h_samples)) { rc = SA_ENOMEM; goto done; }
        goto out;
    }
    {
        const std::vector<SaRecChunk> chunks = sa_view_chunks(V, SA_CHAIN_CHUNK, SA_ORDINAL_PER_JOB);
        const size_t nc = chunks.size();
        std::vector<LbTile> tiles;
        if (want_samples)
            for (size_t j = 0; j < nj; j++)
                for (long long t0 = 0; t0 < in.jobs[j].n_samples; t0 += SA_LABEL_SAMPLE_TILE) tiles.push_back(LbTile{(int) j, (int) t0});
        const size_t nt = tiles.size();
        if (nc > (size_t) INT32_MAX || nt > (size_t) INT32_MAX) return SA_EUNSUPPORTED;
        // [jobs | chunks | tiles | raw starts, lengths | paths | counts per event | their scan | unordered, ordered ordinals | found |
        //  its scan | x ranges | job scans | reads | MEA segments | their starts | full set]; the x slots and the samples are blocks
        // of their own (LB_X, LB_SAMPLES)
        SaLayout L;
        const size_t o_jobs = L.add(sizeof(LbJob) * nj), o_ch = L.add(sizeof(SaRecChunk) * nc), o_tiles = L.add(sizeof(LbTile) * nt),
                     o_raw = L.add(8 * 2 * ns), o_path = L.add(sizeof(LbPair) * np), o_cnt = L.add(4 * (ns + nj)),
                     o_yoff = L.add(8 * (ns + nj)), o_tmp = L.add(4 * nr), o_perm = L.add(4 * nr), o_found = L.add(4 * np),
                     o_poff = L.add(8 * (np + nj)), o_xr = L.add(8 * nj), o_joff = L.add(8 * 2 * (nj + 1)),
                     o_reads = L.add(sizeof(sa_label_read_t) * nj), o_mea = L.add(sizeof(sa_label_segment_t) * np), o_sst = L.add(4 * np),
                     o_full = L.add(want_full ? sizeof(sa_label_segment_t) * nr : 0);
        if ((rc = W.dev(LB_WS, L.end)) != SA_OK) return rc;
        if (want_samples && (rc = W.dev(LB_SAMPLES, 4 * (nsamp ? nsamp : 1))) != SA_OK) return rc;
        if (times && !g_lb_ev_made) {
            for (hipEvent_t &e : g_lb_ev) SA_HIP_GOTO_DONE(hipEventCreate(&e));
            g_lb_ev_made = true;
        }
        bool ran[SA_LABEL_N_KERNELS] = {};
        auto begin = [&](int k) { if (times) { (void) hipEventRecord(g_lb_ev[2 * k], 0); ran[k] = true; } };
        auto end = [&](int k) { if (times) (void) hipEventRecord(g_lb_ev[2 * k + 1], 0); };
        char *d = (char *) W.at(LB_WS);
        const LbJob *d_jobs = (const LbJob *) (d + o_jobs);
        const SaRecChunk *d_ch = (const SaRecChunk *) (d + o_ch);
        const long long *d_rs = (const long long *) (d + o_raw), *d_rl = d_rs + ns;
        int *d_cnt = (int *) (d + o_cnt), *d_tmp = (int *) (d + o_tmp), *d_perm = (int *) (d + o_perm), *d_found = (int *) (d + o_found),
            *d_xr = (int *) (d + o_xr), *d_sst = (int *) (d + o_sst);
        long long *d_yoff = (long long *) (d + o_yoff), *d_poff = (long long *) (d + o_poff), *d_joff = (long long *) (d + o_joff);
        sa_label_read_t *d_reads = (sa_label_read_t *) (d + o_reads);
        sa_label_segment_t *d_mea = (sa_label_segment_t *) (d + o_mea), *d_full = (sa_label_segment_t *) (d + o_full);
        const dim3 per_chunk((unsigned) nc), per_job((unsigned) nj), block(LB_THREADS), scan_block(SA_SCAN_THREADS);
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_jobs, in.jobs.data(), sizeof(LbJob) * nj, hipMemcpyHostToDevice, 0));
        if (nc) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_ch, chunks.data(), sizeof(SaRecChunk) * nc, hipMemcpyHostToDevice, 0));
        if (nt) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_tiles, tiles.data(), sizeof(LbTile) * nt, hipMemcpyHostToDevice, 0));
        if (ns) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_raw, in.raw.data(), 8 * 2 * ns, hipMemcpyHostToDevice, 0));
        if (np) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_path, in.path.data(), sizeof(LbPair) * np, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(W.time_begin());
        SA_HIP_GOTO_DONE(hipMemsetAsync(d_cnt, 0, 4 * (ns + nj), 0));
        if (want_bands) {
            std::vector<int> xr(2 * nj);
            for (size_t j = 0; j < nj; j++) { xr[2 * j] = INT_MAX; xr[2 * j + 1] = -1; }
            SA_HIP_GOTO_DONE(hipMemcpy(d_xr, xr.data(), 8 * nj, hipMemcpyHostToDevice));
        }
        if (nc) {
            begin(SA_LABEL_K_COUNT);
            if (want_bands) hipLaunchKernelGGL(k_lb_count<true>, per_chunk, block, 0, 0, recs, d_ch, d_jobs, d_cnt, d_xr);
            else hipLaunchKernelGGL(k_lb_count<false>, per_chunk, block, 0, 0, recs, d_ch, d_jobs, d_cnt, d_xr);
            end(SA_LABEL_K_COUNT);
        }
        begin(SA_LABEL_K_SCAN_EVENTS);
        hipLaunchKernelGGL(k_lb_scan<LB_SCAN_EVENTS>, per_job, scan_block, 0, 0, d_jobs, (const int *) d_cnt, d_yoff);
        end(SA_LABEL_K_SCAN_EVENTS);
        if (nc && (want_mea || want_full)) {
            begin(SA_LABEL_K_SCATTER);
            hipLaunchKernelGGL(k_lb_scatter, per_chunk, block, 0, 0, recs, d_ch, d_jobs, d_cnt, (const long long *) d_yoff, d_tmp);
            end(SA_LABEL_K_SCATTER);
            begin(SA_LABEL_K_ORDER);
            hipLaunchKernelGGL(k_lb_order, dim3(lb_blocks(ns)), block, 0, 0, d_jobs, (int) nj, (long long) ns, (const long long *) d_yoff,
                               (const int *) d_tmp, d_perm);
            end(SA_LABEL_K_ORDER);
        }
        if (nc && want_full) {
            begin(SA_LABEL_K_FULL);
            hipLaunchKernelGGL(k_lb_full, per_chunk, block, 0, 0, recs, d_ch, d_jobs, (const int *) d_perm, d_rs, d_rl, d_full);
            end(SA_LABEL_K_FULL);
        }
        if (np) {
            begin(SA_LABEL_K_FIND);
            hipLaunchKernelGGL(k_lb_find, dim3(lb_blocks(np)), block, 0, 0, recs, d_jobs, (int) nj, (long long) np,
                               (const LbPair *) (d + o_path), (const long long *) d_yoff, (const int *) d_perm, d_found);
            end(SA_LABEL_K_FIND);
        }
        if (want_mea) {
            begin(SA_LABEL_K_SCAN_PATH);
            hipLaunchKernelGGL(k_lb_scan<LB_SCAN_PATH>, per_job, scan_block, 0, 0, d_jobs, (const int *) d_found, d_poff);
            end(SA_LABEL_K_SCAN_PATH);
        }
        int *d_xcnt = nullptr, *d_ymin = nullptr, *d_ymax = nullptr;
        long long *d_boff = nullptr;
        sa_label_band_t *d_bands = nullptr;
        if (want_bands) {
            // the one readback before the results: every job's x range, from which the x slots are laid out
            std::vector<int> xr(2 * nj);
            SA_HIP_GOTO_DONE(W.time_end());
            SA_HIP_GOTO_DONE(hipMemcpy(xr.data(), d_xr, 8 * nj, hipMemcpyDeviceToHost));
            SA_HIP_GOTO_DONE(W.time_ms(&ms0));
            for (size_t j = 0; j < nj; j++) {
                LbJob &J = in.jobs[j];
                J.x_first = n_x;
                J.x_min = xr[2 * j + 1] >= 0 ? xr[2 * j] : 0;
                J.n_x = xr[2 * j + 1] >= 0 ? xr[2 * j + 1] - xr[2 * j] + 1 : 0;
                n_x += J.n_x;
            }
            if (n_x > (long long) INT32_MAX) { rc = SA_EUNSUPPORTED; goto done; }
            const size_t nx = (size_t) n_x, nb = nx < nr ? nx : nr;   // (a band has a record)
            SaLayout X;
            const size_t o_xcnt = X.add(4 * nx), o_ymax = X.add(4 * nx), o_ymin = X.add(4 * nx), o_boff = X.add(8 * (nx + nj)),
                         o_bands = X.add(sizeof(sa_label_band_t) * nb);
            if ((rc = W.dev(LB_X, X.end)) != SA_OK) goto done;
            char *dx = (char *) W.at(LB_X);
            d_xcnt = (int *) (dx + o_xcnt); d_ymax = (int *) (dx + o_ymax); d_ymin = (int *) (dx + o_ymin);
            d_boff = (long long *) (dx + o_boff); d_bands = (sa_label_band_t *) (dx + o_bands);
            SA_HIP_GOTO_DONE(hipMemcpy(d + o_jobs, in.jobs.data(), sizeof(LbJob) * nj, hipMemcpyHostToDevice));
            SA_HIP_GOTO_DONE(W.time_begin());
            if (nx) {
                SA_HIP_GOTO_DONE(hipMemsetAsync(dx + o_xcnt, 0, o_ymin - o_xcnt, 0));          // counts and largest y: 0
                SA_HIP_GOTO_DONE(hipMemsetAsync(d_ymin, 0x7f, 4 * nx, 0));                     // smallest y: above every event
                begin(SA_LABEL_K_BAND_ACC);
                hipLaunchKernelGGL(k_lb_band_acc, per_chunk, block, 0, 0, recs, d_ch, d_jobs, d_xcnt, d_ymin, d_ymax);
                end(SA_LABEL_K_BAND_ACC);
            }
            begin(SA_LABEL_K_SCAN_BANDS);
            hipLaunchKernelGGL(k_lb_scan<LB_SCAN_X>, per_job, scan_block, 0, 0, d_jobs, (const int *) d_xcnt, d_boff);
            end(SA_LABEL_K_SCAN_BANDS);
        }
        begin(SA_LABEL_K_JOB_SCAN);
        hipLaunchKernelGGL(k_lb_job_scan, dim3(1), scan_block, 0, 0, d_jobs, (int) nj, (const long long *) (want_mea ? d_poff : nullptr),
                           (const long long *) d_boff, d_joff, d_joff + nj + 1, d_reads);
        end(SA_LABEL_K_JOB_SCAN);
        if (np) {
            begin(SA_LABEL_K_MEA_EMIT);
            hipLaunchKernelGGL(k_lb_mea_emit, dim3(lb_blocks(np)), block, 0, 0, recs, d_jobs, (int) nj, (long long) np, (const int *) d_found,
                               (const long long *) d_poff, (const sa_label_read_t *) d_reads, d_rs, d_rl, d_mea, d_sst);
            end(SA_LABEL_K_MEA_EMIT);
        }
        if (want_bands && n_x) {
            begin(SA_LABEL_K_BAND_EMIT);
            hipLaunchKernelGGL(k_lb_band_emit, dim3(lb_blocks((size_t) n_x)), block, 0, 0, d_jobs, (int) nj, n_x, (const int *) d_xcnt,
                               (const int *) d_ymin, (const int *) d_ymax, (const long long *) d_boff, (const sa_label_read_t *) d_reads,
                               d_rs, d_rl, d_bands);
            end(SA_LABEL_K_BAND_EMIT);
        }
        begin(SA_LABEL_K_READS);
        hipLaunchKernelGGL(k_lb_reads, per_job, dim3(64), 0, 0, d_jobs, (const sa_label_segment_t *) d_mea, want_mea ? 1 : 0, d_reads);
        end(SA_LABEL_K_READS);
        if (nt) {
            begin(SA_LABEL_K_FILL);
            hipLaunchKernelGGL(k_lb_fill, dim3((unsigned) nt), block, 0, 0, (const LbTile *) (d + o_tiles), d_jobs,
                               (const sa_label_read_t *) d_reads, (const int *) d_sst, (int *) W.at(LB_SAMPLES));
            end(SA_LABEL_K_FILL);
        }
        SA_HIP_GOTO_DONE(W.time_end());
        SA_HIP_GOTO_DONE(hipMemcpy(reads_out, d_reads, sizeof(sa_label_read_t) * nj, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(W.time_ms(&ms1));
        for (int k = 0; times && k < SA_LABEL_N_KERNELS; k++) {
            float ms = 0;
            if (ran[k]) SA_HIP_GOTO_DONE(hipEventElapsedTime(&ms, g_lb_ev[2 * k], g_lb_ev[2 * k + 1]));
            g_lb_last_ms[k] = ms;
        }
        n_mea_all = reads_out[nj - 1].mea_first + reads_out[nj - 1].n_mea;
        n_bands_all = reads_out[nj - 1].band_first + reads_out[nj - 1].n_bands;
        if (want_mea) h_mea = (sa_label_segment_t *) malloc(sizeof(sa_label_segment_t) * (size_t) (n_mea_all > 0 ? n_mea_all : 1));
        if (want_full) h_full = (sa_label_segment_t *) malloc(sizeof(sa_label_segment_t) * (nr ? nr : 1));
        if (want_bands) h_bands = (sa_label_band_t *) malloc(sizeof(sa_label_band_t) * (size_t) (n_bands_all > 0 ? n_bands_all : 1));
        if (want_samples) h_samples = (int32_t *) malloc(4 * (nsamp ? nsamp : 1));
        if ((want_mea && !h_mea) || (want_full && !h_full) || (want_bands && !h_bands) || (want_samples && !h_samples)) { rc = SA_ENOMEM; goto done; }
        if (want_mea && n_mea_all > 0)
            SA_HIP_GOTO_DONE(hipMemcpy(h_mea, d_mea, sizeof(sa_label_segment_t) * (size_t) n_mea_all, hipMemcpyDeviceToHost));
        if (want_full && nr) SA_HIP_GOTO_DONE(hipMemcpy(h_full, d_full, sizeof(sa_label_segment_t) * nr, hipMemcpyDeviceToHost));
        if (want_bands && n_bands_all > 0)
            SA_HIP_GOTO_DONE(hipMemcpy(h_bands, d_bands, sizeof(sa_label_band_t) * (size_t) n_bands_all, hipMemcpyDeviceToHost));
        if (want_samples && nsamp) SA_HIP_GOTO_DONE(hipMemcpy(h_samples, W.at(LB_SAMPLES), 4 * nsamp, hipMemcpyDeviceToHost));
    }
out:
    if (kernel_ms_out) *kernel_ms_out = (double) ms0 + (double) ms1;
    if (want_mea) *mea_out = h_mea;
    if (want_full) *full_out = h_full;
    if (want_bands) *bands_out = h_bands;
    if (want_samples) *samples_out = h_samples;
    return SA_OK;
done:
    (void) hipStreamSynchronize(0);
    free(h_mea);
    free(h_full);
    free(h_bands);
    free(h_samples);
    return rc;
}

extern "C" int sa_batch_signal_labels(sa_batch_t *b, const sa_label_job_t *jobs, int64_t n_jobs, const sa_mea_pair_t *const *mea_path,
                                      const int64_t *n_mea, unsigned flags, sa_label_read_t *reads_out, sa_label_segment_t **mea_out,
                                      sa_label_segment_t **full_out, sa_label_band_t **bands_out, int32_t **samples_out,
                                      double *kernel_ms_out) {
    if (!b) return SA_EINVAL;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    LbInput in;
    int rc = lb_check(jobs, n_jobs, mea_path, n_mea, flags, reads_out, mea_out, full_out, bands_out, samples_out, &in);
    if (rc) return rc;
    SaScratch &W = g_lb_ws;
    std::lock_guard<std::mutex> guard(W.mu);
    SaBatchView V;
    rc = sa_batch_view(b, &V);
    // (8-byte records name no k-mer, and a batch filtered for the variant-caller output dropped rows: as sa_batch_mea answers)
    if (V.p8 || (V.batch_flags & SA_FLAG_VC_ROWS)) return SA_ESTATE;
    if (rc) return rc;
    if (V.batch_flags & SA_FLAG_EXPECT_INTERNAL) return SA_ESTATE;
    if ((int64_t) V.count.size() != n_jobs) return SA_EINVAL;
    for (int64_t j = 0; j < n_jobs; j++)
        if (V.n_events[(size_t) j] != jobs[j].n_events) return SA_EINVAL;
    if ((rc = W.rebind(V.device)) != SA_OK) return rc;
    return lb_run(W, (const sa_pair16_t *) V.recs, V, in, flags, reads_out, mea_out, full_out, bands_out, samples_out, kernel_ms_out);
}

extern "C" int sa_signal_labels_records(const sa_label_job_t *jobs, int64_t n_jobs, const int64_t *first, const int32_t *x, const int32_t *y,
                                        const int32_t *kmer_id, const int64_t *prob_e7, const sa_mea_pair_t *const *mea_path,
                                        const int64_t *n_mea, int device, unsigned flags, sa_label_read_t *reads_out,
                                        sa_label_segment_t **mea_out, sa_label_segment_t **full_out, sa_label_band_t **bands_out,
                                        int32_t **samples_out, double *kernel_ms_out) {
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    LbInput in;
    int rc = lb_check(jobs, n_jobs, mea_path, n_mea, flags, reads_out, mea_out, full_out, bands_out, samples_out, &in);
    if (rc) return rc;
    if (!first || first[0] != 0) return SA_EINVAL;
    for (int64_t j = 0; j < n_jobs; j++)
        if (first[j + 1] < first[j]) return SA_EINVAL;
    if (first[n_jobs] > (int64_t) INT32_MAX) return SA_EUNSUPPORTED;
    const size_t n = (size_t) first[n_jobs];
    if (n > 0 && (!x || !y || !kmer_id || !prob_e7)) return SA_EINVAL;
    std::vector<sa_pair16_t> recs(n);
    for (int64_t j = 0; j < n_jobs; j++)
        for (int64_t i = first[j]; i < first[j + 1]; i++) {
            if (x[i] < 0 || x[i] >= LB_MAX_COORD || y[i] < 0 || y[i] >= jobs[j].n_events || prob_e7[i] < 0 || prob_e7[i] > (int64_t) SA_PROB_1)
                return SA_EINVAL;
            recs[(size_t) i] = sa_pair16_pack(prob_e7[i], x[i], y[i], 0, kmer_id[i]);
        }
    if ((rc = sa_device_check(device)) != SA_OK) return rc;
    SaBatchView V;
    V.first.assign(first, first + n_jobs);
    V.count.resize((size_t) n_jobs);
    for (int64_t j = 0; j < n_jobs; j++) V.count[(size_t) j] = first[j + 1] - first[j];
    SaScratch &W = g_lb_ws;
    std::lock_guard<std::mutex> guard(W.mu);
    if ((rc = W.rebind(device)) != SA_OK || (rc = W.dev(LB_RECS, sizeof(sa_pair16_t) * (n ? n : 1))) != SA_OK) return rc;
    if (n && hipMemcpy(W.at(LB_RECS), recs.data(), sizeof(sa_pair16_t) * n, hipMemcpyHostToDevice) != hipSuccess) return SA_ENODEVICE;
    return lb_run(W, (const sa_pair16_t *) W.at(LB_RECS), V, in, flags, reads_out, mea_out, full_out, bands_out, samples_out, kernel_ms_out);
}
