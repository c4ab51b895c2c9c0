// Call quality on gfx950 -- call accuracy against the alignment's distance from its guide
// (visualization/plot_accuracy_vs_alignment_deviation.py over get_distance_from_guide_alignment and
// match_ref_position_with_raw_start_band, src/signalalign/alignedsignal.py:388-443) and the breaks of the MEA path
// (visualization/plot_breaks_in_alignments.py, find_gaps_in_alignment_data, :139-148), over the sites and records of a finished
// SA_FLAG_SITE_CALLS batch (include/signalalign_hip.h has the rules and the deliberate differences).
//
// Kernels, all on stream 0, after the fold that sa_batch_site_calls shares (SaSiteFold):
//   k_cq_band     one block per chunk (SaRecChunk, at most SA_CHAIN_CHUNK records of one job): a binary search of the record's x in
//                 the job's ascending site x, then a 32-bit atomic minimum and maximum of its y into the site's y_min / y_max.  The
//                 block first combines, per tile of CQ_BTILE records, the y of the sites within CQ_WIN of the tile's lowest site
//                 in LDS and flushes the touched ones with one global atomic pair each; a record outside the window goes straight
//                 to the global atomics, so the result never depends on the window.  A site batch holds tens of records per site,
//                 and the window won beyond the spread of three calls (profiles/call_quality.json); SA_CQ_BAND_DIRECT keeps the
//                 plain path, a global atomic pair per record, for the A/B.
//   k_cq_calls    one wave per tile (at most CQ_TILE sites of one job), 64 sites a step: the label (sc_site_label, as k_score_sites),
//                 the band, the guide row by binary search of the job's anchor_x, delta2 and the histogram slot.  The count pass
//                 keeps the histogram in LDS and flushes it with 64-bit integer atomics into the job's row and the summed one, adds
//                 the wave-reduced sums to the job's accumulator with integer atomics and leaves the tile's number of calls; the
//                 write pass -- after k_cq_finish has scanned the tiles' counts -- writes every call at the tile's offset plus its
//                 rank among the step's ballot, so a job's calls lie in ascending x whatever the launch shape.
//   k_cq_gaps     one wave per job, 64 path pairs a step: the pair's end is handed to the next lane, lane 63's carried into the next
//                 step; gaps counted (and, in the write pass, ranked) by ballot.
//   k_cq_finish   one block: the exclusive scans of the tiles' calls and of the jobs' gaps (sa_block_excl_scan), then every job's
//                 sa_callq_read_t from its accumulators.
// The host reads the two totals once to size the blocks of calls and gaps, and the results once.  No host pass over records,
// sites or path pairs.  Everything is an integer but prob > threshold, so nothing depends on launch shape or atomic order.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "sa_internal.h"
#include "sa_chain.h"
#include "sa_scratch.h"
#include "sa_site_label.h"

#define CQ_THREADS 256
#define CQ_TILE 1024       // sites of a wave of k_cq_calls
#define CQ_BTILE 2048      // records of a tile of the windowed k_cq_band
#define CQ_WIN 1024        // sites of its window: 8 KiB of LDS
#define CQ_MAX_COORD (1ll << 28)
#define CQ_MAX_GRID (1ll << 40)
#define CQ_X_MASK 0xfffffffull

struct CqJob {
    long long ev_first;     // the job's first event in the call's raw_start / raw_length
    long long anc_first;    // its first anchor in the call's anchor arrays
    long long path_first;   // its first pair in the call's path events
    int n_events, n_anchors, n_path;
    int tile_first;         // the job's first tile (the next job's when it has none)
};
struct CqTile {
    long long s0;   // first site
    int n, job;
};
struct CqAcc {      // per job, added to by the waves of its tiles
    unsigned long long n_calls, n_correct, n_unlabelled, n_other, n_outside, sum_abs, max_key, pad;   // max_key: abs << 28 | ~x
};
struct CqGapAcc {
    long long n_gaps, sum_gap, max_gap, pad;
};
struct CqGrid {
    long long lo2, w2;   // 2 * bin_lo, 2 * bin_width
    int n_bins, min_gap;
};

enum { CQ_WS = 0, CQ_SITES, CQ_RECS, CQ_CALLS, CQ_GAPS };
enum { CQ_EV_BAND = 0, CQ_EV_CALLS, CQ_EV_GAPS, CQ_EV_CALLS_W, CQ_EV_GAPS_W, CQ_EV_N };
static SaScratch g_cq_ws;
static hipEvent_t g_cq_ev[2 * CQ_EV_N];
static bool g_cq_ev_made = false;
static double g_cq_last_ms[3] = {0.0, 0.0, 0.0};

extern "C" void sa_call_quality_release(void) {
    std::lock_guard<std::mutex> guard(g_cq_ws.mu);
    g_cq_ws.release();
}

extern "C" int sa_call_quality_last_kernel_ms(double *out, int32_t n) {
    std::lock_guard<std::mutex> guard(g_cq_ws.mu);
    for (int i = 0; out && i < 3 && i < n; i++) out[i] = g_cq_last_ms[i];
    return 3;
}

// the site of x among x_of_site[s0 .. s1) (ascending), -1 when it is none
__device__ __forceinline__ long long cq_site_of(const int *__restrict__ x_of_site, long long s0, long long s1, int x) {
    long long lo = s0, hi = s1;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (x_of_site[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < s1 && x_of_site[lo] == x ? lo : -1;
}

template <bool WINDOW>
__global__ __launch_bounds__(CQ_THREADS) void k_cq_band(const sa_pair16_t *__restrict__ recs, const SaRecChunk *__restrict__ chunks,
                                                        const CqJob *__restrict__ jobs, const long long *__restrict__ site_off,
                                                        const int *__restrict__ x_of_site, int *__restrict__ ymin, int *__restrict__ ymax) {
    __shared__ int w_min[WINDOW ? CQ_WIN : 1], w_max[WINDOW ? CQ_WIN : 1];
    __shared__ long long s_base;
    const SaRecChunk C = chunks[blockIdx.x];
    const long long s0 = site_off[C.job], s1 = site_off[C.job + 1];
    const int n_events = jobs[C.job].n_events;
    if (s0 == s1) return;
    if (!WINDOW) {
        for (int i = threadIdx.x; i < C.n; i += CQ_THREADS) {
            const unsigned long long a = recs[C.first + i].a;
            const int x = (int) (a & CQ_X_MASK), y = (int) ((a >> 28) & CQ_X_MASK);
            if (y >= n_events) continue;   // (the host checked the caller's records, the batch its own: not reached)
            const long long s = cq_site_of(x_of_site, s0, s1, x);
            if (s < 0) continue;
            atomicMin(&ymin[s], y);
            atomicMax(&ymax[s], y);
        }
        return;
    }
    for (int t0 = 0; t0 < C.n; t0 += CQ_BTILE) {
        const int tn = min(CQ_BTILE, C.n - t0);
        long long site[CQ_BTILE / CQ_THREADS];
        int ys[CQ_BTILE / CQ_THREADS];
        if (threadIdx.x == 0) s_base = LLONG_MAX;
        for (int e = threadIdx.x; e < CQ_WIN; e += CQ_THREADS) { w_min[e] = INT_MAX; w_max[e] = -1; }
        __syncthreads();
        long long lo = LLONG_MAX;
#pragma unroll
        for (int q = 0; q < CQ_BTILE / CQ_THREADS; q++) {
            const int i = q * CQ_THREADS + threadIdx.x;
            site[q] = -1;
            ys[q] = 0;
            if (i < tn) {
                const unsigned long long a = recs[C.first + t0 + i].a;
                const int x = (int) (a & CQ_X_MASK), y = (int) ((a >> 28) & CQ_X_MASK);
                if (y < n_events) {
                    site[q] = cq_site_of(x_of_site, s0, s1, x);
                    ys[q] = y;
                    if (site[q] >= 0 && site[q] < lo) lo = site[q];
                }
            }
        }
        if (lo != LLONG_MAX) atomicMin(&s_base, lo);
        __syncthreads();
        const long long base = s_base;
#pragma unroll
        for (int q = 0; q < CQ_BTILE / CQ_THREADS; q++) {
            if (site[q] < 0) continue;
            const long long w = site[q] - base;
            if (w < (long long) CQ_WIN) {
                atomicMin(&w_min[w], ys[q]);
                atomicMax(&w_max[w], ys[q]);
            } else {
                atomicMin(&ymin[site[q]], ys[q]);
                atomicMax(&ymax[site[q]], ys[q]);
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < CQ_WIN; e += CQ_THREADS)
            if (w_max[e] >= 0) {   // (a touched slot: base + e is the site of a record of the tile)
                atomicMin(&ymin[base + e], w_min[e]);
                atomicMax(&ymax[base + e], w_max[e]);
            }
        __syncthreads();
    }
}

// The guide row of a call at x: the anchor with anchor_x == x (of several the first for x_sign +1, the last for -1), else for
// x_sign +1 the last anchor with anchor_x < x and for -1 the first with anchor_x > x; -1 when the call is outside the guide.
__host__ __device__ static inline int cq_guide_row(const int *ax, int n, int x, int x_sign) {
    int lo = 0, hi = n;
    if (x_sign > 0) {   // the first anchor with anchor_x >= x
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ax[mid] < x) lo = mid + 1;
            else hi = mid;
        }
        if (lo == n) return -1;          // no anchor at or beyond the call
        return ax[lo] == x ? lo : lo - 1;   // (lo - 1 == -1: no row before the call)
    }
    while (lo < hi) {       // the first anchor with anchor_x > x
        const int mid = (lo + hi) >> 1;
        if (ax[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return -1;              // no anchor at or beyond the call, in descending x
    if (ax[lo - 1] == x) return lo - 1;
    return lo == n ? -1 : lo;            // (no row before the call, in descending x)
}

// np.round(raw_start + raw_length / 2) in integers: half goes to the even neighbour
__host__ __device__ static inline long long cq_round_mid(long long raw_start, long long raw_length) {
    if (!(raw_length & 1)) return raw_start + raw_length / 2;
    const long long below = raw_start + (raw_length - 1) / 2;
    return (below & 1) ? below + 1 : below;
}

__device__ __forceinline__ unsigned long long cq_wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long cq_wave_max(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o);
        v = u > v ? u : v;
    }
    return v;
}

struct CqSites {   // the sites of a call on its device, as SaSiteFold has them
    const long long *site_off;        // nj + 1
    const unsigned char *kind, *kind_ok;
    const int *x_of_site;
    const unsigned long long *units;
    const double *prob;
    int stride;
};

template <bool WRITE>
__global__ __launch_bounds__(64) void k_cq_calls(const CqTile *__restrict__ tiles, const ScJob *__restrict__ sjobs,
                                                 const CqJob *__restrict__ jobs, CqSites S, ScTruth T, double threshold,
                                                 const int *__restrict__ ymin, const int *__restrict__ ymax, const int *__restrict__ ax,
                                                 const int *__restrict__ ay, const int *__restrict__ raw_start,
                                                 const int *__restrict__ raw_length, CqGrid G, CqAcc *__restrict__ acc,
                                                 unsigned long long *__restrict__ hist, unsigned long long *__restrict__ total_hist,
                                                 long long *__restrict__ tile_cnt, const long long *__restrict__ tile_off,
                                                 sa_callq_call_t *__restrict__ calls) {
    __shared__ int s_hist[WRITE ? 1 : (SA_CQ_MAX_BINS + 2) * 2];
    const int lane = threadIdx.x;
    const CqTile Tl = tiles[blockIdx.x];
    const ScJob J = sjobs[Tl.job];
    const CqJob Q = jobs[Tl.job];
    const int n_slots = (G.n_bins + 2) * 2;
    const int *rs = raw_start + Q.ev_first, *rl = raw_length + Q.ev_first;
    const int *jx = ax + Q.anc_first, *jy = ay + Q.anc_first;
    if (!WRITE) {
        for (int q = lane; q < n_slots; q += 64) s_hist[q] = 0;
        __syncthreads();
    }
    unsigned long long n_calls = 0, n_correct = 0, n_unl = 0, n_oth = 0, n_out = 0;   // wave-uniform
    unsigned long long sum_abs = 0, max_key = 0;                                       // the lane's own
    long long w = WRITE ? tile_off[blockIdx.x] : 0;
    for (int base = 0; base < Tl.n; base += 64) {
        const long long s = Tl.s0 + base + lane;
        int tl;
        const int what = sc_site_label(J, base + lane < Tl.n, s, S.kind, S.kind_ok, S.x_of_site, S.units, S.stride, T, &tl);
        // (a site with a non-zero total has a record of its x: the second condition is never false)
        const bool lab = what == SC_SITE_LABELLED && ymax[s] >= 0;
        bool correct = false, outside = false;
        sa_callq_call_t c;
        if (lab) {
            const int x = S.x_of_site[s];
            const double p = S.prob[(size_t) s * (size_t) S.stride + (size_t) tl];
            const int y0 = ymin[s], y1 = ymax[s];
            const long long b_start = rs[y0], b_length = (long long) rs[y1] - b_start + rl[y1];
            const int g = cq_guide_row(jx, Q.n_anchors, x, J.x_sign);
            long long delta2 = 0;
            int guide_event = -1;
            correct = p > threshold;
            outside = g < 0;
            if (!outside) {
                guide_event = jy[g];
                delta2 = 2 * b_start + b_length - 2 * cq_round_mid(rs[guide_event], rl[guide_event]);
            }
            if (WRITE) {
                c.raw_start = b_start; c.raw_length = b_length; c.delta2 = delta2; c.prob_true = p;
                c.x = x; c.guide_event = guide_event; c.true_letter = tl; c.correct = correct; c.outside = outside; c.pad = 0;
            }
            if (!WRITE && !outside) {
                const unsigned long long ab = (unsigned long long) (delta2 < 0 ? -delta2 : delta2);
                const unsigned long long key = (ab << 28) | (CQ_X_MASK - (unsigned long long) x);
                sum_abs += ab;
                max_key = key > max_key ? key : max_key;
                int slot = 0;
                if (delta2 >= G.lo2) {
                    const long long b = (delta2 - G.lo2) / G.w2;   // (not negative: a floor)
                    slot = b >= (long long) G.n_bins ? G.n_bins + 1 : (int) b + 1;
                }
                atomicAdd(&s_hist[slot * 2 + (correct ? 1 : 0)], 1);
            }
        }
        const unsigned long long mask = __ballot(lab);
        if (WRITE && lab) calls[w + __popcll(mask & ((1ull << lane) - 1ull))] = c;
        if (!WRITE) {
            n_calls += (unsigned long long) __popcll(mask);
            n_correct += (unsigned long long) __popcll(__ballot(correct));
            n_out += (unsigned long long) __popcll(__ballot(outside));
            n_unl += (unsigned long long) __popcll(__ballot(what == SC_SITE_UNLABELLED));
            n_oth += (unsigned long long) __popcll(__ballot(what == SC_SITE_OTHER));
        }
        w += __popcll(mask);
    }
    if (WRITE) return;
    __syncthreads();
    for (int q = lane; q < n_slots; q += 64) {
        const int v = s_hist[q];
        if (v == 0) continue;
        if (hist) atomicAdd(&hist[(size_t) Tl.job * (size_t) n_slots + (size_t) q], (unsigned long long) v);
        atomicAdd(&total_hist[q], (unsigned long long) v);
    }
    sum_abs = cq_wave_sum(sum_abs);
    max_key = cq_wave_max(max_key);
    if (lane == 0) {
        CqAcc *A = &acc[Tl.job];
        if (n_calls) atomicAdd(&A->n_calls, n_calls);
        if (n_correct) atomicAdd(&A->n_correct, n_correct);
        if (n_unl) atomicAdd(&A->n_unlabelled, n_unl);
        if (n_oth) atomicAdd(&A->n_other, n_oth);
        if (n_out) atomicAdd(&A->n_outside, n_out);
        if (sum_abs) atomicAdd(&A->sum_abs, sum_abs);
        if (max_key) atomicMax(&A->max_key, max_key);
        tile_cnt[blockIdx.x] = (long long) n_calls;
    }
}

template <bool WRITE>
__global__ __launch_bounds__(64) void k_cq_gaps(const CqJob *__restrict__ jobs, const int *__restrict__ path_y,
                                                const int *__restrict__ raw_start, const int *__restrict__ raw_length,
                                                int min_gap, CqGapAcc *__restrict__ gacc, const long long *__restrict__ gap_off,
                                                sa_callq_gap_t *__restrict__ gaps) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const CqJob Q = jobs[j];
    const int *py = path_y + Q.path_first;
    const int *rs = raw_start + Q.ev_first, *rl = raw_length + Q.ev_first;
    long long carry_end = 0, n_gaps = 0, sum_gap = 0, max_gap = 0;   // sum and max the lane's own
    int carry_y = 0;
    long long w = WRITE ? gap_off[j] : 0;
    for (int p0 = 0; p0 < Q.n_path; p0 += 64) {
        const int p = p0 + lane;
        const bool in = p < Q.n_path;
        const int y = in ? py[p] : 0;
        const long long start = in ? rs[y] : 0, end = in ? start + rl[y] : 0;
        long long prev_end = __shfl_up(end, 1);
        int prev_y = __shfl_up(y, 1);
        if (lane == 0) { prev_end = carry_end; prev_y = carry_y; }
        const long long gap = start - prev_end;
        const bool is_gap = in && p > 0 && gap > (long long) min_gap;
        const unsigned long long mask = __ballot(is_gap);
        if (is_gap) {
            if (WRITE) {
                sa_callq_gap_t g;
                g.y_before = prev_y; g.y_after = y; g.gap = gap;
                gaps[w + __popcll(mask & ((1ull << lane) - 1ull))] = g;
            } else {
                sum_gap += gap;
                max_gap = gap > max_gap ? gap : max_gap;
            }
        }
        w += __popcll(mask);
        n_gaps += __popcll(mask);
        carry_end = __shfl(end, 63);
        carry_y = __shfl(y, 63);
    }
    if (WRITE) return;
    sum_gap = (long long) cq_wave_sum((unsigned long long) sum_gap);
    max_gap = (long long) cq_wave_max((unsigned long long) max_gap);
    if (lane == 0) {
        CqGapAcc g;
        g.n_gaps = n_gaps; g.sum_gap = sum_gap; g.max_gap = max_gap; g.pad = 0;
        gacc[j] = g;
    }
}

// every tile's first call and every job's first gap (off[n] the totals), then the jobs' results
__global__ __launch_bounds__(SA_SCAN_THREADS) void k_cq_finish(const CqJob *__restrict__ jobs, int nj, const long long *__restrict__ tile_cnt,
                                                               int n_tiles, long long *__restrict__ tile_off,
                                                               const CqAcc *__restrict__ acc, const CqGapAcc *__restrict__ gacc,
                                                               long long *__restrict__ gap_off, int want_calls,
                                                               sa_callq_read_t *__restrict__ reads) {
    sa_block_excl_scan([tile_cnt](int i) { return tile_cnt[i]; }, tile_off, n_tiles);
    __syncthreads();
    sa_block_excl_scan([gacc](int i) { return gacc[i].n_gaps; }, gap_off, nj);
    __syncthreads();
    for (int j = threadIdx.x; j < nj; j += SA_SCAN_THREADS) {
        const CqJob Q = jobs[j];
        const CqAcc A = acc[j];
        const CqGapAcc g = gacc[j];
        sa_callq_read_t r;
        r.status = (Q.n_anchors == 0 ? SA_CQ_NO_GUIDE : 0) | (A.n_calls + A.n_unlabelled + A.n_other == 0 ? SA_CQ_NO_SITES : 0) |
                   (Q.n_path == 0 ? SA_CQ_NO_PATH : 0);
        r.max_x = A.n_calls > A.n_outside ? (int) (CQ_X_MASK - (A.max_key & CQ_X_MASK)) : -1;
        r.n_calls = (long long) A.n_calls; r.n_correct = (long long) A.n_correct; r.n_unlabelled = (long long) A.n_unlabelled;
        r.n_other_sites = (long long) A.n_other; r.n_outside = (long long) A.n_outside; r.sum_abs_delta2 = (long long) A.sum_abs;
        r.max_abs_delta2 = (long long) (A.max_key >> 28);
        r.n_path = Q.n_path; r.n_gaps = g.n_gaps; r.sum_gap = g.sum_gap; r.max_gap = g.max_gap;
        r.call_first = want_calls ? tile_off[Q.tile_first] : 0;
        r.gap_first = gap_off[j];
        reads[j] = r;
    }
}

static const sa_callq_params_t CQ_DEFAULT = {-10000, 100, 200, 30};

// what both calls check of their arguments, and what goes up: the jobs, the anchors, the raw starts and lengths, the paths' events
struct CqInput {
    std::vector<ScJob> sjobs;
    std::vector<CqJob> jobs;
    std::vector<int> ax, ay, path_y;
    std::vector<int> raw;         // all raw_start, then all raw_length (a raw read ends below 2^31 samples)
    long long n_slots = 0;
};
static int cq_check(const sa_call_scores *s, const sa_score_job_map_t *map, const sa_callq_job_t *jobs, int64_t n_jobs,
                    const sa_mea_pair_t *const *mea_path, const int64_t *n_mea, const sa_callq_params_t *p, unsigned flags,
                    sa_callq_read_t *reads_out, sa_callq_call_t **calls_out, int64_t *n_calls_out, sa_callq_gap_t **gaps_out,
                    int64_t *n_gaps_out, CqInput *in) {
    if (n_jobs < 0 || (n_jobs > 0 && (!jobs || !map || !reads_out)) || !gaps_out || !n_gaps_out || (flags & ~(SA_CQ_CALLS | SA_CQ_BAND_DIRECT)))
        return SA_EINVAL;
    if ((flags & SA_CQ_CALLS) && (!calls_out || !n_calls_out)) return SA_EINVAL;
    if ((mea_path == nullptr) != (n_mea == nullptr)) return SA_EINVAL;
    if (p->bin_width < 1 || p->bin_width > CQ_MAX_GRID || p->bin_lo < -CQ_MAX_GRID || p->bin_lo > CQ_MAX_GRID || p->n_bins < 1 ||
        p->n_bins > SA_CQ_MAX_BINS || p->min_gap < 0)
        return SA_EINVAL;
    if (n_jobs > (int64_t) INT32_MAX) return SA_EUNSUPPORTED;
    in->sjobs.resize((size_t) n_jobs);
    in->jobs.resize((size_t) n_jobs);
    long long n_slots = 0, n_anc = 0, n_path = 0;
    bool too_long = false;
    for (int64_t j = 0; j < n_jobs; j++) {
        const sa_callq_job_t &q = jobs[j];
        if (!sc_job_from_map(map[j], s->nl, &in->sjobs[(size_t) j])) return SA_EINVAL;
        if (q.n_events < 0 || q.n_events > CQ_MAX_COORD || q.n_anchors < 0 || q.n_anchors > (int64_t) INT32_MAX) return SA_EINVAL;
        if ((q.n_anchors > 0 && (!q.anchor_x || !q.anchor_y)) || (q.n_events > 0 && (!q.raw_start || !q.raw_length))) return SA_EINVAL;
        if (mea_path && (n_mea[j] < 0 || (n_mea[j] > 0 && !mea_path[j]))) return SA_EINVAL;
        if (mea_path && n_mea[j] > (int64_t) INT32_MAX) return SA_EUNSUPPORTED;
        for (int64_t y = 0; y < q.n_events; y++) {
            if (q.raw_start[y] < 0 || q.raw_length[y] < 1 || (y > 0 && q.raw_start[y] <= q.raw_start[y - 1])) return SA_EINVAL;
            if (q.raw_start[y] > (int64_t) INT32_MAX || q.raw_length[y] > (int64_t) INT32_MAX - q.raw_start[y]) too_long = true;
        }
        CqJob &J = in->jobs[(size_t) j];
        memset(&J, 0, sizeof(J));
        J.ev_first = n_slots; J.anc_first = n_anc; J.path_first = n_path;
        J.n_events = (int) q.n_events; J.n_anchors = (int) q.n_anchors; J.n_path = mea_path ? (int) n_mea[j] : 0;
        n_slots += q.n_events;
        n_anc += q.n_anchors;
        n_path += J.n_path;
    }
    in->n_slots = n_slots;
    const bool unsupported = too_long || n_slots > (long long) INT32_MAX || n_path > (long long) INT32_MAX;
    in->ax.resize((size_t) n_anc); in->ay.resize((size_t) n_anc); in->path_y.resize((size_t) n_path);
    in->raw.resize(unsupported ? 0 : (size_t) (2 * n_slots));
    size_t ia = 0, ip = 0;
    for (int64_t j = 0; j < n_jobs; j++) {
        const sa_callq_job_t &q = jobs[j];
        const CqJob &J = in->jobs[(size_t) j];
        for (int64_t y = 0; y < q.n_events && !unsupported; y++) {
            in->raw[(size_t) (J.ev_first + y)] = (int) q.raw_start[y];
            in->raw[(size_t) (n_slots + J.ev_first + y)] = (int) q.raw_length[y];
        }
        for (int64_t i = 0; i < q.n_anchors; i++, ia++) {
            const int64_t x = q.anchor_x[i], y = q.anchor_y[i];
            if (x < 0 || x >= CQ_MAX_COORD || y < 0 || y >= q.n_events) return SA_EINVAL;
            if (i > 0 && (y <= q.anchor_y[i - 1] || x < q.anchor_x[i - 1])) return SA_EINVAL;
            in->ax[ia] = (int) x; in->ay[ia] = (int) y;
        }
        for (int64_t i = 0; i < J.n_path; i++, ip++) {
            const int64_t e = mea_path[j][i].event_idx;
            if (e < 0 || e >= q.n_events || (i > 0 && e <= mea_path[j][i - 1].event_idx)) return SA_EINVAL;
            in->path_y[ip] = (int) e;
        }
    }
    return unsupported ? SA_EUNSUPPORTED : SA_OK;   // (after every SA_EINVAL)
}

static inline float cq_ev_ms(int k, const bool *ran) {
    float ms = 0;
    if (ran[k]) (void) hipEventElapsedTime(&ms, g_cq_ev[2 * k], g_cq_ev[2 * k + 1]);
    return ms;
}

// The sites S and the records `recs` lie on W's device (job j's records are V.first[j] .. + V.count[j], its sites
// h_site_off[j] .. h_site_off[j + 1]); the caller holds W.mu and s's lock and has bound W to the device.  The timed regions begin
// after the uploads: *kernel_ms_out gets the kernels' time.
static int cq_run(SaScratch &W, const sa_call_scores *s, const sa_pair16_t *recs, const SaBatchView &V,
                  const CqSites &S, const long long *h_site_off, CqInput &in, const sa_callq_params_t &P, unsigned flags,
                  sa_callq_read_t *reads_out, sa_callq_call_t **calls_out, int64_t *n_calls_out, sa_callq_gap_t **gaps_out,
                  int64_t *n_gaps_out, int64_t *hist_out, int64_t *total_hist_out, double *kernel_ms_out) {
    const bool want_calls = flags & SA_CQ_CALLS;
    const size_t nj = in.jobs.size(), ns = (size_t) h_site_off[nj], nev = (size_t) in.n_slots, na = in.ax.size(), np = in.path_y.size();
    const size_t n_slots = ((size_t) P.n_bins + 2) * 2;
    *gaps_out = nullptr;
    *n_gaps_out = 0;
    if (want_calls) { *calls_out = nullptr; *n_calls_out = 0; }
    for (double &v : g_cq_last_ms) v = 0.0;
    if (nj == 0) {
        for (size_t q = 0; total_hist_out && q < n_slots; q++) total_hist_out[q] = 0;
        *gaps_out = (sa_callq_gap_t *) malloc(sizeof(sa_callq_gap_t));
        if (want_calls) *calls_out = (sa_callq_call_t *) malloc(sizeof(sa_callq_call_t));
        if (!*gaps_out || (want_calls && !*calls_out)) {
            free(*gaps_out);
            *gaps_out = nullptr;
            if (want_calls) { free(*calls_out); *calls_out = nullptr; }
            return SA_ENOMEM;
        }
        return SA_OK;
    }
    std::vector<CqTile> tiles;
    for (size_t j = 0; j < nj; j++) {
        in.jobs[j].tile_first = (int) tiles.size();
        for (long long s0 = h_site_off[j]; s0 < h_site_off[j + 1]; s0 += CQ_TILE)
            tiles.push_back(CqTile{s0, (int) std::min<long long>(CQ_TILE, h_site_off[j + 1] - s0), (int) j});
    }
    const std::vector<SaRecChunk> chunks = ns ? sa_view_chunks(V, SA_CHAIN_CHUNK, SA_ORDINAL_PER_JOB) : std::vector<SaRecChunk>();
    const size_t nt = tiles.size(), nc = chunks.size();
    if (nc > (size_t) INT32_MAX) return SA_EUNSUPPORTED;
    int rc = SA_OK;
    // [site jobs | jobs | tiles | chunks | anchor_x | anchor_y | raw starts, lengths | paths' events | y_min | y_max |
    //  accumulators, gap accumulators, tile counts, total hist | hist | tile offsets | gap offsets | reads]
    SaLayout L;
    const size_t o_sjobs = L.add(sizeof(ScJob) * nj), o_jobs = L.add(sizeof(CqJob) * nj), o_tiles = L.add(sizeof(CqTile) * nt),
                 o_ch = L.add(sizeof(SaRecChunk) * nc), o_ax = L.add(4 * na), o_ay = L.add(4 * na), o_raw = L.add(4 * 2 * nev),
                 o_path = L.add(4 * np), o_ymin = L.add(4 * ns), o_ymax = L.add(4 * ns);
    const size_t zero_bytes = sizeof(CqAcc) * nj + sizeof(CqGapAcc) * nj + 8 * nt + 8 * n_slots;   // one memset spans them
    const size_t o_acc = L.add(zero_bytes), o_gacc = o_acc + sizeof(CqAcc) * nj, o_tcnt = o_gacc + sizeof(CqGapAcc) * nj,
                 o_thist = o_tcnt + 8 * nt;
    const size_t o_hist = L.add(hist_out ? 8 * nj * n_slots : 0), o_toff = L.add(8 * (nt + 1)), o_goff = L.add(8 * (nj + 1)),
                 o_reads = L.add(sizeof(sa_callq_read_t) * nj);
    float ms0 = 0, ms1 = 0;
    long long n_calls = 0, n_gaps = 0;
    sa_callq_call_t *h_calls = nullptr;
    sa_callq_gap_t *h_gaps = nullptr;
    bool ran[CQ_EV_N] = {};
    if ((rc = W.dev(CQ_WS, L.end)) != SA_OK) return rc;
    {
        if (!g_cq_ev_made) {
            for (hipEvent_t &e : g_cq_ev) SA_HIP_GOTO_DONE(hipEventCreate(&e));
            g_cq_ev_made = true;
        }
        auto begin = [&](int k) { (void) hipEventRecord(g_cq_ev[2 * k], 0); ran[k] = true; };
        auto end = [&](int k) { (void) hipEventRecord(g_cq_ev[2 * k + 1], 0); };
        char *d = (char *) W.at(CQ_WS);
        const ScJob *d_sjobs = (const ScJob *) (d + o_sjobs);
        const CqJob *d_jobs = (const CqJob *) (d + o_jobs);
        const CqTile *d_tiles = (const CqTile *) (d + o_tiles);
        const int *d_ax = (const int *) (d + o_ax), *d_ay = (const int *) (d + o_ay), *d_path = (const int *) (d + o_path);
        const int *d_rs = (const int *) (d + o_raw), *d_rl = d_rs + nev;
        int *d_ymin = (int *) (d + o_ymin), *d_ymax = (int *) (d + o_ymax);
        CqAcc *d_acc = (CqAcc *) (d + o_acc);
        CqGapAcc *d_gacc = (CqGapAcc *) (d + o_gacc);
        long long *d_tcnt = (long long *) (d + o_tcnt), *d_toff = (long long *) (d + o_toff), *d_goff = (long long *) (d + o_goff);
        unsigned long long *d_hist = hist_out ? (unsigned long long *) (d + o_hist) : nullptr, *d_thist = (unsigned long long *) (d + o_thist);
        sa_callq_read_t *d_reads = (sa_callq_read_t *) (d + o_reads);
        ScTruth T;
        T.tkey = (const unsigned long long *) s->d_truth;
        T.tlet = (const signed char *) (s->d_truth + s->o_tlet);
        T.n_truth = s->n_truth;
        CqGrid G;
        G.lo2 = 2 * P.bin_lo; G.w2 = 2 * P.bin_width; G.n_bins = P.n_bins; G.min_gap = P.min_gap;
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_sjobs, in.sjobs.data(), sizeof(ScJob) * nj, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_jobs, in.jobs.data(), sizeof(CqJob) * nj, hipMemcpyHostToDevice, 0));
        if (nt) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_tiles, tiles.data(), sizeof(CqTile) * nt, hipMemcpyHostToDevice, 0));
        if (nc) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_ch, chunks.data(), sizeof(SaRecChunk) * nc, hipMemcpyHostToDevice, 0));
        if (na) {
            SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_ax, in.ax.data(), 4 * na, hipMemcpyHostToDevice, 0));
            SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_ay, in.ay.data(), 4 * na, hipMemcpyHostToDevice, 0));
        }
        if (nev) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_raw, in.raw.data(), 4 * 2 * nev, hipMemcpyHostToDevice, 0));
        if (np) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_path, in.path_y.data(), 4 * np, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(W.time_begin());
        SA_HIP_GOTO_DONE(hipMemsetAsync(d + o_acc, 0, zero_bytes, 0));
        if (hist_out) SA_HIP_GOTO_DONE(hipMemsetAsync(d + o_hist, 0, 8 * nj * n_slots, 0));
        if (ns) {
            SA_HIP_GOTO_DONE(hipMemsetAsync(d_ymin, 0x7f, 4 * ns, 0));   // smallest y: above every event
            SA_HIP_GOTO_DONE(hipMemsetAsync(d_ymax, 0xff, 4 * ns, 0));   // largest y: -1, no record
        }
        if (nc) {
            begin(CQ_EV_BAND);
            if (!(flags & SA_CQ_BAND_DIRECT))
                hipLaunchKernelGGL(k_cq_band<true>, dim3((unsigned) nc), dim3(CQ_THREADS), 0, 0, recs, (const SaRecChunk *) (d + o_ch), d_jobs,
                                   S.site_off, S.x_of_site, d_ymin, d_ymax);
            else
                hipLaunchKernelGGL(k_cq_band<false>, dim3((unsigned) nc), dim3(CQ_THREADS), 0, 0, recs, (const SaRecChunk *) (d + o_ch), d_jobs,
                                   S.site_off, S.x_of_site, d_ymin, d_ymax);
            end(CQ_EV_BAND);
        }
        if (nt) {
            begin(CQ_EV_CALLS);
            hipLaunchKernelGGL(k_cq_calls<false>, dim3((unsigned) nt), dim3(64), 0, 0, d_tiles, d_sjobs, d_jobs, S, T, s->threshold,
                               (const int *) d_ymin, (const int *) d_ymax, d_ax, d_ay, d_rs, d_rl, G, d_acc, d_hist, d_thist, d_tcnt,
                               (const long long *) nullptr, (sa_callq_call_t *) nullptr);
            end(CQ_EV_CALLS);
        }
        begin(CQ_EV_GAPS);
        hipLaunchKernelGGL(k_cq_gaps<false>, dim3((unsigned) nj), dim3(64), 0, 0, d_jobs, d_path, d_rs, d_rl, (int) P.min_gap, d_gacc,
                           (const long long *) nullptr, (sa_callq_gap_t *) nullptr);
        hipLaunchKernelGGL(k_cq_finish, dim3(1), dim3(SA_SCAN_THREADS), 0, 0, d_jobs, (int) nj, (const long long *) d_tcnt, (int) nt, d_toff,
                           (const CqAcc *) d_acc, (const CqGapAcc *) d_gacc, d_goff, want_calls ? 1 : 0, d_reads);
        end(CQ_EV_GAPS);
        SA_HIP_GOTO_DONE(W.time_end());
        // the one readback of the counts
        SA_HIP_GOTO_DONE(hipMemcpy(&n_calls, d + o_toff + 8 * nt, 8, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(hipMemcpy(&n_gaps, d + o_goff + 8 * nj, 8, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(W.time_ms(&ms0));
        if (!want_calls) n_calls = 0;
        h_gaps = (sa_callq_gap_t *) malloc(sizeof(sa_callq_gap_t) * (size_t) (n_gaps > 0 ? n_gaps : 1));
        if (want_calls) h_calls = (sa_callq_call_t *) malloc(sizeof(sa_callq_call_t) * (size_t) (n_calls > 0 ? n_calls : 1));
        if (!h_gaps || (want_calls && !h_calls)) { rc = SA_ENOMEM; goto done; }
        if (n_calls > 0 || n_gaps > 0) {
            if (n_calls > 0 && (rc = W.dev(CQ_CALLS, sizeof(sa_callq_call_t) * (size_t) n_calls)) != SA_OK) goto done;
            if (n_gaps > 0 && (rc = W.dev(CQ_GAPS, sizeof(sa_callq_gap_t) * (size_t) n_gaps)) != SA_OK) goto done;
            SA_HIP_GOTO_DONE(W.time_begin());
            if (n_calls > 0) {
                begin(CQ_EV_CALLS_W);
                hipLaunchKernelGGL(k_cq_calls<true>, dim3((unsigned) nt), dim3(64), 0, 0, d_tiles, d_sjobs, d_jobs, S, T, s->threshold,
                                   (const int *) d_ymin, (const int *) d_ymax, d_ax, d_ay, d_rs, d_rl, G, (CqAcc *) nullptr,
                                   (unsigned long long *) nullptr, (unsigned long long *) nullptr, (long long *) nullptr,
                                   (const long long *) d_toff, (sa_callq_call_t *) W.at(CQ_CALLS));
                end(CQ_EV_CALLS_W);
            }
            if (n_gaps > 0) {
                begin(CQ_EV_GAPS_W);
                hipLaunchKernelGGL(k_cq_gaps<true>, dim3((unsigned) nj), dim3(64), 0, 0, d_jobs, d_path, d_rs, d_rl, (int) P.min_gap,
                                   (CqGapAcc *) nullptr, (const long long *) d_goff, (sa_callq_gap_t *) W.at(CQ_GAPS));
                end(CQ_EV_GAPS_W);
            }
            SA_HIP_GOTO_DONE(W.time_end());
            if (n_calls > 0)
                SA_HIP_GOTO_DONE(hipMemcpy(h_calls, W.at(CQ_CALLS), sizeof(sa_callq_call_t) * (size_t) n_calls, hipMemcpyDeviceToHost));
            if (n_gaps > 0) SA_HIP_GOTO_DONE(hipMemcpy(h_gaps, W.at(CQ_GAPS), sizeof(sa_callq_gap_t) * (size_t) n_gaps, hipMemcpyDeviceToHost));
            SA_HIP_GOTO_DONE(W.time_ms(&ms1));
        }
        SA_HIP_GOTO_DONE(hipMemcpy(reads_out, d_reads, sizeof(sa_callq_read_t) * nj, hipMemcpyDeviceToHost));
        if (hist_out) SA_HIP_GOTO_DONE(hipMemcpy(hist_out, d + o_hist, 8 * nj * n_slots, hipMemcpyDeviceToHost));
        if (total_hist_out) SA_HIP_GOTO_DONE(hipMemcpy(total_hist_out, d + o_thist, 8 * n_slots, hipMemcpyDeviceToHost));
        g_cq_last_ms[0] = (double) cq_ev_ms(CQ_EV_BAND, ran);
        g_cq_last_ms[1] = (double) cq_ev_ms(CQ_EV_CALLS, ran) + (double) cq_ev_ms(CQ_EV_CALLS_W, ran);
        g_cq_last_ms[2] = (double) cq_ev_ms(CQ_EV_GAPS, ran) + (double) cq_ev_ms(CQ_EV_GAPS_W, ran);
    }
    if (kernel_ms_out) *kernel_ms_out = (double) ms0 + (double) ms1;
    *gaps_out = h_gaps;
    *n_gaps_out = n_gaps;
    if (want_calls) { *calls_out = h_calls; *n_calls_out = n_calls; }
    return SA_OK;
done:
    (void) hipStreamSynchronize(0);
    free(h_calls);
    free(h_gaps);
    return rc;
}

extern "C" int sa_batch_call_quality(sa_call_scores_t *s, sa_batch_t *b, const sa_score_job_map_t *map, const sa_callq_job_t *jobs,
                                     int64_t n_jobs, const sa_mea_pair_t *const *mea_path, const int64_t *n_mea, const sa_callq_params_t *p,
                                     unsigned flags, sa_callq_read_t *reads_out, sa_callq_call_t **calls_out, int64_t *n_calls_out,
                                     sa_callq_gap_t **gaps_out, int64_t *n_gaps_out, int64_t *hist_out, int64_t *total_hist_out,
                                     double *kernel_ms_out) {
    if (!s || !b) return SA_EINVAL;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    const sa_callq_params_t P = p ? *p : CQ_DEFAULT;
    CqInput in;
    int rc = cq_check(s, map, jobs, n_jobs, mea_path, n_mea, &P, flags, reads_out, calls_out, n_calls_out, gaps_out, n_gaps_out, &in);
    if (rc) return rc;
    // what the batch says of itself, before anything runs: its state, its jobs, their events, its device
    SaAmbigTab *tab = nullptr;
    int64_t nj64 = 0;
    if ((rc = sa_batch_ambig(b, SA_TAB_SITES, &tab, &nj64)) != SA_OK) return rc;
    if (nj64 != n_jobs) return SA_EINVAL;
    ScEnter enter(s);
    if (enter.rc) return enter.rc;
    SaScratch &W = g_cq_ws;
    std::lock_guard<std::mutex> guard(W.mu);
    SaBatchView V;
    if ((rc = sa_batch_view(b, &V)) != SA_OK) return rc;
    if (V.device != s->device) return SA_EINVAL;
    for (int64_t j = 0; j < n_jobs; j++)
        if (V.n_events[(size_t) j] != jobs[j].n_events) return SA_EINVAL;
    SaSiteFold F;
    char *d = nullptr;
    rc = sa_site_fold_run(b, &F);
    if (rc == SA_OK && (rc = W.rebind(s->device)) == SA_OK) {
        const size_t ns = F.ns;
        std::vector<unsigned char> kind_ok(F.letters.size() + 1, 0);
        for (size_t kd = 0; kd < F.letters.size(); kd++) kind_ok[kd] = F.letters[kd] == std::string(s->letters);
        SaLayout L;   // [kind ok | x of site]
        const size_t o_ok = L.add(kind_ok.size()), o_x = L.add(4 * ns);
        CqSites S;
        memset(&S, 0, sizeof(S));
        if ((rc = W.dev(CQ_SITES, L.end)) != SA_OK) goto done;
        d = (char *) W.at(CQ_SITES);
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_ok, kind_ok.data(), kind_ok.size(), hipMemcpyHostToDevice, 0));
        if (ns) SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_x, F.h_x, 4 * ns, hipMemcpyHostToDevice, 0));
        S.site_off = F.site_off; S.kind = F.kind; S.kind_ok = (const unsigned char *) (d + o_ok); S.x_of_site = (const int *) (d + o_x);
        S.units = F.units; S.prob = F.prob; S.stride = (int) F.stride;
        if (ns) SA_HIP_GOTO_DONE(F.ws->time_end());   // the fold's own region ends with its kernels: the uploads below are not in it
        rc = cq_run(W, s, (const sa_pair16_t *) V.recs, V, S, F.h_site_off, in, P, flags, reads_out, calls_out,
                    n_calls_out, gaps_out, n_gaps_out, hist_out, total_hist_out, kernel_ms_out);
        if (rc == SA_OK && ns && kernel_ms_out) {   // (cq_run's copies have synchronised the stream)
            float fold_ms = 0;
            SA_HIP_GOTO_DONE(F.ws->time_ms(&fold_ms));
            *kernel_ms_out += (double) fold_ms;
        }
    }
done:
    sa_site_fold_release(&F, rc != SA_OK);
    return rc;
}

extern "C" int sa_call_quality_records(sa_call_scores_t *s, const sa_score_job_map_t *map, const sa_callq_job_t *jobs, int64_t n_jobs,
                                       const int64_t *site_first, const int32_t *site_x, const double *site_prob, const uint8_t *site_other,
                                       const int64_t *rec_first, const int32_t *rec_x, const int32_t *rec_y,
                                       const sa_mea_pair_t *const *mea_path, const int64_t *n_mea, const sa_callq_params_t *p, unsigned flags,
                                       sa_callq_read_t *reads_out, sa_callq_call_t **calls_out, int64_t *n_calls_out,
                                       sa_callq_gap_t **gaps_out, int64_t *n_gaps_out, int64_t *hist_out, int64_t *total_hist_out,
                                       double *kernel_ms_out) {
    if (!s) return SA_EINVAL;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    const sa_callq_params_t P = p ? *p : CQ_DEFAULT;
    CqInput in;
    int rc = cq_check(s, map, jobs, n_jobs, mea_path, n_mea, &P, flags, reads_out, calls_out, n_calls_out, gaps_out, n_gaps_out, &in);
    if (rc) return rc;
    if (!site_first || !rec_first || site_first[0] != 0 || rec_first[0] != 0) return SA_EINVAL;
    for (int64_t j = 0; j < n_jobs; j++)
        if (site_first[j + 1] < site_first[j] || rec_first[j + 1] < rec_first[j]) return SA_EINVAL;
    if (site_first[n_jobs] > (int64_t) INT32_MAX || rec_first[n_jobs] > (int64_t) INT32_MAX) return SA_EUNSUPPORTED;
    const size_t ns = (size_t) site_first[n_jobs], nr = (size_t) rec_first[n_jobs], nl = (size_t) s->nl;
    if ((ns > 0 && (!site_x || !site_prob)) || (nr > 0 && (!rec_x || !rec_y))) return SA_EINVAL;
    std::vector<sa_pair16_t> recs(nr);
    std::vector<unsigned char> kind(ns, 0), seen(ns, 0);
    std::vector<unsigned long long> units(ns * nl, 0ull);
    for (int64_t j = 0; j < n_jobs; j++) {
        const int64_t a = site_first[j], e = site_first[j + 1];
        for (int64_t i = a; i < e; i++) {
            if (site_x[i] < 0 || site_x[i] >= CQ_MAX_COORD || (i > a && site_x[i] <= site_x[i - 1])) return SA_EINVAL;
            for (size_t l = 0; l < nl; l++) {
                const double v = site_prob[(size_t) i * nl + l];
                if (!(v >= 0.0 && v <= 1.0)) return SA_EINVAL;   // (a NaN compares false)
            }
            kind[(size_t) i] = site_other && site_other[i] ? 1 : 0;
            units[(size_t) i * nl] = 1;   // every site handed in is one with a non-zero total
        }
        for (int64_t i = rec_first[j]; i < rec_first[j + 1]; i++) {
            if (rec_x[i] < 0 || rec_x[i] >= CQ_MAX_COORD || rec_y[i] < 0 || rec_y[i] >= jobs[j].n_events) return SA_EINVAL;
            recs[(size_t) i] = sa_pair16_pack(0, rec_x[i], rec_y[i], 0, 0);
            const int32_t *at = std::lower_bound(site_x + a, site_x + e, rec_x[i]);
            if (at != site_x + e && *at == rec_x[i]) seen[(size_t) (at - site_x)] = 1;
        }
    }
    for (size_t i = 0; i < ns; i++)
        if (!seen[i]) return SA_EINVAL;   // a site with no record of its x
    ScEnter enter(s);
    if (enter.rc) return enter.rc;
    SaBatchView V;
    V.first.assign(rec_first, rec_first + n_jobs);
    V.count.resize((size_t) n_jobs);
    for (int64_t j = 0; j < n_jobs; j++) V.count[(size_t) j] = rec_first[j + 1] - rec_first[j];
    const std::vector<long long> h_site_off(site_first, site_first + n_jobs + 1);
    const unsigned char kind_ok[2] = {1, 0};
    SaScratch &W = g_cq_ws;
    std::lock_guard<std::mutex> guard(W.mu);
    SaLayout L;   // [site offsets | x of site | kind | kind ok | units | prob]
    const size_t o_off = L.add(8 * ((size_t) n_jobs + 1)), o_x = L.add(4 * ns), o_kind = L.add(ns), o_ok = L.add(2), o_units = L.add(8 * ns * nl),
                 o_prob = L.add(8 * ns * nl);
    if ((rc = W.rebind(s->device)) != SA_OK || (rc = W.dev(CQ_SITES, L.end)) != SA_OK ||
        (rc = W.dev(CQ_RECS, sizeof(sa_pair16_t) * (nr ? nr : 1))) != SA_OK)
        return rc;
    char *d = (char *) W.at(CQ_SITES);
    const struct { size_t off; const void *src; size_t n; } up[] = {
        {o_off, h_site_off.data(), 8 * ((size_t) n_jobs + 1)}, {o_x, site_x, 4 * ns}, {o_kind, kind.data(), ns}, {o_ok, kind_ok, 2},
        {o_units, units.data(), 8 * ns * nl}, {o_prob, site_prob, 8 * ns * nl}};
    for (const auto &u : up)
        if (u.n && hipMemcpy(d + u.off, u.src, u.n, hipMemcpyHostToDevice) != hipSuccess) return SA_ENODEVICE;
    if (nr && hipMemcpy(W.at(CQ_RECS), recs.data(), sizeof(sa_pair16_t) * nr, hipMemcpyHostToDevice) != hipSuccess) return SA_ENODEVICE;
    CqSites S;
    S.site_off = (const long long *) (d + o_off); S.kind = (const unsigned char *) (d + o_kind);
    S.kind_ok = (const unsigned char *) (d + o_ok); S.x_of_site = (const int *) (d + o_x);
    S.units = (const unsigned long long *) (d + o_units); S.prob = (const double *) (d + o_prob); S.stride = (int) nl;
    return cq_run(W, s, (const sa_pair16_t *) W.at(CQ_RECS), V, S, h_site_off.data(), in, P, flags, reads_out, calls_out, n_calls_out,
                  gaps_out, n_gaps_out, hist_out, total_hist_out, kernel_ms_out);
}
