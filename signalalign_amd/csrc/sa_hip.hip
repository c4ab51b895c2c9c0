// sa_hip.hip -- gfx950 kernels and the batch runtime behind include/signalalign_hip.h.
//
// Device work per batch (all inputs resident in HBM before the first launch):
//   1. forward sweep      one wavefront per split region, anti-diagonal after anti-diagonal
//   2. backward sweep     one wavefront per traceback segment (independent of each other), fused with the
//                         posterior numerator f.match+b.match and the per-cell terms of totalProbability
//   3. fold               one lane per checkpoint: the reference's strictly sequential logAdd fold of the
//                         per-cell terms (kept sequential on purpose: logAdd is a piecewise cubic, not associative)
//   4. finalize/scan/gather   posterior = exp(fb - total), threshold, floor(p*1e7), compaction into the
//                         reference's output order
//
// One translation unit; the kernel families share the data layout decisions but not the code.  In this order:
//   here                 the device-side views (DevModel, DevPlan, ReadPar, the wave reductions)
//   sa_fast.inc          fast (k_*_fast): one path per cell, Gaussian emissions, the two previous anti-diagonals in registers
//   sa_ring.inc, sa_strip.inc   the ring and strip kernels
//   sa_generic.inc       generic (k_*_generic): any band width, any number of paths per cell, HDP emissions, reference-ordered
//                        un-contracted arithmetic.  State lives in memory.  This is the exactness baseline.
//   sa_result.inc        fold, finalize, scan, gather, k_fill_xc
//   sa_runtime.inc       the process-wide host runtime: HIPCHK / TRY, handles, uploaders, allocators, memos
//   here                 the launch classes, a batch's streams and events (sa_lanes, sa_*_events), sa_batch, make_devplan;
//                        sa_dplan.inc (the device planner); sa_batch_destroy; sa_batch_build.inc (a batch's creation); a pass
//                        (sa_ring_lanes, submit_group, enqueue_pass, after_pass), the two run paths, the accessors and the rest of the API
//
// The file is compiled with -ffp-contract=off; where fused multiply-add is wanted it is spelled fma().
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <time.h>
#include <type_traits>
#include <vector>

#include "sa_internal.h"
#include "sa_plan_rules.h"
#include "sa_chain.h"

#define NEG_INF (-__builtin_inf())

// ---------------------------------------------------------------------------------------------------
// device-side views
// ---------------------------------------------------------------------------------------------------
struct DevModel {
    double t_mm, t_mx, t_my, t_xm, t_xx, t_ym, t_yy;
    const double *tab6;     // per k-mer: mu, sd, c(sd), sdY, c(sdY), 0   with c(s) = -log(sqrt(2 pi)) - log(s)
    long long pow_km1;
    int n_alpha;
    int hdp;
    int emission;           // 0: MeanOnly (what signalMachine installs); 1 / 2: the two-distribution emission with / without descaling (sa_model_set_emission)
    const double *noise3;   // emission 1: per k-mer noise mean, noise lambda, log(lambda)  (columns 2 and 4 of the model table)
    const int *hdp_slot;    // per k-mer: row of y/slope tables of the first observed ancestor, -1 if none
    const double *hdp_y, *hdp_slope, *hdp_grid;
    const double *hdp_tab;  // register kernels: {y[i], slope[i]} interleaved, one row per observed process
    const double *hdp_coef; // k_emit_hdp: the four cubic coefficients of interval i of every row (twice the size of hdp_tab)
    double hdp_g0, hdp_gN, hdp_dx;
    unsigned hdp_tab_bytes;
    unsigned hdp_hot;       // byte offset in hdp_tab of the row most k-mers resolve to (0xffffffff: no such row)
    int grid_len;
};

struct DevPlan {
    const sa_region_t *regions;
    const sa_row_t *rows;
    const int *pk;
    const int *poff;
    const int *pid;
    const int *px;        // reference position (region-relative x) of every pid entry: cell-path -> cell
    const double *xc;
    const sa_prec_t *prec; // per cell-path records of SA_KIND_RING regions with several paths per cell
    const double *ev;
    const double *evn;    // two-distribution emission only: per event its noise and log(noise) (C library's log, from the host)
    const sa_seg_t *segs;
    const sa_ck_t *cks;
    double *F;
    double *E;        // HDP models: emission plane of the register-kernel regions (k_emit_hdp), max_chunk_cellpaths doubles
    const double *two;     // two-distribution emission on the register kernels (k_*_fast_two): the noise constants, else nullptr
    long long two_xn_off;  // ... first entry (double4) of the per-position part (FastT.two_xn_off)
    double *vbuf;
    sa_cand_t *cands;
    int *cand_count;
    int *overflow;
    double *totals;
    double *bscratch;
    double *gsum;     // EXPECT: 8 doubles per checkpoint group (7 live transitions)
    double *gmc;      // EXPECT: the group's scaling maximum
    DevModel m;
    double log_thr;   // log(threshold)
    double threshold;
    double *spec;     // ring / strip kernels: per traceback segment its speculative total (NaN: a segment of another kernel family)
    double spec_slack;
    int expect;       // the expectation pass (sa_expect_batch)
};

// ---------------------------------------------------------------------------------------------------
// logAdd: impl/pairwiseAligner.c:298-318.  The coefficients are float literals promoted to double.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double la_lookup(double x) {
    if (x <= 1.00f)
        return ((-0.009350833524763f * x + 0.130659527668286f) * x + 0.498799810682272f) * x + 0.693203116424741f;
    if (x <= 2.50f)
        return ((-0.014532321752540f * x + 0.139942324101744f) * x + 0.495635523139337f) * x + 0.692140569840976f;
    if (x <= 4.50f)
        return ((-0.004605031767994f * x + 0.063427417320019f) * x + 0.695956496475118f) * x + 0.514272634594009f;
    return ((-0.000458661602210f * x + 0.009695946122598f) * x + 0.930734667215156f) * x + 0.168037164329057f;
}

__device__ __forceinline__ double la_exact(double x, double y) {
    if (x < y) return (x == NEG_INF || y - x >= 7.5) ? y : la_lookup(y - x) + x;
    return (y == NEG_INF || x - y >= 7.5) ? x : la_lookup(x - y) + y;
}

// ---------------------------------------------------------------------------------------------------
// emissions in reference order (impl/stateMachine.c:296-306, :344-348, :527-605)
// ---------------------------------------------------------------------------------------------------
struct ReadPar {
    double scale, shift, var, lvar;
    const double *evn;   // the region's {noise, log noise} pairs (two-distribution emission), else nullptr
};

__device__ __forceinline__ double hdp_interp(const DevModel &m, int slot, double q) {
    const double *x = m.hdp_grid;
    const double *y = m.hdp_y + (long long) slot * m.grid_len;
    const double *s = m.hdp_slope + (long long) slot * m.grid_len;
    int n = m.grid_len;
    if (q <= x[0]) return y[0] - s[0] * (x[0] - q);
    if (q >= x[n - 1]) return y[n - 1] + s[n - 1] * (q - x[n - 1]);
    double dx = x[1] - x[0];
    long long il = (long long) ((q - x[0]) / dx);
    long long ir = il + 1;
    double dy = y[ir] - y[il];
    double a = s[il] * dx - dy;
    double b = dy - s[ir] * dx;
    double tl = (q - x[il]) / dx;
    double tr = 1.0 - tl;
    return tr * y[il] + tl * y[ir] + tl * tr * (a * tr + b * tl);
}

// match != 0: EMISSION_MATCH_MATRIX; == 0: EMISSION_GAP_Y_MATRIX (sd * 1.75).  id < 0: NULL k-mer.
// yi: index of the event (matrix row - 1), read by the two-distribution emission only
__device__ __forceinline__ double emit_ref(const DevModel &m, const ReadPar &rp, int id, double e, int match, long long yi) {
    if (id < 0) return NEG_INF;
    const double *t = m.tab6 + 6ll * id;
    double mu = t[0];
    double en = (e + rp.var * mu - rp.scale * mu - rp.shift) / rp.var;
    if (m.emission != 0) {
        // emissions_signal_strawManGetKmerEventMatchProbWithDescaling (impl/stateMachine.c:607-650): logGaussPdf of the descaled
        // mean + logInvGaussPdf of the event noise (:296-306, :320-330), in the reference's order of operations; emission 2 is
        // emissions_signal_strawManGetKmerEventMatchProb (:659-700): the same on the event mean as it is (the MODEL was scaled)
        if (m.emission == 2) en = e;
        double sd = match ? t[1] : t[3];
        double c = match ? t[2] : t[4];  // -log(sqrt(2 pi)) - log(sd); -inf when sd == 0
        double a = (en - mu) / sd;
        double l1 = c + (-0.5 * a * a);
        double n = rp.evn[2 * yi], l_n = rp.evn[2 * yi + 1];
        const double *nz = m.noise3 + 3ll * id;
        double a2 = (n - nz[0]) / nz[0];
        double l2 = (nz[2] - 1.8378770664093453 - 3 * l_n - nz[1] * a2 * a2 / n) / 2;
        return l1 + l2;
    }
    if (m.hdp) {
        int slot = m.hdp_slot[id];
        if (slot < 0) return NEG_INF;
        double d = hdp_interp(m, slot, en);
        d = d > 0.0 ? d : 0.0;
        double density = (1 / rp.var) * d;
        return log(density);
    }
    double sd = match ? t[1] : t[3];
    double c = match ? t[2] : t[4];  // -inf when sd == 0
    double a = (en - mu) / sd;
    return rp.lvar + (c + (-0.5 * a * a));
}

// Maximum over the 64 lanes, wave-uniform (values may be -inf, never NaN).  Six DPP steps -- butterflies inside a row of 16
// (quad_perm xor 1, xor 2, row_half_mirror, row_mirror), then row_bcast15 into rows 1 and 3 and row_bcast31 into rows 2 and 3 --
// leave the maximum in lane 63, which v_readlane hands to every lane as a scalar: 33 issue slots.  The generic __shfl_xor
// butterfly costs 85 per reduction (ds_bpermute pairs, lane arithmetic, selects, their waits and hazards), and the backward
// sweeps reduce twice per checkpoint, i.e. twice per ten diagonals: an eighth of k_bwd_fast's instructions.
// A lane without a source (or outside the row mask) keeps `old` = its own value: max(v, v).
__device__ __forceinline__ double wave_max(double v) {
    int lo_, hi_;
    double o_;
    // (butterflies: every lane has a source, the move needs no old value -- no copy in front of it)
#define SA_WMAX_BFLY(CTRL)                                                                       \
    lo_ = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);                    \
    hi_ = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);                    \
    o_ = __hiloint2double(hi_, lo_);                                                             \
    asm("v_max_f64 %0, %1, %2" : "=v"(v) : "v"(v), "v"(o_));
    // (broadcasts: a lane outside the row mask keeps what the previous step left in the same registers -- a value that
    // already went into its maximum)
#define SA_WMAX_BCAST(CTRL, ROWS)                                                                \
    lo_ = __builtin_amdgcn_update_dpp(lo_, __double2loint(v), CTRL, ROWS, 0xF, false);           \
    hi_ = __builtin_amdgcn_update_dpp(hi_, __double2hiint(v), CTRL, ROWS, 0xF, false);           \
    o_ = __hiloint2double(hi_, lo_);                                                             \
    asm("v_max_f64 %0, %1, %2" : "=v"(v) : "v"(v), "v"(o_));
    SA_WMAX_BFLY(0xB1)           // quad_perm:[1,0,3,2]
    SA_WMAX_BFLY(0x4E)           // quad_perm:[2,3,0,1]
    SA_WMAX_BFLY(0x141)          // row_half_mirror
    SA_WMAX_BFLY(0x140)          // row_mirror: every lane holds its row's maximum
    SA_WMAX_BCAST(0x142, 0xA)    // row_bcast15 -> rows 1, 3
    SA_WMAX_BCAST(0x143, 0xC)    // row_bcast31 -> rows 2, 3: lane 63 holds the wave's
#undef SA_WMAX_BFLY
#undef SA_WMAX_BCAST
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
// Sum over the 64 lanes, wave-uniform, with the same six DPP steps (the butterflies are true pairings, so every lane of a row
// ends with its row's sum; a lane outside a broadcast's row mask adds 0.0).  The order of the additions differs from a serial
// sum's, as the __shfl_xor butterfly's did.
__device__ __forceinline__ double wave_sum(double v) {
    int lo_, hi_;
#define SA_WSUM_BFLY(CTRL)                                                                       \
    lo_ = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);                    \
    hi_ = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);                    \
    v += __hiloint2double(hi_, lo_);
#define SA_WSUM_BCAST(CTRL, ROWS)                                                                \
    lo_ = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWS, 0xF, false);             \
    hi_ = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWS, 0xF, false);             \
    v += __hiloint2double(hi_, lo_);
    SA_WSUM_BFLY(0xB1)
    SA_WSUM_BFLY(0x4E)
    SA_WSUM_BFLY(0x141)
    SA_WSUM_BFLY(0x140)
    SA_WSUM_BCAST(0x142, 0xA)
    SA_WSUM_BCAST(0x143, 0xC)
#undef SA_WSUM_BFLY
#undef SA_WSUM_BCAST
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
__device__ __forceinline__ int wave_max_i(int v) {
    for (int off = 32; off > 0; off >>= 1) {
        int o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

#include "sa_fast.inc"
#include "sa_ring.inc"
#include "sa_strip.inc"
#include "sa_generic.inc"
#include "sa_result.inc"
#include "sa_runtime.inc"

// Launch classes: every chunk (forward pass over regions) and every group (traceback segments) has one id list per class, laid out
// in d_ids in this order.  launch_class() says which class a region -- and so each of its segments -- belongs to.
enum {
    LC_GENERIC = 0,            // memory-resident kernels
    LC_FAST = 1,               // register kernels
    LC_RING = 2,               // ring kernels: LC_RING + multi * 8 + cap class, cap = 64 * (class + 1)
    LC_STRIP = LC_RING + 16,   // one-path ring-kernel regions taken by the strip kernels (sa_strip.inc)
    LC_RING_WIDE,              // ring kernels, several paths per cell, rows of SA_RING_WIDE_MAX_ROWPATHS (sa_internal.h)
    LC_N
};
struct sa_ids {
    long long off;   // into d_ids
    int n;
};
// how many of the classes [c0, c1) have a non-empty list
static int n_nonempty(const sa_ids *ids, int c0, int c1) {
    int n = 0;
    for (int c = c0; c < c1; c++) n += ids[c].n > 0;
    return n;
}
static int launch_class(const sa_region_t &R, bool strip_on) {
    if (strip_region(&R, strip_on)) return LC_STRIP;
    if (R.kind == SA_KIND_RING) {
        if (R.max_rowpaths > SA_RING_MAX_ROWPATHS) return LC_RING_WIDE;
        const int cl = R.max_rowpaths <= 64 ? 0 : (int) ((R.max_rowpaths - 1) / 64);   // <= 7 (SA_RING_MAX_ROWPATHS)
        return LC_RING + (R.max_p > 1 ? 8 : 0) + (cl > 7 ? 7 : cl);
    }
    return R.kind == SA_KIND_FAST ? LC_FAST : LC_GENERIC;
}
// the ring class cl (launch class LC_RING + cl): rows of up to `cap` cell-paths, several paths per cell when `multi`
struct ring_class_shape {
    int cap;
    bool multi;
};
static ring_class_shape ring_class(int cl) { return {64 * ((cl & 7) + 1), cl >= 8}; }
// The ring classes' lists in launch order: the wide class, then the widest (longest-running) classes first.  Calls
// fn(list, cap, multi) for every non-empty list; the first non-zero return ends the walk and is returned.
template <typename Fn>
static int for_each_ring_list(const sa_ids *ids, Fn fn) {
    if (ids[LC_RING_WIDE].n) TRY(fn(ids[LC_RING_WIDE], SA_RING_WIDE_MAX_ROWPATHS, true));
    for (int cl = 15; cl >= 0; cl--) {
        const sa_ids &L = ids[LC_RING + cl];
        if (L.n) TRY(fn(L, ring_class(cl).cap, ring_class(cl).multi));
    }
    return SA_OK;
}
struct sa_launch_chunk {
    sa_ids ids[LC_N];          // regions
    int g0, g1;                // groups [g0, g1)
};
struct sa_launch_group {
    long long seg0, seg1, ck0, ck1;
    sa_ids ids[LC_N];          // segments, by the class of their region
    unsigned seam_first;       // their first wave slot in the seam storage
};

// A batch's queues.  Compute lane 0 carries a pass's forward sweeps and, in turn with lane 1, its groups; lanes 2 and 3 hold nothing but
// forward launches of the ring-kernel classes (sa_ring_lanes).  Lane 0 is also the device planner's event gather's and sa_expect_batch's.
struct sa_lanes {
    enum { N = 4 };
    hipStream_t compute[N] = {};   // 0 and 1 from the batch's creation, 2 and 3 on first need
    hipStream_t pair = nullptr;    // the pairs themselves: high priority, the copy stream outranks the compute lanes
    // compute lane q, made on first need; nullptr when no stream can be had
    hipStream_t lane(int q, int device) {
        if (!compute[q] && g_handles.stream(&compute[q], device, 0) != hipSuccess) compute[q] = nullptr;
        return compute[q];
    }
    // waits for all of them -- asleep on a blocking event (sa_sync_stream) or, with `spin`, in hipStreamSynchronize; the first error
    hipError_t drain(int device, bool spin) {
        hipError_t first = hipSuccess;
        for (hipStream_t s : {compute[0], compute[1], compute[2], compute[3], pair}) {
            const hipError_t e = !s ? hipSuccess : spin ? hipStreamSynchronize(s) : sa_sync_stream(s, device);
            if (first == hipSuccess) first = e;
        }
        return first;
    }
    void park(int device) {
        for (hipStream_t s : compute) g_handles.park(s, device, 0);
        g_handles.park(pair, device, 1);
    }
};
// The events of a pass, of each of its chunks and of each of its groups: all() is what is made and parked
struct sa_pass_events {
    hipEvent_t pass_begin = nullptr, pass_end = nullptr;
    hipEvent_t lane_fork = nullptr;           // sa_ring_lanes: lane 0 has queued what the other lanes' launches read
    hipEvent_t lane_join[sa_lanes::N] = {};   // ... [q]: lane q has queued its launches, lane 0 waits for it ([0] is never made)
    hipEvent_t planner_gather = nullptr;      // sa_dplan.inc: the upload stream has queued what the event gather on lane 0 reads
    std::array<hipEvent_t *, 7> all() { return {&pass_begin, &lane_fork, &lane_join[1], &lane_join[2], &lane_join[3], &pass_end, &planner_gather}; }
};
struct sa_chunk_events {
    hipEvent_t fwd_begin = nullptr, fwd_end = nullptr;
    std::array<hipEvent_t *, 2> all() { return {&fwd_begin, &fwd_end}; }
};
struct sa_group_events {
    hipEvent_t bwd_begin = nullptr, bwd_end = nullptr, ready = nullptr;   // ready: behind the group's last kernel
    std::array<hipEvent_t *, 3> all() { return {&bwd_begin, &bwd_end, &ready}; }
};
template <typename E>   // (one of the three above)
static int events_make(E &ev, int device) {
    for (hipEvent_t *e : ev.all())
        if (g_handles.event(e, device) != hipSuccess) return SA_ENODEVICE;
    return SA_OK;
}
template <typename E>
static void events_park(E &ev, int device) { for (hipEvent_t *e : ev.all()) g_handles.park(*e, device); }

struct sa_batch {
    sa_plan_t *plan = nullptr;
    int device = -1;
    unsigned flags = 0;
    sa_lanes lanes;
    // device buffers (blocks() lists them)
    sa_region_t *d_regions = nullptr; sa_row_t *d_rows = nullptr; int *d_pk = nullptr; int *d_poff = nullptr; int *d_pid = nullptr;
    int *d_px = nullptr; double *d_xc = nullptr; double *d_ev = nullptr; sa_prec_t *d_prec = nullptr;
    size_t d_blk_bytes = 0;
    char *d_blk = nullptr;   // SA_FLAG_INPUTS_IN_HOST_BLOCK: the image of the caller's block (its event records are gathered on this
                             // batch's own stream, possibly after sa_batch_create has returned: kept until the batch goes)
    sa_seg_t *d_segs = nullptr; sa_ck_t *d_cks = nullptr;
    double *d_F = nullptr; double *d_E = nullptr; double *d_vbuf = nullptr; sa_cand_t *d_cands = nullptr; int *d_cand_count = nullptr;
    double *d_totals = nullptr; double *d_bscratch = nullptr;
    double *d_gsum = nullptr, *d_gmc = nullptr;   // expectation mode only
    bool expect = false;
    bool relax = false;        // memory-resident kernels in their RELAX flavour
    int ring_cap = 0;          // cell-paths per diagonal of their LDS ring (0: rows stay in global memory)
    int wide_cap = 0;          // cells per row of the register kernels' LDS ring for wide diagonals (0: every diagonal fits)
    int gen_threads = 64;      // 64, or 128 when a diagonal of a memory-resident region holds more than 64 cell-paths
    bool strip_on = false;     // one-path ring-kernel regions run on the strip kernels (default; SA_STRIP=0: ring kernels)
    double *d_spec = nullptr;  // ring / strip kernels: speculative totals, one per segment (NaN: a segment of another kernel family)
    double spec_slack = 0;     // candidates: forward + backward >= spec - slack + log(threshold); grows when a pass has to be repeated
    int spec_repeats = 0;      // passes repeated because of it (the second repeat drops the bound altogether)
    bool released = false;     // sa_batch_release_device: the working storage went back to the pool, the results stay
    unsigned long long *d_sortkey = nullptr;   // k_gather_sorted's scratch: 8 + 4 bytes per candidate slot
    unsigned *d_sortidx = nullptr;
    unsigned long long *d_vc_bits = nullptr;   // SA_FLAG_VC_ROWS: see k_finalize
    long long *d_vc_off = nullptr, *d_seg_all = nullptr;
    std::vector<unsigned long long> h_vc_bits;  // (the same on the host, for SA_FLAG_EXACT's host finalisation)
    std::vector<long long> h_vc_off, job_all_n, job_all_sum;
    SaAmbigTab *ambig_tab[SA_TAB_N] = {};       // SA_FLAG_SITE_CALLS / SA_FLAG_POSITION_CALLS: the batch's sites / ambiguous positions
    bool plan_hdp = false;                      // the batch's model holds an HDP
    unsigned hdp_hot = 0xffffffffu;             // DevModel.hdp_hot
    char *d_seam = nullptr;      // their seam storage: per wave two arrays of seam_cap records of 16 bytes
    unsigned seam_cap = 0;
    unsigned seam_cap_bwd = 0;   // records per seam array of the backward launches (a traceback segment is shorter than a region)
    long long seam_bwd_off = 0;  // bytes: the forward launch's slots come first, then those of a pass's backward launches
    double *d_two = nullptr; long long two_xn_off = 0;   // two-distribution emission on the register kernels (DevPlan.two)
    double *d_tab6 = nullptr; double *d_noise3 = nullptr; double *d_evn = nullptr; int *d_hdp_slot = nullptr;
    double *d_hdp_y = nullptr, *d_hdp_slope = nullptr, *d_hdp_grid = nullptr, *d_hdp_tab = nullptr, *d_hdp_coef = nullptr;
    long long *d_prob = nullptr; int *d_seg_pass = nullptr; long long *d_seg_off = nullptr; sa_pair16_t *d_out = nullptr;
    int *d_ids = nullptr;  // region / segment id lists per launch
    long long cand_alloc = 0;
    long long out_alloc = 0;
    int cand_factor = 1;           // candidate capacity relative to the planner's 2 per posterior diagonal (overflow re-runs)
    // launch lists (host): a chunk is one forward-storage pass; its traceback segments are cut into groups of
    // consecutive reads so that the result copy of one group overlaps the backward kernels of the next
    std::vector<sa_launch_chunk> chunks;
    std::vector<sa_launch_group> groups;
    std::vector<int> ids_flat;
    sa_pass_events ev;
    std::vector<sa_chunk_events> chunk_ev;
    std::vector<sa_group_events> group_ev;
    long long *h_seg_off = nullptr;      // pinned: per group n+1 exclusive offsets
    int *h_overflow = nullptr;           // pinned
    // results
    sa_pair16_t *h_pairs = nullptr;   // pinned host copy of all pairs (packed, sa_internal.h), job after job
    bool p8 = false;         // SA_FLAG_PAIRS8: the records are 8 bytes (sa_pair8_t), in h_pairs and in d_out alike
    size_t rec() const { return p8 ? sizeof(sa_pair8_t) : sizeof(sa_pair16_t); }
    sa_pair16_t *out_at(long long slot) const { return reinterpret_cast<sa_pair16_t *>(reinterpret_cast<char *>(d_out) + rec() * (size_t) slot); }
    sa_pair16_t *host_at(long long slot) const { return reinterpret_cast<sa_pair16_t *>(reinterpret_cast<char *>(h_pairs) + rec() * (size_t) slot); }
    long long h_pairs_cap = 0, n_pairs_total = 0;
    std::vector<long long> job_off;
    std::vector<long long> job_dev_off;   // where a job's pairs start in d_out (device finalisation only)
    void *d_pairs_up = nullptr;           // host-finalised records uploaded for a downstream device step (sa_batch_view)
    size_t d_pairs_up_cap = 0;            // bytes
    bool ran = false;
    bool quiet = false;          // the last run returned SA_OK: it waited for everything it had queued, the batch's streams are idle
    bool dev_planned = false;    // the plan was built on the device (sa_dplan.inc): its big arrays exist in HBM only
    std::thread *runner = nullptr;   // sa_batch_start .. sa_batch_wait
    int runner_rc = SA_OK;
    sa_batch_stats_t stats{};
    // Creation in two halves (sa_batch_create_deferred): what the second half needs.  `pending` is the device plan whose kernels
    // are queued; the caller's arrays (c_jobs, c_ambig) are only touched again if that plan turns a read down and the host
    // planner takes over -- which is why a deferred batch asks the caller to keep them until its first run has returned.
    struct DPlanPending *pending = nullptr;
    const sa_model_t *c_m = nullptr;
    int c_k = 0, c_n_alpha = 0;   // c_m's k-mer length and alphabet size (kept: a chained stage asks after the model may be gone)
    sa_params_t c_p{};
    const sa_job_t *c_jobs = nullptr;
    int64_t c_n = 0;
    const char *const *c_ambig = nullptr;
    std::vector<sa_noise_scale_t> c_noise;   // sa_batch_create_noise_scaled: every job's two factors (a copy), else empty
    long long c_budget = 0;
    double c_t0 = 0;
    bool c_deferred = false;
    char *held_stage = nullptr;   // (deferred batches: see dplan_back)
    bool finished = false;
    int prepare_rc = SA_OK;
    bool prepared = false;        // plan collected and launch lists built (sa_batch_prepare, or the first step of finishing)
    long long lw_strip_max_n = 0, lw_strip_max_seg = 0, lw_strip_fwd_slots = 0, lw_strip_bwd_slots = 0;   // from the launch lists: seam storage
    int finish_rc = SA_OK;
    std::mutex fin_mu;

    // Every device block above that the batch takes from the caching allocator, by lifetime:
    //   [0, BLK_PLAN)         working storage: what build_working (batch_finish_body) allocates, released by release_working
    //   [BLK_PLAN, BLK_REST)  the planner's arrays: sa_dplan.inc's dplan_release gives them back when the device plan is dropped
    //   [BLK_REST, BLK_END)   everything else, kept until sa_batch_release_device or sa_batch_destroy
    // d_pairs_up is not listed: it survives sa_batch_release_device.
    enum { BLK_PLAN = 17, BLK_REST = 26, BLK_END = 43 };
    std::array<void **, BLK_END> blocks() {
        const std::array all{
            (void **) &d_F, (void **) &d_E, (void **) &d_vbuf, (void **) &d_cands, (void **) &d_prob, (void **) &d_cand_count,
            (void **) &d_seg_pass, (void **) &d_seg_off, (void **) &d_totals, (void **) &d_bscratch,
            (void **) &d_gsum, (void **) &d_gmc, (void **) &d_seam, (void **) &d_spec, (void **) &d_sortkey, (void **) &d_sortidx,
            (void **) &d_out,
            (void **) &d_regions, (void **) &d_rows, (void **) &d_pk, (void **) &d_poff, (void **) &d_pid, (void **) &d_ev,
            (void **) &d_segs, (void **) &d_cks, (void **) &d_prec,
            (void **) &d_px, (void **) &d_xc, (void **) &d_blk, (void **) &d_tab6, (void **) &d_noise3, (void **) &d_evn,
            (void **) &d_hdp_slot, (void **) &d_hdp_y, (void **) &d_hdp_slope, (void **) &d_hdp_grid, (void **) &d_hdp_tab,
            (void **) &d_hdp_coef, (void **) &d_two, (void **) &d_vc_bits, (void **) &d_vc_off, (void **) &d_seg_all,
            (void **) &d_ids};
        static_assert(all.size() == BLK_END, "sa_batch::blocks: the list and BLK_END disagree");
        return all;
    }
    // gives the blocks [lo, hi) back to the caching allocator
    void put_blocks(int lo, int hi) {
        const auto slot = blocks();
        for (int i = lo; i < hi; i++)
            if (*slot[i]) { g_sa_pool.put(SaPool::DEVICE, *slot[i]); *slot[i] = nullptr; }
    }
};

static DevPlan make_devplan(const sa_batch *b) {
    const sa_plan_t *pl = b->plan;
    const sa_model_t *m = pl->model;
    DevPlan P;
    memset(&P, 0, sizeof(P));
    P.regions = b->d_regions; P.rows = b->d_rows; P.pk = b->d_pk; P.poff = b->d_poff; P.pid = b->d_pid; P.px = b->d_px; P.xc = b->d_xc; P.ev = b->d_ev;
    P.prec = b->d_prec;
    P.segs = b->d_segs; P.cks = b->d_cks; P.F = b->d_F; P.E = b->d_E; P.vbuf = b->d_vbuf; P.cands = b->d_cands;
    P.cand_count = b->d_cand_count; P.overflow = b->h_overflow; P.totals = b->d_totals; P.bscratch = b->d_bscratch;
    P.gsum = b->d_gsum; P.gmc = b->d_gmc;
    P.two = b->d_two; P.two_xn_off = b->two_xn_off;
    P.m.t_mm = m->t_mm; P.m.t_mx = m->t_mx; P.m.t_my = m->t_my; P.m.t_xm = m->t_xm; P.m.t_xx = m->t_xx;
    P.m.t_ym = m->t_ym; P.m.t_yy = m->t_yy;
    P.m.tab6 = b->d_tab6; P.m.emission = m->emission; P.m.noise3 = b->d_noise3; P.evn = b->d_evn; P.m.pow_km1 = m->pow_km1; P.m.n_alpha = m->n_alpha; P.m.hdp = m->hdp ? 1 : 0;
    P.m.hdp_slot = b->d_hdp_slot; P.m.hdp_y = b->d_hdp_y; P.m.hdp_slope = b->d_hdp_slope; P.m.hdp_grid = b->d_hdp_grid;
    P.m.grid_len = m->hdp ? (int) m->hdp->grid_length : 0;
    if (m->hdp) {
        const sa_hdp_t *h = m->hdp;
        P.m.hdp_tab = b->d_hdp_tab;
        P.m.hdp_coef = b->d_hdp_coef;
        P.m.hdp_g0 = h->grid[0];
        P.m.hdp_gN = h->grid[h->grid_length - 1];
        P.m.hdp_dx = h->grid[1] - h->grid[0];  // grid_spline_interp: dx = x[1] - x[0]
        P.m.hdp_tab_bytes = (unsigned) (h->n_slots * h->grid_length * 16);
        P.m.hdp_hot = b->hdp_hot;
    }
    P.threshold = pl->params.threshold;
    P.log_thr = log(pl->params.threshold);
    P.spec = b->d_spec;
    P.spec_slack = b->spec_slack;
    P.expect = b->expect ? 1 : 0;
    return P;
}

static std::atomic<int> g_batches_started(0);   // batches between sa_batch_start and sa_batch_wait (this process)
// The pinned result block holds an eighth more than `total`; a batch that has not run expects what g_pairs_memo says of its kind
static long long pairs_block_cap(long long total) { return total + total / 8 + 1024; }
static long long expected_pairs(const sa_batch *b) {
    return (long long) (g_pairs_memo.estimate(b->plan->model->uid, b->device, b->plan->params.threshold) * (double) b->plan->n_ev) + 4096;
}

#include "sa_dplan.inc"

void sa_batch_destroy(sa_batch_t *b) {
    if (!b) return;
    if (b->runner) { b->runner->join(); delete b->runner; b->runner = nullptr; g_batches_started.fetch_sub(1); }
    if (b->device >= 0) (void) hipSetDevice(b->device);
    if (b->pending) { dplan_release(b, b->pending, true); b->pending = nullptr; }   // created, never used
    // the storage goes back to the caching allocators without the implicit synchronisation of hipFree: nothing of this
    // batch may still be in flight (only possible after an error inside a run)
    const bool trace_d = getenv("SA_TRACE") != nullptr;
    const double td0 = now_ms();
    // (a failed or interrupted run, or a batch that never ran: 0.6-0.9 ms of API calls otherwise, per batch, on the thread that is
    // about to plan the next one)
    if (!b->quiet) (void) b->lanes.drain(b->device, true);
    const double td1 = now_ms();
    b->put_blocks(0, sa_batch::BLK_END);
    events_park(b->ev, b->device);
    for (sa_group_events &e : b->group_ev) events_park(e, b->device);
    for (sa_chunk_events &e : b->chunk_ev) events_park(e, b->device);
    b->lanes.park(b->device);
    g_sa_pool.put(SaPool::PINNED, b->h_pairs);
    g_sa_pool.put(SaPool::PINNED, b->held_stage);
    g_sa_pool.put(SaPool::DEVICE, b->d_pairs_up);
    g_sa_pool.put(SaPool::PINNED, b->h_seg_off);
    g_sa_pool.put(SaPool::PINNED, b->h_overflow);
    for (SaAmbigTab *tab : b->ambig_tab) sa_ambig_free(tab);
    const double td2 = now_ms();
    sa_plan_free(b->plan);
    delete b;
    if (trace_d) fprintf(stderr, "[trace] destroy: streams idle after %.2f ms, blocks parked after %.2f ms, done after %.2f ms\n", td1 - td0, td2 - td0, now_ms() - td0);
}

#include "sa_batch_build.inc"

// One pass = per chunk the forward sweeps (compute lane 0; the ring-kernel classes fork over up to four lanes and join
// it again: sa_ring_lanes), then per group the backward/posterior kernels, the exact fold of its checkpoints and -- with
// `finalize` -- the on-device finalisation (k_scan also writes the segment offsets straight into pinned host memory).
// Consecutive groups alternate between compute lanes 0 and 1: the next group's waves move in while the previous group's
// last waves drain, so cutting the traceback work into groups costs no idle tail.  Everything is queued up front;
// `after_group` waits for one group's `ready` event and requests its pairs on the pair stream.  No copy that
// depends on a kernel is ever queued: the copy engine works in order, and a transfer waiting for a kernel would hold
// back the pair copies of groups that are already finished (measured: probes/copy_overlap.hip).
static int submit_group(sa_batch *b, const DevPlan &P, int g, int which_stream, bool finalize) {
    sa_plan_t *pl = b->plan;
    const sa_launch_group &G = b->groups[g];
    hipStream_t st = b->lanes.compute[which_stream];
    HIPCHK(hipEventRecord(b->group_ev[(size_t) g].bwd_begin, st));
    const sa_ids &Lg = G.ids[LC_GENERIC], &Ls = G.ids[LC_STRIP], &Lf = G.ids[LC_FAST];
    if (Lg.n) launch_bwd_generic(P, b->d_ids + Lg.off, Lg.n, st, b->gen_threads, b->relax, b->ring_cap);
    if (Ls.n)
        launch_bwd_strip(P, b->d_ids + Ls.off, Ls.n, st, b->d_seam + b->seam_bwd_off,
                         make_strip_t(P, pl->n_ev + 8, b->seam_cap_bwd, G.seam_first));
    TRY(for_each_ring_list(G.ids, [&](const sa_ids &L, int cap, bool multi) {
        return launch_bwd_ring(P, b->d_ids + L.off, L.n, st, cap, multi);
    }));
    if (Lf.n) { const int rcl = launch_bwd_fast(P, b->d_ids + Lf.off, Lf.n, st); if (rcl) return rcl; }
    HIPCHK(hipEventRecord(b->group_ev[(size_t) g].bwd_end, st));
    if (G.ck1 > G.ck0)
        hipLaunchKernelGGL(k_fold, dim3((unsigned) ((G.ck1 - G.ck0 + 63) / 64)), dim3(64), 0, st, P, G.ck0, G.ck1);
    if (finalize) {
        const int n = (int) (G.seg1 - G.seg0);
        long long *soff = b->d_seg_off + G.seg0 + g;
        // (groups without register / ring / strip segments: no look at the speculative totals)
        const double *spec = (b->d_spec && n_nonempty(G.ids, LC_FAST, LC_N) > 0) ? b->d_spec : nullptr;
        hipLaunchKernelGGL(k_finalize, dim3((unsigned) n), dim3(64), 0, st, P, (int) G.seg0, n, b->d_prob, b->d_seg_pass, spec,
                           b->spec_slack, (const unsigned long long *) b->d_vc_bits, (const long long *) b->d_vc_off, b->d_seg_all);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, b->d_seg_pass + G.seg0, soff, b->h_seg_off + G.seg0 + g, n);
        sa_pair16_t *const gout = b->out_at(pl->segs[G.seg0].cand_off);
        hipLaunchKernelGGL(k_gather, dim3((unsigned) n), dim3(64), 0, st, P, (int) G.seg0, n, b->d_prob, soff,
                           gout, spec, (b->strip_on && b->d_sortkey) ? 1 : 0, b->p8 ? 1 : 0);
        if (spec && Ls.n > 0 && b->d_sortkey)
            hipLaunchKernelGGL(k_gather_sorted, dim3((unsigned) n), dim3(64), 0, st, P, (int) G.seg0, n, b->d_prob, soff,
                               gout, spec, b->d_sortkey, b->d_sortidx, b->p8 ? 1 : 0);
    }
    HIPCHK(hipEventRecord(b->group_ev[(size_t) g].ready, st));
    return SA_OK;
}

// The lanes of a chunk's ring-kernel forward launches, one launch per class of row capacity (the strip kernels' list among them).
// A forward launch holds one workgroup per read and lasts as long as its longest read's serial chain, so launches that follow each
// other on one stream leave the chip mostly empty three times over: the lists go round the compute lanes and run side by side.
// In this order: make it, queue on lane 0 what the launches read, fork(), one next() per list, join().
struct sa_ring_lanes {
    hipStream_t lane[sa_lanes::N] = {};
    int n = 0, k = 0;
    // as many lanes as lists, four at most, fewer when a stream cannot be had
    sa_ring_lanes(sa_batch *b, const sa_ids *ids) {
        const int n_lists = n_nonempty(ids, LC_RING, LC_N);
        for (n = 0; n < n_lists && n < sa_lanes::N; n++)
            if (!(lane[n] = b->lanes.lane(n, b->device))) break;
        lane[0] = b->lanes.compute[0];
        if (getenv("SA_TRACE")) fprintf(stderr, "[trace] pass: %d ring lists on %d lanes\n", n_lists, n);
    }
    int fork(sa_batch *b) {
        if (n > 1) HIPCHK(hipEventRecord(b->ev.lane_fork, lane[0]));
        for (int q = 1; q < n; q++) HIPCHK(hipStreamWaitEvent(lane[q], b->ev.lane_fork, 0));
        return SA_OK;
    }
    hipStream_t next() { return lane[n > 1 ? k++ % n : 0]; }   // the strip list first: on lane 0
    int join(sa_batch *b) {
        for (int q = 1; q < n; q++) {
            HIPCHK(hipEventRecord(b->ev.lane_join[q], lane[q]));
            HIPCHK(hipStreamWaitEvent(lane[0], b->ev.lane_join[q], 0));
        }
        return SA_OK;
    }
};

template <typename AfterGroup>
static int enqueue_pass(sa_batch *b, bool finalize, AfterGroup after_group) {
    sa_plan_t *pl = b->plan;
    DevPlan P = make_devplan(b);
    hipStream_t s0 = b->lanes.compute[0], s1 = b->lanes.compute[1];
    HIPCHK(hipMemsetAsync(b->d_cand_count, 0, 4 * (size_t) at_least_1(pl->n_segs), s0));
    if (b->d_spec)   // all bits set = NaN: "not a segment of the ring / strip kernels" until their forward sweep says otherwise
        HIPCHK(hipMemsetAsync(b->d_spec, 0xff, 8 * (size_t) at_least_1(pl->n_segs), s0));
    b->h_overflow[0] = 0;  // pinned host word the kernels raise directly
    b->h_overflow[1] = 0;  // ... and the one k_finalize raises when a speculative candidate bound turns out too high
    b->h_overflow[2] = 0;  // ... and k_check_events' / k_spec_match's: an event mean or a forward value that is not a number
    if (pl->n_ev > 0)
        hipLaunchKernelGGL(k_check_events, dim3((unsigned) std::min<long long>((pl->n_ev + 255) / 256, 2048)), dim3(256), 0, s0,
                           (const double *) b->d_ev, (long long) pl->n_ev, b->h_overflow);
    HIPCHK(hipEventRecord(b->ev.pass_begin, s0));
    for (size_t c = 0; c < b->chunks.size(); c++) {
        const sa_launch_chunk &C = b->chunks[c];
        const sa_ids &Lg = C.ids[LC_GENERIC], &Ls = C.ids[LC_STRIP], &Lf = C.ids[LC_FAST];
        HIPCHK(hipEventRecord(b->chunk_ev[c].fwd_begin, s0));
        if (Lg.n) launch_fwd_generic(P, b->d_ids + Lg.off, Lg.n, s0, b->gen_threads, b->relax, b->ring_cap);
        sa_ring_lanes R(b, C.ids);
        if (P.m.hdp) {   // the emission plane of this pass's ring / strip regions, ahead of the sweeps that read it (on s0: the
                         // other lanes wait for the fork)
            if (Ls.n) launch_emit_hdp(P, b->d_ids + Ls.off, Ls.n, pl->regions[b->ids_flat[(size_t) Ls.off]].N, s0, true, false);
            for (int cl = 0; cl < 16; cl++) {
                const sa_ids &L = C.ids[LC_RING + cl];
                if (L.n)
                    launch_emit_hdp(P, b->d_ids + L.off, L.n, pl->regions[b->ids_flat[(size_t) L.off]].N, s0, true, ring_class(cl).multi);
            }
        }
        TRY(R.fork(b));
        if (Ls.n) launch_fwd_strip(P, b->d_ids + Ls.off, Ls.n, R.next(), b->d_seam, make_strip_t(P, pl->n_ev + 8, b->seam_cap, 0));
        TRY(for_each_ring_list(C.ids, [&](const sa_ids &L, int cap, bool multi) {
            return launch_fwd_ring(P, b->d_ids + L.off, L.n, R.next(), cap, multi);
        }));
        TRY(R.join(b));
        // (Round 5, measured and dropped: the pass's HDP regions in 2 / 4 / 8 slices on the two compute streams alternately, so that the
        // forward sweep of slice k runs beside the emission kernel of slice k + 1 -- neither keeps the chip busy alone --: forward
        // stage 15.8 -> 18.6 / 17.1 / 20.0 ms per 5000 reads.  A forward launch of fewer reads lasts as long as its longest chain and
        // the emission kernel slows down beside it by more than the overlap gives.)
        if (Lf.n && P.m.hdp) launch_emit_hdp(P, b->d_ids + Lf.off, Lf.n, pl->regions[b->ids_flat[(size_t) Lf.off]].N, s0, false, false);
        if (Lf.n) launch_fwd_fast(P, b->d_ids + Lf.off, Lf.n, s0, b->wide_cap);
        if (b->d_spec && C.g1 > C.g0) {   // the candidate bounds of this pass's register / ring / strip tracebacks (k_spec_match)
            const long long sa_ = b->groups[(size_t) C.g0].seg0, sb_ = b->groups[(size_t) C.g1 - 1].seg1;
            if (n_nonempty(C.ids, LC_FAST, LC_N) > 0 && sb_ > sa_)
                hipLaunchKernelGGL(k_spec_match, dim3((unsigned) (sb_ - sa_)), dim3(64), 0, s0, P, (int) sa_, (int) (sb_ - sa_), b->d_spec);
        }
        HIPCHK(hipEventRecord(b->chunk_ev[c].fwd_end, s0));
        if (C.g1 - C.g0 > 1) HIPCHK(hipStreamWaitEvent(s1, b->chunk_ev[c].fwd_end, 0));
        int submitted = C.g0, completed = C.g0;
        while (completed < C.g1) {
            for (; submitted < C.g1; submitted++) TRY(submit_group(b, P, submitted, (submitted - C.g0) & 1, finalize));
            TRY(after_group((size_t) completed++));
        }
        // the next chunk's forward sweep reuses the forward storage: both streams must be done with it
        for (int g = C.g0; g < C.g1; g++)
            if ((g - C.g0) & 1) HIPCHK(hipStreamWaitEvent(s0, b->group_ev[(size_t) g].ready, 0));
    }
    HIPCHK(hipEventRecord(b->ev.pass_end, s0));
    HIPCHK(hipGetLastError());
    return SA_OK;
}

// after the stream has drained: kernel times from the events
static int collect_times(sa_batch *b) {
    float ms_f = 0, ms_b = 0, ms_tot = 0, t = 0;
    for (size_t c = 0; c < b->chunks.size(); c++) {
        const sa_launch_chunk &C = b->chunks[c];
        HIPCHK(hipEventElapsedTime(&t, b->chunk_ev[c].fwd_begin, b->chunk_ev[c].fwd_end));
        ms_f += t;
        // backward stage of the chunk: from the end of its forward sweep to the last backward kernel's end (the
        // groups' kernels overlap on two streams; finalisation kernels of earlier groups run inside this window)
        float last = 0;
        for (int g = C.g0; g < C.g1; g++) {
            HIPCHK(hipEventElapsedTime(&t, b->chunk_ev[c].fwd_end, b->group_ev[(size_t) g].bwd_end));
            last = t > last ? t : last;
        }
        ms_b += last;
    }
    HIPCHK(hipEventElapsedTime(&ms_tot, b->ev.pass_begin, b->ev.pass_end));
    b->stats.ms_forward = ms_f;
    b->stats.ms_backward = ms_b;
    b->stats.ms_fold = ms_tot - ms_f - ms_b;  // what follows the last backward kernel: fold (+ finalisation) of the last group
    b->stats.ms_total_device = ms_tot;
    return SA_OK;
}

static int grow_after_overflow(sa_batch *b) {
    sa_plan_t *pl = b->plan;
    // a traceback segment produced more candidates than planned: enlarge and redo the pass
    sa_plan_grow_candidates(pl, 4);
    b->cand_factor = (b->cand_factor > 0 ? b->cand_factor : 1) * 4;
    cand_memo_note(pl->model, pl->params.threshold, b->device, b->cand_factor);
    // the blocks sized by candidate slots (those of them the batch has), at their bytes per slot
    const struct { void **slot; size_t bytes; } per_cand[] = {
        {(void **) &b->d_cands, sizeof(sa_cand_t)}, {(void **) &b->d_prob, 8}, {(void **) &b->d_out, sizeof(sa_pair16_t)},
        {(void **) &b->d_sortkey, 8}, {(void **) &b->d_sortidx, 4}};
    for (const auto &k : per_cand) {
        if (!*k.slot) continue;
        g_sa_pool.put(SaPool::DEVICE, *k.slot);
        *k.slot = nullptr;
        HIPCHK(g_sa_pool.get(SaPool::DEVICE, k.slot, k.bytes * (size_t) pl->n_cand, b->device));
    }
    b->cand_alloc = pl->n_cand;
    if (b->d_out) b->out_alloc = pl->n_cand;
    HIPCHK(hipMemcpy(b->d_segs, pl->segs, sizeof(sa_seg_t) * (size_t) pl->n_segs, hipMemcpyHostToDevice));
    return SA_OK;
}

// SA_SPEC_DEBUG: how far the exact totals of a traceback lie from its speculative total (expected: ~1e-3)
static int spec_debug_dump(sa_batch *b) {
    const sa_plan_t *pl = b->plan;
    const long long n_segs = pl->n_segs;
    std::vector<double> sp((size_t) n_segs), tt((size_t) at_least_1(pl->n_cks));
    HIPCHK(hipMemcpy(sp.data(), b->d_spec, 8 * (size_t) n_segs, hipMemcpyDeviceToHost));
    if (pl->n_cks) HIPCHK(hipMemcpy(tt.data(), b->d_totals, 8 * (size_t) pl->n_cks, hipMemcpyDeviceToHost));
    double worst_lo = 0, worst_hi = 0;
    long long n_spec = 0, shown = 0;
    for (long long sg = 0; sg < n_segs; sg++) {
        if (!(sp[(size_t) sg] == sp[(size_t) sg]) || !(sp[(size_t) sg] > -INFINITY)) continue;
        n_spec++;
        const sa_seg_t *S = &pl->segs[sg];
        for (int c = 0; c < S->n_ck; c++) {
            const double dlt = tt[(size_t) (S->ck_base + c)] - sp[(size_t) sg];
            if (dlt < worst_lo) worst_lo = dlt;
            if (dlt > worst_hi) worst_hi = dlt;
            if (dlt < -b->spec_slack && shown < 6) {
                shown++;
                fprintf(stderr, "[spec] segment %lld (region %d, start %lld from %lld to %lld at_end %d) checkpoint %d of %d: total %.6f spec %.6f\n",
                        sg, S->region, (long long) S->start, (long long) S->from, (long long) S->to, S->at_end, c, S->n_ck,
                        tt[(size_t) (S->ck_base + c)], sp[(size_t) sg]);
            }
        }
    }
    fprintf(stderr, "[spec] %lld segments with a speculative total; exact total - speculative total in [%.3e, %.3e]; slack %.3g\n",
            n_spec, worst_lo, worst_hi, b->spec_slack);
    return SA_OK;
}

// After a pass has been queued: waits for it, takes its times and looks at what its kernels raised.  *again: the pass has to be
// repeated (more candidate slots, or a lower candidate bound).  `finalized`: k_finalize ran and the pairs travel on the pair stream
// (trace_t0: SA_TRACE, the run's start), else host finalisation follows.  The groups' lanes only: the others were joined to lane 0.
static int after_pass(sa_batch *b, bool finalized, const double *trace_t0, bool piped, bool *again) {
    const sa_plan_t *pl = b->plan;
    HIPCHK(sa_sync_stream(b->lanes.compute[1], b->device));
    HIPCHK(sa_sync_stream(b->lanes.compute[0], b->device));
    if (finalized) {
        if (trace_t0) fprintf(stderr, "[trace] compute stream drained at %.3f ms\n", now_ms() - *trace_t0);
        HIPCHK(sa_sync_stream(b->lanes.pair, b->device));
        if (trace_t0) fprintf(stderr, "[trace] copies drained at %.3f ms (piped %d)\n", now_ms() - *trace_t0, (int) piped);
    }
    TRY(collect_times(b));
    if (finalized && b->d_spec && getenv("SA_SPEC_DEBUG")) TRY(spec_debug_dump(b));
    if (b->h_overflow[2]) {   // (k_check_events / k_spec_match)
        if (finalized) fprintf(stderr, "[signalalign_hip] an event mean (or a model entry: a traceback's forward values) is not a finite number: no result\n");
        return SA_EINVAL;
    }
    *again = true;
    if (finalized && b->h_overflow[1] && b->d_spec) {
        // a traceback's exact totals fell below its speculative total minus the slack (not seen with the default slack: the
        // totals of one traceback agree to ~1e-2, the flat HDP fixture's to 0.15; tests/test_gpu_parity.py forces it with
        // SA_TEST_SPEC_SLACK): its candidates may be incomplete -- the pass is repeated with a bound far lower (more candidates,
        // same survivors): x4, then x256 more, and if that is not enough with no bound at all (slack +inf: every posterior
        // cell-path is a candidate and k_finalize's check cannot fire again) -- never accepted as it is
        if (std::isinf(b->spec_slack)) return SA_ESTATE;   // (cannot happen: with an infinite slack the flag is never raised)
        b->spec_repeats++;
        b->spec_slack = b->spec_repeats == 1 ? b->spec_slack * 4.0 : (b->spec_repeats == 2 ? b->spec_slack * 256.0 : (double) INFINITY);
        if (!getenv("SA_TEST_SPEC_SLACK")) spec_memo_note(pl->model, b->device, b->spec_slack);
        fprintf(stderr, "[signalalign_hip] a speculative candidate bound was too high; repeating the pass with slack %g\n", b->spec_slack);
        return SA_OK;
    }
    if (b->h_overflow[0]) return grow_after_overflow(b);
    *again = false;
    return SA_OK;
}

// kernels only (host finalisation follows): SA_FLAG_EXACT and the expectation pass
static int run_passes(sa_batch_t *b) {
    bool again = true;
    for (int attempt = 0; attempt < 6 && again; attempt++) {
        TRY(enqueue_pass(b, false, [](size_t) { return (int) SA_OK; }));
        TRY(after_pass(b, false, nullptr, false, &again));
    }
    return again ? SA_ENOMEM : SA_OK;
}

// the pinned result block: room for `total` records
static int reserve_pairs(sa_batch *b, long long total) {
    if (total > b->h_pairs_cap) {
        g_sa_pool.put(SaPool::PINNED, b->h_pairs);
        b->h_pairs = nullptr;
        const long long cap = pairs_block_cap(total);
        HIPCHK(g_sa_pool.get(SaPool::PINNED, (void **) &b->h_pairs, b->rec() * (size_t) cap, b->device));
        b->h_pairs_cap = cap;
    }
    return SA_OK;
}

// SA_FLAG_EXACT: the kernels, then finalisation on the host with the C library's exp(): bit-identical to the reference's
// posterior arithmetic
static int run_exact(sa_batch *b) {
    sa_plan_t *pl = b->plan;
    TRY(run_passes(b));
    std::vector<sa_cand_t> cands((size_t) at_least_1(pl->n_cand));
    std::vector<int> counts((size_t) at_least_1(pl->n_segs));
    std::vector<double> totals((size_t) at_least_1(pl->n_cks));
    if (pl->n_cand) HIPCHK(hipMemcpy(cands.data(), b->d_cands, sizeof(sa_cand_t) * (size_t) pl->n_cand, hipMemcpyDeviceToHost));
    if (pl->n_segs) HIPCHK(hipMemcpy(counts.data(), b->d_cand_count, 4 * (size_t) pl->n_segs, hipMemcpyDeviceToHost));
    if (pl->n_cks) HIPCHK(hipMemcpy(totals.data(), b->d_totals, 8 * (size_t) pl->n_cks, hipMemcpyDeviceToHost));
    std::vector<sa_pair_t *> pp((size_t) at_least_1(pl->n_jobs), nullptr);
    std::vector<int64_t> np((size_t) at_least_1(pl->n_jobs), 0);
    TRY(sa_plan_finalize(pl, cands.data(), counts.data(), totals.data(), pp.data(), np.data()));
    if (!b->h_vc_bits.empty()) {   // SA_FLAG_VC_ROWS on host-finalised pairs: the same test as k_finalize's
        b->job_all_n.assign((size_t) pl->n_jobs, 0);
        b->job_all_sum.assign((size_t) pl->n_jobs, 0);
        for (long long j = 0; j < pl->n_jobs; j++) {
            const long long base = b->h_vc_off[(size_t) j];
            int64_t kept = 0;
            for (int64_t q = 0; q < np[j]; q++) {
                b->job_all_n[(size_t) j]++;
                b->job_all_sum[(size_t) j] += pp[j][q].prob_e7;
                const long long bit = base + pp[j][q].x;
                if ((b->h_vc_bits[(size_t) (bit >> 6)] >> (bit & 63)) & 1ull) pp[j][kept++] = pp[j][q];
            }
            np[j] = kept;
        }
    }
    long long total = 0;
    for (long long j = 0; j < pl->n_jobs; j++) total += np[j];
    TRY(reserve_pairs(b, total));
    total = 0;
    for (long long j = 0; j < pl->n_jobs; j++) {
        b->job_off[j] = total;
        for (int64_t q = 0; q < np[j]; q++) {
            if (b->p8) reinterpret_cast<sa_pair8_t *>(b->h_pairs)[total + q] = sa_pair8_pack(pp[j][q].prob_e7, pp[j][q].x, pp[j][q].y);
            else b->h_pairs[total + q] = sa_pair16_pack(pp[j][q].prob_e7, pp[j][q].x, pp[j][q].y, pp[j][q].path, pp[j][q].kmer_id);
        }
        total += np[j];
        free(pp[j]);
    }
    b->job_off[pl->n_jobs] = total;
    b->n_pairs_total = total;
    b->job_dev_off.clear();
    return SA_OK;
}

// default: finalisation on the device, group after group; the pairs of group g travel to the pinned host buffer on the pair
// stream while the kernels of group g+1 run.  gbase[g]: where group g's pairs start in it, gbase[n groups]: all pairs.
static int run_device_finalized(sa_batch *b, std::vector<long long> &gbase) {
    sa_plan_t *pl = b->plan;
    const size_t ng = b->groups.size();
    const bool trace = getenv("SA_TRACE") != nullptr;
    bool again = true;
    for (int attempt = 0; attempt < 6 && again; attempt++) {
        const double t0 = now_ms();
        bool piped = true;
        long long running = 0;
        auto after_group = [&](size_t g) -> int {
            const sa_launch_group &G = b->groups[g];
            HIPCHK(hipEventSynchronize(b->group_ev[g].ready));
            long long tg = b->h_seg_off[G.seg0 + g + (G.seg1 - G.seg0)];
            if (trace) fprintf(stderr, "[trace] group %zu ready at %.3f ms, %lld pairs\n", g, now_ms() - t0, tg);
            gbase[g] = running;
            if (piped && running + tg <= b->h_pairs_cap) {
                if (tg > 0)
                    HIPCHK(hipMemcpyAsync(b->host_at(running), b->out_at(pl->segs[G.seg0].cand_off),
                                          b->rec() * (size_t) tg, hipMemcpyDeviceToHost, b->lanes.pair));
            } else {
                piped = false;  // first run (or a larger result than last time): size the pinned buffer afterwards
            }
            running += tg;
            return SA_OK;
        };
        TRY(enqueue_pass(b, true, after_group));
        gbase[ng] = running;
        TRY(after_pass(b, true, trace ? &t0 : nullptr, piped, &again));
        if (again || piped) continue;
        TRY(reserve_pairs(b, running));
        for (size_t g = 0; g < ng; g++) {
            const sa_launch_group &G = b->groups[g];
            long long tg = gbase[g + 1] - gbase[g];
            if (tg > 0)
                HIPCHK(hipMemcpyAsync(b->host_at(gbase[g]), b->out_at(pl->segs[G.seg0].cand_off),
                                      b->rec() * (size_t) tg, hipMemcpyDeviceToHost, b->lanes.pair));
        }
        HIPCHK(sa_sync_stream(b->lanes.pair, b->device));
    }
    return again ? SA_ENOMEM : SA_OK;
}

// job offsets after device finalisation: a job's pairs start where its first segment's do
static void index_jobs(sa_batch *b, const std::vector<long long> &gbase) {
    const sa_plan_t *pl = b->plan;
    const size_t ng = b->groups.size();
    std::vector<int> seg_group((size_t) at_least_1(pl->n_segs), 0);
    for (size_t g = 0; g < ng; g++)
        for (long long sg = b->groups[g].seg0; sg < b->groups[g].seg1; sg++) seg_group[sg] = (int) g;
    long long next = gbase[ng];
    b->job_dev_off.assign((size_t) pl->n_jobs, 0);
    for (long long j = pl->n_jobs - 1; j >= 0; j--) {
        const sa_jobinfo_t *J = &pl->jobs[j];
        long long first_seg = -1;
        for (long long r = J->region_off; r < J->region_off + J->n_regions && first_seg < 0; r++)
            if (pl->regions[r].n_seg > 0) first_seg = pl->regions[r].seg_off;
        if (first_seg >= 0) {
            int g = seg_group[first_seg];
            next = gbase[g] + b->h_seg_off[first_seg + g];
            // the group's pairs sit in d_out from its first segment's candidate slot on
            b->job_dev_off[j] = pl->segs[b->groups[g].seg0].cand_off + b->h_seg_off[first_seg + g];
        }
        b->job_off[j] = next;  // jobs without segments are empty ranges in front of the next job
    }
    b->job_off[pl->n_jobs] = gbase[ng];
    b->n_pairs_total = gbase[ng];
}

// SA_FLAG_VC_ROWS after device finalisation: what the dropped rows would have added to a job's count and score
static int vc_row_totals(sa_batch *b) {
    const sa_plan_t *pl = b->plan;
    const long long n_segs = pl->n_segs;
    std::vector<long long> sa_((size_t) (2 * at_least_1(n_segs)), 0);
    if (n_segs) HIPCHK(hipMemcpy(sa_.data(), b->d_seg_all, sizeof(long long) * 2 * (size_t) n_segs, hipMemcpyDeviceToHost));
    b->job_all_n.assign((size_t) pl->n_jobs, 0);
    b->job_all_sum.assign((size_t) pl->n_jobs, 0);
    for (long long sg = 0; sg < n_segs; sg++) {
        const long long j = pl->regions[pl->segs[sg].region].job;
        b->job_all_n[(size_t) j] += sa_[(size_t) (2 * sg)];
        b->job_all_sum[(size_t) j] += sa_[(size_t) (2 * sg + 1)];
    }
    return SA_OK;
}

static int batch_run_body(sa_batch_t *b) {
    if (b->expect) return SA_ESTATE;
    HIPCHK(hipSetDevice(b->device));
    sa_plan_t *pl = b->plan;
    b->n_pairs_total = 0;
    b->job_off.assign((size_t) pl->n_jobs + 1, 0);
    if (b->flags & SA_FLAG_EXACT) {
        TRY(run_exact(b));
        b->ran = true;
        return SA_OK;
    }
    // A first estimate of the result size (measured: 0.9 pairs per event at the default threshold) lets even the FIRST run
    // of a batch overlap its copies with the kernels; with the caching allocator the buffer is a reused block.  If the
    // estimate is short the run falls back to copying afterwards, as before.
    // (an estimate: when the pinned block cannot be had at that size the run copies after its kernels, exactly as with no estimate)
    if (b->h_pairs_cap == 0 && pl->params.threshold >= 0.005 && reserve_pairs(b, expected_pairs(b)) != SA_OK) {
        (void) hipGetLastError();
        b->h_pairs = nullptr;
        b->h_pairs_cap = 0;
    }
    std::vector<long long> gbase(b->groups.size() + 1, 0);
    TRY(run_device_finalized(b, gbase));
    index_jobs(b, gbase);
    if (b->d_seg_all) TRY(vc_row_totals(b));
    g_pairs_memo.note(pl->model->uid, b->device, pl->params.threshold, (double) b->n_pairs_total, (double) pl->n_ev);
    b->ran = true;
    return SA_OK;
}

int sa_batch_run(sa_batch_t *b) {
    if (!b) return SA_EINVAL;
    if (b->released) return SA_ESTATE;   // (sa_batch_release_device: nothing left to run on)
    { const int rcf = batch_finish(b); if (rcf) return rcf; }   // (a deferred batch: the second half of its creation)
    b->quiet = false;
    const int rc = batch_run_body(b);
    b->quiet = rc == SA_OK;
    return rc;
}

// The records of a finished batch for a step chained onto it (sa_chain.h): where the run left them in d_out, or -- after host
// finalisation (SA_FLAG_EXACT) or sa_batch_release_device -- uploaded again from h_pairs into d_pairs_up.
int sa_batch_view(sa_batch_t *b, SaBatchView *v) {
    if (!b || !v) return SA_EINVAL;
    v->p8 = b->p8;
    v->batch_flags = b->flags;
    v->device = b->device;
    v->k = b->c_k;
    v->n_alpha = b->c_n_alpha;
    if (!b->ran) return SA_ESTATE;
    const sa_plan_t *pl = b->plan;
    const size_t nj = (size_t) pl->n_jobs;
    const bool resident = b->job_dev_off.size() == nj && !b->released;
    v->first.assign(nj, 0); v->count.assign(nj, 0); v->n_events.assign(nj, 0);
    for (size_t j = 0; j < nj; j++) {
        v->first[j] = resident ? b->job_dev_off[j] : b->job_off[j];
        v->count[j] = b->job_off[j + 1] - b->job_off[j];
        v->n_events[j] = pl->jobs[j].n_events;
    }
    HIPCHK(hipSetDevice(b->device));
    if (resident) { v->recs = b->d_out; return SA_OK; }
    const size_t bytes = b->rec() * (size_t) b->n_pairs_total;
    if (bytes > b->d_pairs_up_cap) {
        g_sa_pool.put(SaPool::DEVICE, b->d_pairs_up);
        b->d_pairs_up = nullptr; b->d_pairs_up_cap = 0;
        HIPCHK(g_sa_pool.get(SaPool::DEVICE, &b->d_pairs_up, bytes, b->device));
        b->d_pairs_up_cap = bytes;
    }
    if (bytes) HIPCHK(hipMemcpy(b->d_pairs_up, b->h_pairs, bytes, hipMemcpyHostToDevice));
    v->recs = b->d_pairs_up;
    return SA_OK;
}

int sa_batch_ambig(sa_batch_t *b, int which, SaAmbigTab **tab, int64_t *n_jobs) {
    if (!b || !tab || !n_jobs || which < 0 || which >= SA_TAB_N) return SA_EINVAL;
    if (!b->ambig_tab[which] || !b->ran) return SA_ESTATE;
    *tab = b->ambig_tab[which];
    *n_jobs = b->c_n;
    return SA_OK;
}

// sa_batch_run on a thread of the library's own, so that the caller can plan the next batch (sa_batch_create is host
// work) while this one is on the GPU; sa_batch_wait joins it and returns sa_batch_run's code.
int sa_batch_prepare(sa_batch_t *b) {
    if (!b) return SA_EINVAL;
    std::lock_guard<std::mutex> g(b->fin_mu);
    if (!b->finished && !b->prepared) {
        b->prepare_rc = batch_prepare_body(b);
        b->prepared = true;
    }
    return b->prepare_rc;
}
// Returns a finished batch's working storage in HBM (forward planes, candidate and result slots, plan arrays, seams: everything
// sa_batch_stats_t.device_bytes counts) to the caching allocator and keeps what the caller reads: the packed pairs in pinned host
// memory, the per-job offsets, the statistics.  For a caller that holds batches for their RESULTS while it creates further ones
// (signalMachine --twoD: the template batch while the complement batch runs; a render thread formatting the previous slice): the
// next batch then plans into the whole card.  Afterwards sa_batch_run / sa_batch_start return SA_ESTATE; sa_batch_mea still works
// (the pairs go up again, as after SA_FLAG_EXACT).
int sa_batch_release_device(sa_batch_t *b) {
    if (!b) return SA_EINVAL;
    if (!b->ran || b->runner) return SA_ESTATE;   // (between sa_batch_start and sa_batch_wait: the run is still using it)
    if (b->released) return SA_OK;
    if (hipSetDevice(b->device) != hipSuccess) return SA_ENODEVICE;
    HIPCHK(b->lanes.drain(b->device, false));   // (a finished run has drained them; a failed one may not have)
    b->put_blocks(0, sa_batch::BLK_END);
    if (b->held_stage) { g_sa_pool.put(SaPool::PINNED, b->held_stage); b->held_stage = nullptr; }
    for (SaAmbigTab *tab : b->ambig_tab) sa_ambig_release_device(tab);
    b->released = true;
    return SA_OK;
}

int sa_batch_start(sa_batch_t *b) {
    if (!b) return SA_EINVAL;
    if (b->runner || b->released) return SA_ESTATE;   // (sa_batch_release_device: nothing left to run on)
    b->runner_rc = SA_OK;
    g_batches_started.fetch_add(1);
    b->runner = new (std::nothrow) std::thread([b]() { b->runner_rc = sa_batch_run(b); });
    if (!b->runner) g_batches_started.fetch_sub(1);
    return b->runner ? SA_OK : SA_ENOMEM;
}
int sa_batch_wait(sa_batch_t *b) {
    if (!b) return SA_EINVAL;
    if (!b->runner) return SA_ESTATE;
    b->runner->join();
    delete b->runner;
    b->runner = nullptr;
    g_batches_started.fetch_sub(1);
    return b->runner_rc;
}

int sa_batch_n_pairs(const sa_batch_t *b, int64_t job, int64_t *n) {
    if (!b || !n || job < 0 || job >= b->c_n) return SA_EINVAL;
    if (!b->ran) return SA_ESTATE;
    *n = b->job_off[job + 1] - b->job_off[job];
    return SA_OK;
}
int sa_batch_all_pairs_summary(const sa_batch_t *b, int64_t job, int64_t *n_all, int64_t *sum_prob_e7) {
    if (!b || job < 0 || job >= b->c_n) return SA_EINVAL;
    if (!b->ran) return SA_ESTATE;
    if (b->job_all_n.size() == (size_t) b->c_n) {   // SA_FLAG_VC_ROWS: counted before the rows were dropped
        if (n_all) *n_all = b->job_all_n[(size_t) job];
        if (sum_prob_e7) *sum_prob_e7 = b->job_all_sum[(size_t) job];
        return SA_OK;
    }
    long long s = 0;
    for (long long i = b->job_off[job]; i < b->job_off[job + 1]; i++)
        s += b->p8 ? (long long) (reinterpret_cast<const sa_pair8_t *>(b->h_pairs)[i] >> 40) : (long long) ((b->h_pairs[i].b >> 32) & 0xffffffull);
    if (n_all) *n_all = b->job_off[job + 1] - b->job_off[job];
    if (sum_prob_e7) *sum_prob_e7 = s;
    return SA_OK;
}
int sa_batch_pairs8(const sa_batch_t *b, int64_t job, const sa_pair8_t **out, int64_t *n) {
    if (!b || !out || !n || job < 0 || job >= b->c_n) return SA_EINVAL;
    if (!b->ran || !b->p8) return SA_ESTATE;
    *out = reinterpret_cast<const sa_pair8_t *>(b->h_pairs) + b->job_off[job];
    *n = b->job_off[job + 1] - b->job_off[job];
    return SA_OK;
}
int sa_batch_pairs8_all(const sa_batch_t *b, const sa_pair8_t **out, int64_t *first) {
    if (!b || !out) return SA_EINVAL;
    if (!b->ran || !b->p8) return SA_ESTATE;
    *out = reinterpret_cast<const sa_pair8_t *>(b->h_pairs);
    if (first)
        for (int64_t j = 0; j <= b->c_n; j++) first[j] = b->job_off[(size_t) j];
    return SA_OK;
}
int sa_batch_pairs(const sa_batch_t *b, int64_t job, sa_pair_t *out, int64_t cap) {
    if (!b || job < 0 || job >= b->c_n) return SA_EINVAL;
    if (!b->ran || b->p8) return SA_ESTATE;
    long long n = b->job_off[job + 1] - b->job_off[job];
    if (n > cap) return SA_EINVAL;
    const sa_pair16_t *src = b->h_pairs + b->job_off[job];
    for (long long i = 0; i < n; i++) out[i] = sa_pair16_unpack(src[i]);
    return SA_OK;
}
int sa_batch_pairs16(const sa_batch_t *b, int64_t job, const sa_pair16_t **out, int64_t *n) {
    if (!b || !out || !n || job < 0 || job >= b->c_n) return SA_EINVAL;
    if (!b->ran || b->p8) return SA_ESTATE;
    *n = b->job_off[job + 1] - b->job_off[job];
    *out = b->h_pairs + b->job_off[job];
    return SA_OK;
}
int sa_batch_pairs16_all(const sa_batch_t *b, const sa_pair16_t **out, int64_t *first) {
    if (!b || !out) return SA_EINVAL;
    if (!b->ran || b->p8) return SA_ESTATE;
    *out = b->h_pairs;
    if (first)
        for (long long j = 0; j <= (long long) b->c_n; j++) first[j] = b->job_off[(size_t) j];
    return SA_OK;
}
int sa_batch_pairs_all(const sa_batch_t *b, sa_pair_t *out, int64_t cap, int64_t *first) {
    if (!b || (!out && cap > 0)) return SA_EINVAL;
    if (!b->ran || b->p8) return SA_ESTATE;
    const long long nj = b->c_n, total = b->n_pairs_total;
    if (first)
        for (long long j = 0; j <= nj; j++) first[j] = b->job_off[(size_t) j];
    if (total > cap) return SA_EINVAL;
    // the records are contiguous in job order: equal slices to the host threads (9 million pairs per headline batch, 143 MB read
    // and 215 MB written -- a memory-bound loop, first touch of the caller's buffer included)
    const sa_pair16_t *src = b->h_pairs;
    const size_t piece = 1 << 16, np_ = ((size_t) total + piece - 1) / piece;
    sa_parallel_for(np_, [&](size_t q) {
        const size_t i0 = q * piece, i1 = i0 + piece < (size_t) total ? i0 + piece : (size_t) total;
        for (size_t i = i0; i < i1; i++) out[i] = sa_pair16_unpack(src[i]);
    });
    return SA_OK;
}
int sa_batch_stats(const sa_batch_t *b, sa_batch_stats_t *out) {
    if (!b || !out) return SA_EINVAL;
    { const int rcf = batch_finish(const_cast<sa_batch_t *>(b)); if (rcf) return rcf; }
    *out = b->stats;
    return SA_OK;
}
int sa_batch_job_cells(const sa_batch_t *b, int64_t job, double *cf, double *cb) {
    if (!b || job < 0 || job >= b->c_n) return SA_EINVAL;
    { const int rcf = batch_finish(const_cast<sa_batch_t *>(b)); if (rcf) return rcf; }
    if (cf) *cf = b->plan->jobs[job].cells_fwd;
    if (cb) *cb = b->plan->jobs[job].cells_bwd;
    return SA_OK;
}

int sa_align_batch(const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs, int64_t n_jobs,
                   const char *const *ambig, int device, unsigned flags, sa_pair_t **pairs_out, int64_t *n_pairs_out) {
    sa_batch_t *b = nullptr;
    int rc = sa_batch_create(&b, m, p, jobs, n_jobs, ambig, device, flags);
    if (rc) return rc;
    rc = sa_batch_run(b);
    if (rc == SA_OK)
        for (int64_t j = 0; j < n_jobs; j++) {
            int64_t n = 0;
            sa_batch_n_pairs(b, j, &n);
            pairs_out[j] = (sa_pair_t *) malloc(sizeof(sa_pair_t) * (size_t) at_least_1(n));
            if (!pairs_out[j]) { rc = SA_ENOMEM; break; }
            sa_batch_pairs(b, j, pairs_out[j], n);
            n_pairs_out[j] = n;
        }
    sa_batch_destroy(b);
    return rc;
}

// getExpectationsUsingAnchors for a batch of reads.  The pass runs on the memory-resident kernels (every region is
// planned SA_KIND_GENERIC); the per-group sums are rescaled here with the exact totals of the fold kernel.
static thread_local sa_batch_stats_t tl_expect_stats;   // of this thread's last sa_expect_batch (sa_expect_last_stats)
int sa_expect_last_stats(sa_batch_stats_t *out) {
    if (!out) return SA_EINVAL;
    *out = tl_expect_stats;
    return SA_OK;
}
int sa_expect_batch(const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs, int64_t n_jobs,
                    const char *const *ambig, int device, unsigned flags, double *trans9_out, double *likelihood_out,
                    sa_assignment_t **assign_out, int64_t *n_assign_out) {
    if (!trans9_out || !likelihood_out) return SA_EINVAL;
    sa_batch_t *b = nullptr;
    // regions with one path per cell take the register kernels' expectation variant (k_bwd_fast_expect, sa_fast.inc); several
    // paths per cell, SA_FLAG_EXACT or SA_FLAG_FORCE_GENERIC: the memory-resident kernels (the checker of the former)
    if (m && m->emission != 0) flags |= SA_FLAG_FORCE_GENERIC;
    int rc = sa_batch_create(&b, m, p, jobs, n_jobs, ambig, device, flags | SA_FLAG_EXPECT_INTERNAL);
    if (rc) return rc;
    rc = run_passes(b);
    if (rc) { sa_batch_destroy(b); return rc; }
    const sa_plan_t *pl = b->plan;
    tl_expect_stats = b->stats;
    // The per-read sums are taken on the device (k_expect_reduce): 8 doubles per read come back.  HDP models also return the
    // assignment candidates (24 B x slots per posterior diagonal) with the totals they are tested against -- into ONE pinned
    // block (a copy to pageable memory moves 3 GB/s), tested on all host threads.
    const bool want_cands = m->hdp != nullptr && assign_out != nullptr;
    const size_t n_ck = (size_t) at_least_1(pl->n_cks), n_sg = (size_t) at_least_1(pl->n_segs);
    const size_t o_red = 0, o_tot = o_red + sa_up256(64 * (size_t) at_least_1(n_jobs));
    const size_t o_cnt = o_tot + (want_cands ? sa_up256(8 * n_ck) : 0);
    const size_t o_cand = o_cnt + (want_cands ? sa_up256(4 * n_sg) : 0);
    const size_t host_bytes = o_cand + (want_cands ? sizeof(sa_cand_t) * (size_t) at_least_1(pl->n_cand) : 256);
    char *hb = nullptr;
    double *d_red = nullptr;
    if (g_sa_pool.get(SaPool::PINNED, (void **) &hb, host_bytes, b->device) != hipSuccess) { (void) hipGetLastError(); sa_batch_destroy(b); return SA_ENOMEM; }
    if (g_sa_pool.get(SaPool::DEVICE, (void **) &d_red, 64 * (size_t) at_least_1(n_jobs), b->device) != hipSuccess) {
        (void) hipGetLastError();
        g_sa_pool.put(SaPool::PINNED, hb);
        sa_batch_destroy(b);
        return SA_ENOMEM;
    }
    auto dl = [&](void *dst, const void *src, size_t bytes) -> int {
        if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, b->lanes.compute[0]));
        return SA_OK;
    };
    auto tail = [&]() -> int {
        HIPCHK(hipMemsetAsync(d_red, 0, 64 * (size_t) at_least_1(n_jobs), b->lanes.compute[0]));
        if (pl->n_regions > 0) {
            hipLaunchKernelGGL(k_expect_reduce, dim3((unsigned) pl->n_regions), dim3(64), 0, b->lanes.compute[0], make_devplan(b), d_red,
                               (int) pl->n_regions);
            HIPCHK(hipGetLastError());
        }
        int rc_ = dl(hb + o_red, d_red, 64 * (size_t) n_jobs);
        if (!rc_ && want_cands) rc_ = dl(hb + o_tot, b->d_totals, 8 * (size_t) pl->n_cks);
        if (!rc_ && want_cands) rc_ = dl(hb + o_cnt, b->d_cand_count, 4 * (size_t) pl->n_segs);
        if (!rc_ && want_cands) rc_ = dl(hb + o_cand, b->d_cands, sizeof(sa_cand_t) * (size_t) pl->n_cand);
        if (!rc_ && sa_sync_stream(b->lanes.compute[0], b->device) != hipSuccess) rc_ = SA_ENODEVICE;
        return rc_;
    };
    rc = tail();
    g_sa_pool.put(SaPool::DEVICE, d_red);
    if (rc) { g_sa_pool.put(SaPool::PINNED, hb); sa_batch_destroy(b); return rc; }
    const double *red = reinterpret_cast<const double *>(hb + o_red), *totals = reinterpret_cast<const double *>(hb + o_tot);
    const int *counts = reinterpret_cast<const int *>(hb + o_cnt);
    const sa_cand_t *cands = reinterpret_cast<const sa_cand_t *>(hb + o_cand);
    // (from, to) slots of hmm->transitions[from * 3 + to] in the order the kernels accumulate them
    static const int slot[7] = {0 * 3 + 1, 1 * 3 + 1, 0 * 3 + 0, 1 * 3 + 0, 2 * 3 + 0, 0 * 3 + 2, 2 * 3 + 2};
    const double thr = pl->params.threshold;
    std::atomic<int> oom(0);
    sa_parallel_for((size_t) n_jobs, [&](size_t jj) {
        const int64_t j = (int64_t) jj;
        const sa_jobinfo_t *J = &pl->jobs[j];
        for (int k = 0; k < 7; k++) trans9_out[j * 9 + slot[k]] += red[8 * j + k];
        likelihood_out[j] += red[8 * j + 7];
        std::vector<sa_assignment_t> as;
        for (long long r = J->region_off; want_cands && r < J->region_off + J->n_regions; r++) {
            const sa_region_t *R = &pl->regions[r];
            for (long long sg = R->seg_off; sg < R->seg_off + R->n_seg; sg++) {
                const sa_seg_t *S = &pl->segs[sg];
                for (int i = 0; i < counts[sg]; i++) {
                    const sa_cand_t &cd = cands[S->cand_off + i];
                    long long e = (long long) cd.x + cd.y + 2;
                    double total = totals[S->ck_base + (S->from - e) / SA_CKPT_EVERY];
                    if (exp(cd.fb - total) >= thr) {
                        sa_assignment_t a;
                        a.ref_pos = cd.x + R->x1;
                        a.event = cd.y + R->y1;
                        as.push_back(a);
                    }
                }
            }
        }
        if (assign_out) {
            assign_out[j] = (sa_assignment_t *) malloc(sizeof(sa_assignment_t) * (as.size() ? as.size() : 1));
            if (!assign_out[j]) { oom.store(1); return; }
            if (!as.empty()) memcpy(assign_out[j], as.data(), sizeof(sa_assignment_t) * as.size());
            if (n_assign_out) n_assign_out[j] = (int64_t) as.size();
        }
    });
    g_sa_pool.put(SaPool::PINNED, hb);
    if (oom.load()) { sa_batch_destroy(b); return SA_ENOMEM; }
    sa_batch_destroy(b);
    return SA_OK;
}

int sa_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sa_device_check(int device, bool quiet) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void) hipGetLastError();
        if (!quiet) fprintf(stderr, SA_NO_DEVICE_LINE);
        return SA_ENODEVICE;
    }
    return device < 0 || device >= n ? SA_EINVAL : SA_OK;
}

int sa_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes) {
    if (const int rc = sa_device_check(device, /* quiet */ true)) return rc;
    HIPCHK(hipSetDevice(device));
    size_t f = 0, t = 0;
    HIPCHK(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (int64_t) (f + g_sa_pool.idle_bytes(SaPool::DEVICE, device));   // what the caching allocator holds is available
    if (total_bytes) *total_bytes = (int64_t) t;
    return SA_OK;
}
