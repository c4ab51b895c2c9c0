// sa_detect.hip -- event detection from raw current on the GPU, and the raw-to-event-map chain (load_from_raw2).
//
// What it replaces: detect_events (impl/event_detection.c:268-330, Scrappie's t-statistic detector) as load_from_raw2
// (impl/eventAligner.c:1242-1300) calls it, then reverse_events, estimate_scalings_using_mom, the adaptive banded
// event aligner and the base-to-event map.  The last three are the existing sa_scalings_mom / sa_event_align_batch
// (sa_ea.hip): one event-alignment code path.
//
// Bit parity.  Every stage follows the reference's operations and casts (the file is compiled with -ffp-contract=off,
// correctly rounded f32 division and square root, f32 denormals on):
//   raw to pA       float: unit = range / digitisation, pA = (raw + offset) * unit
//   prefix sums     double, sum[i+1] = sum[i] + x[i], sumsq[i+1] = sumsq[i] + (double)(x[i] * x[i]) with a FLOAT square.
//                   A left-to-right fold: sumsq reaches ~2^38 with float-spaced terms, past 53 bits, so a parallel scan
//                   (another association) is not bit-identical.  One lane per read runs the fold.
//   t-statistics    compute_tstat (:58-115): double window sums, float sum2 / sumsq2, float means, combined_var built in
//                   double and stored as float, clamped to FLT_MIN; fabs and sqrt in DOUBLE as the C library's are (the
//                   HIP float overloads would round differently).  Parallel over samples.
//   peak detector   short_long_peak_detector (:122-205): serial state machine, one lane per read; masked_to starts at 0
//                   and compares as size_t (sample 0 is never examined), window halving is integer.
//   events          create_events / create_event (:207-266): float length, mean = (float) dsum / length, var in float,
//                   stdv = sqrtf(fmaxf(var, 0)).  Per-read offsets from a device scan of the peak counts.
// Departures from undefined behaviour: a read with no peak is one event [0, n) (the reference reads peaks[-1]); an
// empty read is SA_EINVAL.  No trimming: trim_and_segment_raw's result is discarded by every caller in the reference.
//
// Mapping: k_det_prefix and k_det_peaks run one lane per read (64 reads per wave), each lane streaming its own read
// with 16-byte loads; k_det_tstat is one thread per sample (both windows), k_det_events one block per read.
//
// sa_npread_from_raw_batch goes on from the detector's rows on the device to the in-memory .npRead of a 1D read: the same
// MoM scalings and event aligner, then k_raw_finish (one wave per read: the base-to-event map, the compaction to mapped rows,
// the table's seconds); p_model_state and make_event_map on the host ("Reads from raw current").
#include <hip/hip_runtime.h>

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "sa_scratch.h"

struct DetJob {
    long long raw_off;   // samples (int16) into the raw image, a multiple of 8; also the offset of t1 / t2 / peaks
    long long ps_off;    // into sum / sumsq (n + 1 entries per read)
    int n;
    float digitisation, offset, range;
};

struct DetEvent {        // event_t's fields the table needs
    int start;
    float length, mean, stdv;
};

#define DET_LANES 64

// sum / sumsq of the pA values, one lane per read: 8 samples per 16-byte load, the next load in flight meanwhile
__global__ __launch_bounds__(DET_LANES) void k_det_prefix(const DetJob *__restrict__ jobs, int n_jobs, const int16_t *__restrict__ raw,
                                                          double *__restrict__ S, double *__restrict__ Q) {
    const int r = blockIdx.x * DET_LANES + threadIdx.x;
    if (r >= n_jobs) return;
    const DetJob J = jobs[r];
    const uint4 *src = (const uint4 *) (raw + J.raw_off);
    double *s = S + J.ps_off, *q = Q + J.ps_off;
    const float unit = J.range / J.digitisation, off = J.offset;
    double a = 0.0, b = 0.0;
    s[0] = 0.0;
    q[0] = 0.0;
    const int n = J.n, n_chunks = (n + 7) / 8;
    uint4 nxt = src[0];
    for (int c = 0; c < n_chunks; c++) {
        const uint4 cur = nxt;
        if (c + 1 < n_chunks) nxt = src[c + 1];
        const unsigned w[4] = {cur.x, cur.y, cur.z, cur.w};
        const int base = 8 * c;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (base + k < n) {
                const int16_t v = (int16_t) ((w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
                const float x = ((float) v + off) * unit;
                a = a + (double) x;
                b = b + (double) (x * x);
                s[base + k + 1] = a;
                q[base + k + 1] = b;
            }
        }
    }
}

// compute_tstat for one window at sample i (d_length n, w_length w)
__device__ __forceinline__ float det_tstat(const double *s, const double *q, int n, int w, int i) {
    if (n < 2 * w || w < 2) return 0.0f;
    if (i < w || i > n - w) return 0.0f;
    double sum1 = s[i], sumsq1 = q[i];
    if (i > w) {
        sum1 -= s[i - w];
        sumsq1 -= q[i - w];
    }
    const float sum2 = (float) (s[i + w] - s[i]);
    const float sumsq2 = (float) (q[i + w] - q[i]);
    const float wf = (float) w;
    const float mean1 = (float) (sum1 / (double) wf);
    const float mean2 = sum2 / wf;
    float cv = (float) (sumsq1 / (double) wf - (double) (mean1 * mean1) + (double) (sumsq2 / wf) - (double) (mean2 * mean2));
    cv = fmaxf(cv, FLT_MIN);
    const float dm = mean2 - mean1;
    return (float) (fabs((double) dm) / sqrt((double) (cv / wf)));
}

// both t-statistic arrays, one thread per sample; blk[b] = (read, first sample) of block b
__global__ __launch_bounds__(256) void k_det_tstat(const DetJob *__restrict__ jobs, const int2 *__restrict__ blk, const double *__restrict__ S,
                                                   const double *__restrict__ Q, float *__restrict__ T1, float *__restrict__ T2, int w1, int w2) {
    const int2 bi = blk[blockIdx.x];
    const DetJob J = jobs[bi.x];
    const int i = bi.y + (int) threadIdx.x;
    if (i >= J.n) return;
    const double *s = S + J.ps_off, *q = Q + J.ps_off;
    T1[J.raw_off + i] = det_tstat(s, q, J.n, w1, i);
    T2[J.raw_off + i] = det_tstat(s, q, J.n, w2, i);
}

struct DetState {
    long long masked_to;
    int peak_pos;
    float peak_value;
    bool valid;
};

// short_long_peak_detector, one lane per read: peaks in emission order, their number in cnt[r]
__global__ __launch_bounds__(DET_LANES) void k_det_peaks(const DetJob *__restrict__ jobs, int n_jobs, const float *__restrict__ T1,
                                                         const float *__restrict__ T2, int *__restrict__ peaks, int *__restrict__ cnt,
                                                         int w1, int w2, float thr1, float thr2, float ph) {
    const int r = blockIdx.x * DET_LANES + threadIdx.x;
    if (r >= n_jobs) return;
    const DetJob J = jobs[r];
    const float4 *t1 = (const float4 *) (T1 + J.raw_off), *t2 = (const float4 *) (T2 + J.raw_off);
    int *pk = peaks + J.raw_off;
    const int n = J.n, n_chunks = (n + 3) / 4;
    DetState sd = {0, -1, FLT_MAX, false}, ld = {0, -1, FLT_MAX, false};
    const long long half1 = w1 / 2, half2 = w2 / 2;
    int np = 0;
    float4 n1 = t1[0], n2 = t2[0];
    for (int c = 0; c < n_chunks; c++) {
        const float4 c1 = n1, c2 = n2;
        if (c + 1 < n_chunks) { n1 = t1[c + 1]; n2 = t2[c + 1]; }
        const float v1[4] = {c1.x, c1.y, c1.z, c1.w}, v2[4] = {c2.x, c2.y, c2.z, c2.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = 4 * c + k;
            if (i >= n) break;
            // the short detector
            if (sd.masked_to < i) {
                const float v = v1[k];
                if (sd.peak_pos == -1) {
                    if (v < sd.peak_value) sd.peak_value = v;
                    else if (v - sd.peak_value > ph) { sd.peak_value = v; sd.peak_pos = i; }
                } else {
                    if (v > sd.peak_value) { sd.peak_value = v; sd.peak_pos = i; }
                    if (sd.peak_value > thr1) {   // dominate the long detector
                        ld.masked_to = (long long) sd.peak_pos + w1;
                        ld.peak_pos = -1;
                        ld.peak_value = FLT_MAX;
                        ld.valid = false;
                    }
                    if (sd.peak_value - v > ph && sd.peak_value > thr1) sd.valid = true;
                    if (sd.valid && (long long) (i - sd.peak_pos) > half1) {
                        if (np < n) pk[np] = sd.peak_pos;   // peaks rise strictly: np < n always; the test keeps a fault impossible
                        np++;
                        sd.peak_pos = -1;
                        sd.peak_value = v;
                        sd.valid = false;
                    }
                }
            }
            // the long detector
            if (ld.masked_to < i) {
                const float v = v2[k];
                if (ld.peak_pos == -1) {
                    if (v < ld.peak_value) ld.peak_value = v;
                    else if (v - ld.peak_value > ph) { ld.peak_value = v; ld.peak_pos = i; }
                } else {
                    if (v > ld.peak_value) { ld.peak_value = v; ld.peak_pos = i; }
                    if (ld.peak_value - v > ph && ld.peak_value > thr2) ld.valid = true;
                    if (ld.valid && (long long) (i - ld.peak_pos) > half2) {
                        if (np < n) pk[np] = ld.peak_pos;
                        np++;
                        ld.peak_pos = -1;
                        ld.peak_value = v;
                        ld.valid = false;
                    }
                }
            }
        }
    }
    cnt[r] = np < n ? np : n - 1;
}

// events per read (peaks + 1: a read without a peak is one event) -> exclusive offsets, one block; off[n_jobs] = total
__global__ __launch_bounds__(1024) void k_det_scan(const int *__restrict__ cnt, int n_jobs, long long *__restrict__ off) {
    __shared__ long long part[1024];
    const int t = threadIdx.x, per = (n_jobs + 1023) / 1024, a = t * per, b = min(a + per, n_jobs);
    long long sum = 0;
    for (int j = a; j < b; j++) sum += cnt[j] + 1;
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = part[t] - sum;
    for (int j = a; j < b; j++) { off[j] = run; run += cnt[j] + 1; }
    if (t == 1023) off[n_jobs] = part[t];
}

// create_events: event e of read r spans [peaks[e - 1], peaks[e]) with peaks[-1] = 0 and peaks[np] = n
__global__ __launch_bounds__(256) void k_det_events(const DetJob *__restrict__ jobs, const int *__restrict__ peaks, const int *__restrict__ cnt,
                                                    const long long *__restrict__ off, const double *__restrict__ S,
                                                    const double *__restrict__ Q, DetEvent *__restrict__ out) {
    const int r = blockIdx.x;
    const DetJob J = jobs[r];
    const int np = cnt[r];
    const int *pk = peaks + J.raw_off;
    const double *s = S + J.ps_off, *q = Q + J.ps_off;
    DetEvent *o = out + off[r];
    for (int e = threadIdx.x; e <= np; e += blockDim.x) {
        const int st = e == 0 ? 0 : pk[e - 1];
        const int en = e == np ? J.n : pk[e];
        DetEvent ev;
        ev.start = st;
        ev.length = (float) (unsigned long long) ((long long) en - (long long) st);   // size_t difference, as the reference's
        ev.mean = (float) (s[en] - s[st]) / ev.length;
        const float deltasqr = (float) (q[en] - q[st]);
        const float var = deltasqr / ev.length - ev.mean * ev.mean;
        ev.stdv = sqrtf(fmaxf(var, 0.0f));
        o[e] = ev;
    }
}

// ---- k_raw_finish: the detector's rows and the event aligner's pairs -> the rows of a 1D .npRead (sa_npread_from_raw_batch) ----
struct FinJob {
    long long ev_off;    // the read's rows in the detector's event block; also where its output rows start
    long long pair_off;  // its pairs {k-mer, event}, ascending
    int n_ev, n_pairs;   // n_pairs == 0: a read the chain rejected -- no rows
    float sample_rate, start_time;
};

struct FinOut {          // each array has an entry per detected event; a read's rows start at its ev_off, mapped rows only, packed
    double *ev4;         // {mean, stdv, length, start - start of row 0}
    long long *raw_start, *raw_length;
    int *kmer_idx, *move;
    int *n_rows;         // per read
};

#define FIN_WAVE 64
#define FIN_WAVES 4      // reads per block

// One wave per read.
//   1. all lanes clear the read's per-event k-mer index (-1) and move (0);
//   2. alignment_to_base_event_map (impl/eventAligner.c:1310-1360): the pairs come in 64 at a time, one per lane, and are walked in
//      order through wave-uniform state; lane 0 stores an event's k-mer index and move when the walk leaves the event;
//   3. the mapped rows (kmer_idx >= 0) are compacted, 64 events a step: ballot of the mapped lanes, a lane's row is the running
//      count plus the mapped lanes below it; event_table_to_basecalled_table's seconds in its own operation order (fp64 + - / and
//      one float division, no contraction in this file).
// Between the steps the wave's own stores have to be visible to its other lanes: the block synchronises (every wave of the block
// reaches both barriers, also one without a read).
__global__ __launch_bounds__(FIN_WAVE * FIN_WAVES) void k_raw_finish(const FinJob *__restrict__ jobs, int n_jobs, const DetEvent *__restrict__ ev,
                                                                     const int2 *__restrict__ pairs, int *__restrict__ kidx,
                                                                     int *__restrict__ mv, FinOut O) {
    const int lane = threadIdx.x & (FIN_WAVE - 1);
    const int r = blockIdx.x * FIN_WAVES + (int) (threadIdx.x / FIN_WAVE);
    const bool live = r < n_jobs;
    FinJob J = {0, 0, 0, 0, 1.0f, 0.0f};
    if (live) J = jobs[r];
    int *ki = kidx + J.ev_off, *mo = mv + J.ev_off;
    for (int e = lane; e < J.n_ev; e += FIN_WAVE) { ki[e] = -1; mo[e] = 0; }
    __syncthreads();
    {
        const int2 *p = pairs + J.pair_off;
        int prev_k = 0, prev_e = -1, cur_k = -1, cur_mv = 0;
        for (int base = 0; base < J.n_pairs; base += FIN_WAVE) {
            const int2 mine = base + lane < J.n_pairs ? p[base + lane] : make_int2(0, 0);
            const int n_here = min(FIN_WAVE, J.n_pairs - base);
            for (int t = 0; t < n_here; t++) {
                const int k = __shfl(mine.x, t), e = __shfl(mine.y, t);
                if (e == prev_e) {
                    if (k == prev_k || prev_k == 0) continue;   // the reference reports the first, skips the second
                    cur_k = k;
                    cur_mv += k - prev_k;
                } else {
                    if (lane == 0 && prev_e >= 0 && prev_e < J.n_ev) { ki[prev_e] = cur_k; mo[prev_e] = cur_mv; }
                    cur_k = k;
                    cur_mv = k - prev_k;
                }
                prev_k = k;
                prev_e = e;
            }
        }
        if (lane == 0 && prev_e >= 0 && prev_e < J.n_ev) { ki[prev_e] = cur_k; mo[prev_e] = cur_mv; }
    }
    __syncthreads();
    if (!live) return;
    const DetEvent *src = ev + J.ev_off;
    const float sr = J.sample_rate;
    const double st_sr = (double) (J.start_time / sr);
    // row 0: the first mapped event
    int first = -1;
    for (int base = 0; base < J.n_ev && first < 0; base += FIN_WAVE) {
        const int e = base + lane;
        const unsigned long long m = __ballot(e < J.n_ev && ki[e] >= 0);
        if (m) first = base + __ffsll((long long) m) - 1;
    }
    int n_rows = 0;
    if (first >= 0) {
        const double start0 = ((double) (unsigned long long) src[first].start) / sr + st_sr;
        for (int base = 0; base < J.n_ev; base += FIN_WAVE) {
            const int e = base + lane;
            const int k = e < J.n_ev ? ki[e] : -1;
            const unsigned long long m = __ballot(k >= 0);
            if (k >= 0) {
                const long long row = J.ev_off + n_rows + __popcll(m & ((1ull << lane) - 1ull));
                const DetEvent v = src[e];
                O.ev4[4 * row] = (double) v.mean;
                O.ev4[4 * row + 1] = (double) v.stdv;
                O.ev4[4 * row + 2] = (double) (v.length / sr);
                O.ev4[4 * row + 3] = (((double) (unsigned long long) v.start) / sr + st_sr) - start0;
                O.raw_start[row] = v.start;
                O.raw_length[row] = (long long) (unsigned long long) v.length;
                O.kmer_idx[row] = k;
                O.move[row] = mo[e];
            }
            n_rows += __popcll(m);
        }
    }
    if (lane == 0) O.n_rows[r] = n_rows;
}

// Device and pinned-host scratch of sa_detect_events_batch, kept between calls (sa_scratch.h); the last two are the finishing
// stage's (sa_npread_from_raw_batch).
enum { DET_WS, DET_EV, DET_HRAW, DET_HEV, DET_FIN, DET_HFIN };
static SaScratch g_det_ws;

extern "C" void sa_detect_release(void) {
    std::lock_guard<std::mutex> guard(g_det_ws.mu);
    g_det_ws.release();
}

static const sa_detector_params_t k_det_dna = SA_DETECTOR_DNA, k_det_rna = SA_DETECTOR_RNA;

// What one detection run leaves behind for the caller, who holds g_det_ws.mu for as long as it reads any of it: the event rows and
// their offsets on the device (k_raw_finish reads them there), the counts, offsets and rows in pinned memory.
struct DetRun {
    const DetEvent *d_ev, *h_ev;
    const long long *d_off, *h_off;
    const int *h_cnt;
    float kms;
};

// the five detection kernels for a batch whose arguments have been checked; the caller holds g_det_ws.mu
static int det_run(const sa_raw_job_t *jobs, size_t nj, const sa_detector_params_t &P, int device, DetRun *R) {
    int rc;
    std::vector<DetJob> hj(nj);
    std::vector<int2> blk;
    long long raw_tot = 0, ps_tot = 0;
    for (size_t j = 0; j < nj; j++) {
        DetJob &J = hj[j];
        J.n = (int) jobs[j].n_samples;
        J.raw_off = raw_tot;
        J.ps_off = ps_tot;
        J.digitisation = jobs[j].digitisation;
        J.offset = jobs[j].offset;
        J.range = jobs[j].range;
        raw_tot += ((long long) J.n + 7) / 8 * 8;     // zero padding to the 16-byte chunk the lanes load
        ps_tot += (long long) J.n + 1;
        for (int b = 0; b < J.n; b += 256) blk.push_back(make_int2((int) j, b));
    }
    SaScratch &W = g_det_ws;
    if ((rc = W.rebind(device)) != SA_OK) return rc;
    // device workspace: [jobs | blocks | raw | sum | sumsq | t1 | t2 | peaks | counts, offsets]; events in their own block.  Counts
    // and offsets are ONE entry: one copy back
    SaLayout L;
    const size_t raw_bytes = sizeof(int16_t) * (size_t) raw_tot, res_bytes = sa_up256(sizeof(int) * nj) + sizeof(long long) * (nj + 1);
    const size_t o_jobs = L.add(sizeof(DetJob) * nj), o_blk = L.add(sizeof(int2) * blk.size()), o_raw = L.add(raw_bytes),
                 o_s = L.add(sizeof(double) * (size_t) ps_tot), o_q = L.add(sizeof(double) * (size_t) ps_tot),
                 o_t1 = L.add(sizeof(float) * (size_t) raw_tot), o_t2 = L.add(sizeof(float) * (size_t) raw_tot),
                 o_pk = L.add(sizeof(int) * (size_t) raw_tot), o_cnt = L.add(res_bytes), o_off = o_cnt + sa_up256(sizeof(int) * nj);
    long long n_ev_tot = 0;
    if ((rc = W.dev(DET_WS, L.end)) != SA_OK) return rc;
    // events: at most one per peak plus one per read, and peaks are fewer than samples
    if ((rc = W.dev(DET_EV, sizeof(DetEvent) * (size_t) (raw_tot + (long long) nj))) != SA_OK) return rc;
    if ((rc = W.pin(DET_HRAW, raw_bytes > res_bytes ? raw_bytes : res_bytes)) != SA_OK) return rc;
    {
        int16_t *hr = (int16_t *) W.at(DET_HRAW);
        sa_parallel_for(nj, [&](size_t j) {
            const DetJob &J = hj[j];
            memcpy(hr + J.raw_off, jobs[j].raw, sizeof(int16_t) * (size_t) J.n);
            for (int k = J.n; k % 8; k++) hr[J.raw_off + k] = 0;
        });
    }
    {
        char *d = (char *) W.at(DET_WS);
        const DetJob *d_jobs = (const DetJob *) (d + o_jobs);
        double *d_s = (double *) (d + o_s), *d_q = (double *) (d + o_q);
        float *d_t1 = (float *) (d + o_t1), *d_t2 = (float *) (d + o_t2);
        int *d_pk = (int *) (d + o_pk), *d_cnt = (int *) (d + o_cnt);
        long long *d_off = (long long *) (d + o_off);
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_jobs, hj.data(), sizeof(DetJob) * nj, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_blk, blk.data(), sizeof(int2) * blk.size(), hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_raw, W.at(DET_HRAW), raw_bytes, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(W.time_begin());
        const unsigned lane_blocks = (unsigned) ((nj + DET_LANES - 1) / DET_LANES);
        hipLaunchKernelGGL(k_det_prefix, dim3(lane_blocks), dim3(DET_LANES), 0, 0, d_jobs, (int) nj, (const int16_t *) (d + o_raw), d_s, d_q);
        hipLaunchKernelGGL(k_det_tstat, dim3((unsigned) blk.size()), dim3(256), 0, 0, d_jobs, (const int2 *) (d + o_blk), d_s, d_q, d_t1,
                           d_t2, P.window_length1, P.window_length2);
        hipLaunchKernelGGL(k_det_peaks, dim3(lane_blocks), dim3(DET_LANES), 0, 0, d_jobs, (int) nj, d_t1, d_t2, d_pk, d_cnt,
                           P.window_length1, P.window_length2, P.threshold1, P.threshold2, P.peak_height);
        hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(1024), 0, 0, d_cnt, (int) nj, d_off);
        hipLaunchKernelGGL(k_det_events, dim3((unsigned) nj), dim3(256), 0, 0, d_jobs, (const int *) d_pk, (const int *) d_cnt,
                           (const long long *) d_off, (const double *) d_s, (const double *) d_q, (DetEvent *) W.at(DET_EV));
        SA_HIP_GOTO_DONE(W.time_end());
        SA_HIP_GOTO_DONE(hipMemcpyAsync(W.at(DET_HRAW), d + o_cnt, res_bytes, hipMemcpyDeviceToHost, 0));   // the raw image is uploaded by now
        SA_HIP_GOTO_DONE(hipStreamSynchronize(0));
        SA_HIP_GOTO_DONE(W.time_ms(&R->kms));
        R->h_cnt = (const int *) W.at(DET_HRAW);
        R->h_off = (const long long *) ((const char *) W.at(DET_HRAW) + (o_off - o_cnt));
        R->d_off = d_off;
        n_ev_tot = R->h_off[nj];
        if ((rc = W.pin(DET_HEV, sizeof(DetEvent) * (size_t) n_ev_tot)) != SA_OK) goto done;
        SA_HIP_GOTO_DONE(hipMemcpyAsync(W.at(DET_HEV), W.at(DET_EV), sizeof(DetEvent) * (size_t) n_ev_tot, hipMemcpyDeviceToHost, 0));
        SA_HIP_GOTO_DONE(hipStreamSynchronize(0));
        R->d_ev = (const DetEvent *) W.at(DET_EV);
        R->h_ev = (const DetEvent *) W.at(DET_HEV);
    }
done:
    return rc;
}

extern "C" int sa_detect_events_batch(const sa_raw_job_t *jobs, int64_t n_jobs, const sa_detector_params_t *params, int device,
                                      unsigned flags, sa_raw_event_t **events_out, int64_t *n_events_out, int32_t *status_out,
                                      double *kernel_ms_out) {
    if ((!jobs && n_jobs > 0) || n_jobs < 0 || n_jobs > (1 << 30) || !events_out || !n_events_out) return SA_EINVAL;
    const sa_detector_params_t P = params ? *params : ((flags & SA_FLAG_RNA) ? k_det_rna : k_det_dna);
    if (P.window_length1 < 1 || P.window_length2 < 1) return SA_EINVAL;
    for (int64_t j = 0; j < n_jobs; j++) {
        events_out[j] = nullptr;
        n_events_out[j] = 0;
        if (status_out) status_out[j] = 0;
    }
    for (int64_t j = 0; j < n_jobs; j++)
        if (!jobs[j].raw || jobs[j].n_samples < 1 || jobs[j].n_samples > 0x7fffffffLL - 8) return SA_EINVAL;
    int rc = sa_device_check(device);
    if (rc || n_jobs == 0) return rc;
    const size_t nj = (size_t) n_jobs;
    std::lock_guard<std::mutex> guard(g_det_ws.mu);
    DetRun run;
    if ((rc = det_run(jobs, nj, P, device, &run)) != SA_OK) return rc;
    const int *h_cnt = run.h_cnt;
    const long long *h_off = run.h_off;
    const DetEvent *h_ev = run.h_ev;
    if (kernel_ms_out) *kernel_ms_out = (double) run.kms;
    {
        std::atomic<bool> oom(false);
        sa_parallel_for(nj, [&](size_t j) {
            const long long a = h_off[j], n = h_off[j + 1] - a;
            sa_raw_event_t *o = (sa_raw_event_t *) malloc(sizeof(sa_raw_event_t) * (size_t) n);
            if (!o) { oom = true; return; }
            const float sr = jobs[j].sample_rate, st = jobs[j].start_time;
            const double st_sr = (double) (st / sr);
            for (long long e = 0; e < n; e++) {   // event_table_to_basecalled_table (impl/eventAligner.c:753-766)
                const DetEvent &v = h_ev[a + e];
                sa_raw_event_t &r = o[e];
                r.raw_start = v.start;
                r.raw_length = (int64_t) (uint64_t) v.length;
                r.mean = v.mean;
                r.stdv = v.stdv;
                r.start = ((double) (uint64_t) v.start) / sr + st_sr;
                r.length = v.length / sr;
                r.kmer_idx = -1;
                r.move = 0;
                r.p_model_state = 0.0;
            }
            events_out[j] = o;
            n_events_out[j] = n;
            if (status_out) status_out[j] = h_cnt[j] == 0 ? SA_RAW_NO_PEAK : 0;
        });
        if (oom) rc = SA_ENOMEM;
    }
    if (rc != SA_OK)
        for (size_t j = 0; j < nj; j++) { free(events_out[j]); events_out[j] = nullptr; n_events_out[j] = 0; }
    return rc;
}

// MoM scalings of every read's event means (the aligned order) and ONE sa_event_align_batch call with var = 1: the middle of
// load_from_raw2, shared by sa_raw_event_align_batch and sa_npread_from_raw_batch
static int raw_scale_and_align(const sa_model_t *m, const char *const *sequences, const std::vector<std::vector<double>> &means,
                               int device, unsigned flags, std::vector<sa_ea_job_t> &ej, std::vector<double> &shift,
                               std::vector<double> &scale, sa_ea_pair_t **pairs, int64_t *n_pairs, int32_t *ea_st, double *ea_ms) {
    const size_t nj = means.size();
    int rc = SA_OK;
    for (size_t j = 0; j < nj && rc == SA_OK; j++) {
        const int64_t n = (int64_t) means[j].size(), len = (int64_t) strlen(sequences[j]);
        rc = sa_scalings_mom(m, sequences[j], len, means[j].data(), n, flags, &shift[j], &scale[j]);
        ej[j] = sa_ea_job_t{sequences[j], len, means[j].data(), n, scale[j], shift[j], 1.0};
    }
    if (rc == SA_OK) rc = sa_event_align_batch(m, ej.data(), (int64_t) nj, device, flags & SA_FLAG_RNA, pairs, n_pairs, ea_st, nullptr, ea_ms);
    return rc;
}

// p_model_state of an event mapped to a k-mer with level (mu, sd) under the MoM scalings:
// emissions_signal_strawManGetKmerEventMatchProbWithDescaling_MeanOnly with var = 1 (sa_ea.hip: ea_emit), then exp
static inline double raw_p_model_state(double mean, double mu, double sd, double sc, double sh) {
    const double c = sd == 0.0 ? -INFINITY : (-0.91893853320467267 - log(sd));
    const double en = (mean + 1.0 * mu - sc * mu - sh) / 1.0;
    const double a = (en - mu) / (sd == 0.0 ? 1.0 : sd);
    return exp(log(1 / 1.0) + (c + (-0.5 * a * a)));
}

extern "C" int sa_raw_event_align_batch(const sa_model_t *m, const sa_raw_job_t *jobs, const char *const *sequences, int64_t n_jobs,
                                        const sa_detector_params_t *params, int device, unsigned flags, sa_raw_event_t **events_out,
                                        int64_t *n_events_out, sa_ea_pair_t **pairs_out, int64_t *n_pairs_out, int32_t *status_out,
                                        double *shift_out, double *scale_out, double *kernel_ms_out) {
    if (!m || (!sequences && n_jobs > 0) || n_jobs < 0 || !events_out || !n_events_out || !status_out) return SA_EINVAL;
    if (pairs_out && !n_pairs_out) return SA_EINVAL;
    if (m->hdp) return SA_EUNSUPPORTED;
    for (int64_t j = 0; j < n_jobs; j++) {
        if (!sequences[j]) return SA_EINVAL;
        if (pairs_out) { pairs_out[j] = nullptr; n_pairs_out[j] = 0; }
    }
    const bool rna = (flags & SA_FLAG_RNA) != 0;
    const size_t nj = (size_t) n_jobs;
    double det_ms = 0, ea_ms = 0;
    int rc = sa_detect_events_batch(jobs, n_jobs, params, device, flags, events_out, n_events_out, status_out, &det_ms);
    if (rc != SA_OK || n_jobs == 0) return rc;
    // the aligned event order (reverse_events for RNA) and the MoM scalings of it
    std::vector<std::vector<double>> means(nj);
    std::vector<sa_ea_job_t> ej(nj);
    std::vector<double> shift(nj), scale(nj);
    std::vector<sa_ea_pair_t *> pairs(nj, nullptr);
    std::vector<int64_t> n_pairs(nj, 0);
    std::vector<int32_t> ea_st(nj, 0);
    for (size_t j = 0; j < nj; j++) {
        const int64_t n = n_events_out[j];
        means[j].resize((size_t) n);
        for (int64_t e = 0; e < n; e++) means[j][(size_t) e] = events_out[j][rna ? n - 1 - e : e].mean;
    }
    rc = raw_scale_and_align(m, sequences, means, device, flags, ej, shift, scale, pairs.data(), n_pairs.data(), ea_st.data(), &ea_ms);
    if (rc == SA_OK) {
        std::atomic<int> bad(SA_OK);
        sa_parallel_for(nj, [&](size_t j) {
            status_out[j] |= ea_st[j];
            if (shift_out) shift_out[j] = shift[j];
            if (scale_out) scale_out[j] = scale[j];
            const int64_t np = n_pairs[j], n_ev = n_events_out[j], n_kmers = ej[j].seq_len - (m->k - 1);
            if (np == 0) return;
            std::vector<int32_t> ids((size_t) n_kmers);
            const int rck = sa_ea_kmer_ids(m, sequences[j], n_kmers, rna, ids.data());
            if (rck) { bad = rck; return; }
            sa_raw_event_t *ev = events_out[j];
            const double sc = scale[j], sh = shift[j];
            // event index of the aligned table -> row of the time-ordered output
            auto row = [&](int64_t e) -> sa_raw_event_t & { return ev[rna ? n_ev - 1 - e : e]; };
            auto map = [&](int64_t k, int64_t e) {
                sa_raw_event_t &r = row(e);
                const int64_t id = ids[(size_t) k];
                const double mu = m->table5[5 * id], sd = m->table5[5 * id + 1];
                r.p_model_state = raw_p_model_state(r.mean, mu, sd, sc, sh);
                r.kmer_idx = (int32_t) k;
            };
            const sa_ea_pair_t *p = pairs[j];
            int64_t prev_e = -1;
            if (!rna) {   // alignment_to_base_event_map (impl/eventAligner.c:1310-1360)
                int64_t prev_k = 0;
                for (int64_t i = 0; i < np; i++) {
                    const int64_t k = p[i].kmer_idx, e = p[i].event_idx;
                    if (e == prev_e) {
                        if (k == prev_k || prev_k == 0) continue;   // the reference reports the first, skips the second
                        map(k, e);
                        row(e).move += (int32_t) (k - prev_k);
                    } else {
                        map(k, e);
                        row(e).move = (int32_t) (k - prev_k);
                    }
                    prev_k = k;
                    prev_e = e;
                }
            } else {      // rna_alignment_to_base_event_map (:1362-1414), walked from the last pair
                int64_t prev_k = n_kmers - 1;
                for (int64_t i = np - 1; i >= 0; i--) {
                    const int64_t k = p[i].kmer_idx, e = p[i].event_idx;
                    if (e == prev_e) {
                        if (k == prev_k) continue;
                        map(k, e);
                        row(e).move += (int32_t) (prev_k - k);
                    } else {
                        map(k, e);
                        row(e).move = (int32_t) (prev_k - k);
                    }
                    prev_k = k;
                    prev_e = e;
                }
            }
        });
        rc = bad;
    }
    if (kernel_ms_out) *kernel_ms_out = det_ms + ea_ms;
    for (size_t j = 0; j < nj; j++) {
        if (pairs_out && rc == SA_OK) { pairs_out[j] = pairs[j]; n_pairs_out[j] = n_pairs[j]; }
        else free(pairs[j]);
    }
    if (rc != SA_OK)
        for (size_t j = 0; j < nj; j++) { free(events_out[j]); events_out[j] = nullptr; n_events_out[j] = 0; }
    return rc;
}

// ---- raw current -> the in-memory .npRead of a 1D read --------------------------------------------------------------------
static std::atomic<double> g_fin_ms(0.0);

extern "C" double sa_npread_last_finish_ms(void) { return g_fin_ms.load(); }

extern "C" void sa_raw_npread_free(sa_raw_npread_t *r, int64_t n) {
    if (!r) return;
    for (int64_t j = 0; j < n; j++) {
        free(r[j].events4);   // a read's arrays are one allocation that events4 heads
        memset(&r[j], 0, sizeof(r[j]));
    }
}

// NanoporeRead.make_event_map (nanoporeRead.py:313-333) over the rows; returns the map's length, of which at most `cap`
// entries are written
static int64_t raw_make_event_map(const int32_t *move, const double *p, int64_t n, int k, int64_t *map, int64_t cap) {
    int64_t len = 0;
    auto put = [&](int64_t v) { if (len < cap) map[len] = v; len++; };
    auto last = [&]() -> int64_t { return len - 1 < cap ? map[len - 1] : map[cap - 1]; };
    put(0);
    double previous = 0;
    for (int64_t i = 1; i < n; i++) {
        const int32_t mv = move[i];
        if (mv == 1) put(i);
        if (mv > 1) {
            for (int32_t s = 0; s < mv - 1; s++) put(i - 1);
            put(i);
        }
        if (mv == 0 && p[i] > previous && len - 1 < cap) map[len - 1] = i;
        previous = p[i];
    }
    const int64_t fin = last();
    for (int s = 0; s < k - 1; s++) put(fin);
    return len;
}

extern "C" int sa_npread_from_raw_batch(const sa_model_t *m, const sa_raw_job_t *jobs, const char *const *sequences, int64_t n_jobs,
                                        const sa_detector_params_t *params, int device, unsigned flags, sa_raw_npread_t *out,
                                        double *kernel_ms_out) {
    if (!m || n_jobs < 0 || n_jobs > (1 << 30) || ((!jobs || !sequences || !out) && n_jobs > 0)) return SA_EINVAL;
    if (flags & SA_FLAG_RNA) return SA_EUNSUPPORTED;   // the reference's RNA path reverses reads and events: not built here
    if (m->hdp) return SA_EUNSUPPORTED;                // as sa_raw_event_align_batch
    const sa_detector_params_t P = params ? *params : k_det_dna;
    if (P.window_length1 < 1 || P.window_length2 < 1) return SA_EINVAL;
    for (int64_t j = 0; j < n_jobs; j++) memset(&out[j], 0, sizeof(out[j]));
    for (int64_t j = 0; j < n_jobs; j++)
        if (!jobs[j].raw || jobs[j].n_samples < 1 || jobs[j].n_samples > 0x7fffffffLL - 8 || !sequences[j] ||
            (int64_t) strlen(sequences[j]) < m->k)
            return SA_EINVAL;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    int rc = sa_device_check(device);
    if (rc || n_jobs == 0) return rc;
    const size_t nj = (size_t) n_jobs;
    SaScratch &W = g_det_ws;
    std::lock_guard<std::mutex> guard(W.mu);   // held to the end: the detector's rows are read where it left them
    DetRun run;
    if ((rc = det_run(jobs, nj, P, device, &run)) != SA_OK) return rc;
    std::vector<std::vector<double>> means(nj);
    std::vector<sa_ea_job_t> ej(nj);
    std::vector<double> shift(nj), scale(nj);
    std::vector<sa_ea_pair_t *> pairs(nj, nullptr);
    std::vector<int64_t> n_pairs(nj, 0);
    std::vector<int32_t> ea_st(nj, 0);
    std::vector<FinJob> fj(nj);
    double ea_ms = 0;
    float fin_ms = 0;
    sa_parallel_for(nj, [&](size_t j) {
        const long long a = run.h_off[j], n = run.h_off[j + 1] - a;
        means[j].resize((size_t) n);
        for (long long e = 0; e < n; e++) means[j][(size_t) e] = run.h_ev[a + e].mean;
    });
    rc = raw_scale_and_align(m, sequences, means, device, 0, ej, shift, scale, pairs.data(), n_pairs.data(), ea_st.data(), &ea_ms);
    if (rc == SA_OK && (rc = W.rebind(device)) == SA_OK) {
        long long pair_tot = 0;
        const long long ev_tot = run.h_off[nj];
        for (size_t j = 0; j < nj; j++) {
            out[j].status = ea_st[j] | (run.h_cnt[j] == 0 ? SA_RAW_NO_PEAK : 0);
            FinJob &F = fj[j];
            F.ev_off = run.h_off[j];
            F.n_ev = (int) (run.h_off[j + 1] - run.h_off[j]);
            F.pair_off = pair_tot;
            F.n_pairs = out[j].status == 0 ? (int) n_pairs[j] : 0;
            F.sample_rate = jobs[j].sample_rate;
            F.start_time = jobs[j].start_time;
            pair_tot += F.n_pairs;
        }
        // device block: [jobs, pairs (ONE entry: one copy up) | k-mer index and move per event | the rows: events4, raw_start,
        // raw_length, kmer_idx, move, rows per read (ONE entry: one copy back into the pinned block)]
        SaLayout L;
        const size_t ne = (size_t) ev_tot, in_pairs = sa_up256(sizeof(FinJob) * nj), in_bytes = in_pairs + sizeof(int2) * (size_t) pair_tot;
        const size_t r_rs = sa_up256(sizeof(double) * 4 * ne), r_rl = r_rs + sa_up256(sizeof(long long) * ne),
                     r_ki = r_rl + sa_up256(sizeof(long long) * ne), r_mv = r_ki + sa_up256(sizeof(int) * ne),
                     r_n = r_mv + sa_up256(sizeof(int) * ne), res_bytes = r_n + sizeof(int) * nj;
        const size_t o_in = L.add(in_bytes), o_ki = L.add(sizeof(int) * ne), o_mv = L.add(sizeof(int) * ne), o_res = L.add(res_bytes);
        if ((rc = W.dev(DET_FIN, L.end)) != SA_OK) goto done;
        if ((rc = W.pin(DET_HFIN, in_bytes > res_bytes ? in_bytes : res_bytes)) != SA_OK) goto done;
        {
            char *h = (char *) W.at(DET_HFIN), *d = (char *) W.at(DET_FIN);
            memcpy(h, fj.data(), sizeof(FinJob) * nj);
            int2 *hp = (int2 *) (h + in_pairs);
            sa_parallel_for(nj, [&](size_t j) {
                if (fj[j].n_pairs > 0) memcpy(hp + fj[j].pair_off, pairs[j], sizeof(int2) * (size_t) fj[j].n_pairs);
            });
            FinOut O;
            O.ev4 = (double *) (d + o_res);
            O.raw_start = (long long *) (d + o_res + r_rs);
            O.raw_length = (long long *) (d + o_res + r_rl);
            O.kmer_idx = (int *) (d + o_res + r_ki);
            O.move = (int *) (d + o_res + r_mv);
            O.n_rows = (int *) (d + o_res + r_n);
            SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_in, h, in_bytes, hipMemcpyHostToDevice, 0));
            SA_HIP_GOTO_DONE(W.time_begin());
            hipLaunchKernelGGL(k_raw_finish, dim3((unsigned) ((nj + FIN_WAVES - 1) / FIN_WAVES)), dim3(FIN_WAVE * FIN_WAVES), 0, 0,
                               (const FinJob *) (d + o_in), (int) nj, run.d_ev, (const int2 *) (d + o_in + in_pairs), (int *) (d + o_ki),
                               (int *) (d + o_mv), O);
            SA_HIP_GOTO_DONE(W.time_end());
            // (the upload image has been consumed by the time the rows come back over it: one stream)
            SA_HIP_GOTO_DONE(hipMemcpyAsync(h, d + o_res, res_bytes, hipMemcpyDeviceToHost, 0));
            SA_HIP_GOTO_DONE(hipStreamSynchronize(0));
            SA_HIP_GOTO_DONE(W.time_ms(&fin_ms));
            g_fin_ms = (double) fin_ms;
            // the host's share: p_model_state (an exp and a log) and make_event_map, which compares those values
            const double *h_ev4 = (const double *) h;
            const long long *h_rs = (const long long *) (h + r_rs), *h_rl = (const long long *) (h + r_rl);
            const int *h_ki = (const int *) (h + r_ki), *h_mv = (const int *) (h + r_mv), *h_n = (const int *) (h + r_n);
            std::atomic<int> bad(SA_OK);
            sa_parallel_for(nj, [&](size_t j) {
                sa_raw_npread_t &o = out[j];
                o.read_len = ej[j].seq_len;
                o.mom_shift = shift[j];
                o.mom_scale = scale[j];
                if (o.status != 0) return;
                const size_t n = (size_t) h_n[j], a = (size_t) fj[j].ev_off, rl = (size_t) o.read_len;
                if (n == 0) { o.status = SA_RAW_MAP_LENGTH; return; }
                const int64_t n_kmers = o.read_len - (m->k - 1);
                std::vector<int32_t> ids((size_t) n_kmers);
                const int rck = sa_ea_kmer_ids(m, sequences[j], n_kmers, false, ids.data());
                if (rck) { bad = rck; return; }
                // one allocation per read: doubles, then 64-bit integers, then 32-bit ones
                char *blk = (char *) malloc(sizeof(double) * 5 * n + sizeof(int64_t) * (2 * n + rl) + sizeof(int32_t) * 2 * n);
                if (!blk) { bad = SA_ENOMEM; return; }
                o.n_events = (int64_t) n;
                o.events4 = (double *) blk;
                o.p_model_state = o.events4 + 4 * n;
                o.raw_start = (int64_t *) (o.p_model_state + n);
                o.raw_length = o.raw_start + n;
                o.strand_event_map = o.raw_length + n;
                o.kmer_idx = (int32_t *) (o.strand_event_map + rl);
                o.move = o.kmer_idx + n;
                memcpy(o.events4, h_ev4 + 4 * a, sizeof(double) * 4 * n);
                memcpy(o.raw_start, h_rs + a, sizeof(int64_t) * n);
                memcpy(o.raw_length, h_rl + a, sizeof(int64_t) * n);
                memcpy(o.kmer_idx, h_ki + a, sizeof(int32_t) * n);
                memcpy(o.move, h_mv + a, sizeof(int32_t) * n);
                bool in_range = true;
                for (size_t i = 0; i < n; i++) {
                    const int32_t kx = o.kmer_idx[i];
                    if (kx < 0 || kx >= n_kmers) { in_range = false; break; }
                    const int64_t id = ids[(size_t) kx];
                    o.p_model_state[i] = raw_p_model_state(o.events4[4 * i], m->table5[5 * id], m->table5[5 * id + 1], scale[j], shift[j]);
                }
                if (!in_range || raw_make_event_map(o.move, o.p_model_state, (int64_t) n, m->k, o.strand_event_map, o.read_len) != o.read_len) {
                    // the reference's "Read and event map lengths do not match"
                    free(blk);
                    const int64_t len = o.read_len;
                    memset(&o, 0, sizeof(o));
                    o.status = SA_RAW_MAP_LENGTH;
                    o.read_len = len;
                    o.mom_shift = shift[j];
                    o.mom_scale = scale[j];
                }
            });
            rc = bad;
        }
    }
done:
    if (kernel_ms_out) *kernel_ms_out = (double) run.kms + ea_ms + (double) fin_ms;
    for (size_t j = 0; j < nj; j++) free(pairs[j]);
    if (rc != SA_OK) {
        for (size_t j = 0; j < nj; j++) { free(out[j].events4); memset(&out[j], 0, sizeof(out[j])); }
    }
    return rc;
}
