// sa_guide.hip -- guide alignment of a basecalled read to its reference window on the GPU.
//
// What it replaces: the `bwa mem` call of the reference's driver (src/signalalign/signalAlignment.py:262-305), whose one use
// here is the exonerate cigar that anchors the pair-HMM's band.  The caller names the window (sa_guide.c places the read inside
// it); this stage aligns the two: local alignment, affine gaps, integer scores, inside a Suzuki-Kasahara adaptive band -- the
// banding of sa_ea.hip on nucleotides.
//
// The rules ("Guide alignment"; restated band by band in tests/guide_ref.py, and the device equals that bit for bit):
//   bands     anti-diagonals of the (read+1) x (ref+1) matrix, W cells wide; the cell of offset o in a band with origin
//             (ll_i, ll_j) is (ll_i - o, ll_j + o); band 0 has origin (W/2, diag - W/2), i.e. offset W/2 is cell (0, diag)
//   steering  band b+1 moves right (ll_j + 1) when H at offset W-1 of band b is higher than at offset 0, down (ll_i + 1) when it
//             is lower, opposite to the previous move on a tie (the move before band 1 counts as right); once the cell of offset
//             W/2 has reached the last row the move is right, once it has reached the last column it is down, and the band that
//             has reached both is the last one: n_bands = read_len + ref_len - diag moves
//   cells     outside the matrix: -inf; row 0 and column 0: H = E = F = 0; before band 1 nothing else exists (-inf); a neighbour
//             outside its band: -inf; else
//               E = max(0, H(i, j-1) - (open + ext), E(i, j-1) - ext)   "E extended" when the second is strictly higher
//               F = max(0, H(i-1, j) - (open + ext), F(i-1, j) - ext)   "F extended" likewise
//               H = max(0, H(i-1, j-1) + s, E, F)    source: stop when H = 0, else diagonal before E before F
//   end       first maximum of H in band order, then offset order; traceback to the first cell with H = 0
//
// Mapping (that of k_event_align): one wave per read, lane l owns offsets l, l + 64, ... of the band, H / E / F of the previous
// band, the two candidates for the diagonal neighbour and the cells' letter codes stay in registers; neighbours are DPP wave
// rotates with the lane 63 -> next rep hand-over patched; the move is a wave-uniform scalar, so the shifts are static; fresh
// letter codes come out of a 64-entry register buffer per sequence by v_readlane.  The trace is 4 bits per cell (2 bits source,
// E extended, F extended), one coalesced store per band, plus the band's ll_i.  The walk back stages 64 bands in LDS.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "sa_io.h"
#include "sa_scratch.h"

#define GD_NEG (-(1 << 30))
#define GD_MAX_LEN (1 << 24)

struct GdJob {
    long long code_off;    // read codes at codes + code_off, reference codes behind them
    long long trace_off;   // bytes into the trace plane
    long long ll_off;      // ints
    long long op_off;      // packed operations (type << 30 | length), filled from the back
    int n, m, diag, n_bands, op_cap;
};
struct GdRes {
    int status, score, read_start, read_end, ref_start, ref_end, n_ops, pad;
};
struct GdPlan {
    const GdJob *jobs;
    const unsigned char *codes;   // 0..3 = ACGT, 4 = anything else
    unsigned char *trace;
    int *ll;
    unsigned int *ops;
    GdRes *res;
    int match, mismatch, gap_first, gap_ext, amb;   // gap_first = open + ext
};

__device__ __forceinline__ int gd_from_next(int v) { return __builtin_amdgcn_mov_dpp(v, 0x134, 0xF, 0xF, false); }  // lane l <- l+1
__device__ __forceinline__ int gd_from_prev(int v) { return __builtin_amdgcn_mov_dpp(v, 0x13C, 0xF, 0xF, false); }  // lane l <- l-1
// x[o] <- x[o + 1] over the 64 R offsets, `fill` enters at the last one
template <int R>
__device__ __forceinline__ void gd_shl(int (&x)[R], int fill, int lane) {
    int n[R];
#pragma unroll
    for (int r = 0; r < R; r++) n[r] = gd_from_next(x[r]);   // n[r][63] = x[r][0]
#pragma unroll
    for (int r = 0; r < R; r++) x[r] = lane == 63 ? (r + 1 < R ? n[r + 1 < R ? r + 1 : r] : fill) : n[r];
}
// x[o] <- x[o - 1], `fill` enters at offset 0
template <int R>
__device__ __forceinline__ void gd_shr(int (&x)[R], int fill, int lane) {
    int p[R];
#pragma unroll
    for (int r = 0; r < R; r++) p[r] = gd_from_prev(x[r]);   // p[r][0] = x[r][63]
#pragma unroll
    for (int r = 0; r < R; r++) x[r] = lane == 0 ? (r > 0 ? p[r > 0 ? r - 1 : 0] : fill) : p[r];
}
// a loaded value passed through a VALU move, so that the wait for the load sits in the refill branch (see sa_ea.hip: ea_settle)
__device__ __forceinline__ int gd_settle(int v) {
    int w;
    asm volatile("v_mov_b32 %0, %1" : "=v"(w) : "v"(v));
    return w;
}
// H of a cell nothing has been computed for: 0 on row 0 and column 0, -inf elsewhere (outside the matrix, or before band 1)
__device__ __forceinline__ int gd_border(int i, int j, int n, int m) {
    return (i >= 0 && i <= n && j >= 0 && j <= m && (i == 0 || j == 0)) ? 0 : GD_NEG;
}
__device__ __forceinline__ int gd_code(const unsigned char *s, int idx, int len) {
    return (idx >= 0 && idx < len) ? (int) s[idx] : 4;
}

template <int R>
__global__ __launch_bounds__(64) void k_guide_align(GdPlan P, int n_jobs) {
    constexpr int W = 64 * R, HALF = W / 2;
    constexpr int RB = R <= 2 ? 64 : 128;   // bytes of a band's trace row: a byte (two nibbles) or a half-word (four) per lane
    const int job = blockIdx.x;
    if (job >= n_jobs) return;
    const int lane = threadIdx.x;
    const GdJob J = P.jobs[job];
    const int n = J.n, m = J.m, diag = J.diag, n_bands = J.n_bands;
    const unsigned char *rd = P.codes + J.code_off, *rf = rd + n;
    unsigned char *trace = P.trace + J.trace_off;
    int *ll = P.ll + J.ll_off;
    const int s_match = P.match, s_mis = P.mismatch, s_amb = P.amb, g_first = P.gap_first, g_ext = P.gap_ext;

    int ll_i = HALF, ll_j = diag - HALF;
    int Hp[R], Ep[R], Fp[R], dd[R], dr[R], rc[R], fc[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int o = lane + 64 * r, i = ll_i - o, j = ll_j + o;
        Hp[r] = gd_border(i, j, n, m);
        Ep[r] = Hp[r]; Fp[r] = Hp[r];
        dr[r] = gd_border(i - 1, j, n, m);       // band -1 as band 1's diagonal if band 1 moves right ...
        dd[r] = gd_border(i, j - 1, n, m);       // ... and if it moves down
        rc[r] = gd_settle(gd_code(rd, i - 1, n));
        fc[r] = gd_settle(gd_code(rf, j - 1, m));
    }
    if (R <= 2) trace[lane] = 0x33;
    else ((unsigned short *) trace)[lane] = 0x3333;
    if (lane == 0) ll[0] = ll_i;
    // streams: the next read letter to enter at offset 0 (a down move), the next reference letter to enter at offset W-1 (right)
    int es = ll_i, eb_base = es, ks = ll_j + W - 1, kb_base = ks;
    int eb = gd_settle(gd_code(rd, eb_base + lane, n)), kb = gd_settle(gd_code(rf, kb_base + lane, m));
    int lo = __builtin_amdgcn_readlane(Hp[0], 0), hi = __builtin_amdgcn_readlane(Hp[R - 1], 63);
    int best = 0, best_b = 0, best_o = 0;
    int downs = 0, rights = 0;
    bool prev_right = true;
    for (int b = 1; b <= n_bands; b++) {
        bool right;
        if (downs == n) right = true;
        else if (diag + rights == m) right = false;
        else if (hi != lo) right = hi > lo;
        else right = !prev_right;
        int upH[R], upF[R], lfH[R], lfE[R], dg[R];
        if (right) {
            if (ks - kb_base == 64) {
                kb_base += 64;
                kb = gd_settle(gd_code(rf, kb_base + lane, m));
            }
            const int fresh = __builtin_amdgcn_readlane(kb, ks - kb_base);
            ks++; ll_j++; rights++;
            gd_shl<R>(fc, fresh, lane);
#pragma unroll
            for (int r = 0; r < R; r++) { lfH[r] = Hp[r]; lfE[r] = Ep[r]; upH[r] = Hp[r]; upF[r] = Fp[r]; dg[r] = dr[r]; }
            gd_shl<R>(upH, GD_NEG, lane);          // prev[o + 1]; offset W does not exist
            gd_shl<R>(upF, GD_NEG, lane);
        } else {
            if (es - eb_base == 64) {
                eb_base += 64;
                eb = gd_settle(gd_code(rd, eb_base + lane, n));
            }
            const int fresh = __builtin_amdgcn_readlane(eb, es - eb_base);
            es++; ll_i++; downs++;
            gd_shr<R>(rc, fresh, lane);
#pragma unroll
            for (int r = 0; r < R; r++) { lfH[r] = Hp[r]; lfE[r] = Ep[r]; upH[r] = Hp[r]; upF[r] = Fp[r]; dg[r] = dd[r]; }
            gd_shr<R>(lfH, GD_NEG, lane);          // prev[o - 1]; offset -1 does not exist
            gd_shr<R>(lfE, GD_NEG, lane);
        }
        unsigned int word = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
            dr[r] = upH[r];                        // for the NEXT band: band b-1 at the up neighbour's offset if it moves right ...
            dd[r] = lfH[r];                        // ... at the left neighbour's if it moves down
            const int o = lane + 64 * r, i = ll_i - o, j = ll_j + o;
            const bool inside = i >= 0 && i <= n && j >= 0 && j <= m;
            const bool interior = inside && i >= 1 && j >= 1;
            const int e_open = lfH[r] - g_first, e_ext = lfE[r] - g_ext;
            const int f_open = upH[r] - g_first, f_ext = upF[r] - g_ext;
            int E = e_ext > e_open ? e_ext : e_open;
            int F = f_ext > f_open ? f_ext : f_open;
            E = E > 0 ? E : 0;
            F = F > 0 ? F : 0;
            const int s = (rc[r] > 3 || fc[r] > 3) ? s_amb : (rc[r] == fc[r] ? s_match : s_mis);
            const int d = dg[r] + s;
            int H = d > E ? d : E;
            H = F > H ? F : H;
            H = H > 0 ? H : 0;
            unsigned int nib = H <= 0 ? 3u : (H == d ? 0u : (H == E ? 1u : 2u));
            nib |= (e_ext > e_open ? 4u : 0u) | (f_ext > f_open ? 8u : 0u);
            const int off_val = inside ? 0 : GD_NEG;   // row 0, column 0: zero; outside the matrix: -inf
            H = interior ? H : off_val;
            E = interior ? E : off_val;
            F = interior ? F : off_val;
            nib = interior ? nib : 3u;
            word |= nib << (4 * r);
            if (H > best) { best = H; best_b = b; best_o = o; }
            Hp[r] = H; Ep[r] = E; Fp[r] = F;
        }
        if (R <= 2) trace[(long long) b * RB + lane] = (unsigned char) word;
        else ((unsigned short *) (trace + (long long) b * RB))[lane] = (unsigned short) word;
        if (lane == 0) ll[b] = ll_i;
        lo = __builtin_amdgcn_readlane(Hp[0], 0);
        hi = __builtin_amdgcn_readlane(Hp[R - 1], 63);
        prev_right = right;
    }
    // the end cell: first maximum in band order, then offset order
    for (int off = 32; off > 0; off >>= 1) {
        const int ob = __shfl_xor(best, off, 64), obb = __shfl_xor(best_b, off, 64), obo = __shfl_xor(best_o, off, 64);
        if (ob > best || (ob == best && (obb < best_b || (obb == best_b && obo < best_o)))) { best = ob; best_b = obb; best_o = obo; }
    }
    best = __builtin_amdgcn_readfirstlane(best);
    best_b = __builtin_amdgcn_readfirstlane(best_b);
    best_o = __builtin_amdgcn_readfirstlane(best_o);
    GdRes res;
    res.status = 0; res.score = best; res.read_start = res.read_end = res.ref_start = res.ref_end = 0; res.n_ops = 0; res.pad = 0;
    if (best <= 0) {
        res.status = SA_GUIDE_NO_ALIGNMENT;
        if (lane == 0) P.res[job] = res;
        return;
    }
    __threadfence();   // trace rows and ll[] written by other lanes, read below
    __syncthreads();
    // Traceback by the whole wave, as k_event_align's: the trace rows and origins of 64 consecutive bands are staged with coalesced
    // loads (rows into LDS, origins one per lane), the walk inside the block is LDS reads and v_readlane.  Every step checks the
    // band index against [0, n_bands] and the offset against [0, W) before anything is addressed with them.
    __shared__ unsigned int tr_rows[64 * RB / 4];
    unsigned int *ops = P.ops + J.op_off;
    const int op_cap = J.op_cap;
    int ci = __builtin_amdgcn_readfirstlane(ll[best_b]) - best_o, cj = best_b + diag - ci;
    res.read_end = ci; res.ref_end = cj;
    int state = 0, st = 0, n_ops = 0, cur_type = -1, cur_len = 0;
    bool go = true;
    while (go) {
        const int b_hi = ci + cj - diag;
        if (b_hi < 0 || b_hi > n_bands) { st |= SA_GUIDE_TRACE; break; }
        const int b_lo = b_hi - 63 > 0 ? b_hi - 63 : 0;
        const unsigned int *src = (const unsigned int *) (trace + (long long) b_lo * RB);
        const int n_words = (b_hi - b_lo + 1) * (RB / 4);
        __syncthreads();
        {
            unsigned int w[RB / 4];
#pragma unroll
            for (int q = 0; q < RB / 4; q++) w[q] = lane + 64 * q < n_words ? src[lane + 64 * q] : 0x33333333u;
#pragma unroll
            for (int q = 0; q < RB / 4; q++) tr_rows[lane + 64 * q] = w[q];
        }
        const int llv = (b_hi - lane >= b_lo) ? ll[b_hi - lane] : 0;   // ll_i of band b_hi - lane
        __syncthreads();
        for (;;) {
            const int b = ci + cj - diag;
            if (b < b_lo) {
                if (b < 0) { st |= SA_GUIDE_TRACE; go = false; }
                break;
            }
            const int o = __builtin_amdgcn_readlane(llv, b_hi - b) - ci;
            if (o < 0 || o >= W) { st |= SA_GUIDE_TRACE; go = false; break; }
            if (o == 0 || o == W - 1) st |= SA_GUIDE_BAND_EDGE;
            const int cell = (b - b_lo) * 64 + (o & 63);
            unsigned int v;
            if (R <= 2) v = ((const unsigned char *) tr_rows)[cell];
            else v = ((const unsigned short *) tr_rows)[cell];
            const int nib = (__builtin_amdgcn_readfirstlane((int) v) >> (4 * (o >> 6))) & 15;
            int type;
            if (state == 0) {
                const int from = nib & 3;
                if (from == 3) { go = false; break; }
                if (from == 1) { state = 1; continue; }
                if (from == 2) { state = 2; continue; }
                type = 0; ci--; cj--;
            } else if (state == 1) {
                type = 1; cj--;
                state = (nib & 4) ? 1 : 0;
            } else {
                type = 2; ci--;
                state = (nib & 8) ? 2 : 0;
            }
            if (type == cur_type) cur_len++;
            else {
                if (cur_type >= 0) {
                    if (n_ops >= op_cap) { st |= SA_GUIDE_TRACE; go = false; break; }
                    if (lane == 0) ops[op_cap - 1 - n_ops] = ((unsigned int) cur_type << 30) | (unsigned int) cur_len;
                    n_ops++;
                }
                cur_type = type; cur_len = 1;
            }
        }
    }
    if (cur_type >= 0 && n_ops < op_cap) {
        if (lane == 0) ops[op_cap - 1 - n_ops] = ((unsigned int) cur_type << 30) | (unsigned int) cur_len;
        n_ops++;
    }
    res.read_start = ci; res.ref_start = cj;
    res.status = st;
    res.n_ops = (st & SA_GUIDE_TRACE) ? 0 : n_ops;
    if (lane == 0) P.res[job] = res;
}

enum { GD_WS, GD_TRACE, GD_IN, GD_RES };
static SaScratch g_gd_ws;

extern "C" void sa_guide_release(void) {
    std::lock_guard<std::mutex> guard(g_gd_ws.mu);
    g_gd_ws.release();
}

static size_t gd_row_bytes(int band) { return band <= 128 ? 64 : 128; }

// one slice of the batch, as dense arrays: its jobs share the trace plane
static int gd_run_slice(SaScratch &W, const sa_guide_job_t *jobs, std::vector<GdJob> &sj, const sa_guide_params_t &prm,
                        std::vector<GdRes> &res, std::vector<std::vector<unsigned int>> &ops, double *kernel_ms) {
    int rc = SA_OK;
    const size_t nj = sj.size();
    size_t code_tot = 0, ll_tot = 0, op_tot = 0, trace_tot = 0;
    const size_t rb = gd_row_bytes(prm.band);
    for (GdJob &J : sj) {
        J.code_off = (long long) code_tot; code_tot += (size_t) J.n + (size_t) J.m;
        J.ll_off = (long long) ll_tot; ll_tot += (size_t) J.n_bands + 1;
        J.op_off = (long long) op_tot; op_tot += (size_t) J.op_cap;
        J.trace_off = (long long) trace_tot; trace_tot += sa_up256(((size_t) J.n_bands + 1) * rb);
    }
    const size_t in_bytes = sa_up256(sizeof(GdJob) * nj) + code_tot;
    if ((rc = W.pin(GD_IN, in_bytes)) != SA_OK) return rc;
    memcpy(W.at(GD_IN), sj.data(), sizeof(GdJob) * nj);
    unsigned char *codes = (unsigned char *) W.at(GD_IN) + sa_up256(sizeof(GdJob) * nj);
    sa_parallel_for(nj, [&](size_t k) {
        const sa_guide_job_t &jb = jobs[k];
        unsigned char *dst = codes + sj[k].code_off;
        for (int64_t i = 0; i < jb.read_len; i++) dst[i] = (unsigned char) sa_base_code(jb.read[i]);
        dst += jb.read_len;
        for (int64_t i = 0; i < jb.ref_len; i++) dst[i] = (unsigned char) sa_base_code(jb.ref[i]);
    });
    // device workspace: [jobs, codes] (the upload image) | ll | operations, results; the trace plane is a slot of its own.  The
    // operations and the results are ONE entry: they come back in one copy
    SaLayout L;
    const size_t back_bytes = sa_up256(sizeof(unsigned int) * op_tot) + sizeof(GdRes) * nj;
    const size_t o_in = L.add(in_bytes), o_ll = L.add(sizeof(int) * ll_tot), o_ops = L.add(back_bytes),
                 o_res = o_ops + sa_up256(sizeof(unsigned int) * op_tot);
    float kms = 0;
    GdPlan P;
    memset(&P, 0, sizeof(P));
    if ((rc = W.dev(GD_WS, L.end)) != SA_OK) return rc;
    rc = W.dev(GD_TRACE, trace_tot);
    if (rc == SA_ENOMEM) {   // the caching allocator's parked blocks count as free memory: hand them back and try once more
        g_sa_pool.release(SaPool::DEVICE);
        rc = W.dev(GD_TRACE, trace_tot);
    }
    if (rc != SA_OK) return rc;
    if ((rc = W.pin(GD_RES, back_bytes)) != SA_OK) return rc;
    {
        char *d = (char *) W.at(GD_WS);
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_in, W.at(GD_IN), in_bytes, hipMemcpyHostToDevice, 0));
        P.jobs = (const GdJob *) (d + o_in);
        P.codes = (const unsigned char *) (d + o_in + sa_up256(sizeof(GdJob) * nj));
        P.trace = (unsigned char *) W.at(GD_TRACE);
        P.ll = (int *) (d + o_ll);
        P.ops = (unsigned int *) (d + o_ops);
        P.res = (GdRes *) (d + o_res);
        P.match = prm.match; P.mismatch = prm.mismatch; P.amb = prm.ambiguous;
        P.gap_first = prm.gap_open + prm.gap_extend; P.gap_ext = prm.gap_extend;
        SA_HIP_GOTO_DONE(W.time_begin());
        const dim3 grid((unsigned) nj), block(64);
        switch (prm.band / 64) {
            case 1: hipLaunchKernelGGL(k_guide_align<1>, grid, block, 0, 0, P, (int) nj); break;
            case 2: hipLaunchKernelGGL(k_guide_align<2>, grid, block, 0, 0, P, (int) nj); break;
            case 3: hipLaunchKernelGGL(k_guide_align<3>, grid, block, 0, 0, P, (int) nj); break;
            default: hipLaunchKernelGGL(k_guide_align<4>, grid, block, 0, 0, P, (int) nj); break;
        }
        SA_HIP_GOTO_DONE(W.time_end());
        SA_HIP_GOTO_DONE(hipMemcpyAsync(W.at(GD_RES), d + o_ops, back_bytes, hipMemcpyDeviceToHost, 0));
        SA_HIP_GOTO_DONE(hipStreamSynchronize(0));
        SA_HIP_GOTO_DONE(W.time_ms(&kms));
    }
    *kernel_ms += (double) kms;
    {
        const unsigned int *h_ops = (const unsigned int *) W.at(GD_RES);
        const GdRes *h_res = (const GdRes *) ((const char *) W.at(GD_RES) + (o_res - o_ops));
        for (size_t k = 0; k < nj; k++) {
            GdRes r = h_res[k];
            if (r.n_ops < 0 || r.n_ops > sj[k].op_cap) { r.n_ops = 0; r.status |= SA_GUIDE_TRACE; }
            res[k] = r;
            const unsigned int *src = h_ops + sj[k].op_off + (sj[k].op_cap - r.n_ops);
            ops[k].assign(src, src + r.n_ops);
        }
    }
done:
    return rc;
}

extern "C" int sa_guide_align_batch(const sa_guide_job_t *jobs, int64_t n_jobs, const sa_guide_params_t *params, int device,
                                    unsigned flags, sa_guide_result_t *results_out, int32_t **op_type_out, int64_t **op_len_out,
                                    double *kernel_ms_out) {
    (void) flags;
    if ((!jobs && n_jobs > 0) || n_jobs < 0 || !results_out || !op_type_out || !op_len_out) return SA_EINVAL;
    sa_guide_params_t prm = {2, -4, 4, 2, -1, 128, 0.5};
    if (params) prm = *params;
    if (prm.band < 64 || prm.band > 256 || prm.band % 64 != 0) return SA_EINVAL;
    const int32_t sc[5] = {prm.match, prm.mismatch, prm.gap_open, prm.gap_extend, prm.ambiguous};
    for (int i = 0; i < 5; i++)
        if (sc[i] < -1000 || sc[i] > 1000) return SA_EINVAL;
    if (prm.gap_extend < 1 || prm.gap_open < 0 || !(prm.min_read_fraction >= 0.0 && prm.min_read_fraction <= 1.0)) return SA_EINVAL;
    for (int64_t j = 0; j < n_jobs; j++) {
        const sa_guide_job_t &jb = jobs[j];
        if (jb.read_len < 0 || jb.ref_len < 0 || jb.read_len > GD_MAX_LEN || jb.ref_len > GD_MAX_LEN ||
            (jb.read_len > 0 && !jb.read) || (jb.ref_len > 0 && !jb.ref))
            return SA_EINVAL;
    }
    *op_type_out = nullptr;
    *op_len_out = nullptr;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    int rc = sa_device_check(device);
    if (rc) return rc;
    std::vector<GdJob> hj((size_t) n_jobs);
    std::vector<GdRes> res((size_t) n_jobs);
    std::vector<std::vector<unsigned int>> ops((size_t) n_jobs);
    std::vector<int64_t> live;   // the jobs that reach the device: an empty job is answered here
    const size_t rb = gd_row_bytes(prm.band);
    for (int64_t j = 0; j < n_jobs; j++) {
        const sa_guide_job_t &jb = jobs[j];
        GdJob &J = hj[(size_t) j];
        memset(&J, 0, sizeof(J));
        memset(&res[(size_t) j], 0, sizeof(GdRes));
        if (jb.read_len == 0 || jb.ref_len == 0) { res[(size_t) j].status = SA_GUIDE_EMPTY; continue; }
        J.n = (int) jb.read_len; J.m = (int) jb.ref_len;
        J.diag = (int) (jb.diag < 0 ? 0 : (jb.diag > jb.ref_len ? jb.ref_len : jb.diag));
        J.n_bands = J.n + J.m - J.diag;
        J.op_cap = J.n_bands + 2;
        live.push_back(j);
    }
    SaScratch &W = g_gd_ws;
    std::lock_guard<std::mutex> guard(W.mu);
    double kms = 0.0;
    if (!live.empty()) {
        // slices: consecutive jobs whose trace fits three quarters of what is free (this workspace's own plane counts as free)
        int64_t free_b = 0, total_b = 0;
        if ((rc = sa_device_memory(device, &free_b, &total_b)) != SA_OK) return rc;
        size_t budget = (size_t) ((double) ((size_t) free_b + W.cap(GD_TRACE)) * 0.75);
        if ((rc = W.rebind(device)) != SA_OK) return rc;
        if (const char *e = getenv("SA_GUIDE_TRACE_MB")) budget = (size_t) (atof(e) * 1048576.0);   // (tests: several slices)
        // the jobs of a slice are compacted: gd_run_slice works on dense arrays
        std::vector<sa_guide_job_t> cj;
        std::vector<GdJob> ch;
        std::vector<int64_t> who;
        size_t a = 0;
        while (a < live.size() && rc == SA_OK) {
            size_t bytes = 0, z = a;
            while (z < live.size()) {
                const size_t t = sa_up256(((size_t) hj[(size_t) live[z]].n_bands + 1) * rb);
                if (z > a && bytes + t > budget) break;
                bytes += t;
                z++;
            }
            if (bytes > budget && !getenv("SA_GUIDE_TRACE_MB")) { rc = SA_ENOMEM; break; }
            cj.clear(); ch.clear(); who.clear();
            for (size_t q = a; q < z; q++) { cj.push_back(jobs[live[q]]); ch.push_back(hj[(size_t) live[q]]); who.push_back(live[q]); }
            std::vector<GdRes> sres(z - a);
            std::vector<std::vector<unsigned int>> sops(z - a);
            rc = gd_run_slice(W, cj.data(), ch, prm, sres, sops, &kms);
            for (size_t q = 0; q < z - a && rc == SA_OK; q++) { res[(size_t) who[q]] = sres[q]; ops[(size_t) who[q]].swap(sops[q]); }
            a = z;
        }
    }
    if (rc != SA_OK) return rc;
    if (kernel_ms_out) *kernel_ms_out = kms;
    size_t tot = 0;
    for (int64_t j = 0; j < n_jobs; j++) tot += ops[(size_t) j].size();
    int32_t *ot = (int32_t *) malloc(sizeof(int32_t) * (tot ? tot : 1));
    int64_t *ol = (int64_t *) malloc(sizeof(int64_t) * (tot ? tot : 1));
    if (!ot || !ol) { free(ot); free(ol); return SA_ENOMEM; }
    size_t at = 0;
    for (int64_t j = 0; j < n_jobs; j++) {
        const GdRes &r = res[(size_t) j];
        sa_guide_result_t &o = results_out[j];
        o.status = r.status;
        o.score = r.score; o.read_start = r.read_start; o.read_end = r.read_end; o.ref_start = r.ref_start; o.ref_end = r.ref_end;
        o.op_first = (int64_t) at; o.n_ops = (int64_t) ops[(size_t) j].size();
        for (unsigned int v : ops[(size_t) j]) { ot[at] = (int32_t) (v >> 30); ol[at] = (int64_t) (v & 0x3fffffffu); at++; }
        if (!(r.status & (SA_GUIDE_NO_ALIGNMENT | SA_GUIDE_EMPTY)) &&
            (double) (r.read_end - r.read_start) < prm.min_read_fraction * (double) jobs[j].read_len)
            o.status |= SA_GUIDE_SHORT;
    }
    *op_type_out = ot;
    *op_len_out = ol;
    return SA_OK;
}
