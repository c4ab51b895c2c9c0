// sa_dplan.inc -- the planner on the device.  Included by sa_hip.hip.
//
// The host planner builds, per read, the band table (band_construct impl/pairwiseAligner.c:195-246), the packed band words of
// the register kernels, the traceback schedule and the total-probability checkpoints (getPosteriorProbsWithBanding :1450-1590,
// the schedule only) and uploads ~400 KB per read.  For the common batch -- no anchor gap large enough to split a matrix
// (getSplitPoints :1886-1937), Gaussian or HDP emissions through the default kernels -- the same arrays are built here from
// what a read really consists of: its reference letters, event means and anchors (~60 KB).  What is computed per diagonal,
// segment, path and region is sa_plan_rules.h, the one statement both planners compile, and what a batch must be to be planned
// at all are the predicates of sa_internal.h; this file is how the device walks a read: one workgroup per read, strided loops
// over the diagonals (box of a diagonal by binary search over the anchors instead of the host's running index), prefix sums by
// workgroup scans.  The result is bit-identical to the host planner's (tests/test_gpu_dplan.py compares every array), so which
// planner ran is invisible downstream.  Whatever is not covered (split matrices, SA_FLAG_EXACT, the two-distribution
// emissions, a region the rules route to SA_KIND_GENERIC) takes the host planner as before.
//
// Passes: k_dplan_region (one workgroup per read: k-mer ids, band rows, offsets, packed words, schedule into per-read
// slabs) -> k_dplan_scan (one workgroup: running sums over the reads, forward-storage passes) -> k_dplan_compact (per
// read: segments and checkpoints to their final places).  Only the small arrays (regions, segments, per-read counts)
// come back to the host, which needs them for the launch lists.

#define DPLAN_NT 256

struct sa_djob_t {      // per read, written by the host (64 bytes)
    int lX, lY, n_anchors, bits;     // bits: 1 = some ambiguity letter (several paths per cell), 2 / 4 = left / right end NOT ragged
                                     // (sa_job_t.ends: alignmentHasRaggedLeftEnd / RightEnd, impl/pairwiseAligner.c:2052-2080)
    long long ref_off;          // into the packed reference letters
    long long anc_off;          // into the packed anchors (x[], y[] as int32)
    long long row_off, pk_off, poff_off, pid_off, ev_off;
    long long seg_slab, ck_slab;
    double scale, shift, var, lvar;
};

struct sa_dcount_t {    // per read, written by k_dplan_region
    long long n_ck, n_vbuf, n_cand, n_bscratch;
    double cells_fwd, cells_bwd;
    int status, pad;            // 0, or an SA_E* code (the batch then takes the host planner, which reports it properly)
};

struct sa_dtotals_t {
    long long n_segs, n_cks, n_vbuf, n_cand, n_bscratch, max_chunk_cellpaths;
    long long n_fast, n_ring;
    int n_chunks, status;
};

// SA_FLAG_INPUTS_IN_HOST_BLOCK: where a read's event records and anchor arrays lie inside the block image in HBM
struct sa_dsrc_t {
    long long ev_off, ax_off, ay_off;   // bytes from the image's first byte
    long long ev_dst;                   // first event mean of the read in the batch's event array
    int stride, n_events;               // doubles per event record; events
};

struct DPlanArgs {
    const int *ingest_status;   // per read, written by k_dplan_ingest (nullptr: the host checked and packed the reads)
    const sa_djob_t *jobs;
    const unsigned char *refs;
    const int *anchors;
    sa_region_t *regions;
    sa_row_t *rows;
    int *pk;
    int *poff;
    int *pid;
    sa_seg_t *seg_slab;
    sa_ck_t *ck_slab;
    sa_dcount_t *counts;
    long long expansion, trace_back, min_diags;
    int k, n_alpha;
    sa_route_in_t route;        // the batch's part of the routing inputs (flags, model, environment); the kernel adds each region's
    sa_prec_t *prec;            // per-path neighbour records (batches with ambiguous letters only)
    unsigned char lut[256];     // letter -> digit of the sorted alphabet, 255: not in it
    unsigned char amb_n[256];   // options of an ambiguity letter, 1 for every other letter
    unsigned short amb_off[256];// where its options' digits start in amb_dig
    unsigned char amb_dig[512]; // digits of the options, letter after letter
};

// exclusive workgroup scan of one value per thread; returns the workgroup total through `total`
__device__ __forceinline__ long long dp_block_scan(long long v, long long *lds_wave /* >= 4 */, long long &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        long long o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    __syncthreads();
    if (lane == 63) lds_wave[wave] = incl;
    __syncthreads();
    long long before = 0, tot = 0;
    for (int w = 0; w < DPLAN_NT / 64; w++) {
        const long long s = lds_wave[w];
        if (w < wave) before += s;
        tot += s;
    }
    total = tot;
    return before + incl - v;
}

// SA_FLAG_INPUTS_IN_HOST_BLOCK: the caller's block arrived in HBM with ONE DMA (pinned source); this kernel does on the device
// what the host otherwise does per read with the caller's arrays: anchors checked (inside the matrix, strictly increasing, no gap
// that would split the matrix: the conditions of dplan_front) and narrowed to int32, event means gathered out of their records.
// A read that fails sends the batch to the host planner through its status word, as every other refusal of this planner does.
__global__ __launch_bounds__(DPLAN_NT) void k_dplan_ingest(const sa_djob_t *__restrict__ jobs, const sa_dsrc_t *__restrict__ src,
                                                           const char *__restrict__ blk, int *__restrict__ anchors,
                                                           int *__restrict__ status, long long limit) {
    __shared__ int s_bad;
    const int r = blockIdx.x, t = threadIdx.x;
    const sa_djob_t J = jobs[r];
    const sa_dsrc_t S = src[r];
    if (t == 0) s_bad = 0;
    __syncthreads();
    const long long *ax = reinterpret_cast<const long long *>(blk + S.ax_off), *ay = reinterpret_cast<const long long *>(blk + S.ay_off);
    int *an = anchors + J.anc_off;
    const int na = J.n_anchors;
    bool bad = false;
    for (int i = t; i < na; i += DPLAN_NT) {
        const long long nx = ax[i], ny = ay[i];
        const long long px = i ? ax[i - 1] + 1 : 0, py = i ? ay[i - 1] + 1 : 0;   // one past the previous anchor
        bad = bad || !(nx >= px && ny >= py && nx < J.lX && ny < J.lY) || (nx - px) * (ny - py) > limit;
        an[i] = (int) nx;
        an[na + i] = (int) ny;
    }
    if (t == 0) {
        const long long px = na ? ax[na - 1] + 1 : 0, py = na ? ay[na - 1] + 1 : 0;
        bad = bad || ((long long) J.lX - px) * ((long long) J.lY - py) > limit;
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (t == 0) status[r] = s_bad;
}
// ... and the event means out of their records (not needed by the planning kernels: when the caller's block holds the event
// records apart from the anchors, they travel and are gathered on the batch's own stream, behind the plan)
__global__ __launch_bounds__(DPLAN_NT) void k_dplan_events(const sa_dsrc_t *__restrict__ src, const char *__restrict__ blk,
                                                           double *__restrict__ ev_out) {
    const int r = blockIdx.x, t = threadIdx.x;
    const sa_dsrc_t S = src[r];
    const double *evr = reinterpret_cast<const double *>(blk + S.ev_off);
    double *evo = ev_out + S.ev_dst;
    for (long long i = t; i < S.n_events; i += DPLAN_NT) evo[i] = evr[i * (long long) S.stride];
}

#define DPLAN_LDS_ANCHORS 8192
// dynamic LDS: lds_anchors ints (the longest anchor list of the batch, at most DPLAN_LDS_ANCHORS) -- not more than needed:
// the planner of the NEXT batch runs beside the sweeps of the current one and has to find room on their CUs
__global__ __launch_bounds__(DPLAN_NT) void k_dplan_region(DPlanArgs A, int n_jobs, int lds_anchors) {
    extern __shared__ int s_sum[];
    __shared__ long long s_wave[DPLAN_NT / 64];
    __shared__ long long s_red[4];
    __shared__ int s_flag[2];
    const int r = blockIdx.x;
    if (r >= n_jobs) return;
    const int t = threadIdx.x;
    const sa_djob_t J = A.jobs[r];
    const long long lX = J.lX, lY = J.lY, N = lX + lY, e = A.expansion;
    const unsigned char *ref = A.refs + J.ref_off;
    const int *ax = A.anchors + J.anc_off, *ay = ax + J.n_anchors;
    sa_row_t *rows = A.rows + J.row_off;
    int *pk = A.pk + J.pk_off + SA_PK_PAD;
    int *poff = A.poff + J.poff_off, *pid = A.pid + J.pid_off;
    sa_seg_t *segs = A.seg_slab + J.seg_slab;
    sa_ck_t *cks = A.ck_slab + J.ck_slab;
    if (t == 0) { s_flag[0] = 0; s_flag[1] = 0; }
    __syncthreads();
    if (A.ingest_status && A.ingest_status[r]) {   // anchors this planner does not take: nothing of this read is planned
        if (t == 0) {
            sa_region_t R;
            memset(&R, 0, sizeof(R));
            R.job = r; R.kind = SA_KIND_GENERIC; R.f_cellpaths = 1;
            A.regions[r] = R;
            sa_dcount_t c;
            memset(&c, 0, sizeof(c));
            c.status = SA_EUNSUPPORTED;
            A.counts[r] = c;
        }
        return;
    }
    int status = 0;

    // ---- per-position path tables (hdCell_construct2 impl/pairwiseAligner.c:723-801: every substitution of the window's
    // ambiguity letters, last position varying fastest -- the host planner's expand_kmer lists them from the letters themselves,
    // here from their digits); cell x = 0 is the NULL k-mer ----
    int maxP = 1;
    if (!(J.bits & 1)) {   // no ambiguity letter in this read: one path per cell
        for (long long x = t; x <= lX + 1; x += DPLAN_NT) poff[x] = (int) x;
        for (long long x = t; x <= lX; x += DPLAN_NT) {
            int id = -1;
            if (x >= 1) {
                id = 0;
                for (int i = 0; i < A.k; i++) {
                    const unsigned dgt = A.lut[ref[x - 1 + i]];
                    if (dgt == 255u) status = SA_EALPHABET;
                    id = id * A.n_alpha + (int) dgt;
                }
            }
            pid[x] = id;
        }
    } else {
        if (t == 0) { poff[0] = 0; poff[1] = 1; pid[0] = -1; }
        long long carry = 1;   // poff[1]
        for (long long base = 1; base <= lX; base += DPLAN_NT) {
            const long long x = base + t;
            long long P = 0;
            if (x <= lX) {
                P = 1;
                for (int i = 0; i < A.k; i++) P *= A.amb_n[ref[x - 1 + i]];
                if (P > 255) status = SA_EUNSUPPORTED;
                maxP = P > maxP ? (int) P : maxP;
            }
            long long tot;
            const long long ex = dp_block_scan(P, s_wave, tot);
            if (x <= lX) poff[x + 1] = (int) (carry + ex + P);
            carry += tot;
        }
        for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(maxP, off, 64); maxP = o > maxP ? o : maxP; }
        __syncthreads();
        if ((t & 63) == 0) s_wave[t >> 6] = maxP;
        __syncthreads();
        for (int w = 0; w < DPLAN_NT / 64; w++) maxP = (int) s_wave[w] > maxP ? (int) s_wave[w] : maxP;
        __threadfence_block();
        __syncthreads();
        for (long long x = 1 + t; x <= lX; x += DPLAN_NT) {
            const int p0 = poff[x], P = poff[x + 1] - p0;
            for (int p = 0; p < P; p++) {
                int rem = p, id = 0, mul = 1;
                for (int i = A.k - 1; i >= 0; i--) {   // last position fastest; id = sum digit_i * alpha^(k-1-i)
                    const unsigned char ch = ref[x - 1 + i];
                    const int nn = A.amb_n[ch];
                    unsigned dgt = A.lut[ch];
                    if (nn > 1) { dgt = A.amb_dig[A.amb_off[ch] + rem % nn]; rem /= nn; }
                    if (dgt == 255u) status = SA_EALPHABET;
                    id += (int) dgt * mul;
                    mul *= A.n_alpha;
                }
                pid[p0 + p] = id;
            }
        }
    }

    // ---- band: one (x - y of the first cell, width) per anti-diagonal ----
    // (the anchors' x + y, searched twelve steps deep per diagonal, sit in LDS: from L2 the search is 24 dependent loads)
    const bool sums_in_lds = J.n_anchors <= lds_anchors;
    if (sums_in_lds)
        for (int i = t; i < J.n_anchors; i += DPLAN_NT) s_sum[i] = ax[i] + ay[i] + 2;
    __syncthreads();
    const bool small = sa_band_fits32(N, e);   // (32-bit instance of the band rules: every read the result records can name)
    auto band_rows = [&](auto zero) {
        typedef decltype(zero) I;
        const I lXi = (I) lX, lYi = (I) lY, ei = (I) e, Ni = (I) N;
        for (I d = (I) t; d <= Ni; d += DPLAN_NT) {
            I lo = 0, hi = 0;
            int rc = SA_OK;
            if (d >= 1) {
                // the box of diagonal d: first anchor (in matrix coordinates, +1) whose x + y >= d; behind the last: (lX, lY)
                int a = 0, b = J.n_anchors;
                if (sums_in_lds) {
                    while (a < b) {
                        const int m = (a + b) >> 1;
                        if ((I) s_sum[m] >= d) b = m; else a = m + 1;
                    }
                } else {
                    while (a < b) {
                        const int m = (a + b) >> 1;
                        if ((I) ax[m] + ay[m] + 2 >= d) b = m; else a = m + 1;
                    }
                }
                I x = lXi, y = lYi, p_sum = 0, p_dif = 0, c[4];
                if (a < J.n_anchors) { x = (I) ax[a] + 1; y = (I) ay[a] + 1; }
                if (a >= 1) {
                    const I px = (I) ax[a - 1] + 1, py = (I) ay[a - 1] + 1;
                    p_sum = px + py; p_dif = px - py;
                }
                if constexpr (sizeof(I) == 4) {   // the box's corners c, then the diagonal clipped to it: by the rules' instance for I
                    sa_band_box_32(p_sum, p_dif, x + y, x - y, ei, lXi, lYi, c);
                    rc = sa_clip_row_32(d, c[0], c[1], c[2], c[3], &lo, &hi);
                } else {
                    sa_band_box_64(p_sum, p_dif, x + y, x - y, ei, lXi, lYi, c);
                    rc = sa_clip_row_64(d, c[0], c[1], c[2], c[3], &lo, &hi);
                }
            }
            if (rc) status = rc;
            sa_row_t row;
            row.xmyL = (int) lo;
            row.width = rc == SA_OK ? (int) ((hi - lo) / 2 + 1) : 1;
            row.foff = 0;
            rows[d] = row;
        }
    };
    if (small) band_rows((int32_t) 0); else band_rows((int64_t) 0);
    __threadfence_block();
    __syncthreads();

    // ---- offsets of the diagonals in the forward planes (prefix sum of the widths) ----
    long long carry = 0, max_w = 0;
    for (long long base = 0; base <= N; base += DPLAN_NT) {
        const long long d = base + t;
        long long w = 0;   // cell-paths of the diagonal
        if (d <= N) {
            const sa_row_t rw = rows[d];
            const long long x0 = (d + rw.xmyL) / 2;
            w = (long long) poff[x0 + rw.width] - poff[x0];
        }
        long long tot;
        const long long ex = dp_block_scan(w, s_wave, tot);
        if (d <= N) rows[d].foff = carry + ex;
        max_w = w > max_w ? w : max_w;
        carry += tot;
    }
    const long long total_cells = carry;
    if (t == 0) { rows[N + 1].xmyL = 0; rows[N + 1].width = 0; rows[N + 1].foff = total_cells; }
    __threadfence_block();
    __syncthreads();

    // ---- packed band words, widest window, share of cells on diagonals the register kernels cannot hold ----
    const long long K = sa_band_K(lY);
    long long span = 0, wide_cells = 0;
    auto band_words = [&](auto zero) {
        typedef decltype(zero) I;
        const I Ki = (I) K, Ni = (I) N;
        auto span3 = [&](I dd) { if constexpr (sizeof(I) == 4) return sa_span3_32(rows, dd, Ki); else return sa_span3_64(rows, dd, Ki); };
        for (I d = (I) t; d <= Ni; d += DPLAN_NT) {
            const sa_row_t rw = rows[d];
            const int s3 = span3(d), s3b = span3(d + 2 <= Ni ? d + 2 : Ni);
            pk[d] = sa_pk_word(rw.width, (unsigned) (((I) rw.xmyL + Ki) >> 1), s3, s3b);
            span = s3 > span ? s3 : span;
            if (d >= 1 && s3 > 64) wide_cells += rw.width;
        }
    };
    if (small) band_words((int32_t) 0); else band_words((int64_t) 0);
    {   // workgroup reductions: max width, max span, wide cells, status
        long long tot;
        (void) dp_block_scan(wide_cells, s_wave, tot);
        wide_cells = tot;
        for (int off = 32; off > 0; off >>= 1) {
            const long long o1 = __shfl_xor(max_w, off, 64), o2 = __shfl_xor(span, off, 64);
            max_w = o1 > max_w ? o1 : max_w;
            span = o2 > span ? o2 : span;
        }
        if (status) atomicMax(&s_flag[0], -status);   // (codes are negative)
        __syncthreads();
        if ((t & 63) == 0) { s_wave[t >> 6] = max_w; }
        __syncthreads();
        for (int w = 0; w < DPLAN_NT / 64; w++) max_w = s_wave[w] > max_w ? s_wave[w] : max_w;
        __syncthreads();
        if ((t & 63) == 0) { s_wave[t >> 6] = span; }
        __syncthreads();
        for (int w = 0; w < DPLAN_NT / 64; w++) span = s_wave[w] > span ? s_wave[w] : span;
        __syncthreads();
    }
    status = -s_flag[0];
    const long long max_rowpaths = max_w;
    const double cf = (double) (total_cells - (rows[1].foff - rows[0].foff));

    // ---- which kernels ----
    sa_route_in_t route = A.route;
    route.max_p = maxP; route.max_rowpaths = max_rowpaths; route.cellpaths = total_cells;
    route.lX = lX; route.lY = lY; route.K = K; route.cf = cf; route.wide_cells = (double) wide_cells;
    const int kind = sa_route_kind(&route);
    if (kind == SA_KIND_GENERIC && status == 0) status = SA_EUNSUPPORTED;   // not plannable here: the host planner takes the batch

    // ---- traceback schedule (getPosteriorProbsWithBanding, the schedule only) ----
    long long traced_to = 0, n_seg = 0, n_ck = 0, n_vbuf = 0, n_cand = 0, n_bscr = 0;
    double cb = 0;
    const long long wlimit = e * 2 + 1;
    while (status == 0) {
        // first diagonal d >= traced_to + min_diags with a band at most 2 e + 1 wide, else the last one
        long long dstart = traced_to + A.min_diags, found = N;
        if (dstart < 1) dstart = 1;
        for (long long base = dstart; base < N; base += DPLAN_NT) {
            const long long d = base + t;
            const bool hit = d < N && rows[d].width <= wlimit;
            if (t == 0) s_red[0] = N;
            __syncthreads();
            if (hit) atomicMin((unsigned long long *) &s_red[0], (unsigned long long) d);
            __syncthreads();
            const long long m = s_red[0];
            __syncthreads();
            if (m < N) { found = m; break; }
        }
        const long long d = found;
        const int at_end = d == N;
        const long long from = sa_seg_from(d, at_end, A.trace_back), to = traced_to;
        if (from <= to) { status = SA_EINVAL; break; }
        const long long nck = sa_seg_n_ck(from, to), cap = sa_seg_cand_cap(A.route.hdp, from, to);
        // checkpoints: diagonals from, from - 10, ... > to; their per-cell terms are laid out one after the other
        long long vcarry = 0;
        for (long long base = 0; base < nck; base += DPLAN_NT) {
            const long long c = base + t;
            long long nA = 0, nB = 0, ee = 0;
            if (c < nck) {
                ee = from - SA_CKPT_EVERY * c;
                nA = rows[ee].width;
                nB = ee < d ? rows[ee + 1].width : 0;
            }
            long long tot;
            const long long ex = dp_block_scan(nA + nB, s_wave, tot);
            if (c < nck) {
                sa_ck_t ck;
                ck.voff = n_vbuf + vcarry + ex;
                ck.nA = (int) nA;
                ck.nB = (int) nB;
                cks[n_ck + c] = ck;
                pk[ee] |= SA_PK_CK;
            }
            vcarry += tot;
        }
        if (t == 0) {
            sa_seg_t S;
            S.region = r; S.at_end = at_end;
            S.start = d; S.from = from; S.to = to;
            S.ck_base = n_ck; S.n_ck = (int) nck;
            S.cand_cap = (int) cap;
            S.cand_off = n_cand;
            S.bscratch_off = n_bscr;
            segs[n_seg] = S;
            pk[d] |= SA_PK_FULL;   // (the diagonal a traceback starts on keeps all three forward planes)
        }
        n_cand += cap;
        n_bscr += sa_seg_bscratch(kind, max_rowpaths);
        if (to + 2 <= d) cb += (double) (rows[d + 1].foff - rows[to + 2].foff);
        n_ck += nck;
        n_vbuf += vcarry;
        n_seg++;
        traced_to = from;
        if (at_end) break;
    }
    __threadfence_block();
    __syncthreads();

    // ---- derived flags of the packed words (the words behind diagonal N, and the one in front of diagonal 0, are zero) ----
    const int expect = (A.route.flags & SA_FLAG_EXPECT_INTERNAL) != 0;
    for (long long d = t; d <= N && status == 0; d += DPLAN_NT) {
        // every thread writes only its own word, and the bits added here (FULL, FWD_MORE, BWD_MORE) are not among those a
        // neighbour tests (FWD, BWD, CK): a concurrent reader sees the same answer before and after
        const int w = pk[d];
        pk[d] = w | sa_pk_derived(w, d >= 1 ? pk[d - 1] : 0, pk[d + 1], pk[d + 2], d, N, expect);
    }
    if (kind == SA_KIND_RING)
        for (long long d = t; d <= N; d += DPLAN_NT) rows[d].foff |= (long long) poff[(d + rows[d].xmyL) / 2] << 32;   // g0 = poff[first x]
    if (kind == SA_KIND_RING && maxP > 1 && status == 0) {
        // per-path neighbour records (their limits hold here: no window with more than 255 paths came this far)
        sa_prec_t *pr = A.prec + J.pid_off;
        if (t == 0) (void) sa_prec_col0(poff, lX, &pr[0]);
        for (long long x = 1 + t; x <= lX; x += DPLAN_NT) {
            const unsigned char *w = ref + (x - 1);
            sa_prec_col_t col;
            (void) sa_prec_column(&col, poff, x, lX, x >= 2 ? A.amb_n[w[-1]] : 1, A.amb_n[w[0]], A.amb_n[w[A.k - 1]], x < lX ? A.amb_n[w[A.k]] : 1);
            const int p0 = poff[x], P = poff[x + 1] - p0;
            for (int q = 0; q < P; q++) pr[p0 + q] = sa_prec_path(&col, poff, q);
        }
    }

    if (t == 0) {
        sa_region_t R;
        memset(&R, 0, sizeof(R));
        R.job = r; R.kind = kind; R.ragged_l = (J.bits & 2) ? 0 : 1; R.ragged_r = (J.bits & 4) ? 0 : 1;
        R.x1 = 0; R.y1 = 0; R.lX = lX; R.lY = lY; R.N = N;
        R.row_off = J.row_off; R.pk_off = J.pk_off; R.poff_off = J.poff_off; R.pid_off = J.pid_off; R.ev_off = J.ev_off;
        R.f_base = 0; R.seg_off = 0; R.n_seg = (int) n_seg; R.K = (int) K;
        R.max_rowpaths = (int) max_rowpaths; R.slots = (int) ((span + 63) / 64); R.chunk = 0; R.max_p = maxP;
        R.scale = J.scale; R.shift = J.shift; R.var = J.var; R.lvar = J.lvar;
        R.f_cellpaths = total_cells + 1;
        A.regions[r] = R;
        sa_dcount_t c;
        c.n_ck = n_ck; c.n_vbuf = n_vbuf; c.n_cand = n_cand; c.n_bscratch = n_bscr;
        c.cells_fwd = cf; c.cells_bwd = cb; c.status = status; c.pad = 0;
        A.counts[r] = c;
    }
}

// running sums over the reads and the forward-storage passes (sa_plan_build's tail); one workgroup, reads staged through
// LDS in tiles so that the single thread doing the (inherently sequential) packing never waits for global memory
#define DPLAN_TILE 1024
__global__ __launch_bounds__(DPLAN_NT) void k_dplan_scan(sa_region_t *regions, const sa_dcount_t *counts, long long *bases /* 5 per read */,
                                                         sa_dtotals_t *totals, int n, long long chunk_budget) {
    __shared__ long long s_f[DPLAN_TILE], s_seg[DPLAN_TILE], s_ck[DPLAN_TILE], s_v[DPLAN_TILE], s_c[DPLAN_TILE], s_b[DPLAN_TILE];
    __shared__ int s_kind[DPLAN_TILE], s_st[DPLAN_TILE];
    __shared__ long long o_fbase[DPLAN_TILE], o_seg[DPLAN_TILE], o_ck[DPLAN_TILE], o_v[DPLAN_TILE], o_c[DPLAN_TILE], o_b[DPLAN_TILE];
    __shared__ int o_chunk[DPLAN_TILE];
    __shared__ long long run[8];
    __shared__ int irun[4];
    __shared__ long long s_wave5[DPLAN_NT / 64];
    __shared__ int s_first_bad;          // first read (in read order) with a status: its code is the batch's
    const int t = threadIdx.x;
    if (t == 0) { for (int i = 0; i < 8; i++) run[i] = 0; for (int i = 0; i < 4; i++) irun[i] = 0; s_first_bad = 0x7fffffff; }
    __syncthreads();
    for (int base = 0; base < n; base += DPLAN_TILE) {
        const int m = n - base < DPLAN_TILE ? n - base : DPLAN_TILE;
        for (int i = t; i < m; i += DPLAN_NT) {
            const sa_region_t *R = &regions[base + i];
            const sa_dcount_t c = counts[base + i];
            s_f[i] = R->f_cellpaths; s_seg[i] = R->n_seg; s_kind[i] = R->kind;
            s_ck[i] = c.n_ck; s_v[i] = c.n_vbuf; s_c[i] = c.n_cand; s_b[i] = c.n_bscratch; s_st[i] = c.status;
        }
        __syncthreads();
        // the five running sums: workgroup scans over the tile, 256 reads at a time (carry in run[1..5])
        for (int sub = 0; sub < m; sub += DPLAN_NT) {
            const int i = sub + t;
            const bool in = i < m;
            long long tot;
            long long ex = dp_block_scan(in ? s_seg[i] : 0, s_wave5, tot);
            if (in) o_seg[i] = run[1] + ex;
            const long long t_seg = tot;
            ex = dp_block_scan(in ? s_ck[i] : 0, s_wave5, tot);
            if (in) o_ck[i] = run[2] + ex;
            const long long t_ck = tot;
            ex = dp_block_scan(in ? s_v[i] : 0, s_wave5, tot);
            if (in) o_v[i] = run[3] + ex;
            const long long t_v = tot;
            ex = dp_block_scan(in ? s_c[i] : 0, s_wave5, tot);
            if (in) o_c[i] = run[4] + ex;
            const long long t_c = tot;
            ex = dp_block_scan(in ? s_b[i] : 0, s_wave5, tot);
            if (in) o_b[i] = run[5] + ex;
            const long long t_b = tot;
            long long nf, nr;
            (void) dp_block_scan(in && s_kind[i] == SA_KIND_FAST ? 1 : 0, s_wave5, nf);
            (void) dp_block_scan(in && s_kind[i] == SA_KIND_RING ? 1 : 0, s_wave5, nr);
            if (in && s_st[i] != 0) atomicMin(&s_first_bad, base + i);
            __syncthreads();
            if (t == 0) {
                run[1] += t_seg; run[2] += t_ck; run[3] += t_v; run[4] += t_c; run[5] += t_b;
                irun[2] += (int) nf; irun[3] += (int) nr;
            }
            __syncthreads();
        }
        if (t == 0) {   // forward-storage passes: greedy in read order (sa_plan_build), inherently sequential, LDS only
            long long used = run[0], maxc = run[6];
            int chunk = irun[0];
            for (int i = 0; i < m; i++) {
                if (used > 0 && chunk_budget > 0 && used + s_f[i] > chunk_budget) { chunk++; used = 0; }
                o_chunk[i] = chunk; o_fbase[i] = used;
                used += s_f[i];
                maxc = used > maxc ? used : maxc;
            }
            run[0] = used; run[6] = maxc;
            irun[0] = chunk;
        }
        __syncthreads();
        for (int i = t; i < m; i += DPLAN_NT) {
            sa_region_t *R = &regions[base + i];
            R->chunk = o_chunk[i]; R->f_base = o_fbase[i]; R->seg_off = o_seg[i];
            long long *bb = bases + 5ll * (base + i);
            bb[0] = o_seg[i]; bb[1] = o_ck[i]; bb[2] = o_v[i]; bb[3] = o_c[i]; bb[4] = o_b[i];
        }
        __syncthreads();
    }
    if (t == 0) {
        sa_dtotals_t T;
        T.n_segs = run[1]; T.n_cks = run[2]; T.n_vbuf = run[3]; T.n_cand = run[4]; T.n_bscratch = run[5];
        T.max_chunk_cellpaths = run[6]; T.n_fast = irun[2]; T.n_ring = irun[3];
        T.n_chunks = n > 0 ? irun[0] + 1 : 0; T.status = s_first_bad != 0x7fffffff ? counts[s_first_bad].status : 0;
        *totals = T;
    }
}

__global__ __launch_bounds__(DPLAN_NT) void k_dplan_compact(const sa_djob_t *jobs, const sa_region_t *regions, const sa_dcount_t *counts,
                                                            const long long *bases, const sa_seg_t *seg_slab, const sa_ck_t *ck_slab,
                                                            sa_seg_t *segs, sa_ck_t *cks, int n) {
    const int r = blockIdx.x;
    if (r >= n) return;
    const long long *bb = bases + 5ll * r;
    const long long seg0 = bb[0], ck0 = bb[1], v0 = bb[2], c0 = bb[3], b0 = bb[4];
    const sa_seg_t *ss = seg_slab + jobs[r].seg_slab;
    const sa_ck_t *cs = ck_slab + jobs[r].ck_slab;
    const int nseg = regions[r].n_seg;
    const long long nck = counts[r].n_ck;
    for (int i = threadIdx.x; i < nseg; i += DPLAN_NT) {
        sa_seg_t S = ss[i];
        S.ck_base += ck0; S.cand_off += c0; S.bscratch_off += b0;
        segs[seg0 + i] = S;
    }
    for (long long i = threadIdx.x; i < nck; i += DPLAN_NT) {
        sa_ck_t c = cs[i];
        c.voff += v0;
        cks[ck0 + i] = c;
    }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
static bool dplan_enabled() {
    const char *e = getenv("SA_DEVICE_PLAN");   // (read per batch: a test hook)
    return !(e && atoi(e) == 0);
}

// Plans the batch on the device.  Returns SA_OK (b->plan and the device arrays of the plan are set), a negative SA_E* code
// (hard failure), or 1: not a batch for this planner -- nothing is left allocated and the caller runs sa_plan_build.
// A device plan between its two halves: dplan_front packs and uploads the reads and queues the planner kernels and the copies
// of what the host needs back; dplan_back waits for them and builds the host-side plan.  sa_batch_create runs both, one after
// the other; sa_batch_create_deferred returns after the first and the batch's first use runs the second (sa_hip.hip).
struct DPlanPending {
    const sa_model_t *m;
    sa_params_t p;
    unsigned flags;
    int64_t n_jobs;
    std::vector<sa_djob_t> dj;
    long long n_rows, n_pk, n_poff, n_pid, n_ev, n_sslab;
    char *stage;                   // pinned staging block of the reads' data
    std::vector<void *> temps;     // device blocks the planner kernels use and nobody afterwards
    sa_dtotals_t *d_tot;
    sa_dcount_t *d_counts;
    sa_dtotals_t tot;
    sa_plan_t *pl;
    sa_region_t *h_regions;
    sa_jobinfo_t *h_jobs;
    sa_seg_t *h_segs;
    std::vector<sa_dcount_t> h_counts;
    hipEvent_t done;               // behind the last copy back to the host
    char *back;                    // pinned landing block of those copies: totals | regions | counts | segments
    size_t back_regions, back_counts, back_segs;
    double t0;
};
// gives up a device plan: staging, temporaries, the host blocks and the batch's planner-built arrays go back
static void dplan_release(sa_batch *b, DPlanPending *P, bool arrays_too) {
    if (!P) return;
    if (P->done) { (void) hipEventSynchronize(P->done); g_handles.park(P->done, b->device); P->done = nullptr; }
    if (arrays_too && b->d_blk && b->lanes.compute[0]) (void) hipStreamSynchronize(b->lanes.compute[0]);   // (the event gather writes d_ev from there)
    if (P->stage) g_sa_pool.put(SaPool::PINNED, P->stage);
    if (P->back) g_sa_pool.put(SaPool::PINNED, P->back);
    for (void *q : P->temps) g_sa_pool.put(SaPool::DEVICE, q);
    if (arrays_too) {
        b->put_blocks(sa_batch::BLK_PLAN, sa_batch::BLK_REST);
        free(P->pl); free(P->h_regions); free(P->h_jobs); free(P->h_segs);
    }
    delete P;
}

// returns SA_OK with *pending set (kernels and copies queued), 1 when the batch is not one the device planner takes, or < 0
static int dplan_front(sa_batch *b, const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs, int64_t n_jobs,
                       const char *const *ambig, unsigned flags, long long chunk_budget, DPlanPending **pending) {
    *pending = nullptr;
    if (!dplan_enabled() || n_jobs <= 0 || n_jobs > 0x3fffffff) return 1;
    if (flags & (SA_FLAG_EXACT | SA_FLAG_FORCE_GENERIC)) return 1;
    if (m->emission != 0) return 1;   // the two-distribution emission: host planner (its constants are built from the host's pid array)
    if (!(p->threshold > 0.0) || !sa_params_plannable(p)) return 1;   // (threshold 0: capacities the host sizes; else sa_plan_build reports it)
    const bool trace = getenv("SA_TRACE") != nullptr;
    const double t0 = now_ms();
    DPlanArgs A;
    memset(&A, 0, sizeof(A));
    memset(A.lut, 255, sizeof(A.lut));
    for (int i = 0; i < m->n_alpha; i++) A.lut[(unsigned char) m->alphabet[i]] = (unsigned char) i;
    // ambiguity letters: options as digits; a letter whose options repeat, leave the alphabet or do not fit the tables sends the
    // batch to the host planner (the index form of path legality needs distinct options)
    bool amb_any[256], amb_bad[256];
    int amb_used = 0;
    for (int c = 0; c < 256; c++) {
        amb_any[c] = ambig && ambig[c] != nullptr;
        amb_bad[c] = false;
        A.amb_n[c] = 1;
        A.amb_off[c] = 0;
        if (!amb_any[c]) continue;
        const char *o = ambig[c];
        const size_t no = strlen(o);
        if (no < 1 || no > 16 || amb_used + (int) no > (int) sizeof(A.amb_dig)) { amb_bad[c] = true; continue; }
        for (size_t i = 0; i < no && !amb_bad[c]; i++) {
            if (A.lut[(unsigned char) o[i]] == 255) amb_bad[c] = true;
            for (size_t q = 0; q < i; q++) amb_bad[c] = amb_bad[c] || o[q] == o[i];
        }
        if (amb_bad[c]) continue;
        A.amb_n[c] = (unsigned char) no;
        A.amb_off[c] = (unsigned short) amb_used;
        for (size_t i = 0; i < no; i++) A.amb_dig[amb_used++] = A.lut[(unsigned char) o[i]];
    }
    // (reads with ambiguity letters are planned here only for the ring kernels; without them -- SA_RING=0, the expectation pass, an
    // HDP table too large for the emission plane's 32-bit offsets -- such a read sends the batch to the host planner)
    const bool ring_possible = sa_ring_env_on() && sa_hdp_plane_fits(m) &&
                               !((flags & SA_FLAG_EXPECT_INTERNAL) && m->hdp != nullptr);   // (expectation pass: Gaussian models only)
    const int k = m->k;
    const long long limit = p->split_matrix_bigger_than_this;

    // SA_FLAG_INPUTS_IN_HOST_BLOCK: every job's event records and anchor arrays lie inside ONE block from sa_host_alloc.  The
    // block (its part that holds them) crosses PCIe with one DMA and k_dplan_ingest does the checking, narrowing and gathering
    // the host otherwise does: sa_batch_create then touches the reference letters only (416 MB per 2000 reads stay unread: the
    // two host threads a rank has under a tight CPU quota could not keep up with the GPU).
    bool in_block = (flags & SA_FLAG_INPUTS_IN_HOST_BLOCK) != 0;
    size_t blk_referenced = 0;                         // bytes of the block this batch's jobs actually name
    const char *blk_lo = nullptr, *blk_hi = nullptr;   // what the jobs use of the block ...
    const char *rng_lo[2] = {nullptr, nullptr}, *rng_hi[2] = {nullptr, nullptr};   // ... event records [0] and anchors [1] apart
    if (in_block) {
        const char *base = nullptr;
        size_t bytes = 0;
        for (int64_t j = 0; j < n_jobs; j++) {
            const sa_job_t *jb = &jobs[j];
            const long long stp = jb->event_stride > 0 ? jb->event_stride : 1;
            const void *ptr[3] = {jb->n_events > 0 ? (const void *) jb->events : nullptr, jb->n_anchors > 0 ? (const void *) jb->anchor_x : nullptr,
                                  jb->n_anchors > 0 ? (const void *) jb->anchor_y : nullptr};
            const size_t len[3] = {jb->n_events > 0 ? (size_t) (((jb->n_events - 1) * stp + 1) * 8) : 0, 8 * (size_t) (jb->n_anchors > 0 ? jb->n_anchors : 0),
                                   8 * (size_t) (jb->n_anchors > 0 ? jb->n_anchors : 0)};
            for (int q = 0; q < 3; q++) {
                if (!ptr[q]) continue;
                const char *pq = (const char *) ptr[q];
                if (!base && !sa_host_block_of(pq, &base, &bytes)) return SA_EINVAL;   // not memory from sa_host_alloc
                if (pq < base || pq + len[q] > base + bytes || ((size_t) (pq - base) & 7)) return SA_EINVAL;
                const int w = q > 0;
                blk_referenced += len[q];
                rng_lo[w] = (!rng_lo[w] || pq < rng_lo[w]) ? pq : rng_lo[w];
                rng_hi[w] = (!rng_hi[w] || pq + len[q] > rng_hi[w]) ? pq + len[q] : rng_hi[w];
            }
        }
        for (int w = 0; w < 2; w++) {
            if (!rng_lo[w]) continue;
            blk_lo = (!blk_lo || rng_lo[w] < blk_lo) ? rng_lo[w] : blk_lo;
            blk_hi = (!blk_hi || rng_hi[w] > blk_hi) ? rng_hi[w] : blk_hi;
        }
        if (!blk_lo) { blk_lo = blk_hi = (const char *) jobs; }   // (no events and no anchors at all)
        // What travels is the covering range of this batch's arrays (one or two DMAs), not the arrays one by one: a caller that
        // keeps ONE arena for several batches, or leaves gaps, would send -- and hold in HBM -- bytes of other batches.  When the
        // covering ranges hold more than twice what the jobs name (+ 1 MB), the batch takes the pageable path instead: host
        // threads read the same (page-locked) memory and pack exactly what is used.  (include/signalalign_hip.h says so.)
        const bool apart = rng_lo[0] && rng_lo[1] && (rng_hi[0] <= rng_lo[1] || rng_hi[1] <= rng_lo[0]);
        const size_t covered = apart ? (size_t) (rng_hi[0] - rng_lo[0]) + (size_t) (rng_hi[1] - rng_lo[1]) : (size_t) (blk_hi - blk_lo);
        if (covered > 2 * blk_referenced + (1u << 20)) {
            if (trace) fprintf(stderr, "[trace] dplan: host block: %.1f MB covered for %.1f MB referenced -- packed by the host instead\n",
                               covered / 1048576.0, blk_referenced / 1048576.0);
            in_block = false;
            blk_lo = blk_hi = nullptr;
            rng_lo[0] = rng_lo[1] = rng_hi[0] = rng_hi[1] = nullptr;
        }
    }
    // The planning kernels need the anchors only.  A block that holds them apart from the event records (a caller that lays out
    // its block chooses so) is sent in two pieces: the anchors on the upload stream, ahead of the planning kernels, and the
    // event records -- three quarters of the bytes -- on the batch's own stream, where every kernel that reads the event
    // means is queued later: sa_batch_create does not wait for them.
    const bool blk_split = in_block && b->lanes.compute[0] && rng_lo[0] && rng_lo[1] && (rng_hi[0] <= rng_lo[1] || rng_hi[1] <= rng_lo[0]) &&
                           !(getenv("SA_BLOCK_SPLIT") && atoi(getenv("SA_BLOCK_SPLIT")) == 0);   // (test hook)

    // ---- sizes and offsets from the reads' headers (no read data touched yet) ----
    DPlanPending *PP = new DPlanPending();
    PP->m = m; PP->p = *p; PP->flags = flags; PP->n_jobs = n_jobs; PP->stage = nullptr; PP->d_tot = nullptr; PP->d_counts = nullptr;
    PP->pl = nullptr; PP->h_regions = nullptr; PP->h_jobs = nullptr; PP->h_segs = nullptr; PP->done = nullptr; PP->t0 = t0;
    PP->back = nullptr;
    PP->dj.resize((size_t) n_jobs);
    std::vector<sa_djob_t> &dj = PP->dj;
    const long long seg_step = p->min_diags_between_trace_back - p->trace_back_diagonals - 1;
    long long n_rows = 0, n_pk = 0, n_poff = 0, n_pid = 0, n_ev = 0, n_ref = 0, n_anc = 0, n_sslab = 0, n_cslab = 0;
    for (int64_t j = 0; j < n_jobs; j++) {
        const sa_job_t *jb = &jobs[j];
        bool ok = sa_job_header_ok(jb);
        long long lX = 0, lY = 0;
        if (ok) {
            lX = sa_job_lX(jb->ref_len, k);
            lY = jb->n_events;
            ok = lX + lY > 0 && lX < (1 << 28) && lY < (1 << 28) && jb->n_anchors < (1 << 28);
        }
        if (!ok) { delete PP; return 1; }
        sa_djob_t d;
        memset(&d, 0, sizeof(d));
        d.lX = (int) lX; d.lY = (int) lY; d.n_anchors = (int) jb->n_anchors;
        d.scale = jb->scale; d.shift = jb->shift; d.var = jb->var; d.lvar = log((1 / jb->var));
        const long long N = lX + lY;
        d.row_off = n_rows; d.pk_off = n_pk; d.poff_off = n_poff; d.ev_off = n_ev;
        d.ref_off = n_ref; d.anc_off = n_anc; d.seg_slab = n_sslab; d.ck_slab = n_cslab;
        n_rows += sa_region_rows(N); n_pk += sa_region_pk_words(N); n_poff += sa_region_poffs(lX); n_ev += lY;
        n_ref += (jb->ref_len + 15) & ~15ll; n_anc += 2ll * d.n_anchors;
        const long long sb = N / seg_step + 2;
        n_sslab += sb; n_cslab += N / SA_CKPT_EVERY + sb + 2;
        dj[(size_t) j] = d;
    }

    // ---- the reads' own data, packed into one pinned block: descriptors | reference letters | anchors | event means ----
    const size_t off_dj = 0, off_src = (sizeof(sa_djob_t) * (size_t) n_jobs + 255) & ~(size_t) 255;
    const size_t off_ref = off_src + (in_block ? ((sizeof(sa_dsrc_t) * (size_t) n_jobs + 255) & ~(size_t) 255) : 0);
    const size_t off_anc = (off_ref + (size_t) n_ref + 255) & ~(size_t) 255;
    const size_t raw_bytes = (off_anc + 4 * (size_t) n_anc + 255) & ~(size_t) 255;
    const size_t off_ev = raw_bytes, stage_bytes = off_ev + (in_block ? 0 : 8 * (size_t) n_ev);
    const int device = b->device;
    char *stage = nullptr;
    if (g_sa_pool.get(SaPool::PINNED, (void **) &stage, stage_bytes, device) != hipSuccess) { (void) hipGetLastError(); delete PP; return SA_ENOMEM; }
    PP->stage = stage;

    // ---- device arrays ----
    char *d_raw = nullptr;
    sa_seg_t *d_sslab = nullptr;
    sa_ck_t *d_cslab = nullptr;
    sa_dcount_t *d_counts = nullptr;
    long long *d_bases = nullptr;
    sa_dtotals_t *d_tot = nullptr;
    std::vector<void *> &temps = PP->temps;
    auto fail = [&](int rc) {
        (void) hipStreamSynchronize(g_uploader.stream);   // nothing of this plan may still be in flight when its blocks go back
        if (b->d_blk && b->lanes.compute[0]) (void) hipStreamSynchronize(b->lanes.compute[0]);
        dplan_release(b, PP, true);
        if (b->d_blk) { g_sa_pool.put(SaPool::DEVICE, b->d_blk); b->d_blk = nullptr; }
        return rc;
    };
#define DP_ALLOC(ptr, bytes, temp)                                                                          \
    do {                                                                                                    \
        if (g_sa_pool.get(SaPool::DEVICE, (void **) &(ptr), (size_t) ((bytes) > 0 ? (bytes) : 8), device) != hipSuccess) { \
            (void) hipGetLastError();                                                                       \
            return fail(SA_ENOMEM);                                                                         \
        }                                                                                                   \
        if (temp) temps.push_back((void *) (ptr));                                                          \
    } while (0)
#define DP_HIP(call)                                                                                        \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess) {                                                                             \
            fprintf(stderr, "[signalalign_hip] %s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return fail(e_ == hipErrorOutOfMemory ? SA_ENOMEM : SA_ENODEVICE);                              \
        }                                                                                                   \
    } while (0)
    DP_ALLOC(d_raw, raw_bytes, true);
    char *d_blk = nullptr;
    int *d_ingest = nullptr;
    // image of the block in HBM: the covering range as it is, or (two pieces) the anchors' range followed by the events' range
    // ... and behind it the table that says where each read's arrays lie in it (the event gather may run after the plan's own
    // temporaries have gone back)
    const size_t img_anc = 0, img_ev = blk_split ? sa_up256((size_t) (rng_hi[1] - rng_lo[1])) : 0;
    const size_t img_src = in_block ? sa_up256((blk_split ? img_ev + (size_t) (rng_hi[0] - rng_lo[0]) : (size_t) (blk_hi - blk_lo)) + 64) : 0;
    if (in_block) {
        DP_ALLOC(b->d_blk, img_src + sizeof(sa_dsrc_t) * (size_t) n_jobs, false);
        b->d_blk_bytes = img_src + sizeof(sa_dsrc_t) * (size_t) n_jobs;
        d_blk = b->d_blk;
        DP_ALLOC(d_ingest, 4 * (size_t) n_jobs, true);
    }
    DP_ALLOC(d_sslab, sizeof(sa_seg_t) * (size_t) n_sslab, true);
    DP_ALLOC(d_cslab, sizeof(sa_ck_t) * (size_t) n_cslab, true);
    DP_ALLOC(d_counts, sizeof(sa_dcount_t) * (size_t) n_jobs, true);
    DP_ALLOC(d_bases, 40 * (size_t) n_jobs, true);
    DP_ALLOC(d_tot, sizeof(sa_dtotals_t), true);
    DP_ALLOC(b->d_regions, sizeof(sa_region_t) * (size_t) n_jobs, false);
    DP_ALLOC(b->d_rows, sizeof(sa_row_t) * (size_t) (n_rows + 192), false);
    DP_ALLOC(b->d_pk, 4 * (size_t) n_pk, false);
    DP_ALLOC(b->d_poff, 4 * (size_t) n_poff, false);
    DP_ALLOC(b->d_ev, 8 * (size_t) (n_ev + 8), false);
    DP_ALLOC(b->d_segs, sizeof(sa_seg_t) * (size_t) n_sslab, false);
    DP_ALLOC(b->d_cks, sizeof(sa_ck_t) * (size_t) n_cslab, false);
    hipStream_t st = g_uploader.stream;
    if (trace) fprintf(stderr, "[trace] dplan: device arrays at %.1f ms\n", now_ms() - t0);
    // Every read is CHECKED AND PACKED in one pass over its data (the anchors alone are 96 MB per 2000 reads: a separate
    // eligibility pass read them twice, 4.7 of 15 ms of sa_batch_create on the two host threads a rank of an 8-GPU run has under
    // a 16-CPU quota), in slices, and a slice travels while the next one is packed (126 MB per 2000 reads).  Every block of the
    // staging area is laid out in read order, so a slice of reads is one contiguous range of each.  A read the device planner
    // does not take (a letter outside the alphabet, anchors that leave the matrix or split it, ...) ends the attempt: what was
    // queued is waited for, everything goes back and the host planner -- which names the error -- takes the batch.
    std::atomic<int> bad(0);
    {
        const int64_t n_slices = n_jobs >= 64 ? 4 : 1;
        for (int64_t sl = 0; sl < n_slices; sl++) {
            const int64_t j0 = n_jobs * sl / n_slices, j1 = n_jobs * (sl + 1) / n_slices;
            if (j1 <= j0) continue;
            sa_parallel_for((size_t) (j1 - j0), [&](size_t jj) {
                if (bad.load(std::memory_order_relaxed)) return;
                const size_t j = (size_t) j0 + jj;
                const sa_job_t *jb = &jobs[j];
                sa_djob_t &d = dj[j];
                const long long lX = d.lX, lY = d.lY;
                bool ok = true, multi = false;
                long long n_paths = lX + 1;   // one path per cell unless ...
                unsigned char *rf = reinterpret_cast<unsigned char *>(stage + off_ref + d.ref_off);
                if (lX >= 1) {
                    unsigned worst = 0;       // letters: copied while they are looked up (255: outside the alphabet)
                    bool amb = false;
                    for (long long i = 0; i < jb->ref_len; i++) {
                        const unsigned char c = (unsigned char) jb->ref[i];
                        rf[i] = c;
                        amb = amb || amb_any[c];
                        worst |= amb_any[c] ? 0u : (unsigned) (A.lut[c] == 255);
                    }
                    ok = worst == 0;
                    if (ok && amb) {
                        multi = true;
                        for (long long i = 0; i < jb->ref_len && ok; i++) {
                            const unsigned char c = (unsigned char) jb->ref[i];
                            if (amb_any[c]) ok = !amb_bad[c] && ring_possible;
                        }
                        if (ok) {   // ... ambiguity letters multiply the paths of the windows that hold them
                            n_paths = 1;
                            for (long long x = 1; x <= lX && ok; x++) {
                                long long P = 1;
                                for (int i = 0; i < k; i++) P *= A.amb_n[(unsigned char) jb->ref[x - 1 + i]];
                                ok = P <= 255;
                                n_paths += P;
                            }
                        }
                    }
                } else if (jb->ref_len > 0) {
                    memcpy(rf, jb->ref, (size_t) jb->ref_len);
                }
                if (ok && !in_block) {   // anchors inside the matrix and strictly increasing; no gap that would split the matrix
                    int *an = reinterpret_cast<int *>(stage + off_anc) + d.anc_off;
                    const int na = d.n_anchors;
                    long long px = 0, py = 0;
                    bool good = true;
                    for (int i = 0; i < na; i++) {
                        const long long nx = jb->anchor_x[i], ny = jb->anchor_y[i];
                        // (px, py: one past the previous anchor, 0 at the start -- so nx >= px also says nx >= 0)
                        good = good && nx >= px && ny >= py && nx < lX && ny < lY && (nx - px) * (ny - py) <= limit;
                        an[i] = (int) nx; an[na + i] = (int) ny;
                        px = nx + 1; py = ny + 1;
                    }
                    ok = good && (lX - px) * (lY - py) <= limit;
                }
                if (!ok) { bad.store(1); return; }
                d.bits = (multi ? 1 : 0) | (int) ((jb->ends & 3u) << 1);
                d.pid_off = n_paths;   // (its count for now: turned into an offset below)
                if (in_block) {
                    sa_dsrc_t *sr = reinterpret_cast<sa_dsrc_t *>(stage + off_src) + j;
                    const char *ev_base = blk_split ? rng_lo[0] - img_ev : blk_lo, *an_base = blk_split ? rng_lo[1] - img_anc : blk_lo;
                    sr->ev_off = lY > 0 ? (long long) ((const char *) jb->events - ev_base) : 0;
                    sr->ax_off = d.n_anchors > 0 ? (long long) ((const char *) jb->anchor_x - an_base) : 0;
                    sr->ay_off = d.n_anchors > 0 ? (long long) ((const char *) jb->anchor_y - an_base) : 0;
                    sr->ev_dst = d.ev_off;
                    sr->stride = (int) (jb->event_stride > 0 ? jb->event_stride : 1);
                    sr->n_events = (int) lY;
                    return;
                }
                double *ev = reinterpret_cast<double *>(stage + off_ev) + d.ev_off;
                const long long stp = jb->event_stride > 0 ? jb->event_stride : 1;
                if (stp == 1) memcpy(ev, jb->events, 8 * (size_t) lY);
                else for (long long i = 0; i < lY; i++) ev[i] = jb->events[i * stp];
            });
            if (bad.load()) return fail(1);
            const sa_djob_t &a = dj[(size_t) j0];
            const bool last = j1 == n_jobs;
            const size_t ref_a = (size_t) a.ref_off, ref_b = last ? (size_t) n_ref : (size_t) dj[(size_t) j1].ref_off;
            const size_t anc_a = 4 * (size_t) a.anc_off, anc_b = 4 * (last ? (size_t) n_anc : (size_t) dj[(size_t) j1].anc_off);
            const size_t ev_a = 8 * (size_t) a.ev_off, ev_b = 8 * (last ? (size_t) n_ev : (size_t) dj[(size_t) j1].ev_off);
            if (ref_b > ref_a) DP_HIP(hipMemcpyAsync(d_raw + off_ref + ref_a, stage + off_ref + ref_a, ref_b - ref_a, hipMemcpyHostToDevice, st));
            if (!in_block && anc_b > anc_a) DP_HIP(hipMemcpyAsync(d_raw + off_anc + anc_a, stage + off_anc + anc_a, anc_b - anc_a, hipMemcpyHostToDevice, st));
            if (!in_block && ev_b > ev_a) DP_HIP(hipMemcpyAsync((char *) b->d_ev + ev_a, stage + off_ev + ev_a, ev_b - ev_a, hipMemcpyHostToDevice, st));
        }
    }
    bool any_multi = false;
    for (int64_t j = 0; j < n_jobs; j++) {   // path offsets: known once the letters have been seen
        sa_djob_t &d = dj[(size_t) j];
        const long long my_paths = d.pid_off;
        any_multi = any_multi || (d.bits & 1) != 0;
        d.pid_off = n_pid;
        n_pid += my_paths;
    }
    DP_ALLOC(b->d_pid, 4 * (size_t) n_pid, false);
    if (any_multi) DP_ALLOC(b->d_prec, sizeof(sa_prec_t) * (size_t) n_pid, false);
    memcpy(stage + off_dj, dj.data(), sizeof(sa_djob_t) * (size_t) n_jobs);
    DP_HIP(hipMemcpyAsync(d_raw + off_dj, stage + off_dj, sizeof(sa_djob_t) * (size_t) n_jobs, hipMemcpyHostToDevice, st));
    if (in_block) {
        const sa_dsrc_t *d_src = reinterpret_cast<const sa_dsrc_t *>(d_blk + img_src);
        DP_HIP(hipMemcpyAsync(d_blk + img_src, stage + off_src, sizeof(sa_dsrc_t) * (size_t) n_jobs, hipMemcpyHostToDevice, st));
        // (pinned source: one DMA each)
        if (blk_split) DP_HIP(hipMemcpyAsync(d_blk + img_anc, rng_lo[1], (size_t) (rng_hi[1] - rng_lo[1]), hipMemcpyHostToDevice, st));
        else if (blk_hi > blk_lo) DP_HIP(hipMemcpyAsync(d_blk, blk_lo, (size_t) (blk_hi - blk_lo), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_dplan_ingest, dim3((unsigned) n_jobs), dim3(DPLAN_NT), 0, st, reinterpret_cast<const sa_djob_t *>(d_raw + off_dj),
                           d_src, (const char *) d_blk, reinterpret_cast<int *>(d_raw + off_anc), d_ingest, (long long) limit);
        if (!blk_split) {
            hipLaunchKernelGGL(k_dplan_events, dim3((unsigned) n_jobs), dim3(DPLAN_NT), 0, st, d_src, (const char *) d_blk, b->d_ev);
        } else {
            // the event records: on the batch's own stream, behind the table they are gathered with, ahead of everything the
            // batch will ever queue there
            DP_HIP(hipEventRecord(b->ev.planner_gather, st));
            DP_HIP(hipStreamWaitEvent(b->lanes.compute[0], b->ev.planner_gather, 0));
            DP_HIP(hipMemcpyAsync(d_blk + img_ev, rng_lo[0], (size_t) (rng_hi[0] - rng_lo[0]), hipMemcpyHostToDevice, b->lanes.compute[0]));
            hipLaunchKernelGGL(k_dplan_events, dim3((unsigned) n_jobs), dim3(DPLAN_NT), 0, b->lanes.compute[0], d_src, (const char *) d_blk, b->d_ev);
        }
        A.ingest_status = d_ingest;
    }
    if (trace) fprintf(stderr, "[trace] dplan: inputs packed (%.1f MB) at %.1f ms\n", stage_bytes / 1048576.0, now_ms() - t0);
    DP_HIP(hipMemsetAsync(b->d_ev + n_ev, 0, 64, st));
    DP_HIP(hipMemsetAsync(b->d_pk, 0, 4 * (size_t) n_pk, st));
    DP_HIP(hipMemsetAsync(b->d_rows + n_rows, 0, 192 * sizeof(sa_row_t), st));
    A.jobs = reinterpret_cast<const sa_djob_t *>(d_raw + off_dj);
    A.refs = reinterpret_cast<const unsigned char *>(d_raw + off_ref);
    A.anchors = reinterpret_cast<const int *>(d_raw + off_anc);
    A.regions = b->d_regions; A.rows = b->d_rows; A.pk = b->d_pk; A.poff = b->d_poff; A.pid = b->d_pid; A.prec = b->d_prec;
    A.seg_slab = d_sslab; A.ck_slab = d_cslab; A.counts = d_counts;
    A.expansion = p->diagonal_expansion; A.trace_back = p->trace_back_diagonals; A.min_diags = p->min_diags_between_trace_back;
    A.k = k; A.n_alpha = m->n_alpha;
    // the batch's routing inputs, from the host planner's predicates.  ambig_distinct: a read that USES a letter with repeated options was refused
    // above.  Known difference: the host's ambig_options_distinct() also sees an UNUSED such letter and then takes the reference-ordered kernels.
    A.route.flags = flags; A.route.emission = m->emission; A.route.hdp = m->hdp != nullptr; A.route.hdp_plane_fits = sa_hdp_plane_fits(m);
    A.route.ring_env = sa_ring_env_on(); A.route.ring_wide_env = sa_ring_wide_env_on(); A.route.ambig_distinct = 1;
    int lds_anchors = 0;
    for (int64_t j = 0; j < n_jobs; j++) lds_anchors = dj[(size_t) j].n_anchors > lds_anchors ? dj[(size_t) j].n_anchors : lds_anchors;
    if (lds_anchors > DPLAN_LDS_ANCHORS) lds_anchors = DPLAN_LDS_ANCHORS;
    hipLaunchKernelGGL(k_dplan_region, dim3((unsigned) n_jobs), dim3(DPLAN_NT), sizeof(int) * (size_t) lds_anchors, st, A, (int) n_jobs,
                       lds_anchors);
    hipLaunchKernelGGL(k_dplan_scan, dim3(1), dim3(DPLAN_NT), 0, st, b->d_regions, d_counts, d_bases, d_tot, (int) n_jobs, chunk_budget);
    hipLaunchKernelGGL(k_dplan_compact, dim3((unsigned) n_jobs), dim3(DPLAN_NT), 0, st, A.jobs, b->d_regions, d_counts, d_bases, d_sslab,
                       d_cslab, b->d_segs, b->d_cks, (int) n_jobs);
    DP_HIP(hipGetLastError());
    if (trace) fprintf(stderr, "[trace] dplan: kernels queued at %.1f ms\n", now_ms() - t0);
    // ---- what the host needs back: regions, per-read counts, totals, segments ----
    PP->n_rows = n_rows; PP->n_pk = n_pk; PP->n_poff = n_poff; PP->n_pid = n_pid; PP->n_ev = n_ev; PP->n_sslab = n_sslab;
    PP->d_tot = d_tot; PP->d_counts = d_counts;
    PP->pl = (sa_plan_t *) calloc(1, sizeof(sa_plan_t));
    PP->h_regions = (sa_region_t *) malloc(sizeof(sa_region_t) * (size_t) n_jobs);
    PP->h_jobs = (sa_jobinfo_t *) calloc((size_t) n_jobs, sizeof(sa_jobinfo_t));
    PP->h_segs = (sa_seg_t *) malloc(sizeof(sa_seg_t) * (size_t) (n_sslab > 0 ? n_sslab : 1));
    PP->h_counts.resize((size_t) n_jobs);
    if (!PP->pl || !PP->h_regions || !PP->h_jobs || !PP->h_segs) return fail(SA_ENOMEM);
    // The copies land in pinned memory (plain DMA, complete when the event is): to pageable destinations the runtime stages them
    // through buffers and host work of its own, in line with whatever else the process is copying.
    PP->back_regions = sa_up256(sizeof(sa_dtotals_t));
    PP->back_counts = PP->back_regions + sa_up256(sizeof(sa_region_t) * (size_t) n_jobs);
    PP->back_segs = PP->back_counts + sa_up256(sizeof(sa_dcount_t) * (size_t) n_jobs);
    const size_t back_bytes = PP->back_segs + sa_up256(sizeof(sa_seg_t) * (size_t) (n_sslab > 0 ? n_sslab : 1));
    if (g_sa_pool.get(SaPool::PINNED, (void **) &PP->back, back_bytes, device) != hipSuccess) { (void) hipGetLastError(); PP->back = nullptr; return fail(SA_ENOMEM); }
    DP_HIP(hipMemcpyAsync(PP->back, d_tot, sizeof(sa_dtotals_t), hipMemcpyDeviceToHost, st));
    DP_HIP(hipMemcpyAsync(PP->back + PP->back_regions, b->d_regions, sizeof(sa_region_t) * (size_t) n_jobs, hipMemcpyDeviceToHost, st));
    DP_HIP(hipMemcpyAsync(PP->back + PP->back_counts, d_counts, sizeof(sa_dcount_t) * (size_t) n_jobs, hipMemcpyDeviceToHost, st));
    if (n_sslab > 0) DP_HIP(hipMemcpyAsync(PP->back + PP->back_segs, b->d_segs, sizeof(sa_seg_t) * (size_t) n_sslab, hipMemcpyDeviceToHost, st));
    if (g_handles.event(&PP->done, device) != hipSuccess) { (void) hipGetLastError(); PP->done = nullptr; return fail(SA_ENODEVICE); }
    DP_HIP(hipEventRecord(PP->done, st));
#undef DP_ALLOC
#undef DP_HIP
    *pending = PP;
    return SA_OK;
}

// second half: SA_OK (b->plan set, the device plan is this batch's), 1 when a read turned out to be one the device planner does
// not take (everything released: the host planner takes over and names errors), or < 0
static int dplan_back(sa_batch *b, DPlanPending *P) {
    const bool trace = getenv("SA_TRACE") != nullptr;
    const hipError_t e = hipEventSynchronize(P->done);   // (a blocking-sync event: the waiting thread sleeps)
    g_handles.park(P->done, b->device);
    P->done = nullptr;
    if (e != hipSuccess) {
        fprintf(stderr, "[signalalign_hip] device planner: %s\n", hipGetErrorString(e));
        dplan_release(b, P, true);
        return SA_ENODEVICE;
    }
    memcpy(&P->tot, P->back, sizeof(sa_dtotals_t));
    memcpy(P->h_regions, P->back + P->back_regions, sizeof(sa_region_t) * (size_t) P->n_jobs);
    memcpy(P->h_counts.data(), P->back + P->back_counts, sizeof(sa_dcount_t) * (size_t) P->n_jobs);
    if (P->n_sslab > 0) memcpy(P->h_segs, P->back + P->back_segs, sizeof(sa_seg_t) * (size_t) P->n_sslab);
    const sa_dtotals_t &tot = P->tot;
    if (trace) fprintf(stderr, "[trace] dplan: planned on the device at %.1f ms (status %d)\n", now_ms() - P->t0, tot.status);
    if (tot.status != 0) {   // a read the device planner does not take (or an error the host planner will name)
        dplan_release(b, P, true);
        return 1;
    }
    sa_plan_t *pl = P->pl;
    const int64_t n_jobs = P->n_jobs;
    pl->model = P->m; pl->params = P->p; pl->flags = P->flags | SA_FLAG_DEVICE_XC_INTERNAL; pl->n_jobs = n_jobs;
    pl->jobs = P->h_jobs; pl->regions = P->h_regions; pl->n_regions = pl->cap_regions = n_jobs;
    pl->segs = P->h_segs; pl->n_segs = tot.n_segs; pl->cap_segs = P->n_sslab;
    pl->n_cks = tot.n_cks; pl->n_rows = P->n_rows; pl->n_pk = P->n_pk; pl->n_poff = P->n_poff; pl->n_pid = P->n_pid; pl->n_ev = P->n_ev;
    pl->n_vbuf = tot.n_vbuf; pl->n_cand = tot.n_cand; pl->n_bscratch = tot.n_bscratch;
    pl->max_chunk_cellpaths = tot.max_chunk_cellpaths; pl->n_chunks = tot.n_chunks;
    pl->n_fast_regions = tot.n_fast; pl->n_ring_regions = tot.n_ring;
    for (int64_t j = 0; j < n_jobs; j++) {
        sa_jobinfo_t *J = &P->h_jobs[j];
        J->region_off = j; J->n_regions = 1; J->ev_off = P->dj[(size_t) j].ev_off; J->n_events = P->dj[(size_t) j].lY;
        J->cells_fwd = P->h_counts[(size_t) j].cells_fwd; J->cells_bwd = P->h_counts[(size_t) j].cells_bwd;
        pl->cells_fwd += J->cells_fwd; pl->cells_bwd += J->cells_bwd;
        const long long sp = (long long) P->h_regions[j].slots * 64;
        if (sp > pl->max_span) pl->max_span = sp;
    }
    b->plan = pl;
    b->dev_planned = true;
    const double t_rel = now_ms(), t0_ = P->t0;
    if (b->c_deferred) {   // a deferred batch keeps its staging block until it is destroyed: the pinned cache then sees the same
                           // requests in the same order in every step of a caller's loop, whenever this half happens to run (a
                           // second 1.7 GB block first needed in the middle of a timed loop is a 300-400 ms hipHostMalloc)
        b->held_stage = P->stage;
        P->stage = nullptr;
    }
    dplan_release(b, P, false);   // staging and temporaries; the plan and the arrays stay with the batch
    if (trace) fprintf(stderr, "[trace] dplan: host plan built at %.1f ms, staging released at %.1f ms\n", t_rel - t0_, now_ms() - t0_);
    return SA_OK;
}

// both halves, one after the other (sa_dplan_compare)
static int dplan_build(sa_batch *b, const sa_model_t *m, const sa_params_t *p, const sa_job_t *jobs, int64_t n_jobs,
                       const char *const *ambig, unsigned flags, long long chunk_budget) {
    DPlanPending *P = nullptr;
    const int rc = dplan_front(b, m, p, jobs, n_jobs, ambig, flags, chunk_budget, &P);
    if (rc != SA_OK) return rc;
    return dplan_back(b, P);
}
