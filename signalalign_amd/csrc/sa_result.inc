// sa_result.inc -- what follows the sweeps of a pass: the exact fold of the checkpoint totals, the speculative totals and their
// check, finalisation, scan and gather into the reference's output order; the expectation pass's reduction; k_check_events and
// k_fill_xc, which prepare a batch's inputs.  Included by sa_hip.hip behind the sweep kernels (strip_region: sa_strip.inc).
// ---------------------------------------------------------------------------------------------------
// fold: totalProbability of every checkpoint, folded exactly as dpDiagonal_dotProduct does
// (impl/pairwiseAligner.c:1167-1180): a left fold over the cells in ascending x-y.
// ---------------------------------------------------------------------------------------------------
// branch-free form of la_exact (same comparisons, same un-contracted polynomial), coefficients from LDS
__device__ __forceinline__ double la_exact_bf(const double *tab, double x, double y) {
    double mx = __builtin_fmax(x, y);
    double mn = __builtin_fmin(x, y);
    double d = mx - mn;
    int idx = (d > 1.0 ? 1 : 0) + (d > 2.5 ? 1 : 0) + (d > 4.5 ? 1 : 0);
    const double4 c = *reinterpret_cast<const double4 *>(tab + 4 * idx);
    double r = ((c.x * d + c.y) * d + c.z) * d + c.w;
    r = r + mn;
    return (d < 7.5) ? r : mx;
}

// One wave folds 64 consecutive checkpoints, one per lane.  A checkpoint's terms are contiguous in vbuf -- nA terms of its own
// diagonal, then nB of the diagonal above -- and its total is logAdd(fold(A), fold(B)): the two folds are independent chains, walked
// side by side (round 4: two logAdds in flight per lane instead of one; the chain is latency, ~25 dependent instructions and an LDS
// read per term).  Terms come in with coalesced loads, FOLD_TW per checkpoint and chain (a load instruction serves 64 / FOLD_TW
// checkpoints), and are transposed through LDS so that every lane then walks its own checkpoint.  Two tiles of 64 x (FOLD_TW + 1)
// doubles: 9 KB per wave at FOLD_TW 8, seventeen waves per CU (FOLD_TW 4 / 8 / 16 / 32: 0.88 / 0.57 / 0.60 / 1.14 ms on the headline batch, 2.04 / 1.31 / 1.58 / 2.99 on the realistic one) (the 64-term tile of rounds 1-3 took 33 KB: four waves per CU, one
// chain each -- k_fold 0.84 ms of the headline batch's 9.9 and 2.4 of the realistic batch's 29).
#define FOLD_TW 8
#define FOLD_LD (FOLD_TW + 1)
__global__ __launch_bounds__(64) void k_fold(DevPlan P, long long ck0, long long ck1) {
    __shared__ double tileA[64 * FOLD_LD], tileB[64 * FOLD_LD];
    __shared__ __attribute__((aligned(32))) double LT[16];
    const int lane = threadIdx.x;
    if (lane < 4) {
        const float a3[4] = {-0.009350833524763f, -0.014532321752540f, -0.004605031767994f, -0.000458661602210f};
        const float a2[4] = {0.130659527668286f, 0.139942324101744f, 0.063427417320019f, 0.009695946122598f};
        const float a1[4] = {0.498799810682272f, 0.495635523139337f, 0.695956496475118f, 0.930734667215156f};
        const float a0[4] = {0.693203116424741f, 0.692140569840976f, 0.514272634594009f, 0.168037164329057f};
        LT[4 * lane + 0] = (double) a3[lane]; LT[4 * lane + 1] = (double) a2[lane];
        LT[4 * lane + 2] = (double) a1[lane]; LT[4 * lane + 3] = (double) a0[lane];
    }
    const long long ckid = ck0 + (long long) blockIdx.x * 64 + lane;
    sa_ck_t ck = {0, 0, 0};
    if (ckid < ck1) ck = P.cks[ckid];
    const int nA = ck.nA, nB = ck.nB;
    const int maxlen = wave_max_i(nA > nB ? nA : nB);
    const int vo_lo = (int) (ck.voff & 0xffffffffll), vo_hi = (int) (ck.voff >> 32);
    double tA = NEG_INF, tB = NEG_INF;
    constexpr int CPL = 64 / FOLD_TW;              // checkpoints per load instruction
    const int sub = lane / FOLD_TW, t = lane % FOLD_TW;
    __syncthreads();
    for (int j0 = 0; j0 < maxlen; j0 += FOLD_TW) {
#pragma unroll 4
        for (int c0 = 0; c0 < 64; c0 += CPL) {
            const int c = c0 + sub;                // this lane's checkpoint of the load
            const int cnA = __shfl(nA, c), cnB = __shfl(nB, c);
            const long long vo = ((long long) __shfl(vo_hi, c) << 32) | (unsigned int) __shfl(vo_lo, c);
            const int j = j0 + t;
            double va = NEG_INF, vb = NEG_INF;     // -inf past the end: logAdd(t, -inf) == t
            if (j < cnA) va = P.vbuf[vo + j];
            if (j < cnB) vb = P.vbuf[vo + cnA + j];
            tileA[c * FOLD_LD + t] = va;
            tileB[c * FOLD_LD + t] = vb;
        }
        __syncthreads();
        const int lim = maxlen - j0 < FOLD_TW ? maxlen - j0 : FOLD_TW;
        for (int i = 0; i < lim; i++) {
            tA = la_exact_bf(LT, tA, tileA[lane * FOLD_LD + i]);
            tB = la_exact_bf(LT, tB, tileB[lane * FOLD_LD + i]);
        }
        __syncthreads();
    }
    if (ckid < ck1) P.totals[ckid] = (nB > 0) ? la_exact_bf(LT, tA, tB) : tA;
}

// ---------------------------------------------------------------------------------------------------
// finalize: posterior, threshold, floor; count survivors per segment
// ---------------------------------------------------------------------------------------------------
// The speculative total of every traceback segment of the ring / strip kernels (sa_strip.inc, "the speculative total of a
// traceback"): log-sum-exp over the cell-paths and states of the segment's first diagonal of forward state + end state, from the
// three planes the forward sweeps of these kernels keep on such diagonals.  One wave per segment, between the two sweeps of a pass;
// segments of other kernel families keep their NaN.
__global__ __launch_bounds__(64) void k_spec_match(DevPlan P, int seg0, int n_segs, double *__restrict__ spec) {
    if ((int) blockIdx.x >= n_segs) return;
    const int seg = seg0 + blockIdx.x;
    const sa_seg_t *S = &P.segs[seg];
    const sa_region_t *R = &P.regions[S->region];
    if (R->kind != SA_KIND_RING && R->kind != SA_KIND_FAST) return;
    const sa_row_t *rows = P.rows + R->row_off;
    const long long start = S->start;
    const long long o0 = rows[start].foff & 0xffffffffll, o1 = rows[start + 1].foff & 0xffffffffll;   // (g0 << 32 | offset; row N + 1 closes)
    const long long C = R->f_cellpaths;
    const double *Fm = P.F + 3 * R->f_base + o0;   // planes [match | gapX | gapY] of C cell-paths each
    const int np = (int) (o1 - o0), lane = threadIdx.x;
    const bool ragged_end = S->at_end && R->ragged_r;   // endStateProb / raggedEndStateProb (impl/stateMachine.c:1145-1173)
    const double em = ragged_end ? (P.m.t_mx + P.m.t_my) / 2.0 : P.m.t_mm, ex = ragged_end ? P.m.t_xx : P.m.t_xm,
                 ey = ragged_end ? P.m.t_yy : P.m.t_ym;
    double mx = NEG_INF;
    for (int j = lane; j < np; j += 64) {
        const double a = Fm[j] + em, b_ = Fm[C + j] + ex, c = Fm[2 * C + j] + ey;
        const double v = a > b_ ? (a > c ? a : c) : (b_ > c ? b_ : c);
        mx = v > mx ? v : mx;
    }
    mx = wave_max(mx);
    double sum = 0.0;
    if (mx > NEG_INF)
        for (int j = lane; j < np; j += 64) sum += exp(Fm[j] + em - mx) + exp(Fm[C + j] + ex - mx) + exp(Fm[2 * C + j] + ey - mx);
    sum = wave_sum(sum);
    if (lane == 0) {
        double r = (mx > NEG_INF && sum > 0.0) ? mx + log(sum) : NEG_INF;
        // NaN means "a segment of another kernel family" to the kernels that read this array: a NaN that comes out of the DATA (an
        // event mean or a model entry that is not a number poisons the forward values) must not pass for that -- the traceback
        // would return nothing without a word.  It is reported instead (sa_batch_run: SA_EINVAL).
        if (!(sum == sum) || !(mx == mx)) { r = NEG_INF; P.overflow[2] = 1; }
        spec[seg] = r;
    }
}

// An event mean that is not a finite number: the reference's logAdd turns such a cell's NaN into NaN everywhere (every comparison
// with it is false), the kernels' max/min drop it silently -- the read would come back with an alignment that steps around the
// event, or with none.  One coalesced pass over the batch's event means per run (80 MB per 2000 x 5000-event reads: ~0.03 ms)
// raises P.overflow[2] instead, whatever path brought the events here (packed by the host, gathered from the caller's block).
__global__ __launch_bounds__(256) void k_check_events(const double *__restrict__ ev, long long n, int *flag) {
    bool bad = false;
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < n; i += (long long) gridDim.x * 256) {
        const unsigned hi = (unsigned) __double2hiint(ev[i]);
        bad = bad || ((hi >> 20) & 0x7ffu) == 0x7ffu;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) flag[2] = 1;
}

// spec (register, ring and strip kernels, sa_strip.inc): per segment the speculative total its candidate bound was derived from, NaN
// for every other segment.  The bound is only valid while no exact total of the segment lies below spec - slack: checked here,
// raised in P.overflow[1] (the pass is then repeated with a larger slack).
// vc_bits (SA_FLAG_VC_ROWS): one bit per reference position of every job (job j's from bit vc_off[j] on): set where the k-mer that
// starts there holds the ambiguity letter 'X' -- the rows writePosteriorProbsVC prints (impl/signalMachine.c:161-232).  Pairs
// elsewhere are counted and summed into seg_all (their number and the sum of their floor(p 1e7), what
// scoreByPosteriorProbabilityIgnoringGaps needs) and dropped here, on the device.
__global__ __launch_bounds__(64) void k_finalize(DevPlan P, int seg0, int n_segs, long long *prob_e7, int *seg_pass,
                                                 const double *__restrict__ spec, double spec_slack,
                                                 const unsigned long long *__restrict__ vc_bits, const long long *__restrict__ vc_off,
                                                 long long *__restrict__ seg_all) {
    if ((int) blockIdx.x >= n_segs) return;
    int seg = seg0 + blockIdx.x;
    const sa_seg_t *S = &P.segs[seg];
    int n = P.cand_count[seg];
    int lane = threadIdx.x;
    int cnt = 0;
    long long all_n = 0, all_sum = 0;
    const sa_region_t *Rv = &P.regions[S->region];
    const long long vc_base = vc_bits ? vc_off[Rv->job] : 0;
    if (spec) {
        const double sp = spec[seg];
        if (sp == sp && sp > NEG_INF) {
            bool bad = false;
            for (int c = lane; c < S->n_ck; c += 64) bad = bad || (P.totals[S->ck_base + c] < sp - spec_slack + 1e-9);
            if (__ballot(bad) && lane == 0) P.overflow[1] = 1;
        }
    }
    for (int i = lane; i < ((n + 63) & ~63); i += 64) {
        bool pass = false;
        if (i < n) {
            sa_cand_t c = P.cands[S->cand_off + i];
            long long e = (long long) c.x + c.y + 2;
            double total = P.totals[S->ck_base + (S->from - e) / SA_CKPT_EVERY];
            double p = exp(c.fb - total);
            long long v = -1;
            if (p >= P.threshold) {
                if (p > 1.0) p = 1.0;
                v = (long long) floor(p * SA_PROB_1);
                pass = true;
            }
            if (vc_bits && pass) {
                all_n++; all_sum += v;
                const long long bit = vc_base + (long long) c.x + Rv->x1;
                if (!((vc_bits[bit >> 6] >> (bit & 63)) & 1ull)) { pass = false; v = -1; }
            }
            prob_e7[S->cand_off + i] = v;
        }
        cnt += __popcll(__ballot(pass));
    }
    if (lane == 0) seg_pass[seg] = cnt;
    if (vc_bits) {
        for (int off = 32; off > 0; off >>= 1) { all_n += __shfl_xor(all_n, off, 64); all_sum += __shfl_xor(all_sum, off, 64); }
        if (lane == 0) { seg_all[2ll * seg] = all_n; seg_all[2ll * seg + 1] = all_sum; }
    }
}

// Expectation pass: the per-read sums on the device.  Every checkpoint group holds its seven transition sums scaled by its
// maximum (gsum / gmc) and its exact total (k_fold); a read's expectations are sum_groups gsum * exp(gmc - total), its
// likelihood the totals once per diagonal (hmm->likelihood += totalProbability, impl/pairwiseAligner.c:1432).  One wave per
// region, a lane per checkpoint group; 8 doubles per read come back instead of 80 bytes per group (130 MB per 2000 reads).
// Bit-reproducible from run to run: a read's regions (consecutive in the plan) are summed by ONE wave in region order -- the
// wave of the read's first region; the others return -- with a fixed lane assignment and a fixed butterfly, no atomics.  What is
// NOT the reference's order of additions: it adds cell by cell and the likelihood once per diagonal (:1432) where this adds
// total * rows; transition expectations agree with the restatement to 1e-9 relative and the likelihood to 1e-12
// (tests/test_gpu_expectations.py) -- that tolerance, not bit equality, is the parity statement of this entry point.
__global__ __launch_bounds__(64) void k_expect_reduce(DevPlan P, double *__restrict__ red, int n_regions) {
    const int r0 = (int) blockIdx.x;
    const int job = P.regions[r0].job;
    if (r0 > 0 && P.regions[r0 - 1].job == job) return;
    const int lane = threadIdx.x;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = r0; r < n_regions && P.regions[r].job == job; r++) {
        const sa_region_t *R = &P.regions[r];
        for (long long sg = R->seg_off; sg < R->seg_off + R->n_seg; sg++) {
            const sa_seg_t *S = &P.segs[sg];
            const long long nrows = S->from - S->to;
            for (int c = lane; c < S->n_ck; c += 64) {
                const double total = P.totals[S->ck_base + c];
                long long rows_here = nrows - (long long) c * SA_CKPT_EVERY;
                if (rows_here > SA_CKPT_EVERY) rows_here = SA_CKPT_EVERY;
                if (rows_here > 0) acc[7] += total * (double) rows_here;
                if (!(total > NEG_INF)) continue;
                const double sc = exp(P.gmc[S->ck_base + c] - total);
                for (int k = 0; k < 7; k++) acc[k] += P.gsum[8 * (S->ck_base + c) + k] * sc;
            }
        }
    }
    for (int k = 0; k < 8; k++) {
        double v = acc[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) red[8ll * job + k] = v;
    }
}

// exclusive scan of seg_pass (single block)
// out_host (pinned host memory, written straight from the kernel) spares a copy-engine transfer: a queued copy that
// waits for a kernel blocks every later copy on the engine, including the pair copies of groups already finished
__global__ __launch_bounds__(1024) void k_scan(const int *in, long long *out, long long *out_host, int n) {
    __shared__ long long part[1024];
    int t = threadIdx.x;
    int per = (n + 1023) / 1024;
    int lo = t * per, hi = lo + per < n ? lo + per : n;
    long long s = 0;
    for (int i = lo; i < hi; i++) s += in[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        long long v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long base = t ? part[t - 1] : 0;
    for (int i = lo; i < hi; i++) {
        out[i] = base;
        out_host[i] = base;
        base += in[i];
    }
    if (t == 1023) { out[n] = part[1023]; out_host[n] = part[1023]; }
}

// gather survivors of a segment in REVERSE candidate order (=> ascending diagonals, x descending, path descending:
// the order of stList_pop + stable sort by x+y, impl/pairwiseAligner.c:2043-2050, impl/signalMachine.c:872)
// seg_off: exclusive scan over the n_segs segments starting at seg0 (indexed from 0); out: first slot of that range
// spec: per segment its speculative total where the ring / strip kernels produced the candidates (NaN elsewhere), or nullptr.
//   * a strip segment's candidates arrive strip by strip: k_gather_sorted writes it;
//   * a ring segment's candidates arrive diagonal by diagonal (the workgroup's barrier separates diagonals) but, inside a
//     diagonal, in the order the waves got there: a survivor's place is the number of survivors ahead of it in the list, minus
//     those of its own diagonal among them, plus those of its own diagonal with a smaller (column, path) -- its neighbours in the
//     list, a handful.
// a result record at slot `pos` of a group's range: 16 bytes, or (SA_FLAG_PAIRS8: one path per cell, coordinates below 2^20) 8
__device__ __forceinline__ void put_pair(sa_pair16_t *out, long long pos, int p8, long long pe, int x, int y, int path, int kmer) {
    if (p8) reinterpret_cast<unsigned long long *>(out)[pos] = sa_pair8_pack(pe, x, y);
    else out[pos] = sa_pair16_pack(pe, x, y, path, kmer);
}
__global__ __launch_bounds__(64) void k_gather(DevPlan P, int seg0, int n_segs, const long long *prob_e7,
                                               const long long *seg_off, sa_pair16_t *out, const double *__restrict__ spec, int strip_on,
                                               int p8) {
    if ((int) blockIdx.x >= n_segs) return;
    const int lseg = blockIdx.x;
    int seg = seg0 + lseg;
    const sa_seg_t *S = &P.segs[seg];
    const sa_region_t *R = &P.regions[S->region];
    const int *poff = P.poff + R->poff_off;
    const int *pid = P.pid + R->pid_off;
    int n = P.cand_count[seg];
    int lane = threadIdx.x;
    long long total = seg_off[lseg + 1] - seg_off[lseg];
    long long done = 0;
    bool unordered = false;
    if (spec) {
        const double sp = spec[seg];
        if (sp == sp) {
            if (strip_region(R, strip_on)) return;
            unordered = R->kind == SA_KIND_RING;   // (a register-kernel segment is one wave: its candidates are in order)
        }
    }
    const sa_cand_t *cd = P.cands + S->cand_off;
    const long long *pe = prob_e7 + S->cand_off;
    for (int base = 0; base < n; base += 64) {
        int i = base + lane;
        bool pass = i < n && pe[i] >= 0;
        unsigned long long mask = __ballot(pass);
        int rank = __popcll(mask & ((1ull << lane) - 1ull));
        if (pass) {
            sa_cand_t c = cd[i];
            long long k = done + rank;              // index in candidate order
            if (unordered) {
                const int e_i = c.x + c.y;
                const long long key_i = ((long long) c.x << 20) | c.path;
                int same_before = 0, less = 0;
                for (int j = i - 1; j >= 0; j--) {
                    const sa_cand_t q = cd[j];
                    if (q.x + q.y != e_i) break;
                    if (pe[j] >= 0) { same_before++; less += (((long long) q.x << 20) | q.path) < key_i ? 1 : 0; }
                }
                for (int j = i + 1; j < n; j++) {
                    const sa_cand_t q = cd[j];
                    if (q.x + q.y != e_i) break;
                    if (pe[j] >= 0) less += (((long long) q.x << 20) | q.path) < key_i ? 1 : 0;
                }
                k += less - same_before;
            }
            long long pos = seg_off[lseg] + (total - 1 - k);
            put_pair(out, pos, p8, pe[i], (int) (c.x + R->x1), (int) (c.y + R->y1), c.path, pid[poff[c.x + 1] + c.path]);
        }
        done += __popcll(mask);
    }
}

// The same for the segments of the ring kernels and of the strip kernels (sa_ring.inc, sa_strip.inc), whose candidates are
// appended in the order the waves / strips get to them instead of in candidate order (diagonals downwards, columns upwards, a
// cell's paths upwards): the survivors are put in candidate order first -- a counting sort by diagonal (histogram of the
// segment's diagonals in LDS, GATHER_H at a time), then every diagonal's few survivors by (column, path) -- and written as k_gather
// writes them.  A survivor's key: diagonals below the start << 40 | column << 12 | path (28 and 12 bits: the planners' limits are
// 2^28 columns and 255 paths per cell on these kernels); its candidate slot travels beside the key.  keys / idx: 12 bytes of
// scratch per candidate slot.  The result does not depend on the order the candidates arrived in.
#define GATHER_H 1024   // (4 KB of LDS per wave: 8192 entries held a wave to four per CU and cost the realistic batch 0.97 ms)
__global__ __launch_bounds__(64) void k_gather_sorted(DevPlan P, int seg0, int n_segs, const long long *prob_e7, const long long *seg_off,
                                                      sa_pair16_t *out, const double *__restrict__ spec,
                                                      unsigned long long *keys_all, unsigned *idx_all, int p8) {
    __shared__ int H[GATHER_H + 64];
    if ((int) blockIdx.x >= n_segs) return;
    const int lseg = blockIdx.x, seg = seg0 + lseg;
    { const double sp = spec[seg]; if (!(sp == sp)) return; }   // not a segment of these kernels: k_gather wrote it
    const sa_seg_t *S = &P.segs[seg];
    const sa_region_t *R = &P.regions[S->region];
    if (!strip_region(R, 1)) return;                             // a ring segment: k_gather wrote it
    const int *poff = P.poff + R->poff_off;
    const int *pid = P.pid + R->pid_off;
    const int n = P.cand_count[seg];
    const int lane = threadIdx.x;
    const long long total = seg_off[lseg + 1] - seg_off[lseg];
    if (total <= 0) return;
    volatile unsigned long long *keys = keys_all + S->cand_off;   // (written and read by different lanes: not through this CU's L1)
    volatile unsigned *idx = idx_all + S->cand_off;
    const long long start = S->start, span = S->start - S->to;   // diagonals below the start: 0 .. span - 1
    long long placed = 0;   // survivors on diagonals above the current range (all in place)
    for (long long r0 = 0; r0 < span && placed < total; r0 += GATHER_H) {
        const int hn = (int) (span - r0 < GATHER_H ? span - r0 : GATHER_H);
        for (int i = lane; i < hn + 1; i += 64) H[i] = 0;
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            if (prob_e7[S->cand_off + i] < 0) continue;
            const sa_cand_t c = P.cands[S->cand_off + i];
            const long long de = start - ((long long) c.x + c.y + 2);
            if (de >= r0 && de < r0 + hn) atomicAdd(&H[(int) (de - r0)], 1);
        }
        __syncthreads();
        // exclusive scan of H[0 .. hn) in place (a wave scan per 64 entries, carried), H[hn] = the range's count
        int carry = 0;
        for (int b0 = 0; b0 < hn; b0 += 64) {
            const int i = b0 + lane;
            const int v = i < hn ? H[i] : 0;
            int incl = v;
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(incl, off, 64);
                if (lane >= off) incl += o;
            }
            if (i < hn) H[i] = carry + incl - v;
            carry += __shfl(incl, 63, 64);
        }
        if (lane == 0) H[hn] = carry;
        __syncthreads();
        const int in_range = H[hn];
        if (in_range > 0) {
            // placement: any order inside a diagonal (sorted below); the cursor of diagonal i runs from H[i] up to the old H[i + 1]
            for (int i = lane; i < n; i += 64) {
                if (prob_e7[S->cand_off + i] < 0) continue;
                const sa_cand_t c = P.cands[S->cand_off + i];
                const long long de = start - ((long long) c.x + c.y + 2);
                if (de < r0 || de >= r0 + hn) continue;
                const int slot = atomicAdd(&H[(int) (de - r0)], 1);
                keys[placed + slot] = ((unsigned long long) de << 40) | ((unsigned long long) (unsigned) c.x << 12) | (unsigned long long) (unsigned) c.path;
                idx[placed + slot] = (unsigned) i;
            }
            __threadfence_block();
            __syncthreads();
            // H[i] is now the END of diagonal i's group (= the old start of i + 1): sort every group (a handful of entries)
            for (int i = lane; i < hn; i += 64) {
                const int ge = H[i], gs = i == 0 ? 0 : H[i - 1];
                for (int a = gs + 1; a < ge; a++) {
                    const unsigned long long k = keys[placed + a];
                    const unsigned ki = idx[placed + a];
                    int b = a - 1;
                    while (b >= gs && keys[placed + b] > k) { keys[placed + b + 1] = keys[placed + b]; idx[placed + b + 1] = idx[placed + b]; b--; }
                    keys[placed + b + 1] = k;
                    idx[placed + b + 1] = ki;
                }
            }
            __threadfence_block();
            __syncthreads();
        }
        placed += in_range;
    }
    // candidate order is ascending key order; written in reverse, as k_gather does
    for (long long k = lane; k < total; k += 64) {
        const unsigned i = idx[k];
        const sa_cand_t c = P.cands[S->cand_off + i];
        put_pair(out, seg_off[lseg] + (total - 1 - k), p8, prob_e7[S->cand_off + i], (int) (c.x + R->x1), (int) (c.y + R->y1), c.path,
                 pid[poff[c.x + 1] + c.path]);
    }
}

// Emission constants per (reference position, path) with the read's scale / shift / var folded in -- what fill_xc of the
// planner computes (sa_plan.c), here on the device: 32 bytes per path that the host neither has to write nor to upload.
// One block per region.  The per-k-mer logarithms come from tab6 (computed once per batch on the host with the C
// library's log), so the values are bit-identical to the host's.
__global__ __launch_bounds__(256) void k_fill_xc(const sa_region_t *__restrict__ regions, const int *__restrict__ poff_all,
                                                 const int *__restrict__ pid_all, const double *__restrict__ tab6,
                                                 const int *__restrict__ hdp_slot, long long hdp_grid_length, double4 *xc, int emission) {
    const sa_region_t *R = &regions[blockIdx.x];
    const int *poff = poff_all + R->poff_off;
    const int *pid = pid_all + R->pid_off;
    const long long n = poff[R->lX + 1];
    double4 *o = xc + R->pid_off;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
        const int id = pid[i];
        double4 v;
        if (hdp_slot) {   // e' = e/var - v.x; v.y = byte offset of the k-mer's {y, slope} row (or past the table: no density)
            const double mu = id >= 0 ? tab6[6ll * id] : 0.0;
            const int slot = id >= 0 ? hdp_slot[id] : -1;
            v.x = ((R->scale - R->var) * mu + R->shift) / R->var;
            v.y = slot >= 0 ? (double) ((long long) slot * hdp_grid_length * 16) : (double) SA_HDP_FAST_MAX_BYTES;
            v.z = 0.0; v.w = 0.0;
        } else if (id < 0) {   // NULL k-mer: both emissions are log(0); inv_s = 1 keeps (e - m) * inv_s finite
            v.x = 0.0; v.y = 1.0; v.z = NEG_INF; v.w = NEG_INF;
        } else {
            const double mu = tab6[6ll * id], sd = tab6[6ll * id + 1], c = tab6[6ll * id + 2], cy = tab6[6ll * id + 4];
            // (the two-distribution emissions carry no log(1 / var) -- impl/stateMachine.c:607-700 against :557-605 --, and the one on the
            // scaled model, emission 2, takes the event as it is: scale 1, shift 0, var 1)
            const double sc = emission == 2 ? 1.0 : R->scale, sh = emission == 2 ? 0.0 : R->shift, va = emission == 2 ? 1.0 : R->var;
            const double lv = emission != 0 ? 0.0 : R->lvar;
            v.x = sc * mu + sh;
            if (c == NEG_INF) {   // sd == 0: emissions_signal_logGaussPdf returns LOG_ZERO
                v.y = 1.0; v.z = NEG_INF; v.w = NEG_INF;
            } else {
                v.y = 1.0 / (va * sd);
                v.z = lv + c;
                v.w = lv + cy;
            }
        }
        o[i] = v;
    }
}
