// sa_generic.inc -- memory-resident forward / backward kernels (any band width, any number of paths per cell) and their launchers.
// Included by sa_hip.hip behind sa_fast.inc, whose la_fast and emit_gauss the RELAX flavour shares.

__device__ __forceinline__ bool legal_step(const DevModel &m, int from, int to) {
    if (from < 0 || to < 0) return true;
    return (from % m.pow_km1) == (to / m.n_alpha);
}

// ---------------------------------------------------------------------------------------------------
// The memory-resident kernels come in two flavours.  EXACT (SA_FLAG_EXACT, the expectation pass, HDP with several
// paths per cell): the reference's arithmetic in the reference's order, rows read back from global memory.
// RELAX (default for everything the register kernels cannot take: several paths per cell, windows wider than 64
// lanes): the same recurrence with the register kernels' arithmetic -- logAdd from the LDS table, Gaussian emissions
// from the folded per-position constants, legality by a float-reciprocal division -- and the three live diagonals in
// an LDS ring (dynamic shared memory: 68 doubles of logAdd table + 3 x ring_cap x 3 doubles; ring_cap == 0 keeps the
// rows in global memory).  Results agree with EXACT to ~1e-9 on a posterior (bar: 1e-5).
// ---------------------------------------------------------------------------------------------------
template <bool RELAX>
__device__ __forceinline__ double la_any(const double *LT, double x, double y) {
    return RELAX ? la_fast(LT, x, y) : la_exact(x, y);
}
// k-mer ids are < 2^24: exact in float; one correction step makes the truncated quotient exact
__device__ __forceinline__ int div_small(int a, int d, float inv_d) {
    int q = (int) ((float) a * inv_d);
    int r = a - q * d;
    q += (r >= d) ? 1 : 0;
    q -= (r < 0) ? 1 : 0;
    return q;
}
template <bool RELAX>
__device__ __forceinline__ bool legal_any(const DevModel &m, float inv_pow, float inv_alpha, int from, int to) {
    if (!RELAX) return legal_step(m, from, to);
    if (from < 0 || to < 0) return true;
    int fq = div_small(from, (int) m.pow_km1, inv_pow);
    return from - fq * (int) m.pow_km1 == div_small(to, m.n_alpha, inv_alpha);
}

// One cell-path of forward diagonal d.  P1 / P2 are rows d-1 / d-2; the function is instantiated twice so that, when both
// rows sit in the LDS ring (the rule), the compiler sees shared-memory pointers and emits ds_read: a pointer that may
// be either LDS or global is a FLAT access, and flat loads wait on the vector-memory counter as well, i.e. on the
// stores of the previous diagonal to the forward storage.
template <bool RELAX>
__device__ __forceinline__ void fwd_generic_cellpath(const DevModel &m, const ReadPar &rp, const double *LT, float inv_pow,
                                                     float inv_alpha, const sa_row_t &rd, const sa_row_t &r1, const sa_row_t &r2,
                                                     long long d, long long x01, long long x02, const int *poff, const int *pid,
                                                     const int *px, const double *ev, const double4 *xc4, const double *P1,
                                                     const double *P2, double *F, double *L0, int g0, int j, bool lds0) {
    const int g = g0 + j;
    const long long x = px[g];
    const int p = g - poff[x];
    const long long xmy = 2 * x - d, y = d - x;
    double e = y >= 1 ? ev[y - 1] : NEG_INF;
    const int id = pid[g];
    double *cur = F + 3 * (rd.foff + j);
    double *lcur = L0 + 3 * j;
    long long i_lo = xmy - 1 - r1.xmyL, i_up = xmy + 1 - r1.xmyL, i_mid = xmy - r2.xmyL;
    bool has_lo = x >= 1 && i_lo >= 0 && (i_lo >> 1) < r1.width;
    bool has_up = i_up >= 0 && (i_up >> 1) < r1.width;
    bool has_mid = d >= 2 && x >= 1 && i_mid >= 0 && (i_mid >> 1) < r2.width;
    const double *lo = has_lo ? P1 + 3 * (poff[x - 1] - poff[x01]) : nullptr;
    const double *up = has_up ? P1 + 3 * (poff[x] - poff[x01]) : nullptr;
    const double *mid = has_mid ? P2 + 3 * (poff[x - 1] - poff[x02]) : nullptr;
    int nq = x >= 1 ? poff[x] - poff[x - 1] : 0;
    const int *idq = x >= 1 ? pid + poff[x - 1] : nullptr;
    {
        double sm = NEG_INF, sx = NEG_INF, sy = NEG_INF;
        double eM, eY;  // match / gapY emission of this cell-path
        if (RELAX) {
            emit_gauss(xc4[g], e, eM, eY);
        } else {
            eM = has_mid ? emit_ref(m, rp, id, e, 1, y - 1) : NEG_INF;
            eY = has_up ? emit_ref(m, rp, id, e, 0, y - 1) : NEG_INF;
        }
        if (has_lo) {
            double eP = (m.hdp || id >= 0) ? SA_LOG_GAPX : NEG_INF;
            for (int q = 0; q < nq; q++)
                if (legal_any<RELAX>(m, inv_pow, inv_alpha, idq[q], id)) {
                    sx = la_any<RELAX>(LT, sx, lo[3 * q + 0] + (eP + m.t_mx));
                    sx = la_any<RELAX>(LT, sx, lo[3 * q + 1] + (eP + m.t_xx));
                }
        }
        if (has_mid) {
            double eP = eM;
            for (int q = 0; q < nq; q++)
                if (legal_any<RELAX>(m, inv_pow, inv_alpha, idq[q], id)) {
                    sm = la_any<RELAX>(LT, sm, mid[3 * q + 0] + (eP + m.t_mm));
                    sm = la_any<RELAX>(LT, sm, mid[3 * q + 1] + (eP + m.t_xm));
                    sm = la_any<RELAX>(LT, sm, mid[3 * q + 2] + (eP + m.t_ym));
                }
        }
        if (has_up) {
            double eP = eY;
            sy = la_any<RELAX>(LT, sy, up[3 * p + 0] + (eP + m.t_my));
            sy = la_any<RELAX>(LT, sy, up[3 * p + 2] + (eP + m.t_yy));
        }
        cur[0] = sm;
        cur[1] = sx;
        cur[2] = sy;
        if (lds0) { lcur[0] = sm; lcur[1] = sx; lcur[2] = sy; }
    }

}

// ---------------------------------------------------------------------------------------------------
// generic forward: cellCalculate with doTransitionForward (impl/stateMachine.c:1306-1437,
// impl/pairwiseAligner.c:852-858, :1280-1322).  Row layout: [cell-path][3].
// ---------------------------------------------------------------------------------------------------
template <bool RELAX>
__global__ __launch_bounds__(128) void k_fwd_generic(DevPlan P, const int *region_ids, int n, int ring_cap) {
    extern __shared__ __attribute__((aligned(32))) double dyn_lds[];
    double *LT = dyn_lds;                          // RELAX only
    double *lring = dyn_lds + LA_TAB_DOUBLES;      // RELAX && ring_cap > 0: rows d, d-1, d-2 as [cell-path][3]
    int w = blockIdx.x;
    if (w >= n) return;
    // one lane per cell-path of a diagonal: 64 threads, or 128 (two waves sharing the LDS ring) when some diagonal of the
    // launch holds more than 64 cell-paths -- ambiguous positions put ~70 on a 51-cell band, and a second pass of one
    // wave over the last few would double the time of every diagonal
    const int lane = threadIdx.x, nthr = blockDim.x;
    if (RELAX) {
        la_tab_init(LT, lane);
        __syncthreads();
    }
    const bool use_ring = RELAX && ring_cap > 0;
    const float inv_pow = 1.0f / (float) P.m.pow_km1, inv_alpha = 1.0f / (float) P.m.n_alpha;
    const sa_region_t *R = &P.regions[region_ids[w]];
    const double4 *xc4 = reinterpret_cast<const double4 *>(P.xc) + R->pid_off;
    const sa_row_t *rows = P.rows + R->row_off;
    const int *poff = P.poff + R->poff_off;
    const int *pid = P.pid + R->pid_off;
    const int *px = P.px + R->pid_off;
    const double *ev = P.ev + R->ev_off;
    double *F = P.F + 3 * R->f_base;
    const DevModel &m = P.m;
    ReadPar rp = {R->scale, R->shift, R->var, R->lvar, P.evn ? P.evn + 2 * R->ev_off : nullptr};
    const long long N = R->N;

    {   // diagonal 0: startStateProb / raggedStartStateProb (impl/stateMachine.c:1134-1143)
        sa_row_t r0 = rows[0];
        long long x0 = (0 + r0.xmyL) / 2;
        for (int i = lane; i < r0.width; i += nthr) {
            long long x = x0 + i;
            int np = poff[x + 1] - poff[x];
            double *c = F + 3 * (r0.foff + poff[x] - poff[x0]);
            double *lc = lring + 3 * (poff[x] - poff[x0]);
            const bool row_in_lds = use_ring && poff[x0 + r0.width] - poff[x0] <= ring_cap;
            for (int p = 0; p < np; p++) {
                c[3 * p + 0] = R->ragged_l ? NEG_INF : 0.0;
                c[3 * p + 1] = R->ragged_l ? 0.0 : NEG_INF;
                c[3 * p + 2] = R->ragged_l ? 0.0 : NEG_INF;
                if (row_in_lds) { lc[3 * p + 0] = c[3 * p + 0]; lc[3 * p + 1] = c[3 * p + 1]; lc[3 * p + 2] = c[3 * p + 2]; }
            }
        }
    }
    __syncthreads();
    for (long long d = 1; d <= N; d++) {
        sa_row_t rd = rows[d], r1 = rows[d - 1];
        sa_row_t r2 = {0, 0, 0};
        if (d >= 2) r2 = rows[d - 2];
        long long x0 = (d + rd.xmyL) >> 1;
        long long x01 = (d - 1 + r1.xmyL) >> 1;
        long long x02 = d >= 2 ? ((d - 2 + r2.xmyL) >> 1) : 0;
        // previous diagonals: the LDS ring, or the forward storage itself
        // a diagonal lives in the ring if it fits (ring_cap cell-paths); the few that do not are read back from F
        const bool lds1 = use_ring && poff[x01 + r1.width] - poff[x01] <= ring_cap;
        const bool lds2 = use_ring && d >= 2 && poff[x02 + r2.width] - poff[x02] <= ring_cap;
        const double *P1 = lds1 ? lring + ((d - 1) % 3) * (long long) ring_cap * 3 : F + 3 * r1.foff;
        const double *P2 = lds2 ? lring + ((d + 1) % 3) * (long long) ring_cap * 3 : F + 3 * r2.foff;
        double *L0 = lring + (d % 3) * (long long) ring_cap * 3;
        // one lane per cell-path of the diagonal (cells with many paths would otherwise serialise the whole wave)
        const int g0 = poff[x0];
        const int rowpaths = poff[x0 + rd.width] - g0;
        const bool lds0 = use_ring && rowpaths <= ring_cap;
        if (lds1 && (lds2 || d < 2)) {   // both previous rows in the ring: shared-memory accesses
            const double *Q1 = lring + ((d - 1) % 3) * (long long) ring_cap * 3;
            const double *Q2 = lring + ((d + 1) % 3) * (long long) ring_cap * 3;
            for (int j = lane; j < rowpaths; j += nthr)
                fwd_generic_cellpath<RELAX>(m, rp, LT, inv_pow, inv_alpha, rd, r1, r2, d, x01, x02, poff, pid, px, ev, xc4, Q1, Q2, F,
                                            L0, g0, j, lds0);
        } else {
            for (int j = lane; j < rowpaths; j += nthr)
                fwd_generic_cellpath<RELAX>(m, rp, LT, inv_pow, inv_alpha, rd, r1, r2, d, x01, x02, poff, pid, px, ev, xc4, P1, P2, F,
                                            L0, g0, j, lds0);
        }
        __syncthreads();
    }
}

// EXPECT mode: close a checkpoint group -- lane 0 stores the wave sums of exp(term - Mc) and Mc itself; the host
// rescales by exp(Mc - totalProbability) once the exact fold of the group's total is known.
__device__ __forceinline__ void expect_flush(const DevPlan &P, long long ck, double Mc, double *acc, int lane) {
    for (int k = 0; k < 7; k++) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) P.gsum[ck * 8 + k] = v;
        acc[k] = 0.0;
    }
    if (lane == 0) { P.gsum[ck * 8 + 7] = 0.0; P.gmc[ck] = Mc; }
}

// ---------------------------------------------------------------------------------------------------
// generic backward + posterior numerators + checkpoint terms.
// The reference scatters (doTransitionBackward, impl/pairwiseAligner.c:866-871); here each cell GATHERS
// the same terms in the same order: first from (x+1,y+1) (it was that cell's "middle"), then from (x,y+1)
// (its "upper"), then from (x+1,y) (its "lower").  Backward rows live in a 3-row ring in memory.
// ---------------------------------------------------------------------------------------------------
template <bool EXPECT, bool RELAX>
__global__ __launch_bounds__(128) void k_bwd_generic(DevPlan P, const int *seg_ids, int n, int ring_cap) {
    extern __shared__ __attribute__((aligned(32))) double dyn_lds[];
    double *LT = dyn_lds;                          // RELAX only
    double *lring = dyn_lds + LA_TAB_DOUBLES;      // RELAX && ring_cap > 0: backward rows e, e+1, e+2
    int w = blockIdx.x;
    if (w >= n) return;
    // 64 or 128 threads (see k_fwd_generic): the cell-path sweep of a diagonal is shared by all threads; what follows a
    // diagonal (checkpoint terms, candidates, expectations: per cell, wave-wide scans) is the first wave's alone, while
    // the second goes on to the barrier of the next diagonal
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
    const bool first_wave = tid < 64;
    if (RELAX) {
        la_tab_init(LT, tid);
        __syncthreads();
    }
    const bool use_ring = RELAX && ring_cap > 0;
    const float inv_pow = 1.0f / (float) P.m.pow_km1, inv_alpha = 1.0f / (float) P.m.n_alpha;
    const int seg = seg_ids[w];
    const sa_seg_t *S = &P.segs[seg];
    const sa_region_t *R = &P.regions[S->region];
    const sa_row_t *rows = P.rows + R->row_off;
    const int *poff = P.poff + R->poff_off;
    const int *pid = P.pid + R->pid_off;
    const double *ev = P.ev + R->ev_off;
    const double *F = P.F + 3 * R->f_base;
    const DevModel &m = P.m;
    ReadPar rp = {R->scale, R->shift, R->var, R->lvar, P.evn ? P.evn + 2 * R->ev_off : nullptr};
    // backward rows: the LDS ring for diagonals of at most ring_cap cell-paths, the global ring for the others
    const long long grow = R->max_rowpaths;
    double *gring = P.bscratch + S->bscratch_off;  // 3 rows x grow x 3
    const double4 *xc4 = reinterpret_cast<const double4 *>(P.xc) + R->pid_off;
    const int *px = P.px + R->pid_off;
    const long long start = S->start, from = S->from, to = S->to;
    double end_m, end_x, end_y;  // endStateProb / raggedEndStateProb (impl/stateMachine.c:1145-1173)
    if (S->at_end && R->ragged_r) {
        end_m = (m.t_mx + m.t_my) / 2.0; end_x = m.t_xx; end_y = m.t_yy;
    } else {
        end_m = m.t_mm; end_x = m.t_xm; end_y = m.t_ym;
    }
    int count = 0;
    double Mc = NEG_INF;
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};  // EXPECT: sum of exp(term - Mc) per live transition, current checkpoint group
    for (long long e = start; e > to; e--) {
        sa_row_t re = rows[e];
        long long x0 = (e + re.xmyL) >> 1;
        auto row_ptr = [&](long long row, long long xfirst, int width) -> double * {
            const bool in_lds = use_ring && poff[xfirst + width] - poff[xfirst] <= ring_cap;
            return in_lds ? lring + (row % 3) * (long long) ring_cap * 3 : gring + (row % 3) * grow * 3;
        };
        double *Be = row_ptr(e, x0, re.width);
        sa_row_t r1 = {0, 0, 0}, r2 = {0, 0, 0};
        long long x01 = 0, x02 = 0;
        const double *B1 = nullptr, *B2 = nullptr;
        if (e + 1 <= start) {
            r1 = rows[e + 1];
            x01 = (e + 1 + r1.xmyL) >> 1;
            B1 = row_ptr(e + 1, x01, r1.width);
        }
        if (e + 2 <= start) {
            r2 = rows[e + 2];
            x02 = (e + 2 + r2.xmyL) >> 1;
            B2 = row_ptr(e + 2, x02, r2.width);
        }
        // one lane per cell-path of the diagonal
        const int g0 = poff[x0];
        const int rowpaths = poff[x0 + re.width] - g0;
        for (int j = tid; j < rowpaths; j += nthr) {
            const int g = g0 + j;
            const long long x = px[g];
            const int q = g - poff[x];
            const long long xmy = 2 * x - e, y = e - x;
            double *cur = Be + 3 * j;
            if (e == start) {
                cur[0] = end_m; cur[1] = end_x; cur[2] = end_y;
                continue;
            }
            long long i_mid = xmy - r2.xmyL, i_up = xmy - 1 - r1.xmyL, i_lo = xmy + 1 - r1.xmyL;
            bool has_mid = B2 && i_mid >= 0 && (i_mid >> 1) < r2.width && x + 1 <= R->lX;
            bool has_up = B1 && i_up >= 0 && (i_up >> 1) < r1.width;                    // cell (x, y+1)
            bool has_lo = B1 && i_lo >= 0 && (i_lo >> 1) < r1.width && x + 1 <= R->lX;  // cell (x+1, y)
            const double *cm = has_mid ? B2 + 3 * (poff[x + 1] - poff[x02]) : nullptr;
            const double *cu = has_up ? B1 + 3 * (poff[x] - poff[x01]) : nullptr;
            const double *cl = has_lo ? B1 + 3 * (poff[x + 1] - poff[x01]) : nullptr;
            int nn = (x + 1 <= R->lX) ? poff[x + 2] - poff[x + 1] : 0;
            const int *idn = (x + 1 <= R->lX) ? pid + poff[x + 1] : nullptr;
            double e_next = (y < R->lY) ? ev[y] : NEG_INF;  // event of matrix row y+1
            {
                int idq = pid[g];
                double tm = NEG_INF, tx = NEG_INF, ty = NEG_INF;
                if (has_mid)
                    for (int p = 0; p < nn; p++)
                        if (legal_any<RELAX>(m, inv_pow, inv_alpha, idq, idn[p])) {
                            double eP, eU;
                            if (RELAX) emit_gauss(xc4[poff[x + 1] + p], e_next, eP, eU);
                            else eP = emit_ref(m, rp, idn[p], e_next, 1, y);
                            double c = cm[3 * p + 0];
                            tm = la_any<RELAX>(LT, tm, c + (eP + m.t_mm));
                            tx = la_any<RELAX>(LT, tx, c + (eP + m.t_xm));
                            ty = la_any<RELAX>(LT, ty, c + (eP + m.t_ym));
                        }
                if (has_up) {
                    double eP, eU;
                    if (RELAX) emit_gauss(xc4[g], e_next, eU, eP);
                    else eP = emit_ref(m, rp, idq, e_next, 0, y);
                    double c = cu[3 * q + 2];
                    tm = la_any<RELAX>(LT, tm, c + (eP + m.t_my));
                    ty = la_any<RELAX>(LT, ty, c + (eP + m.t_yy));
                }
                if (has_lo)
                    for (int p = 0; p < nn; p++)
                        if (legal_any<RELAX>(m, inv_pow, inv_alpha, idq, idn[p])) {
                            double eP = (m.hdp || idn[p] >= 0) ? SA_LOG_GAPX : NEG_INF;
                            double c = cl[3 * p + 1];
                            tm = la_any<RELAX>(LT, tm, c + (eP + m.t_mx));
                            tx = la_any<RELAX>(LT, tx, c + (eP + m.t_xx));
                        }
                cur[0] = tm; cur[1] = tx; cur[2] = ty;
            }
        }
        __syncthreads();
        if (e > from || !first_wave) continue;
        // ---- checkpoint: per-cell terms of diagonalCalculationTotalProbability (impl/pairwiseAligner.c:1335-1353)
        if ((from - e) % SA_CKPT_EVERY == 0) {
            if (EXPECT && e != from) expect_flush(P, S->ck_base + (from - e) / SA_CKPT_EVERY - 1, Mc, acc, lane);
            const sa_ck_t ck = P.cks[S->ck_base + (from - e) / SA_CKPT_EVERY];
            double mx = NEG_INF;
            for (int i = lane; i < re.width; i += 64) {
                long long x = x0 + i;
                int np = poff[x + 1] - poff[x];
                const double *cf = F + 3 * (re.foff + poff[x] - poff[x0]);
                const double *cb = Be + 3 * (poff[x] - poff[x0]);
                double cell = NEG_INF;
                for (int q = 0; q < np; q++) {
                    double t = cf[3 * q] + cb[3 * q];
                    t = la_any<RELAX>(LT, t, cf[3 * q + 1] + cb[3 * q + 1]);
                    t = la_any<RELAX>(LT, t, cf[3 * q + 2] + cb[3 * q + 2]);
                    cell = la_any<RELAX>(LT, cell, t);
                }
                P.vbuf[ck.voff + i] = cell;
                mx = cell > mx ? cell : mx;
            }
            if (ck.nB > 0) {  // match-only forward step into diagonal e+1 == F[e+1].match (same arithmetic, same band)
                for (int i = lane; i < r1.width; i += 64) {
                    long long x = x01 + i;
                    int np = poff[x + 1] - poff[x];
                    const double *cf = F + 3 * (r1.foff + poff[x] - poff[x01]);
                    const double *cb = B1 + 3 * (poff[x] - poff[x01]);
                    double cell = NEG_INF;
                    for (int q = 0; q < np; q++) cell = la_any<RELAX>(LT, cell, cf[3 * q] + cb[3 * q]);
                    P.vbuf[ck.voff + ck.nA + i] = cell;
                    mx = cell > mx ? cell : mx;
                }
            }
            Mc = wave_max(mx);
        }
        if (!EXPECT) {
        // ---- posterior candidates of this diagonal (impl/pairwiseAligner.c:1355-1421); total >= Mc
        int nchunks = (re.width + 63) >> 6;
        for (int c = 0; c < nchunks; c++) {
            int i = c * 64 + lane;
            bool in = i < re.width;
            long long x = x0 + (in ? i : 0), y = e - x;
            int np = (in && x > 0 && y > 0) ? poff[x + 1] - poff[x] : 0;
            const double *cf = F + 3 * (re.foff + poff[x] - poff[x0]);
            const double *cb = Be + 3 * (poff[x] - poff[x0]);
            const double lim = Mc + P.log_thr - SA_CAND_EPS;
            int mine = 0;
            if (Mc > NEG_INF)
                for (int q = 0; q < np; q++) mine += (cf[3 * q] + cb[3 * q] >= lim) ? 1 : 0;
            // exclusive prefix over lanes: candidates are laid out cell by cell, path by path
            int incl = mine;
            for (int off = 1; off < 64; off <<= 1) {
                int o = __shfl_up(incl, off, 64);
                if (lane >= off) incl += o;
            }
            int total = __shfl(incl, 63, 64);
            int pos = count + incl - mine;
            if (mine > 0)
                for (int q = 0; q < np; q++) {
                    double fb = cf[3 * q] + cb[3 * q];
                    if (fb >= lim) {
                        if (pos < S->cand_cap) {
                            sa_cand_t cd;
                            cd.x = (int) (x - 1); cd.y = (int) (y - 1); cd.path = q; cd.pad = 0; cd.fb = fb;
                            P.cands[S->cand_off + pos] = cd;
                        } else {
                            P.overflow[0] = 1;
                        }
                        pos++;
                    }
                }
            count += total;
        }
        } else {
        // ---- EXPECT: diagonalCalculation_Expectations (impl/pairwiseAligner.c:1423-1443): the cell calculation with
        // current = backward diagonal e, lower/upper = forward diagonal e-1, middle = forward diagonal e-2, every
        // transition adding exp(F[from] + B[to] + (eP + tP) - total) (cell_signal_updateExpectations :914-944).
        // Forward diagonal e-2 has already been deleted for the first diagonal of a traceback (:1563-1578).
        {
            const sa_row_t rm1 = rows[e - 1];
            const bool have2 = e - 2 >= to && e - 2 >= 0;
            sa_row_t rm2 = {0, 0, 0};
            if (have2) rm2 = rows[e - 2];
            const long long x0m1 = (e - 1 + rm1.xmyL) >> 1, x0m2 = have2 ? (e - 2 + rm2.xmyL) >> 1 : 0;
            const double lim = Mc + P.log_thr - SA_CAND_EPS;
            const bool live = Mc > NEG_INF;
            int nchunks = (re.width + 63) >> 6;
            for (int c = 0; c < nchunks; c++) {
                int i = c * 64 + lane;
                bool in = live && i < re.width;
                long long xmy = (long long) re.xmyL + 2 * (in ? i : 0);
                long long x = x0 + (in ? i : 0), y = e - x;
                int np = in ? poff[x + 1] - poff[x] : 0;
                const int *idc = pid + poff[x];
                const double *cb = Be + 3 * (poff[x] - poff[x0]);
                long long il = xmy - 1 - rm1.xmyL, iu = xmy + 1 - rm1.xmyL, im = xmy - rm2.xmyL;
                bool has_lo = in && il >= 0 && (il >> 1) < rm1.width && x >= 1;
                bool has_up = in && iu >= 0 && (iu >> 1) < rm1.width && y >= 1;
                bool has_mid = in && have2 && im >= 0 && (im >> 1) < rm2.width && x >= 1 && y >= 1;
                int nl = (has_lo || has_mid) ? poff[x] - poff[x - 1] : 0;
                const int *idl = pid + poff[x >= 1 ? x - 1 : 0];
                const double *fl = has_lo ? F + 3 * (rm1.foff + poff[x - 1] - poff[x0m1]) : nullptr;
                const double *fm = has_mid ? F + 3 * (rm2.foff + poff[x - 1] - poff[x0m2]) : nullptr;
                const double *fu = has_up ? F + 3 * (rm1.foff + poff[x] - poff[x0m1]) : nullptr;
                double e_cur = (y >= 1) ? ev[y - 1] : NEG_INF;  // NULLEVENT for y == 0 (impl/pairwiseAligner.c:509-512)
                int mine = 0;
                for (int p = 0; p < np; p++) {
                    int idp = idc[p];
                    if (has_lo) {
                        double eP = (m.hdp || idp >= 0) ? SA_LOG_GAPX : NEG_INF;
                        for (int q = 0; q < nl; q++)
                            if (legal_step(m, idl[q], idp)) {
                                acc[0] += exp(fl[3 * q + 0] + cb[3 * p + 1] + (eP + m.t_mx) - Mc);
                                acc[1] += exp(fl[3 * q + 1] + cb[3 * p + 1] + (eP + m.t_xx) - Mc);
                            }
                    }
                    if (has_mid) {
                        double eP = emit_ref(m, rp, idp, e_cur, 1, y - 1);
                        for (int q = 0; q < nl; q++)
                            if (legal_step(m, idl[q], idp)) {
                                double v2 = fm[3 * q + 0] + cb[3 * p + 0] + (eP + m.t_mm);
                                double v3 = fm[3 * q + 1] + cb[3 * p + 0] + (eP + m.t_xm);
                                double v4 = fm[3 * q + 2] + cb[3 * p + 0] + (eP + m.t_ym);
                                acc[2] += exp(v2 - Mc);
                                acc[3] += exp(v3 - Mc);
                                acc[4] += exp(v4 - Mc);
                                if (m.hdp) mine += (v2 >= lim ? 1 : 0) + (v3 >= lim ? 1 : 0) + (v4 >= lim ? 1 : 0);
                            }
                    }
                    if (has_up) {
                        double eP = emit_ref(m, rp, idp, e_cur, 0, y - 1);
                        acc[5] += exp(fu[3 * p + 0] + cb[3 * p + 2] + (eP + m.t_my) - Mc);
                        acc[6] += exp(fu[3 * p + 2] + cb[3 * p + 2] + (eP + m.t_yy) - Mc);
                    }
                }
                if (!m.hdp) continue;
                // assignment candidates (cell_signal_updateExpectationsAndAssignments :946-968), reference order
                int incl = mine;
                for (int off = 1; off < 64; off <<= 1) {
                    int o = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += o;
                }
                int total = __shfl(incl, 63, 64);
                int pos = count + incl - mine;
                if (mine > 0)
                    for (int p = 0; p < np; p++) {
                        int idp = idc[p];
                        double eP = emit_ref(m, rp, idp, e_cur, 1, y - 1);
                        for (int q = 0; q < nl; q++)
                            if (legal_step(m, idl[q], idp)) {
                                double v[3] = {fm[3 * q + 0] + cb[3 * p + 0] + (eP + m.t_mm),
                                               fm[3 * q + 1] + cb[3 * p + 0] + (eP + m.t_xm),
                                               fm[3 * q + 2] + cb[3 * p + 0] + (eP + m.t_ym)};
                                for (int t = 0; t < 3; t++)
                                    if (v[t] >= lim) {
                                        if (pos < S->cand_cap) {
                                            sa_cand_t cd;
                                            cd.x = (int) (x - 1); cd.y = (int) (y - 1); cd.path = p; cd.pad = t; cd.fb = v[t];
                                            P.cands[S->cand_off + pos] = cd;
                                        } else {
                                            P.overflow[0] = 1;
                                        }
                                        pos++;
                                    }
                            }
                    }
                count += total;
            }
        }
        }
    }
    if (EXPECT && S->n_ck > 0 && first_wave) expect_flush(P, S->ck_base + S->n_ck - 1, Mc, acc, lane);
    if (tid == 0) P.cand_count[seg] = count < S->cand_cap ? count : S->cand_cap;
}

// One workgroup of `threads` (64 / 128) per region (forward) / segment (backward).  relax: the RELAX flavour, its LDS ring
// `ring_cap` cell-paths per row; otherwise EXACT (the expectation pass among them: a batch in that pass is never relaxed).
static size_t generic_lds(bool relax, int ring_cap) {
    return relax ? sizeof(double) * (size_t) (LA_TAB_DOUBLES + 9 * ring_cap) : 0;
}
static void launch_fwd_generic(const DevPlan &P, const int *ids, int n, hipStream_t st, int threads, bool relax, int ring_cap) {
    auto k = relax ? k_fwd_generic<true> : k_fwd_generic<false>;
    hipLaunchKernelGGL(k, dim3(n), dim3(threads), generic_lds(relax, ring_cap), st, P, ids, n, relax ? ring_cap : 0);
}
static void launch_bwd_generic(const DevPlan &P, const int *ids, int n, hipStream_t st, int threads, bool relax, int ring_cap) {
    auto k = P.expect ? k_bwd_generic<true, false> : (relax ? k_bwd_generic<false, true> : k_bwd_generic<false, false>);
    hipLaunchKernelGGL(k, dim3(n), dim3(threads), generic_lds(relax, ring_cap), st, P, ids, n, relax ? ring_cap : 0);
}
