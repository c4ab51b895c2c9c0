// sa_strip.inc -- strip kernels: one-path regions whose band is wider than a wave, swept in strips of 64 REFERENCE
// COLUMNS.  Included by sa_hip.hip after sa_ring.inc (logAdd, buffer access and emission helpers are shared).
//
// Why.  The register kernels (sa_fast.inc) map a cell to a lane by its position inside the band, (x-y+K)>>1: a diagonal
// then needs its neighbours on BOTH sides, so a band wider than 64 lanes has to be spread over several waves that meet at a
// barrier every diagonal (sa_ring.inc: messages through LDS, 55-60 % of the wave cycles parked).  Here a lane is a
// reference column, x = 64 s + lane, and a wave sweeps strip s over every diagonal that crosses it before it moves on to
// strip s + 1.  The recurrence only ever looks towards smaller x (forward: (x-1,y), (x-1,y-1), (x,y-1); backward the mirror
// image), so
//   * inside a strip everything is in registers exactly as in sa_fast.inc: the lower neighbour and the middle one come
//     from lane - 1 (one DPP wave shift each per diagonal), the upper one from the lane itself; no LDS state, no barrier;
//   * between strips the dependency is one-directional: lane 63 of strip s leaves its two outgoing messages of every
//     diagonal in a seam array (16 bytes per diagonal, L2-resident), lane 0 of strip s + 1 picks them up as the `old` value
//     of the same DPP shift (lanes without a source keep it) -- a strip never waits for another wave;
//   * a lane's reference position is fixed for a whole strip: the position constants are loaded once per strip, the event
//     index is (d - 1 - x), so the per-diagonal inputs are one 8-byte event load and the broadcast seam record (two 8-byte
//     loads), requested two diagonals ahead (backward, which also streams the forward values from HBM: four), and the
//     geometry of a diagonal is two integer VALU instructions (cell index, in-band);
//   * any band shape is taken: a strip covers the diagonals [dlo, dhi] that cross its columns (found by a pass over the
//     row records when the wave starts), cells outside the band publish -inf (their emission is made -inf through the
//     addend of an fma), and the band's width only decides how many diagonals a strip has.
// Lane utilisation is (band height) / (band height + 64 (1 + events per base)): 66 % for the 124-cell bands a real guide
// alignment leaves, more for wider ones, 44 % for the 51-cell bands of dense anchors -- which stay on the register kernels.
//
// Arithmetic and order of operations per cell are those of the ring kernels' one-path flavour (messages oM, oX, oY with the
// transitions folded in, la_fast, folded Gaussian constants): results are bit-identical to theirs.
//
// Backward: a traceback segment's candidate bound depends on its total, which sums whole diagonals, and a strip only sees its
// own 64 columns of one.  So the bound comes from the segment's speculative total (below), known before the sweep starts: one
// wave sweeps the segment's strips once, appends every posterior cell that passes the bound to the segment's candidates as it
// meets it, and writes each checkpoint's per-cell terms (and the match-through terms of the diagonal above it) to vbuf in cell
// order.  The fold and finalisation kernels are those of every other kernel; k_finalize applies the exact test with the exact
// totals.
//
// Forward storage: the planes of SA_KIND_RING regions (match | gapX | gapY, gap planes on checkpoint diagonals only).

#define STRIP_WAVES 4
#define STRIP_NS_MAX 256      // strips per region: reference windows below 16384 k-mers (longer ones stay on the ring kernels)

// The regions these kernels sweep: one-path SA_KIND_RING regions with fewer than 64 * STRIP_NS_MAX reference positions, in a
// batch that runs them (strip_on).  The host's launch lists and k_gather / k_gather_sorted (which of the two writes a
// segment's pairs) both decide by this one test.
__host__ __device__ __forceinline__ bool strip_region(const sa_region_t *R, int strip_on) {
    return strip_on && R->kind == SA_KIND_RING && R->max_p == 1 && R->lX < 64ll * STRIP_NS_MAX && R->N >= 1;
}

struct StripT {
    FastT f;
    long long ev_total;              // doubles in the batch's event array (padding included): range of the event buffer
    unsigned long long seam_stride;  // bytes of seam storage per wave: two arrays of seam_cap records
    unsigned seam_cap;               // records (16 bytes) per seam array
    unsigned seam_first;             // this launch's first wave slot in the seam storage
    double *spec;                    // backward: per traceback segment its speculative total (below)
    double slack;                    // ... and how far below it the candidate bound is put (STRIP_SPEC_SLACK unless a pass is repeated)
};

// ---- the speculative total of a traceback (k_bwd_strip1; the ring kernels use it too) ----
// A traceback's posteriors are exp(f + b - total) with the total refreshed at every tenth diagonal (impl/pairwiseAligner.c:1538);
// all those totals estimate the same quantity, the probability of the data given the band, and differ only by what the
// reference's approximate logAdd and the band's clipping leave between them (~1e-3).  One of them can be bounded BEFORE the
// backward sweep starts: on the traceback's first diagonal the backward state of every cell is the end-state vector, so the
// total there is the sum over the diagonal's cells of forward state x end state: the forward sweeps of these kernels keep all
// three planes of the diagonals tracebacks start on, and k_spec_match (sa_hip.hip: one wave per segment between the two sweeps,
// true log-sum-exp) adds them up.  The backward sweep takes `spec - slack + log(threshold)` as its candidate bound, k_finalize
// applies the exact test with the exact totals of k_fold as for every other kernel, and checks that no exact total lies below
// spec - slack (if one ever does, the pass is repeated with a larger slack).
// (measured, probes/spec_probe.py: exact total - speculative total in [-7.6e-3, +4.8e-3] over the tracebacks of Gaussian reads, dense
// or sparse anchors, one or several paths per cell; with the bundled HDP model's flat densities the reference's totals drift DOWN
// along a traceback by 1.6e-4 per diagonal -- its approximate logAdd summing fifty nearly equal terms -- and end 0.15 below)
#define STRIP_SPEC_SLACK 0.5

// The DPP move's destination is also its `old` operand.  `fill` comes out of a prefetch stage (a register that lives across
// the loop's back edge): tied directly, the register allocator joins the stage register with the state register the shift
// writes, and then parks the freshly requested stage value somewhere else and copies it home on the back edge -- behind an
// s_waitcnt for a load that was issued a few instructions earlier.  The explicit move (the compiler needs one anyway) keeps
// the two apart.
__device__ __forceinline__ int strip_mov(int v) {
    int r;
    asm("v_mov_b32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}
// lane i <- lane i-1; lane 0 keeps `fill` (v_mov_b32_dpp wave_shr:1: a lane without a source is not written)
__device__ __forceinline__ double strip_from_below(double v, double fill) {
    int lo = __builtin_amdgcn_update_dpp(strip_mov(__double2loint(fill)), __double2loint(v), 0x138, 0xF, 0xF, false);
    int hi = __builtin_amdgcn_update_dpp(strip_mov(__double2hiint(fill)), __double2hiint(v), 0x138, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
// lane i <- lane i+1; lane 63 keeps `fill` (wave_shl:1)
__device__ __forceinline__ double strip_from_above(double v, double fill) {
    int lo = __builtin_amdgcn_update_dpp(strip_mov(__double2loint(fill)), __double2loint(v), 0x130, 0xF, 0xF, false);
    int hi = __builtin_amdgcn_update_dpp(strip_mov(__double2hiint(fill)), __double2hiint(v), 0x130, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

struct StripIn {
    double e;        // event mean of the lane's cell (0 where the cell has no event: such a cell is a border or outside the band)
    double sa, sb;   // seam record of the diagonal, the same in every lane
};
// two-distribution emission (the TWO instances): the noise constants {n, 1 / n, 1.5 log n} of the cell's event, requested with the
// event (zeros where the cell has no event, like the event itself).  Kept beside the stage: the other instances never name it.
struct StripTwo {
    double n, rn, l3;
};
__device__ __forceinline__ void strip_request_two(StripTwo &tw, rsrc_t rs_en, unsigned vo) {
    const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(rs_en, vo, 0, 0);
    const u32x2 b = __builtin_amdgcn_raw_buffer_load_b64(rs_en, vo, 16, 0);
    tw.n = __hiloint2double((int) a.y, (int) a.x); tw.rn = __hiloint2double((int) a.w, (int) a.z);
    tw.l3 = __hiloint2double((int) b.y, (int) b.x);
}
// the noise term of a cell (two_l2, sa_ring.inc: the same operations in the same order); a lane outside the band adds nothing --
// its emission is -inf already, and what it read may belong to another read.  One place where the two families do NOT compute the same
// term: a band cell without an event (row y = 0) reads zeros here (the descriptor's range check: l2 = cn.x) and the padding entry and
// the NULL position in the ring kernels (l2 = 0).  Both are finite, and every predecessor sum of such a cell is -inf, so the term never
// reaches a stored value: the byte equality of strip and one-path ring rests on that -- keep it in mind when the border handling changes.
__device__ __forceinline__ double strip_two_l2(const double4 &cn, const StripTwo &tw, bool act) {
    double4 n3;
    n3.x = tw.n; n3.y = tw.rn; n3.z = tw.l3; n3.w = 0.0;
    const double l2 = two_l2(cn, n3);
    return act ? l2 : 0.0;
}
// the events' half of the noise constants as the region sees it: entry y - 1 of the region, the batch's padding included
__device__ __forceinline__ rsrc_t strip_rsrc_en(const double *E_all, long long ev_off, long long two_xn_off) {
    const long long left = (two_xn_off - ev_off) * 32;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double4 *>(reinterpret_cast<const double4 *>(E_all) + ev_off), 0,
                                             (int) (left < 0x7fffffffll ? (left > 0 ? left : 0) : 0x7fffffffll), 0x00020000);
}
// A seam array holds its records' first values, then (half an array further on) their second values: two 8-byte loads the
// compiler cannot merge into one 16-byte register tuple -- a tuple does not survive the loop's back edge without a copy, and
// the copy waits for the load.  `so` = byte offset of the record's first value, `half_` = bytes between the two.
__device__ __forceinline__ void seam_store(rsrc_t rs, unsigned vo, unsigned so, unsigned half_, double a, double b) {
    u32x2 v;
    v.x = (unsigned) __double2loint(a); v.y = (unsigned) __double2hiint(a);
    __builtin_amdgcn_raw_buffer_store_b64(v, rs, vo, so, 0);
    v.x = (unsigned) __double2loint(b); v.y = (unsigned) __double2hiint(b);
    __builtin_amdgcn_raw_buffer_store_b64(v, rs, vo, so + half_, 0);
}
// device-scope load (sc1): served by L2, never by a line this CU's vector L1 fetched before the data was written
__device__ __forceinline__ double buf_load_f64_l2(rsrc_t r, unsigned voff, unsigned soff) {
    u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 16);
    return __hiloint2double((int) v.y, (int) v.x);
}

// Strip ranges: lo[s] / hi[s] = first / last diagonal of [da, db] with a cell in the columns of strip s
__device__ __forceinline__ void strip_ranges(const int4 *rows4, int da, int db, int lane, int ns, int *lo, int *hi, int &smin,
                                             int &smax) {
    for (int i = lane; i < ns; i += 64) { lo[i] = 0x7fffffff; hi[i] = -1; }
    for (int base = da; base <= db; base += 64) {
        const int d = base + lane;
        const bool ok = d <= db;
        const int4 r = rows4[ok ? d : db];
        const int sL = r.w >> 6;
        int sR = (r.w + r.y - 1) >> 6;
        if (!ok || r.y <= 0) sR = sL - 1;
        if (sR >= ns) sR = ns - 1;
        for (int s = sL; s <= sR; s++) {
            atomicMin(&lo[s], d);
            atomicMax(&hi[s], d);
        }
    }
    wave_fence();
    smin = ns; smax = -1;   // lowest / highest strip with a cell (the band is connected: every strip between them has one)
    for (int base = 0; base < ns; base += 64) {
        const int i = base + lane;
        const unsigned long long has = __ballot(i < ns && hi[i] >= lo[i]);
        if (has) {
            const int first = base + (int) __builtin_ctzll(has), last = base + 63 - (int) __builtin_clzll(has);
            smin = first < smin ? first : smin;
            smax = last > smax ? last : smax;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------
// HDP: a lane's per-diagonal input is its cell's emission from the region's emission plane (k_emit_hdp_ring, sa_fast.inc: value t
// of the diagonal at its offset + t, -inf sentinel in entry C - 1) instead of the event mean -- the request then needs the
// requested diagonal's row record (two diagonals ahead: still inside the 64-entry tile), and no position constants are loaded.
// TWO (Gaussian models only): the two-distribution emission -- E_all is then the buffer of noise constants (FastT.two_xn_off); a
// lane's position constants are loaded once per strip like the Gaussian ones, the event's arrive with the event.
template <bool HDP, bool TWO = false>
__global__ __launch_bounds__(64 * STRIP_WAVES) void k_fwd_strip(const sa_region_t *__restrict__ regions, const sa_row_t *__restrict__ rows_all,
                                                                const int *__restrict__ pk_all, const double4 *__restrict__ xc_all,
                                                                const double *__restrict__ ev_all, double *__restrict__ F_all,
                                                                char *__restrict__ seam_all, StripT ST, const int *__restrict__ region_ids,
                                                                int n, const double *__restrict__ E_all,
                                                                const sa_seg_t *__restrict__ segs_all) {
    __shared__ __attribute__((aligned(32))) double LS[LA_SITES * LA_TAB_DOUBLES];
    __shared__ int s_lo[STRIP_WAVES][STRIP_NS_MAX], s_hi[STRIP_WAVES][STRIP_NS_MAX];
    const FastT &T = ST.f;
    const LaSiteK SK = la_sites_fwd(T);
    la_tab_init_site(LS, threadIdx.x, SK.k0);
    la_tab_init_site(LS + LA_TAB_DOUBLES, threadIdx.x, SK.k1);
    la_tab_init_site(LS + 2 * LA_TAB_DOUBLES, threadIdx.x, SK.k2);
    la_tab_init_site(LS + 3 * LA_TAB_DOUBLES, threadIdx.x, SK.k3);
    __syncthreads();
    const int wv = __builtin_amdgcn_readfirstlane((int) ((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wv >= n) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const sa_region_t *R = &regions[__builtin_amdgcn_readfirstlane(region_ids[wv])];
    const int4 *rows4 = reinterpret_cast<const int4 *>(rows_all + R->row_off);
    const int *pk = pk_all + R->pk_off + SA_PK_PAD;
    const int N = (int) R->N, lX = (int) R->lX;
    const long long C = R->f_cellpaths;
    double *F = F_all + 3 * R->f_base;
    const int ns = (lX >> 6) + 1;
    int *lo = s_lo[wid], *hi = s_hi[wid];
    int smin, smax;
    strip_ranges(rows4, 0, N, lane, ns, lo, hi, smin, smax);

    const rsrc_t rs_xc = make_rsrc(xc_all + R->pid_off), rs_F = make_rsrc(F);
    const long long ev_left = (ST.ev_total - R->ev_off) * 8;
    const rsrc_t rs_ev = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(ev_all + R->ev_off), 0,
                                                           (int) (ev_left < 0x7fffffffll ? (ev_left > 0 ? ev_left : 0) : 0x7fffffffll),
                                                           0x00020000);
    char *seam = seam_all + (unsigned long long) (ST.seam_first + (unsigned) wv) * ST.seam_stride;
    const rsrc_t rs_seam = __builtin_amdgcn_make_buffer_rsrc(seam, 0, (int) ST.seam_stride, 0x00020000);
    const unsigned C8 = (unsigned) C * 8u;
    const unsigned OOB = 0xfffffff0u;
    const rsrc_t rs_E = make_rsrc(HDP ? (const void *) (E_all + R->f_base) : (const void *) ev_all);
    const rsrc_t rs_en = TWO ? strip_rsrc_en(E_all, R->ev_off, T.two_xn_off) : rs_ev;
    const rsrc_t rs_xn = TWO ? make_rsrc(reinterpret_cast<const double4 *>(E_all) + T.two_xn_off + R->pid_off) : rs_xc;
    const unsigned sentinel8 = C8 - 8u;
    const unsigned seam_vo = lane == 63 ? 0u : OOB;   // lane 63 publishes
    const unsigned sh = ST.seam_cap * 8u;             // bytes between a record's two values
    unsigned sw = 0u, sr = ST.seam_cap * 16u;        // byte base of the seam array this strip writes / reads
    // seam records: index 0 is a -inf sentinel, 1 .. n the diagonals d0 .. d0 + n - 1 of the strip that wrote the array,
    // n + 1 a closing -inf sentinel; a reader clamps its index into [0, n + 1]
    if (lane == 0) {
        seam_store(rs_seam, 0u, sw, sh, NEG_INF, NEG_INF);
        seam_store(rs_seam, 0u, sw + 8u, sh, NEG_INF, NEG_INF);
        seam_store(rs_seam, 0u, sr, sh, NEG_INF, NEG_INF);
        seam_store(rs_seam, 0u, sr + 8u, sh, NEG_INF, NEG_INF);
        F[C - 1] = NEG_INF;   // sentinel of the match plane (read by backward lanes without a cell)
    }
    // the diagonals the region's tracebacks start on keep all three planes (k_spec_match, sa_hip.hip, takes the traceback's total there)
    const sa_seg_t *segs_r = segs_all + R->seg_off;
    const int n_seg = R->n_seg;
    wave_fence();
    int d0_r = 0, n_r = 0;   // first diagonal and count of the array being read (no strip in front of strip 0: all -inf)
    const double st_m = R->ragged_l ? NEG_INF : 0.0, st_g = R->ragged_l ? 0.0 : NEG_INF;   // diagonal 0 (impl/stateMachine.c:1134-1143)

    for (int s = 0; s <= smax; s++) {
        const int dlo = __builtin_amdgcn_readfirstlane(lo[s]), dhi = __builtin_amdgcn_readfirstlane(hi[s]);
        if (dhi < dlo) {   // no cell in these columns (cannot happen for a band; kept for safety): the next strip reads -inf
            if (lane == 0) seam_store(rs_seam, 0u, sw + 8u, sh, NEG_INF, NEG_INF);
            wave_fence();
            d0_r = 0; n_r = 0;
            { const unsigned t_ = sw; sw = sr; sr = t_; }
            continue;
        }
        // two diagonals of lead-in (every lane idle) bring the seam values of dlo-1 and dlo-2 into place; the loop runs in
        // (even, odd) pairs and has a single exit: it starts on an even diagonal and may end one (idle) diagonal above dhi
        const int d0 = s == 0 ? 0 : ((dlo - 2) & ~1);
        const int d_stop = dhi | 1;
        const int nst = d_stop - d0 + 1;
        if (lane == 0) seam_store(rs_seam, 0u, sw + (unsigned) (nst + 1) * 8u, sh, NEG_INF, NEG_INF);
        const int x = 64 * s + lane;
        const unsigned x8 = (unsigned) x * 8u;
        double4 c = {0.0, 0.0, 0.0, 0.0};
        if (!HDP) c = buf_load_f64x4(rs_xc, (x <= lX ? (unsigned) x : 0u) * 32u);
        double4 cn = {0.0, 0.0, 0.0, 0.0};
        if (TWO) cn = buf_load_f64x4(rs_xn, (x <= lX ? (unsigned) x : 0u) * 32u);
        double oY = NEG_INF, sX = NEG_INF, sMe = NEG_INF, sMo = NEG_INF;
        int d = d0;
        int sg_k = 0;   // the first traceback that starts at or above this strip's first diagonal (a scalar search: a dozen segments)
        while (sg_k < n_seg && (int) segs_r[sg_k].start < d0) sg_k++;
        int sg_next = sg_k < n_seg ? (int) segs_r[sg_k].start : 0x7fffffff;
        // row records and packed words of 64 diagonals from the 32-aligned one at or below d; the 32 that move in next.
        // Diagonals outside [dlo, dhi] (the lead-in, the one above dhi) get width 0: every lane idles there.
        auto tile_at = [&](int base) -> int4 {
            const int i = base + lane;
            int4 r = rows4[i];
            r.y = (i >= dlo && i <= dhi) ? r.y : 0;
            return r;
        };
        int4 tile = tile_at(d & ~31), tile_n = tile_at((d & ~31) + 32);
        int pkv = pk[(d & ~31) + lane], pkn = pk[(d & ~31) + 32 + lane];
        if (s == 0 && lane == 0) pkv |= SA_PK_CK;   // diagonal 0 takes the branch that stores every plane
        double pend_m = NEG_INF, pend_a = NEG_INF, pend_b = NEG_INF;
        unsigned pend_vo = OOB, pend_so = 0u, pend_svo = OOB, pend_sso = sw;   // (pend_sso advances by 8 bytes per diagonal)
        // running values of the diagonal being requested (requests are issued for consecutive diagonals upwards)
        unsigned evo_r = (unsigned) ((d - 1) * 8);   // byte offset of the event of column 0 (y < 1: beyond the range, reads 0)
        int si_r = d - d0_r + 1;                     // its record in the seam array being read
        const int n1_r = n_r + 1;

        auto request = [&](StripIn &in, StripTwo &tw, int li_r) {   // li_r: entry of the requested diagonal in the row tile (HDP only)
            if (TWO) strip_request_two(tw, rs_en, (evo_r - x8) * 4u);
            if (HDP) {
                const int xL_r = __builtin_amdgcn_readlane(tile.w, li_r), w_r = __builtin_amdgcn_readlane(tile.y, li_r);
                const unsigned fo8_r = (unsigned) __builtin_amdgcn_readlane(tile.z, li_r) * 8u;
                const int t_r = x - xL_r;
                in.e = buf_load_f64(rs_E, (unsigned) t_r < (unsigned) w_r ? (unsigned) t_r * 8u + fo8_r : sentinel8, 0);
            } else {
                in.e = buf_load_f64(rs_ev, evo_r - x8, 0);
            }
            int si = si_r < 0 ? 0 : si_r;
            si = si > n1_r ? n1_r : si;
            const unsigned so = sr + (unsigned) si * 8u;
            in.sa = buf_load_f64_l2(rs_seam, 0u, so);
            in.sb = buf_load_f64_l2(rs_seam, 0u, so + sh);
            evo_r += 8u;
            si_r++;
        };
        // one diagonal.  `cur` was requested two diagonals earlier and is refilled at the end of the step; sMp holds oM of
        // (x-1, y-1) (written two diagonals ago) and is overwritten with this diagonal's shifted oM.
        auto half = [&](StripIn &cur, StripTwo &curn, double &sMp) {
            const int li = d & 31;
            // the previous diagonal's stores, behind that diagonal's request (vmcnt retires in order: sa_fast.inc)
            buf_store_f64(rs_F, pend_vo, pend_so, pend_m);
            seam_store(rs_seam, pend_svo, pend_sso, sh, pend_a, pend_b);
            const int xL = __builtin_amdgcn_readlane(tile.w, li), w = __builtin_amdgcn_readlane(tile.y, li);
            const unsigned fo8 = (unsigned) __builtin_amdgcn_readlane(tile.z, li) * 8u;
            const int pw = __builtin_amdgcn_readlane(pkv, li);
            const int t = x - xL;
            const bool act = (unsigned) t < (unsigned) w;
            // a cell outside the band has emission -inf: +inf enters the squared deviation through the addend
            double lM, lY_;
            if (HDP) {   // the plane holds -inf outside the band (and for cells without a k-mer / event pair)
                lM = cur.e; lY_ = cur.e;
            } else {
                const double pmask = __hiloint2double(act ? 0 : 0x7ff00000, 0);
                const double a = (cur.e - c.x) * c.y;
                emit_gauss_q(c, fma(a, a, pmask), lM, lY_);
            }
            if (TWO) {
                const double l2 = strip_two_l2(cn, curn, act);
                lM += l2; lY_ += l2;
            }
            double m = sMp + lM;
            double xg = act ? sX : NEG_INF;
            double yg = oY + lY_;
            const unsigned vo = act ? (unsigned) t * 8u : OOB;
            const bool seg_start = d == sg_next;
            if (seg_start) {
                sg_k++;
                sg_next = sg_k < n_seg ? (int) segs_r[sg_k].start : 0x7fffffff;
            }
            if ((pw & SA_PK_CK) || seg_start) {   // gap planes: checkpoint diagonals, the diagonals tracebacks start on -- and diagonal 0
                                                   // (its word carries the flag here)
                if (d == 0) {        // the start state of cell (0, 0)
                    m = act ? st_m : NEG_INF;
                    xg = act ? st_g : NEG_INF;
                    yg = xg;
                }
                buf_store_f64(rs_F, vo, fo8 + C8, xg);
                buf_store_f64(rs_F, vo, fo8 + 2u * C8, yg);
            }
            // the four logAdds of a cell through the per-site tables (sa_fast.inc: three operand additions instead of seven)
            LaP pm, px, py, pq;
            la_prep(pm, m, xg + SK.a0);
            la_prep(px, m, xg + SK.a1);
            la_prep(py, m, yg + SK.a2);
            la_fetch(pm, LS);
            la_fetch(px, LS + LA_TAB_DOUBLES);
            la_fetch(py, LS + 2 * LA_TAB_DOUBLES);
            __builtin_amdgcn_sched_barrier(0);
            la_wait();
            const double om1 = la_finish(pm);
            const double oX = la_finish(px);
            oY = la_finish(py);
            la_prep(pq, om1, yg);
            la_fetch(pq, LS + 3 * LA_TAB_DOUBLES);
            la_wait();
            const double oM = la_finish(pq);
            sX = strip_from_below(oX, cur.sb);
            sMp = strip_from_below(oM, cur.sa);
            pend_m = m; pend_vo = vo; pend_so = fo8;
            pend_a = oM; pend_b = oX; pend_svo = seam_vo; pend_sso += 8u;
            __builtin_amdgcn_sched_barrier(0);
            request(cur, curn, li + 2);   // the stage is free again: it takes the inputs of the diagonal two steps on
            d++;
        };
        auto next_tile = [&]() {   // d is a multiple of 32
            tile = tile_n; pkv = pkn;
            tile_n = tile_at(d + 32);
            pkn = pk[d + 32 + lane];
        };
        StripIn S0, S1;
        StripTwo N0, N1;
        request(S0, N0, d & 31);
        request(S1, N1, (d & 31) + 1);
        for (;;) {
            do {
                half(S0, N0, sMe);
                half(S1, N1, sMo);
            } while (d <= d_stop && (d & 31) != 0);
            if (d > d_stop) break;
            next_tile();
        }
        buf_store_f64(rs_F, pend_vo, pend_so, pend_m);
        seam_store(rs_seam, pend_svo, pend_sso, sh, pend_a, pend_b);
        wave_fence();   // the seam is complete in L2 before the next strip asks for it
        d0_r = d0; n_r = nst;
        { const unsigned t_ = sw; sw = sr; sr = t_; }
    }
}

// ---------------------------------------------------------------------------------------------------
// backward: one sweep per segment, candidates and checkpoint terms written as the sweep meets them
// ---------------------------------------------------------------------------------------------------
struct StripInB {
    double e;
    double fm;       // forward.match of the lane's cell (-inf: no cell)
    double sa, sb;   // seam record {mM, mX} of the diagonal from strip s + 1 (two 8-byte loads: a 16-byte register tuple
                     // does not survive the loop's back edge without a copy, and the copy waits for the load)
};

#define STRIP_BWD_OCC 4
// The candidate bound is known before the sweep starts (the traceback's speculative total, above), so
//   * a posterior cell is tested and, when it passes, appended to the segment's candidates right away;
//   * a checkpoint's per-cell terms logAdd(logAdd(f.m + b.m, f.x + b.x), f.y + b.y) and the match-through terms of the diagonal
//     above it go straight to vbuf, in cell order, where k_fold reads them (the forward gap states of a checkpoint diagonal are
//     loaded inside that diagonal's branch: one diagonal in ten);
//   * candidates arrive strip by strip (high columns first), not in output order: k_finalize tests them against the exact
//     totals as for every other kernel and k_gather_sorted writes a segment's survivors in (diagonal, column) order (sa_hip.hip).
// TWO: as in k_fwd_strip.  Its four stages hold twelve doubles more: at four waves per SIMD (128 registers) 43 of them spilled into
// the loop, so this instance is built for three.
template <bool HDP, bool TWO = false>
__global__ __launch_bounds__(64 * STRIP_WAVES)
__attribute__((amdgpu_waves_per_eu(TWO ? STRIP_BWD_OCC - 1 : STRIP_BWD_OCC, TWO ? STRIP_BWD_OCC - 1 : STRIP_BWD_OCC))) void k_bwd_strip1(
    const sa_region_t *__restrict__ regions, const sa_seg_t *__restrict__ segs, const sa_row_t *__restrict__ rows_all,
    const sa_ck_t *__restrict__ cks, const double4 *__restrict__ xc_all, const double *__restrict__ ev_all, double *__restrict__ F_all,
    double *__restrict__ vbuf, sa_cand_t *__restrict__ cands, int *__restrict__ cand_count, int *__restrict__ overflow,
    char *__restrict__ seam_all, StripT ST, const int *__restrict__ seg_ids, int n, const double *__restrict__ E_all) {
    __shared__ __attribute__((aligned(32))) double LT[LA_TAB_DOUBLES];
    __shared__ int s_lo[STRIP_WAVES][STRIP_NS_MAX], s_hi[STRIP_WAVES][STRIP_NS_MAX];
    const FastT &T = ST.f;
    la_tab_init(LT, threadIdx.x);
    __syncthreads();
    const int wv = __builtin_amdgcn_readfirstlane((int) ((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wv >= n) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int seg = __builtin_amdgcn_readfirstlane(seg_ids[wv]);
    const sa_seg_t *S = &segs[seg];
    const sa_region_t *R = &regions[S->region];
    const int4 *rows4 = reinterpret_cast<const int4 *>(rows_all + R->row_off);
    const int lX = (int) R->lX;
    const long long C = R->f_cellpaths;
    double *F = F_all + 3 * R->f_base;
    const int start = (int) S->start, from = (int) S->from, to = (int) S->to;
    const long long ck_base = S->ck_base;
    const int n_ck = S->n_ck;
    const int4 *cks4 = reinterpret_cast<const int4 *>(cks + ck_base);   // {voff lo, voff hi, nA, nB}
    const int ns = (lX >> 6) + 1;
    int *lo = s_lo[wid], *hi = s_hi[wid];
    int smin, smax;
    strip_ranges(rows4, to + 1, start, lane, ns, lo, hi, smin, smax);

    const rsrc_t rs_xc = make_rsrc(xc_all + R->pid_off), rs_F = make_rsrc(F);
    const long long ev_left = (ST.ev_total - R->ev_off) * 8;
    const rsrc_t rs_ev = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(ev_all + R->ev_off), 0,
                                                           (int) (ev_left < 0x7fffffffll ? (ev_left > 0 ? ev_left : 0) : 0x7fffffffll),
                                                           0x00020000);
    char *seam = seam_all + (unsigned long long) (ST.seam_first + (unsigned) wv) * ST.seam_stride;
    const rsrc_t rs_seam = __builtin_amdgcn_make_buffer_rsrc(seam, 0, (int) ST.seam_stride, 0x00020000);
    const unsigned C8 = (unsigned) C * 8u;
    const unsigned OOB = 0xfffffff0u;
    const unsigned sentinel8 = C8 - 8u;
    const rsrc_t rs_E = make_rsrc(HDP ? (const void *) (E_all + R->f_base) : (const void *) ev_all);
    const rsrc_t rs_en = TWO ? strip_rsrc_en(E_all, R->ev_off, T.two_xn_off) : rs_ev;
    const rsrc_t rs_xn = TWO ? make_rsrc(reinterpret_cast<const double4 *>(E_all) + T.two_xn_off + R->pid_off) : rs_xc;
    const unsigned seam_vo = lane == 0 ? 0u : OOB;
    const unsigned sh = ST.seam_cap * 8u;
    unsigned sw = 0u, sr = ST.seam_cap * 16u;
    if (lane == 0) {
        seam_store(rs_seam, 0u, sw, sh, NEG_INF, NEG_INF);
        seam_store(rs_seam, 0u, sw + 8u, sh, NEG_INF, NEG_INF);
        seam_store(rs_seam, 0u, sr, sh, NEG_INF, NEG_INF);
        seam_store(rs_seam, 0u, sr + 8u, sh, NEG_INF, NEG_INF);
    }
    wave_fence();
    double end_m, end_x, end_y;
    if (S->at_end && R->ragged_r) {
        end_m = (T.t_mx + T.t_my) / 2.0; end_x = T.t_xx; end_y = T.t_yy;
    } else {
        end_m = T.t_mm; end_x = T.t_xm; end_y = T.t_ym;
    }
    // the candidate bound: no checkpoint's exact total may lie below spec - slack (k_finalize checks that it does not)
    const double spec = ST.spec[seg];
    const double lim = (spec > NEG_INF) ? spec - ST.slack + T.thr_off : __builtin_inf();
    sa_cand_t *my_cands = cands + S->cand_off;
    const int cand_cap = S->cand_cap;
    int count = 0;
    int e0_r = 0, n_r = 0;

    for (int s = smax; s >= smin; s--) {
        const int dlo = __builtin_amdgcn_readfirstlane(lo[s]), dhi = __builtin_amdgcn_readfirstlane(hi[s]);
        if (dhi < dlo) {
            if (lane == 0) seam_store(rs_seam, 0u, sw + 8u, sh, NEG_INF, NEG_INF);
            wave_fence();
            e0_r = 0; n_r = 0;
            { const unsigned t_ = sw; sw = sr; sr = t_; }
            continue;
        }
        const int e0 = (dhi + 2) | 3;
        const int e_stop = (dlo & ~3) - 1;
        const int nst = e0 - e_stop;
        if (lane == 0) seam_store(rs_seam, 0u, sw + (unsigned) (nst + 1) * 8u, sh, NEG_INF, NEG_INF);
        const int x = 64 * s + lane;
        const unsigned x8 = (unsigned) x * 8u;
        double4 c = {0.0, 0.0, 0.0, 0.0};
        if (!HDP) c = buf_load_f64x4(rs_xc, (x <= lX ? (unsigned) x : 0u) * 32u);
        double4 cn = {0.0, 0.0, 0.0, 0.0};
        if (TWO) cn = buf_load_f64x4(rs_xn, (x <= lX ? (unsigned) x : 0u) * 32u);
        double mY1 = NEG_INF, sX = NEG_INF, sMe = NEG_INF, sMo = NEG_INF;
        int e = e0;
        auto tile_at = [&](int base) -> int4 {
            const int i = base + lane;
            int4 r = rows4[i < 0 ? 0 : i];
            r.y = (i >= dlo && i <= dhi) ? r.y : 0;
            return r;
        };
        // per diagonal (one per lane, 64 at a time): bit 0 a posterior diagonal, bit 1 a checkpoint, bit 2 the diagonal above a
        // checkpoint (its cells are that checkpoint's match-through terms; never a checkpoint itself), bits 8..: the checkpoint
        auto flags_at = [&](int base) -> int {
            const int i = base + lane;
            const int qi = from - i;
            const bool post = qi >= 0 && i > to;
            const int qq = qi >= 0 ? qi : 0;
            const int ck_i = qq / SA_CKPT_EVERY, ph_i = qq - ck_i * SA_CKPT_EVERY;
            const bool isck = post && ph_i == 0;
            const int qa = qi + 1;                                  // from - (i - 1)
            const bool abv = qa >= 0 && i - 1 > to && qa % SA_CKPT_EVERY == 0;
            const int ck_a = (qa >= 0 ? qa : 0) / SA_CKPT_EVERY;
            return (post ? 1 : 0) | (isck ? 2 : 0) | (abv ? 4 : 0) | ((isck ? ck_i : (abv ? ck_a : 0)) << 8);
        };
        int4 tile = tile_at((e & ~31) - 32), tile_n = tile_at((e & ~31) - 64);
        int ft = flags_at((e & ~31) - 32), ft_n = flags_at((e & ~31) - 64);
        int ckt_base = from - e >= 0 ? (from - e) / SA_CKPT_EVERY : 0;
        auto ck_tile_at = [&](int base) -> int4 { const int i = base + lane; return cks4[i < n_ck ? i : (n_ck > 0 ? n_ck - 1 : 0)]; };
        int4 ckt = ck_tile_at(ckt_base);
        double pend_a = NEG_INF, pend_b = NEG_INF;
        unsigned pend_svo = OOB, pend_sso = sw;
        unsigned evo_r = (unsigned) ((e - 1) * 8);
        int si_r = e0_r - e + 1;
        const int n1_r = n_r + 1;

        auto request = [&](StripInB &in, StripTwo &tw, int li) {
            if (!HDP) in.e = buf_load_f64(rs_ev, evo_r - x8, 0);
            if (TWO) strip_request_two(tw, rs_en, (evo_r - x8) * 4u);
            int si = si_r < 0 ? 0 : si_r;
            si = si > n1_r ? n1_r : si;
            const unsigned so = sr + (unsigned) si * 8u;
            in.sa = buf_load_f64_l2(rs_seam, 0u, so);
            in.sb = buf_load_f64_l2(rs_seam, 0u, so + sh);
            const int xL = __builtin_amdgcn_readlane(tile.w, li), w = __builtin_amdgcn_readlane(tile.y, li);
            const unsigned fo8 = (unsigned) __builtin_amdgcn_readlane(tile.z, li) * 8u;
            const int t = x - xL;
            const bool act = (unsigned) t < (unsigned) w;
            in.fm = buf_load_f64_stream(rs_F, act ? (unsigned) t * 8u + fo8 : sentinel8, 0);
            if (HDP) in.e = buf_load_f64(rs_E, act ? (unsigned) t * 8u + fo8 : sentinel8, 0);
            evo_r -= 8u;
            si_r++;
        };
        auto half = [&](auto head, StripInB &cur, StripTwo &curn, double &sMp) {
            const int li = (e & 31) + 32;
            seam_store(rs_seam, pend_svo, pend_sso, sh, pend_a, pend_b);
            const int xL = __builtin_amdgcn_readlane(tile.w, li), w = __builtin_amdgcn_readlane(tile.y, li);
            const unsigned fo8 = (unsigned) __builtin_amdgcn_readlane(tile.z, li) * 8u;
            const int fl = __builtin_amdgcn_readlane(ft, li);
            const int t = x - xL;
            const bool act = (unsigned) t < (unsigned) w;
            const unsigned vo = act ? (unsigned) t * 8u : OOB;
            double lM, lY_;
            if (HDP) {
                lM = cur.e; lY_ = cur.e;
            } else {
                const double pmask = __hiloint2double(act ? 0 : 0x7ff00000, 0);
                const double a = (cur.e - c.x) * c.y;
                emit_gauss_q(c, fma(a, a, pmask), lM, lY_);
            }
            if (TWO) {
                const double l2 = strip_two_l2(cn, curn, act);
                lM += l2; lY_ += l2;
            }
            LaP pm, px, py;
            la_prep(pm, sMp + T.t_mm, mY1 + T.t_my);
            la_prep(px, sMp + T.t_xm, sX + T.t_xx);
            la_prep(py, sMp + T.t_ym, mY1 + T.t_yy);
            la_fetch(pm, LT);
            la_fetch(px, LT);
            la_fetch(py, LT);
            __builtin_amdgcn_sched_barrier(0);
            const double tm1 = la_finish(pm);
            double tx = la_finish(px);
            double ty = la_finish(py);
            double tm = la_fast(LT, tm1, sX + T.t_mx);
            if (decltype(head)::value) {
                const bool is_start = e == start;
                tm = vmax(tm, is_start ? end_m : NEG_INF);
                tx = vmax(tx, is_start ? end_x : NEG_INF);
                ty = vmax(ty, is_start ? end_y : NEG_INF);
            }
            const double mM = tm + lM;
            mY1 = ty + lY_;
            const double mX = act ? tx + SA_LOG_GAPX : NEG_INF;
            sX = strip_from_above(mX, cur.sb);
            sMp = strip_from_above(mM, cur.sa);
            pend_a = mM; pend_b = mX; pend_svo = seam_vo; pend_sso += 8u;
            // posterior side (all conditions wave-uniform)
            const double fb = cur.fm + tm;   // -inf for lanes without a cell and for border cells (their forward value is -inf)
            if (fl & 7) {
                if (fl & 1) {   // a posterior diagonal: candidates, in cell order within this strip
                    const bool pass = fb >= lim;
                    const unsigned long long mask = __ballot(pass);
                    if (mask) {
                        const int rank = __popcll(mask & ((1ull << lane) - 1ull));
                        if (pass) {
                            const int pos = count + rank;
                            if (pos < cand_cap) {
                                sa_cand_t cd;
                                cd.x = x - 1; cd.y = e - x - 1; cd.path = 0; cd.pad = 0; cd.fb = fb;
                                my_cands[pos] = cd;
                            } else {
                                overflow[0] = 1;
                            }
                        }
                        count += __popcll(mask);
                    }
                }
                if (fl & 6) {
                    const int cl = (fl >> 8) - ckt_base;
                    const long long voff = ((long long) __builtin_amdgcn_readlane(ckt.y, cl) << 32) |
                                           (unsigned) __builtin_amdgcn_readlane(ckt.x, cl);
                    if (fl & 2) {   // the checkpoint's per-cell terms, as every other kernel writes them.  The forward gap states of
                                    // the lane's cell are loaded here, one diagonal in ten (asked for ahead of the arithmetic they
                                    // cost four registers in every step and the kernel its fourth wave per SIMD)
                        const double fx = buf_load_f64(rs_F, act ? vo + fo8 + C8 : sentinel8, 0);
                        const double fy = buf_load_f64(rs_F, act ? vo + fo8 + 2u * C8 : sentinel8, 0);
                        double v = la_fast(LT, la_fast(LT, fb, fx + tx), fy + ty);
                        v = act ? v : NEG_INF;
                        buf_store_f64(make_rsrc(vbuf + voff), vo, 0u, v);
                    } else {        // the diagonal above a checkpoint: its match-through terms
                        const int nA = __builtin_amdgcn_readlane(ckt.z, cl), nB = __builtin_amdgcn_readlane(ckt.w, cl);
                        if (nB > 0) buf_store_f64(make_rsrc(vbuf + voff + nA), vo, 0u, fb);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            request(cur, curn, li - 4);
            e--;
        };
        auto next_tile = [&]() {
            tile = tile_n; ft = ft_n;
            tile_n = tile_at((e & ~31) - 64);
            ft_n = flags_at((e & ~31) - 64);
            const int cki = from - e >= 0 ? (from - e) / SA_CKPT_EVERY : 0;
            if (cki + 8 - ckt_base >= 64) {
                ckt_base = cki;
                ckt = ck_tile_at(ckt_base);
            }
        };
        StripInB S0, S1, S2, S3;
        StripTwo N0, N1, N2, N3;
        request(S0, N0, (e & 31) + 32);
        request(S1, N1, (e & 31) + 31);
        request(S2, N2, (e & 31) + 30);
        request(S3, N3, (e & 31) + 29);
        const std::integral_constant<bool, false> BODY;
        const std::integral_constant<bool, true> HEAD;
        half(HEAD, S0, N0, sMo);
        half(HEAD, S1, N1, sMe);
        half(HEAD, S2, N2, sMo);
        half(HEAD, S3, N3, sMe);
        if ((e & 31) == 31) next_tile();
        half(HEAD, S0, N0, sMo);
        half(HEAD, S1, N1, sMe);
        half(HEAD, S2, N2, sMo);
        half(HEAD, S3, N3, sMe);
        while (e > e_stop) {
            if ((e & 31) == 31) next_tile();
            do {
                half(BODY, S0, N0, sMo);
                half(BODY, S1, N1, sMe);
                half(BODY, S2, N2, sMo);
                half(BODY, S3, N3, sMe);
            } while (e > e_stop && (e & 31) != 31);
        }
        seam_store(rs_seam, pend_svo, pend_sso, sh, pend_a, pend_b);
        wave_fence();
        e0_r = e0; n_r = nst;
        { const unsigned t_ = sw; sw = sr; sr = t_; }
    }
    if (lane == 0) cand_count[seg] = count < cand_cap ? count : cand_cap;
}

// seam: the launch's seam storage, seam_cap records per seam array and its first wave slot seam_first; ev_total: doubles in the
// batch's event array
static StripT make_strip_t(const DevPlan &P, long long ev_total, unsigned seam_cap, unsigned seam_first) {
    StripT ST;
    ST.f = make_fast_t(P);
    ST.ev_total = ev_total; ST.seam_cap = seam_cap; ST.seam_stride = 32ull * seam_cap; ST.seam_first = seam_first;
    ST.spec = P.spec;
    ST.slack = P.spec_slack;
    return ST;
}
// one wave per region (forward) / segment (backward), STRIP_WAVES to a workgroup
static void launch_fwd_strip(const DevPlan &P, const int *ids, int n, hipStream_t st, char *seam, const StripT &ST) {
    auto k = P.m.hdp ? k_fwd_strip<true> : (P.two ? k_fwd_strip<false, true> : k_fwd_strip<false>);
    hipLaunchKernelGGL(k, dim3((n + STRIP_WAVES - 1) / STRIP_WAVES), dim3(64 * STRIP_WAVES), 0, st, P.regions, P.rows, P.pk,
                       reinterpret_cast<const double4 *>(P.xc), P.ev, P.F, seam, ST, ids, n, P.m.hdp ? (const double *) P.E : P.two,
                       P.segs);
}
static void launch_bwd_strip(const DevPlan &P, const int *ids, int n, hipStream_t st, char *seam, const StripT &ST) {
    auto k = P.m.hdp ? k_bwd_strip1<true> : (P.two ? k_bwd_strip1<false, true> : k_bwd_strip1<false>);
    hipLaunchKernelGGL(k, dim3((n + STRIP_WAVES - 1) / STRIP_WAVES), dim3(64 * STRIP_WAVES), 0, st, P.regions, P.segs, P.rows, P.cks,
                       reinterpret_cast<const double4 *>(P.xc), P.ev, P.F, P.vbuf, P.cands, P.cand_count, P.overflow, seam, ST, ids, n,
                       P.m.hdp ? (const double *) P.E : P.two);
}
