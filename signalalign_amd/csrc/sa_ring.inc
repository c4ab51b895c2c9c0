// sa_ring.inc -- LDS-ring kernels: one lane per cell-path, any band width, any number of paths per cell.
// Included by sa_hip.hip after sa_fast.inc (logAdd, buffer access and emission helpers are shared).
//
// The register kernels (sa_fast.inc) hold one path per cell and three diagonals of at most 64 lanes.  Two workloads
// fall outside: reference windows with ambiguous letters (several paths per cell: BASELINE configs[2], hdCell_construct2
// impl/pairwiseAligner.c:723-801) and anchors as sparse as a real guide alignment leaves them (bands of 100-300 cells,
// impl/pairwiseAligner.c:234-241).  Here a diagonal is a row of CELL-PATHS in path space: cell x owns the indices
// poff[x] .. poff[x+1]-1, a diagonal the contiguous range [g0, g0 + rowpaths), one lane per index, 64 lanes per chunk.
// What a finished cell-path publishes is what the register kernels publish (sa_fast.inc header): three messages with the
// transitions folded in, so a receiver adds its own emission to sums over the sender's states.  The messages of the three
// live diagonals sit in an LDS ring (3 rows x 3 messages x cap doubles), indexed by the row-local path index; a
// neighbour is found by subtracting its row's g0, and a neighbour outside its row's range reads as -inf (one unsigned
// compare), so a diagonal costs the same whatever the band does around it.  All per-diagonal geometry is one 16-byte
// scalar record (rows[d]: x-y of the first cell, width, offset in the forward planes, g0; the next record's offset closes
// the row); with several paths per cell a 16-byte per-path record (sa_prec_t, written by the planner) names the legal
// predecessors (strided) and successors (contiguous) in the neighbouring columns -- no k-mer arithmetic, no division and
// no dependent metadata loads in the sweep.
//
// One workgroup of 1, 2 or 4 waves per region (forward) or traceback segment (backward): a wide diagonal is spread over
// the waves, the ring is shared (LDS per wave stays small enough for 4 waves per SIMD), one barrier per diagonal.  A
// diagonal's inputs (position constants, event, per-path record, forward value) are requested one diagonal AHEAD, before
// the current one is computed: the serial chain of a sweep then holds LDS accesses and arithmetic only.  Backward: the
// candidates of a diagonal are laid out in cell order across the waves through per-chunk counts in LDS; their prefix is
// taken one diagonal later, behind the barrier that diagonal needs anyway.
//
// The sweeps have no exec-masked branch around a memory access: a neighbour outside its row reads a fixed LDS cell that
// holds -inf (address select), a lane without a cell-path writes its messages to a scrap cell and its forward values beyond
// the buffer's range (dropped by the range check), the gap planes of diagonals that are not checkpoints likewise.  The
// loop is unrolled over two diagonals so that the two input stages swap roles without copies.  Both matter for the same
// reason as in sa_fast.inc: vmcnt retires in order and the compiler waits with vmcnt(0) behind a divergent join or a copy
// of a loaded register -- i.e. for this diagonal's stores to reach HBM -- instead of just for the loads it needs.
//
// Forward storage: planes [match | gapX | gapY] like the register kernels; the gap planes are written on total-probability
// checkpoints only (SA_PK_CK), which is all the backward sweep reads of them.
//
// Arithmetic: the RELAX flavour of sa_hip.hip (la_fast, folded Gaussian constants).  The reference's logAdd
// (impl/pairwiseAligner.c:301-318) is a piecewise-cubic approximation: exactly shift-invariant, logAdd(a + k, b + k) =
// logAdd(a, b) + k -- which is what lets emissions and transitions travel inside messages -- but not associative at the 1e-4
// level, so every fold over several neighbour paths keeps the reference's order term by term.  Posteriors agree with the
// oracle to ~1e-7 (bar 1e-5, asserted in the tests).

struct RingT {
    FastT f;
    int cap;        // cell-paths per ring row
    double *spec;   // per traceback segment: the speculative total its candidate bound comes from (k_spec_match, sa_hip.hip: the
                    // total on the traceback's first diagonal, taken between the forward and the backward sweep)
    double slack;   // candidates are the cell-paths with forward + backward >= spec - slack + log(threshold)
    int all_planes; // forward: keep all three planes of every diagonal (the expectation pass reads them)
    double *wscr;   // backward, WIDE: the segments' global scratch (sa_seg_t.bscratch_off) -- the checkpoint sums that do not fit in LDS
};

#define RING_XTRA 2   // doubles behind the logAdd table: [0] holds -inf (neighbour outside its row), [1] is scrap

// inputs of one cell-path, requested one diagonal ahead
struct RingIn {
    double4 c;     // position constants (m, inv_s, cM, cY) of the path's k-mer
    double e;      // event mean of the cell's row
    double fm;     // backward only: forward match value of the cell-path
    double fx, fy; // backward, several paths per cell: forward gapX / gapY values when the diagonal is a checkpoint
    int x, a0;     // column; first legal predecessor (forward) / successor (backward) in path space
    int na, stride;
    int po;        // backward, several paths per cell: poff[x] (the path index of a candidate is g - poff[x])
    int p0, npd;   // backward expectation pass: first legal predecessor in column x - 1 and their number (stride as above)
};

// two-distribution emission (the TWO instances): the noise constants of the cell-path's k-mer and of the cell's event
// (FastT.two_xn_off), requested with the other inputs.  Kept beside RingIn: the other instances never name them.
struct RingTwo {
    double4 cn, n3;
};
// The inverse-Gaussian term of the event's noise (emit_two, sa_fast.inc: the same operations in the same order); the strip
// kernels add the same term, bit for bit.
__device__ __forceinline__ double two_l2(const double4 &cn, const double4 &n3) {
    const double a = fma(n3.x, cn.y, -1.0);
    return cn.x - n3.z - cn.z * (a * a) * n3.y;
}

// The per-path record of a cell-path is requested TWO diagonals ahead and its other inputs one diagonal ahead: the event's
// address depends on the record's column, and a dependent pair of loads inside one diagonal is a memory latency in the
// serial chain.  The record is asked for by row position alone (entry g0 + j of the row, whether or not the row is that
// long): the descriptor carries the region's exact size, so what lies beyond reads as zeros, and a lane beyond its row
// does not use what it got.
template <bool MULTI>
__device__ __forceinline__ u32x4 ring_rec(rsrc_t rs_pr, int g) {
    u32x4 rec = {0u, 0u, 0u, 0u};
    if (MULTI) rec = __builtin_amdgcn_raw_buffer_load_b128(rs_pr, (unsigned) g * 16u, 0, 0);
    return rec;
}
typedef const __attribute__((address_space(1))) char *ring_xc_t;   // byte pointers into global memory
typedef const __attribute__((address_space(1))) char *ring_ev_t;
typedef const __attribute__((address_space(1))) u32x4 *ring_gq_t;
typedef const __attribute__((address_space(1))) double *ring_gd_t;
// HDP: the emission itself arrives instead of constants and event -- one 8-byte load from the region's emission plane
// (k_emit_hdp_ring, sa_fast.inc: value j of the diagonal at its offset + j; pe8 = byte offset of the lane's value, or of the
// plane's -inf sentinel for a lane without a cell-path)
// TWO: xn / en = the region's position and event halves of the noise constants, en_pad = the last entry of the events' padding (1.0
// throughout).  A lane without a k-mer/event pair reads that entry and the region's NULL position (zeros): both finite.
template <bool MULTI, bool BWD, bool HDP = false, bool TWO = false>
__device__ __forceinline__ void ring_request(RingIn &in, const u32x4 rec, bool act, int g, int d, ring_xc_t rs_xc, ring_ev_t rs_ev,
                                             rsrc_t rs_E, unsigned pe8, RingTwo *tw = nullptr, ring_xc_t rs_xn = nullptr,
                                             ring_ev_t rs_en = nullptr, ring_ev_t en_pad = nullptr) {
    in.x = g; in.a0 = BWD ? g + 1 : g - 1; in.na = 1; in.stride = 0; in.po = 0; in.p0 = g - 1; in.npd = 1;
    if (MULTI) {
        // all four words stay live up to here: the register of a word this direction does not use would otherwise be handed
        // out while the load is in flight, and its next writer would wait for the load
        asm volatile("" ::"v"(rec.x), "v"(rec.y), "v"(rec.z), "v"(rec.w));
        in.x = (int) rec.x;
        in.a0 = BWD ? (int) rec.z : (int) rec.y;
        in.na = BWD ? (int) (rec.w & 255u) : (int) ((rec.w >> 8) & 255u);
        in.stride = (int) (rec.w >> 16);
        in.p0 = (int) rec.y;
        in.npd = (int) ((rec.w >> 8) & 255u);
    }
    const int y = d - in.x;
    // (plain global loads, scalar base + 32-bit lane offset: every index is clamped into the arrays, so the range check of a
    // buffer descriptor buys nothing here and its four scalars -- two of them re-materialised per access -- cost issue slots)
    if (HDP) {
        in.e = buf_load_f64(rs_E, pe8, 0);
    } else {
        const ring_gq_t p = (ring_gq_t) (rs_xc + (unsigned) g * 32u);
        const u32x4 a = p[0], b = p[1];
        in.c.x = __hiloint2double((int) a.y, (int) a.x); in.c.y = __hiloint2double((int) a.w, (int) a.z);
        in.c.z = __hiloint2double((int) b.y, (int) b.x); in.c.w = __hiloint2double((int) b.w, (int) b.z);
        in.e = *(ring_gd_t) (rs_ev + ((act && y >= 1) ? (unsigned) (y - 1) : 0u) * 8u);
    }
    if (TWO) {
        const bool ok = act && y >= 1;
        const ring_gq_t pn = (ring_gq_t) (rs_xn + (ok ? (unsigned) g : 0u) * 32u);
        const ring_gq_t pe = (ring_gq_t) (ok ? rs_en + (unsigned) (y - 1) * 32u : en_pad);
        const u32x4 a = pn[0], b = pn[1], c_ = pe[0], d_ = pe[1];
        tw->cn.x = __hiloint2double((int) a.y, (int) a.x); tw->cn.y = __hiloint2double((int) a.w, (int) a.z);
        tw->cn.z = __hiloint2double((int) b.y, (int) b.x); tw->cn.w = 0.0;
        tw->n3.x = __hiloint2double((int) c_.y, (int) c_.x); tw->n3.y = __hiloint2double((int) c_.w, (int) c_.z);
        tw->n3.z = __hiloint2double((int) d_.y, (int) d_.x); tw->n3.w = 0.0;
    }
}

// LDS byte address of entry idx of a row plane, or of the -inf cell when idx is outside [0, n)
__device__ __forceinline__ unsigned ring_addr(unsigned plane_base, int idx, int n, unsigned ninf_addr) {
    return ((unsigned) idx < (unsigned) n) ? plane_base + (unsigned) idx * 8u : ninf_addr;
}
typedef __attribute__((address_space(3))) double lds_double_t;
__device__ __forceinline__ double lds_ld(unsigned addr) { return *(const lds_double_t *) (size_t) addr; }
__device__ __forceinline__ void lds_st(unsigned addr, double v) { *(lds_double_t *) (size_t) addr = v; }
// LDS byte offset of a pointer into shared memory (the low half of its flat address)
__device__ __forceinline__ unsigned lds_base(const void *p) { return (unsigned) (size_t) p; }

// ---------------------------------------------------------------------------------------------------
// forward.  K: cell-paths per thread and diagonal (cap == K * blockDim.x)
// ---------------------------------------------------------------------------------------------------
// DENSE (several paths per cell only): a region's sweep comes in two instances, launched one after the other over the same
// list -- a workgroup whose region is of the other kind leaves at once.  Regions dense in ambiguity letters (on average more
// than 1.3 paths per column: C/E at every CpG of a random reference gives 1.375, and only one wave in sixteen would have no
// second predecessor to fold) fold the second predecessor unconditionally; sparse ones (variant candidates here and there) test
// per wave and diagonal whether any of its 64 cell-paths has one and skip the five logAdds otherwise (what they would add is -inf,
// which leaves the sums unchanged exactly): every 8th / 40th CpG ambiguous, 2000 reads: forward 10.7 -> 9.0 / 10.2 -> 7.5 ms,
// backward 12.8 -> 12.3 / 9.9 -> 8.9 ms.  One instance with the test inside cost the dense regions 1.5 % (the branch splits the
// diagonal's code), both loops in one kernel twenty registers (88 -> 108: four waves per SIMD instead of five).
// TWO (Gaussian models only): the two-distribution emission -- E_all is then the buffer of noise constants (FastT.two_xn_off),
// indexed in path space like the position constants: every path of a cell has its own k-mer, hence its own noise mean and lambda.
template <bool MULTI, int K, bool HDP, bool DENSE = true, bool TWO = false>
__global__ __launch_bounds__(256) void k_fwd_ring(const sa_region_t *__restrict__ regions, const sa_row_t *__restrict__ rows_all,
                                                  const int *__restrict__ pk_all, const sa_prec_t *__restrict__ prec_all,
                                                  const double4 *__restrict__ xc_all, const double *__restrict__ ev_all,
                                                  double *__restrict__ F_all, RingT RT, const int *__restrict__ region_ids, int n,
                                                  const int *__restrict__ poff_all, const double *__restrict__ E_all,
                                                  const sa_seg_t *__restrict__ segs_all) {
    extern __shared__ __attribute__((aligned(32))) double ring_dyn[];
    __shared__ __attribute__((aligned(32))) double LS[LA_SITES * LA_TAB_DOUBLES];   // one path per cell: per-site tables
    double *LT = ring_dyn;
    double *ring = ring_dyn + LA_TAB_DOUBLES + RING_XTRA;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const LaSiteK SK = la_sites_fwd(RT.f);
    la_tab_init(LT, tid);
    if (!MULTI) {
        la_tab_init_site(LS, tid, SK.k0);
        la_tab_init_site(LS + LA_TAB_DOUBLES, tid, SK.k1);
        la_tab_init_site(LS + 2 * LA_TAB_DOUBLES, tid, SK.k2);
        la_tab_init_site(LS + 3 * LA_TAB_DOUBLES, tid, SK.k3);
    }
    if (tid == 0) { LT[LA_TAB_DOUBLES] = NEG_INF; LT[LA_TAB_DOUBLES + 1] = 0.0; }
    if ((int) blockIdx.x >= n) return;   // (uniform for the workgroup)
    const FastT &T = RT.f;
    const int cap = RT.cap;
    const sa_region_t *R = &regions[__builtin_amdgcn_readfirstlane(region_ids[blockIdx.x])];
    if (MULTI && (10ll * poff_all[R->poff_off + R->lX + 1] > 13ll * (R->lX + 1)) != DENSE) return;   // (uniform: the other instance's region)
    const int4 *rows4 = reinterpret_cast<const int4 *>(rows_all + R->row_off);
    const int *pk = pk_all + R->pk_off + SA_PK_PAD;
    const int N = (int) R->N;
    const long long C = R->f_cellpaths;
    double *F = F_all + 3 * R->f_base;
    const ring_xc_t rs_xc = (ring_xc_t) (xc_all + R->pid_off);
    const ring_ev_t rs_ev = (ring_ev_t) (ev_all + R->ev_off);
    const rsrc_t rs_F = make_rsrc(F);
    const rsrc_t rs_pr = MULTI ? make_rsrc_n(prec_all + R->pid_off, 16u * (unsigned) poff_all[R->poff_off + R->lX + 1])
                               : make_rsrc(rows_all);
    const unsigned C8 = (unsigned) C * 8u;
    const unsigned OOB = 0xfffffff0u;
    const rsrc_t rs_E = make_rsrc(HDP ? (const void *) (E_all + R->f_base) : (const void *) ev_all);   // HDP: the region's emission plane
    const unsigned sentinel8 = C8 - 8u;
    const ring_xc_t rs_xn = TWO ? (ring_xc_t) (reinterpret_cast<const double4 *>(E_all) + T.two_xn_off + R->pid_off) : rs_xc;
    const ring_ev_t rs_en = TWO ? (ring_ev_t) (reinterpret_cast<const double4 *>(E_all) + R->ev_off) : rs_ev;
    const ring_ev_t en_pad = TWO ? (ring_ev_t) (reinterpret_cast<const double4 *>(E_all) + T.two_xn_off - 1) : rs_ev;
    const double cx_m = SA_LOG_GAPX + T.t_mx, cx_x = SA_LOG_GAPX + T.t_xx;
    const unsigned ninf_a = lds_base(LT + LA_TAB_DOUBLES), scrap_a = ninf_a + 8u;
    // (round 4, forward sweep only -- in the backward sweep the same change measured 1-2 % slower) every plane of a ring row ends
    // in a GUARD cell: entry n of a row of n cell-paths holds -inf (thread 0 writes it with the row), and a neighbour is read at
    // min_u32(idx, n) -- an index of -1 lands on the guard as well.  One instruction less per neighbour than the compare-and-select
    // onto a shared -inf cell, and the planes of a neighbour are addressed with one stride whether it exists or not: configs[2]
    // forward 15.4 -> 14.9 ms per 2000 reads.
    const unsigned plane = (unsigned) (cap + 1) * 8u, slot = 3u * plane;
    auto gaddr = [](unsigned plane_base, int idx, int n) -> unsigned {
        const unsigned u = (unsigned) idx, m = (unsigned) n;
        return plane_base + (u < m ? u : m) * 8u;
    };

    // ring rows: a slot holds three planes of cap doubles (messages oM | oX | oY, or the states with several paths)
    unsigned b0 = lds_base(ring), b1 = b0 + 2u * slot, b2 = b0 + slot;   // LDS byte base of the slots of diagonal d, d-1, d-2
    // Row records and packed words reach the sweep through 64-entry register tiles (one coalesced load per 64 diagonals,
    // requested a tile ahead) and v_readlane: a scalar load per diagonal would sit in front of every LDS wait -- lgkmcnt
    // counts both, and scalar loads return out of order, so each wait for a neighbour would also wait for memory
    const int lane_ = tid & 63;
    int4 tile = rows4[lane_], tile_n = rows4[64 + lane_];
    int pkt = pk[lane_], pkt_n = pk[64 + lane_];
    int tile_id = 0;
    auto row_at = [&](int idx) -> int4 {   // idx inside the current tile
        int4 r;
        r.x = __builtin_amdgcn_readlane(tile.x, idx & 63); r.y = __builtin_amdgcn_readlane(tile.y, idx & 63);
        r.z = __builtin_amdgcn_readlane(tile.z, idx & 63); r.w = __builtin_amdgcn_readlane(tile.w, idx & 63);
        return r;
    };
    int4 rd = row_at(0), r1 = row_at(1), r2 = row_at(2);   // rows d, d+1, d+2 (N >= 1: the sentinel row N + 1 exists)
    int g0_1 = 0, np_1 = 0, g0_2 = 0, np_2 = 0;
    __syncthreads();   // the logAdd table
    {   // diagonal 0: startStateProb / raggedStartStateProb (impl/stateMachine.c:1134-1143)
        const int np = r1.z - rd.z;
        const double m = R->ragged_l ? NEG_INF : 0.0, x = R->ragged_l ? 0.0 : NEG_INF, y = x;
        const double oM = la_fast(LT, la_fast(LT, m + T.t_mm, x + T.t_xm), y + T.t_ym);
        const double oX = la_fast(LT, m + cx_m, x + cx_x);
        const double oY = la_fast(LT, m + T.t_my, y + T.t_yy);
        for (int j = tid; j < np; j += nthr) {
            const unsigned a = b0 + (unsigned) j * 8u;
            if (MULTI) { lds_st(a, m); lds_st(a + plane, x); lds_st(a + 2u * plane, y); }   // states (see the sweep below)
            else { lds_st(a, oM); lds_st(a + plane, oX); lds_st(a + 2u * plane, oY); }
            const unsigned vo = (unsigned) (rd.z + j) * 8u;
            buf_store_f64(rs_F, vo, 0, m);
            buf_store_f64(rs_F, vo, C8, x);
            buf_store_f64(rs_F, vo, 2u * C8, y);
        }
        if (tid == 0) {
            F[C - 1] = NEG_INF;
            for (unsigned pl_ = 0; pl_ < 3u; pl_++) {
                lds_st(b0 + pl_ * plane + (unsigned) np * 8u, NEG_INF);   // the guard of diagonal 0's row
                lds_st(b1 + pl_ * plane, NEG_INF);                        // the two rows nothing has been written to yet: empty
                lds_st(b2 + pl_ * plane, NEG_INF);
            }
        }
        g0_1 = rd.w; np_1 = np;
    }
    // The diagonals the region's tracebacks start on (ascending) keep all three planes too: k_spec_match (sa_hip.hip) takes each
    // traceback's total there -- forward state x end state -- as the backward sweep's candidate bound.  A scalar compare per diagonal.
    const sa_seg_t *segs_r = segs_all + R->seg_off;
    const int n_seg = R->n_seg;
    int sg_k = 0, sg_next = n_seg > 0 ? (int) segs_r[0].start : 0x7fffffff;
    RingIn A[K], B[K];
    RingTwo An[TWO ? K : 1], Bn[TWO ? K : 1];   // (the other instances: one unused entry)
    u32x4 rq[K];   // per-path records of diagonal d + 1 (behind the request below: d + 2)
    int pkc;
    {   // inputs of diagonal 1
        const int g0 = r1.w, np = r2.z - r1.z;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int j = tid + k * nthr;
            const bool act = j < np;
            ring_request<MULTI, false, HDP, TWO>(A[k], ring_rec<MULTI>(rs_pr, g0 + j), act, g0 + (act ? j : 0), 1, rs_xc, rs_ev, rs_E,
                                                 act ? (unsigned) (r1.z + j) * 8u : sentinel8, &An[TWO ? k : 0], rs_xn, rs_en, en_pad);
            rq[k] = ring_rec<MULTI>(rs_pr, r2.w + j);
        }
        pkc = __builtin_amdgcn_readlane(pkt, 1);
    }
    int pkn1 = __builtin_amdgcn_readlane(pkt, 2);   // packed word of diagonal d + 1 (carried: read one diagonal earlier)
    __syncthreads();
    int d = 1;
    // one diagonal: `cur` was requested one diagonal earlier, `nxt` receives the request for d + 1 (harmless behind the
    // last diagonal: the sentinel row has no cell-path, every lane asks for entry 0)
    auto half = [&](RingIn (&cur)[K], RingIn (&nxt)[K], RingTwo (&curn)[TWO ? K : 1], RingTwo (&nxtn)[TWO ? K : 1]) {
        { const unsigned t = b2; b2 = b1; b1 = b0; b0 = t; }
        rd = r1; r1 = r2;
        const int idx = d + 2 <= N + 1 ? d + 2 : N + 1;
        r2 = row_at(idx);
        const int pk_d2 = __builtin_amdgcn_readlane(pkt, idx & 63);
        const int g0 = rd.w, np = r1.z - rd.z;
        const unsigned fo8 = (unsigned) rd.z * 8u;
        if (tid == 0) {   // this row's guards (no cell-path writes entry np: lanes without one write the scrap cell)
            const unsigned ga = b0 + (unsigned) np * 8u;
            lds_st(ga, NEG_INF); lds_st(ga + plane, NEG_INF); lds_st(ga + 2u * plane, NEG_INF);
        }
        const bool full = (pkc & SA_PK_CK) != 0 || d == sg_next || RT.all_planes;
        if (d == sg_next) {
            sg_k++;
            sg_next = sg_k < n_seg ? (int) segs_r[sg_k].start : 0x7fffffff;
        }
        {
            const int g0n = r1.w, npn = r2.z - r1.z;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int j = tid + k * nthr;
                const bool act = j < npn;
                ring_request<MULTI, false, HDP, TWO>(nxt[k], rq[k], act, g0n + (act ? j : 0), d + 1, rs_xc, rs_ev, rs_E,
                                                     act ? (unsigned) (r1.z + j) * 8u : sentinel8, &nxtn[TWO ? k : 0], rs_xn, rs_en, en_pad);
                rq[k] = ring_rec<MULTI>(rs_pr, r2.w + j);
            }
            pkc = pkn1;
            pkn1 = pk_d2;
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int j = tid + k * nthr;
            // a wave whose 64 entries all lie beyond the row has nothing to do (scalar branch: no exec mask involved)
            if (__builtin_amdgcn_readfirstlane(j & ~63) >= np) continue;
            const bool act = j < np;
            const RingIn &in = cur[k];
            const int g = g0 + (act ? j : 0);
            double lM, lY_;
            emit_fast<HDP>(in.c, in.e, lM, lY_);
            if (TWO) {
                const double l2 = two_l2(curn[k].cn, curn[k].n3);
                lM += l2; lY_ += l2;
            }
            int i2 = in.a0 - g0_2, i1 = in.a0 - g0_1;
            const int iu = g - g0_1;
            double m, xg, yg;
            const unsigned wa = act ? b0 + (unsigned) j * 8u : scrap_a;
            const unsigned wstep = act ? plane : 0u;
            if (!MULTI) {
                // one path per cell: the rows hold MESSAGES (oM, oX, oY), the receiver adds its emission
                const double am = lds_ld(gaddr(b2, i2, np_2));                  // oM of (x-1, y-1)
                const double ax = lds_ld(gaddr(b1 + plane, i1, np_1));          // oX of (x-1, y)
                const double ay = lds_ld(gaddr(b1 + 2u * plane, iu, np_1));     // oY of (x, y-1)
                m = am + lM;
                xg = ax;
                yg = ay + lY_;
                // (per-site tables: sa_fast.inc -- the strip kernels do the same arithmetic, bit for bit)
                LaP pm, px, py;
                la_prep(pm, m, xg + SK.a0);
                la_prep(px, m, xg + SK.a1);
                la_prep(py, m, yg + SK.a2);
                la_fetch(pm, LS); la_fetch(px, LS + LA_TAB_DOUBLES); la_fetch(py, LS + 2 * LA_TAB_DOUBLES);
                const double om1 = la_finish(pm);
                lds_st(wa + wstep, la_finish(px));
                lds_st(wa + 2u * wstep, la_finish(py));
                lds_st(wa, la_fast(LS + 3 * LA_TAB_DOUBLES, om1, yg));
            } else {
                // several paths per cell: the rows hold the STATES (m, x, y) and the receiver folds the terms of its legal
                // predecessors one by one in the reference's order (stateMachine3_cellCalculate with doTransitionForward,
                // impl/stateMachine.c:1306-1369: per predecessor path match, gapX, gapY).  The reference's logAdd is a
                // piecewise-cubic approximation: it is exactly shift-invariant (the emission can be added after the fold)
                // but NOT associative at the 1e-4 level, so predecessors' sums must not be pre-combined.  A term of -inf
                // leaves a sum unchanged exactly, so the second predecessor is folded without a branch (a lane with one
                // predecessor reads the -inf cell); third and later ones (codes with more than two letters) take a loop.
                double sm, sx;
                {
                    const bool has_ = in.na >= 1;   // (a cell-path of the first column has no predecessor: onto the guards)
                    const unsigned a2 = gaddr(b2, has_ ? i2 : -1, np_2), a1 = gaddr(b1, has_ ? i1 : -1, np_1);
                    const double pm_ = lds_ld(a2), px_ = lds_ld(a2 + plane), py_ = lds_ld(a2 + 2u * plane);
                    const double qm_ = lds_ld(a1), qx_ = lds_ld(a1 + plane);
                    sm = la_fast(LT, la_fast(LT, pm_ + T.t_mm, px_ + T.t_xm), py_ + T.t_ym);
                    sx = la_fast(LT, qm_ + cx_m, qx_ + cx_x);
                }
                // (the sparse instance: see DENSE above the kernel)
                if (DENSE || __builtin_amdgcn_ballot_w64(in.na >= 2) != 0ull) {
                    i2 += in.stride; i1 += in.stride;
                    const bool has_ = in.na >= 2;
                    const unsigned a2 = gaddr(b2, has_ ? i2 : -1, np_2), a1 = gaddr(b1, has_ ? i1 : -1, np_1);
                    const double pm_ = lds_ld(a2), px_ = lds_ld(a2 + plane), py_ = lds_ld(a2 + 2u * plane);
                    const double qm_ = lds_ld(a1), qx_ = lds_ld(a1 + plane);
                    sm = la_fast(LT, la_fast(LT, la_fast(LT, sm, pm_ + T.t_mm), px_ + T.t_xm), py_ + T.t_ym);
                    sx = la_fast(LT, la_fast(LT, sx, qm_ + cx_m), qx_ + cx_x);
                }
                if (__builtin_amdgcn_ballot_w64(in.na > 2) != 0ull) {
                    for (int i = 2; i < in.na; i++) {
                        i2 += in.stride; i1 += in.stride;
                        const unsigned a2 = gaddr(b2, i2, np_2), a1 = gaddr(b1, i1, np_1);
                        const double pm_ = lds_ld(a2), px_ = lds_ld(a2 + plane), py_ = lds_ld(a2 + 2u * plane);
                        const double qm_ = lds_ld(a1), qx_ = lds_ld(a1 + plane);
                        sm = la_fast(LT, la_fast(LT, la_fast(LT, sm, pm_ + T.t_mm), px_ + T.t_xm), py_ + T.t_ym);
                        sx = la_fast(LT, la_fast(LT, sx, qm_ + cx_m), qx_ + cx_x);
                    }
                }
                const unsigned au = gaddr(b1, iu, np_1);
                const double um = lds_ld(au), uy = lds_ld(au + 2u * plane);
                m = sm + lM;
                xg = sx;
                yg = la_fast(LT, um + T.t_my, uy + T.t_yy) + lY_;
                lds_st(wa, m); lds_st(wa + wstep, xg); lds_st(wa + 2u * wstep, yg);
            }
            const unsigned vo = act ? (unsigned) j * 8u : OOB;
            buf_store_f64(rs_F, vo, fo8, m);
            const unsigned vog = (act && full) ? (unsigned) j * 8u : OOB;   // gap planes: checkpoints only
            buf_store_f64(rs_F, vog, fo8 + C8, xg);
            buf_store_f64(rs_F, vog, fo8 + 2u * C8, yg);
        }
        g0_2 = g0_1; np_2 = np_1; g0_1 = g0; np_1 = np;
        d++;
        __syncthreads();
    };
    // the tile that holds row min(d + 2, N + 1) of the coming diagonal; the hand-over sits between diagonals, outside `half`
    auto next_tile = [&]() {
        const int want = (d + 2 <= N + 1 ? d + 2 : N + 1) >> 6;
        if (want != tile_id) {
            tile = tile_n; pkt = pkt_n;
            tile_id = want;
            tile_n = rows4[(want + 1) * 64 + lane_];   // (readable past the region: the next region's rows or the array's padding)
            pkt_n = pk[(want + 1) * 64 + lane_];
        }
    };
    while (d <= N) {
        half(A, B, An, Bn);
        next_tile();
        if (d > N) break;
        half(B, A, Bn, An);
        next_tile();
    }
}

// ---------------------------------------------------------------------------------------------------
// backward + posterior numerators + checkpoint terms (see the header of bwd_fast_body for the messages)
// ---------------------------------------------------------------------------------------------------
#define RING_MAX_WAVES 4
#define RING_MAX_CHUNKS 8
// EXPECT (several paths per cell, Gaussian emissions): the expectation pass of getExpectationsUsingAnchors
// (diagonalCalculation_Expectations impl/pairwiseAligner.c:1423-1443, cell_signal_updateExpectations :914-944) instead of the
// posterior candidates.  For every cell-path of a posterior diagonal e and every legal predecessor path the reference adds
// exp(F[from] + B[to] + (eP + tP) - total), F from the lower / upper neighbour on e-1 and the middle one on e-2.  B[to] + eP is the
// message this sweep publishes for the cell-path (sa_fast.inc, bwd_fast_body); the forward states come from the forward planes
// (the forward sweep of such a batch keeps all three on every diagonal), the legal predecessors from the per-path record.  Sums
// are kept per lane, scaled by the traceback's speculative total (any scale near the totals will do: sa_expect_batch rescales
// with the exact total of each checkpoint group, k_expect_reduce), and flushed per checkpoint group (gsum / gmc).
// TWO: as in k_fwd_ring (never with HDP or EXPECT).
// WIDE (several paths per cell, TWO, K = 8 on four waves: rows of SA_RING_WIDE_MAX_ROWPATHS cell-paths): the ring alone is 144 KB of
// LDS, so the two copies of a checkpoint diagonal's sums (scr) live in the segment's global scratch instead.  They are written in front
// of a diagonal's barrier and read behind it by the same workgroup -- the barrier orders them --, on two diagonals in ten.
template <bool MULTI, int K, bool HDP, bool EXPECT = false, bool DENSE = true, bool TWO = false, bool WIDE = false>
__global__ __launch_bounds__(256) void k_bwd_ring(const sa_region_t *__restrict__ regions, const sa_seg_t *__restrict__ segs,
                                                  const sa_row_t *__restrict__ rows_all, const int *__restrict__ poff_all,
                                                  const sa_ck_t *__restrict__ cks, const sa_prec_t *__restrict__ prec_all,
                                                  const double4 *__restrict__ xc_all, const double *__restrict__ ev_all,
                                                  const double *__restrict__ F_all, double *__restrict__ vbuf,
                                                  sa_cand_t *__restrict__ cands, int *__restrict__ cand_count,
                                                  int *__restrict__ overflow, RingT RT, const int *__restrict__ seg_ids, int n,
                                                  const double *__restrict__ E_all, double *__restrict__ gsum = nullptr,
                                                  double *__restrict__ gmc = nullptr) {
    extern __shared__ __attribute__((aligned(32))) double ring_dyn[];
    __shared__ double s_xsum[4][8];            // EXPECT: the waves' shares of a checkpoint group's seven sums
    __shared__ int s_count;                    // candidates appended so far (all waves)
    __shared__ double s_end[3];                // states of the segment's first diagonal (read there only: kept out of registers)
    const FastT &T = RT.f;
    const int cap = RT.cap;
    double *LT = ring_dyn;
    double *ring = ring_dyn + LA_TAB_DOUBLES + RING_XTRA;   // 3 slots x [mM | mY | mX][cap]
    double *scr = ring + 9 * cap;                            // MULTI: 2 x [tm | tx | ty][cap] of a checkpoint diagonal, by its parity
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
    la_tab_init(LT, tid);
    if (tid == 0) { LT[LA_TAB_DOUBLES] = NEG_INF; LT[LA_TAB_DOUBLES + 1] = 0.0; s_count = 0; }
    if ((int) blockIdx.x >= n) return;   // whole workgroup
    const int seg = __builtin_amdgcn_readfirstlane(seg_ids[blockIdx.x]);
    const sa_seg_t *S = &segs[seg];
    const sa_region_t *R = &regions[S->region];
    if (WIDE) scr = RT.wscr + S->bscratch_off;
    if (tid == 0) {   // endStateProb / raggedEndStateProb (impl/stateMachine.c:1145-1173)
        const bool ragged = S->at_end && R->ragged_r;
        s_end[0] = ragged ? (T.t_mx + T.t_my) / 2.0 : T.t_mm;
        s_end[1] = ragged ? T.t_xx : T.t_xm;
        s_end[2] = ragged ? T.t_yy : T.t_ym;
    }
    __syncthreads();
    const int4 *rows4 = reinterpret_cast<const int4 *>(rows_all + R->row_off);
    const int *poff = poff_all + R->poff_off;
    if (MULTI && !EXPECT && (10ll * poff[R->lX + 1] > 13ll * (R->lX + 1)) != DENSE) return;   // (uniform: the other instance's segment)
    // addresses of vector stores that the sweep touches on few diagonals live in vector registers: the scalar file is the
    // scarce one here (spilled scalars cost v_readlane + s_nop in the serial chain)
    // (declared as global-memory pointers: behind the asm the compiler no longer sees where they came from, and a flat store
    // counts on lgkmcnt as well -- every LDS wait would wait for it)
    typedef __attribute__((address_space(1))) double gdouble_t;
    typedef __attribute__((address_space(1))) int gint_t;
    typedef __attribute__((address_space(1))) u32x4 gu32x4_t;
    typedef __attribute__((address_space(1))) u32x2 gu32x2_t;
    gdouble_t *vbuf_g = (gdouble_t *) vbuf;
    gint_t *overflow_g = (gint_t *) overflow;
    if (K == 1) asm volatile("" : "+v"(vbuf_g), "+v"(overflow_g));   // (K > 1: the vector registers are the scarce ones)
    const long long C = R->f_cellpaths;
    const double *F = F_all + 3 * R->f_base;
    const ring_xc_t rs_xc = (ring_xc_t) (xc_all + R->pid_off);
    const ring_ev_t rs_ev = (ring_ev_t) (ev_all + R->ev_off);
    const rsrc_t rs_F = make_rsrc(F);
    const rsrc_t rs_pr = MULTI ? make_rsrc_n(prec_all + R->pid_off, 16u * (unsigned) poff[R->lX + 1]) : make_rsrc(rows_all);
    const unsigned C8 = (unsigned) C * 8u;
    const rsrc_t rs_E = make_rsrc(HDP ? (const void *) (E_all + R->f_base) : (const void *) ev_all);   // HDP: the region's emission plane
    const ring_xc_t rs_xn = TWO ? (ring_xc_t) (reinterpret_cast<const double4 *>(E_all) + T.two_xn_off + R->pid_off) : rs_xc;
    const ring_ev_t rs_en = TWO ? (ring_ev_t) (reinterpret_cast<const double4 *>(E_all) + R->ev_off) : rs_ev;
    const ring_ev_t en_pad = TWO ? (ring_ev_t) (reinterpret_cast<const double4 *>(E_all) + T.two_xn_off - 1) : rs_ev;
    const int start = (int) S->start, from = (int) S->from, to = (int) S->to;
    gu32x2_t *my_cands = (gu32x2_t *) (cands + S->cand_off);   // 24-byte records, written as a 16-byte and an 8-byte store
    if (K == 1) asm volatile("" : "+v"(my_cands));
    const int cand_cap = S->cand_cap;
    const long long ck_base = S->ck_base;
    const unsigned ninf_a = lds_base(LT + LA_TAB_DOUBLES), scrap_a = ninf_a + 8u;
    const unsigned plane = (unsigned) cap * 8u, slot = 3u * plane;
    // the transitions too (one VGPR pair each, same v_add_f64): 14 scalars less to spill
    double t_mm = T.t_mm, t_my = T.t_my, t_xm = T.t_xm, t_xx = T.t_xx, t_ym = T.t_ym, t_yy = T.t_yy, t_mx = T.t_mx;
    if (K == 1 && !MULTI) asm volatile("" : "+v"(t_mm), "+v"(t_my), "+v"(t_xm), "+v"(t_xx), "+v"(t_ym), "+v"(t_yy), "+v"(t_mx));
    if (K == 1 && MULTI) asm volatile("" : "+v"(t_mm), "+v"(t_my));   // (two of them: measured best of five choices, round 2)
    // Candidates (round 4): the bound is known before the sweep starts -- the traceback's speculative total from the forward sweep
    // (RingT.spec; sa_strip.inc) -- so a posterior cell-path is tested where it is computed and appended at once, in whatever
    // order the waves get there (a slot from one LDS counter per workgroup); k_finalize applies the exact test with the exact
    // totals of k_fold and k_gather_sorted puts a segment's survivors in candidate order (diagonals downwards, cells and paths
    // upwards).  What this sweep no longer does: the per-checkpoint maxima (two wave-wide reductions and an LDS exchange per ten
    // diagonals, a second barrier on the checkpoint diagonals of regions with several paths per cell), the per-chunk counts and
    // their prefix one diagonal later, and the parked candidates that waited for it.
    const double spec = RT.spec[seg];
    const double lim = (spec > NEG_INF) ? spec - RT.slack + T.thr_off : __builtin_inf();
    unsigned b0 = lds_base(ring), b1 = b0 + 2u * slot, b2 = b0 + slot;
    int g0_1 = 0, np_1 = 0, g0_2 = 0, np_2 = 0;
    // EXPECT: the seven sums of the current checkpoint group (this lane's share), and the group whose shares wait in s_xsum for
    // thread 0 (behind the barrier of the diagonal that closed it)
    double xa0 = 0.0, xa1 = 0.0, xa2 = 0.0, xa3 = 0.0, xa4 = 0.0, xa5 = 0.0, xa6 = 0.0;
    int x_pending = -1;
    auto x_close = [&](int group) {   // all waves: this wave's share of the group's sums into s_xsum
        const double v_[7] = {xa0, xa1, xa2, xa3, xa4, xa5, xa6};
#pragma unroll
        for (int k_ = 0; k_ < 7; k_++) {
            const double s_ = wave_sum(v_[k_]);
            if (lane == 0) s_xsum[tid >> 6][k_] = s_;
        }
        xa0 = xa1 = xa2 = xa3 = xa4 = xa5 = xa6 = 0.0;
        x_pending = group;
    };
    auto x_write = [&]() {            // behind a barrier: thread 0 adds the waves' shares up, in wave order
        if (x_pending >= 0 && tid == 0) {
            for (int k_ = 0; k_ < 7; k_++) {
                double s_ = 0.0;
                for (int w_ = 0; w_ < (nthr >> 6); w_++) s_ += s_xsum[w_][k_];
                gsum[(ck_base + x_pending) * 8 + k_] = s_;
            }
            gsum[(ck_base + x_pending) * 8 + 7] = 0.0;
            gmc[ck_base + x_pending] = spec;
        }
        x_pending = -1;
    };
    // Posterior diagonals are those with e <= from; checkpoints sit at e = from, from - 10, ...  tck counts the diagonals down
    // to the next checkpoint (0 on it), cki is that checkpoint's index -- carried along instead of divided out per diagonal
    int tck = start - from, cki = 0;   // (start >= from)
    int4 rup = rows4[start + 1], re = rows4[start], rdn = rows4[start - 1 >= 0 ? start - 1 : 0];   // rows e+1, e, e-1
    RingIn A[K], B[K];
    RingTwo An[TWO ? K : 1], Bn[TWO ? K : 1];   // (the other instances: one unused entry)
    u32x4 rq[K];   // per-path records of diagonal e - 1 (behind the request of a diagonal: e - 2)
    int g0nn = rows4[start - 2 >= 0 ? start - 2 : 0].w;   // first path of the row two below
    {   // inputs of diagonal `start`
        const int g0 = re.w, np = rup.z - re.z;
        // the forward value of a cell-path is needed on the posterior diagonals and on the one above the first checkpoint
        const bool wf = start <= from || (start - 1 == from && start - 1 > to);
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int j = tid + k * nthr;
            const bool act = j < np;
            ring_request<MULTI, true, HDP, TWO>(A[k], ring_rec<MULTI>(rs_pr, g0 + j), act, g0 + (act ? j : 0), start, rs_xc, rs_ev, rs_E,
                                                act ? (unsigned) (re.z + j) * 8u : C8 - 8u, &An[TWO ? k : 0], rs_xn, rs_en, en_pad);
            if (MULTI) A[k].po = poff[act ? (unsigned) A[k].x : 0u];
            rq[k] = ring_rec<MULTI>(rs_pr, rdn.w + j);
            A[k].fm = buf_load_f64_stream(rs_F, (act && wf) ? (unsigned) j * 8u + (unsigned) re.z * 8u : C8 - 8u, 0);   // else: -inf sentinel
            A[k].fx = A[k].fy = B[k].fx = B[k].fy = NEG_INF;
            if (MULTI && start == from) {   // (a traceback whose first diagonal is its first checkpoint)
                const unsigned vo_ = (act ? (unsigned) j * 8u : 0u) + (unsigned) re.z * 8u;
                A[k].fx = buf_load_f64_stream(rs_F, vo_, C8);
                A[k].fy = buf_load_f64_stream(rs_F, vo_, 2u * C8);
            }
        }
    }
    // several paths per cell: the path range of this thread's cell on a checkpoint diagonal (or the one above it), asked for one
    // diagonal ahead like every other input
    int2 PA = make_int2(0, 0), PB = make_int2(0, 0);
    if (MULTI && (start == from || (start - 1 == from && start - 1 > to))) {
        const int x0 = (start + re.x) >> 1;
        const int i = tid < re.y ? tid : 0;
        PA.x = poff[x0 + i]; PA.y = poff[x0 + i + 1];
    }

    int e = start;
    auto half = [&](RingIn (&cur)[K], RingIn (&nxt)[K], const int2 &pcur, int2 &pnxt, RingTwo (&curn)[TWO ? K : 1], RingTwo (&nxtn)[TWO ? K : 1]) {
        { const unsigned t = b2; b2 = b1; b1 = b0; b0 = t; }
        const int g0 = re.w, np = rup.z - re.z;
        const unsigned fo8 = (unsigned) re.z * 8u;
        const bool post = e <= from;
        const bool is_ck = tck == 0;                       // (a posterior diagonal)
        const bool pre_ck = tck == 1 && e - 1 > to;        // the next diagonal is a checkpoint
        sa_ck_t ck = {0, 0, 0}, ckn = {0, 0, 0};
        if (is_ck) ck = cks[ck_base + cki];
        if (pre_ck) ckn = cks[ck_base + cki];
        double *const scr_e = scr + (e & 1) * 3 * cap;     // (two copies by the diagonal's parity: see the per-cell loop below)
        int4 rdd = {0, 0, 0, 0};                            // EXPECT: row e - 2 (the middle neighbours' forward states)
        if (EXPECT) {
            x_write();                                      // (a group closed on the previous diagonal: behind that diagonal's barrier)
            if (is_ck && cki > 0) x_close(cki - 1);         // the group above this checkpoint is complete
            rdd = rows4[e - 2 >= 0 ? e - 2 : 0];
        }
        {   // request the inputs of diagonal e - 1 (behind the last diagonal: row `to`, valid and unused)
            const int g0n = rdn.w, npn = re.z - rdn.z;
            // diagonal e - 1 is a posterior diagonal or sits above the first checkpoint
            const bool wf = (e - 1 <= from || (e - 2 == from && e - 2 > to)) && (e - 1 > to);
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int j = tid + k * nthr;
                const bool act = j < npn;
                ring_request<MULTI, true, HDP, TWO>(nxt[k], rq[k], act, g0n + (act ? j : 0), e - 1, rs_xc, rs_ev, rs_E,
                                                    act ? (unsigned) (rdn.z + j) * 8u : C8 - 8u, &nxtn[TWO ? k : 0], rs_xn, rs_en, en_pad);
                if (MULTI) nxt[k].po = poff[act ? (unsigned) nxt[k].x : 0u];   // with the request: no load behind the candidate test
                rq[k] = ring_rec<MULTI>(rs_pr, g0nn + j);
                nxt[k].fm = buf_load_f64_stream(rs_F, (act && wf) ? (unsigned) j * 8u + (unsigned) rdn.z * 8u : C8 - 8u, 0);
                if (MULTI && pre_ck) {   // diagonal e - 1 is a checkpoint: its gap planes too (a scalar branch, one diagonal in ten)
                    const unsigned vo_ = (act ? (unsigned) j * 8u : 0u) + (unsigned) rdn.z * 8u;
                    nxt[k].fx = buf_load_f64_stream(rs_F, vo_, C8);
                    nxt[k].fy = buf_load_f64_stream(rs_F, vo_, 2u * C8);
                }
            }
            // ... and the path range of this thread's cell when e - 1 is a checkpoint or the diagonal above one
            if (MULTI && (pre_ck || (tck == 2 && e - 2 > to))) {
                const int x0n = (e - 1 + rdn.x) >> 1;
                const int i = tid < rdn.y ? tid : 0;
                pnxt.x = poff[x0n + i]; pnxt.y = poff[x0n + i + 1];
            }
        }
        const bool is_start = e == start;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int j = tid + k * nthr;
            if (__builtin_amdgcn_readfirstlane(j & ~63) >= np) continue;   // nothing of this wave's chunk is in the row
            const bool act = j < np;
            const RingIn &in = cur[k];
            const int g = g0 + (act ? j : 0);
            const int x = MULTI ? in.x : g, y = e - x;
            const int a0 = MULTI ? in.a0 : g + 1;
            double lM, lY_;
            emit_fast<HDP>(in.c, in.e, lM, lY_);
            if (TWO) {
                const double l2 = two_l2(curn[k].cn, curn[k].n3);
                lM += l2; lY_ += l2;
            }
            // EXPECT (round 6): the forward states the expectation terms of this cell-path need -- lower neighbour (x - 1, y) on e - 1 and
            // middle neighbour (x - 1, y - 1) on e - 2 for its first two legal predecessor paths, upper neighbour (x, y - 1) on e - 1 for its
            // own path -- are requested HERE, in front of the diagonal's arithmetic, with an address select instead of a branch (no
            // neighbour: the -inf sentinel of the match plane).  Until round 5 they were loaded behind the arithmetic inside per-lane
            // branches: a memory latency in the serial chain of every posterior diagonal.
            const bool xon = EXPECT && post && spec > NEG_INF;   // (wave-uniform)
            double xf[12];
            if (EXPECT && xon) {
                const int g0m1 = rdn.w, npm1 = re.z - rdn.z, g0m2 = rdd.w, npm2 = rdn.z - rdd.z;
                const unsigned om1 = (unsigned) rdn.z * 8u, om2 = (unsigned) rdd.z * 8u, sent = C8 - 8u;
                const bool have2 = e - 2 >= to && e - 2 >= 0;
#pragma unroll
                for (int i_ = 0; i_ < 2; i_++) {
                    const int q_ = in.p0 + i_ * in.stride;
                    const int jl = q_ - g0m1, jm = q_ - g0m2;
                    const bool has_ = act && i_ < in.npd && x >= 1;
                    const bool lo_ = has_ && (unsigned) jl < (unsigned) npm1;
                    const bool mi_ = has_ && have2 && y >= 1 && (unsigned) jm < (unsigned) npm2;
                    const unsigned vl = (unsigned) jl * 8u + om1, vm = (unsigned) jm * 8u + om2;
                    xf[5 * i_ + 0] = buf_load_f64(rs_F, lo_ ? vl : sent, 0);
                    xf[5 * i_ + 1] = buf_load_f64(rs_F, lo_ ? vl + C8 : sent, 0);
                    xf[5 * i_ + 2] = buf_load_f64(rs_F, mi_ ? vm : sent, 0);
                    xf[5 * i_ + 3] = buf_load_f64(rs_F, mi_ ? vm + C8 : sent, 0);
                    xf[5 * i_ + 4] = buf_load_f64(rs_F, mi_ ? vm + 2u * C8 : sent, 0);
                }
                const int ju = g - g0m1;
                const bool up_ = act && y >= 1 && (unsigned) ju < (unsigned) npm1;
                const unsigned vu = (unsigned) ju * 8u + om1;
                xf[10] = buf_load_f64(rs_F, up_ ? vu : sent, 0);
                xf[11] = buf_load_f64(rs_F, up_ ? vu + 2u * C8 : sent, 0);
            }
            // The reference scatters (doTransitionBackward, impl/pairwiseAligner.c:866-871); gathered, a cell-path folds the
            // terms of (x+1, y+1) successor by successor, then the one of (x, y+1), then those of (x+1, y) successor by
            // successor -- in that order (its logAdd is not associative at the 1e-4 level).  The fold over the first group may
            // be taken over the messages themselves: every term carries the same transition.  A -inf term leaves a sum
            // unchanged exactly: the second successor is folded without a branch, third and later ones in a loop.
            const int i2 = a0 - g0_2, i1 = a0 - g0_1;
            double cm = lds_ld(ring_addr(b2, i2, np_2, ninf_a));                         // mM of (x+1, y+1)
            const double cx = lds_ld(ring_addr(b1 + 2u * plane, i1, np_1, ninf_a));      // mX of (x+1, y)
            double cx2 = NEG_INF;
            // (the sparse instance -- DENSE, k_fwd_ring: a wave none of whose cell-paths has a second successor skips the three logAdds)
            const bool any2 = MULTI && (DENSE || __builtin_amdgcn_ballot_w64(in.na >= 2) != 0ull);
            if (MULTI && any2) {
                const int n2 = in.na >= 2 ? np_2 : 0, n1 = in.na >= 2 ? np_1 : 0;
                cm = la_fast(LT, cm, lds_ld(ring_addr(b2, i2 + 1, n2, ninf_a)));
                cx2 = lds_ld(ring_addr(b1 + 2u * plane, i1 + 1, n1, ninf_a));
                if (__builtin_amdgcn_ballot_w64(in.na > 2) != 0ull)
                    for (int s_ = 2; s_ < in.na; s_++) cm = la_fast(LT, cm, lds_ld(ring_addr(b2, i2 + s_, np_2, ninf_a)));
            }
            const double vy = lds_ld(ring_addr(b1 + plane, g - g0_1, np_1, ninf_a));     // mY of (x, y+1), same path
            LaP pa, px, py;
            la_prep(pa, cm + t_mm, vy + t_my);
            la_prep(px, cm + t_xm, cx + t_xx);
            la_prep(py, cm + t_ym, vy + t_yy);
            la_fetch(pa, LT); la_fetch(px, LT); la_fetch(py, LT);
            double tm = la_fast(LT, la_finish(pa), cx + t_mx);
            double tx = la_finish(px);
            double ty = la_finish(py);
            if (MULTI && any2) {
                tm = la_fast(LT, tm, cx2 + t_mx);
                tx = la_fast(LT, tx, cx2 + t_xx);
                if (__builtin_amdgcn_ballot_w64(in.na > 2) != 0ull)
                    for (int s_ = 2; s_ < in.na; s_++) {
                        const double cxs = lds_ld(ring_addr(b1 + 2u * plane, i1 + s_, np_1, ninf_a));
                        tm = la_fast(LT, tm, cxs + t_mx);
                        tx = la_fast(LT, tx, cxs + t_xx);
                    }
            }
            if (is_start) { tm = s_end[0]; tx = s_end[1]; ty = s_end[2]; }
            const unsigned wa = act ? b0 + (unsigned) j * 8u : scrap_a;
            const unsigned wstep = act ? plane : 0u;
            lds_st(wa, tm + lM); lds_st(wa + wstep, ty + lY_); lds_st(wa + 2u * wstep, tx + SA_LOG_GAPX);
            const double fb = in.fm + tm;   // -inf for lanes without a cell-path and where the forward value is not needed
            if (EXPECT && xon) {
                // this cell-path's messages, relative to the scale; the forward states of its neighbours arrived above (a neighbour
                // that does not exist reads the -inf sentinel: its terms are exp(-inf) = 0)
                const double bM = tm + lM - spec, bY = ty + lY_ - spec, bX = tx + SA_LOG_GAPX - spec;
                // (term by term in the order of round 5's per-lane loop: the same sums bit for bit)
                xa0 += exp_term(xf[0] + t_mx + bX); xa1 += exp_term(xf[1] + t_xx + bX);
                xa2 += exp_term(xf[2] + t_mm + bM); xa3 += exp_term(xf[3] + t_xm + bM); xa4 += exp_term(xf[4] + t_ym + bM);
                xa0 += exp_term(xf[5] + t_mx + bX); xa1 += exp_term(xf[6] + t_xx + bX);
                xa2 += exp_term(xf[7] + t_mm + bM); xa3 += exp_term(xf[8] + t_xm + bM); xa4 += exp_term(xf[9] + t_ym + bM);
                xa5 += exp_term(xf[10] + t_my + bY);
                xa6 += exp_term(xf[11] + t_yy + bY);
                // a third and later predecessor (ambiguity codes of more than two letters): on the spot
                if (__builtin_amdgcn_ballot_w64(act && in.npd > 2) != 0ull) {
                    const int g0m1 = rdn.w, npm1 = re.z - rdn.z, g0m2 = rdd.w, npm2 = rdn.z - rdd.z;
                    const unsigned om1 = (unsigned) rdn.z * 8u, om2 = (unsigned) rdd.z * 8u;
                    const bool have2 = e - 2 >= to && e - 2 >= 0;
                    for (int i_ = 2; act && i_ < in.npd; i_++) {
                        const int q_ = in.p0 + i_ * in.stride;
                        const int jl = q_ - g0m1, jm = q_ - g0m2;
                        if (x >= 1 && (unsigned) jl < (unsigned) npm1) {
                            const unsigned vo_ = (unsigned) jl * 8u + om1;
                            const double f_m = buf_load_f64(rs_F, vo_, 0), f_x = buf_load_f64(rs_F, vo_, C8);
                            xa0 += exp_term(f_m + t_mx + bX);
                            xa1 += exp_term(f_x + t_xx + bX);
                        }
                        if (have2 && x >= 1 && y >= 1 && (unsigned) jm < (unsigned) npm2) {
                            const unsigned vo_ = (unsigned) jm * 8u + om2;
                            const double f_m = buf_load_f64(rs_F, vo_, 0), f_x = buf_load_f64(rs_F, vo_, C8), f_y = buf_load_f64(rs_F, vo_, 2u * C8);
                            xa2 += exp_term(f_m + t_mm + bM);
                            xa3 += exp_term(f_x + t_xm + bM);
                            xa4 += exp_term(f_y + t_ym + bM);
                        }
                    }
                }
            }
            if (post && !EXPECT) {
                // this diagonal's candidates (border cells excluded)
                const bool pass = act && x > 0 && y > 0 && fb >= lim;
                const unsigned long long mask = __ballot(pass);
                if (mask) {
                    int base = 0;
                    if (lane == 0) base = atomicAdd(&s_count, __popcll(mask));
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (pass) {
                        const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
                        if (pos < cand_cap) {
                            u32x4 w4;   // sa_cand_t: x, y, path, pad | fb
                            w4.x = (unsigned) (x - 1); w4.y = (unsigned) (y - 1);
                            w4.z = MULTI ? (unsigned) (g - in.po) : 0u; w4.w = 0u;
                            u32x2 w2;
                            w2.x = (unsigned) __double2loint(fb); w2.y = (unsigned) __double2hiint(fb);
                            gu32x2_t *rec = my_cands + 3 * (long long) pos;
                            *(gu32x4_t *) rec = w4;
                            rec[2] = w2;
                        } else {
                            overflow_g[0] = 1;
                        }
                    }
                }
            }
            if (MULTI) {
                // (round 6) the cell-path's own term of the checkpoint's dot product, from values that came with its inputs: the
                // per-cell fold behind the barrier then reads LDS only.  Until round 5 the fold loaded the three forward values of
                // every path from memory inside the diagonal -- a memory latency in the serial chain on two diagonals in ten, 21 of
                // configs[2]'s 86 ms (probe: the sweep without the fold).  Same operands, same order: same bits.
                if (is_ck) {
                    const double v = la_fast(LT, la_fast(LT, fb, in.fx + tx), in.fy + ty);
                    if (act) scr_e[j] = v;
                }
                if (pre_ck && act) scr_e[cap + j] = fb;
            } else {
                if (pre_ck && act) vbuf_g[ckn.voff + ckn.nA + j] = fb;
                if (is_ck) {
                    const unsigned vo = (unsigned) j * 8u;
                    const double fx = act ? buf_load_f64(rs_F, vo, fo8 + C8) : NEG_INF;
                    const double fy = act ? buf_load_f64(rs_F, vo, fo8 + 2u * C8) : NEG_INF;
                    const double v = la_fast(LT, la_fast(LT, fb, fx + tx), fy + ty);
                    if (act) vbuf_g[ck.voff + j] = v;
                }
            }
        }
        __syncthreads();   // messages of this diagonal (and, several paths per cell: the sums of a checkpoint diagonal in scr_e)
        if (MULTI && (is_ck || pre_ck)) {
            // per CELL: dot products over the cell's paths in path order (cell_dotProduct / hdCell_totalProbability,
            // impl/pairwiseAligner.c:828-890), exactly as the memory-resident kernels fold them.  No barrier behind the loop: the
            // next diagonal that writes sums (a checkpoint follows the diagonal above it) takes the other copy of scr, and the one
            // after that is separated from this loop by two barriers.
            const int x0 = (e + re.x) >> 1;
            auto cell_fold = [&](int i, int pa, int pb) {
                double cellA = NEG_INF, cellB = NEG_INF;
                for (int p = pa; p < pb; p++) {
                    if (pre_ck) cellB = la_fast(LT, cellB, scr_e[cap + p]);
                    if (is_ck) cellA = la_fast(LT, cellA, scr_e[p]);
                }
                if (is_ck) vbuf_g[ck.voff + i] = cellA;
                if (pre_ck) vbuf_g[ckn.voff + ckn.nA + i] = cellB;
            };
            // the thread's first cell: its path range was asked for a diagonal ahead -- no load on this path (a conditional load here
            // made the compiler wait with vmcnt(0), i.e. for the next diagonal's inputs and this diagonal's stores, on every checkpoint
            // diagonal); rows wider than the workgroup (several cell-paths per thread): the further cells on the spot
            if (tid < re.y) cell_fold(tid, pcur.x - g0, pcur.y - g0);
            if (K > 1)
                for (int i = tid + nthr; i < re.y; i += nthr) cell_fold(i, poff[x0 + i] - g0, poff[x0 + i + 1] - g0);
        }
        g0_2 = g0_1; np_2 = np_1; g0_1 = g0; np_1 = np;
        rup = re; re = rdn;
        rdn = rows4[e - 2 >= 0 ? e - 2 : 0];
        g0nn = rows4[e - 3 >= 0 ? e - 3 : 0].w;
        if (tck == 0) { tck = SA_CKPT_EVERY; cki++; }
        tck--;
        e--;
    };
    while (e > to) {
        half(A, B, PA, PB, An, Bn);
        if (e <= to) break;
        half(B, A, PB, PA, Bn, An);
    }
    __syncthreads();
    if (EXPECT) {
        x_write();
        __syncthreads();   // (thread 0 has read the shares of a group the last diagonal closed before the waves write the next)
        if (S->n_ck > 0) { x_close(S->n_ck - 1); __syncthreads(); x_write(); }
    }
    if (tid == 0) cand_count[seg] = s_count < cand_cap ? s_count : cand_cap;
}

// waves per workgroup and cell-paths per thread for a ring of `cap` entries per row
static int ring_waves(int cap) {
    const char *e = getenv("SA_RING_WAVES");   // tuning / test hook, read at every launch like SA_RING / SA_STRIP
    const int forced = e ? atoi(e) : 0;
    if (forced == 1 || forced == 2 || forced == 4) return forced;
    return cap <= 64 ? 1 : (cap <= 128 ? 2 : 4);
}
static size_t ring_lds_fwd(int cap) { return sizeof(double) * (size_t) (LA_TAB_DOUBLES + RING_XTRA + 9 * (cap + 1)); }   // (+1: the guard cells)
static size_t ring_lds_bwd(int cap, bool multi) {
    return sizeof(double) * (size_t) (LA_TAB_DOUBLES + RING_XTRA + (multi ? 15 : 9) * cap);
}
static RingT make_ring_t(const DevPlan &P, int cap, bool all_planes) {
    RingT RT;
    RT.f = make_fast_t(P);
    RT.cap = cap;
    RT.spec = P.spec;
    RT.slack = P.spec_slack;
    RT.all_planes = all_planes;
    RT.wscr = P.bscratch;
    return RT;
}
// calls f(std::integral_constant<int, K>()) with the instance K -- cell-paths per thread and diagonal, 1, 2, 4 or 8 -- that
// covers a ring of `cap` entries per row on `waves` waves
template <typename Fn>
static void with_ring_k(int cap, int waves, Fn f) {
    const int K = (cap + 64 * waves - 1) / (64 * waves);
    if (K <= 1) f(std::integral_constant<int, 1>());
    else if (K == 2) f(std::integral_constant<int, 2>());
    else if (K <= 4) f(std::integral_constant<int, 4>());
    else f(std::integral_constant<int, 8>());
}

// a launch with more dynamic LDS than the default limit of a kernel: say so first
template <typename Kern>
static void ring_lds_limit(Kern k, size_t bytes) {
    if (bytes > 64u * 1024u) (void) hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
}
// the wide class (SA_RING_WIDE_MAX_ROWPATHS, sa_internal.h) exists for the two-distribution instances with several paths per cell
// only: the planner sends no other region there, and a launch without a kernel is an error (SA_EUNSUPPORTED from the launch)
static int ring_wide(int cap, bool multi, bool two, bool *wide) {
    *wide = cap > SA_RING_MAX_ROWPATHS;
    if (*wide && (!multi || !two || cap != SA_RING_WIDE_MAX_ROWPATHS)) {
        fprintf(stderr, "[signalalign_hip] no ring kernel for rows of %d cell-paths (multi %d, two-distribution %d)\n", cap, (int) multi, (int) two);
        return SA_EUNSUPPORTED;
    }
    return SA_OK;
}

// One workgroup per region (forward) / segment (backward).  cap: cell-paths per ring row, a multiple of 64 up to 512 (or the wide
// class's 2048); multi: several paths per cell, where the dense and then the sparse instance run over the same list (DENSE above
// k_fwd_ring).
static int launch_fwd_ring(const DevPlan &P, const int *ids, int n, hipStream_t st, int cap, bool multi) {
    bool wide_ = false;
    const int rcw = ring_wide(cap, multi, P.two != nullptr && !P.m.hdp, &wide_);
    if (rcw) return rcw;
    const int waves = wide_ ? RING_MAX_WAVES : ring_waves(cap);   // (wide: K = 8 on four waves, whatever SA_RING_WAVES says)
    const RingT RT = make_ring_t(P, cap, P.expect);
    const bool hdp = P.m.hdp;
    const bool two = P.two != nullptr;   // the two-distribution emission (never with an HDP model)
    with_ring_k(cap, waves, [&](auto KK) {
        constexpr int K = decltype(KK)::value;
        auto launch = [&](auto k) {
            ring_lds_limit(k, ring_lds_fwd(cap));
            hipLaunchKernelGGL(k, dim3(n), dim3(64 * waves), ring_lds_fwd(cap), st, P.regions, P.rows, P.pk, P.prec,
                               reinterpret_cast<const double4 *>(P.xc), P.ev, P.F, RT, ids, n, P.poff,
                               hdp ? (const double *) P.E : P.two, P.segs);
        };
        if (two) {
            if (multi) {
                launch(k_fwd_ring<true, K, false, true, true>);
                launch(k_fwd_ring<true, K, false, false, true>);
            } else {
                launch(k_fwd_ring<false, K, false, true, true>);
            }
        } else if (multi) {
            launch(hdp ? k_fwd_ring<true, K, true> : k_fwd_ring<true, K, false>);
            launch(hdp ? k_fwd_ring<true, K, true, false> : k_fwd_ring<true, K, false, false>);
        } else {
            launch(hdp ? k_fwd_ring<false, K, true> : k_fwd_ring<false, K, false>);
        }
    });
    return SA_OK;
}
// the expectation pass (P.expect) takes the EXPECT instance for several paths per cell (Gaussian emissions)
static int launch_bwd_ring(const DevPlan &P, const int *ids, int n, hipStream_t st, int cap, bool multi) {
    const bool expect = P.expect && multi;
    bool wide_ = false;
    const int rcw = ring_wide(cap, multi, P.two != nullptr && !expect && !P.m.hdp, &wide_);
    if (rcw) return rcw;
    const int waves = wide_ ? RING_MAX_WAVES : ring_waves(cap);
    const size_t lds = ring_lds_bwd(cap, multi && !wide_);
    const RingT RT = make_ring_t(P, cap, expect);
    const bool hdp = P.m.hdp && !expect;
    const bool two = P.two != nullptr && !expect;   // (the expectation pass of such a model never gets here: reference-ordered kernels)
    with_ring_k(cap, waves, [&](auto KK) {
        constexpr int K = decltype(KK)::value;
        auto launch = [&](auto k) {
            ring_lds_limit(k, lds);
            hipLaunchKernelGGL(k, dim3(n), dim3(64 * waves), lds, st, P.regions, P.segs, P.rows, P.poff, P.cks,
                               P.prec, reinterpret_cast<const double4 *>(P.xc), P.ev, (const double *) P.F, P.vbuf, P.cands,
                               P.cand_count, P.overflow, RT, ids, n, hdp ? (const double *) P.E : P.two,
                               expect ? P.gsum : nullptr, expect ? P.gmc : nullptr);
        };
        if (wide_) {
            if constexpr (K == 8) {
                launch(k_bwd_ring<true, 8, false, false, true, true, true>);
                launch(k_bwd_ring<true, 8, false, false, false, true, true>);
            }
        } else if (two) {
            if (multi) {
                launch(k_bwd_ring<true, K, false, false, true, true>);
                launch(k_bwd_ring<true, K, false, false, false, true>);
            } else {
                launch(k_bwd_ring<false, K, false, false, true, true>);
            }
        } else if (expect) {
            launch(k_bwd_ring<true, K, false, true>);
        } else if (multi) {
            launch(hdp ? k_bwd_ring<true, K, true> : k_bwd_ring<true, K, false>);
            launch(hdp ? k_bwd_ring<true, K, true, false, false> : k_bwd_ring<true, K, false, false, false>);
        } else {
            launch(hdp ? k_bwd_ring<false, K, true> : k_bwd_ring<false, K, false>);
        }
    });
    return SA_OK;
}
