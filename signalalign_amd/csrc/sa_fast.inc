// sa_fast.inc -- register-resident forward / backward kernels (one path per cell, Gaussian emissions).
// Included by sa_hip.hip.
//
// Lane mapping.  A cell (x,y) sits on anti-diagonal d = x+y at u = (x-y+K)>>1 (K even, per region).  It is
// handled by lane u mod 64.  With that mapping
//     middle  neighbour (x-1,y-1) on d-2 : same u   -> same lane, value kept in a register for two steps
//     d even: lower (x-1,y) on d-1 is u-1 -> lane-1 ; upper (x,y-1) on d-1 is u   -> same lane
//     d odd : lower                is u   -> same  ; upper                is u+1 -> lane+1
// so one step needs ONE cross-lane move of ONE double (a DPP whole-wave rotate).  The band drifts through
// the lanes circularly, no data ever moves.  Lanes outside the band hold -inf, which logAdd ignores, so
// "neighbour missing" needs no test as long as three consecutive diagonals plus one cell each side fit in
// 64 lanes (SA_PK_FWD / SA_PK_BWD).  Diagonals that do not fit (start/end of a read, sparse anchors) take the
// memory-resident path, in the same kernel, reading the previous diagonals back from memory.
//
// What travels between cells.  logAdd(a+k, b+k) = logAdd(a,b)+k, so the emission of the receiving cell can be
// added AFTER the sums over the sending cell's states.  A finished forward cell (m, x, y) therefore publishes
//     oM = m(+)x(+)y with the match-bound transitions   -> cell (x+1,y+1), same lane two steps later
//     oX = m(+)x     with log(0.1) + gapX transitions   -> cell (x+1,y)
//     oY = m(+)y     with the gapY transitions          -> cell (x,y+1)
// and the receiver only adds its own emission: m' = oM + eM, x' = oX, y' = oY + eY.  The backward sweep is the
// mirror image (its messages carry the sender's emission).
//
// Instruction economy (the sweeps are issue-bound: every VALU or SALU instruction costs a wave ~4.4 cycles):
//   * everything integer and wave-uniform about a diagonal is one packed 32-bit word (sa_internal.h SA_PK_*),
//     flags included; a wave fetches 64 words with one coalesced load and picks the current one with v_readlane;
//   * the loop is unrolled over an (even, odd) pair of diagonals so the direction of the DPP rotate and the
//     register that carries oM are static; the value slots are named by the parity of the diagonal that wrote them;
//   * loads and stores are raw buffer instructions: base in SGPRs, a 32-bit per-lane byte offset, the running
//     offset of the diagonal in the scalar offset operand -- no 64-bit address arithmetic in vector registers;
//   * inputs of the next diagonal are requested before the current one is stored (vmcnt is in-order);
//   * logAdd: see la_fast below.
//
// Arithmetic: per-position constants (m, inv_s, cM, cY) fold the read's scale/shift/var in (sa_plan.c:fill_xc).

#define FAST_WAVES 4

struct FastT {  // transition constants, wave-uniform
    double t_mm, t_xm, t_ym, t_my, t_yy, t_mx, t_xx;
    double thr_off;  // log(threshold) - SA_CAND_EPS
    // HDP emissions only: the uniform grid of the posterior-predictive splines
    double g0, gN, dx, inv_dx, nm2;  // first/last grid point, spacing, grid_length - 2
    unsigned hdp_bytes;              // size of the interleaved {y, slope} table
    unsigned hdp_hot;                // byte offset (in that table) of the row most k-mers resolve to, 0xffffffff: none (k_emit_hdp)
    int wide_cap;                    // cells per row of the forward kernel's LDS ring for wide diagonals (0: none)
    // per traceback segment its speculative total (k_spec_match, sa_hip.hip; sa_strip.inc "the speculative total of a traceback"):
    // the candidate bound of the backward sweep is spec - slack + log(threshold), known before the sweep starts.  nullptr: the
    // bound comes from the maximum term of each checkpoint (the expectation pass, which scales its sums by that maximum anyway)
    const double *spec;
    double slack;
    // two-distribution emission (SA_EMISSION_TWO_DIST*, the *_two kernels): the kernels' E argument is a buffer of double4 entries --
    // per event {noise, 1 / noise, 1.5 log noise, 0}, then from entry two_xn_off on per path-space index {(log lambda - log 2 pi) / 2,
    // 1 / noise mean, lambda / 2, 0} of the position's k-mer
    long long two_xn_off;
};

// logAdd(x, y) = max + log(1 + exp(-|x-y|)), with the reference's approximation of the second term
// (impl/pairwiseAligner.c:285-318: four cubic pieces on [0,1], (1,2.5], (2.5,4.5], (4.5,7.5), zero from 7.5 on).
// Evaluated as mx + P_j(dc), dc = min(|x-y|, 8), where P_j = piece - identity (the reference adds the piece to the
// minimum).  All break points are multiples of 0.5, so the piece is selected by j = floor(2 dc): dc + 8 lies in
// [8, 16], where one ulp of the top mantissa bits is 0.5 -- j is bits 16..20 of its high word (dc == 8 flips the
// exponent bit and gives j = 16).  One add, one v_bfe, one shift and a 32-byte LDS read replace three fp64 compares
// and the selects; row 15 is zero and replaces the cut-off select (dc is clipped just below 8).  The clip also keeps +inf (one side
// -inf) and NaN (both -inf: v_min returns the other operand) out of the polynomial; the result is then the maximum.
//
// Layout: rows of 48 bytes (32 of coefficients + 16 unused).  A lane reads its row with two ds_read_b128, which the LDS serves
// in groups of 16 lanes over 64 banks of 4 bytes (MI355X_MICROARCH.md, LDS): with 32-byte rows the quarter-rows of rows j and
// j + 8 share their four banks, and a group that holds both pays a second cycle -- a third of all LDS-array cycles of the
// register kernels were such conflicts (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE, profiles/r03_lds_*.json).  With 48-byte
// rows the first quarter-rows of rows 0..15 start at banks 12 j mod 64 = sixteen different multiples of four, the second
// ones four banks further: any mix of rows in a group is conflict-free.  Row 16 (dc == 8 exactly) would share row 0's banks,
// so dc is clipped just below 8 instead and row 15 -- zeros as well -- serves the cut-off.
#define LA_ROWS 16
#define LA_ROW_DOUBLES 6
#define LA_TAB_DOUBLES (LA_ROW_DOUBLES * LA_ROWS)
__device__ __forceinline__ void la_tab_init(double *tab, int tid) {
    if (tid < LA_ROWS) {
        const float a3[4] = {-0.009350833524763f, -0.014532321752540f, -0.004605031767994f, -0.000458661602210f};
        const float a2[4] = {0.130659527668286f, 0.139942324101744f, 0.063427417320019f, 0.009695946122598f};
        const float a1[4] = {0.498799810682272f, 0.495635523139337f, 0.695956496475118f, 0.930734667215156f};
        const float a0[4] = {0.693203116424741f, 0.692140569840976f, 0.514272634594009f, 0.168037164329057f};
        // row j <-> dc in [j/2, (j+1)/2): 0..1 -> [0,1); 2..4 -> [1,2.5); 5..8 -> [2.5,4.5); 9..14 -> [4.5,7.5); 15 -> 0
        int piece = tid <= 1 ? 0 : (tid <= 4 ? 1 : (tid <= 8 ? 2 : (tid <= 14 ? 3 : -1)));
        double *row = tab + LA_ROW_DOUBLES * tid;
        if (piece >= 0) {
            row[0] = (double) a3[piece];
            row[1] = (double) a2[piece];
            row[2] = (double) a1[piece] - 1.0;
            row[3] = (double) a0[piece];
        } else {
            row[0] = 0.0; row[1] = 0.0; row[2] = 0.0; row[3] = 0.0;
        }
        for (int q = 4; q < LA_ROW_DOUBLES; q++) row[q] = 0.0;
    }
}

// Per-site tables.  logAdd(a + k1, b + k2) = k1 + logAdd(a, b + (k2 - k1)) and the constant k1 can sit in the table's constant
// term (row 15, the cut-off, then holds k1 instead of 0): a cell's four logAdds need three operand additions instead
// of seven.  The forward sweeps keep four such tables (sites 0..3, see la_sites_fwd); the backward sweeps stay on the plain
// table: there the extra constants cost registers (k_bwd_fast: twelve spilled at its 96-register budget) and the sweeps came
// out 2-4 % slower.
#define LA_SITES 4
__device__ __forceinline__ void la_tab_init_site(double *tab, int tid, double k) {
    la_tab_init(tab, tid);
    if (tid < LA_ROWS) tab[LA_ROW_DOUBLES * tid + 3] += k;
}
// forward: site 0 folds match-bound sums of (m, x), site 1 the gapX message, site 2 the gapY message, site 3 adds y to site 0
struct LaSiteK { double k0, k1, k2, k3, a0, a1, a2; };   // table constants and the three operand offsets
// the three fetched logAdds of a step are waited for with ONE s_waitcnt lgkmcnt(0) (the compiler otherwise counts the six
// reads down with six waits: every wait is an issue slot of a sweep that is bound by instruction issue)
__device__ __forceinline__ void la_wait() { __builtin_amdgcn_s_waitcnt(0xc07f); }

// v_max_f64 / v_min_f64 as written: the compiler otherwise adds a canonicalising v_max(x,x) in front of values that
// crossed a branch.  Both return the other operand when one is NaN.
__device__ __forceinline__ double vmax(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double vmin_abs_8(double a) {  // min(|a|, 8 - 2^-40): the last value of row 15
    // (round 4: as a builtin.  Its argument is always the difference la_prep has just taken, which the compiler knows to be
    // canonical -- no v_max(x, x) in front -- and the hazard recogniser keeps one wait state between an inline-asm VALU and a
    // VALU that reads its result: an s_nop per logAdd wherever the scheduler had nothing to put there)
    return __builtin_fmin(__builtin_fabs(a), 0x1.fffffffffcp+2);
}

// two-phase logAdd: the coefficient reads of independent logAdds are issued together, then consumed
struct LaP {
    double mx, dc;
    double4 c;
};
__device__ __forceinline__ void la_prep(LaP &p, double x, double y) {
    p.mx = vmax(x, y);
    p.dc = vmin_abs_8(x - y);  // x - y: +-inf if one side is -inf, NaN if both are
}
__device__ __forceinline__ void la_fetch(LaP &p, const double *tab) {
    const unsigned j = __builtin_amdgcn_ubfe((unsigned) __double2hiint(p.dc + 8.0), 16u, 5u);
    p.c = *reinterpret_cast<const double4 *>(reinterpret_cast<const char *>(tab) + j * (unsigned) (8 * LA_ROW_DOUBLES));
}
__device__ __forceinline__ double la_finish(const LaP &p) {
    return p.mx + fma(fma(fma(p.c.x, p.dc, p.c.y), p.dc, p.c.z), p.dc, p.c.w);
}
__device__ __forceinline__ double la_fast(const double *tab, double x, double y) {
    LaP p;
    la_prep(p, x, y);
    la_fetch(p, tab);
    return la_finish(p);
}

// whole-wave rotates by one lane (v_mov_b32_dpp wave_ror:1 / wave_rol:1; verified on gfx950 with probes/dpp_probe.hip)
__device__ __forceinline__ double from_lane_below(double v) {  // lane i <- lane i-1, lane 0 <- lane 63
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, 0x13C, 0xF, 0xF, false);  // every lane has a source: no old value needed
    hi = __builtin_amdgcn_mov_dpp(hi, 0x13C, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double from_lane_above(double v) {  // lane i <- lane i+1, lane 63 <- lane 0
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, 0x134, 0xF, 0xF, false);
    hi = __builtin_amdgcn_mov_dpp(hi, 0x134, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ void wave_fence() {
    // make this wave's earlier global stores visible to its later loads from other lanes
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

__device__ __forceinline__ int pk_width(int p) { return p & SA_PK_WIDTH_MASK; }
__device__ __forceinline__ unsigned pk_row_bytes(int p) {  // storage of a diagonal inside a plane (128-byte granules)
    return (unsigned) (((p & SA_PK_WIDTH_MASK) + (SA_FAST_ROW_ALIGN - 1)) & ~(SA_FAST_ROW_ALIGN - 1)) * 8u;
}
__device__ __forceinline__ int pk_ul(int p) { return (int) ((unsigned) p >> SA_PK_SHIFT); }

// raw buffer access: 48-bit base + flags in four SGPRs, byte offset = per-lane voffset + scalar soffset
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void *base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ rsrc_t make_rsrc_n(const void *base, unsigned bytes) {   // exact size: beyond it loads return 0
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int) bytes, 0x00020000);
}
__device__ __forceinline__ double buf_load_f64(rsrc_t r, unsigned voff, unsigned soff) {
    u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
    return __hiloint2double((int) v.y, (int) v.x);
}
#define SA_F_CACHE_POLICY 2  // nt: the forward planes are written once and read once, much later -- do not keep them in L2
__device__ __forceinline__ void buf_store_f64(rsrc_t r, unsigned voff, unsigned soff, double x) {
    u32x2 v;
    v.x = (unsigned) __double2loint(x);
    v.y = (unsigned) __double2hiint(x);
    __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, soff, SA_F_CACHE_POLICY);
}
__device__ __forceinline__ double buf_load_f64_stream(rsrc_t r, unsigned voff, unsigned soff) {
    u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, SA_F_CACHE_POLICY);
    return __hiloint2double((int) v.y, (int) v.x);
}
__device__ __forceinline__ double4 buf_load_f64x4(rsrc_t r, unsigned voff) {
    u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0);
    u32x4 b = __builtin_amdgcn_raw_buffer_load_b128(r, voff + 16u, 0, 0);
    double4 o;
    o.x = __hiloint2double((int) a.y, (int) a.x);
    o.y = __hiloint2double((int) a.w, (int) a.z);
    o.z = __hiloint2double((int) b.y, (int) b.x);
    o.w = __hiloint2double((int) b.w, (int) b.z);
    return o;
}

// one diagonal's per-lane geometry and inputs (requested, not yet waited for)
struct Stage {
    int t;      // cell index inside the diagonal
    int x, y;   // matrix coordinates (meaningful when act)
    bool act;
    double4 c;  // position constants; the NULL entry (-inf emissions) for lanes without a cell or without an event
    double e;   // event mean
    double4 cn, n3;   // two-distribution emission only: the position's and the event's noise constants (FastT.two_xn_off)
};

// d: diagonal, p: its packed word.  x = u + (d + (d&1) - K)/2 with u = uL + t.
__device__ __forceinline__ Stage stage_inputs(int p, int d, int K, int lane, rsrc_t xc, rsrc_t ev) {
    Stage s;
    const int uL = pk_ul(p);
    const int hb = (d + (d & 1) - K) >> 1;
    s.t = (lane - uL) & 63;
    s.act = s.t < pk_width(p);
    s.x = s.t + (uL + hb);
    s.y = d - s.x;
    const bool ok = s.act && s.y >= 1;  // a k-mer/event pair exists (x == 0 is the NULL entry itself)
    const unsigned xi = ok ? (unsigned) s.x : 0u;
    const unsigned yi = ok ? (unsigned) (s.y - 1) : 0u;
    s.c = buf_load_f64x4(xc, xi * 32u);
    s.e = buf_load_f64(ev, yi * 8u, 0);
    return s;
}

// ... and with the noise constants of the two-distribution emission (k_fwd_fast_two / k_bwd_fast_two)
__device__ __forceinline__ Stage stage_inputs_two(int p, int d, int K, int lane, rsrc_t xc, rsrc_t ev, rsrc_t xn, rsrc_t en) {
    Stage s = stage_inputs(p, d, K, lane, xc, ev);
    const bool ok = s.act && s.y >= 1;
    s.cn = buf_load_f64x4(xn, (ok ? (unsigned) s.x : 0u) * 32u);
    s.n3 = buf_load_f64x4(en, (ok ? (unsigned) (s.y - 1) : 0u) * 32u);
    return s;
}
// The inverse-Gaussian term of the event's noise, emissions_signal_logInvGaussPdf (impl/stateMachine.c:285-294):
// (log lambda - log 2 pi - 3 log n - lambda ((n - mu) / mu)^2 / n) / 2, the same for the match and the gapY state
// (emissions_signal_strawManGetKmerEventMatchProb[WithDescaling] :607-700 add it to the Gaussian of the level); cn = {(log lambda -
// log 2 pi) / 2, 1 / mu, lambda / 2}, n3 = {n, 1 / n, 1.5 log n}
__device__ __forceinline__ void emit_two(const double4 &cn, const double4 &n3, double &lM, double &lY) {
    const double a = fma(n3.x, cn.y, -1.0);
    const double l2 = cn.x - n3.z - cn.z * (a * a) * n3.y;
    lM += l2;
    lY += l2;
}

// HDP regions: the emission of every band cell was computed by k_emit_hdp (below) into a plane laid out like the match plane
// of the forward storage (cell t of diagonal d at foff(d) + t; cell C-1 is a -inf sentinel for lanes without a cell; cells
// without a k-mer/event pair hold -inf).  A stage then is ONE 8-byte load and no arithmetic: fo8 = byte offset of diagonal d.
__device__ __forceinline__ Stage stage_inputs_plane(int p, int d, int K, int lane, rsrc_t pe, unsigned fo8, unsigned sentinel8) {
    Stage s;
    const int uL = pk_ul(p);
    const int hb = (d + (d & 1) - K) >> 1;
    s.t = (lane - uL) & 63;
    s.act = s.t < pk_width(p);
    s.x = s.t + (uL + hb);
    s.y = d - s.x;
    s.e = buf_load_f64(pe, s.act ? (unsigned) s.t * 8u + fo8 : sentinel8, 0);
    return s;
}

__device__ __forceinline__ LaSiteK la_sites_fwd(const FastT &T) {
    LaSiteK K;
    const double cx_m = SA_LOG_GAPX + T.t_mx, cx_x = SA_LOG_GAPX + T.t_xx;
    K.k0 = T.t_mm - T.t_ym; K.a0 = T.t_xm - T.t_mm;   // site 0: (m (+) x) with the match-bound transitions, minus t_ym
    K.k1 = cx_m;            K.a1 = cx_x - cx_m;       // site 1: oX
    K.k2 = T.t_my;          K.a2 = T.t_yy - T.t_my;   // site 2: oY
    K.k3 = T.t_ym;                                    // site 3: (site 0) (+) y
    return K;
}
// Gaussian MeanOnly emission from the per-position constants (sa_plan.c:fill_xc), from the squared, scaled deviation q.  (Forcing the two fmas into VOP3 form -- the compiler writes v_mov_b64 + v_fmac --
// saves two instructions and made k_bwd_fast 3.5 % slower: measured, left to the compiler.)
__device__ __forceinline__ void emit_gauss_q(const double4 &c, double q, double &lM, double &lY) {
    lM = fma(q, -0.5, c.z);
    lY = fma(q, -0.5 / (SA_GAPY_SD_MULT * SA_GAPY_SD_MULT), c.w);
}
__device__ __forceinline__ void emit_gauss(const double4 &c, double e, double &lM, double &lY) {
    const double a = (e - c.x) * c.y;
    emit_gauss_q(c, a * a, lM, lY);
}

// HDP emission (emissions_signal_getHdpKmerDensity impl/stateMachine.c:527-554, grid_spline_interp
// impl/hdp_math_utils.c:471-495): match and gapY emissions are both log((1/var) * max(0, spline(e'))), with
// e' = e/var - ((scale - var) mu + shift)/var.  xc[x].x holds the second term, xc[x].y the byte offset of the k-mer's row
// of interleaved {y[i], slope[i]} (beyond the table for k-mers without an observed ancestor and for the NULL entry: the
// buffer range check then returns zeros, the density is 0 and the emission log(0)).  Two dependent 16-byte gathers per cell.
// The HDP emission depends on (k-mer, event) only and is the same for the match and the gapY state: it is computed ONCE per
// band cell, by all lanes of the chip in parallel, instead of twice (forward and backward sweep) inside a chain that is
// serial in the diagonal index and bound by instruction issue -- two dependent 16-byte gathers, a Hermite spline and a log
// per cell (round 2: k_bwd_fast_hdp 17 ms against k_bwd_fast 5.4 ms on the same cells).  One workgroup takes EMIT_TILE
// diagonals of one region, a wave one diagonal at a time; the plane is laid out like the match plane of the forward
// storage, so both sweeps address it with the offsets they already hold.  8 B per cell written, read twice.
#define EMIT_TILE 64

// exp() of an expectation term (round 4).  The terms of the expectation pass are forward + transition + backward - scale: at most a
// little above zero, often -inf.  The device library's exp guards both ends of the range with two compares and three selects per
// call and seven calls per cell make it a third of k_bwd_fast_expect's instructions; here: arguments below -746 (and -inf, NaN) are
// raised to -746, whose exponential is below the smallest denormal's half and comes out as 0 or one denormal; no upper guard
// (exp(700) is finite).  Cody-Waite reduction with the two-part ln 2 of fdlibm, Taylor polynomial of degree 13 on |r| <= 0.347
// (truncation 4e-18 relative), v_ldexp.  20 instructions against 26; 1 ulp-class accuracy (checked against the C library on the
// host side of tests/test_gpu_expectations.py through the sums themselves: rtol 1e-9 to the restatement, unchanged).
__device__ __forceinline__ double exp_term(double x) {
    x = __builtin_fmax(x, -746.0);
    const double n = __builtin_rint(x * 1.4426950408889634074);
    double r = fma(n, -6.93147180369123816490e-01, x);
    r = fma(n, -1.90821492927058770002e-10, r);
    double p = 1.6059043836821613e-10;              // 1 / 13!
    p = fma(p, r, 2.0876756987868100e-09);          // 1 / 12!
    p = fma(p, r, 2.5052108385441720e-08);          // 1 / 11!
    p = fma(p, r, 2.7557319223985888e-07);          // 1 / 10!
    p = fma(p, r, 2.7557319223985893e-06);          // 1 / 9!
    p = fma(p, r, 2.4801587301587302e-05);          // 1 / 8!
    p = fma(p, r, 1.9841269841269841e-04);          // 1 / 7!
    p = fma(p, r, 1.3888888888888889e-03);          // 1 / 6!
    p = fma(p, r, 8.3333333333333332e-03);          // 1 / 5!
    p = fma(p, r, 4.1666666666666664e-02);          // 1 / 4!
    p = fma(p, r, 1.6666666666666666e-01);          // 1 / 3!
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int) n);
}

// log of a finite v >= 0 by table (round 5; 18 instructions against 35 for round 3's frexp / s = f / (2 + f) / degree-7 routine and 105
// for the device library's): v = 2^e m, m in [0.5, 1); the top seven
// fraction bits of m name one of 128 rows {1/c, log c} (c the midpoint of the row's part of [0.5, 1): sa_logtab.inc, 2 KB of LDS),
// r = m (1/c) - 1 with |r| <= 2^-8 exactly representable up to the rounding of ONE fma, log m = log c + r (1 - r/2 + r^2/3 - r^3/4
// + r^4/5 - r^5/6) (truncation r^7 / 7 = 2e-18).  log c is the logarithm of the reciprocal of the ROUNDED 1/c, so the identity is
// exact; what is left is the rounding of e ln 2 with a one-piece ln 2 (|e| < 64 for a density: 4e-15 absolute).  Against the C
// library on 2 million values in [e^-40, e^5]: 7e-15 absolute, 1e-13 relative (gen_logtab.py's check).  LT holds `bias` added to
// every log c (the emission's constant term, per region), so the sum costs nothing.
static __device__ const double2 g_log_rows[128] = {
#include "sa_logtab.inc"
};
__device__ __forceinline__ double log_tab(double v, const double2 *LT) {
    const double m = __builtin_amdgcn_frexp_mant(v);
    const int e = __builtin_amdgcn_frexp_exp(v);
    const unsigned idx = __builtin_amdgcn_ubfe((unsigned) __double2hiint(m), 13u, 7u);
    const double2 row = LT[idx];
    const double r = fma(m, row.x, -1.0);
    double p = fma(r, -1.0 / 6.0, 0.2);
    p = fma(p, r, -0.25);
    p = fma(p, r, 1.0 / 3.0);
    p = fma(p, r, -0.5);
    p = fma(p, r, 1.0);
    const double lg = fma(r, p, fma((double) e, 6.93147180559945286227e-01, row.y));
    return v > 0.0 ? lg : NEG_INF;
}

// double -> int as the hardware converts: saturating at both ends, NaN -> 0 (v_cvt_i32_f64).  Written as the instruction because the
// language's conversion is undefined for exactly the values the emission kernels meet in every tile (a lane without an event holds
// NaN): the compiler emits this instruction for `(int) x` today, but may assume the operand is in range.
__device__ __forceinline__ int cvt_i32_sat(double v) {
    int r;
    asm("v_cvt_i32_f64 %0, %1" : "=v"(r) : "v"(v));
    return r;
}
// ... and to unsigned (a row's byte offset travels as a double beside the other constants; a lane beyond its diagonal reads slack of
// the staged constants that nobody wrote: any bit pattern, converted and not used)
__device__ __forceinline__ unsigned cvt_u32_sat(double v) {
    unsigned r;
    asm("v_cvt_u32_f64 %0, %1" : "=v"(r) : "v"(v));
    return r;
}

// Round 5: the cell's arithmetic cut to what it needs (121 -> 62 instructions per 64 cells; they cost four cycles each whatever
// they compute, so the count is the time):
//   * the spline as a cubic in t = position inside the interval, coefficients {y0, s0 dx, 3 dy - (2 s0 + s1) dx, (s0 + s1) dx - 2 dy}
//     per interval from a second table (`coef`: 32 B per interval, the same two 16-byte reads as {y, slope} of the two grid points):
//     three fma instead of fifteen operations.  The identity is exact in real arithmetic (expand grid_spline_interp's
//     t_r y0 + t_l y1 + t_l t_r (a t_r + b t_l) in t_l); in floating point the two forms differ by a few ulp of the larger of the two
//     grid values (1e-16 absolute for a density) -- the default kernels' HDP parity bar is 1e-5 on a posterior, measured worst
//     |dp| in DESIGN.md section 4; SA_FLAG_EXACT's kernels evaluate the reference's form in the reference's order and stay the checker;
//   * outside the grid (hardly ever) the reference extrapolates linearly: a wave-uniform branch reads {y, slope} of the end point
//     from the first table, as before;
//   * interval index: one fma, one conversion (saturating, NaN -> 0), an integer min / max instead of the fp64 clamp;
//   * the logarithm by table (log_tab), the emission's constant folded into the table.
// the density of a cell from its standardised event `en`, its position in grid units `tc`, the interval `il` and the interval's cubic
// coefficients {a, b} (`coef` table, 32 B per interval); off16: byte offset of grid point il in the {y, slope} table, read only by a
// wave that holds a cell at or beyond an end of the grid, where the reference extrapolates linearly (grid_spline_interp,
// impl/hdp_math_utils.c:471-495).  NaN (no event) -> 0.
__device__ __forceinline__ double hdp_density_coef(double en, double tc, int il, unsigned off16, bool ok, const u32x4 &a, const u32x4 &b,
                                                   rsrc_t rs_tab, const FastT &T) {
    const double c0 = __hiloint2double((int) a.y, (int) a.x), c1 = __hiloint2double((int) a.w, (int) a.z);
    const double c2 = __hiloint2double((int) b.y, (int) b.x), c3 = __hiloint2double((int) b.w, (int) b.z);
    const double tl = tc - (double) il;
    double v = fma(fma(fma(c3, tl, c2), tl, c1), tl, c0);
    if (__ballot(ok && !(tc > 0.0 && tc < T.nm2 + 1.0))) {   // wave-uniform, rare
        const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(rs_tab, off16 + (tc > 0.0 ? 16u : 0u), 0, 0);
        const double yq = __hiloint2double((int) q.y, (int) q.x), sq = __hiloint2double((int) q.w, (int) q.z);
        v = (en <= T.g0) ? yq - sq * (T.g0 - en) : v;
        v = (en >= T.gN) ? yq + sq * (en - T.gN) : v;
    }
    return __builtin_fmax(v, 0.0);
}

// the four coefficients of interval off16 / 16 as two 16-byte words of doubles (a probe build, -DEMIT_F32TAB, keeps them as floats in
// ONE 16-byte word: what a float-pair table would save and cost -- profiles/r05_emit_float_table_probe.txt)
__device__ __forceinline__ void hdp_load_coef(rsrc_t rs_coef, unsigned off16, u32x4 &a, u32x4 &b) {
    a = __builtin_amdgcn_raw_buffer_load_b128(rs_coef, off16 * 2u, 0, 0);
    b = __builtin_amdgcn_raw_buffer_load_b128(rs_coef, off16 * 2u + 16u, 0, 0);
}

#define EMIT_U 2        // diagonals in flight per wave
#define EMIT_WAVES 8    // waves per SIMD the register allocation is held to
#define EMIT_ATTR __attribute__((amdgpu_waves_per_eu(EMIT_WAVES, EMIT_WAVES)))
#define EMIT_HOT_MAX 256   // intervals of the hot row held in LDS (8 KB)
#define EMIT_XCAP 256   // reference positions of a tile whose constants are staged in LDS (+ 64 of slack for lanes beyond a diagonal)
#define EMIT_YCAP 320   // events of a tile staged in LDS (+ 64 on either side)
__global__ __launch_bounds__(256) EMIT_ATTR void k_emit_hdp(const sa_region_t *__restrict__ regions, const sa_row_t *__restrict__ rows_all,
                                                  const double4 *__restrict__ xc_all, const double *__restrict__ ev_all,
                                                  const double *__restrict__ hdp_tab, const double *__restrict__ hdp_coef,
                                                  double *__restrict__ E_all, FastT T, const int *__restrict__ region_ids) {
    __shared__ double2 LT[128];
    __shared__ double2 LX[EMIT_XCAP + 80];   // {e' offset, row offset} of reference position xlo + i
    __shared__ double4 LH[EMIT_HOT_MAX];     // the coefficients of the HOT row: the one most k-mers resolve to (see below)
    __shared__ double LE[EMIT_YCAP + 128];   // event of matrix row ylo - 64 + i (NaN where there is none)
    const sa_region_t *R = &regions[region_ids[blockIdx.y]];
    const int N = (int) R->N;
    const int d0 = (int) blockIdx.x * EMIT_TILE;
    if (d0 > N) return;
    const sa_row_t *rows = rows_all + R->row_off;
    double *E = E_all + R->f_base;
    const rsrc_t rs_xc = make_rsrc(xc_all + R->pid_off), rs_ev = make_rsrc(ev_all + R->ev_off), rs_E = make_rsrc(E);
    const rsrc_t rs_tab = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(hdp_tab), 0, (int) T.hdp_bytes, 0x00020000);
    const rsrc_t rs_coef = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(hdp_coef), 0, (int) (2u * T.hdp_bytes), 0x00020000);
    const double inv_var = 1.0 / R->var, lvar = R->lvar;
    if (threadIdx.x < 128) {
        double2 row = g_log_rows[threadIdx.x];
        row.y += lvar;
        LT[threadIdx.x] = row;
    }
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    if (blockIdx.x == 0 && threadIdx.x == 0) E[R->f_cellpaths - 1] = NEG_INF;   // what lanes without a cell read
    // The tile's 64 row records, lane q holding diagonal d0 + q (every wave loads them: the same 1 KB).  A cell moves 64 bytes
    // through the CU's texture-address path if it fetches its own constants (16 B), its event (8 B), its two table entries (32 B)
    // and stores 8 B -- and that path takes 64 B per clock: 3.4 ms per 5000 reads before anything is computed, where the kernel
    // measured 8.7 (without the table reads 6.5, without the stores 7.9, with neither 4.5: additive, one queue).  The constants and
    // the events of a tile are a few hundred entries that every diagonal of the tile reads again: they go to LDS once per workgroup
    // (its own path), which leaves 40 B per cell on the texture path.  A tile whose band does not fit the LDS arrays (a band that
    // jumps: never seen with anchors a chain apart) reads from memory as before.
    const int dq = d0 + lane;
    const sa_row_t rq = rows[dq <= N ? dq : N];
    const int rq_foff = (int) rq.foff;                 // register-kernel regions hold fewer than 2^27 cells
    int xlo, xhi, ylo, yhi;
    {
        const int dd = dq <= N ? dq : N;
        const int x0 = (dd + rq.xmyL) >> 1, xe = x0 + rq.width;   // cells x0 .. xe - 1, matrix rows dd - xe + 1 .. dd - x0
        xlo = x0; xhi = xe; ylo = dd - xe + 1; yhi = dd - x0;
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            xlo = min(xlo, __shfl_xor(xlo, m, 64)); xhi = max(xhi, __shfl_xor(xhi, m, 64));
            ylo = min(ylo, __shfl_xor(ylo, m, 64)); yhi = max(yhi, __shfl_xor(yhi, m, 64));
        }
        xlo = __builtin_amdgcn_readfirstlane(xlo); xhi = __builtin_amdgcn_readfirstlane(xhi);
        ylo = __builtin_amdgcn_readfirstlane(ylo); yhi = __builtin_amdgcn_readfirstlane(yhi);
    }
    const bool staged = xhi - xlo <= EMIT_XCAP && yhi - ylo < EMIT_YCAP && xlo >= 0;
    // The hot row.  A k-mer without data of its own takes the density of its first observed ancestor (impl/nanopore_hdp.c:420-429
    // through hdp_check_for_observed): in a model built from a limited number of reads most k-mers share ONE row -- the base
    // process's; in the bundled model 46 305 of 46 656.  That row's coefficients (grid_length x 32 B) go to LDS once per workgroup and
    // a cell whose k-mer resolves to it reads them there; the table in memory is read only by waves that hold another k-mer (a third
    // of them on the bundled model), for those lanes.  The values are the same doubles either way.
    const unsigned hot = T.hdp_hot;
    const int n_iv = (int) T.nm2 + 2;   // grid points
    const bool hot_on = hot != 0xffffffffu && n_iv <= EMIT_HOT_MAX;
    if (hot_on)
        for (int i = threadIdx.x; i < n_iv; i += 256) {
            u32x4 a, b;
            hdp_load_coef(rs_coef, hot + (unsigned) i * 16u, a, b);
            LH[i] = make_double4(__hiloint2double((int) a.y, (int) a.x), __hiloint2double((int) a.w, (int) a.z),
                                 __hiloint2double((int) b.y, (int) b.x), __hiloint2double((int) b.w, (int) b.z));
        }
    if (staged) {
        for (int i = threadIdx.x; i < xhi - xlo; i += 256) {
            const u32x4 c = __builtin_amdgcn_raw_buffer_load_b128(rs_xc, (unsigned) (xlo + i) * 32u, 0, 0);
            LX[i] = make_double2(__hiloint2double((int) c.y, (int) c.x), __hiloint2double((int) c.w, (int) c.z));
        }
        for (int i = threadIdx.x; i < yhi - ylo + 1 + 128; i += 256) {
            const int y = ylo - 64 + i;
            LE[i] = (y >= 1 && y <= yhi) ? buf_load_f64(rs_ev, (unsigned) (y - 1) * 8u, 0) : __builtin_nan("");
        }
    }
    __syncthreads();
    const double tc0 = -T.g0 * T.inv_dx;
    const int nm2 = (int) T.nm2;
    auto value = [&](double en, double tc, int il, unsigned off16, bool ok, const u32x4 &a, const u32x4 &b) -> double {
        return hdp_density_coef(en, tc, il, off16, ok, a, b, rs_tab, T);
    };
    // a cell beyond the first 64 of a wide diagonal, from memory
    auto cell = [&](int d, int x0, int i, unsigned fo8) {
        const int x = x0 + i, y = d - x;
        const bool ok = y >= 1;   // x == 0 is the NULL entry itself: its row offset lies beyond the table
        const u32x4 cw = __builtin_amdgcn_raw_buffer_load_b128(rs_xc, ok ? (unsigned) x * 32u : 0u, 0, 0);   // c.x, c.y
        const double e = buf_load_f64(rs_ev, ok ? (unsigned) (y - 1) * 8u : 0u, 0);
        const double cx = __hiloint2double((int) cw.y, (int) cw.x), cy = __hiloint2double((int) cw.w, (int) cw.z);
        const double en = fma(e, inv_var, -cx);
        const double tc = fma(en, T.inv_dx, tc0);
        const int il = max(0, min(cvt_i32_sat(tc), nm2));
        const unsigned off16 = cvt_u32_sat(cy) + (unsigned) il * 16u;
        u32x4 a, b;
        hdp_load_coef(rs_coef, off16, a, b);
        buf_store_f64(rs_E, (unsigned) i * 8u, fo8, log_tab(value(en, tc, il, off16, true, a, b), LT));
    };
    // EMIT_U diagonals in flight per wave: the chain of a cell is the table read behind the arithmetic on its event, and the reads of
    // independent diagonals are issued together.  Measured (5000 reads, same box): 4 in flight at 5 waves per SIMD (87 registers)
    // 8.1-8.4 ms, 2 in flight at 8 waves per SIMD (64 registers) 7.7-8.0, 8 in flight 10.1; an explicit ping-pong of two groups (the
    // next group's reads issued before this group's arithmetic) 8.5-9.1 -- reads and stores share one counter on this target, so a
    // wave that waits for its reads waits for everything it has in flight.  Chunks beyond the first 64 cells of a wide diagonal
    // follow one by one.
    // (`staged` and `hot_on` do not change inside a workgroup: the loop exists in its four flavours and the choice is made once --
    // tested per cell they were a dozen scalar instructions per diagonal of a kernel that is back at its instruction-issue bound)
    auto sweep = [&](auto staged_c, auto hot_c) {
        constexpr bool ST = decltype(staged_c)::value, HOT = decltype(hot_c)::value;
        for (int q0 = 0; q0 < EMIT_TILE / 4; q0 += EMIT_U) {
            if (d0 + w + 4 * q0 > N) break;
            int x0_[EMIT_U], wd_[EMIT_U], il_[EMIT_U];
            unsigned fo_[EMIT_U], off_[EMIT_U];
            bool ok_[EMIT_U];
            u32x4 a_[EMIT_U], b_[EMIT_U];
            double cx_[EMIT_U], cy_[EMIT_U], e_[EMIT_U], en_[EMIT_U], tc_[EMIT_U];
#pragma unroll
            for (int u = 0; u < EMIT_U; u++) {
                const int d = d0 + w + 4 * (q0 + u);
                const int xmyL = __builtin_amdgcn_readlane(rq.xmyL, w + 4 * (q0 + u));
                wd_[u] = d <= N ? __builtin_amdgcn_readlane(rq.width, w + 4 * (q0 + u)) : 0;
                fo_[u] = (unsigned) __builtin_amdgcn_readlane(rq_foff, w + 4 * (q0 + u)) * 8u;
                x0_[u] = (d + xmyL) >> 1;
                const int x = x0_[u] + lane, y = d - x;
                ok_[u] = y >= 1 && lane < wd_[u];
                if (ST) {   // (lanes beyond the diagonal read the slack of the arrays: values nobody stores)
                    const double2 c = LX[x - xlo];
                    cx_[u] = c.x; cy_[u] = c.y;
                    e_[u] = LE[y - ylo + 64];
                } else {
                    const u32x4 cw = __builtin_amdgcn_raw_buffer_load_b128(rs_xc, ok_[u] ? (unsigned) x * 32u : 0u, 0, 0);
                    cx_[u] = __hiloint2double((int) cw.y, (int) cw.x); cy_[u] = __hiloint2double((int) cw.w, (int) cw.z);
                    e_[u] = buf_load_f64(rs_ev, ok_[u] ? (unsigned) (y - 1) * 8u : 0u, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < EMIT_U; u++) {
                en_[u] = fma(e_[u], inv_var, -cx_[u]);
                tc_[u] = fma(en_[u], T.inv_dx, tc0);
                il_[u] = max(0, min(cvt_i32_sat(tc_[u]), nm2));
                const unsigned cyu = cvt_u32_sat(cy_[u]);
                off_[u] = cyu + (unsigned) il_[u] * 16u;
                if (HOT) {
                    const double4 hc = LH[il_[u]];
                    a_[u].x = (unsigned) __double2loint(hc.x); a_[u].y = (unsigned) __double2hiint(hc.x);
                    a_[u].z = (unsigned) __double2loint(hc.y); a_[u].w = (unsigned) __double2hiint(hc.y);
                    b_[u].x = (unsigned) __double2loint(hc.z); b_[u].y = (unsigned) __double2hiint(hc.z);
                    b_[u].z = (unsigned) __double2loint(hc.w); b_[u].w = (unsigned) __double2hiint(hc.w);
                    if (cyu != hot && ok_[u]) {   // a k-mer with a row of its own: only these lanes take part in the read (exec mask)
                        hdp_load_coef(rs_coef, off_[u], a_[u], b_[u]);
                    }
                    // (the read written as an instruction landing in the registers that hold the hot row's values -- the compiler
                    // merges the conditional load with eight selects per cell instead -- measured the same: 6.56 against 6.58 ms)
                } else {
                    hdp_load_coef(rs_coef, off_[u], a_[u], b_[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < EMIT_U; u++) {
                const double val = log_tab(value(en_[u], tc_[u], il_[u], off_[u], ok_[u], a_[u], b_[u]), LT);
                buf_store_f64(rs_E, lane < wd_[u] ? (unsigned) lane * 8u : 0xfffffff0u, fo_[u], val);   // (no cell: beyond the buffer)
            }
#pragma unroll
            for (int u = 0; u < EMIT_U; u++)
                for (int i = lane + 64; i < wd_[u]; i += 64) cell(d0 + w + 4 * (q0 + u), x0_[u], i, fo_[u]);
        }
    };
    if (staged && hot_on) sweep(std::true_type{}, std::true_type{});
    else if (staged) sweep(std::true_type{}, std::false_type{});
    else if (hot_on) sweep(std::false_type{}, std::true_type{});
    else sweep(std::false_type{}, std::false_type{});
}

// The same plane for SA_KIND_RING regions (ring and strip kernels, sa_ring.inc / sa_strip.inc): rows in PATH space -- a
// diagonal is the contiguous range [g0, g0 + np) of cell-paths, np from the next row's offset, rows[d].foff = (g0 << 32) | offset
// -- and one emission per cell-PATH (every path of a cell has its own k-mer: stateMachine3HDP_cellCalculate,
// impl/stateMachine.c:1371-1437, over hdCell_construct2's paths).  xc is indexed by the path-space index g; the column of a
// cell-path is g itself with one path per cell and the per-path record's x otherwise.  Value j of diagonal d at offset + j,
// entry C - 1 the -inf sentinel.  A wave takes a diagonal at a time, 64 cell-paths per step (not the four diagonals in flight of
// k_emit_hdp: these regions are the minority of an HDP batch).
template <bool MULTI>
__global__ __launch_bounds__(256) void k_emit_hdp_ring(const sa_region_t *__restrict__ regions, const sa_row_t *__restrict__ rows_all,
                                                       const sa_prec_t *__restrict__ prec_all, const double4 *__restrict__ xc_all,
                                                       const double *__restrict__ ev_all, const double *__restrict__ hdp_tab,
                                                       const double *__restrict__ hdp_coef, double *__restrict__ E_all, FastT T,
                                                       const int *__restrict__ region_ids) {
    __shared__ double2 LT[128];
    __shared__ double4 LH[EMIT_HOT_MAX];   // the hot row's coefficients (k_emit_hdp)
    const sa_region_t *R = &regions[region_ids[blockIdx.y]];
    const int N = (int) R->N;
    const int d0 = (int) blockIdx.x * EMIT_TILE;
    if (d0 > N) return;
    if (threadIdx.x < 128) {   // log_tab's rows, the emission's constant term added
        double2 row = g_log_rows[threadIdx.x];
        row.y += R->lvar;
        LT[threadIdx.x] = row;
    }
    const rsrc_t rs_coef = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(hdp_coef), 0, (int) (2u * T.hdp_bytes), 0x00020000);
    const unsigned hot = T.hdp_hot;
    const int n_iv = (int) T.nm2 + 2;
    const bool hot_on = hot != 0xffffffffu && n_iv <= EMIT_HOT_MAX;
    if (hot_on)
        for (int i = threadIdx.x; i < n_iv; i += 256) {
            u32x4 a, b;
            hdp_load_coef(rs_coef, hot + (unsigned) i * 16u, a, b);
            LH[i] = make_double4(__hiloint2double((int) a.y, (int) a.x), __hiloint2double((int) a.w, (int) a.z),
                                 __hiloint2double((int) b.y, (int) b.x), __hiloint2double((int) b.w, (int) b.z));
        }
    __syncthreads();
    const double tc0 = -T.g0 * T.inv_dx;
    const int nm2 = (int) T.nm2;
    const int4 *rows4 = reinterpret_cast<const int4 *>(rows_all + R->row_off);
    double *E = E_all + R->f_base;
    const rsrc_t rs_xc = make_rsrc(xc_all + R->pid_off), rs_ev = make_rsrc(ev_all + R->ev_off), rs_E = make_rsrc(E);
    const rsrc_t rs_tab = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(hdp_tab), 0, (int) T.hdp_bytes, 0x00020000);
    const rsrc_t rs_pr = make_rsrc(MULTI ? (const void *) (prec_all + R->pid_off) : (const void *) rows_all);
    const double inv_var = 1.0 / R->var;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const unsigned OOB = 0xfffffff0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) E[R->f_cellpaths - 1] = NEG_INF;   // what lanes without a cell-path read
    // The chain of a cell-path is two (three with per-path records) dependent memory round trips: a wave keeps four independent
    // ones in flight -- 128 cell-paths of each of two diagonals (d and d + 4) per step.  A unit without a cell-path asks beyond
    // its buffers (loads return zeros, the store is dropped): no exec-masked branch around a memory access.
    auto sweep = [&](auto hot_c) {   // (with and without a hot row: fixed per workgroup, chosen once -- see k_emit_hdp)
        constexpr bool HOT = decltype(hot_c)::value;
        for (int d = d0 + w; d < d0 + EMIT_TILE && d <= N; d += 8) {
            const int dB = d + 4;
            const bool hasB = dB < d0 + EMIT_TILE && dB <= N;
            const int4 rA = rows4[d], rAn = rows4[d + 1];   // (row N + 1 is the sentinel that closes the last diagonal)
            const int4 rB = rows4[hasB ? dB : d], rBn = rows4[hasB ? dB + 1 : d + 1];
            const int npA = rAn.z - rA.z, npB = hasB ? rBn.z - rB.z : 0;
            const int npm = npA > npB ? npA : npB;
            for (int j0 = 0; j0 < npm; j0 += 128) {
                int g_[4], dd_[4], x_[4], il_[4];
                unsigned st_[4], fo_[4];
                bool ok_[4];
                u32x4 cw_[4], a_[4], b_[4];
                unsigned off_[4];
                double e_[4], en_[4], tc_[4];
    #pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int j = j0 + lane + 64 * (u & 1);
                    const bool second = u >= 2;
                    const int np = second ? npB : npA;
                    const bool in = j < np;
                    g_[u] = (second ? rB.w : rA.w) + j;
                    dd_[u] = second ? dB : d;
                    fo_[u] = (unsigned) (second ? rB.z : rA.z) * 8u;
                    st_[u] = in ? (unsigned) j * 8u : OOB;
                    ok_[u] = in;
                    x_[u] = g_[u];
                    if (MULTI) x_[u] = (int) __builtin_amdgcn_raw_buffer_load_b32(rs_pr, in ? (unsigned) g_[u] * 16u : OOB, 0, 0);   // sa_prec_t.x
                }
    #pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int y = dd_[u] - x_[u];
                    ok_[u] = ok_[u] && y >= 1;   // (x == 0 is the NULL entry: its row offset lies beyond the table)
                    cw_[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_xc, ok_[u] ? (unsigned) g_[u] * 32u : 0u, 0, 0);
                    e_[u] = buf_load_f64(rs_ev, ok_[u] ? (unsigned) (y - 1) * 8u : 0u, 0);
                }
    #pragma unroll
                for (int u = 0; u < 4; u++) {
                    const double cx = __hiloint2double((int) cw_[u].y, (int) cw_[u].x), cy = __hiloint2double((int) cw_[u].w, (int) cw_[u].z);
                    en_[u] = fma(e_[u], inv_var, -cx);
                    tc_[u] = fma(en_[u], T.inv_dx, tc0);
                    il_[u] = max(0, min(cvt_i32_sat(tc_[u]), nm2));
                    const unsigned cyu = cvt_u32_sat(cy);   // (a unit without a cell-path converts zeros or whatever slot 0 holds: as k_emit_hdp)
                    off_[u] = cyu + (unsigned) il_[u] * 16u;
                    a_[u] = u32x4{0u, 0u, 0u, 0u}; b_[u] = a_[u];   // (no cell-path: zeros, as a read beyond the table gives)
                    if (HOT) {
                        const double4 hc = LH[il_[u]];
                        a_[u].x = (unsigned) __double2loint(hc.x); a_[u].y = (unsigned) __double2hiint(hc.x);
                        a_[u].z = (unsigned) __double2loint(hc.y); a_[u].w = (unsigned) __double2hiint(hc.y);
                        b_[u].x = (unsigned) __double2loint(hc.z); b_[u].y = (unsigned) __double2hiint(hc.z);
                        b_[u].z = (unsigned) __double2loint(hc.w); b_[u].w = (unsigned) __double2hiint(hc.w);
                    }
                    if (ok_[u] && !(HOT && cyu == hot)) {   // a row of its own: these lanes only
                        hdp_load_coef(rs_coef, off_[u], a_[u], b_[u]);
                    }
                }
    #pragma unroll
                for (int u = 0; u < 4; u++)
                    buf_store_f64(rs_E, st_[u], fo_[u], log_tab(hdp_density_coef(en_[u], tc_[u], il_[u], off_[u], ok_[u], a_[u], b_[u], rs_tab, T), LT));
            }
        }
    };
    if (hot_on) sweep(std::true_type{});
    else sweep(std::false_type{});
}

// (Measured and dropped: the same plane filled column by column -- one wave per reference position, a lane per cell of the
// column, so that all lanes gather from ONE row of the table and the gathers hit L1.  The emissions of a column lie on
// consecutive diagonals, i.e. a scattered 8-byte store per lane: 16.3 ms per 5000 reads with plain stores, 88 ms with the
// streaming kind, against 10.7 ms for the diagonal-wise kernel above, whose stores are coalesced.)

// HDP: `e` IS the emission (read from the plane k_emit_hdp filled), match and gapY alike
template <bool HDP>
__device__ __forceinline__ void emit_fast(const double4 &c, double e, double &lM, double &lY) {
    if (HDP) { lM = e; lY = e; }
    else emit_gauss(c, e, lM, lY);
}

// ---------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------
template <bool HDP, bool TWO = false>
__device__ __forceinline__ void fwd_fast_body(const sa_region_t *__restrict__ regions,
                                              const sa_row_t *__restrict__ rows_all, const int *__restrict__ pk_all,
                                              const double4 *__restrict__ xc_all, const double *__restrict__ ev_all,
                                              double *__restrict__ F_all, const double *__restrict__ E_all, FastT T,
                                              const int *__restrict__ region_ids, int n, const sa_seg_t *__restrict__ segs_all) {
    __shared__ __attribute__((aligned(32))) double LT[LA_TAB_DOUBLES];
    __shared__ __attribute__((aligned(32))) double LS[LA_SITES * LA_TAB_DOUBLES];
    extern __shared__ __attribute__((aligned(32))) double fast_dyn[];   // T.wide_cap > 0: per wave 3 rows x 3 planes x wide_cap
    const LaSiteK SK = la_sites_fwd(T);
    la_tab_init(LT, threadIdx.x);
    la_tab_init_site(LS, threadIdx.x, SK.k0);
    la_tab_init_site(LS + LA_TAB_DOUBLES, threadIdx.x, SK.k1);
    la_tab_init_site(LS + 2 * LA_TAB_DOUBLES, threadIdx.x, SK.k2);
    la_tab_init_site(LS + 3 * LA_TAB_DOUBLES, threadIdx.x, SK.k3);
    __syncthreads();
    int wv = __builtin_amdgcn_readfirstlane((int) ((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wv >= n) return;
    const int lane = threadIdx.x & 63;
    // Wide diagonals (more than 64 lanes in the three-diagonal window: anchors as sparse as a real guide alignment
    // leaves them make this the rule, not the exception) cannot live in registers.  Their last three rows sit in an LDS
    // ring of this wave; the forward storage is still written for the backward pass but no longer read back, which took
    // a store -> fence -> load round trip through L2 per diagonal.
    const int wcap = T.wide_cap;
    double *const wring = fast_dyn + (size_t) (threadIdx.x >> 6) * 9 * (size_t) wcap;
    int held0 = -1, held1 = -1, held2 = -1;   // diagonal held by ring slot 0, 1, 2 (slot = diagonal % 3)
    const sa_region_t *R = &regions[__builtin_amdgcn_readfirstlane(region_ids[wv])];
    const sa_row_t *rows = rows_all + R->row_off;
    const int *pk = pk_all + R->pk_off + SA_PK_PAD;
    const double4 *xc = xc_all + R->pid_off;  // entry x <-> matrix column x
    const double *ev = ev_all + R->ev_off;
    // forward storage of a register-kernel region: three planes [match | gapX | gapY], each C cells, a diagonal's
    // cells at [foff, foff+width).  The match plane is written for every diagonal (one sequential stream per wave);
    // the gap planes only where they are read back (SA_PK_FULL).  Cell C-1 of the match plane is a -inf sentinel.
    double *F = F_all + 3 * R->f_base;
    const long long C = R->f_cellpaths;
    const int K = R->K;
    const int N = (int) R->N;
    const double cx_m = SA_LOG_GAPX + T.t_mx, cx_x = SA_LOG_GAPX + T.t_xx;
    const rsrc_t rs_xc = make_rsrc(xc), rs_ev = make_rsrc(ev), rs_F = make_rsrc(F);
    const unsigned C8 = (unsigned) C * 8u;
    const double *Eg = HDP ? E_all + R->f_base : nullptr;   // HDP: the region's emission plane (k_emit_hdp)
    const rsrc_t rs_E = make_rsrc(HDP ? Eg : ev);
    const unsigned sentinel8 = C8 - 8u;
    // two-distribution emission: the events' and the positions' noise constants (FastT.two_xn_off)
    const double4 *en3 = TWO ? reinterpret_cast<const double4 *>(E_all) + R->ev_off : nullptr;
    const double4 *xn = TWO ? reinterpret_cast<const double4 *>(E_all) + T.two_xn_off + R->pid_off : nullptr;
    const rsrc_t rs_en = make_rsrc(TWO ? (const void *) en3 : (const void *) ev), rs_xn = make_rsrc(TWO ? (const void *) xn : (const void *) ev);

    {   // diagonal 0 and the sentinel
        sa_row_t r0 = rows[0];
        double s0 = R->ragged_l ? NEG_INF : 0.0, s1 = R->ragged_l ? 0.0 : NEG_INF;
        for (int i = lane; i < r0.width; i += 64) {
            F[r0.foff + i] = s0;
            F[C + r0.foff + i] = s1;
            F[2 * C + r0.foff + i] = s1;
        }
        if (lane == 0) F[C - 1] = NEG_INF;
    }
    // (the diagonals the region's tracebacks start on carry SA_PK_FULL too -- the planners set it -- and keep all three planes:
    // k_spec_match, sa_hip.hip, takes each traceback's total there as the backward sweep's candidate bound)
    int d = 1;
    while (d <= N) {
        if ((pk[d] & SA_PK_FWD) && (d & 3) == 0) {
            // ---- register-resident section: starts on a multiple of 4 (the loop below is unrolled over four diagonals;
            // up to three diagonals in front of it take the memory-resident path), runs until a diagonal does not fit
            // or the matrix ends ----
            wave_fence();
            held0 = held1 = held2 = -1;   // the ring goes stale while the registers hold the band
            // oM of the last even / odd diagonal (a diagonal reads the slot of its own parity: written two steps ago)
            double oMe, oMo, oX, oY;  // oX/oY: published by diagonal d-1
            {
                const sa_row_t r1 = rows[d - 1];
                int t1 = (lane - ((r1.xmyL + K) >> 1)) & 63;
                bool a1 = t1 < r1.width;
                const double *p1 = F + r1.foff + t1;
                double m = a1 ? p1[0] : NEG_INF, x = a1 ? p1[C] : NEG_INF, y = a1 ? p1[2 * C] : NEG_INF;
                double o1 = la_fast(LT, la_fast(LT, m + T.t_mm, x + T.t_xm), y + T.t_ym);
                oX = la_fast(LT, m + cx_m, x + cx_x);
                oY = la_fast(LT, m + T.t_my, y + T.t_yy);
                double o2 = NEG_INF;
                if (d >= 2) {
                    const sa_row_t r2 = rows[d - 2];
                    int t2 = (lane - ((r2.xmyL + K) >> 1)) & 63;
                    bool a2 = t2 < r2.width;
                    const double *p2 = F + r2.foff + t2;
                    double m2 = a2 ? p2[0] : NEG_INF, x2 = a2 ? p2[C] : NEG_INF, y2 = a2 ? p2[2 * C] : NEG_INF;
                    o2 = la_fast(LT, la_fast(LT, m2 + T.t_mm, x2 + T.t_xm), y2 + T.t_ym);
                }
                oMe = (d & 1) ? o1 : o2;  // d odd: d-1 is even
                oMo = (d & 1) ? o2 : o1;
            }
            unsigned fo8 = (unsigned) rows[d].foff * 8u;  // byte offset of the diagonal; advanced by every finished one
            // 64 packed words from the 32-aligned diagonal at or below d: diagonals d, d+1 are lanes (d&31), (d&31)+1
            // pkv: 64 words in use; pkn: the 32 that move in at the next multiple of 32.  The hand-over happens between
            // pairs, outside the inner loop: inside it the request would sit in a branch and drag a vmcnt(0) along.
            int pkv = pk[(d & ~31) + lane];
            int pkn = pk[(d & ~31) + 32 + lane];
            int pc = __builtin_amdgcn_readlane(pkv, d & 31);

            // one diagonal of static parity: `cur` was requested one step earlier; the oM slot that is read (written two
            // diagonals ago) is overwritten with this diagonal's own oM
            double pend_m = NEG_INF;                 // match value of the previous diagonal, not stored yet
            unsigned pend_vo = 0xfffffff0u, pend_so = 0;  // out-of-range offset: nothing pending
            unsigned fo8_2 = 0;                           // HDP: byte offset of diagonal d + 2 (the one being requested)
            auto step = [&](auto odd, double lM, double lY_, int cur_t, bool cur_act, int pw, double &oM2) {
                double in_x, in_y;
                if (!decltype(odd)::value) {  // lower from lane-1, upper own
                    in_x = from_lane_below(oX);
                    in_y = oY;
                } else {                      // lower own, upper from lane+1
                    in_x = oX;
                    in_y = from_lane_above(oY);
                }
                const double m = oM2 + lM;                 // -inf outside the band (NULL entry)
                const double x = cur_act ? in_x : NEG_INF;
                const double y = in_y + lY_;               // -inf outside the band
                // lanes without a cell get an offset beyond num_records: the buffer range check drops their store, so the
                // loop body has no exec-masked branch (a branch makes the compiler fall back to s_waitcnt vmcnt(0))
                const unsigned vo = cur_act ? (unsigned) cur_t * 8u : 0xfffffff0u;
                pend_m = m; pend_vo = vo; pend_so = fo8;  // stored by the next half (or after the loop)
                if (pw & SA_PK_FULL) {
                    buf_store_f64(rs_F, vo, fo8 + C8, x);
                    buf_store_f64(rs_F, vo, fo8 + 2u * C8, y);
                }
                LaP pm, px, py;
                la_prep(pm, m, x + SK.a0);
                la_prep(px, m, x + SK.a1);
                la_prep(py, m, y + SK.a2);
                la_fetch(pm, LS);
                la_fetch(px, LS + LA_TAB_DOUBLES);
                la_fetch(py, LS + 2 * LA_TAB_DOUBLES);
                __builtin_amdgcn_sched_barrier(0);  // keep the three LDS reads in flight together
                la_wait();
                const double om1 = la_finish(pm);
                oX = la_finish(px);
                oY = la_finish(py);
                LaP pq;
                la_prep(pq, om1, y);
                la_fetch(pq, LS + 3 * LA_TAB_DOUBLES);
                la_wait();
                oM2 = la_finish(pq);
            };
            // one half of the unrolled pair: request the next diagonal's inputs, then issue the PREVIOUS diagonal's
            // match store, then compute this diagonal.  vmcnt retires in order, so waiting for a load also waits for
            // every older store; a store issued just before a request costs the wave the store's latency one diagonal
            // later (+150 ns per diagonal, probes/store_probe.hip).  Issued right after the request it is younger than
            // the loads that are waited for, and has two diagonals to complete.  Returns whether the section continues.
            // `nxt2` receives the request for diagonal d+2: inputs are requested TWO diagonals ahead (a new cache line of
            // position constants or events comes from HBM and takes longer than one diagonal), into one of four stages so
            // that no stage is read and refilled in the same half
            auto half = [&](auto odd, const Stage &cur, Stage &nxt2, double &oM2) -> bool {
                const int li = d & 31;
                const int pn = __builtin_amdgcn_readlane(pkv, li + 1);
                const int pn2 = __builtin_amdgcn_readlane(pkv, li + 2);
                if (HDP) {
                    nxt2 = stage_inputs_plane(pn2, d + 2, K, lane, rs_E, fo8_2, sentinel8);
                    fo8_2 += pk_row_bytes(pn2);
                } else {
                    nxt2 = TWO ? stage_inputs_two(pn2, d + 2, K, lane, rs_xc, rs_ev, rs_xn, rs_en)
                               : stage_inputs(pn2, d + 2, K, lane, rs_xc, rs_ev);  // harmless past the end (zero words: no cell)
                }
                buf_store_f64(rs_F, pend_vo, pend_so, pend_m);
                double lM, lY_;
                emit_fast<HDP>(cur.c, cur.e, lM, lY_);
                if (TWO) emit_two(cur.cn, cur.n3, lM, lY_);
                step(odd, lM, lY_, cur.t, cur.act, pc, oM2);
                const bool more = (pc & SA_PK_FWD_MORE) != 0;
                fo8 += pk_row_bytes(pc);
                d++;
                pc = pn;
                return more;
            };
            auto next_tile = [&]() {  // d is a multiple of 32
                pkv = pkn;
                pkn = pk[d + 32 + lane];
            };
            const std::integral_constant<bool, false> EVEN;
            const std::integral_constant<bool, true> ODD;
            Stage S0, S1, S2, S3;
            if (HDP) {
                const int p1 = __builtin_amdgcn_readlane(pkv, (d & 31) + 1);
                S0 = stage_inputs_plane(pc, d, K, lane, rs_E, fo8, sentinel8);
                S1 = stage_inputs_plane(p1, d + 1, K, lane, rs_E, fo8 + pk_row_bytes(pc), sentinel8);
                fo8_2 = fo8 + pk_row_bytes(pc) + pk_row_bytes(p1);
            } else {
                if (TWO) {
                    S0 = stage_inputs_two(pc, d, K, lane, rs_xc, rs_ev, rs_xn, rs_en);
                    S1 = stage_inputs_two(__builtin_amdgcn_readlane(pkv, (d & 31) + 1), d + 1, K, lane, rs_xc, rs_ev, rs_xn, rs_en);
                } else {
                S0 = stage_inputs(pc, d, K, lane, rs_xc, rs_ev);                                               // d % 4 == 0
                S1 = stage_inputs(__builtin_amdgcn_readlane(pkv, (d & 31) + 1), d + 1, K, lane, rs_xc, rs_ev);  // == 1
                }
            }
            bool more = true;
            while (more) {
                do {
                    more = false;
                    if (!half(EVEN, S0, S2, oMe)) break;
                    if (!half(ODD, S1, S3, oMo)) break;
                    if (!half(EVEN, S2, S0, oMe)) break;
                    more = half(ODD, S3, S1, oMo);
                } while (more && (d & 31) != 0);
                if (more) next_tile();
            }
            buf_store_f64(rs_F, pend_vo, pend_so, pend_m);  // the last diagonal of the section
        } else {
            // ---- memory-resident path: any width (all three planes of every diagonal) ----
            const sa_row_t rd = rows[d];
            const sa_row_t r1 = rows[d - 1];
            sa_row_t r2 = {0, 0, 0};
            if (d >= 2) r2 = rows[d - 2];
            const int x0 = (d + rd.xmyL) >> 1;
            const int s0 = d % 3, s1 = (d + 2) % 3, s2 = (d + 1) % 3;   // ring slots of d, d-1, d-2
            if (wcap > 0 && rd.width <= wcap && r1.width <= wcap && r2.width <= wcap) {
                // rows d-1 and d-2 from the LDS ring (filled from the forward storage when a wide stretch begins)
                const int h1 = s1 == 0 ? held0 : (s1 == 1 ? held1 : held2), h2 = s2 == 0 ? held0 : (s2 == 1 ? held1 : held2);
                const bool need1 = h1 != d - 1, need2 = d >= 2 && h2 != d - 2;
                if (need1 || need2) {
                    wave_fence();
                    if (need1) {
                        double *L = wring + s1 * 3 * wcap;
                        for (int i = lane; i < r1.width; i += 64) {
                            L[i] = F[r1.foff + i]; L[wcap + i] = F[C + r1.foff + i]; L[2 * wcap + i] = F[2 * C + r1.foff + i];
                        }
                    }
                    if (need2) {
                        double *L = wring + s2 * 3 * wcap;
                        for (int i = lane; i < r2.width; i += 64) {
                            L[i] = F[r2.foff + i]; L[wcap + i] = F[C + r2.foff + i]; L[2 * wcap + i] = F[2 * C + r2.foff + i];
                        }
                    }
                }
                const double *L1 = wring + s1 * 3 * wcap, *L2 = wring + s2 * 3 * wcap;
                double *L0 = wring + s0 * 3 * wcap;
                // the inputs of all (at most four) 64-cell chunks of the diagonal are requested before the first chunk is
                // computed: one memory latency per diagonal instead of one per chunk
                double4 cq[4];
                double eq[4];
                double4 cnq[4], n3q[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = lane + 64 * q;
                    const int x = x0 + i, y = d - x;
                    const bool in = i < rd.width;
                    if (HDP) {
                        eq[q] = in ? Eg[rd.foff + i] : NEG_INF;
                    } else {
                        cq[q] = xc[in && y >= 1 ? x : 0];
                        eq[q] = ev[in && y >= 1 ? y - 1 : 0];
                        if (TWO) { cnq[q] = xn[in && y >= 1 ? x : 0]; n3q[q] = en3[in && y >= 1 ? y - 1 : 0]; }
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = lane + 64 * q;
                    if (i >= rd.width) break;
                    int xmy = rd.xmyL + 2 * i;
                    double lM, lY_;
                    emit_fast<HDP>(cq[q], eq[q], lM, lY_);
                    if (TWO) emit_two(cnq[q], n3q[q], lM, lY_);
                    int ilo = xmy - 1 - r1.xmyL, iup = xmy + 1 - r1.xmyL, imid = xmy - r2.xmyL;
                    bool hlo = ilo >= 0 && (ilo >> 1) < r1.width;
                    bool hup = iup >= 0 && (iup >> 1) < r1.width;
                    bool hmid = d >= 2 && imid >= 0 && (imid >> 1) < r2.width;
                    ilo >>= 1; iup >>= 1; imid >>= 1;
                    double lom = hlo ? L1[ilo] : NEG_INF, lox = hlo ? L1[wcap + ilo] : NEG_INF;
                    double upm = hup ? L1[iup] : NEG_INF, upy = hup ? L1[2 * wcap + iup] : NEG_INF;
                    double mm = hmid ? L2[imid] : NEG_INF, mx = hmid ? L2[wcap + imid] : NEG_INF,
                           my = hmid ? L2[2 * wcap + imid] : NEG_INF;
                    double sm = la_fast(LT, la_fast(LT, mm + T.t_mm, mx + T.t_xm), my + T.t_ym) + lM;
                    double sx = la_fast(LT, lom + cx_m, lox + cx_x);
                    double sy = la_fast(LT, upm + T.t_my, upy + T.t_yy) + lY_;
                    double *o = F + rd.foff + i;
                    o[0] = sm;
                    o[C] = sx;
                    o[2 * C] = sy;
                    L0[i] = sm; L0[wcap + i] = sx; L0[2 * wcap + i] = sy;
                }
                if (s0 == 0) held0 = d; else if (s0 == 1) held1 = d; else held2 = d;
            } else {
                // wider than the ring (or no ring): state rows are read back from the forward storage
                wave_fence();
                if (s0 == 0) held0 = -1; else if (s0 == 1) held1 = -1; else held2 = -1;
                const double *F1 = F + r1.foff, *F2 = F + r2.foff;
                for (int i = lane; i < rd.width; i += 64) {
                    int xmy = rd.xmyL + 2 * i;
                    int x = x0 + i, y = d - x;
                    double4 c;
                    double e;
                    if (HDP) {
                        e = Eg[rd.foff + i];
                    } else {
                        c = xc[y >= 1 ? x : 0];
                        e = ev[y >= 1 ? y - 1 : 0];
                    }
                    double lM, lY_;
                    emit_fast<HDP>(c, e, lM, lY_);
                    if (TWO) emit_two(xn[y >= 1 ? x : 0], en3[y >= 1 ? y - 1 : 0], lM, lY_);
                    int ilo = xmy - 1 - r1.xmyL, iup = xmy + 1 - r1.xmyL, imid = xmy - r2.xmyL;
                    bool hlo = ilo >= 0 && (ilo >> 1) < r1.width;
                    bool hup = iup >= 0 && (iup >> 1) < r1.width;
                    bool hmid = d >= 2 && imid >= 0 && (imid >> 1) < r2.width;
                    ilo >>= 1; iup >>= 1; imid >>= 1;
                    double lom = hlo ? F1[ilo] : NEG_INF, lox = hlo ? F1[C + ilo] : NEG_INF;
                    double upm = hup ? F1[iup] : NEG_INF, upy = hup ? F1[2 * C + iup] : NEG_INF;
                    double mm = hmid ? F2[imid] : NEG_INF, mx = hmid ? F2[C + imid] : NEG_INF,
                           my = hmid ? F2[2 * C + imid] : NEG_INF;
                    double sm = la_fast(LT, la_fast(LT, mm + T.t_mm, mx + T.t_xm), my + T.t_ym) + lM;
                    double sx = la_fast(LT, lom + cx_m, lox + cx_x);
                    double sy = la_fast(LT, upm + T.t_my, upy + T.t_yy) + lY_;
                    double *o = F + rd.foff + i;
                    o[0] = sm;
                    o[C] = sx;
                    o[2 * C] = sy;
                }
            }
            d++;
        }
    }
}

__global__ __launch_bounds__(64 * FAST_WAVES) void k_fwd_fast(const sa_region_t *__restrict__ regions,
                                                              const sa_row_t *__restrict__ rows_all,
                                                              const int *__restrict__ pk_all,
                                                              const double4 *__restrict__ xc_all,
                                                              const double *__restrict__ ev_all, double *__restrict__ F_all,
                                                              FastT T, const int *__restrict__ region_ids, int n,
                                                              const sa_seg_t *__restrict__ segs_all) {
    fwd_fast_body<false>(regions, rows_all, pk_all, xc_all, ev_all, F_all, nullptr, T, region_ids, n, segs_all);
}
__global__ __launch_bounds__(64 * FAST_WAVES) void k_fwd_fast_hdp(
    const sa_region_t *__restrict__ regions, const sa_row_t *__restrict__ rows_all, const int *__restrict__ pk_all,
    const double4 *__restrict__ xc_all, const double *__restrict__ ev_all, double *__restrict__ F_all,
    const double *__restrict__ E_all, FastT T, const int *__restrict__ region_ids, int n, const sa_seg_t *__restrict__ segs_all) {
    fwd_fast_body<true>(regions, rows_all, pk_all, xc_all, ev_all, F_all, E_all, T, region_ids, n, segs_all);
}
// Gaussian on the level x inverse Gaussian on the event's noise (SA_EMISSION_TWO_DIST / _SCALED_MODEL: what getStateMachine3 installs and
// every known answer the reference holds was produced with); N_all: the noise constants (FastT.two_xn_off).  Round 6: the reference's
// literal 14 / 7 matrices and its whole-read 1076 come out of these kernels (tests/test_gpu_reference_kats.py).
__global__ __launch_bounds__(64 * FAST_WAVES) void k_fwd_fast_two(
    const sa_region_t *__restrict__ regions, const sa_row_t *__restrict__ rows_all, const int *__restrict__ pk_all,
    const double4 *__restrict__ xc_all, const double *__restrict__ ev_all, double *__restrict__ F_all,
    const double *__restrict__ N_all, FastT T, const int *__restrict__ region_ids, int n, const sa_seg_t *__restrict__ segs_all) {
    fwd_fast_body<false, true>(regions, rows_all, pk_all, xc_all, ev_all, F_all, N_all, T, region_ids, n, segs_all);
}

// A tighter lower bound of a checkpoint's total than the largest of its terms, for posteriors that are flat across the band
// (HDP densities as broad as the bundled model's: fifty terms of equal size, the maximum is log 50 below the total and every
// band cell became a candidate -- 51 per diagonal where 0.1 pairs survive).  If n terms lie within t of the maximum, the
// total is at least max + log n - t; the reference's own fold of n equal terms falls short of log n by 7.4e-4 at most
// (n <= 64, measured over its cubic pieces), 0.05 covers it with room.  d = max - term per lane (NaN or +inf where there is
// no term); returns the gain over the maximum, >= 0.  Three ballots and a v_log_f32 each, once per ten diagonals.
__device__ __forceinline__ double tight_bound_gain(double d) {
    const float n1 = (float) __popcll(__ballot(d <= 0.25)), n2 = (float) __popcll(__ballot(d <= 0.7)),
                n3 = (float) __popcll(__ballot(d <= 2.0));
    float g = fmaxf(fmaxf(__logf(n1) - 0.25f, __logf(n2) - 0.7f), __logf(n3) - 2.0f) - 0.05f;
    return (double) fmaxf(g, 0.0f);   // (no term at all: log 0 = -inf -> 0)
}

// the same over two terms per lane (the strip kernels hold a diagonal's first 128 cells in two registers)
__device__ __forceinline__ double tight_bound_gain2(double d0, double d1) {
    const float n1 = (float) (__popcll(__ballot(d0 <= 0.25)) + __popcll(__ballot(d1 <= 0.25))),
                n2 = (float) (__popcll(__ballot(d0 <= 0.7)) + __popcll(__ballot(d1 <= 0.7))),
                n3 = (float) (__popcll(__ballot(d0 <= 2.0)) + __popcll(__ballot(d1 <= 2.0)));
    float g = fmaxf(fmaxf(__logf(n1) - 0.25f, __logf(n2) - 0.7f), __logf(n3) - 2.0f) - 0.05f;
    return (double) fmaxf(g, 0.0f);
}

// ---------------------------------------------------------------------------------------------------
// backward + posterior numerators + checkpoint terms.
// Each finished backward cell C publishes three messages (its value plus the emission it carries):
//     mM = C.match + eM(C)   consumed two diagonals later by (x-1,y-1), same lane
//     mY = C.gapY  + eY(C)   consumed next diagonal by (x, y-1)
//     mX = C.gapX  + log 0.1 consumed next diagonal by (x-1, y)
// A target adds the transition and gathers mid, up, low in that order (the reference's scatter order).
// Ring rows (memory-resident path and hand-over): [mM | mY | mX | b.match][rowcap]; b.match only for the cells the
// candidate sweep reads back (chunks beyond the second of a wide diagonal).
// ---------------------------------------------------------------------------------------------------
// EXPECT: the expectation pass (getExpectationsUsingAnchors; diagonalCalculation_Expectations impl/pairwiseAligner.c:1423-1443,
// cell_signal_updateExpectations[AndAssignments] :914-968) instead of the posterior candidates.  For every cell of a posterior
// diagonal e and every live transition into it the reference adds exp(F[from] + B[to] + (eP + tP) - total), F from the cell's
// lower / upper neighbour on e-1 and its middle neighbour on e-2.  B[to] + eP is exactly the message the backward sweep
// publishes for the cell (mX, mM, mY below), so a term is forward STATE + transition + backward MESSAGE: the forward sweep
// stores all three planes of every diagonal for such a batch (SA_PK_FULL everywhere), a lane keeps the three states of "its"
// cell on e-1 and e-2 in registers (sets named by the parity of their diagonal, like the oM slots) and fetches lower / upper
// with the DPP rotate of the forward sweep.  Sums are kept per lane, scaled by the checkpoint group's maximum, and flushed per
// group (gsum / gmc) as k_bwd_generic<EXPECT> does; sa_expect_batch rescales them with the exact totals.  HDP: the transitions
// into the match state whose probability may reach the threshold are listed as candidates in the reference's order.
struct ExpAcc {
    double a0, a1, a2, a3, a4, a5, a6;
};
__device__ __forceinline__ void exp_flush(double *__restrict__ gsum, double *__restrict__ gmc, long long ck, double Mc, ExpAcc &A,
                                          int lane) {
    double v[7] = {A.a0, A.a1, A.a2, A.a3, A.a4, A.a5, A.a6};
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const double s = wave_sum(v[k]);
        if (lane == 0) gsum[ck * 8 + k] = s;
    }
    if (lane == 0) { gsum[ck * 8 + 7] = 0.0; gmc[ck] = Mc; }
    A.a0 = A.a1 = A.a2 = A.a3 = A.a4 = A.a5 = A.a6 = 0.0;
}

template <bool HDP, bool EXPECT, bool TWO = false>
__device__ __forceinline__ void bwd_fast_body(
    const sa_region_t *__restrict__ regions, const sa_seg_t *__restrict__ segs, const sa_row_t *__restrict__ rows_all,
    const int *__restrict__ pk_all, const sa_ck_t *__restrict__ cks, const double4 *__restrict__ xc_all,
    const double *__restrict__ ev_all, const double *__restrict__ F_all, double *__restrict__ vbuf,
    sa_cand_t *__restrict__ cands, int *__restrict__ cand_count, int *__restrict__ overflow,
    double *__restrict__ bscratch, const double *__restrict__ E_all, FastT T, const int *__restrict__ seg_ids, int n,
    double *__restrict__ gsum = nullptr, double *__restrict__ gmc = nullptr) {
    __shared__ __attribute__((aligned(32))) double LT[LA_TAB_DOUBLES];
    la_tab_init(LT, threadIdx.x);
    __syncthreads();
    int wv = __builtin_amdgcn_readfirstlane((int) ((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wv >= n) return;
    const int lane = threadIdx.x & 63;
    const int seg = __builtin_amdgcn_readfirstlane(seg_ids[wv]);
    const sa_seg_t *S = &segs[seg];
    const sa_region_t *R = &regions[S->region];
    const sa_row_t *rows = rows_all + R->row_off;
    const int *pk = pk_all + R->pk_off + SA_PK_PAD;
    const double4 *xc = xc_all + R->pid_off;
    const double *ev = ev_all + R->ev_off;
    const double *F = F_all + 3 * R->f_base;  // planes [match | gapX | gapY] of C cells each (see k_fwd_fast)
    const long long C = R->f_cellpaths;
    const int K = R->K;
    const int start = (int) S->start, from = (int) S->from, to = (int) S->to;
    // ring geometry and end-state values are needed outside the register sections only: re-derived on use instead of
    // being carried in SGPRs across the hot loop (the kernel is short of them: it spills scalars to vector lanes)
#define rowcap ((long long) R->max_rowpaths)
#define ring (bscratch + S->bscratch_off)
    sa_cand_t *my_cands = cands + S->cand_off;
    const int cand_cap = S->cand_cap;
    const long long ck_base = S->ck_base;
    int count = 0;
    double Mc = NEG_INF;     // max per-cell term of the current checkpoint (a lower bound of its total)
    double maxB = NEG_INF;   // max of the match-through terms written for the next checkpoint

    // appends the passing lanes in cell order; `ordered` has bit i set when cell i of the diagonal passes
    auto emit_cand = [&](bool pass, unsigned long long ordered, int cell, int x, int y, double fb) {
        int rank = __popcll(ordered & ((1ull << cell) - 1ull));
        if (pass) {
            int pos = count + rank;
            if (pos < cand_cap) {
                sa_cand_t cd;
                cd.x = x - 1; cd.y = y - 1; cd.path = 0; cd.pad = 0; cd.fb = fb;
                my_cands[pos] = cd;
            } else {
                overflow[0] = 1;
            }
        }
        count += __popcll(ordered);
    };

    // EXPECT + HDP: a cell's transitions into the match state that may reach the threshold (t = from-state 0..2), appended in
    // the reference's order: cells in ascending x, transitions of a cell in the order match, gapX, gapY
    auto emit_assign = [&](bool p0, bool p1, bool p2, int rot, int cell, int x, int y, double v0, double v1, double v2) {
        unsigned long long b0 = __ballot(p0), b1 = __ballot(p1), b2 = __ballot(p2);
        if (!(b0 | b1 | b2)) return;
        if (rot) { b0 = (b0 >> rot) | (b0 << (64 - rot)); b1 = (b1 >> rot) | (b1 << (64 - rot)); b2 = (b2 >> rot) | (b2 << (64 - rot)); }
        const unsigned long long below = (1ull << cell) - 1ull;
        int pos = count + __popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below);
        const double vv[3] = {v0, v1, v2};
        const bool pp[3] = {p0, p1, p2};
#pragma unroll
        for (int t = 0; t < 3; t++)
            if (pp[t]) {
                if (pos < cand_cap) {
                    sa_cand_t cd;
                    cd.x = x - 1; cd.y = y - 1; cd.path = 0; cd.pad = t; cd.fb = vv[t];
                    my_cands[pos] = cd;
                } else {
                    overflow[0] = 1;
                }
                pos++;
            }
        count += __popcll(b0) + __popcll(b1) + __popcll(b2);
    };
    ExpAcc XA = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double t_lo_m = T.t_mx, t_lo_x = T.t_xx;   // (the gapX message carries log 0.1)

    const rsrc_t rs_xc = make_rsrc(xc), rs_ev = make_rsrc(ev), rs_F = make_rsrc(F);
    const unsigned C8 = (unsigned) C * 8u;
    const unsigned sentinel8 = C8 - 8u;  // cell C-1 of the match plane holds -inf (written by k_fwd_fast)
    const double *Eg = HDP ? E_all + R->f_base : nullptr;   // HDP: the region's emission plane (k_emit_hdp)
    const rsrc_t rs_E = make_rsrc(HDP ? Eg : ev);
    // two-distribution emission: the events' and the positions' noise constants (FastT.two_xn_off)
    const double4 *en3 = TWO ? reinterpret_cast<const double4 *>(E_all) + R->ev_off : nullptr;
    const double4 *xn = TWO ? reinterpret_cast<const double4 *>(E_all) + T.two_xn_off + R->pid_off : nullptr;
    const rsrc_t rs_en = make_rsrc(TWO ? (const void *) en3 : (const void *) ev), rs_xn = make_rsrc(TWO ? (const void *) xn : (const void *) ev);
    // candidate bound: spec - slack + log(threshold) - eps for the whole traceback (T.spec), or -- the expectation pass -- per
    // checkpoint group Mc + log(threshold) - eps
    // (a compile-time constant since round 4: every batch that reaches these kernels has its speculative totals -- launch_bwd_fast
    // checks it --, and the maxima path, four DPP reduction chains per checkpoint diagonal, no longer sits in the hot loop's code)
    constexpr bool use_spec = !EXPECT;
    double lim = __builtin_inf();
    if (use_spec) {
        const double sp = T.spec[seg];
        lim = (sp > NEG_INF) ? sp - T.slack + T.thr_off : __builtin_inf();
    }

    int e = start;
    bool first = true;  // diagonal `start` is initialised with the end-state vector, always through memory
    while (e > to) {
        // (EXPECT also reads the forward states of e-1 and e-2 through the lanes: that window must fit a wave as well, which is
        // what SA_PK_FWD says of diagonal e -- without it a cell's lower neighbour aliased the far end of a wider band)
        if (!first && (pk[e] & SA_PK_BWD) && (!EXPECT || (pk[e] & SA_PK_FWD))) {
            // ---- register-resident section ----
            wave_fence();
            // mM of the last even / odd diagonal (a diagonal reads the slot of its own parity: written by e+2)
            double mMe = NEG_INF, mMo = NEG_INF, mY1 = NEG_INF, mX1 = NEG_INF;
            {
                double m1 = NEG_INF, m2 = NEG_INF;  // from e+1, e+2
                if (e + 1 <= start) {
                    const sa_row_t r1 = rows[e + 1];
                    int t1 = (lane - ((r1.xmyL + K) >> 1)) & 63;
                    const double *g = ring + ((e + 1) % 3) * 4 * rowcap;
                    if (t1 < r1.width) {
                        m1 = g[t1]; mY1 = g[rowcap + t1]; mX1 = g[2 * rowcap + t1];
                    }
                }
                if (e + 2 <= start) {
                    const sa_row_t r2 = rows[e + 2];
                    int t2 = (lane - ((r2.xmyL + K) >> 1)) & 63;
                    const double *g = ring + ((e + 2) % 3) * 4 * rowcap;
                    if (t2 < r2.width) m2 = g[t2];
                }
                mMe = (e & 1) ? m1 : m2;  // e odd: e+1 is even
                mMo = (e & 1) ? m2 : m1;
            }
            unsigned fo8 = (unsigned) rows[e].foff * 8u;
            // checkpoints of this traceback already behind us: from, from-10, ... > e
            int ck_seen = e > from ? 0 : (from - e + SA_CKPT_EVERY - 1) / SA_CKPT_EVERY;
            // 64 packed words covering diagonals [base, base+63], base = (e & ~31) - 32: e and e-1 are lanes >= 31.
            // What the sweep asks of a diagonal D besides its geometry depends on this traceback (from, to) but not on the
            // sweep's state, so it is folded into the words when a tile is loaded (ten vector instructions per 32 diagonals)
            // instead of being derived per diagonal by scalar compares -- the scalar unit is this kernel's second bottleneck
            // (DESIGN.md section 4).  Bits the backward sweep has no use for carry it:
            //   SA_PK_FWD      := D <= from                                   (a posterior diagonal)
            //   SA_PK_CK       := checkpoint and D <= from
            //   SA_PK_FULL     := D - 1 is a checkpoint, to < D - 1 <= from   (D holds the next checkpoint's match-through terms)
            //   SA_PK_BWD_MORE := D - 1 continues the register section and D - 1 > to
            auto bwd_tile = [&](int base) -> int {
                const int D = base + lane;
                int w = pk[D];
                const int below = __builtin_amdgcn_update_dpp(0, w, 0x138, 0xF, 0xF, false);   // word of D - 1 (lane 0: none, never used)
                const bool post_ = D <= from;
                const bool pre_ = (below & SA_PK_CK) && (D - 1 > to) && (D - 1 <= from);
                const bool more_ = (w & SA_PK_BWD_MORE) && (D - 1 > to) && (!EXPECT || (below & SA_PK_FWD));
                w &= ~(SA_PK_FWD | SA_PK_FULL | SA_PK_BWD_MORE | (post_ ? 0 : SA_PK_CK));
                w |= (post_ ? SA_PK_FWD : 0) | (pre_ ? SA_PK_FULL : 0) | (more_ ? SA_PK_BWD_MORE : 0);
                return w;
            };
            int pkv = bwd_tile((e & ~31) - 32);
            int pkn = bwd_tile((e & ~31) - 64);
            int pc = __builtin_amdgcn_readlane(pkv, (e & 31) + 32);

            auto load_fm = [&](const Stage &s, unsigned fo8_) -> double {
                // forward.match of the lane's cell; lanes outside the band read the -inf sentinel
                const unsigned vo = s.act ? (unsigned) s.t * 8u + fo8_ : sentinel8;
                return buf_load_f64_stream(rs_F, vo, 0);
            };
            // EXPECT: forward states (match, gapX, gapY) of the lane's cell on the last even / odd diagonal below e
            double fEm = NEG_INF, fEx = NEG_INF, fEy = NEG_INF, fOm = NEG_INF, fOx = NEG_INF, fOy = NEG_INF;
            auto load_set = [&](int p, unsigned fo8_, double &sm, double &sx, double &sy) {
                const int t = (lane - pk_ul(p)) & 63;
                const bool act = t < pk_width(p);
                const unsigned vo = (unsigned) t * 8u + fo8_;
                sm = buf_load_f64_stream(rs_F, act ? vo : sentinel8, 0);
                sx = buf_load_f64_stream(rs_F, act ? vo + C8 : sentinel8, 0);
                sy = buf_load_f64_stream(rs_F, act ? vo + 2u * C8 : sentinel8, 0);
            };
            // one diagonal of static parity; the mM slot that is read (from e+2) is overwritten with this diagonal's own mM.
            // pw / pnw: packed words of e and e-1.  EXPECT: (own_*) = states on e-2 (same lane: the middle neighbour), (oth_*) =
            // states on e-1 (lower / upper neighbour after the rotate the forward sweep uses); mid_ok: e-2 belongs to the traceback
            auto step = [&](auto odd, double lM, double lY_, int cur_t, int cur_x, int cur_y, bool cur_act, double fm,
                            int pw, int pnw, double &mM2, double own_m, double own_x, double own_y, double oth_m, double oth_x,
                            double oth_y, bool mid_ok) {
                double upm, lowm;
                if (!decltype(odd)::value) {  // upper source (x,y+1) is u-1, lower source (x+1,y) is u
                    upm = from_lane_below(mY1);
                    lowm = mX1;
                } else {                      // upper source is u, lower source is u+1
                    upm = mY1;
                    lowm = from_lane_above(mX1);
                }
                // (the per-site tables of the forward sweep do not pay here: this kernel is held at 96 registers for five
                // waves per SIMD, and the extra constants push twelve of them into scratch -- 5.33 -> 5.57 ms)
                LaP pm, px, py;
                la_prep(pm, mM2 + T.t_mm, upm + T.t_my);
                la_prep(px, mM2 + T.t_xm, lowm + T.t_xx);
                la_prep(py, mM2 + T.t_ym, upm + T.t_yy);
                la_fetch(pm, LT);
                la_fetch(px, LT);
                la_fetch(py, LT);
                __builtin_amdgcn_sched_barrier(0);
                const double tm1 = la_finish(pm);
                const double tx = la_finish(px);
                const double ty = la_finish(py);
                const double tm = la_fast(LT, tm1, lowm + T.t_mx);
                mM2 = tm + lM;                                   // -inf outside the band (NULL entry)
                mY1 = ty + lY_;                                  // -inf outside the band
                mX1 = cur_act ? tx + SA_LOG_GAPX : NEG_INF;
                // posterior side (all conditions wave-uniform: bits of the tile word, see bwd_tile)
                const bool post = (pw & SA_PK_FWD) != 0;
                const bool pre_ck = (pw & SA_PK_FULL) != 0;
                if (pw & (SA_PK_FWD | SA_PK_FULL)) {
                    const double fb = fm + tm;  // fm is -inf outside the band and on the x == 0 / y == 0 borders
                    if (pw & SA_PK_CK) {
                        if (EXPECT && ck_seen > 0) exp_flush(gsum, gmc, ck_base + ck_seen - 1, Mc, XA, lane);
                        const sa_ck_t ck = cks[ck_base + ck_seen];
                        ck_seen++;
                        const unsigned vo = (unsigned) cur_t * 8u;
                        double fx = cur_act ? buf_load_f64(rs_F, vo, fo8 + C8) : NEG_INF;
                        double fy = cur_act ? buf_load_f64(rs_F, vo, fo8 + 2u * C8) : NEG_INF;
                        double v = la_fast(LT, la_fast(LT, fb, fx + tx), fy + ty);
                        v = cur_act ? v : NEG_INF;
                        if (cur_act) vbuf[ck.voff + cur_t] = v;
                        if (!use_spec) {
                            double mA = wave_max(v);
                            if (HDP) mA += tight_bound_gain(mA - v);
                            Mc = (ck.nB > 0 && maxB > mA) ? maxB : mA;
                            lim = (Mc > NEG_INF) ? Mc + T.thr_off : __builtin_inf();
                        }
                    }
                    if (pre_ck) {  // this diagonal is "e+1" of the next checkpoint
                        const sa_ck_t ckn = cks[ck_base + ck_seen];
                        if (cur_act) vbuf[ckn.voff + ckn.nA + cur_t] = fb;
                        if (!use_spec) maxB = wave_max(fb);
                    }
                    if (post && !EXPECT) {
                        bool pass = fb >= lim;
                        unsigned long long mask = __ballot(pass);
                        if (mask) {
                            int s = pk_ul(pw) & 63;
                            unsigned long long ordered = s ? ((mask >> s) | (mask << (64 - s))) : mask;
                            emit_cand(pass, ordered, cur_t, cur_x, cur_y, fb);
                        }
                    }
                    if (EXPECT && post && Mc > NEG_INF) {
                        double lo_m, lo_x, up_m, up_y;
                        if (!decltype(odd)::value) {  // e even: lower (x-1,y) on e-1 is lane-1, upper (x,y-1) the lane itself
                            lo_m = from_lane_below(oth_m); lo_x = from_lane_below(oth_x);
                            up_m = oth_m; up_y = oth_y;
                        } else {                      // e odd: lower the lane itself, upper lane+1
                            lo_m = oth_m; lo_x = oth_x;
                            up_m = from_lane_above(oth_m); up_y = from_lane_above(oth_y);
                        }
                        const double bX = mX1 - Mc, bM = mM2 - Mc, bY = mY1 - Mc;   // this diagonal's messages (-inf without a cell)
                        XA.a0 += exp_term(lo_m + t_lo_m + bX);
                        XA.a1 += exp_term(lo_x + t_lo_x + bX);
                        if (mid_ok) {
                            const double v2 = own_m + T.t_mm + bM, v3 = own_x + T.t_xm + bM, v4 = own_y + T.t_ym + bM;
                            XA.a2 += exp_term(v2);
                            XA.a3 += exp_term(v3);
                            XA.a4 += exp_term(v4);
                            if (HDP) {
                                const double l2 = T.thr_off;   // v - (lim - Mc) >= 0  <=>  term >= lim
                                emit_assign(v2 >= l2, v3 >= l2, v4 >= l2, pk_ul(pw) & 63, cur_t, cur_x, cur_y, v2 + Mc, v3 + Mc, v4 + Mc);
                            }
                        }
                        XA.a5 += exp_term(up_m + T.t_my + bY);
                        XA.a6 += exp_term(up_y + T.t_yy + bY);
                    }
                }
            };
            auto half = [&](auto odd, const Stage &cur, double fm, Stage &nxt, double &fm_nxt, double &mM2) -> bool {
                const int li = (e & 31) + 32;
                const int pn = __builtin_amdgcn_readlane(pkv, li - 1);
                const unsigned fo8_n = fo8 - pk_row_bytes(pn);
                if (EXPECT) {   // the states on e-2 move into the set of e's own parity (whose old content, e's states, is done with)
                    const int pn2 = __builtin_amdgcn_readlane(pkv, li - 2);
                    if (!decltype(odd)::value) load_set(pn2, fo8_n - pk_row_bytes(pn2), fEm, fEx, fEy);
                    else load_set(pn2, fo8_n - pk_row_bytes(pn2), fOm, fOx, fOy);
                }
                if (HDP) nxt = stage_inputs_plane(pn, e - 1, K, lane, rs_E, fo8_n, sentinel8);
                else if (TWO) nxt = stage_inputs_two(pn, e - 1, K, lane, rs_xc, rs_ev, rs_xn, rs_en);
                else nxt = stage_inputs(pn, e - 1, K, lane, rs_xc, rs_ev);  // harmless when the sweep ends here
                fm_nxt = load_fm(nxt, fo8_n);
                double lM, lY_;
                emit_fast<HDP>(cur.c, cur.e, lM, lY_);
                if (TWO) emit_two(cur.cn, cur.n3, lM, lY_);
                if (!decltype(odd)::value) step(odd, lM, lY_, cur.t, cur.x, cur.y, cur.act, fm, pc, pn, mM2, fEm, fEx, fEy, fOm, fOx, fOy, e - 2 >= to);
                else step(odd, lM, lY_, cur.t, cur.x, cur.y, cur.act, fm, pc, pn, mM2, fOm, fOx, fOy, fEm, fEx, fEy, e - 2 >= to);
                const bool more = (pc & SA_PK_BWD_MORE) != 0;
                e--;
                pc = pn;
                fo8 = fo8_n;
                return more;
            };
            auto next_tile = [&]() {  // e just crossed a multiple of 32 downwards: (e & 31) == 31
                pkv = pkn;
                pkn = bwd_tile((e & ~31) - 64);
            };
            const std::integral_constant<bool, false> EVEN;
            const std::integral_constant<bool, true> ODD;
            Stage Se, So;
            double fe = NEG_INF, fo_ = NEG_INF;
            bool more = true;
            if (EXPECT) {   // the states on e-1, into the set of its parity
                const int p1 = __builtin_amdgcn_readlane(pkv, (e & 31) + 31);
                if (e & 1) load_set(p1, fo8 - pk_row_bytes(p1), fEm, fEx, fEy);
                else load_set(p1, fo8 - pk_row_bytes(p1), fOm, fOx, fOy);
            }
            if (e & 1) {
                if (HDP) So = stage_inputs_plane(pc, e, K, lane, rs_E, fo8, sentinel8);
                else if (TWO) So = stage_inputs_two(pc, e, K, lane, rs_xc, rs_ev, rs_xn, rs_en);
                else So = stage_inputs(pc, e, K, lane, rs_xc, rs_ev);
                fo_ = load_fm(So, fo8);
            } else {  // pairs are (odd, even) so that a tile ends with a pair: peel the even diagonal
                if (HDP) Se = stage_inputs_plane(pc, e, K, lane, rs_E, fo8, sentinel8);
                else if (TWO) Se = stage_inputs_two(pc, e, K, lane, rs_xc, rs_ev, rs_xn, rs_en);
                else Se = stage_inputs(pc, e, K, lane, rs_xc, rs_ev);
                fe = load_fm(Se, fo8);
                more = half(EVEN, Se, fe, So, fo_, mMe);
                if (more && (e & 31) == 31) next_tile();  // the peeled diagonal was the last of its tile
            }
            while (more) {
                do {
                    if (!half(ODD, So, fo_, Se, fe, mMo)) { more = false; break; }
                    more = half(EVEN, Se, fe, So, fo_, mMe);
                } while (more && (e & 31) != 31);
                if (more) next_tile();
            }
            if (e > to) {
                // the sweep goes on through memory: hand the live messages over to the ring
                const double m_e1 = ((e + 1) & 1) ? mMo : mMe;
                const double m_e2 = ((e + 1) & 1) ? mMe : mMo;
                const sa_row_t r1 = rows[e + 1];
                int t1 = (lane - ((r1.xmyL + K) >> 1)) & 63;
                double *g = ring + ((e + 1) % 3) * 4 * rowcap;
                if (t1 < r1.width) {
                    g[t1] = m_e1; g[rowcap + t1] = mY1; g[2 * rowcap + t1] = mX1;
                }
                if (e + 2 <= start) {
                    const sa_row_t r2 = rows[e + 2];
                    int t2 = (lane - ((r2.xmyL + K) >> 1)) & 63;
                    double *g2 = ring + ((e + 2) % 3) * 4 * rowcap;
                    if (t2 < r2.width) g2[t2] = m_e2;
                }
            }
        } else {
            // ---- memory-resident path: messages of the three live diagonals in the ring ----
            wave_fence();
            const sa_row_t re = rows[e];
            const bool post = e <= from;
            const bool is_ck = post && ((from - e) % SA_CKPT_EVERY == 0);
            const bool pre_ck = (e - 1 > to) && (e - 1 <= from) && ((from - (e - 1)) % SA_CKPT_EVERY == 0);
            const bool want_f = post || pre_ck;
            sa_ck_t ck = {0, 0, 0}, ckn = {0, 0, 0};
            if (is_ck) ck = cks[ck_base + (from - e) / SA_CKPT_EVERY];
            if (pre_ck) ckn = cks[ck_base + (from - (e - 1)) / SA_CKPT_EVERY];
            sa_row_t r1 = {0, 0, 0}, r2 = {0, 0, 0};
            const double *g1 = nullptr, *g2 = nullptr;
            if (e + 1 <= start) { r1 = rows[e + 1]; g1 = ring + ((e + 1) % 3) * 4 * rowcap; }
            if (e + 2 <= start) { r2 = rows[e + 2]; g2 = ring + ((e + 2) % 3) * 4 * rowcap; }
            double *g0 = ring + (e % 3) * 4 * rowcap;
            const int x0 = (e + re.xmyL) >> 1;
            double mA = NEG_INF, mB = NEG_INF;
            const int nch = (re.width + 63) >> 6;
            double fb_c0 = NEG_INF, fb_c1 = NEG_INF;
            for (int cch = 0; cch < nch; cch++) {
                int i = cch * 64 + lane;
                bool act = i < re.width;
                int ii = act ? i : 0;
                int xmy = re.xmyL + 2 * ii;
                int x = x0 + ii, y = e - x;
                double4 c;
                double ee;
                if (HDP) {
                    ee = act ? Eg[re.foff + ii] : NEG_INF;
                } else {
                    c = xc[y >= 1 ? x : 0];
                    ee = ev[y >= 1 ? y - 1 : 0];
                }
                double lM, lY_;
                emit_fast<HDP>(c, ee, lM, lY_);
                if (TWO) emit_two(xn[y >= 1 ? x : 0], en3[y >= 1 ? y - 1 : 0], lM, lY_);
                double tm, tx, ty;
                if (e == start) {
                    // endStateProb / raggedEndStateProb (impl/stateMachine.c:1145-1173)
                    const bool ragged_end = S->at_end && R->ragged_r;
                    tm = ragged_end ? (T.t_mx + T.t_my) / 2.0 : T.t_mm;
                    tx = ragged_end ? T.t_xx : T.t_xm;
                    ty = ragged_end ? T.t_yy : T.t_ym;
                } else {
                    int imid = xmy - r2.xmyL, iup = xmy - 1 - r1.xmyL, ilo = xmy + 1 - r1.xmyL;
                    bool hmid = g2 && imid >= 0 && (imid >> 1) < r2.width;
                    bool hup = g1 && iup >= 0 && (iup >> 1) < r1.width;
                    bool hlo = g1 && ilo >= 0 && (ilo >> 1) < r1.width;
                    double vM = hmid ? g2[imid >> 1] : NEG_INF;
                    double vY = hup ? g1[rowcap + (iup >> 1)] : NEG_INF;
                    double vX = hlo ? g1[2 * rowcap + (ilo >> 1)] : NEG_INF;
                    tm = la_fast(LT, la_fast(LT, vM + T.t_mm, vY + T.t_my), vX + T.t_mx);
                    tx = la_fast(LT, vM + T.t_xm, vX + T.t_xx);
                    ty = la_fast(LT, vM + T.t_ym, vY + T.t_yy);
                }
                if (act) {
                    g0[i] = tm + lM; g0[rowcap + i] = ty + lY_; g0[2 * rowcap + i] = tx + SA_LOG_GAPX;
                    if (cch >= 2) g0[3 * rowcap + i] = tm;   // read back by the candidate sweep (chunks beyond the second)
                }
                if (want_f) {
                    const double *pf = F + re.foff + ii;
                    double fm = act ? pf[0] : NEG_INF;
                    double fb = fm + tm;
                    if (cch == 0) fb_c0 = fb;
                    if (cch == 1) fb_c1 = fb;
                    if (pre_ck && ckn.nB > 0) {
                        if (act) vbuf[ckn.voff + ckn.nA + i] = fb;
                        if (!use_spec) {
                            double q = wave_max(act ? fb : NEG_INF);
                            mB = q > mB ? q : mB;
                        }
                    }
                    if (is_ck) {
                        double fx = act ? pf[C] : NEG_INF, fy = act ? pf[2 * C] : NEG_INF;
                        double v = la_fast(LT, la_fast(LT, fm + tm, fx + tx), fy + ty);
                        if (act) vbuf[ck.voff + i] = v;
                        if (!use_spec) {
                            double q = wave_max(act ? v : NEG_INF);
                            mA = q > mA ? q : mA;
                        }
                    }
                }
            }
            if (is_ck && !use_spec) {
                if (EXPECT && e != from) exp_flush(gsum, gmc, ck_base + (from - e) / SA_CKPT_EVERY - 1, Mc, XA, lane);
                Mc = (ck.nB > 0 && maxB > mA) ? maxB : mA;
                lim = (Mc > NEG_INF) ? Mc + T.thr_off : __builtin_inf();
            }
            if (pre_ck && ckn.nB > 0 && !use_spec) maxB = mB;
            if (EXPECT && post && Mc > NEG_INF) {
                // expectation terms of this diagonal: its messages are in the ring (g0), the forward states of e-1 and e-2 in
                // the forward planes
                wave_fence();
                const sa_row_t rm1 = rows[e - 1];
                const bool have2 = e - 2 >= to && e - 2 >= 0;
                sa_row_t rm2 = {0, 0, 0};
                if (have2) rm2 = rows[e - 2];
                for (int cch = 0; cch < nch; cch++) {
                    const int i = cch * 64 + lane;
                    const bool act = i < re.width;
                    const int ii = act ? i : 0;
                    const int xmy = re.xmyL + 2 * ii;
                    const int x = x0 + ii, y = e - x;
                    const double bM = (act ? g0[ii] : NEG_INF) - Mc, bY = (act ? g0[rowcap + ii] : NEG_INF) - Mc,
                                 bX = (act ? g0[2 * rowcap + ii] : NEG_INF) - Mc;
                    const int il = xmy - 1 - rm1.xmyL, iu = xmy + 1 - rm1.xmyL, im = xmy - rm2.xmyL;
                    const bool has_lo = act && il >= 0 && (il >> 1) < rm1.width && x >= 1;
                    const bool has_up = act && iu >= 0 && (iu >> 1) < rm1.width && y >= 1;
                    const bool has_mid = act && have2 && im >= 0 && (im >> 1) < rm2.width && x >= 1 && y >= 1;
                    const double *pl_ = F + rm1.foff + (has_lo ? il >> 1 : 0), *pu_ = F + rm1.foff + (has_up ? iu >> 1 : 0),
                                 *pm_ = F + rm2.foff + (has_mid ? im >> 1 : 0);
                    const double lo_m = has_lo ? pl_[0] : NEG_INF, lo_x = has_lo ? pl_[C] : NEG_INF;
                    const double up_m = has_up ? pu_[0] : NEG_INF, up_y = has_up ? pu_[2 * C] : NEG_INF;
                    const double mi_m = has_mid ? pm_[0] : NEG_INF, mi_x = has_mid ? pm_[C] : NEG_INF, mi_y = has_mid ? pm_[2 * C] : NEG_INF;
                    XA.a0 += exp_term(lo_m + t_lo_m + bX);
                    XA.a1 += exp_term(lo_x + t_lo_x + bX);
                    const double v2 = mi_m + T.t_mm + bM, v3 = mi_x + T.t_xm + bM, v4 = mi_y + T.t_ym + bM;
                    XA.a2 += exp_term(v2);
                    XA.a3 += exp_term(v3);
                    XA.a4 += exp_term(v4);
                    XA.a5 += exp_term(up_m + T.t_my + bY);
                    XA.a6 += exp_term(up_y + T.t_yy + bY);
                    if (HDP) emit_assign(v2 >= T.thr_off, v3 >= T.thr_off, v4 >= T.thr_off, 0, lane, x, y, v2 + Mc, v3 + Mc, v4 + Mc);
                }
            }
            if (post && !EXPECT) {  // second sweep: the checkpoint maximum is known now
                // the match products of the first two chunks (diagonals up to 128 cells) are still in registers; wider
                // diagonals read the rest back
                if (nch > 2) wave_fence();
                for (int cch = 0; cch < nch; cch++) {
                    int i = cch * 64 + lane;
                    bool act = i < re.width;
                    int ii = act ? i : 0;
                    int x = x0 + ii, y = e - x;
                    double fb;
                    if (cch < 2) {
                        fb = cch == 0 ? fb_c0 : fb_c1;
                    } else {
                        double fm = act ? F[re.foff + ii] : NEG_INF;
                        double tm = act ? g0[3 * rowcap + i] : NEG_INF;
                        fb = fm + tm;
                    }
                    bool pass = act && x > 0 && y > 0 && (use_spec ? fb >= lim : ((Mc > NEG_INF) && (fb >= Mc + T.thr_off)));
                    unsigned long long mask = __ballot(pass);
                    if (mask) emit_cand(pass, mask, lane, x, y, fb);
                }
            }
            first = false;
            e--;
        }
    }
    if (EXPECT && S->n_ck > 0) exp_flush(gsum, gmc, ck_base + S->n_ck - 1, Mc, XA, lane);
    if (lane == 0) cand_count[seg] = count < cand_cap ? count : cand_cap;
}

#undef rowcap
#undef ring

#define SA_BWD_FAST_OCC 5
// 96 VGPRs -> 5 waves per SIMD: measured 7 % faster than the 110 registers / 4 waves the compiler picks on its own
// (6 waves spill and lose)
__global__ __launch_bounds__(64 * FAST_WAVES) __attribute__((amdgpu_waves_per_eu(SA_BWD_FAST_OCC, SA_BWD_FAST_OCC))) void k_bwd_fast(
    const sa_region_t *__restrict__ regions, const sa_seg_t *__restrict__ segs, const sa_row_t *__restrict__ rows_all,
    const int *__restrict__ pk_all, const sa_ck_t *__restrict__ cks, const double4 *__restrict__ xc_all,
    const double *__restrict__ ev_all, const double *__restrict__ F_all, double *__restrict__ vbuf,
    sa_cand_t *__restrict__ cands, int *__restrict__ cand_count, int *__restrict__ overflow,
    double *__restrict__ bscratch, FastT T, const int *__restrict__ seg_ids, int n) {
    bwd_fast_body<false, false>(regions, segs, rows_all, pk_all, cks, xc_all, ev_all, F_all, vbuf, cands, cand_count, overflow,
                                bscratch, nullptr, T, seg_ids, n);
}
__global__ __launch_bounds__(64 * FAST_WAVES) void k_bwd_fast_hdp(
    const sa_region_t *__restrict__ regions, const sa_seg_t *__restrict__ segs, const sa_row_t *__restrict__ rows_all,
    const int *__restrict__ pk_all, const sa_ck_t *__restrict__ cks, const double4 *__restrict__ xc_all,
    const double *__restrict__ ev_all, const double *__restrict__ F_all, double *__restrict__ vbuf,
    sa_cand_t *__restrict__ cands, int *__restrict__ cand_count, int *__restrict__ overflow,
    double *__restrict__ bscratch, const double *__restrict__ E_all, FastT T, const int *__restrict__ seg_ids, int n) {
    bwd_fast_body<true, false>(regions, segs, rows_all, pk_all, cks, xc_all, ev_all, F_all, vbuf, cands, cand_count, overflow,
                               bscratch, E_all, T, seg_ids, n);
}
__global__ __launch_bounds__(64 * FAST_WAVES) void k_bwd_fast_two(
    const sa_region_t *__restrict__ regions, const sa_seg_t *__restrict__ segs, const sa_row_t *__restrict__ rows_all,
    const int *__restrict__ pk_all, const sa_ck_t *__restrict__ cks, const double4 *__restrict__ xc_all,
    const double *__restrict__ ev_all, const double *__restrict__ F_all, double *__restrict__ vbuf,
    sa_cand_t *__restrict__ cands, int *__restrict__ cand_count, int *__restrict__ overflow,
    double *__restrict__ bscratch, const double *__restrict__ N_all, FastT T, const int *__restrict__ seg_ids, int n) {
    bwd_fast_body<false, false, true>(regions, segs, rows_all, pk_all, cks, xc_all, ev_all, F_all, vbuf, cands, cand_count, overflow,
                                      bscratch, N_all, T, seg_ids, n);
}
// the expectation pass (see bwd_fast_body); E_all == nullptr: Gaussian emissions
#define SA_BWD_EXPECT_OCC 3
template <bool HDP>
__global__ __launch_bounds__(64 * FAST_WAVES) __attribute__((amdgpu_waves_per_eu(SA_BWD_EXPECT_OCC, SA_BWD_EXPECT_OCC))) void k_bwd_fast_expect(
    const sa_region_t *__restrict__ regions, const sa_seg_t *__restrict__ segs, const sa_row_t *__restrict__ rows_all,
    const int *__restrict__ pk_all, const sa_ck_t *__restrict__ cks, const double4 *__restrict__ xc_all,
    const double *__restrict__ ev_all, const double *__restrict__ F_all, double *__restrict__ vbuf,
    sa_cand_t *__restrict__ cands, int *__restrict__ cand_count, int *__restrict__ overflow,
    double *__restrict__ bscratch, const double *__restrict__ E_all, FastT T, const int *__restrict__ seg_ids, int n,
    double *__restrict__ gsum, double *__restrict__ gmc) {
    bwd_fast_body<HDP, true>(regions, segs, rows_all, pk_all, cks, xc_all, ev_all, F_all, vbuf, cands, cand_count, overflow,
                             bscratch, E_all, T, seg_ids, n, gsum, gmc);
}

// wide_cap: cells per row of k_fwd_fast*'s LDS ring for wide diagonals (0 for every other kernel)
static FastT make_fast_t(const DevPlan &P, int wide_cap = 0) {
    FastT T;
    memset(&T, 0, sizeof(T));
    T.t_mm = P.m.t_mm; T.t_xm = P.m.t_xm; T.t_ym = P.m.t_ym; T.t_my = P.m.t_my; T.t_yy = P.m.t_yy;
    T.t_mx = P.m.t_mx; T.t_xx = P.m.t_xx;
    T.thr_off = P.log_thr - SA_CAND_EPS;
    T.wide_cap = wide_cap;
    T.spec = P.spec;
    T.slack = P.spec_slack;
    T.two_xn_off = P.two_xn_off;
    if (P.m.hdp) {
        T.g0 = P.m.hdp_g0; T.gN = P.m.hdp_gN; T.dx = P.m.hdp_dx; T.inv_dx = 1.0 / P.m.hdp_dx;
        T.nm2 = (double) (P.m.grid_len - 2);
        T.hdp_bytes = P.m.hdp_tab_bytes;
        T.hdp_hot = P.m.hdp_hot;
    }
    return T;
}

// The register kernels: one wave per region (forward) / segment (backward), FAST_WAVES to a workgroup.  The emission flavour
// (HDP plane, two distributions, Gaussian) and the expectation pass pick the instance; the HDP and two-distribution kernels
// take their extra table through the same parameter.
static void launch_fwd_fast(const DevPlan &P, const int *ids, int n, hipStream_t st, int wide_cap) {
    const dim3 grid((n + FAST_WAVES - 1) / FAST_WAVES), block(64 * FAST_WAVES);
    const size_t lds = sizeof(double) * 9 * (size_t) wide_cap * FAST_WAVES;   // 3 rows x 3 planes per wave
    const FastT T = make_fast_t(P, wide_cap);
    const double4 *xc = reinterpret_cast<const double4 *>(P.xc);
    if (P.m.hdp || P.two) {
        auto k = P.m.hdp ? k_fwd_fast_hdp : k_fwd_fast_two;
        hipLaunchKernelGGL(k, grid, block, lds, st, P.regions, P.rows, P.pk, xc, P.ev, P.F, P.m.hdp ? (const double *) P.E : P.two,
                           T, ids, n, P.segs);
    } else {
        hipLaunchKernelGGL(k_fwd_fast, grid, block, lds, st, P.regions, P.rows, P.pk, xc, P.ev, P.F, T, ids, n, P.segs);
    }
}
// returns SA_OK, or SA_ESTATE when the batch's state does not allow the launch (the caller's pass fails with that code: a library does
// not abort its process)
static int launch_bwd_fast(const DevPlan &P, const int *ids, int n, hipStream_t st) {
    if (!P.expect && P.spec == nullptr) {   // (cannot happen: a batch with register-kernel regions allocates d_spec, batch_finish_body)
        fprintf(stderr, "[signalalign_hip] internal error: backward register kernels launched without speculative totals\n");
        return SA_ESTATE;
    }
    const dim3 grid((n + FAST_WAVES - 1) / FAST_WAVES), block(64 * FAST_WAVES);
    const FastT T = make_fast_t(P);
    const double4 *xc = reinterpret_cast<const double4 *>(P.xc);
    const double *F = P.F;
    if (P.expect) {
        auto k = P.m.hdp ? k_bwd_fast_expect<true> : k_bwd_fast_expect<false>;
        hipLaunchKernelGGL(k, grid, block, 0, st, P.regions, P.segs, P.rows, P.pk, P.cks, xc, P.ev, F, P.vbuf, P.cands, P.cand_count,
                           P.overflow, P.bscratch, P.m.hdp ? (const double *) P.E : nullptr, T, ids, n, P.gsum, P.gmc);
    } else if (P.m.hdp || P.two) {
        auto k = P.m.hdp ? k_bwd_fast_hdp : k_bwd_fast_two;
        hipLaunchKernelGGL(k, grid, block, 0, st, P.regions, P.segs, P.rows, P.pk, P.cks, xc, P.ev, F, P.vbuf, P.cands, P.cand_count,
                           P.overflow, P.bscratch, P.m.hdp ? (const double *) P.E : P.two, T, ids, n);
    } else {
        hipLaunchKernelGGL(k_bwd_fast, grid, block, 0, st, P.regions, P.segs, P.rows, P.pk, P.cks, xc, P.ev, F, P.vbuf, P.cands,
                           P.cand_count, P.overflow, P.bscratch, T, ids, n);
    }
    return SA_OK;
}
// The emission plane (HDP models only) of one launch list, one 256-thread workgroup per EMIT_TILE diagonals of each region: the
// register-kernel regions of a forward-storage pass (ring == false), or the ring / strip regions of one launch list (ring == true;
// multi: several paths per cell, per-path records).  max_n: diagonals of the longest region of the list.
static void launch_emit_hdp(const DevPlan &P, const int *ids, int n, long long max_n, hipStream_t st, bool ring, bool multi) {
    const unsigned tiles = (unsigned) ((max_n + 1 + EMIT_TILE - 1) / EMIT_TILE);
    const FastT T = make_fast_t(P);
    const double4 *xc = reinterpret_cast<const double4 *>(P.xc);
    for (int a = 0; a < n; a += 32768) {   // (grid.y is a 16-bit quantity)
        const dim3 grid(tiles, (unsigned) (n - a < 32768 ? n - a : 32768));
        if (ring) {
            auto k = multi ? k_emit_hdp_ring<true> : k_emit_hdp_ring<false>;
            hipLaunchKernelGGL(k, grid, dim3(256), 0, st, P.regions, P.rows, P.prec, xc, P.ev, P.m.hdp_tab, P.m.hdp_coef, P.E, T, ids + a);
        } else {
            hipLaunchKernelGGL(k_emit_hdp, grid, dim3(256), 0, st, P.regions, P.rows, xc, P.ev, P.m.hdp_tab, P.m.hdp_coef, P.E, T, ids + a);
        }
    }
}
