/* sa_plan_rules.h -- the planner's rules, stated once for the host planner (sa_plan.c, C11) and the device planner
 * (sa_dplan.inc, HIP device code).  Rules only: pure functions of their arguments -- no allocation, no environment, no
 * sa_plan_t.  How a planner walks a read (the host's serial loops, the device's strided loops, scans and searches) is its
 * own; what it computes per diagonal, per segment, per path and per region is here, so the two agree by construction
 * (tests/test_gpu_dplan.py still compares every byte).  Floating-point inputs (cf, wide_cells) are the callers'. */
#ifndef SA_PLAN_RULES_H_
#define SA_PLAN_RULES_H_

#include "sa_internal.h"

#if defined(__HIPCC__)   /* (__forceinline__ less the `inline` that `static inline` has said already) */
#define SA_HD __host__ __device__ __attribute__((always_inline))
#else
#define SA_HD
#endif

/* ---- band (band_construct, impl/pairwiseAligner.c:195-246) ---------------------------------------------------------
 * Generated per integer type I: the host uses the 64-bit instance only; the device evaluates the band in 32 bits when every
 * coordinate sum of the read fits 30 bits (sa_band_fits32) -- same operations, same results, and 64-bit integer arithmetic
 * costs two to four instructions per operation in what is most of the device planner's instructions.
 *   sa_clampz:    z clamped to [0, hi]
 *   sa_clip_row:  one anti-diagonal of the band: the stretch of x-y between the lower corner (xL,yL) and the upper corner
 *                 (xU,yU) of the current anchor-to-anchor box, snapped to the parity of xay.  *lo and *hi are always
 *                 written; SA_EBAND when they are no diagonal.
 *   sa_band_box:  those corners {xL, yL, xU, yU} for the diagonals between the previous anchor (p_sum, p_dif: its x+y and x-y
 *                 in matrix coordinates, 0, 0 in front of the first) and the next one (n_sum, n_dif; (lX, lY) behind the last), expanded by e
 *   sa_span3:     lanes needed to hold diagonal d, the two before it and one neighbour each side, as (x-y+K)>>1 */
#define SA_BAND_RULES(I, sfx)                                                                                          \
    static inline SA_HD I sa_clampz##sfx(I z, I hi) { return z < 0 ? 0 : (z > hi ? hi : z); }                          \
    static inline SA_HD int sa_clip_row##sfx(I xay, I xL, I yL, I xU, I yU, I *lo, I *hi) {                            \
        I a = xL - yL, b = xU - yU;                                                                                    \
        if ((xay + a) % 2 != 0) a++;                                                                                   \
        if ((xay + b) % 2 != 0) b++;                                                                                   \
        I x = (xay + a) / 2;                                                                                           \
        if (x < xL) a += 2 * (xL - x);                                                                                 \
        I y = (xay - a) / 2;                                                                                           \
        if (yL < y) a += 2 * (y - yL);                                                                                 \
        x = (xay + b) / 2;                                                                                             \
        if (xU < x) b -= 2 * (x - xU);                                                                                 \
        y = (xay - b) / 2;                                                                                             \
        if (y < yU) b -= 2 * (yU - y);                                                                                 \
        *lo = a, *hi = b;                                                                                              \
        return ((xay + a) % 2 != 0 || (xay + b) % 2 != 0 || a > b) ? SA_EBAND : SA_OK;                                 \
    }                                                                                                                  \
    static inline SA_HD void sa_band_box##sfx(I p_sum, I p_dif, I n_sum, I n_dif, I e, I lX, I lY, I *box) {           \
        box[0] = sa_clampz##sfx((p_sum + p_dif - e) / 2, lX); /* xL */                                                 \
        box[1] = sa_clampz##sfx((n_sum - n_dif + e) / 2, lY); /* yL */                                                 \
        box[2] = sa_clampz##sfx((n_sum + n_dif + e) / 2, lX); /* xU */                                                 \
        box[3] = sa_clampz##sfx((p_sum - p_dif - e) / 2, lY); /* yU */                                                 \
    }                                                                                                                  \
    static inline SA_HD int32_t sa_span3##sfx(const sa_row_t *rows, I d, I K) {                                        \
        const sa_row_t r = rows[d];                                                                                    \
        const I uL = ((I) r.xmyL + K) >> 1, uR = uL + r.width - 1;                                                     \
        I wl = uL - 1, wr = uR + 1;                                                                                    \
        for (I b = 1; b <= 2 && d - b >= 0; b++) {                                                                     \
            const sa_row_t q = rows[d - b];                                                                            \
            const I l2 = ((I) q.xmyL + K) >> 1, r2 = l2 + q.width - 1;                                                 \
            wl = l2 < wl ? l2 : wl;                                                                                    \
            wr = r2 > wr ? r2 : wr;                                                                                    \
        }                                                                                                              \
        return (int32_t) (wr - wl + 1);                                                                                \
    }
SA_BAND_RULES(int64_t, _64)
SA_BAND_RULES(int32_t, _32)
#undef SA_BAND_RULES
static inline SA_HD int sa_band_fits32(int64_t N, int64_t e) { return N + 2 * e + 4 < (1ll << 30) && e >= 0; }

/* ---- per-diagonal words --------------------------------------------------------------------------------------------- */
/* even offset so that (x-y+K)>>1 >= 0 */
static inline SA_HD int64_t sa_band_K(int64_t lY) { return lY + (lY & 1) + 2; }
/* packed band word of a diagonal `width` cells wide whose first cell is uL = (x-y+K)>>1; s3 = sa_span3 of the diagonal,
 * s3b = sa_span3 of diagonal min(d + 2, N) */
static inline SA_HD int32_t sa_pk_word(int32_t width, uint32_t uL, int32_t s3, int32_t s3b) {
    int32_t word = (int32_t) ((uint32_t) (width > SA_PK_WIDTH_MASK ? SA_PK_WIDTH_MASK : width) | (uL << SA_PK_SHIFT));
    if (s3 <= 64) word |= SA_PK_FWD;
    if (s3b <= 64) word |= SA_PK_BWD;
    return word;
}
/* derived flags of diagonal d's word w from the words of d-1 (not looked at for d = 0), d+1 and d+2 (zero behind diagonal N), once the
 * schedule has set SA_PK_CK; `expect`: the expectation pass reads all three forward states of every diagonal
 * (impl/pairwiseAligner.c:1423-1443).  The bits returned are not among those tested here. */
static inline SA_HD int32_t sa_pk_derived(int32_t w, int32_t w_prev, int32_t w1, int32_t w2, int64_t d, int64_t N, int expect) {
    int32_t add = 0;
    if ((w & SA_PK_CK) || !(w1 & SA_PK_FWD) || !(w2 & SA_PK_FWD) || d + 2 > N || expect) add |= SA_PK_FULL;
    if (d < N && (w1 & SA_PK_FWD)) add |= SA_PK_FWD_MORE;
    if (d >= 1 && (w_prev & SA_PK_BWD)) add |= SA_PK_BWD_MORE;
    return add;
}

/* ---- sizes of a region's arrays ------------------------------------------------------------------------------------- */
static inline SA_HD int64_t sa_job_lX(int64_t ref_len, int k) { /* sequence_correctSeqLength */
    const int64_t lX = ref_len == 0 ? 0 : ref_len - (k - 1);
    return lX < 0 ? 0 : lX;
}
/* rows: diagonals 0..N and one sentinel row behind them (SA_KIND_RING: its offset closes the last diagonal); packed words: SA_PK_PAD
 * readable zero words in front of diagonal 0, 160 behind diagonal N; path offsets: x = 0 (the NULL k-mer) .. lX and the closing one */
static inline SA_HD int64_t sa_region_rows(int64_t N) { return N + 2; }
static inline SA_HD int64_t sa_region_pk_words(int64_t N) { return N + 1 + SA_PK_PAD + 160; }
static inline SA_HD int64_t sa_region_poffs(int64_t lX) { return lX + 2; }

/* ---- routing: which kernels sweep a region ---------------------------------------------------------------------------
 * SA_KIND_FAST: the register kernels, one path per cell.  SA_KIND_RING (sa_ring.inc): several paths per cell, or one path
 * and a band mostly wider than a wave.  SA_KIND_GENERIC: the reference-ordered kernels, everything else. */
typedef struct sa_route_in {
    unsigned flags;           /* the batch: its flags, ... */
    int emission;             /* SA_EMISSION_*: the two-distribution emissions exist in the register kernels and the reference-
                               * ordered ones, and in the ring and strip kernels under SA_FLAG_TWO_DIST_ALL_KERNELS */
    int hdp, hdp_plane_fits;  /* the model has an HDP; sa_hdp_plane_fits(): the register kernels address its {y, slope} table with
                               * 32-bit byte offsets and the ring / strip kernels read the emission plane built from it */
    int ring_env, ring_wide_env;   /* sa_ring_env_on(), sa_ring_wide_env_on() */
    int ambig_distinct;       /* the index form of path legality (sa_prec_t) needs the options of every ambiguity letter distinct */
    int32_t max_p;            /* the region: paths of the cell with the most, ... */
    int64_t max_rowpaths, cellpaths, lX, lY, K;   /* cell-paths of the widest diagonal, of all diagonals */
    double cf, wide_cells;    /* cell-paths of diagonals 1..N; cells of those whose sa_span3 is more than a wave */
} sa_route_in_t;

static inline SA_HD int sa_route_kind(const sa_route_in_t *r) {
    const int forced = (r->flags & (SA_FLAG_EXACT | SA_FLAG_FORCE_GENERIC)) != 0;
    const int expect = (r->flags & SA_FLAG_EXPECT_INTERNAL) != 0;
    const int all_kernels = (r->flags & SA_FLAG_TWO_DIST_ALL_KERNELS) != 0;
    const int cells_ok = r->cellpaths + 1 <= SA_FAST_MAX_CELLS;   /* forward planes addressed with 32-bit byte offsets */
    const int fast_ok = r->max_p == 1 && !forced && r->hdp_plane_fits && cells_ok &&
                        ((r->lX + r->lY + r->K) >> 1) < (1ll << (31 - SA_PK_SHIFT));
    /* a two-distribution batch's regions with several paths per cell: rows of up to SA_RING_WIDE_MAX_ROWPATHS */
    const int64_t ring_max_rowpaths = (r->emission != 0 && all_kernels && r->max_p > 1 && !expect && !r->hdp)
                                          ? SA_RING_WIDE_MAX_ROWPATHS : SA_RING_MAX_ROWPATHS;
    /* (the expectation pass: ring kernels for regions with several paths per cell under a Gaussian model, never for one-path
     * regions, which keep the register kernels' expectation variant) */
    const int ring_ok = !forced && r->hdp_plane_fits && (r->emission == 0 || all_kernels) &&
                        (!expect || (r->max_p > 1 && !r->hdp)) && r->max_rowpaths <= ring_max_rowpaths && cells_ok &&
                        r->ring_env && (r->max_p == 1 || (r->max_p <= 255 && r->ambig_distinct));
    if (ring_ok && r->max_p > 1) return SA_KIND_RING;
    if (ring_ok && fast_ok && r->wide_cells > SA_RING_WIDE_FRACTION * r->cf && r->ring_wide_env) return SA_KIND_RING;
    return fast_ok ? SA_KIND_FAST : SA_KIND_GENERIC;
}

/* ---- traceback schedule (getPosteriorProbsWithBanding, impl/pairwiseAligner.c:1450-1590: the schedule only) ----------
 * A traceback that starts on diagonal d emits the posteriors of diagonals (to, from], to = where the previous one stopped. */
static inline SA_HD int64_t sa_seg_from(int64_t d, int at_end, int64_t trace_back) { return d - (at_end ? 0 : trace_back + 1); }
/* total-probability checkpoints: diagonals from, from - SA_CKPT_EVERY, ... > to */
static inline SA_HD int64_t sa_seg_n_ck(int64_t from, int64_t to) { return (from - to + SA_CKPT_EVERY - 1) / SA_CKPT_EVERY; }
/* candidate slots.  Measured: 0.54 pairs per diagonal at threshold 0.01 with Gaussian emissions; HDP densities as broad as
 * the bundled model's leave the posteriors flat across the band (3-6 candidates per diagonal at threshold 0.1); overflow
 * re-runs the pass with 4x.  (The 32: short tracebacks at a read's end.) */
static inline SA_HD int64_t sa_seg_cand_cap(int hdp, int64_t from, int64_t to) {
    const int64_t cap = (hdp ? SA_CAND_PER_DIAG_HDP : SA_CAND_PER_DIAG) * (from - to + 32);
    return cap > INT32_MAX ? INT32_MAX : cap;
}
/* doubles of backward scratch: 3 rows x 4 for the memory-resident path; the ring kernels keep backward rows in LDS (a wide
 * ring's checkpoint sums: 6 rows of its capacity, k_bwd_ring<WIDE>) */
static inline SA_HD int64_t sa_seg_bscratch(int kind, int64_t max_rowpaths) {
    if (kind != SA_KIND_RING) return 12 * max_rowpaths;
    return max_rowpaths > SA_RING_MAX_ROWPATHS ? 6 * (int64_t) SA_RING_WIDE_MAX_ROWPATHS : 0;
}

/* ---- per-path neighbour records of a SA_KIND_RING region with ambiguous positions -------------------------------------
 * Paths of column x enumerate the substitutions of the window s[x-1 .. x+k-2] with the LAST position varying fastest, so
 * with n(c) options for letter c,
 *   shared(x) = product of n over the first k-1 letters of the window = P(x) / n(last letter),
 * path p of column x and path q of column x-1 are a legal step (k-1 shared letters, path_checkLegal) iff
 *   q mod shared(x) == p / n(last letter of x):
 * the legal predecessors of p are q = j * shared(x) + p / n_last(x), j < n(first letter of x-1) (strided), and the legal
 * successors of q in column x+1 are the n_last(x+1) consecutive paths from (q mod shared(x+1)) * n_last(x+1).  The NULL
 * k-mer of column 0 is a legal neighbour of everything (path_checkLegal with a NULL k-mer). */
typedef struct sa_prec_col { int64_t x, lX, n_last, shared_n, n_last_n; uint32_t meta; } sa_prec_col_t;
/* column 0: the NULL k-mer; every path of column 1 is a successor.  poff: the region's path offsets. */
static inline SA_HD int sa_prec_col0(const int32_t *poff, int64_t lX, sa_prec_t *o) {
    const int64_t P1 = lX >= 1 ? poff[2] - poff[1] : 0;
    o->x = 0; o->pred0 = -1; o->succ0 = lX >= 1 ? poff[1] : -1; o->meta = (uint32_t) P1;
    return P1 > 255 ? SA_EUNSUPPORTED : SA_OK;
}
/* column x >= 1 of lX: n_prev, n_first, n_last, n_next = options of the letter in front of the window (1 at x = 1), of its
 * first and last letter, and of the letter behind it (1 at x = lX).  SA_EUNSUPPORTED when the record cannot hold the column. */
static inline SA_HD int sa_prec_column(sa_prec_col_t *c, const int32_t *poff, int64_t x, int64_t lX, int64_t n_prev,
                                       int64_t n_first, int64_t n_last, int64_t n_next) {
    const int64_t P = (int64_t) poff[x + 1] - poff[x], shared = P / n_last;
    int64_t npred = 1, stride = 0, nsucc = 0;
    if (x >= 2) { npred = n_prev; stride = shared; }
    c->x = x; c->lX = lX; c->n_last = n_last; c->shared_n = 1; c->n_last_n = 1;
    if (x < lX) { c->n_last_n = n_next; c->shared_n = P / n_first; nsucc = n_next; }
    c->meta = (uint32_t) (stride << 16) | (uint32_t) (npred << 8) | (uint32_t) nsucc;
    return (npred > 255 || nsucc > 255 || stride > 65535) ? SA_EUNSUPPORTED : SA_OK;
}
/* ... and its path p */
static inline SA_HD sa_prec_t sa_prec_path(const sa_prec_col_t *c, const int32_t *poff, int64_t p) {
    sa_prec_t o;
    o.x = (int32_t) c->x;
    o.pred0 = (int32_t) (c->x >= 2 ? poff[c->x - 1] + p / c->n_last : 0);
    o.succ0 = c->x < c->lX ? (int32_t) (poff[c->x + 1] + (p % c->shared_n) * c->n_last_n) : -1;
    o.meta = c->meta;
    return o;
}

#endif
