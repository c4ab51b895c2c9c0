// HDP distribution distances on the GPU (include/signalalign_hip.h, DESIGN.md "HDP distribution distances"):
//   k_hdp_dist_tiles   DistributionMetricMemo filled at once (impl/hdp.c:2614-2636 fills it lazily, a pair at a time): all pairs
//                      i > j among n rows sampled on one grid, for one of kl_divergence (:2666-2683), hellinger_distance
//                      (:2693-2710), l2_distance (:2720-2738), shannon_jensen_distance (:2748-2767)
//   k_hdp_dist_pairs   the same point functions for a list of pairs (get_dir_proc_distance :2614-2636, compare_hdp_distrs :2809-2842)
//   k_hdp_density      dir_proc_density (:2588-2612) = max(0, grid_spline_interp (impl/hdp_math_utils.c:471-495))
//   k_hdp_vs_gauss     a DP's posterior row against a normal density: scipy's entropy in bits, hellinger2 and the distance of the
//                      mode from the mean (src/signalalign/hiddenMarkovModel.py:775-837), one wave per entry
// One thread owns a pair from the first grid point to the last: the trapezoid sum starts at 0.0 and adds 0.5 * (left + right) * dx
// in grid order, as the reference does, and the point functions are the reference's expressions term for term.  Built with
// -ffp-contract=off like everything else; no clamping and no special cases, so a zero density is a NaN for the two logarithmic
// metrics and an integral above one is a NaN for Hellinger, as in the reference.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "signalalign_hip.h"
#include "sa_hdpdev.h"
#include "sa_hdpstate.h"
#include "sa_scratch.h"

namespace {

// ---- what differs between the metrics: the point function and the final step -----------------------------------------------------
template <int M>
__device__ __forceinline__ double dist_point(double p, double q) {
    if (M == SA_HDP_METRIC_KL) return p * log(p / q) + q * log(q / p);
    if (M == SA_HDP_METRIC_HELLINGER) return sqrt(p * q);
    if (M == SA_HDP_METRIC_L2) {
        const double diff = p - q;
        return diff * diff;
    }
    const double mean = 0.5 * (p + q);
    return 0.5 * (p * log(p / mean) + q * log(q / mean));
}

template <int M>
__device__ __forceinline__ double dist_final(double integral) {
    if (M == SA_HDP_METRIC_KL) return integral;
    if (M == SA_HDP_METRIC_HELLINGER) return sqrt(1.0 - integral);
    return sqrt(integral);
}

// ---- all pairs ---------------------------------------------------------------------------------------------------------------------
// A block of 256 threads covers DT_TILE rows i x DT_TILE rows j; a thread holds DT_REG x DT_REG pairs in registers (their sums and
// their left points), rows i = i0 + ty + 16 a, rows j = j0 + tx + 16 b: the 16 threads of a tx run write 16 adjacent j of one
// triangular row.  The two row sets go through LDS in chunks of DT_CHUNK grid points, transposed ([grid point][row], padded by one
// double: the staging stores of a 16-lane group then fall into 16 different bank pairs and the q reads of a wave are contiguous),
// with the chunk's dx values beside them: a row value is read from HBM once per tile and from LDS once per 4 pairs.
constexpr int DT_TILE = 64, DT_REG = 4, DT_CHUNK = 32, DT_LD = DT_TILE + 1;

// tile_first: index of the band's first tile in the sequence (0,0) (1,0) (1,1) (2,0) ... of the tiles on or below the diagonal;
// out_base: triangular index of the band's first element -- slab[(i - 1) * i / 2 + j - out_base]
template <int M>
__global__ __launch_bounds__(256) void k_hdp_dist_tiles(const double *__restrict__ grid, int grid_length, const double *__restrict__ rows,
                                                        long long n_rows, long long tile_first, long long out_base,
                                                        double *__restrict__ slab) {
    __shared__ double s_i[DT_CHUNK][DT_LD], s_j[DT_CHUNK][DT_LD], s_dx[DT_CHUNK];
    const long long t = tile_first + (long long) blockIdx.x;
    long long ti = (long long) ((sqrt(8.0 * (double) t + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > t) ti--;
    while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
    const long long tj = t - ti * (ti + 1) / 2;
    const long long i0 = ti * DT_TILE, j0 = tj * DT_TILE;
    const int tx = (int) threadIdx.x & 15, ty = (int) threadIdx.x >> 4;
    double acc[DT_REG][DT_REG], left[DT_REG][DT_REG];
#pragma unroll
    for (int a = 0; a < DT_REG; a++)
#pragma unroll
        for (int b = 0; b < DT_REG; b++) { acc[a][b] = 0.0; left[a][b] = 0.0; }
    for (int g0 = 0; g0 < grid_length; g0 += DT_CHUNK) {
        const int c = grid_length - g0 < DT_CHUNK ? grid_length - g0 : DT_CHUNK;
        __syncthreads();
        for (int k = (int) threadIdx.x; k < DT_TILE * DT_CHUNK; k += 256) {
            const int r = k / DT_CHUNK, g = k % DT_CHUNK;
            double vi = 1.0, vj = 1.0;   // (rows past the end and points past the grid: computed on, never written)
            if (g < c) {
                if (i0 + r < n_rows) vi = rows[(size_t) (i0 + r) * (size_t) grid_length + (size_t) (g0 + g)];
                if (j0 + r < n_rows) vj = rows[(size_t) (j0 + r) * (size_t) grid_length + (size_t) (g0 + g)];
            }
            s_i[g][r] = vi;
            s_j[g][r] = vj;
        }
        if ((int) threadIdx.x < c) {
            const int g = g0 + (int) threadIdx.x;
            s_dx[threadIdx.x] = g > 0 ? grid[g] - grid[g - 1] : 0.0;
        }
        __syncthreads();
        for (int g = 0; g < c; g++) {
            double p[DT_REG], q[DT_REG];
#pragma unroll
            for (int a = 0; a < DT_REG; a++) p[a] = s_i[g][ty + 16 * a];
#pragma unroll
            for (int b = 0; b < DT_REG; b++) q[b] = s_j[g][tx + 16 * b];
            const double dx = s_dx[g];
            const bool first = g0 + g == 0;   // (the first grid point is a left point only)
#pragma unroll
            for (int a = 0; a < DT_REG; a++)
#pragma unroll
                for (int b = 0; b < DT_REG; b++) {
                    const double right = dist_point<M>(p[a], q[b]);
                    if (!first) acc[a][b] += 0.5 * (left[a][b] + right) * dx;
                    left[a][b] = right;
                }
        }
    }
#pragma unroll
    for (int a = 0; a < DT_REG; a++)
#pragma unroll
        for (int b = 0; b < DT_REG; b++) {
            const long long i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            if (i < n_rows && j < i) slab[(i - 1) * i / 2 + j - out_base] = dist_final<M>(acc[a][b]);
        }
}

// ---- a list of pairs: row ia[t] of A against row ib[t] of B (ia / ib == nullptr: row t) ---------------------------------------------
template <int M>
__global__ __launch_bounds__(64) void k_hdp_dist_pairs(const double *__restrict__ grid, int grid_length, const double *__restrict__ A,
                                                       const long long *__restrict__ ia, const double *__restrict__ B,
                                                       const long long *__restrict__ ib, long long n, double *__restrict__ out) {
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double *p = A + (size_t) (ia ? ia[t] : t) * (size_t) grid_length;
    const double *q = B + (size_t) (ib ? ib[t] : t) * (size_t) grid_length;
    double acc = 0.0, left = dist_point<M>(p[0], q[0]);
    for (int g = 1; g < grid_length; g++) {
        const double right = dist_point<M>(p[g], q[g]);
        const double dx = grid[g] - grid[g - 1];
        acc += 0.5 * (left + right) * dx;
        left = right;
    }
    out[t] = dist_final<M>(acc);
}

// ---- densities -------------------------------------------------------------------------------------------------------------------------
// grid_spline_interp (impl/hdp_math_utils.c:471-495) operation for operation, both linear extrapolation branches included.  The one
// difference: the reference's left knot index, the truncated (query - x[0]) / dx, can round up to the last knot for a query just
// below it, and its right knot is then one past the arrays; here the index stays within [0, length - 2].
__device__ __forceinline__ double spline_interp(double query_x, const double *__restrict__ x, const double *__restrict__ y,
                                                const double *__restrict__ slope, int length) {
    if (query_x <= x[0]) return y[0] - slope[0] * (x[0] - query_x);
    if (query_x >= x[length - 1]) {
        const int n = length - 1;
        return y[n] + slope[n] * (query_x - x[n]);
    }
    const double dx = x[1] - x[0];
    long long idx_left = (long long) ((query_x - x[0]) / dx);
    if (!(idx_left >= 0)) idx_left = 0;
    if (idx_left > length - 2) idx_left = length - 2;
    const long long idx_right = idx_left + 1;
    const double dy = y[idx_right] - y[idx_left];
    const double a = slope[idx_left] * dx - dy;
    const double b = dy - slope[idx_right] * dx;
    const double t_left = (query_x - x[idx_left]) / dx;
    const double t_right = 1.0 - t_left;
    return t_right * y[idx_left] + t_left * y[idx_right] + t_left * t_right * (a * t_right + b * t_left);
}

// out[d * n_x + q] = max(0, spline of row row_of[d] at qx[q])
__global__ __launch_bounds__(256) void k_hdp_density(const double *__restrict__ x, int grid_length, const double *__restrict__ post,
                                                     const double *__restrict__ slope, const long long *__restrict__ row_of,
                                                     long long n_dps, const double *__restrict__ qx, long long n_x,
                                                     double *__restrict__ out) {
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_dps * n_x) return;
    const long long d = t / n_x, q = t - d * n_x;
    const size_t off = (size_t) row_of[d] * (size_t) grid_length;
    const double interp = spline_interp(qx[q], x, post + off, slope + off, grid_length);
    out[t] = interp > 0.0 ? interp : 0.0;
}

// ---- an HDP distribution against a normal density (hiddenMarkovModel.py:775-837) ---------------------------------------------------------
// get_kl_divergence / get_hellinger_distance / get_median_delta for one DP: p is its stored posterior row on the state's own grid g,
// q = exp(-((g - mean) / sd)^2 / 2) / sqrt(2 pi) / sd (scipy's norm.pdf, operation for operation).
//   kl_bits     scipy.stats.entropy(pk=p, qk=q, base=2): both divided by their sums, the sum of rel_entr, divided by log(2)
//   hellinger   hellinger2 (:1119-1120) on the values as they are: ||sqrt(p) - sqrt(q)|| / sqrt(2)
//   mode_delta  |g[first argmax p] - mean|
// One wave per entry: the lanes evaluate 64 grid points at a time (exp, log, sqrt), lane 0 adds them up in grid order, one
// accumulator per sum started at 0.0 (scipy adds pairwise: the restatement's sequential sum is within 1.5e-15 of it, relative).
// scipy.special.rel_entr (1.15: special/_convex_analysis.pxd)
__device__ __forceinline__ double rel_entr(double a, double b) {
    if (isnan(a) || isnan(b)) return NAN;
    if (a <= 0.0 || b <= 0.0) return (a == 0.0 && b >= 0.0) ? 0.0 : INFINITY;
    const double ratio = a / b;
    if (0.5 < ratio && ratio < 2.0) return a * log1p((a - b) / b);               // (close together: more accurate)
    if (2.2250738585072014e-308 < ratio && ratio < INFINITY) return a * log(ratio);
    return a * (log(a) - log(b));                                                 // (the quotient under- or overflows, or is subnormal)
}

__device__ __forceinline__ double norm_pdf(double g, double mean, double sd) {
    const double z = (g - mean) / sd;
    return exp(-(z * z) / 2.0) / 2.5066282746310002 / sd;
}

__global__ __launch_bounds__(64) void k_hdp_vs_gauss(const double *__restrict__ grid, int grid_length, const double *__restrict__ post,
                                                     const long long *__restrict__ row_of, const double *__restrict__ mean,
                                                     const double *__restrict__ sd, sa_hdp_gauss_cmp_t *__restrict__ out) {
    __shared__ double s_p[64], s_q[64], s_v[64], s_sum[2];
    const long long e = blockIdx.x, row = row_of[e];
    const int lane = threadIdx.x;
    sa_hdp_gauss_cmp_t R;
    R.kl_bits = 0.0; R.hellinger = 0.0; R.mode_delta = 0.0; R.status = 0; R.pad = 0;
    if (row < 0) {   // not observed: the Python reads an empty row and returns None
        R.status = 1;
        if (lane == 0) out[e] = R;
        return;
    }
    const double *p = post + (size_t) row * (size_t) grid_length;
    const double mu = mean[e], sg = sd[e];
    double sum_p = 0.0, sum_q = 0.0, sum_h = 0.0, sum_kl = 0.0, best = -INFINITY;
    int arg = 0;
    for (int g0 = 0; g0 < grid_length; g0 += 64) {
        const int c = grid_length - g0 < 64 ? grid_length - g0 : 64;
        if (lane < c) {
            const double pv = p[g0 + lane], qv = norm_pdf(grid[g0 + lane], mu, sg), diff = sqrt(pv) - sqrt(qv);
            s_p[lane] = pv; s_q[lane] = qv; s_v[lane] = diff * diff;
        }
        __syncthreads();
        if (lane == 0)
            for (int i = 0; i < c; i++) {
                sum_p += s_p[i]; sum_q += s_q[i]; sum_h += s_v[i];
                if (s_p[i] > best) { best = s_p[i]; arg = g0 + i; }
            }
        __syncthreads();
    }
    if (lane == 0) { s_sum[0] = sum_p; s_sum[1] = sum_q; }
    __syncthreads();
    sum_p = s_sum[0]; sum_q = s_sum[1];
    for (int g0 = 0; g0 < grid_length; g0 += 64) {
        const int c = grid_length - g0 < 64 ? grid_length - g0 : 64;
        if (lane < c) s_v[lane] = rel_entr(p[g0 + lane] / sum_p, norm_pdf(grid[g0 + lane], mu, sg) / sum_q);
        __syncthreads();
        if (lane == 0)
            for (int i = 0; i < c; i++) sum_kl += s_v[i];
        __syncthreads();
    }
    if (lane == 0) {
        R.kl_bits = sum_kl / 0.6931471805599453;
        R.hellinger = sqrt(sum_h) / 1.4142135623730951;
        R.mode_delta = fabs(grid[arg] - mu);
        R.status = isfinite(R.kl_bits) ? 0 : 2;
        out[e] = R;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
bool known_metric(int metric) { return metric >= SA_HDP_METRIC_KL && metric <= SA_HDP_METRIC_SHANNON_JENSEN; }

void launch_tiles(int metric, hipStream_t st, unsigned n_tiles, const double *grid, int G, const double *rows, long long n,
                  long long tile_first, long long out_base, double *slab) {
#define SA_TILES(M) hipLaunchKernelGGL(k_hdp_dist_tiles<M>, dim3(n_tiles), dim3(256), 0, st, grid, G, rows, n, tile_first, out_base, slab)
    switch (metric) {
        case SA_HDP_METRIC_KL: SA_TILES(SA_HDP_METRIC_KL); break;
        case SA_HDP_METRIC_HELLINGER: SA_TILES(SA_HDP_METRIC_HELLINGER); break;
        case SA_HDP_METRIC_L2: SA_TILES(SA_HDP_METRIC_L2); break;
        default: SA_TILES(SA_HDP_METRIC_SHANNON_JENSEN); break;
    }
#undef SA_TILES
}

void launch_pairs(int metric, hipStream_t st, const double *grid, int G, const double *A, const long long *ia, const double *B,
                  const long long *ib, long long n, double *out) {
    const dim3 blocks((unsigned) ((n + 63) / 64));
#define SA_PAIRS(M) hipLaunchKernelGGL(k_hdp_dist_pairs<M>, blocks, dim3(64), 0, st, grid, G, A, ia, B, ib, n, out)
    switch (metric) {
        case SA_HDP_METRIC_KL: SA_PAIRS(SA_HDP_METRIC_KL); break;
        case SA_HDP_METRIC_HELLINGER: SA_PAIRS(SA_HDP_METRIC_HELLINGER); break;
        case SA_HDP_METRIC_L2: SA_PAIRS(SA_HDP_METRIC_L2); break;
        default: SA_PAIRS(SA_HDP_METRIC_SHANNON_JENSEN); break;
    }
#undef SA_PAIRS
}

// Device and pinned-host scratch of sa_hdp_distances, kept between calls (sa_scratch.h): the rows, and two slabs of triangular
// output with a pinned buffer each -- band k's kernel fills one slab while band k - 1's leaves the other.
enum { DS_ROWS, DS_GRID, DS_SLAB, DS_HSLAB = DS_SLAB + 2 };   // (two slabs, two pinned buffers)
SaScratch g_dist_ws;

struct Band {
    long long tile_first, n_tiles, out_base, n_out;
};

// Slab size in doubles: 8 M (64 MB) unless SA_HDP_DIST_SLAB says otherwise (a test and measurement hook: with a small slab a small
// problem leaves in many bands).  A band holds at least one row of tiles whatever the size.
size_t slab_doubles() {
    if (const char *e = getenv("SA_HDP_DIST_SLAB")) {
        const long long v = atoll(e);
        if (v > 0) return (size_t) v;
    }
    return (size_t) 8 << 20;
}

// all-pairs distances of rows already on the device; tri_out is ordinary host memory
int distances_from_device(SaScratch &W, const double *d_grid, int64_t G, const double *d_rows, int64_t n, int metric, double *tri_out,
                          double *kernel_ms_out) {
    const long long n_tile_rows = (n + DT_TILE - 1) / DT_TILE;
    const size_t cap = slab_doubles();
    std::vector<Band> bands;
    for (long long ta = 0; ta < n_tile_rows;) {
        const long long r0 = ta * DT_TILE, base = r0 > 0 ? (r0 - 1) * r0 / 2 : 0;
        long long tb = ta + 1;
        auto end_of = [&](long long t_end) {
            const long long r1 = t_end * DT_TILE < n ? t_end * DT_TILE : n;
            return (r1 - 1) * r1 / 2;
        };
        while (tb < n_tile_rows && (size_t) (end_of(tb + 1) - base) <= cap && (tb + 1) * (tb + 2) / 2 - ta * (ta + 1) / 2 < (1ll << 30)) tb++;
        bands.push_back({ta * (ta + 1) / 2, tb * (tb + 1) / 2 - ta * (ta + 1) / 2, base, end_of(tb) - base});
        ta = tb;
    }
    size_t need = 1;
    for (const Band &b : bands) need = (size_t) b.n_out > need ? (size_t) b.n_out : need;
    int rc;
    const int n_slabs = bands.size() > 1 ? 2 : 1;
    for (int k = 0; k < n_slabs; k++) {
        if ((rc = W.dev(DS_SLAB + k, sizeof(double) * need))) return rc;
        if ((rc = W.pin(DS_HSLAB + k, sizeof(double) * need))) return rc;
    }
    hipStream_t s_kernel = nullptr, s_copy = nullptr;
    hipEvent_t k0[2] = {nullptr, nullptr}, k1[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
    bool ok = hipStreamCreateWithFlags(&s_kernel, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&s_copy, hipStreamNonBlocking) == hipSuccess;
    for (int k = 0; k < 2 && ok; k++)
        ok = hipEventCreate(&k0[k]) == hipSuccess && hipEventCreate(&k1[k]) == hipSuccess && hipEventCreate(&copied[k]) == hipSuccess;
    double kernel_ms = 0.0;
    // band b: its kernel waits until band b - 2 has left the slab, its copy waits for its kernel; the host hands band b - 1 to the
    // caller's buffer while band b computes
    auto collect = [&](size_t b) {
        const int k = (int) (b & 1);
        if (hipEventSynchronize(copied[k]) != hipSuccess) return false;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, k0[k], k1[k]) != hipSuccess) return false;
        kernel_ms += (double) ms;
        memcpy(tri_out + bands[b].out_base, W.at(DS_HSLAB + k), sizeof(double) * (size_t) bands[b].n_out);
        return true;
    };
    for (size_t b = 0; b < bands.size() && ok; b++) {
        const int k = (int) (b & 1);
        const Band &B = bands[b];
        if (b >= 2) ok = hipStreamWaitEvent(s_kernel, copied[k], 0) == hipSuccess;
        ok = ok && hipEventRecord(k0[k], s_kernel) == hipSuccess;
        if (ok) launch_tiles(metric, s_kernel, (unsigned) B.n_tiles, d_grid, (int) G, d_rows, (long long) n, B.tile_first, B.out_base, (double *) W.at(DS_SLAB + k));
        ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(k1[k], s_kernel) == hipSuccess;
        if (b >= 1) ok = ok && collect(b - 1);   // (frees the pinned buffer band b + 1 copies into)
        ok = ok && hipStreamWaitEvent(s_copy, k1[k], 0) == hipSuccess &&
             hipMemcpyAsync(W.at(DS_HSLAB + k), W.at(DS_SLAB + k), sizeof(double) * (size_t) B.n_out, hipMemcpyDeviceToHost, s_copy) == hipSuccess &&
             hipEventRecord(copied[k], s_copy) == hipSuccess;
    }
    if (ok && !bands.empty()) ok = collect(bands.size() - 1);
    if (s_kernel) (void) hipStreamSynchronize(s_kernel);
    if (s_copy) (void) hipStreamSynchronize(s_copy);
    for (int k = 0; k < 2; k++) {
        if (k0[k]) (void) hipEventDestroy(k0[k]);
        if (k1[k]) (void) hipEventDestroy(k1[k]);
        if (copied[k]) (void) hipEventDestroy(copied[k]);
    }
    if (s_kernel) (void) hipStreamDestroy(s_kernel);
    if (s_copy) (void) hipStreamDestroy(s_copy);
    if (!ok) { (void) hipGetLastError(); return SA_ENODEVICE; }
    if (kernel_ms_out) *kernel_ms_out = kernel_ms;
    return SA_OK;
}

// n pairs on the device, timed with HIP events; out is host memory
int pairs_from_device(int metric, const double *d_grid, int64_t G, const double *dA, const long long *d_ia, const double *dB,
                      const long long *d_ib, int64_t n, double *out, double *kernel_ms_out) {
    DevBuf d_out;
    int rc = d_out.alloc(sizeof(double) * (size_t) n);
    if (rc) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        if (e0) (void) hipEventDestroy(e0);
        return SA_ENODEVICE;
    }
    (void) hipEventRecord(e0, 0);
    launch_pairs(metric, 0, d_grid, (int) G, dA, d_ia, dB, d_ib, (long long) n, (double *) d_out.p);
    (void) hipEventRecord(e1, 0);
    float ms = 0.f;
    const bool ok = hipGetLastError() == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
                    hipEventElapsedTime(&ms, e0, e1) == hipSuccess &&
                    hipMemcpy(out, d_out.p, sizeof(double) * (size_t) n, hipMemcpyDeviceToHost) == hipSuccess;
    (void) hipEventDestroy(e0);
    (void) hipEventDestroy(e1);
    if (!ok) { (void) hipGetLastError(); return SA_ENODEVICE; }
    if (kernel_ms_out) *kernel_ms_out = (double) ms;
    return SA_OK;
}

// the row of a DP's nearest observed ancestor (impl/hdp.c:2600-2602, :2651-2658), -1 if there is none
int64_t resolve_row(const sa_hdp_state_t *s, int64_t dp) {
    while (dp >= 0 && !s->observed[dp]) dp = s->dp_parent[dp];
    return dp >= 0 ? s->row_of_dp[dp] : -1;
}

int check_state(const sa_hdp_state_t *s) {
    if (!s->splines_finalized || !s->post || !s->slope || s->n_observed < 1) return SA_ESTATE;
    return s->grid_length < 2 ? SA_EINVAL : SA_OK;
}

// ids -> rows; SA_EINVAL for an id outside [0, num_dps)
int resolve_rows(const sa_hdp_state_t *s, const int64_t *ids, int64_t n, std::vector<long long> &rows) {
    rows.resize((size_t) (n > 0 ? n : 0));
    for (int64_t i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= s->num_dps) return SA_EINVAL;
        const int64_t r = resolve_row(s, ids[i]);
        if (r < 0) return SA_ESTATE;
        rows[(size_t) i] = (long long) r;
    }
    return SA_OK;
}

// densities of s at n_x query points already on the device, for the DPs of `rows`: d_out[d * n_x + q]
int densities_on_device(const sa_hdp_state_t *s, const std::vector<long long> &rows, const double *d_x, int64_t n_x, DevBuf &d_out) {
    const size_t plane = sizeof(double) * (size_t) s->n_observed * (size_t) s->grid_length;
    const long long total = (long long) rows.size() * (long long) n_x;
    if (total >= (1ll << 31) * 256) return SA_EINVAL;
    DevBuf d_grid, d_post, d_slope, d_rows;
    int rc;
    if ((rc = d_grid.put(s->grid, sizeof(double) * (size_t) s->grid_length)) || (rc = d_post.put(s->post, plane)) ||
        (rc = d_slope.put(s->slope, plane)) || (rc = d_rows.put(rows.data(), sizeof(long long) * rows.size())) ||
        (rc = d_out.alloc(sizeof(double) * (size_t) total)))
        return rc;
    hipLaunchKernelGGL(k_hdp_density, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, 0, (const double *) d_grid.p, (int) s->grid_length,
                       (const double *) d_post.p, (const double *) d_slope.p, (const long long *) d_rows.p, (long long) rows.size(),
                       d_x, (long long) n_x, (double *) d_out.p);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void) hipGetLastError(); return SA_ENODEVICE; }
    return SA_OK;
}

}  // namespace

extern "C" void sa_hdp_distances_release(void) {
    std::lock_guard<std::mutex> guard(g_dist_ws.mu);
    g_dist_ws.release();
}

extern "C" int sa_hdp_distances(const double *grid, int64_t grid_length, const double *rows, int64_t n_rows, int metric, int device,
                                double *tri_out, double *kernel_ms_out) {
    if (!grid || !rows || !tri_out || grid_length < 2 || grid_length > (1 << 24) || n_rows < 1 || !known_metric(metric)) return SA_EINVAL;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (n_rows == 1) return SA_OK;   // (no pair: nothing to write)
    int rc = use_device(device);
    if (rc) return rc;
    SaScratch &W = g_dist_ws;
    std::lock_guard<std::mutex> guard(W.mu);
    const size_t plane = sizeof(double) * (size_t) n_rows * (size_t) grid_length;
    if ((rc = W.rebind(device)) || (rc = W.dev(DS_ROWS, plane)) || (rc = W.dev(DS_GRID, sizeof(double) * (size_t) grid_length))) return rc;
    if (hipMemcpy(W.at(DS_ROWS), rows, plane, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(W.at(DS_GRID), grid, sizeof(double) * (size_t) grid_length, hipMemcpyHostToDevice) != hipSuccess)
        return SA_ENODEVICE;
    return distances_from_device(W, (const double *) W.at(DS_GRID), grid_length, (const double *) W.at(DS_ROWS), n_rows, metric, tri_out,
                                 kernel_ms_out);
}

extern "C" int sa_hdp_distances_paired(const double *grid, int64_t grid_length, const double *a, const double *b, int64_t n, int metric,
                                       int device, double *out, double *kernel_ms_out) {
    if (!grid || !a || !b || !out || grid_length < 2 || grid_length > (1 << 24) || n < 1 || !known_metric(metric)) return SA_EINVAL;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    int rc = use_device(device);
    if (rc) return rc;
    const size_t plane = sizeof(double) * (size_t) n * (size_t) grid_length;
    DevBuf d_grid, d_a, d_b;
    if ((rc = d_grid.put(grid, sizeof(double) * (size_t) grid_length)) || (rc = d_a.put(a, plane)) || (rc = d_b.put(b, plane))) return rc;
    return pairs_from_device(metric, (const double *) d_grid.p, grid_length, (const double *) d_a.p, nullptr, (const double *) d_b.p, nullptr, n,
                             out, kernel_ms_out);
}

extern "C" int sa_hdp_state_densities(const sa_hdp_state_t *s, const int64_t *dp_ids, int64_t n_dps, const double *x, int64_t n_x,
                                      int device, double *out) {
    if (!s || !dp_ids || !x || !out || n_dps < 1 || n_x < 1) return SA_EINVAL;
    int rc = check_state(s);
    if (rc) return rc;
    std::vector<long long> rows;
    if ((rc = resolve_rows(s, dp_ids, n_dps, rows))) return rc;
    if ((rc = use_device(device))) return rc;
    DevBuf d_x, d_out;
    if ((rc = d_x.put(x, sizeof(double) * (size_t) n_x))) return rc;
    if ((rc = densities_on_device(s, rows, (const double *) d_x.p, n_x, d_out))) return rc;
    return hipMemcpy(out, d_out.p, sizeof(double) * (size_t) n_dps * (size_t) n_x, hipMemcpyDeviceToHost) == hipSuccess ? SA_OK : SA_ENODEVICE;
}

extern "C" int sa_hdp_state_distances(const sa_hdp_state_t *s, int metric, int device, double *tri_out, double *kernel_ms_out) {
    if (!s || !tri_out || !known_metric(metric)) return SA_EINVAL;
    const int rc = check_state(s);
    if (rc) return rc;
    return sa_hdp_distances(s->grid, s->grid_length, s->post, s->n_observed, metric, device, tri_out, kernel_ms_out);
}

extern "C" int sa_hdp_state_distance_pairs(const sa_hdp_state_t *s, int metric, const int64_t *dp1, const int64_t *dp2, int64_t n,
                                           int device, double *out) {
    if (!s || !dp1 || !dp2 || !out || n < 1 || !known_metric(metric)) return SA_EINVAL;
    int rc = check_state(s);
    if (rc) return rc;
    // get_dir_proc_distance (:2614-2636): equal ids are 0.0 without evaluating, otherwise the larger id's distribution comes first;
    // two different ids that resolve to one row are evaluated
    std::vector<int64_t> hi, lo, where;
    for (int64_t i = 0; i < n; i++) {
        if (dp1[i] < 0 || dp2[i] < 0 || dp1[i] >= s->num_dps || dp2[i] >= s->num_dps) return SA_EINVAL;
        if (dp1[i] == dp2[i]) continue;
        hi.push_back(dp1[i] > dp2[i] ? dp1[i] : dp2[i]);
        lo.push_back(dp1[i] > dp2[i] ? dp2[i] : dp1[i]);
        where.push_back(i);
    }
    std::vector<long long> r_hi, r_lo;
    if ((rc = resolve_rows(s, hi.data(), (int64_t) hi.size(), r_hi)) || (rc = resolve_rows(s, lo.data(), (int64_t) lo.size(), r_lo))) return rc;
    if ((rc = use_device(device))) return rc;
    for (int64_t i = 0; i < n; i++) out[i] = 0.0;
    if (where.empty()) return SA_OK;
    const size_t plane = sizeof(double) * (size_t) s->n_observed * (size_t) s->grid_length;
    DevBuf d_grid, d_post, d_hi, d_lo;
    if ((rc = d_grid.put(s->grid, sizeof(double) * (size_t) s->grid_length)) || (rc = d_post.put(s->post, plane)) ||
        (rc = d_hi.put(r_hi.data(), sizeof(long long) * r_hi.size())) || (rc = d_lo.put(r_lo.data(), sizeof(long long) * r_lo.size())))
        return rc;
    std::vector<double> got(where.size());
    if ((rc = pairs_from_device(metric, (const double *) d_grid.p, s->grid_length, (const double *) d_post.p, (const long long *) d_hi.p,
                                (const double *) d_post.p, (const long long *) d_lo.p, (int64_t) where.size(), got.data(), nullptr)))
        return rc;
    for (size_t k = 0; k < where.size(); k++) out[where[k]] = got[k];
    return SA_OK;
}

extern "C" int sa_hdp_state_compare(const sa_hdp_state_t *s1, const int64_t *dp1, const sa_hdp_state_t *s2, const int64_t *dp2, int64_t n,
                                    int metric, int device, double *out) {
    if (!s1 || !s2 || !dp1 || !dp2 || !out || n < 1 || !known_metric(metric)) return SA_EINVAL;
    int rc;
    if ((rc = check_state(s1)) || (rc = check_state(s2))) return rc;
    std::vector<long long> r1, r2;
    if ((rc = resolve_rows(s1, dp1, n, r1)) || (rc = resolve_rows(s2, dp2, n, r2))) return rc;
    if ((rc = use_device(device))) return rc;
    // distr_2[i] = dir_proc_density(hdp_2, grid_1[i]) (:2835-2839), then the metric on s1's grid
    const int64_t G = s1->grid_length;
    DevBuf d_grid, d_post, d_r1, d_second;
    if ((rc = d_grid.put(s1->grid, sizeof(double) * (size_t) G)) ||
        (rc = d_post.put(s1->post, sizeof(double) * (size_t) s1->n_observed * (size_t) G)) ||
        (rc = d_r1.put(r1.data(), sizeof(long long) * r1.size())))
        return rc;
    if ((rc = densities_on_device(s2, r2, (const double *) d_grid.p, G, d_second))) return rc;
    return pairs_from_device(metric, (const double *) d_grid.p, G, (const double *) d_post.p, (const long long *) d_r1.p,
                             (const double *) d_second.p, nullptr, n, out, nullptr);
}

extern "C" int sa_hdp_state_vs_gaussian(const sa_hdp_state_t *s, const int64_t *dp_ids, int64_t n, const double *mean, const double *sd,
                                        int device, sa_hdp_gauss_cmp_t *out, double *kernel_ms_out) {
    if (!s || !dp_ids || !mean || !sd || !out || n < 0 || n > 0x7fffffffll) return SA_EINVAL;
    for (int64_t i = 0; i < n; i++)
        if (dp_ids[i] < 0 || dp_ids[i] >= s->num_dps || !std::isfinite(mean[i]) || !std::isfinite(sd[i]) || !(sd[i] > 0.0)) return SA_EINVAL;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    int rc = check_state(s);
    if (rc) return rc;
    if (n == 0) return SA_OK;
    if ((rc = use_device(device))) return rc;
    std::vector<long long> rows((size_t) n);   // (no ancestor stands in for a DP that is not observed)
    for (int64_t i = 0; i < n; i++) rows[(size_t) i] = s->observed[dp_ids[i]] ? (long long) s->row_of_dp[dp_ids[i]] : -1;
    DevBuf d_grid, d_post, d_rows, d_mean, d_sd, d_out;
    if ((rc = d_grid.put(s->grid, sizeof(double) * (size_t) s->grid_length)) ||
        (rc = d_post.put(s->post, sizeof(double) * (size_t) s->n_observed * (size_t) s->grid_length)) ||
        (rc = d_rows.put(rows.data(), sizeof(long long) * rows.size())) || (rc = d_mean.put(mean, sizeof(double) * (size_t) n)) ||
        (rc = d_sd.put(sd, sizeof(double) * (size_t) n)) || (rc = d_out.alloc(sizeof(sa_hdp_gauss_cmp_t) * (size_t) n)))
        return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        if (e0) (void) hipEventDestroy(e0);
        return SA_ENODEVICE;
    }
    (void) hipEventRecord(e0, 0);
    hipLaunchKernelGGL(k_hdp_vs_gauss, dim3((unsigned) n), dim3(64), 0, 0, (const double *) d_grid.p, (int) s->grid_length,
                       (const double *) d_post.p, (const long long *) d_rows.p, (const double *) d_mean.p, (const double *) d_sd.p,
                       (sa_hdp_gauss_cmp_t *) d_out.p);
    (void) hipEventRecord(e1, 0);
    float ms = 0.f;
    const bool ok = hipGetLastError() == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess &&
                    hipMemcpy(out, d_out.p, sizeof(sa_hdp_gauss_cmp_t) * (size_t) n, hipMemcpyDeviceToHost) == hipSuccess;
    (void) hipEventDestroy(e0);
    (void) hipEventDestroy(e1);
    if (!ok) { (void) hipGetLastError(); return SA_ENODEVICE; }
    if (kernel_ms_out) *kernel_ms_out = (double) ms;
    return SA_OK;
}
