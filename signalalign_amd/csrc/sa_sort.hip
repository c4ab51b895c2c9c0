// Device-wide sort of 64-bit keys on gfx950: a least-significant-digit radix sort with 8-bit digits, keys only, ascending.
// It exists for sa_scores.hip, whose AUC over 10^7 - 10^8 scores is a sort; every other sort of the library is a bucket of tens of
// entries or a bitonic network in LDS.
//
// A tile is SA_SORT_TILE keys (256 threads x 16), one workgroup per tile.  Workgroups are ordered by kernel boundaries only: no
// workgroup waits for another one inside a kernel.
//
// Kernels of a sort of n keys:
//   k_sort_digits       the counts of all eight digits over the whole input (LDS atomics, one global atomic per non-empty bin
//                       and workgroup).  They come back to the host: a digit with one non-empty bin orders nothing, and its
//                       pass is skipped
// and per remaining digit, from the least significant one up:
//   k_sort_hist         per tile the counts of the digit's 256 values, written digit-major: hist[value * n_tiles + tile]
//   k_sort_scan_reduce  the sums of blocks of 4096 entries of hist
//   k_sort_scan_top     ONE workgroup: exclusive scan of those sums
//   k_sort_scan_apply   every block of hist scanned in place from its sum on: hist[value * n_tiles + tile] is now where the
//                       tile's keys of that value start in the output
//   k_sort_scatter      the tile's keys ranked inside the tile and written out.  A pass must keep the order of the pass before it
//                       among keys of equal digit (only wholly equal keys may trade places), so the rank is a stable one: per
//                       wave and round of 64 keys the lanes of equal digit find each other by eight ballots, their rank is
//                       the wave's running count of the digit (LDS) plus the peers in lower lanes; the waves' counts are scanned
//                       across the waves and the values.  The keys go through LDS in rank order, so that neighbouring lanes
//                       write neighbouring addresses of a value's run
// The passes alternate between `tmp` and `out` so that the last one lands in `out`; the input is only read.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>
#include <string.h>

#include "sa_internal.h"
#include "sa_chain.h"
#include "sa_sort.h"

#define SORT_THREADS 256
#define SORT_WAVES (SORT_THREADS / 64)
#define SORT_ITEMS 16
#define SORT_SCAN_CHUNK 4096   // entries of hist per workgroup of the scan: 256 threads x 16
static_assert(SORT_THREADS * SORT_ITEMS == SA_SORT_TILE, "a tile is one workgroup's keys");

__global__ __launch_bounds__(SORT_THREADS) void k_sort_digits(const unsigned long long *__restrict__ keys, unsigned n,
                                                              unsigned *__restrict__ cnt) {
    __shared__ unsigned h[8 * 256];
    for (int i = threadIdx.x; i < 8 * 256; i += SORT_THREADS) h[i] = 0;
    __syncthreads();
    for (size_t i = (size_t) blockIdx.x * SORT_THREADS + threadIdx.x; i < n; i += (size_t) gridDim.x * SORT_THREADS) {
        const unsigned long long k = keys[i];
#pragma unroll
        for (int b = 0; b < 8; b++) atomicAdd(&h[b * 256 + (int) ((k >> (8 * b)) & 255ull)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 8 * 256; i += SORT_THREADS)
        if (h[i]) atomicAdd(&cnt[i], h[i]);
}

__global__ __launch_bounds__(SORT_THREADS) void k_sort_hist(const unsigned long long *__restrict__ keys, unsigned n, int shift,
                                                            unsigned n_tiles, unsigned *__restrict__ hist) {
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t) blockIdx.x * SA_SORT_TILE;
#pragma unroll
    for (int i = 0; i < SORT_ITEMS; i++) {
        const size_t q = base + (size_t) i * SORT_THREADS + threadIdx.x;
        if (q < n) atomicAdd(&h[(int) ((keys[q] >> shift) & 255ull)], 1u);
    }
    __syncthreads();
    hist[(size_t) threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// the sum of v over the workgroup's 256 threads, in every thread
__device__ __forceinline__ unsigned sort_block_sum(unsigned v, unsigned *wave_tot) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned s = 0;
    for (int q = 0; q < SORT_WAVES; q++) s += wave_tot[q];
    return s;
}

// v's exclusive prefix over the workgroup's 256 threads
__device__ __forceinline__ unsigned sort_block_excl(unsigned v, unsigned *wave_tot) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned incl = sa_wave_incl_scan(v, lane);
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    unsigned before = 0;
    for (int q = 0; q < wv; q++) before += wave_tot[q];
    return before + incl - v;
}

__global__ __launch_bounds__(SORT_THREADS) void k_sort_scan_reduce(const unsigned *__restrict__ hist, size_t n_ent,
                                                                   unsigned *__restrict__ bsum) {
    __shared__ unsigned wave_tot[SORT_WAVES];
    const size_t base = (size_t) blockIdx.x * SORT_SCAN_CHUNK;
    unsigned v = 0;
    for (int i = 0; i < SORT_SCAN_CHUNK / SORT_THREADS; i++) {
        const size_t q = base + (size_t) i * SORT_THREADS + threadIdx.x;
        if (q < n_ent) v += hist[q];
    }
    const unsigned s = sort_block_sum(v, wave_tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = s;
}

__global__ __launch_bounds__(SA_SCAN_THREADS) void k_sort_scan_top(const unsigned *__restrict__ bsum, long long *__restrict__ boff,
                                                                   unsigned nb) {
    sa_block_excl_scan([bsum](unsigned i) { return (long long) bsum[i]; }, boff, nb);
}

__global__ __launch_bounds__(SORT_THREADS) void k_sort_scan_apply(unsigned *__restrict__ hist, size_t n_ent,
                                                                  const long long *__restrict__ boff) {
    __shared__ unsigned wave_tot[SORT_WAVES];
    const int per = SORT_SCAN_CHUNK / SORT_THREADS;
    const size_t base = (size_t) blockIdx.x * SORT_SCAN_CHUNK + (size_t) threadIdx.x * per;
    unsigned v[SORT_SCAN_CHUNK / SORT_THREADS];
    unsigned mine = 0;
#pragma unroll
    for (int i = 0; i < per; i++) {
        v[i] = base + i < n_ent ? hist[base + i] : 0u;
        mine += v[i];
    }
    unsigned run = (unsigned) boff[blockIdx.x] + sort_block_excl(mine, wave_tot);
#pragma unroll
    for (int i = 0; i < per; i++) {
        if (base + i < n_ent) hist[base + i] = run;
        run += v[i];
    }
}

__global__ __launch_bounds__(SORT_THREADS) void k_sort_scatter(const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out,
                                                               unsigned n, int shift, unsigned n_tiles, const unsigned *__restrict__ offs) {
    __shared__ unsigned long long skey[SA_SORT_TILE];
    __shared__ unsigned wcnt[SORT_WAVES][256];   // a wave's count of every value; then the counts of the waves before it
    __shared__ unsigned toff[256];               // where a value's run starts in the tile
    __shared__ unsigned gofs[256];               // where it starts in the output, less toff
    __shared__ unsigned wave_tot[SORT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t tbase = (size_t) blockIdx.x * SA_SORT_TILE;
    const unsigned tn = (unsigned) min((size_t) SA_SORT_TILE, (size_t) n - tbase);
    for (int w = 0; w < SORT_WAVES; w++) wcnt[w][tid] = 0;
    __syncthreads();
    unsigned long long key[SORT_ITEMS];
    unsigned rk[SORT_ITEMS];
    volatile unsigned *mine = wcnt[wv];
#pragma unroll
    for (int i = 0; i < SORT_ITEMS; i++) {
        const unsigned pos = (unsigned) (wv * 64 * SORT_ITEMS + i * 64 + lane);   // rank order is position order: wave, round, lane
        const bool valid = pos < tn;
        const unsigned long long k = valid ? in[tbase + pos] : ~0ull;
        const unsigned d = (unsigned) ((k >> shift) & 255ull);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const unsigned prev = mine[d];
        rk[i] = prev + (unsigned) __popcll(peers & ((1ull << lane) - 1ull));
        __builtin_amdgcn_wave_barrier();   // (every lane of the wave has read the count before the first of the peers moves it on)
        if (valid && lane == __ffsll((long long) peers) - 1) mine[d] = prev + (unsigned) __popcll(peers);
        __builtin_amdgcn_wave_barrier();
        key[i] = k;
    }
    __syncthreads();
    {   // thread tid is value tid: the waves' counts into the counts before each wave, the value's total scanned over the values
        unsigned total = 0;
        for (int w = 0; w < SORT_WAVES; w++) {
            const unsigned c = wcnt[w][tid];
            wcnt[w][tid] = total;
            total += c;
        }
        const unsigned at = sort_block_excl(total, wave_tot);
        toff[tid] = at;
        gofs[tid] = offs[(size_t) tid * n_tiles + blockIdx.x] - at;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SORT_ITEMS; i++) {
        const unsigned pos = (unsigned) (wv * 64 * SORT_ITEMS + i * 64 + lane);
        const unsigned d = (unsigned) ((key[i] >> shift) & 255ull);
        const unsigned p = toff[d] + wcnt[wv][d] + rk[i];
        if (pos < tn && p < SA_SORT_TILE) skey[p] = key[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SORT_ITEMS; i++) {
        const unsigned q = (unsigned) (i * SORT_THREADS + tid);
        if (q >= tn) continue;
        const unsigned long long k = skey[q];
        const unsigned dst = gofs[(unsigned) ((k >> shift) & 255ull)] + q;
        if (dst < n) out[dst] = k;   // (always, when the counts are the tile's: the guard keeps a wrong count inside the array)
    }
}

struct SortWork {
    size_t n_tiles, n_ent, nb, o_digits, o_hist, o_bsum, o_boff, bytes;
};
static SortWork sort_work(size_t n) {
    SortWork w;
    w.n_tiles = n ? (n + SA_SORT_TILE - 1) / SA_SORT_TILE : 1;
    w.n_ent = 256 * w.n_tiles;
    w.nb = (w.n_ent + SORT_SCAN_CHUNK - 1) / SORT_SCAN_CHUNK;
    SaLayout L;
    w.o_digits = L.add(4 * 8 * 256);
    w.o_hist = L.add(4 * w.n_ent);
    w.o_bsum = L.add(4 * w.nb);
    w.o_boff = L.add(8 * (w.nb + 1));
    w.bytes = L.end;
    return w;
}

size_t sa_sort_work_bytes(size_t n) { return sort_work(n).bytes; }

int sa_sort_u64_device(const uint64_t *d_in, size_t n, uint64_t *d_out, uint64_t *d_tmp, char *d_work, int *passes_out) {
    if (passes_out) *passes_out = 0;
    if (n == 0) return SA_OK;
    if (n > (size_t) INT32_MAX) return SA_EUNSUPPORTED;
    int rc = SA_OK;
    const SortWork w = sort_work(n);
    const unsigned un = (unsigned) n, nt = (unsigned) w.n_tiles;
    unsigned *digits = (unsigned *) (d_work + w.o_digits), *hist = (unsigned *) (d_work + w.o_hist), *bsum = (unsigned *) (d_work + w.o_bsum);
    long long *boff = (long long *) (d_work + w.o_boff);
    unsigned h_digits[8 * 256];
    int shifts[8], n_pass = 0;
    const unsigned long long *src = (const unsigned long long *) d_in;
    SA_HIP_GOTO_DONE(hipMemsetAsync(digits, 0, 4 * 8 * 256, 0));
    hipLaunchKernelGGL(k_sort_digits, dim3((unsigned) std::min((n + SORT_THREADS - 1) / SORT_THREADS, (size_t) 2048)), dim3(SORT_THREADS), 0, 0,
                       src, un, digits);
    SA_HIP_GOTO_DONE(hipGetLastError());
    SA_HIP_GOTO_DONE(hipMemcpy(h_digits, digits, sizeof h_digits, hipMemcpyDeviceToHost));
    for (int b = 0; b < 8; b++) {
        int used = 0;
        for (int v = 0; v < 256; v++) used += h_digits[b * 256 + v] != 0;
        if (used > 1) shifts[n_pass++] = 8 * b;
    }
    if (passes_out) *passes_out = n_pass;
    if (n_pass == 0) {   // (all keys are equal)
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d_out, d_in, 8 * n, hipMemcpyDeviceToDevice, 0));
        return SA_OK;
    }
    for (int i = 0; i < n_pass; i++) {
        unsigned long long *dst = (unsigned long long *) (((n_pass - 1 - i) & 1) ? d_tmp : d_out);
        hipLaunchKernelGGL(k_sort_hist, dim3(nt), dim3(SORT_THREADS), 0, 0, src, un, shifts[i], nt, hist);
        hipLaunchKernelGGL(k_sort_scan_reduce, dim3((unsigned) w.nb), dim3(SORT_THREADS), 0, 0, (const unsigned *) hist, w.n_ent, bsum);
        hipLaunchKernelGGL(k_sort_scan_top, dim3(1), dim3(SA_SCAN_THREADS), 0, 0, (const unsigned *) bsum, boff, (unsigned) w.nb);
        hipLaunchKernelGGL(k_sort_scan_apply, dim3((unsigned) w.nb), dim3(SORT_THREADS), 0, 0, hist, w.n_ent, (const long long *) boff);
        hipLaunchKernelGGL(k_sort_scatter, dim3(nt), dim3(SORT_THREADS), 0, 0, src, dst, un, shifts[i], nt, (const unsigned *) hist);
        src = dst;
    }
    SA_HIP_GOTO_DONE(hipGetLastError());
done:
    return rc;
}

// the timing events and the lock around them; the call's device block comes from the caching allocator and goes back to it
static SaScratch g_sort_ws;

extern "C" int sa_sort_u64(const uint64_t *keys, int64_t n, uint64_t *sorted_out, int device, double *kernel_ms_out) {
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (n < 0 || (n > 0 && (!keys || !sorted_out))) return SA_EINVAL;
    if (const int rc = sa_device_check(device)) return rc;
    if (n > (int64_t) INT32_MAX) return SA_EUNSUPPORTED;
    if (n == 0) return SA_OK;
    const size_t sn = (size_t) n;
    SaLayout L;   // [in | out | tmp | work]
    const size_t o_in = L.add(8 * sn), o_out = L.add(8 * sn), o_tmp = L.add(8 * sn), o_work = L.add(sa_sort_work_bytes(sn));
    SaScratch &W = g_sort_ws;
    std::lock_guard<std::mutex> guard(W.mu);
    int rc = W.rebind(device);
    if (rc != SA_OK) return rc;
    char *d = nullptr;
    float kms = 0;
    if (g_sa_pool.get(SaPool::DEVICE, (void **) &d, L.end, device) != hipSuccess) return SA_ENOMEM;
    SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_in, keys, 8 * sn, hipMemcpyHostToDevice, 0));
    SA_HIP_GOTO_DONE(W.time_begin());
    rc = sa_sort_u64_device((const uint64_t *) (d + o_in), sn, (uint64_t *) (d + o_out), (uint64_t *) (d + o_tmp), d + o_work, nullptr);
    if (rc != SA_OK) goto done;
    SA_HIP_GOTO_DONE(W.time_end());
    SA_HIP_GOTO_DONE(hipMemcpy(sorted_out, d + o_out, 8 * sn, hipMemcpyDeviceToHost));
    SA_HIP_GOTO_DONE(W.time_ms(&kms));
    if (kernel_ms_out) *kernel_ms_out = (double) kms;
done:
    if (rc != SA_OK) (void) hipStreamSynchronize(0);   // (a failed call may have left work queued on its block)
    g_sa_pool.put(SaPool::DEVICE, d);
    return rc;
}
