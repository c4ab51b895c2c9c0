// What the stages chained onto a finished batch share (sa_mea.hip, sa_calls.hip, sa_train.hip): the view of the batch's packed
// result records where sa_batch_run left them in HBM, the ambiguity table of the site and position calls, the printed units, the
// chunks the record kernels run over, and the scans.  The error macro and the layout of a call's device block are sa_scratch.h's.
#ifndef SA_CHAIN_H
#define SA_CHAIN_H

#include <algorithm>
#include <string>

#include "sa_scratch.h"

// A finished batch's records on its device: job j's are recs[first[j] .. first[j] + count[j]), in records of 16 bytes or (p8)
// of 8.  They are read where the run left them, or -- after host finalisation (SA_FLAG_EXACT) or sa_batch_release_device --
// uploaded again from the pinned host copy.
struct SaBatchView {
    const void *recs = nullptr;
    bool p8 = false;
    unsigned batch_flags = 0;   // the batch's creation flags (SA_FLAG_EXPECT_INTERNAL among them)
    int device = 0;
    int k = 0, n_alpha = 0;     // of the model the batch was created with: what a record's kmer_id is made of
    std::vector<long long> first, count, n_events;
};
// sa_hip.hip: SA_ESTATE for a batch that has not run (p8, batch_flags, device and the model's k and n_alpha are filled even
// then).  Which batches a stage accepts is the stage's own rule.
int sa_batch_view(sa_batch_t *b, SaBatchView *v);

// The table of a batch's ambiguity letters (sa_calls.hip), built at sa_batch_create.  Index i of job j names the letter
// ref[i + tail]: tail k - 1 for the sites (k-mer indices, the k-mer's last letter), 0 for the positions (reference positions).
// The device copy of the table goes back with the batch's working storage (sa_ambig_release_device), everything with the batch.
enum { SA_TAB_SITES = 0, SA_TAB_POSITIONS = 1, SA_TAB_N };
#define SA_POS_MAX_K 32   // the position calls hold a k-mer's digits in registers
struct SaAmbigTab;
int sa_ambig_build(const sa_model_t *m, const sa_job_t *jobs, int64_t n_jobs, const char *const *ambig, int tail, SaAmbigTab **out);
long long sa_ambig_count(const SaAmbigTab *s);   // 0 for NULL
void sa_ambig_release_device(SaAmbigTab *s);     // NULL: nothing
void sa_ambig_free(SaAmbigTab *s);               // NULL: nothing
// sa_hip.hip: a finished batch's table `which` (SA_ESTATE: created without the table's flag, or not run)
int sa_batch_ambig(sa_batch_t *b, int which, SaAmbigTab **tab, int64_t *n_jobs);

// The accumulate-and-normalise half of the site calls of a finished batch, left on its device (sa_calls.hip): what
// sa_batch_site_calls compacts and copies out and what sa_call_scores_add_batch (sa_scores.hip) labels in place.  Site s of job j,
// site_off[j] <= s < site_off[j + 1], in ascending x: units[s * stride + e] and prob[s * stride + e] for letter e of the site's kind
// (prob 0 where the units sum to 0: such a site is not a call), count[j] the job's sites with a non-zero sum.  With ns == 0 nothing
// is on the device.  sa_site_fold_run takes the lock of the site calls' scratch and starts its timed region (ws->time_begin), which
// the caller ends after its own launches; sa_site_fold_release gives the lock back with the device block; release after a failed
// run is allowed.
struct SaSiteFold {
    size_t nj = 0, stride = 1, ns = 0;
    int device = 0;
    double kernel_ms = 0.0;
    const long long *site_off = nullptr;           // device, nj + 1
    const unsigned char *kind = nullptr;           // device, per site
    const unsigned long long *units = nullptr;     // device
    const double *prob = nullptr;
    const int *count = nullptr;
    const int *h_x = nullptr;                      // host, per site: its k-mer index x
    const long long *h_site_off = nullptr;         // host, nj + 1
    std::vector<std::string> letters;              // host, per kind: the sorted letters
    SaScratch *ws = nullptr;
    char *d = nullptr;                             // the fold's device block (g_sa_pool)
    char *d_recs = nullptr;                        // the records of sa_site_calls_records (g_sa_pool); a batch's stay the batch's
    std::unique_lock<std::mutex> guard;
};
int sa_site_fold_run(sa_batch_t *b, SaSiteFold *F);
void sa_site_fold_release(SaSiteFold *F, bool failed);

// The position fold of a finished batch, left on its device (sa_calls.hip): what sa_batch_position_calls copies out and what
// sa_snp_marginals_add_batch (sa_marginals.hip) reads in place.  Record r of job j, off[j] <= r < off[j + 1], in position order:
// slot[r] (the batch-wide index of the position), n_rows[r], prob[r * stride + e] for letter e of the slot's kind.
// sa_pos_fold_run takes the lock of the position calls' scratch and sa_pos_fold_release gives it back with the device blocks;
// release after a failed run is allowed.
struct SaPosFold {
    size_t nj = 0, stride = 1, n_kept = 0;
    int device = 0;
    double kernel_ms = 0.0;
    std::vector<long long> count;          // per job: its records
    std::vector<long long> h_off;          // nj + 1
    const long long *off = nullptr;        // device, nj + 1
    const int *slot = nullptr, *xmin = nullptr, *xmax = nullptr;   // xmin / xmax: per job, of a job with records only
    const unsigned *n_rows = nullptr;
    const double *sum = nullptr, *prob = nullptr;
    const unsigned char *kind = nullptr;   // device, per slot
    const int *h_x = nullptr;              // host, per slot: its index in the job's ref
    std::vector<signed char> acgt;         // host, kind * 4 + l: which letter of the kind is "ACGT"[l], -1 none
    SaAmbigTab *tab = nullptr;
    char *d = nullptr;                     // the call's device blocks (g_sa_pool)
    unsigned long long *d_ent = nullptr;
    char *d_recs = nullptr;                // the records of sa_position_calls_records (g_sa_pool); a batch's stay the batch's
    std::unique_lock<std::mutex> guard;
};
int sa_pos_fold_run(sa_batch_t *b, SaPosFold *F);
void sa_pos_fold_release(SaPosFold *F, bool failed);

// The posterior the TSV prints, "%f" of prob_e7 / 1e7, in integers of 1e-6: a decimal rounding of a binary double.  Only a
// last digit of 5 can tie; then the sign of q * 1e7 - prob_e7 (one fma, exact in sign) says on which side of the tie the
// double q = prob_e7 / 1e7 lies, and an exact tie goes to even as glibc's printf does.  tests/test_host_mea.py checks every
// value of prob_e7 against Python's "%f".
__host__ __device__ static inline long long sa_printed_units(long long prob_e7) {
    long long k = prob_e7 / 10;
    const long long rem = prob_e7 % 10;
    if (rem > 5) {
        k++;
    } else if (rem == 5) {
        const double q = (double) prob_e7 / 1e7;
        const double side = fma(q, 1e7, -(double) prob_e7);
        if (side > 0 || (side == 0 && (k & 1))) k++;
    }
    return k;
}

// One block of a record kernel: n records of one job from `first` on
#define SA_CHAIN_CHUNK 4096
struct SaRecChunk {
    long long first;   // first record of the chunk in the view's records
    long long local;   // ordinal of that record (sa_view_chunks)
    int n, job;
};
// Every job's records cut into chunks of at most chunk_records.  The ordinals run through the view's records from
// ordinal_base on, or restart at 0 in every job (SA_ORDINAL_PER_JOB).
#define SA_ORDINAL_PER_JOB (-1ll)
static inline std::vector<SaRecChunk> sa_view_chunks(const SaBatchView &V, long long chunk_records, long long ordinal_base) {
    std::vector<SaRecChunk> chunks;
    long long run = ordinal_base == SA_ORDINAL_PER_JOB ? 0 : ordinal_base;
    for (size_t j = 0; j < V.count.size(); j++) {
        for (long long c = 0; c < V.count[j]; c += chunk_records)
            chunks.push_back(SaRecChunk{V.first[j] + c, run + c, (int) std::min(chunk_records, V.count[j] - c), (int) j});
        if (ordinal_base != SA_ORDINAL_PER_JOB) run += V.count[j];
    }
    return chunks;
}

// inclusive scan over the 64 lanes of a wave
template <class T>
__device__ __forceinline__ T sa_wave_incl_scan(T v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// Exclusive scan of get(0 .. n) into off[0 .. n], by ONE block of SA_SCAN_THREADS threads: each thread sums a contiguous run of
// ceil(n / SA_SCAN_THREADS) elements, the run sums are scanned across the block (wave scans, then the waves' totals through
// LDS), and each thread writes its run's offsets.
#define SA_SCAN_THREADS 1024
template <class Get, class Idx>
__device__ __forceinline__ void sa_block_excl_scan(Get get, long long *__restrict__ off, Idx n) {
    __shared__ long long wave_tot[SA_SCAN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const Idx per = (n + SA_SCAN_THREADS - 1) / SA_SCAN_THREADS;
    const Idx a = min(n, (Idx) t * per), e = min(n, a + per);
    long long mine = 0;
    for (Idx i = a; i < e; i++) mine += get(i);
    const long long incl = sa_wave_incl_scan(mine, lane);
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    long long before = 0;
    for (int q = 0; q < wv; q++) before += wave_tot[q];
    long long run = before + incl - mine;
    for (Idx i = a; i < e; i++) { off[i] = run; run += get(i); }
    if (t == SA_SCAN_THREADS - 1) off[n] = before + incl;   // (the last thread's inclusive sum is the total)
}

#endif
