// Site calls scored against known truth on gfx950 -- the numbers of visualization/plot_variant_accuracy.py:44-175 over
// generate_labels / generate_labels2 (src/signalalign/variantCaller.py:413-442); include/signalalign_hip.h has the definitions.
//
// The accumulator holds one append-only array of 64-bit keys per (level, read strand, letter, class) in HBM: a score in [0, 1] as
// the bit pattern of its double, which orders as an unsigned integer.  The host holds the arrays' lengths: a checkpoint is a copy
// of the lengths, a rollback puts them back.  An array grows by doubling through g_sa_pool.
//
// Kernels of an add chained onto a batch, after the fold that sa_batch_site_calls shares (SaSiteFold):
//   k_score_sites   one wave per job, 64 sites at a time: a site with a non-zero total and the accumulator's letters gets its true
//                   letter (the job's label, or a binary search of the sorted positions table: sc_site_label, sa_site_label.h,
//                   which sa_callq.hip shares); per (letter, class) the lanes that append are counted by ballot, ONE integer atomic moves the array's cursor for all of them, and each
//                   writes its key at the cursor plus its rank.  The order inside an array is whatever the atomics hand out:
//                   finish sorts, so nothing reported depends on it
//   k_score_reads   one lane per (job with a label, letter): the site probabilities added serially in the reference's order, the
//                   mean appended
// Every array is grown, before the launch, by the most the add can append (the sites of its strand's jobs), so no count has to come
// back between the kernels; the cursors come back once, at the end.
// Kernels of finish, per (level, letter), after sa_sort_u64_device of its four arrays (t / c x positive / negative) into scratch:
//   k_score_auc     one thread per positive: lower and upper bound in both strands' sorted negatives; 64-bit integer sums reduced
//                   over the wave and added with one atomic per wave to the strand's group and to the group of both
//   k_score_counts  one thread per grid point (and one for the threshold): scores >= t in each of the four arrays, per group
#include <hip/hip_runtime.h>

#include <inttypes.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "sa_internal.h"
#include "sa_chain.h"
#include "sa_sort.h"
#include "sa_site_label.h"

#define SC_LEVELS 3
#define SC_MAX_ADD (1ll << 30)
#define SC_MAX_ARRAY ((long long) INT32_MAX)
__host__ __device__ static inline int sc_array(int nl, int level, int strand, int letter, int cls) {
    return ((level * 2 + strand) * nl + letter) * 2 + cls;   // cls 1: positive
}
// a score's key: its bit pattern, -0.0 as +0.0
__device__ static inline unsigned long long sc_key_dev(double v) { return v == 0.0 ? 0ull : (unsigned long long) __double_as_longlong(v); }
static inline unsigned long long sc_key_host(double v) {
    unsigned long long u = 0;
    if (v != 0.0) memcpy(&u, &v, 8);
    return u;
}

struct ScDev {   // what the appending kernels share
    unsigned long long *const *ptr;    // per array
    const unsigned *cap;               // per array: entries it has room for
    unsigned *cur;                     // per array: entries it holds
    unsigned long long *misc;          // [0] unlabelled calls, [1] sites of other letters
    ScTruth T;                         // the positions table
    int nl;
};

__global__ __launch_bounds__(64) void k_score_sites(const ScJob *__restrict__ jobs, const long long *__restrict__ site_off,
                                                    const unsigned char *__restrict__ kind, const unsigned char *__restrict__ kind_ok,
                                                    const int *__restrict__ x_of_site, const unsigned long long *__restrict__ units,
                                                    const double *__restrict__ prob, int stride, ScDev D) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const ScJob J = jobs[j];
    const long long s0 = site_off[j], s1 = site_off[j + 1];
    unsigned long long n_unl = 0, n_oth = 0;
    for (long long base = s0; base < s1; base += 64) {
        const long long s = base + lane;
        int tl;
        const int what = sc_site_label(J, s < s1, s, kind, kind_ok, x_of_site, units, stride, D.T, &tl);
        n_oth += (unsigned long long) __popcll(__ballot(what == SC_SITE_OTHER));
        n_unl += (unsigned long long) __popcll(__ballot(what == SC_SITE_UNLABELLED));
        const bool lab = what == SC_SITE_LABELLED;
        if (!__any(lab)) continue;
        for (int l = 0; l < D.nl; l++)
            for (int cls = 0; cls < 2; cls++) {
                const bool mine = lab && ((l == tl) == (cls == 1));
                const unsigned long long m = __ballot(mine);
                if (m == 0) continue;
                const int a = sc_array(D.nl, 0, J.strand, l, cls), leader = __ffsll((long long) m) - 1;
                unsigned at = 0;
                if (lane == leader) at = atomicAdd(&D.cur[a], (unsigned) __popcll(m));
                at = __shfl(at, leader);
                if (mine) {
                    const unsigned idx = at + (unsigned) __popcll(m & ((1ull << lane) - 1ull));
                    if (idx < D.cap[a]) D.ptr[a][idx] = sc_key_dev(prob[(size_t) s * (size_t) stride + (size_t) l]);
                }
            }
    }
    if (lane == 0) {
        if (n_unl) atomicAdd(&D.misc[0], n_unl);
        if (n_oth) atomicAdd(&D.misc[1], n_oth);
    }
}

__global__ __launch_bounds__(256) void k_score_reads(const ScJob *__restrict__ jobs, int nj, const long long *__restrict__ site_off,
                                                     const unsigned char *__restrict__ kind, const unsigned char *__restrict__ kind_ok,
                                                     const unsigned long long *__restrict__ units, const double *__restrict__ prob,
                                                     int stride, ScDev D) {
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    const int j = (int) (t / D.nl), l = (int) (t % D.nl);
    if (j >= nj) return;
    const ScJob J = jobs[j];
    if (J.true_letter < 0) return;
    const long long s0 = site_off[j], s1 = site_off[j + 1];
    double sum = 0.0;
    long long n = 0;
    for (long long q = 0; q < s1 - s0; q++) {
        const long long s = J.ascending ? s0 + q : s1 - 1 - q;
        if (!kind_ok[kind[s]] || !sc_site_live(units, s, stride)) continue;
        sum += prob[(size_t) s * (size_t) stride + (size_t) l];
        n++;
    }
    if (n == 0) return;
    const int a = sc_array(D.nl, 1, J.strand, l, l == J.true_letter ? 1 : 0);
    const unsigned idx = atomicAdd(&D.cur[a], 1u);
    if (idx < D.cap[a]) D.ptr[a][idx] = sc_key_dev(sum / (double) n);
}

// out[ps] and out[2] += sum over the positives p of strand ps of (negatives < p) + (negatives <= p)
__global__ __launch_bounds__(256) void k_score_auc(const unsigned long long *__restrict__ pos, unsigned long long n_pos,
                                                   const unsigned long long *__restrict__ neg_t, unsigned long long n_neg_t,
                                                   const unsigned long long *__restrict__ neg_c, unsigned long long n_neg_c, int ps,
                                                   unsigned long long *__restrict__ out) {
    unsigned long long same = 0, all = 0;
    for (unsigned long long i = (unsigned long long) blockIdx.x * blockDim.x + threadIdx.x; i < n_pos; i += (unsigned long long) gridDim.x * blockDim.x) {
        const unsigned long long p = pos[i];
        const unsigned long long vt = n_neg_t ? sc_bound<false>(neg_t, n_neg_t, p) + sc_bound<true>(neg_t, n_neg_t, p) : 0ull;
        const unsigned long long vc = n_neg_c ? sc_bound<false>(neg_c, n_neg_c, p) + sc_bound<true>(neg_c, n_neg_c, p) : 0ull;
        same += ps == 0 ? vt : vc;
        all += vt + vc;
    }
    for (int o = 32; o > 0; o >>= 1) {
        same += __shfl_xor(same, o);
        all += __shfl_xor(all, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (same) atomicAdd(&out[ps], same);
        if (all) atomicAdd(&out[2], all);
    }
}

struct ScFour {   // the four sorted arrays of one (level, letter): index strand * 2 + cls
    const unsigned long long *a[4];
    unsigned long long n[4];
};

// ge[(g * 2 + cls) * (n_bins + 2) + k] = scores of group g and class cls that are >= t_k; k == n_bins + 1 is the threshold
__global__ __launch_bounds__(256) void k_score_counts(ScFour F, int n_bins, unsigned long long thr_key, long long *__restrict__ ge) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n_bins + 1) return;
    unsigned long long key = thr_key;
    if (k <= n_bins) {
        const double t = (double) k / (double) n_bins;
        key = sc_key_dev(t);
    }
    long long c[4];
    for (int q = 0; q < 4; q++) c[q] = F.n[q] ? (long long) (F.n[q] - sc_bound<false>(F.a[q], F.n[q], key)) : 0ll;
    const size_t w = (size_t) n_bins + 2;
    for (int cls = 0; cls < 2; cls++) {
        ge[(size_t) (0 * 2 + cls) * w + (size_t) k] = c[0 * 2 + cls];
        ge[(size_t) (1 * 2 + cls) * w + (size_t) k] = c[1 * 2 + cls];
        ge[(size_t) (2 * 2 + cls) * w + (size_t) k] = c[0 * 2 + cls] + c[1 * 2 + cls];
    }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------
// room for `need` entries in array a; what it holds is kept
static int sc_grow(sa_call_scores *s, ScArray &A, size_t need) {
    if (need <= A.cap) return SA_OK;
    const size_t cap = std::max(std::max(need, 2 * A.cap), (size_t) 1024);
    unsigned long long *d = nullptr;
    if (g_sa_pool.get(SaPool::DEVICE, (void **) &d, 8 * cap, s->device) != hipSuccess) return SA_ENOMEM;
    if (A.n && (hipMemcpyAsync(d, A.d, 8 * A.n, hipMemcpyDeviceToDevice, 0) != hipSuccess || hipStreamSynchronize(0) != hipSuccess)) {
        g_sa_pool.put(SaPool::DEVICE, d);
        return SA_ENODEVICE;
    }
    if (A.d) g_sa_pool.put(SaPool::DEVICE, A.d);
    A.d = d;
    A.cap = cap;
    return SA_OK;
}

extern "C" void sa_call_scores_destroy(sa_call_scores_t *s) {
    if (!s) return;
    if (s->device >= 0) (void) hipSetDevice(s->device);
    for (ScArray &A : s->arr)
        if (A.d) g_sa_pool.put(SaPool::DEVICE, A.d);
    if (s->d_truth) g_sa_pool.put(SaPool::DEVICE, s->d_truth);
    if (s->e0) (void) hipEventDestroy(s->e0);
    if (s->e1) (void) hipEventDestroy(s->e1);
    delete s;
}

extern "C" int sa_call_scores_create(sa_call_scores_t **out, const char *letters, int32_t n_bins, double threshold,
                                     const sa_truth_site_t *truth, int64_t n_truth, int device) {
    if (!out) return SA_EINVAL;
    *out = nullptr;
    if (!letters || n_bins < 1 || threshold != threshold || n_truth < 0 || (n_truth > 0 && !truth)) return SA_EINVAL;
    const size_t nl = strlen(letters);
    if (nl < 2 || nl > SA_SITE_MAX_LETTERS) return SA_EINVAL;
    for (size_t i = 1; i < nl; i++)
        if ((unsigned char) letters[i - 1] >= (unsigned char) letters[i]) return SA_EINVAL;
    // the table in key order, the first of the lines that name one key (stable sort, then the first of each run)
    std::vector<unsigned long long> tkey;
    std::vector<signed char> tlet;
    {
        std::vector<std::pair<unsigned long long, signed char>> v((size_t) n_truth);
        for (int64_t i = 0; i < n_truth; i++) {
            const sa_truth_site_t &t = truth[i];
            const char *at = t.change_to ? strchr(letters, t.change_to) : nullptr;
            if (!at || t.contig < 0 || t.contig >= SC_MAX_CONTIG || t.pos < 0 || t.pos >= SC_MAX_POS ||
                (t.mapped_strand != 0 && t.mapped_strand != 1))
                return SA_EINVAL;
            v[(size_t) i] = {sc_truth_key(t.contig, t.pos, t.mapped_strand), (signed char) (at - letters)};
        }
        std::stable_sort(v.begin(), v.end(), [](const std::pair<unsigned long long, signed char> &a,
                                                const std::pair<unsigned long long, signed char> &b) { return a.first < b.first; });
        for (size_t i = 0; i < v.size(); i++)
            if (i == 0 || v[i].first != v[i - 1].first) { tkey.push_back(v[i].first); tlet.push_back(v[i].second); }
    }
    if (const int rc = sa_device_check(device)) return rc;
    sa_call_scores *s = new (std::nothrow) sa_call_scores();
    if (!s) return SA_ENOMEM;
    s->device = device;
    s->nl = (int) nl;
    s->n_bins = n_bins;
    s->threshold = threshold;
    memcpy(s->letters, letters, nl);
    s->arr.assign((size_t) (SC_LEVELS * 2 * 2) * nl, ScArray());
    s->n_truth = tkey.size();
    int rc = SA_OK;
    {
        SaLayout L;
        L.add(8 * s->n_truth);
        s->o_tlet = L.add(s->n_truth + 1);
        if (hipSetDevice(device) != hipSuccess) { rc = SA_ENODEVICE; goto done; }
        if (g_sa_pool.get(SaPool::DEVICE, (void **) &s->d_truth, L.end, device) != hipSuccess) { s->d_truth = nullptr; rc = SA_ENOMEM; goto done; }
        if (s->n_truth) {
            SA_HIP_GOTO_DONE(hipMemcpy(s->d_truth, tkey.data(), 8 * s->n_truth, hipMemcpyHostToDevice));
            SA_HIP_GOTO_DONE(hipMemcpy(s->d_truth + s->o_tlet, tlet.data(), s->n_truth, hipMemcpyHostToDevice));
        }
        SA_HIP_GOTO_DONE(hipEventCreate(&s->e0));
        SA_HIP_GOTO_DONE(hipEventCreate(&s->e1));
    }
done:
    if (rc != SA_OK) { sa_call_scores_destroy(s); return rc; }
    *out = s;
    return SA_OK;
}

extern "C" int sa_call_scores_add_records(sa_call_scores_t *s, int32_t level, int32_t strand, const double *prob, const int8_t *true_letter,
                                          int64_t n) {
    if (!s || n < 0 || (n > 0 && (!prob || !true_letter)) || level < 0 || level >= SC_LEVELS || (strand != 0 && strand != 1)) return SA_EINVAL;
    const size_t nl = (size_t) s->nl;
    if (n * (int64_t) nl > SC_MAX_ADD) return SA_EUNSUPPORTED;
    std::vector<size_t> cnt(2 * nl, 0);
    for (int64_t i = 0; i < n; i++) {
        const int tl = true_letter[i];
        if (tl < 0 || tl >= (int) nl) return SA_EINVAL;
        for (size_t l = 0; l < nl; l++) {
            const double v = prob[(size_t) i * nl + l];
            if (!(v >= 0.0 && v <= 1.0)) return SA_EINVAL;   // (a NaN compares false)
            cnt[2 * l + ((int) l == tl)]++;
        }
    }
    ScEnter in(s);
    if (in.rc) return in.rc;
    if (n == 0) return SA_OK;
    for (size_t q = 0; q < 2 * nl; q++)
        if ((long long) (s->arr[(size_t) sc_array((int) nl, level, strand, (int) (q / 2), (int) (q % 2))].n + cnt[q]) > SC_MAX_ARRAY)
            return SA_EUNSUPPORTED;
    std::vector<std::vector<unsigned long long>> keys(2 * nl);
    for (size_t q = 0; q < 2 * nl; q++) keys[q].reserve(cnt[q]);
    for (int64_t i = 0; i < n; i++)
        for (size_t l = 0; l < nl; l++) keys[2 * l + ((int) l == true_letter[i])].push_back(sc_key_host(prob[(size_t) i * nl + l]));
    for (size_t q = 0; q < 2 * nl; q++) {   // every array has its room before the first copy: a refused add adds nothing
        ScArray &A = s->arr[(size_t) sc_array((int) nl, level, strand, (int) (q / 2), (int) (q % 2))];
        if (const int rc = sc_grow(s, A, A.n + cnt[q])) return rc;
    }
    for (size_t q = 0; q < 2 * nl; q++) {
        if (cnt[q] == 0) continue;
        ScArray &A = s->arr[(size_t) sc_array((int) nl, level, strand, (int) (q / 2), (int) (q % 2))];
        if (hipMemcpy(A.d + A.n, keys[q].data(), 8 * cnt[q], hipMemcpyHostToDevice) != hipSuccess) {
            s->poisoned = true;   // (some arrays of the add may have been copied)
            return SA_ENODEVICE;
        }
    }
    for (size_t q = 0; q < 2 * nl; q++) s->arr[(size_t) sc_array((int) nl, level, strand, (int) (q / 2), (int) (q % 2))].n += cnt[q];
    return SA_OK;
}

extern "C" int sa_call_scores_add_batch(sa_call_scores_t *s, sa_batch_t *b, const sa_score_job_map_t *map, int64_t n_jobs,
                                        double *kernel_ms_out) {
    if (!s || !b || n_jobs < 0 || (n_jobs > 0 && !map)) return SA_EINVAL;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    ScEnter in(s);
    if (in.rc) return in.rc;
    SaSiteFold F;
    int rc = sa_site_fold_run(b, &F);
    const size_t nj = F.nj, ns = F.ns, na = s->arr.size();
    const int nl = s->nl;
    char *d = nullptr;
    bool appending = false;
    std::vector<ScJob> jobs(nj);
    std::vector<unsigned char> kind_ok(F.letters.size() + 1, 0);
    std::vector<unsigned long long *> h_ptr(na, nullptr);
    std::vector<unsigned> h_cap(na, 0), h_cur(na, 0);
    unsigned long long h_misc[2] = {0, 0};
    long long ub0[2] = {0, 0}, ub1[2] = {0, 0};
    float kms = 0;
    if (rc != SA_OK) goto done;
    if ((size_t) n_jobs != nj || (ns > 0 && F.device != s->device)) { rc = SA_EINVAL; goto done; }
    for (size_t j = 0; j < nj; j++) {
        const sa_score_job_map_t &m = map[j];
        if (!sc_job_from_map(m, nl, &jobs[j])) { rc = SA_EINVAL; goto done; }
        const long long sites = F.h_site_off[j + 1] - F.h_site_off[j];
        ub0[m.strand] += sites;
        ub1[m.strand] += m.true_letter >= 0 && sites > 0;
    }
    if (ns == 0) goto done;   // (nothing is on the device)
    if ((long long) ns * nl > SC_MAX_ADD) { rc = SA_EUNSUPPORTED; goto done; }
    for (size_t kd = 0; kd < F.letters.size(); kd++) kind_ok[kd] = F.letters[kd] == std::string(s->letters);
    for (int level = 0; level < 2; level++)
        for (int st = 0; st < 2; st++) {
            const long long ub = level == 0 ? ub0[st] : ub1[st];
            for (int q = 0; q < 2 * nl && ub > 0; q++)
                if ((long long) s->arr[(size_t) sc_array(nl, level, st, q / 2, q % 2)].n + ub > SC_MAX_ARRAY) { rc = SA_EUNSUPPORTED; goto done; }
        }
    for (int level = 0; level < 2; level++)
        for (int st = 0; st < 2; st++) {
            const long long ub = level == 0 ? ub0[st] : ub1[st];
            for (int q = 0; q < 2 * nl && ub > 0; q++) {
                ScArray &A = s->arr[(size_t) sc_array(nl, level, st, q / 2, q % 2)];
                if ((rc = sc_grow(s, A, A.n + (size_t) ub)) != SA_OK) goto done;
            }
        }
    for (size_t a = 0; a < na; a++) {
        h_ptr[a] = s->arr[a].d;
        h_cap[a] = (unsigned) s->arr[a].cap;
        h_cur[a] = (unsigned) s->arr[a].n;
    }
    {
        SaLayout L;   // [jobs | kind ok | x of site | ptr | cap | cur | misc]
        const size_t o_jobs = L.add(sizeof(ScJob) * nj), o_ok = L.add(kind_ok.size()), o_x = L.add(4 * ns), o_ptr = L.add(8 * na),
                     o_cap = L.add(4 * na), o_cur = L.add(4 * na), o_misc = L.add(16);
        if (g_sa_pool.get(SaPool::DEVICE, (void **) &d, L.end, s->device) != hipSuccess) { d = nullptr; rc = SA_ENOMEM; goto done; }
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_jobs, jobs.data(), sizeof(ScJob) * nj, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_ok, kind_ok.data(), kind_ok.size(), hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_x, F.h_x, 4 * ns, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_ptr, h_ptr.data(), 8 * na, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_cap, h_cap.data(), 4 * na, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemcpyAsync(d + o_cur, h_cur.data(), 4 * na, hipMemcpyHostToDevice, 0));
        SA_HIP_GOTO_DONE(hipMemsetAsync(d + o_misc, 0, 16, 0));
        ScDev D;
        D.ptr = (unsigned long long *const *) (d + o_ptr);
        D.cap = (const unsigned *) (d + o_cap);
        D.cur = (unsigned *) (d + o_cur);
        D.misc = (unsigned long long *) (d + o_misc);
        D.T.tkey = (const unsigned long long *) s->d_truth;
        D.T.tlet = (const signed char *) (s->d_truth + s->o_tlet);
        D.T.n_truth = s->n_truth;
        D.nl = nl;
        appending = true;
        hipLaunchKernelGGL(k_score_sites, dim3((unsigned) nj), dim3(64), 0, 0, (const ScJob *) (d + o_jobs), F.site_off, F.kind,
                           (const unsigned char *) (d + o_ok), (const int *) (d + o_x), F.units, F.prob, (int) F.stride, D);
        if (ub1[0] + ub1[1] > 0)
            hipLaunchKernelGGL(k_score_reads, dim3((unsigned) ((nj * (size_t) nl + 255) / 256)), dim3(256), 0, 0, (const ScJob *) (d + o_jobs),
                               (int) nj, F.site_off, F.kind, (const unsigned char *) (d + o_ok), F.units, F.prob, (int) F.stride, D);
        SA_HIP_GOTO_DONE(F.ws->time_end());
        SA_HIP_GOTO_DONE(hipMemcpy(h_cur.data(), d + o_cur, 4 * na, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(hipMemcpy(h_misc, d + o_misc, 16, hipMemcpyDeviceToHost));
        SA_HIP_GOTO_DONE(F.ws->time_ms(&kms));
        for (size_t a = 0; a < na; a++)
            if (h_cur[a] > s->arr[a].cap) { rc = SA_ENODEVICE; goto done; }   // (cannot happen: an add appends at most its bound)
        for (size_t a = 0; a < na; a++) s->arr[a].n = h_cur[a];
        s->counts.unlabelled += (int64_t) h_misc[0];
        s->counts.other_sites += (int64_t) h_misc[1];
        if (kernel_ms_out) *kernel_ms_out = (double) kms;
    }
done:
    if (rc != SA_OK && appending) s->poisoned = true;   // (what the arrays hold past their lengths is harmless, the lengths are not known to be)
    if (rc != SA_OK && d) (void) hipStreamSynchronize(0);
    if (d) g_sa_pool.put(SaPool::DEVICE, d);
    sa_site_fold_release(&F, rc != SA_OK);
    return rc;
}

extern "C" int sa_call_scores_checkpoint(sa_call_scores_t *s) {
    if (!s) return SA_EINVAL;
    ScEnter in(s);
    if (in.rc) return in.rc;
    s->ck_n.resize(s->arr.size());
    for (size_t a = 0; a < s->arr.size(); a++) s->ck_n[a] = s->arr[a].n;
    s->ck_counts = s->counts;
    s->has_ck = true;
    return SA_OK;
}

extern "C" int sa_call_scores_rollback(sa_call_scores_t *s) {
    if (!s) return SA_EINVAL;
    ScEnter in(s);
    if (in.rc) return in.rc;
    if (!s->has_ck) return SA_ESTATE;
    for (size_t a = 0; a < s->arr.size(); a++) s->arr[a].n = s->ck_n[a];
    s->counts = s->ck_counts;
    return SA_OK;
}

extern "C" int sa_call_scores_finish(sa_call_scores_t *s, sa_call_score_row_t **rows_out, int64_t *n_rows_out, int64_t **curves_out,
                                     sa_call_scores_counts_t *counts_out, double *kernel_ms_out) {
    if (!s || !rows_out || !n_rows_out) return SA_EINVAL;
    *rows_out = nullptr;
    *n_rows_out = 0;
    if (curves_out) *curves_out = nullptr;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    ScEnter in(s);
    if (in.rc) return in.rc;
    const int nl = s->nl;
    const size_t w = (size_t) s->n_bins + 2;
    size_t max_sum = 0, max_one = 0;
    for (int level = 0; level < SC_LEVELS; level++)
        for (int l = 0; l < nl; l++) {
            size_t sum = 0;
            for (int q = 0; q < 4; q++) {
                const size_t n = s->arr[(size_t) sc_array(nl, level, q / 2, l, q % 2)].n;
                sum += sa_up256(8 * n) / 8;
                max_one = std::max(max_one, n);
            }
            max_sum = std::max(max_sum, sum);
            // the group of both strands counts 2 n_pos n_neg in 64 bits
            const unsigned __int128 np = (unsigned __int128) s->arr[(size_t) sc_array(nl, level, 0, l, 1)].n + s->arr[(size_t) sc_array(nl, level, 1, l, 1)].n,
                                    nn = (unsigned __int128) s->arr[(size_t) sc_array(nl, level, 0, l, 0)].n + s->arr[(size_t) sc_array(nl, level, 1, l, 0)].n;
            if (2 * np * nn > (unsigned __int128) UINT64_MAX) return SA_EUNSUPPORTED;
        }
    std::vector<sa_call_score_row_t> rows;
    std::vector<int64_t> curves;
    if (counts_out) *counts_out = s->counts;
    if (max_one == 0) return SA_OK;
    int rc = SA_OK;
    SaLayout L;   // [sorted x 4 | tmp | sort work | auc2[3], ge[3][2][n_bins + 2]]
    const size_t o_sorted = L.add(8 * max_sum), o_tmp = L.add(8 * max_one), o_work = L.add(sa_sort_work_bytes(max_one)),
                 o_out = L.add(8 * (4 + 6 * w)), out_bytes = 8 * (4 + 6 * w);
    char *d = nullptr;
    std::vector<long long> h_out(4 + 6 * w);
    float kms = 0;
    if (g_sa_pool.get(SaPool::DEVICE, (void **) &d, L.end, s->device) != hipSuccess) return SA_ENOMEM;
    SA_HIP_GOTO_DONE(hipEventRecord(s->e0, 0));
    for (int level = 0; level < SC_LEVELS; level++) {
        std::vector<sa_call_score_row_t> lev((size_t) nl * 3);
        std::vector<int64_t> lev_curves((size_t) nl * 3 * 2 * (w - 1));
        std::vector<char> have((size_t) nl * 3, 0);
        for (int l = 0; l < nl; l++) {
            ScFour F4;
            size_t at = 0, total = 0;
            for (int q = 0; q < 4; q++) {   // q = strand * 2 + cls
                const ScArray &A = s->arr[(size_t) sc_array(nl, level, q / 2, l, q % 2)];
                unsigned long long *dst = (unsigned long long *) (d + o_sorted) + at;
                F4.a[q] = dst;
                F4.n[q] = A.n;
                at += sa_up256(8 * A.n) / 8;
                total += A.n;
                if (A.n && (rc = sa_sort_u64_device((const uint64_t *) A.d, A.n, (uint64_t *) dst, (uint64_t *) (d + o_tmp), d + o_work, nullptr)) != SA_OK) goto done;
            }
            if (total == 0) continue;
            SA_HIP_GOTO_DONE(hipMemsetAsync(d + o_out, 0, out_bytes, 0));
            for (int ps = 0; ps < 2; ps++) {
                const unsigned long long np = F4.n[ps * 2 + 1];
                if (np == 0 || F4.n[0] + F4.n[2] == 0) continue;
                hipLaunchKernelGGL(k_score_auc, dim3((unsigned) std::min<unsigned long long>((np + 255) / 256, 8192)), dim3(256), 0, 0,
                                   F4.a[ps * 2 + 1], np, F4.a[0], F4.n[0], F4.a[2], F4.n[2], ps, (unsigned long long *) (d + o_out));
            }
            hipLaunchKernelGGL(k_score_counts, dim3((unsigned) ((w + 255) / 256)), dim3(256), 0, 0, F4, s->n_bins,
                               s->threshold <= 0.0 ? 0ull : sc_key_host(s->threshold), (long long *) (d + o_out) + 4);
            SA_HIP_GOTO_DONE(hipGetLastError());
            SA_HIP_GOTO_DONE(hipMemcpy(h_out.data(), d + o_out, out_bytes, hipMemcpyDeviceToHost));
            for (int g = 0; g < 3; g++) {
                const long long *ge_neg = h_out.data() + 4 + (size_t) (g * 2 + 0) * w, *ge_pos = h_out.data() + 4 + (size_t) (g * 2 + 1) * w;
                const long long n_pos = ge_pos[0], n_neg = ge_neg[0];   // (every score is >= t_0 = 0)
                if (n_pos + n_neg == 0) continue;
                sa_call_score_row_t &r = lev[(size_t) l * 3 + (size_t) g];
                memset(&r, 0, sizeof r);
                r.level = level;
                r.group = g;
                r.letter = s->letters[l];
                r.n_pos = n_pos;
                r.n_neg = n_neg;
                r.auc2 = (uint64_t) h_out[(size_t) g];
                r.auc = n_pos && n_neg ? (double) r.auc2 / (2.0 * (double) n_pos * (double) n_neg) : (double) NAN;
                r.tp = ge_pos[w - 1];
                r.fp = ge_neg[w - 1];
                r.fn = n_pos - r.tp;
                r.tn = n_neg - r.fp;
                int64_t *c = lev_curves.data() + ((size_t) l * 3 + (size_t) g) * 2 * (w - 1);
                for (size_t k = 0; k + 1 < w; k++) { c[k] = ge_pos[k]; c[(w - 1) + k] = ge_neg[k]; }
                have[(size_t) l * 3 + (size_t) g] = 1;
            }
        }
        for (int g = 0; g < 3; g++)
            for (int l = 0; l < nl; l++) {
                const size_t q = (size_t) l * 3 + (size_t) g;
                if (!have[q]) continue;
                rows.push_back(lev[q]);
                curves.insert(curves.end(), lev_curves.begin() + (long) (q * 2 * (w - 1)), lev_curves.begin() + (long) ((q + 1) * 2 * (w - 1)));
            }
    }
    SA_HIP_GOTO_DONE(hipEventRecord(s->e1, 0));
    SA_HIP_GOTO_DONE(hipEventSynchronize(s->e1));
    SA_HIP_GOTO_DONE(hipEventElapsedTime(&kms, s->e0, s->e1));
    if (kernel_ms_out) *kernel_ms_out = (double) kms;
    {
        sa_call_score_row_t *ro = (sa_call_score_row_t *) malloc(sizeof(sa_call_score_row_t) * std::max(rows.size(), (size_t) 1));
        int64_t *co = curves_out ? (int64_t *) malloc(8 * std::max(curves.size(), (size_t) 1)) : nullptr;
        if (!ro || (curves_out && !co)) { free(ro); free(co); rc = SA_ENOMEM; goto done; }
        if (!rows.empty()) memcpy(ro, rows.data(), sizeof(sa_call_score_row_t) * rows.size());
        if (co && !curves.empty()) memcpy(co, curves.data(), 8 * curves.size());
        *rows_out = ro;
        *n_rows_out = (int64_t) rows.size();
        if (curves_out) *curves_out = co;
    }
done:
    if (rc != SA_OK) (void) hipStreamSynchronize(0);   // (a failed call may have left work queued on its block)
    g_sa_pool.put(SaPool::DEVICE, d);
    return rc;
}

static double sc_ratio(int64_t a, int64_t b) { return b ? (double) a / (double) b : (double) NAN; }

extern "C" int sa_call_scores_write(const char *summary_path, const char *curves_path, int32_t n_bins, const sa_call_score_row_t *rows,
                                    int64_t n_rows, const int64_t *curves) {
    if (!summary_path || n_bins < 1 || n_rows < 0 || (n_rows > 0 && !rows) || (curves_path && n_rows > 0 && !curves)) return SA_EINVAL;
    static const char *const group_name[3] = {"t", "c", "all"};
    for (int64_t i = 0; i < n_rows; i++)
        if (rows[i].group < 0 || rows[i].group > 2) return SA_EINVAL;
    char num[6][40];
    FILE *fh = fopen(summary_path, "w");
    if (!fh) return SA_EIO;
    fprintf(fh, "level\tstrand\tletter\tn_pos\tn_neg\tauc\ttp\tfp\ttn\tfn\taccuracy\tprecision\trecall\n");
    for (int64_t i = 0; i < n_rows; i++) {
        const sa_call_score_row_t &r = rows[i];
        sa_format_py_repr(num[0], r.auc);
        sa_format_py_repr(num[1], sc_ratio(r.tp + r.tn, r.n_pos + r.n_neg));
        sa_format_py_repr(num[2], sc_ratio(r.tp, r.tp + r.fp));
        sa_format_py_repr(num[3], sc_ratio(r.tp, r.n_pos));
        fprintf(fh, "%d\t%s\t%c\t%" PRId64 "\t%" PRId64 "\t%s\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%" PRId64 "\t%s\t%s\t%s\n", (int) r.level,
                group_name[r.group], r.letter, r.n_pos, r.n_neg, num[0], r.tp, r.fp, r.tn, r.fn, num[1], num[2], num[3]);
    }
    if (fclose(fh) != 0) return SA_EIO;
    if (!curves_path) return SA_OK;
    fh = fopen(curves_path, "w");
    if (!fh) return SA_EIO;
    setvbuf(fh, NULL, _IOFBF, 1 << 16);
    fprintf(fh, "level\tstrand\tletter\tk\tthreshold\ttp_ge\tfp_ge\ttpr\tfpr\tprecision\n");
    const size_t nb1 = (size_t) n_bins + 1;
    for (int64_t i = 0; i < n_rows; i++) {
        const sa_call_score_row_t &r = rows[i];
        const int64_t *tp = curves + (size_t) i * 2 * nb1, *fp = tp + nb1;
        for (size_t k = 0; k < nb1; k++) {
            sa_format_py_repr(num[0], (double) k / (double) n_bins);
            sa_format_py_repr(num[1], sc_ratio(tp[k], r.n_pos));
            sa_format_py_repr(num[2], sc_ratio(fp[k], r.n_neg));
            sa_format_py_repr(num[3], sc_ratio(tp[k], tp[k] + fp[k]));
            fprintf(fh, "%d\t%s\t%c\t%zu\t%s\t%" PRId64 "\t%" PRId64 "\t%s\t%s\t%s\n", (int) r.level, group_name[r.group], r.letter, k, num[0],
                    tp[k], fp[k], num[1], num[2], num[3]);
        }
    }
    return fclose(fh) == 0 ? SA_OK : SA_EIO;
}
