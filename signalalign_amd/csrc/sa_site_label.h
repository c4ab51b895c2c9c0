// How a site call gets its true letter, stated once for the stages that label the sites of a site fold (SaSiteFold, sa_chain.h):
// k_score_sites (sa_scores.hip), which appends the labelled scores to an accumulator, and k_cq_calls (sa_callq.hip), which holds
// every labelled call against its guide.  Also the accumulator itself (sa_call_scores_t), whose letters, threshold and positions
// table both read.
#ifndef SA_SITE_LABEL_H
#define SA_SITE_LABEL_H

#include <mutex>
#include <vector>

#include "sa_internal.h"
#include "sa_scratch.h"

#define SC_MAX_CONTIG (1ll << 21)
#define SC_MAX_POS (1ll << 41)

struct ScArray {
    unsigned long long *d = nullptr;
    size_t n = 0, cap = 0;
};

struct ScJob {   // sa_score_job_map_t as the device reads it
    long long x0;
    int contig, x_sign, strand, mapped, true_letter, ascending;   // ascending: the read-level sum walks the job's sites in ascending x
};

struct sa_call_scores {
    std::mutex mu;
    int device = -1, nl = 0, n_bins = 0;
    double threshold = 0.0;
    char letters[SA_SITE_MAX_LETTERS + 1] = {0};
    std::vector<ScArray> arr;                 // index sc_array(level, strand, letter, cls)
    std::vector<size_t> ck_n;
    sa_call_scores_counts_t counts = {0, 0}, ck_counts = {0, 0};
    bool has_ck = false, poisoned = false;
    char *d_truth = nullptr;                  // [keys | letters], sorted by key
    size_t n_truth = 0, o_tlet = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
};

struct ScEnter {   // the lock, the poison check and the device of every call on an accumulator
    std::unique_lock<std::mutex> g;
    int rc;
    explicit ScEnter(sa_call_scores *s) : g(s->mu), rc(SA_OK) {
        if (s->poisoned) rc = SA_ESTATE;
        else if (hipSetDevice(s->device) != hipSuccess) rc = SA_ENODEVICE;
    }
};

// one entry of a job map as the device reads it; false for an entry the labelling stages refuse
static inline bool sc_job_from_map(const sa_score_job_map_t &m, int nl, ScJob *J) {
    if (m.contig < 0 || m.contig >= SC_MAX_CONTIG || (m.x_sign != 1 && m.x_sign != -1) || (m.strand != 0 && m.strand != 1) ||
        (m.mapped_strand != 0 && m.mapped_strand != 1) || m.true_letter < -1 || m.true_letter >= nl)
        return false;
    J->x0 = m.x0; J->contig = m.contig; J->x_sign = m.x_sign; J->strand = m.strand; J->mapped = m.mapped_strand;
    J->true_letter = m.true_letter;
    J->ascending = (m.x_sign == 1) == (m.mapped_strand == 0);   // ascending reference_index on '+', descending on '-'
    return true;
}

__host__ __device__ static inline unsigned long long sc_truth_key(long long contig, long long pos, int mapped) {
    return ((unsigned long long) contig << 42) | ((unsigned long long) pos << 1) | (unsigned long long) mapped;
}

// the first index of a[0 .. n) whose entry is >= key (upper: > key)
template <bool UPPER>
__device__ __forceinline__ unsigned long long sc_bound(const unsigned long long *__restrict__ a, unsigned long long n, unsigned long long key) {
    unsigned long long lo = 0, hi = n;
    while (lo < hi) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        const unsigned long long v = a[mid];
        if (UPPER ? v <= key : v < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool sc_site_live(const unsigned long long *__restrict__ units, long long s, int stride) {
    unsigned long long tot = 0;
    for (int l = 0; l < stride; l++) tot += units[(size_t) s * (size_t) stride + (size_t) l];   // (the entries past a kind's letters are 0)
    return tot != 0;
}

struct ScTruth {   // the positions table of an accumulator, sorted by key
    const unsigned long long *tkey;
    const signed char *tlet;
    unsigned long long n_truth;
};

// What site s (x = x_of_site[s]) of job J is: not a call (its units sum to 0, or `in_range` is false: a lane past the job's
// sites), a site of other letters, an unlabelled call, or a labelled one with *tl its true letter.
enum { SC_SITE_NONE = 0, SC_SITE_OTHER, SC_SITE_UNLABELLED, SC_SITE_LABELLED };
__device__ __forceinline__ int sc_site_label(const ScJob &J, bool in_range, long long s, const unsigned char *__restrict__ kind,
                                             const unsigned char *__restrict__ kind_ok, const int *__restrict__ x_of_site,
                                             const unsigned long long *__restrict__ units, int stride, const ScTruth &T, int *tl_out) {
    *tl_out = -1;
    if (!in_range || !sc_site_live(units, s, stride)) return SC_SITE_NONE;
    if (!kind_ok[kind[s]]) return SC_SITE_OTHER;
    int tl = J.true_letter;
    if (tl < 0) {
        const long long r = J.x0 + (long long) J.x_sign * x_of_site[s];
        if (r >= 0 && r < SC_MAX_POS) {
            const unsigned long long key = sc_truth_key(J.contig, r, J.mapped);
            const unsigned long long at = sc_bound<false>(T.tkey, T.n_truth, key);
            if (at < T.n_truth && T.tkey[at] == key) tl = T.tlet[at];
        }
    }
    *tl_out = tl;
    return tl < 0 ? SC_SITE_UNLABELLED : SC_SITE_LABELLED;
}

#endif
