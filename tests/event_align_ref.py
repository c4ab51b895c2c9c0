"""A plain reference for the event <-> k-mer pre-alignment: the Viterbi recurrence of adaptive_banded_simple_event_align2
(impl/eventAligner.c:899-1235) over the WHOLE (n_events + 1) x (n_k-mers + 1) matrix.  Nothing of the reference's adaptive
banding is here: a cell is addressed by (event, k-mer) and every cell is filled, so wherever the banded code's band
covers the path this must give the same pairs and the same status word, and it shares none of the banded code's index
arithmetic.  What is kept, because it decides ties and roundings: scores stored as float32 (the reference computes a cell
in `float`), the three candidates formed in double and rounded once, the D / U / L tie rule as the reference writes it,
the first maximum over the last column, the four checks.

Cells of an anti-diagonal are independent, so the matrix is filled one anti-diagonal at a time with numpy.
math.log / math.exp (the C library's) are used for every logarithm so that they round as the C code's do.
"""
import math

import numpy as np

FROM_D, FROM_U, FROM_L = 0, 1, 2


def emission_matrix(table5, kmer_ids, event_mean, scale, shift, var):
    """emissions_signal_strawManGetKmerEventMatchProbWithDescaling_MeanOnly (impl/stateMachine.c:557-605) for every
    (event, k-mer) pair: [n_events, n_kmers] float64."""
    table5 = np.asarray(table5, dtype=np.float64)
    ids = np.asarray(kmer_ids, dtype=np.int64)
    mu = table5[5 * ids][None, :]
    sd_of = table5[5 * ids + 1]
    log_sd = np.array([math.log(s) if s > 0.0 else 0.0 for s in sd_of])[None, :]
    sd = sd_of[None, :]
    e = np.asarray(event_mean, dtype=np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        en = (e + var * mu - scale * mu - shift) / var
        a = (en - mu) / sd
        lp = math.log(1 / var) + (-0.91893853320467267 - log_sd + (-0.5 * a * a))
    return np.where(sd == 0.0, -np.inf, lp)


def event_align(table5, kmer_ids, event_mean, scale, shift, var=1.0):
    """Returns (pairs, status): pairs an [n, 2] int array of (k-mer, event) in ascending order, the whole walk whatever the
    status; status the reference's four checks as bits (0: average log emission < -5.2, 1: first or last k-mer not
    reached, 2: more than 50 k-mers skipped in a row, 3: more than 5 events per k-mer)."""
    n_events, n_kmers = len(event_mean), len(kmer_ids)
    assert n_events > 0 and n_kmers > 0
    events_per_kmer = float(n_events) / float(n_kmers)
    p_stay = 1 - (1 / (events_per_kmer + 1))
    lp_skip = math.log(1e-10)
    lp_stay = math.log(p_stay)
    lp_step = math.log(1.0 - math.exp(lp_skip) - math.exp(lp_stay))
    lp_trim = math.log(0.01)
    em = emission_matrix(table5, kmer_ids, event_mean, scale, shift, var)

    # S[e + 1, k + 1] = score of (event e, k-mer k); row 0 is event -1, column 0 is k-mer -1.  Stored as the reference
    # READS it: every read of a neighbour goes through `float`.
    S = np.full((n_events + 1, n_kmers + 1), -np.inf, dtype=np.float32)
    T = np.zeros((n_events, n_kmers), dtype=np.uint8)
    S[0, 0] = 0.0
    S[1:, 0] = (lp_trim * np.arange(1, n_events + 1, dtype=np.float64)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        for d in range(n_events + n_kmers - 1):
            e = np.arange(max(0, d - n_kmers + 1), min(n_events - 1, d) + 1)
            k = d - e
            up = S[e, k + 1].astype(np.float64)      # (e - 1, k)
            left = S[e + 1, k].astype(np.float64)    # (e, k - 1)
            diag = S[e, k].astype(np.float64)        # (e - 1, k - 1)
            lp_em = em[e, k]
            s_d = (diag + lp_step + lp_em).astype(np.float32)
            s_u = (up + lp_stay + lp_em).astype(np.float32)
            s_l = (left + lp_skip).astype(np.float32)
            best = s_d.copy()
            frm = np.full(len(e), FROM_D, dtype=np.uint8)
            best = np.where(s_u > best, s_u, best)
            frm = np.where(best == s_u, FROM_U, frm)
            best = np.where(s_l > best, s_l, best)
            frm = np.where(best == s_l, FROM_L, frm)
            S[e + 1, k + 1] = best
            T[e, k] = frm

    # best (event, last k-mer) cell with the events behind it trimmed: the first maximum
    last = (S[1:, n_kmers].astype(np.float64) + (n_events - np.arange(n_events)).astype(np.float64) * lp_trim).astype(np.float32)
    best, cur_ev = np.float32(-np.inf), 0
    for e in range(n_events):
        if last[e] > best:
            best, cur_ev = last[e], e
    cur_km = n_kmers - 1
    pairs, sum_em, cur_gap, max_gap = [], 0.0, 0, 0
    while cur_km >= 0 and cur_ev >= 0:
        pairs.append((cur_km, cur_ev))
        sum_em += float(em[cur_ev, cur_km])
        frm = T[cur_ev, cur_km]
        if frm == FROM_D:
            cur_km -= 1
            cur_ev -= 1
            cur_gap = 0
        elif frm == FROM_U:
            cur_ev -= 1
            cur_gap = 0
        else:
            cur_km -= 1
            cur_gap += 1
            max_gap = max(max_gap, cur_gap)
    pairs.reverse()
    status = 0
    if sum_em / len(pairs) < -5.2:
        status |= 1
    if not (pairs[0][0] == 0 and pairs[-1][0] == n_kmers - 1):
        status |= 2
    if max_gap > 50:
        status |= 4
    if events_per_kmer > 5.0:
        status |= 8
    return np.array(pairs, dtype=np.int32).reshape(-1, 2), status
