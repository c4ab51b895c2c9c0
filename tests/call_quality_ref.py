"""Call quality restated in plain Python and numpy, integers throughout (rules 1-8 of include/signalalign_hip.h, "Call quality"):
what sa_batch_call_quality and sa_call_quality_records are held against.  `script_walk=True` reproduces the one-guide-row-per-call
walk of get_distance_from_guide_alignment (alignedsignal.py:388-425), so that a test can show where the two part."""
import bisect

import numpy as np

NO_GUIDE, NO_SITES, NO_PATH = 1, 2, 4
DEFAULT_PARAMS = (-10000, 100, 200, 30)


def true_letter_of(job_map, x, truth):
    """the index of the site's true letter, or -1: the job's label, else the positions table {(contig, pos, mapped strand): index}"""
    if job_map["true_letter"] >= 0:
        return job_map["true_letter"]
    return truth.get((job_map["contig"], job_map["x0"] + job_map["x_sign"] * x, job_map["mapped_strand"]), -1)


def bands(rec_x, rec_y, raw_start, raw_length):
    """{x: (raw_start, raw_length)} over the records of every x: the SA_LABEL_BANDS rule"""
    span = {}
    for x, y in zip(rec_x, rec_y):
        x, y = int(x), int(y)
        lo, hi = span.get(x, (y, y))
        span[x] = (min(lo, y), max(hi, y))
    return {x: (int(raw_start[y0]), int(raw_start[y1]) - int(raw_start[y0]) + int(raw_length[y1])) for x, (y0, y1) in span.items()}


def guide_row(ax, x, x_sign):
    """rule 3: the index of the call's guide row, or -1 for a call outside the guide"""
    ax = [int(v) for v in ax]
    n = len(ax)
    if x_sign > 0:
        i = bisect.bisect_left(ax, x)
        if i == n:
            return -1                      # no anchor at or beyond the call: the script leaves NaN
        return i if ax[i] == x else i - 1  # (i - 1 == -1: the script's iloc[-1] wraps)
    i = bisect.bisect_right(ax, x)
    if i == 0:
        return -1
    if ax[i - 1] == x:
        return i - 1
    return -1 if i == n else i


def script_walk_rows(ax, xs, x_sign):
    """the guide row of every call (xs in ascending reference_index) as the script's loop finds it: one guide row per call; -1 where
    it wraps, None where the loop ends before the call (NaN)"""
    order = list(range(len(ax))) if x_sign > 0 else list(range(len(ax)))[::-1]
    r = [x_sign * int(ax[i]) for i in order]
    rows, v = [], 0
    for i, ri in enumerate(r):
        if v >= len(xs):
            break
        if ri >= x_sign * xs[v]:
            gi = i if ri == x_sign * xs[v] else i - 1
            rows.append(order[gi] if gi >= 0 else -1)
            v += 1
    return rows + [None] * (len(xs) - len(rows))


def round_mid(raw_start, raw_length):
    """np.round(raw_start + raw_length / 2) in integers: half goes to the even neighbour"""
    raw_start, raw_length = int(raw_start), int(raw_length)
    if raw_length % 2 == 0:
        return raw_start + raw_length // 2
    below = raw_start + (raw_length - 1) // 2
    return below + 1 if below % 2 else below


def hist_slot(delta2, bin_lo, bin_width, n_bins):
    if delta2 < 2 * bin_lo:
        return 0
    b = (delta2 - 2 * bin_lo) // (2 * bin_width)          # Python's // is a floor
    return n_bins + 1 if b >= n_bins else b + 1


def gaps_of(path_y, raw_start, raw_length, min_gap):
    out = []
    for i in range(1, len(path_y)):
        a, b = int(path_y[i - 1]), int(path_y[i])
        gap = int(raw_start[b]) - (int(raw_start[a]) + int(raw_length[a]))
        if gap > min_gap:
            out.append((a, b, gap))
    return out


def call_quality(job_map, job, site_x, site_prob, rec_x, rec_y, path_y, threshold, truth, site_other=None, params=DEFAULT_PARAMS,
                 script_walk=False):
    """One job.  job: dict with ax, ay, raw_start, raw_length; site_x ascending with site_prob[i][letter]; path_y the events of its MEA
    path (None or empty: no path).  Returns (read dict, calls list of dicts, gaps list of (y_before, y_after, gap), hist
    [n_bins + 2][2])."""
    bin_lo, bin_width, n_bins, min_gap = params
    ax, ay, rs, rl = job["ax"], job["ay"], job["raw_start"], job["raw_length"]
    x_sign = job_map["x_sign"]
    hist = np.zeros((n_bins + 2, 2), dtype=np.int64)
    read = dict(status=0, max_x=-1, n_calls=0, n_correct=0, n_unlabelled=0, n_other_sites=0, n_outside=0, sum_abs_delta2=0,
                max_abs_delta2=0, n_path=0, n_gaps=0, sum_gap=0, max_gap=0)
    calls = []
    labelled = []
    for i, x in enumerate(site_x):
        x = int(x)
        if site_other is not None and site_other[i]:
            read["n_other_sites"] += 1
            continue
        tl = true_letter_of(job_map, x, truth)
        if tl < 0:
            read["n_unlabelled"] += 1
            continue
        labelled.append((i, x, tl))
    rows = [guide_row(ax, x, x_sign) for _, x, _ in labelled]
    if script_walk:
        by_ref = sorted(range(len(labelled)), key=lambda q: x_sign * labelled[q][1])
        walked = script_walk_rows(ax, [labelled[q][1] for q in by_ref], x_sign)
        for q, row in zip(by_ref, walked):
            rows[q] = -1 if row is None else row
    best = None
    band_of = bands(rec_x, rec_y, rs, rl)
    for (i, x, tl), g in zip(labelled, rows):
        b_start, b_length = band_of[x]
        p = float(site_prob[i][tl])
        c = dict(x=x, guide_event=-1, raw_start=b_start, raw_length=b_length, delta2=0, prob_true=p, true_letter=tl,
                 correct=int(p > threshold), outside=int(g < 0))
        read["n_calls"] += 1
        read["n_correct"] += c["correct"]
        if g < 0:
            read["n_outside"] += 1
        else:
            e = int(ay[g])
            c["guide_event"] = e
            c["delta2"] = 2 * b_start + b_length - 2 * round_mid(rs[e], rl[e])
            ab = abs(c["delta2"])
            read["sum_abs_delta2"] += ab
            if best is None or ab > best[0] or (ab == best[0] and x < best[1]):
                best = (ab, x)
            hist[hist_slot(c["delta2"], bin_lo, bin_width, n_bins), c["correct"]] += 1
        calls.append(c)
    if best is not None:
        read["max_abs_delta2"], read["max_x"] = best
    path_y = [] if path_y is None else [int(y) for y in path_y]
    gaps = gaps_of(path_y, rs, rl, min_gap)
    read["n_path"], read["n_gaps"] = len(path_y), len(gaps)
    read["sum_gap"] = sum(g for _, _, g in gaps)
    read["max_gap"] = max([g for _, _, g in gaps] + [0])
    read["status"] = ((NO_GUIDE if len(ax) == 0 else 0) | (NO_SITES if len(site_x) == 0 else 0) | (NO_PATH if not path_y else 0))
    return read, calls, gaps, hist


def call_quality_jobs(job_maps, jobs, site_first, site_x, site_prob, rec_first, rec_x, rec_y, paths, threshold, truth,
                      site_other=None, params=DEFAULT_PARAMS):
    """every job of a call, with call_first / gap_first into the back-to-back lists; returns (reads, calls, gaps, hist per job, total)"""
    reads, calls, gaps, hists = [], [], [], []
    for j, (m, job) in enumerate(zip(job_maps, jobs)):
        a, e, ra, re_ = int(site_first[j]), int(site_first[j + 1]), int(rec_first[j]), int(rec_first[j + 1])
        r, c, g, h = call_quality(m, job, site_x[a:e], site_prob[a:e], rec_x[ra:re_], rec_y[ra:re_],
                                  None if paths is None else paths[j], threshold, truth,
                                  None if site_other is None else site_other[a:e], params)
        r["call_first"], r["gap_first"] = len(calls), len(gaps)
        reads.append(r)
        calls += c
        gaps += g
        hists.append(h)
    n_bins = params[2]
    total = np.sum(hists, axis=0) if hists else np.zeros((n_bins + 2, 2), dtype=np.int64)
    return reads, calls, gaps, hists, total


# The hand-worked table of tests/test_host_call_quality.py: 12 events, 5 anchors, 4 sites with the read-level label 1, threshold 0.5.
# Events 6 and 9 follow holes of 40 and of exactly 30 samples.  The guide's events 1 and 5 have an odd raw_length whose middle
# rounds up to the even neighbour (15.5 -> 16, 33.5 -> 34), 7 and 10 one whose middle rounds down (82.5 -> 82, 126.5 -> 126).
HAND = dict(
    job_map=dict(contig=0, x_sign=1, x0=100, strand=0, mapped_strand=0, true_letter=1),
    job=dict(ax=[2, 4, 5, 8, 9], ay=[1, 3, 5, 7, 10],
             raw_start=[10, 14, 17, 22, 26, 32, 75, 80, 85, 119, 123, 130], raw_length=[4, 3, 5, 4, 6, 3, 5, 5, 4, 4, 7, 2]),
    site_x=[1, 4, 7, 10],
    site_prob=[[0.1, 0.9], [0.5, 0.5], [0.3, 0.7], [0.8, 0.2]],
    rec_x=[1, 1, 3, 4, 4, 4, 7, 7, 10],
    rec_y=[0, 1, 2, 2, 3, 4, 6, 8, 11],
    path_y=[0, 1, 2, 3, 5, 6, 8, 9, 11],
    threshold=0.5)
