"""numpy restatement of the reference's raw-current front end, operation for operation with its float / double casts:

  raw_to_pa            fast5_get_raw_samples           impl/eventAligner.c:423-470 (attributes read as floats, :508-530)
  detect_events        detect_events                   impl/event_detection.c:268-330
                         compute_sum_sumsq             :35-47   sequential double folds, the square a float product
                         compute_tstat                 :58-115  double sums, float means, combined_var built in double
                         short_long_peak_detector      :122-205 serial state machine (a plain loop here)
                         create_events                 :220-266
  basecalled_table     event_table_to_basecalled_table impl/eventAligner.c:744-768
  base_event_map       alignment_to_base_event_map     impl/eventAligner.c:1310-1360 (DNA)
                       rna_alignment_to_base_event_map impl/eventAligner.c:1362-1414 (RNA)

Two departures from undefined behaviour, as in signalalign_amd/csrc/sa_detect.hip: a read without a peak is one event
[0, n) (the reference reads peaks[-1]); an empty read is rejected.  No trimming: every caller of trim_and_segment_raw
discards its result (load_from_raw2, :1267-1271), so detection always runs over all samples.  Test infrastructure, not
product code.
"""
import math
import struct

import numpy as np

f32, f64 = np.float32, np.float64
FLT_MIN = f32(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)

# inc/event_detection.h: window_length1, window_length2, threshold1, threshold2, peak_height
DEFAULTS = (3, 6, 1.4, 9.0, 0.2)
RNA = (7, 14, 2.5, 9.0, 1.0)


def attrs_of(fixture):
    """the five f64 attributes of a tests/golden/raw fixture, as the floats the reference reads them as"""
    a = np.asarray(fixture["attrs_f64_bits"], dtype=np.uint64).view(np.float64)
    return dict(digitisation=f32(a[0]), offset=f32(a[1]), range=f32(a[2]), sample_rate=f32(a[3]), start_time=f32(a[4]))


def raw_to_pa(raw, digitisation, offset, range, **_):
    unit = f32(range) / f32(digitisation)
    return (np.asarray(raw).astype(f32) + f32(offset)) * unit


def sum_sumsq(x):
    x = np.asarray(x, dtype=f32)
    s = np.zeros(len(x) + 1, dtype=f64)
    q = np.zeros(len(x) + 1, dtype=f64)
    np.cumsum(x.astype(f64), out=s[1:])            # add.accumulate: a left-to-right fold
    np.cumsum((x * x).astype(f64), out=q[1:])
    return s, q


def tstat(s, q, n, w):
    t = np.zeros(n, dtype=f32)
    if n < 2 * w or w < 2:
        return t
    i = np.arange(w, n - w + 1)
    sum1 = s[i] - s[i - w]                          # s[0] == 0: at i == w this is s[w] itself
    sumsq1 = q[i] - q[i - w]
    sum2 = (s[i + w] - s[i]).astype(f32)
    sumsq2 = (q[i + w] - q[i]).astype(f32)
    wf = f32(w)
    mean1 = (sum1 / f64(wf)).astype(f32)
    mean2 = sum2 / wf
    cv = (((sumsq1 / f64(wf)) - (mean1 * mean1).astype(f64)) + (sumsq2 / wf).astype(f64) - (mean2 * mean2).astype(f64))
    cv = np.fmax(cv.astype(f32), FLT_MIN)
    dm = mean2 - mean1
    t[i] = (np.abs(dm.astype(f64)) / np.sqrt((cv / wf).astype(f64))).astype(f32)
    return t


def _r32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def peaks(t1, t2, w1, w2, thr1, thr2, peak_height):
    """short_long_peak_detector: the emitted peak positions in emission order"""
    sig = (t1.tolist(), t2.tolist())
    thr = (float(f32(thr1)), float(f32(thr2)))
    wl = (w1, w2)
    ph = float(f32(peak_height))
    masked = [0, 0]
    pos = [-1, -1]
    val = [FLT_MAX, FLT_MAX]
    valid = [False, False]
    out = []
    for i in range(len(sig[0])):
        for k in (0, 1):
            if masked[k] >= i:
                continue
            v = sig[k][i]
            if pos[k] == -1:
                if v < val[k]:
                    val[k] = v
                elif _r32(v - val[k]) > ph:
                    val[k] = v
                    pos[k] = i
            else:
                if v > val[k]:
                    val[k] = v
                    pos[k] = i
                if k == 0 and val[0] > thr[0]:
                    masked[1] = pos[0] + wl[0]
                    pos[1] = -1
                    val[1] = FLT_MAX
                    valid[1] = False
                if _r32(val[k] - v) > ph and val[k] > thr[k]:
                    valid[k] = True
                if valid[k] and (i - pos[k]) > wl[k] // 2:
                    out.append(pos[k])
                    pos[k] = -1
                    val[k] = v
                    valid[k] = False
    return np.array(out, dtype=np.int64)


def events_from_peaks(p, s, q, n):
    """create_events / create_event: structured array (start, length, mean, stdv) with the reference's types"""
    p = np.asarray(p, dtype=np.int64)
    p = p[(p > 0) & (p < n)]
    if len(p) == 0:
        starts, ends = np.array([0], dtype=np.uint64), np.array([n], dtype=np.uint64)
    else:
        starts = np.concatenate([[0], p]).astype(np.uint64)
        ends = np.concatenate([p, [n]]).astype(np.uint64)
    length = (ends - starts).astype(f32)
    si, ei = starts.astype(np.int64), ends.astype(np.int64)
    mean = (s[ei] - s[si]).astype(f32) / length
    var = (q[ei] - q[si]).astype(f32) / length - mean * mean
    stdv = np.sqrt(np.fmax(var, f32(0)))
    ev = np.zeros(len(starts), dtype=[("start", "<u8"), ("length", "<f4"), ("mean", "<f4"), ("stdv", "<f4")])
    ev["start"], ev["length"], ev["mean"], ev["stdv"] = starts, length, mean, stdv
    return ev


def detect_events(pa, params=DEFAULTS):
    w1, w2, thr1, thr2, ph = params
    pa = np.asarray(pa, dtype=f32)
    n = len(pa)
    if n == 0:
        raise ValueError("empty read")
    s, q = sum_sumsq(pa)
    t1, t2 = tstat(s, q, n, w1), tstat(s, q, n, w2)
    return events_from_peaks(peaks(t1, t2, w1, w2, thr1, thr2, ph), s, q, n)


def basecalled_table(ev, sample_rate, start_time, **_):
    """event_table_to_basecalled_table: raw_start, raw_length, mean, stdv, start (s), length (s)"""
    sr, st = f32(sample_rate), f32(start_time)
    out = np.zeros(len(ev), dtype=[("raw_start", "<i8"), ("raw_length", "<i8"), ("mean", "<f8"), ("stdv", "<f8"),
                                   ("start", "<f8"), ("length", "<f8")])
    out["raw_start"] = ev["start"].astype(np.int64)
    out["raw_length"] = ev["length"].astype(np.uint64).astype(np.int64)
    out["mean"] = ev["mean"].astype(f64)
    out["stdv"] = ev["stdv"].astype(f64)
    out["start"] = ev["start"].astype(f64) / f64(sr) + f64(st / sr)
    out["length"] = (ev["length"] / sr).astype(f64)
    return out


def kmer_strings(seq, k, rna):
    """build_kmer_list (impl/eventAligner.c:772-790)"""
    if rna:
        seq = seq.replace("U", "T")
        return [seq[i:i + k][::-1] for i in range(len(seq) - k + 1)]
    return [seq[i:i + k] for i in range(len(seq) - k + 1)]


def emission(mu, sd, e, scale, shift, var=1.0):
    """emissions_signal_strawManGetKmerEventMatchProbWithDescaling_MeanOnly (impl/stateMachine.c:557-605)"""
    c = -0.91893853320467267 - math.log(sd)
    en = (e + var * mu - scale * mu - shift) / var
    a = (en - mu) / sd
    return math.log(1 / var) + (c + (-0.5 * a * a))


def base_event_map(kmer_idx, event_idx, n_events, n_kmers, rna):
    """alignment_to_base_event_map / rna_alignment_to_base_event_map over an alignment in ascending order: per event
    (indexed as the aligned table is) the mapped k-mer position (-1: none) and the move"""
    km = np.full(n_events, -1, dtype=np.int64)
    mv = np.zeros(n_events, dtype=np.int64)
    prev_e = -1
    if not rna:
        prev_k = 0
        for k, e in zip(kmer_idx.tolist(), event_idx.tolist()):
            if e == prev_e:
                if k == prev_k:
                    continue                     # the reference prints an error and maps nothing
                if prev_k == 0:
                    continue
                km[e] = k
                mv[e] += k - prev_k
            else:
                km[e] = k
                mv[e] = 0 if k == prev_k else k - prev_k
            prev_k, prev_e = k, e
    else:
        prev_k = n_kmers - 1
        for k, e in zip(kmer_idx.tolist()[::-1], event_idx.tolist()[::-1]):
            if e == prev_e:
                if k == prev_k:
                    continue
                km[e] = k
                mv[e] += prev_k - k
            else:
                km[e] = k
                mv[e] = 0 if k == prev_k else prev_k - k
            prev_k, prev_e = k, e
    return km, mv
