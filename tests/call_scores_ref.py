"""The restatement of the call scores (sa_call_scores_*, include/signalalign_hip.h) in Python integers: auc2, the confusion counts
and the grid counts by np.sort / np.searchsorted on the uint64 views of the scores; the per-read mean as a serial Python float sum;
the two files of sa_call_scores_write as text."""
import numpy as np

GROUP_NAMES = ("t", "c", "all")


def keys(scores):
    """the bit patterns of doubles in [0, 1] as uint64 (-0.0 as +0.0): they order as the doubles do"""
    v = np.array(scores, dtype=np.float64).reshape(-1)
    assert not np.isnan(v).any() and ((v >= 0) & (v <= 1)).all()
    v = v + 0.0                                   # (-0.0 + 0.0 is +0.0)
    return v.view(np.uint64)


def auc2(pos, neg):
    """sum over positives p of 2 #(negatives < p) + #(negatives == p), a Python integer"""
    p, n = keys(pos), np.sort(keys(neg))
    lo, hi = np.searchsorted(n, p, side="left"), np.searchsorted(n, p, side="right")
    return sum(int(a) + int(b) for a, b in zip(lo.tolist(), hi.tolist()))   # 2 lo + (hi - lo)


def count_ge(scores, t):
    """scores >= t, for a threshold that may lie outside [0, 1]"""
    s = np.sort(keys(scores))
    if t <= 0:
        return len(s)
    key = np.array([t], dtype=np.float64).view(np.uint64)[0]
    return len(s) - int(np.searchsorted(s, key, side="left"))


def row(pos, neg, n_bins, threshold):
    n_pos, n_neg = len(pos), len(neg)
    a2 = auc2(pos, neg)
    tp, fp = count_ge(pos, threshold), count_ge(neg, threshold)
    grid = [float(k) / float(n_bins) for k in range(n_bins + 1)]
    return dict(n_pos=n_pos, n_neg=n_neg, auc2=a2, auc=(float(a2) / (2.0 * float(n_pos) * float(n_neg))) if n_pos and n_neg else float("nan"),
                tp=tp, fp=fp, fn=n_pos - tp, tn=n_neg - fp, tp_ge=[count_ge(pos, t) for t in grid], fp_ge=[count_ge(neg, t) for t in grid])


def read_mean(probs):
    """the per-read score: the site probabilities added serially from 0, in the order given, divided by their number"""
    acc = 0
    for p in probs:
        acc += float(p)
    return acc / len(probs)


class Scores:
    """the accumulator: per (level, strand, letter index, class) a list of scores"""

    def __init__(self, letters, n_bins, threshold):
        self.letters, self.n_bins, self.threshold = letters, n_bins, threshold
        self.arr = {}
        self.unlabelled = self.other_sites = 0

    def add(self, level, strand, prob, true_letter):
        """one record: prob per letter, true_letter an index"""
        for l, p in enumerate(prob):
            self.arr.setdefault((level, strand, l, int(l == true_letter)), []).append(float(p))

    def add_records(self, level, strand, prob, true_letter):
        for p, t in zip(np.asarray(prob, dtype=np.float64).reshape(-1, len(self.letters)), true_letter):
            self.add(level, strand, p, int(t))

    def add_site_calls(self, calls, job_map, truth):
        """levels 0 and 1 from Batch.site_calls(): truth a dict (contig, reference_index, mapped strand) -> letter"""
        for c, m in zip(calls, job_map):
            kept = []
            for i, x in enumerate(c["x"].tolist()):
                if c["letters"][i] != self.letters:
                    self.other_sites += 1
                    continue
                prob = c["prob"][i][:len(self.letters)]
                kept.append((m["x0"] + m["x_sign"] * x, prob))
                tl = m["true_letter"]
                if tl < 0:
                    letter = truth.get((m["contig"], m["x0"] + m["x_sign"] * x, m["mapped_strand"]))
                    if letter is None:
                        self.unlabelled += 1
                        continue
                    tl = self.letters.index(letter)
                self.add(0, m["strand"], prob, tl)
            if m["true_letter"] >= 0 and kept:
                kept.sort(key=lambda e: e[0], reverse=m["mapped_strand"] == 1)
                self.add(1, m["strand"], [read_mean([p[l] for _, p in kept]) for l in range(len(self.letters))], m["true_letter"])

    def rows(self):
        """the rows of finish, in its order: level, strand group, letter"""
        out = []
        for level in range(3):
            for g in range(3):
                for l, letter in enumerate(self.letters):
                    strands = (0, 1) if g == 2 else (g,)
                    pos = [v for s in strands for v in self.arr.get((level, s, l, 1), [])]
                    neg = [v for s in strands for v in self.arr.get((level, s, l, 0), [])]
                    if not pos and not neg:
                        continue
                    r = row(pos, neg, self.n_bins, self.threshold)
                    r.update(level=level, group=g, letter=letter)
                    out.append(r)
        return out


def _ratio(a, b):
    return str(float(a) / float(b)) if b else "nan"


def summary_text(rows):
    lines = ["level\tstrand\tletter\tn_pos\tn_neg\tauc\ttp\tfp\ttn\tfn\taccuracy\tprecision\trecall\n"]
    for r in rows:
        lines.append("%d\t%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%s\t%s\t%s\n" % (
            r["level"], GROUP_NAMES[r["group"]], r["letter"], r["n_pos"], r["n_neg"], str(float(r["auc"])), r["tp"], r["fp"], r["tn"], r["fn"],
            _ratio(r["tp"] + r["tn"], r["n_pos"] + r["n_neg"]), _ratio(r["tp"], r["tp"] + r["fp"]), _ratio(r["tp"], r["n_pos"])))
    return "".join(lines)


def curves_text(rows, n_bins):
    lines = ["level\tstrand\tletter\tk\tthreshold\ttp_ge\tfp_ge\ttpr\tfpr\tprecision\n"]
    for r in rows:
        for k in range(n_bins + 1):
            tp, fp = r["tp_ge"][k], r["fp_ge"][k]
            lines.append("%d\t%s\t%s\t%d\t%s\t%d\t%d\t%s\t%s\t%s\n" % (
                r["level"], GROUP_NAMES[r["group"]], r["letter"], k, str(float(k) / float(n_bins)), tp, fp, _ratio(tp, r["n_pos"]),
                _ratio(fp, r["n_neg"]), _ratio(tp, tp + fp)))
    return "".join(lines)


def check_rows(got_rows, got_curves, exp):
    """the rows and curves of CallScores.finish against rows(): the counts and auc2 exactly, auc bit for bit"""
    assert [(int(r["level"]), int(r["group"]), r["letter"].decode()) for r in got_rows] == [(e["level"], e["group"], e["letter"]) for e in exp]
    for g, c, e in zip(got_rows, got_curves, exp):
        for f in ("n_pos", "n_neg", "auc2", "tp", "fp", "tn", "fn"):
            assert int(g[f]) == e[f], (f, e["level"], e["group"], e["letter"], int(g[f]), e[f])
        assert np.float64(g["auc"]).tobytes() == np.float64(e["auc"]).tobytes() or (np.isnan(g["auc"]) and np.isnan(e["auc"]))
        assert c[0].tolist() == e["tp_ge"] and c[1].tolist() == e["fp_ge"]
