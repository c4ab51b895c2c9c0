"""Plain-Python restatements of the two call folds (sa_calls.hip), written from the reference's code, and the comparisons the GPU
tests make against them.  Sites: MarginalizeFullVariants.get_data (src/signalalign/variantCaller.py:141-172).  Positions:
CallMethylation.call_methyls (src/signalalign/scripts/alignmentAnalysisLib.py:217-233).  tests/test_host_calls_ref.py pins both
on a hand-worked table, without a device."""
import numpy as np


def printed_units(prob_e7):
    """"%f" of prob_e7 / 1e7 in integers of 1e-6 (the posterior column of the full TSV)"""
    p = np.asarray(prob_e7, dtype=np.int64)
    k, rem = p // 10, p % 10
    out = k + (rem > 5)
    for i in np.nonzero(rem == 5)[0]:
        out[i] = int(("%f" % (int(p[i]) / 1e7)).replace(".", ""))
    return out


RECORD_DTYPE = np.dtype([("x", np.int32), ("kmer_id", np.int32), ("prob_e7", np.int64)])


def kmer_id(kmer, alphabet):
    """a k-mer's index in the model's table: its letters as digits of base len(alphabet), first letter most significant"""
    v = 0
    for c in kmer:
        v = v * len(alphabet) + alphabet.index(c)
    return v


def records(rows, alphabet):
    """[(x, path k-mer, prob_e7)] as the structured array the restatements and the *_records entries read"""
    return np.array([(x, kmer_id(kmer, alphabet), p) for x, kmer, p in rows], dtype=RECORD_DTYPE)


# The prob_e7 of the rows of a planted position bucket: they print 0.000001, 0.499999 and 1.000000 in a fixed irregular mix, so
# that a letter's serial double sum depends on the order of its rows (tests/test_host_calls_ref.py shows it does).
BUCKET_PROB_E7 = (10, 4999990, 10000000)


def bucket_prob_e7(n, salt=0):
    return [BUCKET_PROB_E7[(i * i + i // 3 + salt) % 3] for i in range(n)]


def restate_sites(pairs, ref, k, alphabet, amb):
    """get_data (:141-172) over one job's pairs: a site is a k-mer index whose last letter is an ambiguity letter; per letter
    the printed posteriors of the pairs whose path k-mer ends in it, summed; normalised over the site's letters; sites with a
    zero total are not reported.  Returns {x: (letters, units, prob)}."""
    units = printed_units(pairs["prob_e7"])
    last = np.array([alphabet[i] for i in (pairs["kmer_id"] % len(alphabet))])
    acc = {}
    for x, l, u in zip(pairs["x"].tolist(), last.tolist(), units.tolist()):
        c = ref[x + k - 1]
        if c not in amb:
            continue
        letters = "".join(sorted(set(amb[c])))
        if x not in acc:
            acc[x] = (letters, [0] * len(letters))
        if l in letters:
            acc[x][1][letters.index(l)] += u
    out = {}
    for x, (letters, u) in acc.items():
        tot = sum(u)
        if tot > 0:
            out[x] = (letters, u, [np.float64(v) / np.float64(tot) for v in u])
    return out


def check_site_calls(got, exp):
    assert sorted(exp) == got["x"].tolist()
    assert np.all(np.diff(got["x"]) > 0)
    for i, x in enumerate(got["x"].tolist()):
        letters, u, p = exp[x]
        n = len(letters)
        assert got["letters"][i] == letters
        assert got["units"][i][:n].tolist() == u, x
        assert got["prob"][i][:n].tobytes() == np.asarray(p, dtype=np.float64).tobytes(), x
        assert not got["units"][i][n:].any() and not got["prob"][i][n:].any()


def restate_positions(pairs, ref, k, alphabet, amb):
    """call_methyls over one job's rows: every row whose k-mer covers an ambiguous position adds the posterior the TSV prints,
    read back with float(), to the letter its path k-mer has there -- serially, in row order, from 0; the total runs over the
    position's sorted letters; each sum is divided by it.  Where every covering row prints 0.000000 the total is 0 and the
    reference raises ZeroDivisionError (:230-233); the library's rule is pinned instead: the position is reported with its rows
    and every probability 0.0, as a site with a zero sum has.  Returns {p: (letters, n_rows, sums, probs)}."""
    n_alpha = len(alphabet)
    acc = {}
    for x, kmer_id, prob_e7 in zip(pairs["x"].tolist(), pairs["kmer_id"].tolist(), pairs["prob_e7"].tolist()):
        value = None
        digits = []
        v = kmer_id
        for _ in range(k):
            digits.append(alphabet[v % n_alpha])
            v //= n_alpha
        digits.reverse()
        for d in range(k):
            c = ref[x + d]
            if c not in amb:
                continue
            if value is None:
                value = float("%f" % (prob_e7 / 1e7))
            letters = "".join(sorted(set(amb[c])))
            entry = acc.setdefault(x + d, [letters, 0, [0] * len(letters)])
            if digits[d] in letters:
                entry[1] += 1
                entry[2][letters.index(digits[d])] += value
    out = {}
    for p, (letters, n, sums) in acc.items():
        if n == 0:
            continue
        total = 0
        for s in sums:
            total += s
        out[p] = (letters, n, [float(s) for s in sums], [s / total if total != 0 else 0.0 for s in sums])
    return out


def check_position_calls(got, exp, pairs):
    assert got["p"].tolist() == sorted(exp)
    for i, p in enumerate(got["p"].tolist()):
        letters, n, sums, probs = exp[p]
        m = len(letters)
        assert got["letters"][i] == letters
        assert int(got["n_rows"][i]) == n, p
        assert got["sum"][i][:m].tobytes() == np.asarray(sums, dtype=np.float64).tobytes(), (p, got["sum"][i][:m], sums)
        assert got["prob"][i][:m].tobytes() == np.asarray(probs, dtype=np.float64).tobytes(), (p, got["prob"][i][:m], probs)
        assert not got["sum"][i][m:].any() and not got["prob"][i][m:].any()
    if len(pairs):
        assert got["x_min"] == int(pairs["x"].min()) and got["x_max"] == int(pairs["x"].max())
    else:
        assert got["x_min"] == -1 and got["x_max"] == -1
