"""Restatement of the Gaussian emission training the library runs on the GPU (sa_kmer_table_*, sa_model_write_trained):
generate_top_n_kmers_from_sa_output (build_alignments.py:76-275), train_normal_emmissions (trainModels.py:735-828) and
HmmModel.write (hiddenMarkovModel.py:304-336), in plain Python / numpy with exact rational statistics.  Rows are
(strand, kmer_id, descaled text, prob text) as the -s 2 file prints them; run order is the order of the list."""
import math
from fractions import Fraction

import numpy as np

NDTRI_075 = 0.6744897501960817


def units(text):
    """a "%f" string in integers of 1e-6 and its negative-zero flag"""
    neg = text.startswith("-")
    a, b = text.lstrip("-").split(".")
    u = int(a) * 1000000 + int(b)
    return (-u if neg else u), int(neg and u == 0)


def f6(v):
    return "%f" % v


def descaled(e, level, scale, shift, var):
    """signalMachine.c descale(): Python does not contract to fma"""
    return (e + var * level - scale * level - shift) / var


def top_n(rows, n, min_prob):
    """rows: list of (strand, kmer_id, desc_text, prob_text) in run order -> {(strand, kmer_id): [row, ...]} posterior
    descending, then run order"""
    groups = {}
    for r in rows:
        if float(r[3]) >= min_prob:
            groups.setdefault((r[0], r[1]), []).append(r)
    out = {}
    for key, g in groups.items():
        order = sorted(range(len(g)), key=lambda i: (-units(g[i][3])[0], i))
        out[key] = [g[i] for i in order[:n]]
    return out


def table_lines(kept, alphabet, k):
    """the table file: strand t then c, k-mer ascending, rows as kept"""
    lines = []
    for strand in ("t", "c"):
        for (s, km) in sorted(x for x in kept if x[0] == strand):
            name = kmer_name(km, alphabet, k)
            lines += ["%s\t%s\t%s\t%s\n" % (name, s, r[2], r[3]) for r in kept[(s, km)]]
    return "".join(lines)


def kmer_name(km, alphabet, k):
    a = sorted(alphabet)
    out = []
    for _ in range(k):
        out.append(a[km % len(a)])
        km //= len(a)
    return "".join(reversed(out))


def stats(values_units, use_median):
    """(n, m, s) of integer values in 1e-6, exactly as the contract defines them"""
    x = sorted(int(v) for v in values_units)
    n = len(x)
    if n == 0:
        return 0, 0.0, 0.0
    if use_median:
        med2 = x[(n - 1) // 2] + x[n // 2]
        dev = sorted(abs(2 * v - med2) for v in x)
        mad4 = dev[(n - 1) // 2] + dev[n // 2]
        return n, float(Fraction(med2, 2 * 10**6)), float(Fraction(mad4, 4 * 10**6)) / NDTRI_075
    S = sum(x)
    Q = sum(v * v for v in x)
    return n, float(Fraction(S, n * 10**6)), math.sqrt(float(Fraction(n * Q - S * S, n * n * 10**12)))


def read_model(path):
    with open(path) as f:
        head = f.readline().split()
        trans = [float(t) for t in f.readline().split()]
        params = [float(t) for t in f.readline().split()]
    return head, trans, params


def write_trained(prior_path, st, out_path, weight=100.0, min_sd=0.0, mod_only=False, kmers=None):
    """st: {kmer_id: (n, m, s)}; kmers: set of k-mer names (training-k-mers file) or None"""
    head, trans, params = read_model(prior_path)
    alphabet, k = head[2], int(head[3])
    means, sds, lambdas = params[0::5], params[1::5], params[4::5]
    for km, (n, m, s) in st.items():
        if n == 0:
            continue
        name = kmer_name(km, alphabet, k)
        if mod_only and len(set(name) - {"A", "T", "G", "C"}) == 0:
            continue
        if kmers is not None and name not in kmers:
            continue
        mean = np.float64(m) * n
        sd = np.float64(s) * n
        normal_mean, normal_sd = means[km] * weight, sds[km] * weight
        mu = (mean + normal_mean) / (n + weight)
        sigma = np.max([(sd + normal_sd) / (n + weight), min_sd])
        means[km], sds[km] = mu, sigma
        lambdas[km] = (mu ** 3) / (sigma ** 2)
    params[0::5], params[1::5], params[4::5] = means, sds, lambdas
    with open(out_path, "w") as f:
        f.write("3\t%d\t%s\t%d\n" % (int(head[1]), alphabet, k))
        for t in trans[:-1]:
            f.write("%s\t" % str(t))
        f.write("%s\n" % str(trans[-1]))
        for v in params:
            f.write("%s\t" % v)
        f.write("\n")


RUN_BITS = 40
RUN_MASK = (1 << RUN_BITS) - 1
LEVELS = (50, 40, 30, 20, 10, 0)


def min_units(min_prob):
    """the smallest printed posterior, in units, with float(text) >= min_prob"""
    u = 0
    while u <= 1000000 and not (u / 1e6 >= min_prob):
        u += 1
    return u


def key(prob_units, ordinal):
    """a row's selection key as sa_train.hip defines it"""
    return (int(prob_units) << RUN_BITS) | (RUN_MASK - int(ordinal))


def top_n_arrays(kmer, prob_units, n, min_units, first_ordinal=0):
    """top_n over integer arrays: row i has run ordinal first_ordinal + i -> {kmer_id: kept run ordinals (int64 array), posterior
    descending, then ordinal ascending}"""
    kmer = np.asarray(kmer, dtype=np.int64)
    pu = np.asarray(prob_units, dtype=np.int64)
    idx = np.nonzero(pu >= min_units)[0]
    idx = idx[np.lexsort((idx, -pu[idx], kmer[idx]))]   # k-mer, then posterior descending, then run order
    km = kmer[idx]
    start = np.nonzero(np.r_[True, km[1:] != km[:-1]])[0] if len(km) else np.zeros(0, dtype=np.int64)
    end = np.r_[start[1:], len(km)]
    return {int(km[a]): idx[a:min(b, a + n)] + first_ordinal for a, b in zip(start.tolist(), end.tolist())}


def settle_shift(keys, n):
    """The radix selection of one k-mer written out: -> (shift, owner lane, digit) of the level that settles it, (None, None,
    None) if it has at most n candidates (all are kept at the first level)."""
    keys = [int(k) for k in keys]
    if len(keys) <= n:
        return None, None, None
    need = n
    for shift in LEVELS:
        count = {}
        for k in keys:
            d = (k >> shift) & 1023
            count[d] = count.get(d, 0) + 1
        acc = 0
        for digit in sorted(count, reverse=True):   # from the top bin down to the one holding the need-th largest key
            if acc + count[digit] >= need:
                break
            acc += count[digit]
        need -= acc
        if count[digit] == need or shift == 0:
            return shift, digit // 16, digit
        keys = [k for k in keys if ((k >> shift) & 1023) == digit]
