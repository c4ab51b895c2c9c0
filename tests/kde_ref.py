"""numpy / plain-Python restatements of the two comparisons of include/signalalign_hip.h, in the order of operations the
header states:

  kde_log_density    sa_kmer_table_kde: sklearn's KernelDensity(kernel="gaussian").score_samples, one accumulator per query
                     point, the rows added in ascending order (reverse=True: descending, for the summation-order noise floor)
  hdp_vs_gaussian    sa_hdp_state_vs_gaussian: scipy.stats.entropy in bits, hellinger2 and the mode's distance from the mean,
                     every sum one accumulator in grid order

Both are pinned by the libraries themselves in tests/golden/kde/ (tests/golden/make_kde_fixtures.py)."""
import math

import numpy as np

KDE_CUT = 64.0                       # KT_KDE_CUT (sa_train.hip)
HALF_LOG_2PI = 0.9189385332046727
SQRT_2PI = 2.5066282746310002        # scipy's _norm_pdf_C
LN2 = 0.6931471805599453
SQRT2 = 1.4142135623730951
DBL_MIN = 2.2250738585072014e-308


def kde_log_density(units, q, h, reverse=False):
    """units: the k-mer's descaled_units (integers of 1e-6), any order; q: query points; -> log density at every q"""
    q = np.asarray(q, dtype=np.float64)
    u = np.sort(np.asarray(units, dtype=np.int64))
    if len(u) == 0:
        return np.full(len(q), -np.inf)
    x = u.astype(np.float64) / 1e6
    r = 1.0 / float(h)
    dmin = np.full(len(q), np.inf)
    for xi in x:
        dmin = np.minimum(dmin, np.abs(q - xi))
    z = dmin * r
    E = -0.5 * (z * z)
    S = np.zeros(len(q))
    for xi in (x[::-1] if reverse else x):
        z = (q - xi) * r
        e = -0.5 * (z * z) - E
        m = e >= -KDE_CUT
        S[m] += np.exp(e[m])
    return (E + np.log(S)) - ((math.log(float(len(x))) + math.log(float(h))) + HALF_LOG_2PI)


def kde_closed_form(units, q, h):
    """the definition without shift-by-nearest bookkeeping of its own: scipy's logsumexp over all rows"""
    from scipy.special import logsumexp
    x = np.asarray(units, dtype=np.float64) / 1e6
    q = np.asarray(q, dtype=np.float64)
    e = -0.5 * ((q[:, None] - x[None, :]) / h) ** 2
    return logsumexp(e, axis=1) - math.log(len(x)) - math.log(h) - HALF_LOG_2PI


def rel_entr(a, b):
    """scipy.special.rel_entr (1.15)"""
    if math.isnan(a) or math.isnan(b):
        return math.nan
    if a <= 0 or b <= 0:
        return 0.0 if (a == 0 and b >= 0) else math.inf
    ratio = a / b
    if 0.5 < ratio < 2:
        return a * math.log1p((a - b) / b)
    if DBL_MIN < ratio < math.inf:
        return a * math.log(ratio)
    return a * (math.log(a) - math.log(b))


def norm_pdf(g, mean, sd):
    z = (g - mean) / sd
    return math.exp(-(z * z) / 2.0) / SQRT_2PI / sd


def hdp_vs_gaussian(p, grid, mean, sd, reverse=False):
    """-> (kl_bits, hellinger, mode_delta, status) of one observed DP's row p; reverse: the sums from the last grid point down"""
    p = [float(v) for v in p]
    grid = [float(v) for v in grid]
    qv = [norm_pdf(g, float(mean), float(sd)) for g in grid]
    order = range(len(p) - 1, -1, -1) if reverse else range(len(p))
    sum_p = sum_q = sum_h = 0.0
    for i in order:
        sum_p += p[i]
        sum_q += qv[i]
        d = math.sqrt(p[i]) - math.sqrt(qv[i])
        sum_h += d * d
    kl = 0.0
    for i in order:
        kl += rel_entr(p[i] / sum_p, qv[i] / sum_q)
    kl /= LN2
    arg = max(range(len(p)), key=lambda i: (p[i], -i))   # the first largest
    return kl, math.sqrt(sum_h) / SQRT2, abs(grid[arg] - float(mean)), (0 if math.isfinite(kl) else 2)
