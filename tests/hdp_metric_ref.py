"""numpy restatement of the HDP distribution metrics (kl_divergence, hellinger_distance, l2_distance, shannon_jensen_distance:
impl/hdp.c:2666-2767) and of grid_spline_interp / linspace (impl/hdp_math_utils.c:471-510), for the tests of sa_hdp_distances and
its relatives.  Vectorised over pairs, sequential over the grid, every operation a separate ufunc call in the reference's order
(numpy does not fuse them, so each is rounded once, as in the reference's build); `log` is glibc's through math.log, element by
element.  No clamping: zeros, infinities and NaNs flow through as IEEE arithmetic takes them."""
import math

import numpy as np

KL, HELLINGER, L2, SHANNON_JENSEN = 0, 1, 2, 3
METRICS = (KL, HELLINGER, L2, SHANNON_JENSEN)
EPS = 2.0 ** -52


def _log_one(v):
    if v > 0.0:
        return math.log(v)          # (math.log(inf) is inf)
    if v == 0.0:
        return -math.inf
    return math.nan                 # negative or NaN


_log_obj = np.frompyfunc(_log_one, 1, 1)


def log(a):
    return _log_obj(np.asarray(a, dtype=np.float64)).astype(np.float64)


def _point(metric, p, q):
    """(point function, sum of the absolute values of its two log terms as they enter it -- Shannon-Jensen's carry its factor 0.5;
    0 for the metrics without a logarithm)"""
    if metric == KL:
        t1 = p * log(p / q)
        t2 = q * log(q / p)
        return t1 + t2, np.abs(t1) + np.abs(t2)
    if metric == HELLINGER:
        return np.sqrt(p * q), 0.0 * p
    if metric == L2:
        diff = p - q
        return diff * diff, 0.0 * p
    mean = 0.5 * (p + q)
    t1 = p * log(p / mean)
    t2 = q * log(q / mean)
    return 0.5 * (t1 + t2), 0.5 * (np.abs(t1) + np.abs(t2))


def integral(grid, P, Q, metric):
    """Row k of P against row k of Q (both n x len(grid)): (the trapezoid sum before the metric's final step, the trapezoid sum S of
    the absolute values of the two log terms)."""
    grid = np.asarray(grid, dtype=np.float64)
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    with np.errstate(all="ignore"):
        acc = np.zeros(P.shape[0])
        s_acc = np.zeros(P.shape[0])
        left, s_left = _point(metric, P[:, 0], Q[:, 0])
        for i in range(1, len(grid)):
            right, s_right = _point(metric, P[:, i], Q[:, i])
            dx = grid[i] - grid[i - 1]
            acc = acc + 0.5 * (left + right) * dx
            s_acc = s_acc + 0.5 * (s_left + s_right) * dx
            left, s_left = right, s_right
    return acc, s_acc


def final(metric, acc):
    with np.errstate(all="ignore"):
        if metric == KL:
            return acc
        if metric == HELLINGER:
            return np.sqrt(1.0 - acc)
        return np.sqrt(acc)


def tri_pairs(n):
    """(i, j) of every element of the triangular vector, in its order: index (i - 1) * i / 2 + j for i > j"""
    i = np.repeat(np.arange(n), np.arange(n))
    j = np.concatenate([np.arange(k) for k in range(n)]) if n > 1 else np.zeros(0, dtype=np.int64)
    return i.astype(np.int64), j.astype(np.int64)


def all_pairs(grid, rows, metric):
    """(distance, integral, S) of every pair i > j, triangular order: row i is the first distribution"""
    rows = np.asarray(rows, dtype=np.float64)
    i, j = tri_pairs(rows.shape[0])
    acc, s = integral(grid, rows[i], rows[j], metric)
    return final(metric, acc), acc, s


def linspace(start, stop, length):
    n = length - 1
    dx = (stop - start) / float(n)
    lin = np.empty(length)
    for i in range(n):
        lin[i] = start + i * dx
    lin[n] = stop
    return lin


def spline_interp(query, x, y, slope):
    """grid_spline_interp for an array of queries against one row; the left knot index is kept within [0, len(x) - 2] (the
    reference reads past its arrays where the truncated quotient reaches the last knot)"""
    q = np.asarray(query, dtype=np.float64)
    n = len(x) - 1
    with np.errstate(all="ignore"):
        below = y[0] - slope[0] * (x[0] - q)
        above = y[n] + slope[n] * (q - x[n])
        dx = x[1] - x[0]
        quotient = (q - x[0]) / dx
        il = np.minimum(np.trunc(np.where(quotient >= 0, quotient, 0.0)), n - 1).astype(np.int64)
        ir = il + 1
        dy = y[ir] - y[il]
        a = slope[il] * dx - dy
        b = dy - slope[ir] * dx
        t_left = (q - x[il]) / dx
        t_right = 1.0 - t_left
        inside = t_right * y[il] + t_left * y[ir] + t_left * t_right * (a * t_right + b * t_left)
    return np.where(q <= x[0], below, np.where(q >= x[n], above, inside))


def density(query, x, y, slope):
    """dir_proc_density (impl/hdp.c:2588-2612): the spline, clamped at zero"""
    v = spline_interp(query, x, y, slope)
    return np.where(v > 0.0, v, 0.0)


def resolve_row(observed, parent, row_of_dp, dp):
    """the row of a DP's nearest observed ancestor (impl/hdp.c:2600-2602)"""
    while not observed[dp]:
        dp = parent[dp]
    return int(row_of_dp[dp])


def check_against(metric, got, want, acc_want, s, label=""):
    """The comparison rules of the GPU tests.  L2 and Hellinger hold only correctly rounded operations: bit for bit.  KL (and the
    Shannon-Jensen divergence) may differ by the two logarithms: each implementation is within 1 ulp, so the two differ by at most
    2 ulp of a log term, and the bound is twice that: 4 eps S per pair.  The Shannon-Jensen distance is the square root of its
    divergence: the bound goes through the derivative, plus one rounding of the root."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    if metric in (L2, HELLINGER):
        bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
        assert len(bad) == 0, (label, metric, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
        return 0.0
    assert np.array_equal(np.isnan(got), np.isnan(want)), (label, metric, "NaN positions differ")
    ok = ~np.isnan(want) & np.isfinite(want)
    assert np.array_equal(got[~ok & ~np.isnan(want)], want[~ok & ~np.isnan(want)]), (label, metric, "infinities differ")
    bound = 4.0 * EPS * s
    if metric == KL:
        err = np.abs(got[ok] - want[ok])
        worst = float(np.max(err / np.maximum(EPS * s[ok], 1e-300))) if ok.any() else 0.0
        print("%s metric %d: worst |got - want| = %.3g eps S" % (label, metric, worst))
        assert np.all(err <= bound[ok]), (label, metric, worst)
        return worst
    div = acc_want
    zero = ok & (div == 0.0)
    assert np.all(got[zero] == 0.0), (label, "a zero divergence must give a zero distance")
    assert not np.any(ok & (div < 0.0)), (label, "negative divergence in the reference")
    pos = ok & (div > 0.0)
    window = pos & (div < 1000.0 * bound)
    assert not window.any(), (label, "pairs with a divergence within 1000 bounds of zero", int(window.sum()))
    err = np.abs(got[pos] - want[pos])
    allowed = bound[pos] / (2.0 * np.sqrt(div[pos])) + EPS * want[pos]
    worst = float(np.max(err / allowed)) if pos.any() else 0.0
    print("%s metric %d: worst |got - want| = %.3g of the allowance" % (label, metric, worst))
    assert np.all(err <= allowed), (label, metric, worst)
    return worst
