"""numpy restatement of the k-mer mixture fit (include/signalalign_hip.h, sa_kmer_table_mixture) and of the two host helpers
around it.  Nothing here calls the library: the tests compare the library against this file, and this file against sklearn.

The fit of one (strand, k-mer), x = descaled_units / 1e6 in sa_kmer_table_rows order:
  start   labels min(K - 1, floor(K (x - lo) / (hi - lo))) (all 0 when hi == lo), one M-step on the one-hot responsibilities;
          the loop starts from (weights, means, sds) -- the sd, not the variance, is what is carried, as for an explicit start
  M-step  nk = sum r + 10 eps, mean = sum r x / nk, var = sum r (x - mean)^2 / nk + reg_covar, weight = nk / sum nk
  E-step  lp = -(log 2 pi + ((x - mean) / sd)^2) / 2 - log sd + log weight, norm = logsumexp(lp), r = exp(lp - norm),
          lower_bound = mean(norm)
  loop    lb = -inf; for it = 1 .. max_iter: prev = lb, E-step, M-step, converged when |lb - prev| < tol
which is sklearn.mixture.GaussianMixture.fit with n_init = 1 started from weights_init / means_init / precisions_init."""
import itertools

import numpy as np

EPS10 = 10.0 * np.finfo(np.float64).eps
LOG_2PI = float(np.log(2.0 * np.pi))


def m_step(x, r, reg_covar):
    nk = r.sum(axis=0) + EPS10
    mean = (r * x[:, None]).sum(axis=0) / nk
    var = (r * (x[:, None] - mean[None, :]) ** 2).sum(axis=0) / nk + reg_covar
    return nk / nk.sum(), mean, np.sqrt(var)


def e_step(x, w, mean, sd):
    z = (x[:, None] - mean[None, :]) / sd[None, :]
    lp = -0.5 * (LOG_2PI + z * z) - np.log(sd)[None, :] + np.log(w)[None, :]
    mx = lp.max(axis=1)
    norm = mx + np.log(np.exp(lp - mx[:, None]).sum(axis=1))
    return float(norm.sum() / len(x)), np.exp(lp - norm[:, None])


def start(x, K, reg_covar=1e-6):
    """(weights, means, sds) of the deterministic start"""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = x.min(), x.max()
    if hi == lo:
        label = np.zeros(len(x), dtype=np.int64)
    else:
        label = np.minimum(K - 1, np.floor(K * (x - lo) / (hi - lo))).astype(np.int64)
    r = np.zeros((len(x), K))
    r[np.arange(len(x)), label] = 1.0
    return m_step(x, r, reg_covar)


def fit(x, K, max_iter=100, tol=1e-3, reg_covar=1e-6, init=None, changes=None):
    """dict(n, n_iter, converged, status, lower_bound, weight, mean, sd); init: (weights, means, sds) or None.
    changes: a list that receives |lb - prev| of every iteration (to see how near the tol threshold a case comes)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if n < K:
        return dict(n=n, n_iter=0, converged=0, status=1, lower_bound=0.0, weight=np.zeros(K), mean=np.zeros(K), sd=np.zeros(K))
    w, mean, sd = start(x, K, reg_covar) if init is None else [np.asarray(a, dtype=np.float64) for a in init]
    lb, it, converged = -np.inf, 0, 0
    while it < max_iter:
        it += 1
        prev = lb
        lb, r = e_step(x, w, mean, sd)
        w, mean, sd = m_step(x, r, reg_covar)
        if changes is not None:
            changes.append(abs(lb - prev))
        if abs(lb - prev) < tol:
            converged = 1
            break
    return dict(n=n, n_iter=it, converged=converged, status=0, lower_bound=lb, weight=w, mean=mean, sd=sd)


def sklearn_fit(x, K, max_iter, tol, reg_covar=1e-6):
    """the same fit by sklearn, from the same start: (weights, means, sds, n_iter, converged, lower_bound)"""
    import warnings
    from sklearn.mixture import GaussianMixture
    x = np.asarray(x, dtype=np.float64)
    w, mean, sd = start(x, K, reg_covar)
    g = GaussianMixture(K, tol=tol, max_iter=max_iter, reg_covar=reg_covar, weights_init=w, means_init=mean.reshape(-1, 1),
                        precisions_init=(1.0 / (sd * sd)).reshape(-1, 1, 1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (ConvergenceWarning of the tol = 0 cases)
        g.fit(x.reshape(-1, 1))
    return (g.weights_.copy(), g.means_[:, 0].copy(), np.sqrt(g.covariances_[:, 0, 0]), int(g.n_iter_), int(bool(g.converged_)),
            float(g.lower_bound_))


def planted(seed, n, parts):
    """n values of a planted mixture, parts = [(weight, mean, sd), ...], rounded to 1e-6 as the table holds them"""
    rng = np.random.RandomState(seed)
    wts = np.array([p[0] for p in parts], dtype=np.float64)
    comp = rng.choice(len(parts), size=n, p=wts / wts.sum())
    mu = np.array([p[1] for p in parts])[comp]
    sg = np.array([p[2] for p in parts])[comp]
    return np.round(mu + sg * rng.standard_normal(n), 6)


TWO = [(0.4, 78.0, 1.2), (0.6, 84.0, 1.5)]
THREE = [(0.3, 76.0, 1.0), (0.3, 81.0, 1.2), (0.4, 86.0, 1.4)]


def host_cases():
    """(name, x, K, max_iter, tol) of the CPU comparison with sklearn: n from 2 to 5000, K from 1 to 4, both loop settings"""
    out = []
    seed = 100
    for K in (1, 2, 3, 4):
        for n in (max(K, 2), 7, 64, 257, 1000, 5000):
            seed += 1
            x = planted(seed, n, TWO if seed % 2 else THREE)
            out.append(("K%d_n%d_fixed25" % (K, n), x, K, 25, 0.0))
            out.append(("K%d_n%d_defaults" % (K, n), x, K, 100, 1e-3))
    return out


# ---- the host helpers -----------------------------------------------------------------------------------------------------------
def motif_kmer_pairs(k, canonical, modified, alphabet="ATGC"):
    """sorted, de-duplicated [canonical k-mer, modified k-mer] of every window of k letters over the modified position; the
    canonical k-mer replaces the FIRST occurrence of the new letter"""
    canonical, modified = canonical.upper(), modified.upper()
    pos = [i for i in range(len(canonical)) if canonical[i] != modified[i]]
    assert len(canonical) == len(modified) and len(pos) == 1 and set(canonical) <= set("ATGC")
    pos = pos[0]
    old, new = canonical[pos], modified[pos]
    pairs = set()
    for i in range(k):
        s = pos + i - k + 1
        nf, nb = max(0, -s), max(0, s + k - len(modified))
        core = modified[max(s, 0):min(s + k, len(modified))]
        for f in itertools.product(alphabet, repeat=nf):
            for b in itertools.product(alphabet, repeat=nb):
                kmer = "".join(f) + core + "".join(b)
                at = kmer.find(new)
                pairs.add((kmer[:at] + old + kmer[at + 1:], kmer))
    return sorted(pairs)


def assign(means, canonical_mean):
    """closest_to_canonical for two components: (match, other, distance)"""
    min_index, min_distance = 0, 1000
    for i in range(2):
        d = abs(means[i] - canonical_mean)
        if d < min_distance:
            min_index, min_distance = i, d
    return min_index, 1 - min_index, float(min_distance)
