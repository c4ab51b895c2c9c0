"""Writes tests/golden/kde/: what scikit-learn and scipy themselves give for the two comparisons of tests/kde_ref.py.

    python tests/golden/make_kde_fixtures.py

  sklearn_kde.npz            KernelDensity(kernel="gaussian", bandwidth=0.5).score_samples on linspace(30, 90, 600) for 64 k-mers
                             of the bundled assignments file: the 60 with the most rows and the first 4 with one row
  scipy_hdp_vs_gaussian.npz  scipy.stats.entropy(base=2) / hellinger2 / the mode's distance for the observed leaf DPs of
                             templateSingleLevelFixed.nhdp against testModelR73_acegot_template.model, at the model's sd and at
                             four times that sd (hiddenMarkovModel.py:775-837 and :1119-1120, written out here)

Needs scikit-learn and scipy; reading the .nhdp is host code of the built library.  Run on a CPU machine, by hand, when the
cases change; the tests only read what it wrote."""
import gzip
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

ASSIGNMENTS = os.path.join(HERE, "hdp", "d6160b0b-a35e-43b5-947f-adaa1abade28.sm.assignments.tsv.gz")
NHDP = os.path.join(HERE, "models", "templateSingleLevelFixed.nhdp")
MODEL = os.path.join(HERE, "models", "testModelR73_acegot_template.model")
GRID = (30.0, 90.0, 600)
BANDWIDTH = 0.5
SD_SCALES = (1.0, 4.0)


def assignment_rows():
    """{k-mer: [event means]} of the bundled file, every strand, in file order"""
    per = {}
    with gzip.open(ASSIGNMENTS, "rt") as f:
        for ln in f:
            t = ln.split()
            if t:
                per.setdefault(t[0], []).append(float(t[2]))
    return per


def kde_kmers(per):
    by_count = sorted(per, key=lambda k: (-len(per[k]), k))
    return by_count[:60] + sorted(k for k in per if len(per[k]) == 1)[:4]


def sklearn_kde():
    from sklearn.neighbors import KernelDensity
    per = assignment_rows()
    kmers = kde_kmers(per)
    x = np.linspace(*GRID)
    out = np.zeros((len(kmers), len(x)))
    for i, k in enumerate(kmers):
        kd = KernelDensity(kernel="gaussian", bandwidth=BANDWIDTH).fit(np.asarray(per[k])[:, None])
        out[i] = kd.score_samples(x[:, None])
    return dict(kmers=np.array(kmers), n_rows=np.array([len(per[k]) for k in kmers], dtype=np.int64), x=x,
                bandwidth=np.array([BANDWIDTH]), log_density=out)


def scipy_hdp_vs_gaussian():
    from scipy.spatial.distance import euclidean
    from scipy.stats import entropy, norm
    import signalalign_amd as sa
    from signalalign_amd import synth
    s = sa.HdpState(NHDP)
    alpha, k, _, tab = synth.parse_model_table(MODEL)
    assert s.alphabet() == alpha and int(s.info.kmer_length) == k
    tab = np.asarray(tab).reshape(-1, 5)
    n_kmers = len(alpha) ** k
    observed, row_of, post, grid = s.array("observed"), s.array("row_of_dp"), s.array("post"), s.array("grid")
    ids = np.array([d for d in range(n_kmers) if observed[d]], dtype=np.int64)
    z = dict(dp_ids=ids, mean=tab[ids, 0], sd=tab[ids, 1], sd_scales=np.array(SD_SCALES))
    for scale in SD_SCALES:
        kl, hel, delta = [], [], []
        for d in ids:
            p = post[row_of[d]]
            q = norm.pdf(grid, tab[d, 0], scale * tab[d, 1])
            kl.append(entropy(pk=p, qk=q, base=2))
            hel.append(euclidean(np.sqrt(p), np.sqrt(q)) / np.sqrt(2))
            delta.append(abs(grid[list(p).index(max(p))] - tab[d, 0]))
        tag = "_x%d" % scale
        z["kl_bits" + tag], z["hellinger" + tag], z["mode_delta" + tag] = np.array(kl), np.array(hel), np.array(delta)
    return z


def main():
    out_dir = os.path.join(HERE, "kde")
    os.makedirs(out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(out_dir, "sklearn_kde.npz"), **sklearn_kde())
    np.savez_compressed(os.path.join(out_dir, "scipy_hdp_vs_gaussian.npz"), **scipy_hdp_vs_gaussian())


if __name__ == "__main__":
    main()
