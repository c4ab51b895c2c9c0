"""Gaussian mixtures over a k-mer table's rows on the GPU (sa_kmer_table_mixture) against the numpy restatement
(tests/kmer_mixture_ref.py): parity at the sizes where the kernel changes path, iteration counts, bit-for-bit determinism
however a table was filled, properties of the fit, the error contract, and the reference's own assignments file.

The parity bar is measured in the test: d = max(1e-13, worst difference between the restatement on a k-mer's rows in table
order and on the same rows reversed), the noise floor of the summation order; the GPU has to be within 100 d (the factor is
for the device's exp / log, a few ulp each).  Differences are taken relative to max(1, |value|)."""
import gzip
import os

import numpy as np
import pytest

import signalalign_amd as sa

import kmer_mixture_ref as ref
import sa_cases as cases

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(cases.GOLDEN, "hdp", "d6160b0b-a35e-43b5-947f-adaa1abade28.sm.assignments.tsv.gz")
LDS_ROWS = 2048   # KT_MIX_LDS_ROWS (sa_train.hip): a longer segment is sorted in HBM and streamed
BIG = 1 << 20     # max_per_kmer: nothing is dropped
SETTINGS = ((25, 0.0), (100, 1e-3))   # (max_iter, tol): a fixed number of iterations, and sklearn's defaults


def sizes(K):
    return [K, K + 1, 63, 64, 65, 255, 256, 257, LDS_ROWS + 1, 5000]


def fill(tab, per_kmer, seed, calls=1):
    """per_kmer: {kmer id: values}.  The rows of all k-mers go in shuffled together, so that segments fill in arrival order."""
    rng = np.random.RandomState(seed)
    km = np.concatenate([np.full(len(v), k, dtype=np.int32) for k, v in per_kmer.items()])
    x = np.concatenate([np.asarray(v, dtype=np.float64) for v in per_kmer.values()])
    prob = np.round(rng.uniform(0.5, 1.0, len(x)), 6)
    order = rng.permutation(len(x))
    km, x, prob = km[order], x[order], prob[order]
    edges = np.linspace(0, len(x), calls + 1).astype(int)
    for a, b in zip(edges[:-1], edges[1:]):
        tab.add_rows(km[a:b], x[a:b], prob[a:b])


def rows_by_kmer(tab):
    rows = tab.rows(0)
    return {int(k): rows["descaled_units"][rows["kmer_id"] == k].astype(np.float64) / 1e6 for k in np.unique(rows["kmer_id"])}


def diff(got, exp):
    """worst difference of a fit (a MIXTURE_FIT_DTYPE entry or a restatement dict) from a restatement dict"""
    K = len(exp["weight"])
    worst = abs(float(got["lower_bound"]) - exp["lower_bound"]) / max(1.0, abs(exp["lower_bound"]))
    for f in ("weight", "mean", "sd"):
        g = np.asarray(got[f], dtype=np.float64)[:K]
        worst = max(worst, float((np.abs(g - exp[f]) / np.maximum(1.0, np.abs(exp[f]))).max()))
    return worst


@pytest.fixture(scope="module")
def model():
    return sa.Model.load(cases.MODEL_6MER)


@pytest.fixture(scope="module")
def parity(model):
    """one table with every parity shape on a k-mer of its own, and the restatement's fits of them (computed once)"""
    per_kmer, shape = {}, {}
    kid = 10
    for K in (1, 2, 3, 4):
        for n in sizes(K):
            per_kmer[kid] = ref.planted(1000 * K + n, n, ref.TWO if (n + K) % 2 else ref.THREE)
            shape[kid] = (K, "n%d" % n)
            kid += 7
        per_kmer[kid] = np.full(50, 81.25)          # hi == lo
        shape[kid] = (K, "equal")
        kid += 7
        if K > 1:
            per_kmer[kid] = ref.planted(77 + K, K - 1, ref.TWO)   # fewer rows than components
        shape[kid] = (K, "short")                   # (K = 1: a k-mer without rows)
        kid += 7
    tab = sa.KmerTable(model, BIG, 0.0)
    fill(tab, per_kmer, 5, calls=3)
    x = rows_by_kmer(tab)
    exp, rev, changes = {}, {}, {}
    for kid, (K, name) in shape.items():
        xs = x.get(kid, np.zeros(0))
        assert sorted(xs.tolist()) == sorted(np.asarray(per_kmer.get(kid, [])).tolist())
        for max_iter, tol in SETTINGS:
            ch = []
            exp[kid, max_iter] = ref.fit(xs, K, max_iter=max_iter, tol=tol, changes=ch)
            rev[kid, max_iter] = ref.fit(xs[::-1], K, max_iter=max_iter, tol=tol)
            changes[kid, max_iter] = ch
    yield tab, shape, exp, rev, changes
    tab.close()


def test_parity_with_the_restatement(parity):
    tab, shape, exp, rev, changes = parity
    d = 1e-13
    for key, e in exp.items():
        if e["status"] == 0:
            d = max(d, diff(rev[key], e))
            assert (rev[key]["n_iter"], rev[key]["converged"]) == (e["n_iter"], e["converged"]), key
    worst, fitted = 0.0, 0
    for K in (1, 2, 3, 4):
        ids = [kid for kid, (k, _) in shape.items() if k == K]
        for max_iter, tol in SETTINGS:
            got = tab.mixture(ids, n_components=K, max_iter=max_iter, tol=tol)
            for g, kid in zip(got, ids):
                e = exp[kid, max_iter]
                assert (int(g["kmer_id"]), int(g["n"]), int(g["status"])) == (kid, e["n"], e["status"]), (K, shape[kid])
                if e["status"]:
                    assert int(g["n_iter"]) == 0 and int(g["converged"]) == 0 and g["lower_bound"] == 0
                    assert not g["weight"].any() and not g["mean"].any() and not g["sd"].any()
                    continue
                fitted += 1
                w = diff(g, e)
                worst = max(worst, w)
                assert w <= 100 * d, (K, shape[kid], max_iter, w, d)
                assert not g["weight"][K:].any() and not g["mean"][K:].any() and not g["sd"][K:].any()
                assert abs(g["weight"][:K].sum() - 1.0) <= 1e-12
                if tol == 0:
                    assert (int(g["n_iter"]), int(g["converged"])) == (max_iter, 0)
    print("parity: d = %.3g (restatement, table order against reversed), GPU worst difference = %.3g over %d fits" % (d, worst, fitted))
    assert fitted == 2 * 4 * 11


def test_iteration_counts_equal_the_restatement(parity):
    tab, shape, exp, rev, changes = parity
    max_iter, tol = SETTINGS[1]
    # no case of these seeds comes near the threshold, so none is left out of the comparison
    for (kid, mi), ch in changes.items():
        if mi == max_iter:
            assert not any(abs(c - tol) <= 1e-6 * tol for c in ch), shape[kid]
    stopped_early = 0
    for K in (1, 2, 3, 4):
        ids = [kid for kid, (k, _) in shape.items() if k == K and exp[kid, max_iter]["status"] == 0]
        got = tab.mixture(ids, n_components=K)
        for g, kid in zip(got, ids):
            e = exp[kid, max_iter]
            assert (int(g["n_iter"]), int(g["converged"])) == (e["n_iter"], e["converged"]), (K, shape[kid])
            stopped_early += e["converged"] and e["n_iter"] < max_iter
    assert stopped_early > 20


def test_filling_in_one_call_or_three_gives_the_same_bits(model):
    per_kmer = {3: ref.planted(1, 300, ref.TWO), 900: ref.planted(2, LDS_ROWS + 700, ref.THREE), 4000: ref.planted(3, 64, ref.TWO),
                4095: ref.planted(4, LDS_ROWS, ref.TWO)}
    res = []
    for calls in (1, 3):
        tab = sa.KmerTable(model, BIG, 0.0)
        fill(tab, per_kmer, 9, calls=calls)
        res.append([tab.mixture(sorted(per_kmer), n_components=K).tobytes() for K in (1, 2, 3, 4)] +
                   [tab.mixture(None, n_components=2).tobytes()])
        again = [tab.mixture(sorted(per_kmer), n_components=K).tobytes() for K in (1, 2, 3, 4)]
        assert again == res[-1][:4]   # two calls on one table
        tab.close()
    assert res[0] == res[1]


def test_table_from_a_batch_and_from_its_file_give_the_same_bits(model, tmp_path):
    jobs = cases.synthetic_jobs(cases.MODEL_6MER, 2, 700, 4100)
    b = sa.Batch(model, sa.default_params(), jobs)
    b.run()
    one = sa.KmerTable(model, BIG, 0.1)
    one.add_batch(b, 0)
    b.close()
    path = str(tmp_path / "table.tsv")
    one.write(path, strand=0)
    raw = [ln.split() for ln in open(path) if ln.strip()]
    assert len(raw) > 500
    two = sa.KmerTable(model, BIG, 0.1)
    two.add_rows([model.kmer_id(r[0]) for r in raw], [float(r[2]) for r in raw], [float(r[3]) for r in raw])
    a, c = one.mixture(None, n_components=2), two.mixture(None, n_components=2)
    assert (a["status"] == 0).sum() > 100
    assert a.tobytes() == c.tobytes()
    one.close()
    two.close()


def test_one_component_is_the_tables_mean_and_sd(parity):
    tab, shape, exp, rev, changes = parity
    ids = [kid for kid, (k, name) in shape.items() if k == 1 and name != "short"]
    st = tab.stats(0)
    got = tab.mixture(ids, n_components=1)
    d = max([1e-13] + [diff(rev[kid, 100], exp[kid, 100]) for kid in ids])
    for g, kid in zip(got, ids):
        m, s = st["m"][kid], st["s"][kid]
        assert abs(g["mean"][0] - m) <= 100 * d * max(1.0, abs(m)), shape[kid]
        assert abs(g["sd"][0] ** 2 - (s * s + 1e-6)) <= 100 * d * max(1.0, s * s), shape[kid]
        assert g["weight"][0] == 1.0 and int(g["converged"]) == 1


def test_lower_bound_never_falls(parity):
    tab, shape, exp, rev, changes = parity
    for K in (2, 3, 4):
        ids = [kid for kid, (k, name) in shape.items() if k == K and exp[kid, 25]["status"] == 0]
        lb = np.array([tab.mixture(ids, n_components=K, max_iter=m, tol=0.0)["lower_bound"] for m in range(1, 12)])
        assert np.all(lb[1:] >= lb[:-1] - 1e-12), K


def test_planted_pair_is_recovered(model):
    n = 5000
    x = ref.planted(424242, n, ref.TWO)
    tab = sa.KmerTable(model, BIG, 0.0)
    fill(tab, {1234: x}, 11)
    g = tab.mixture([1234], n_components=2)[0]
    tab.close()
    assert int(g["converged"]) == 1
    for c, (w, mu, sd) in enumerate(ref.TWO):   # (the start puts the lower component first)
        nc = n * w
        assert abs(g["weight"][c] - w) <= 5 * np.sqrt(w * (1 - w) / n)
        assert abs(g["mean"][c] - mu) <= 5 * sd / np.sqrt(nc)
        assert abs(g["sd"][c] - sd) <= 5 * sd / np.sqrt(2 * nc)


def test_the_default_start_handed_back_gives_the_same_bits(parity):
    tab, shape, exp, rev, changes = parity
    x = rows_by_kmer(tab)
    for K in (1, 2, 3, 4):
        ids = [kid for kid, (k, name) in shape.items() if k == K and exp[kid, 100]["status"] == 0]
        start = tab.mixture_start(ids, n_components=K)
        assert start.shape == (len(ids), 3, K)
        for s, kid in zip(start, ids):   # the start itself is the restatement's
            w, m, sd = ref.start(x[kid], K)
            assert max(np.abs(s[0] - w).max(), np.abs(s[1] - m).max(), np.abs(s[2] - sd).max()) <= 1e-11, (K, shape[kid])
        for max_iter, tol in SETTINGS:
            a = tab.mixture(ids, n_components=K, max_iter=max_iter, tol=tol)
            b = tab.mixture(ids, n_components=K, max_iter=max_iter, tol=tol, init=start)
            assert a.tobytes() == b.tobytes(), K


def test_error_contract(parity):
    tab, shape, exp, rev, changes = parity
    ids = [kid for kid, (k, name) in shape.items() if k == 2 and name == "n64"]

    def refused(**kw):
        args = dict(kmer_ids=ids, n_components=2)
        args.update(kw)
        with pytest.raises(sa.SaError) as ei:
            tab.mixture(**args)
        return ei.value.code == -1

    assert refused(n_components=0)
    assert refused(n_components=5)
    assert refused(max_iter=0)
    assert refused(tol=-1e-9)
    assert refused(tol=float("inf"))
    assert refused(tol=float("nan"))
    assert refused(reg_covar=-1e-9)
    assert refused(kmer_ids=[4096])
    assert refused(kmer_ids=[-1])
    good = np.array([[[0.5, 0.5], [78.0, 84.0], [1.0, 1.0]]])
    assert tab.mixture(ids, init=good)[0]["status"] == 0
    for f, c, v in ((0, 0, 0.0), (0, 1, float("nan")), (2, 0, 0.0), (2, 1, -1.0), (2, 0, float("inf")), (0, 0, float("inf")),
                    (1, 0, float("nan"))):
        bad = good.copy()
        bad[0, f, c] = v
        assert refused(init=bad), (f, c, v)


def test_reference_assignments(model):
    with gzip.open(FIXTURE, "rt") as f:
        raw = [ln.split() for ln in f if ln.strip()]
    tab = sa.KmerTable(model, BIG, 0.0)
    tab.add_rows([model.kmer_id(r[0]) for r in raw], [float(r[2]) for r in raw], [float(r[3]) for r in raw])
    x = rows_by_kmer(tab)
    ids = sorted(k for k, v in x.items() if len(v) >= 8)
    assert len(ids) > 100
    got = tab.mixture(ids, n_components=2)
    tab.close()
    exp = [ref.fit(x[k], 2) for k in ids]
    d = max([1e-13] + [diff(ref.fit(x[k][::-1], 2), e) for k, e in zip(ids, exp)])
    worst = 0.0
    for g, e, k in zip(got, exp, ids):
        assert (int(g["n"]), int(g["status"])) == (e["n"], 0)
        worst = max(worst, diff(g, e))
        assert diff(g, e) <= 100 * d, (k, diff(g, e), d)
    print("reference assignments: %d k-mers, d = %.3g, GPU worst difference = %.3g" % (len(ids), d, worst))
