"""Gaussian kernel density estimates over a k-mer table's rows on the GPU (sa_kmer_table_kde) against the numpy restatement
(tests/kde_ref.py) and against scikit-learn's own numbers (tests/golden/kde/sklearn_kde.npz): parity at the row counts and
point counts where the kernel changes path, three bandwidths, duplicated rows, points far from every row, an empty k-mer,
bit-for-bit independence of the other jobs and points of a call, of the chunking and of how the table was filled, and the
error contract.

The parity bar is measured in the test: d = max(1e-13, worst difference between the restatement with the rows added in
ascending and in descending order), the noise floor of the summation order; the GPU has to be within 100 d (the factor is
for the device's exp / log, a few ulp each).  Differences are taken relative to max(1, |value|)."""
import gzip
import os

import numpy as np
import pytest

import signalalign_amd as sa

import kde_ref as ref
import sa_cases as cases

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(cases.GOLDEN, "hdp", "d6160b0b-a35e-43b5-947f-adaa1abade28.sm.assignments.tsv.gz")
SKLEARN = os.path.join(cases.GOLDEN, "kde", "sklearn_kde.npz")
LDS_ROWS = 2048   # KT_KDE_LDS_ROWS (sa_train.hip): a longer segment goes through LDS in several chunks
TILE = 512        # KT_KDE_TILE: query points per work-group
BIG = 1 << 20     # max_per_kmer: nothing is dropped
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, LDS_ROWS + 1, 5000)
N_X = (1, 63, 64, 65, 600)
BANDWIDTHS = (0.05, 0.5, 5.0)
GRID = np.linspace(30.0, 90.0, 600)


def rel(got, exp):
    return float((np.abs(got - exp) / np.maximum(1.0, np.abs(exp))).max())


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


def units_by_kmer(tab):
    rows = tab.rows(0)
    return {int(k): rows["descaled_units"][rows["kmer_id"] == k] for k in np.unique(rows["kmer_id"])}


def draw(seed, n):
    """n event means of a k-mer: two levels a few pA apart, as a modified and a canonical k-mer mixed give"""
    rng = np.random.RandomState(seed)
    return np.where(rng.uniform(size=n) < 0.6, rng.normal(72.0, 1.2, n), rng.normal(79.0, 2.5, n))


@pytest.fixture(scope="module")
def model():
    return sa.Model.load(cases.MODEL_6MER)


@pytest.fixture(scope="module")
def parity(model):
    """one table with every row count on a k-mer of its own, and the restatement of every (k-mer, bandwidth) on the whole grid
    in both orders (computed once)"""
    per_kmer, name = {}, {}
    kid = 11
    for n in SIZES:
        per_kmer[kid] = draw(100 + n, n)
        name[kid] = "n%d" % n
        kid += 13
    per_kmer[kid] = np.repeat(draw(7, 40), 5)   # every value five times
    name[kid] = "duplicates"
    kid += 13
    per_kmer[kid] = np.full(300, 81.25)         # one value only
    name[kid] = "equal"
    empty = kid + 13
    tab = sa.KmerTable(model, BIG, 0.0)
    fill(tab, per_kmer, 5, calls=3)
    units = units_by_kmer(tab)
    exp, rev = {}, {}
    for kid in name:
        assert sorted(units[kid].tolist()) == sorted(sa.f6_units(v)[0] for v in per_kmer[kid])
        for h in BANDWIDTHS:
            exp[kid, h] = ref.kde_log_density(units[kid], GRID, h)
            rev[kid, h] = ref.kde_log_density(units[kid], GRID, h, reverse=True)
    yield tab, name, units, exp, rev, empty
    tab.close()


def floor(exp, rev):
    return max([1e-13] + [rel(rev[key], exp[key]) for key in exp])


def test_parity_with_the_restatement(parity):
    tab, name, units, exp, rev, empty = parity
    d = floor(exp, rev)
    ids = sorted(name)
    worst = 0.0
    for h in BANDWIDTHS:
        for n_x in N_X:
            info = {}
            got = tab.kde(GRID[:n_x], ids, bandwidth=h, info=info)
            assert got.shape == (len(ids), n_x) and np.isfinite(got).all()
            assert list(info["n_rows"]) == [len(units[k]) for k in ids] and info["kernel_ms"] > 0
            for g, kid in zip(got, ids):
                w = rel(g, exp[kid, h][:n_x])
                worst = max(worst, w)
                assert w <= 100 * d, (name[kid], h, n_x, w, d)
    print("KDE parity: d = %.3g (restatement, ascending against descending), GPU worst difference = %.3g over %d x %d x %d "
          "(k-mers, bandwidths, point counts)" % (d, worst, len(ids), len(BANDWIDTHS), len(N_X)))


def test_points_far_from_every_row_and_an_empty_kmer(parity):
    tab, name, units, exp, rev, empty = parity
    ids = sorted(name)
    far = np.array([-130.0, 300.0, 1e4])   # 200 pA and more from every row
    for h in BANDWIDTHS:
        info = {}
        got = tab.kde(far, ids + [empty], bandwidth=h, info=info)
        assert np.isfinite(got[:-1]).all() and (got[:-1] < -0.5 * (190.0 / h) ** 2).all()
        assert np.all(np.isneginf(got[-1])) and info["n_rows"][-1] == 0
        d = 1e-13
        for g, kid in zip(got, ids):
            e = ref.kde_log_density(units[kid], far, h)
            d = max(d, rel(ref.kde_log_density(units[kid], far, h, reverse=True), e))
            assert rel(g, e) <= 100 * d, (name[kid], h)
    # one row: the kernel itself, whatever the other rows of the table
    one = [k for k in ids if name[k] == "n1"]
    x0 = float(units[one[0]][0]) / 1e6
    g = tab.kde([x0, x0 + 0.5], one, bandwidth=0.5)[0]
    assert abs(g[0] + (np.log(0.5) + ref.HALF_LOG_2PI)) <= 1e-14 and abs(g[1] - (g[0] - 0.5)) <= 1e-13


def test_sklearn_fixture_on_the_bundled_assignments(model):
    z = np.load(SKLEARN)
    with gzip.open(FIXTURE, "rt") as f:
        raw = [ln.split() for ln in f if ln.strip()]
    tab = sa.KmerTable(model, BIG, 0.0)
    tab.add_rows([model.kmer_id(r[0]) for r in raw], [float(r[2]) for r in raw], [float(r[3]) for r in raw])
    ids = [model.kmer_id(str(k)) for k in z["kmers"]]
    info = {}
    got = tab.kde(z["x"], ids, bandwidth=float(z["bandwidth"][0]), info=info)
    units = units_by_kmer(tab)
    tab.close()
    assert np.array_equal(info["n_rows"], z["n_rows"])
    exp = [ref.kde_log_density(units[k], z["x"], 0.5) for k in ids]
    d = max([1e-13] + [rel(ref.kde_log_density(units[k], z["x"], 0.5, reverse=True), e) for k, e in zip(ids, exp)])
    worst = rel(got, z["log_density"])
    print("sklearn fixture: %d k-mers, d = %.3g, GPU against sklearn = %.3g, against the restatement = %.3g" %
          (len(ids), d, worst, rel(got, np.array(exp))))
    assert rel(got, np.array(exp)) <= 100 * d
    # sklearn is within 1e-13 of the restatement (tests/test_host_kde.py): within 100 d + 1e-13 of the GPU
    assert worst <= 100 * d + 1e-13


def test_a_value_depends_on_the_tables_contents_only(model, monkeypatch):
    per_kmer = {3: draw(1, 300), 900: draw(2, LDS_ROWS + 700), 4000: draw(3, 64), 4095: draw(4, LDS_ROWS)}
    kid, sub = 900, np.arange(37, 600, 7)
    res = []
    for calls in (1, 3):
        tab = sa.KmerTable(model, BIG, 0.0)
        fill(tab, per_kmer, 9, calls=calls)
        whole = tab.kde(GRID, None, bandwidth=0.5)                       # all k-mers x the whole grid
        assert whole.shape == (4096, 600) and np.isneginf(whole[5]).all()
        alone = tab.kde(GRID[sub], [kid], bandwidth=0.5)                  # that k-mer alone x a sub-grid
        assert alone.tobytes() == whole[kid, sub].tobytes()
        perm = np.random.RandomState(8).permutation(600)
        shuffled = tab.kde(GRID[perm], [4095, kid, 3, kid], bandwidth=0.5)   # a permuted x, repeated and unordered jobs
        assert shuffled[1].tobytes() == whole[kid, perm].tobytes() == shuffled[3].tobytes()
        assert shuffled[0].tobytes() == whole[4095, perm].tobytes()
        monkeypatch.setenv("SA_KDE_SLAB", "60000")                        # a hundred jobs per chunk of the output
        assert tab.kde(GRID, None, bandwidth=0.5).tobytes() == whole.tobytes()
        monkeypatch.delenv("SA_KDE_SLAB")
        monkeypatch.setenv("SA_KDE_NO_SKIP", "1")                         # every exp evaluated: the same bits
        assert tab.kde(GRID, sorted(per_kmer), bandwidth=0.5).tobytes() == whole[sorted(per_kmer)].tobytes()
        monkeypatch.delenv("SA_KDE_NO_SKIP")
        res.append(whole.tobytes())
        tab.close()
    assert res[0] == res[1]                                               # a table filled in one call or in three


def test_more_points_than_a_tile_and_both_strands(model):
    tab = sa.KmerTable(model, BIG, 0.0)
    a, b = draw(21, 130), draw(22, 70)
    tab.add_rows(np.full(len(a), 77, dtype=np.int32), a, np.full(len(a), 0.9), strand=0)
    tab.add_rows(np.full(len(b), 77, dtype=np.int32), b, np.full(len(b), 0.9), strand=1)
    x = np.random.RandomState(2).uniform(40.0, 100.0, 2 * TILE + 1)
    for strand, v in ((0, a), (1, b)):
        e = ref.kde_log_density([sa.f6_units(q)[0] for q in v], x, 0.5)
        d = max(1e-13, rel(ref.kde_log_density([sa.f6_units(q)[0] for q in v], x, 0.5, reverse=True), e))
        assert rel(tab.kde(x, [77], bandwidth=0.5, strand=strand)[0], e) <= 100 * d, strand
    tab.close()


def test_error_contract(parity):
    tab, name, units, exp, rev, empty = parity
    ids = [k for k in name if name[k] == "n64"]

    def refused(**kw):
        args = dict(x=GRID[:10], kmer_ids=ids, bandwidth=0.5)
        args.update(kw)
        with pytest.raises(sa.SaError) as ei:
            tab.kde(**args)
        return ei.value.code == -1

    assert refused(strand=2) and refused(strand=-1)
    assert refused(x=[])
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        assert refused(bandwidth=bad), bad
    assert refused(x=[50.0, float("nan")]) and refused(x=[float("inf")]) and refused(x=[-float("inf"), 50.0])
    assert refused(kmer_ids=[4096]) and refused(kmer_ids=[-1]) and refused(kmer_ids=[ids[0], 4096])
    L, C = sa.lib(), __import__("ctypes")
    x = np.ascontiguousarray(GRID[:10])
    out = np.full((1, 10), 7.0)
    xp, op = x.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double))
    i32 = np.array(ids, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert L.sa_kmer_table_kde(None, 0, i32, 1, xp, 10, 0.5, op, None, None) == -1
    assert L.sa_kmer_table_kde(tab._h, 0, i32, 1, None, 10, 0.5, op, None, None) == -1
    assert L.sa_kmer_table_kde(tab._h, 0, i32, 1, xp, 10, 0.5, None, None, None) == -1
    assert L.sa_kmer_table_kde(tab._h, 0, i32, -1, xp, 10, 0.5, op, None, None) == -1
    assert L.sa_kmer_table_kde(tab._h, 0, i32, 1, xp, 0, 0.5, op, None, None) == -1
    assert L.sa_kmer_table_kde(tab._h, 0, i32, 0, xp, 10, 0.5, op, None, None) == 0 and (out == 7.0).all()   # nothing written
    assert L.sa_kmer_table_kde(tab._h, 0, i32, 1, xp, 10, 0.5, op, None, None) == 0 and np.isfinite(out).all() and (out != 7.0).all()
    assert tab.kde(GRID[:10], []).shape == (0, 10)
