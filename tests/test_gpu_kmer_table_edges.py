"""The k-mer table's top-N selection and statistics (sa_train.hip) on planted rows (tests/kmer_table_cases.py): every radix
level, owner lane and bin offset of k_kt_cut that run ordinals below 2^30 can reach, posterior 0, long ties, hundreds of k-mers
open at once, old rows against new, both strands; sums of squares that carry in a thread and in the tree, negative values,
medians and MADs in half and quarter units, negative zero; refusals raised on the device leave the table as it was.  Every
comparison is an equality with the restatement (tests/kmer_training_ref.py): integers, bytes, float64 bit patterns."""
import ctypes as C

import numpy as np
import pytest

import signalalign_amd as sa

import kmer_table_cases as kc
import kmer_training_ref as ref
import sa_cases as cases
from test_gpu_kmer_training import CE, batch_rows, check_rows_and_stats, check_table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    return sa.Model.load(cases.MODEL_6MER)


def fill(tab, t, calls=None, reverse=False):
    prob = t.prob()
    for s, lo, hi in (t.calls if calls is None else calls):
        sl = slice(lo, hi)
        km, desc, p = t.km[sl], t.desc[sl], prob[sl]
        if reverse:
            km, desc, p = km[::-1], desc[::-1], p[::-1]
        tab.add_rows(km, desc, p, strand=s)


def row_tuples(tab, strand=0):
    got = tab.rows(strand)
    return list(zip(got["kmer_id"].tolist(), got["prob_units"].tolist(), got["descaled_units"].tolist(), got["neg_zero"].tolist(),
                    got["run"].tolist()))


@pytest.mark.parametrize("name", sorted(kc.SELECTION))
def test_selection_table(model, name, tmp_path):
    t = kc.selection_table(name)
    tab = sa.KmerTable(model, t.n, t.min_prob)
    fill(tab, t)
    for s in (0, 1):
        if s in t.strands():
            exp = t.expected_rows(s)
            assert {c["kmer"] for c in t.cases.values() if c["strand"] == s and c["n_rows"]} >= {r[0] for r in exp}
            check_rows_and_stats(tab, exp, s)
        else:
            assert len(tab.rows(s)) == 0 and int(tab.stats(s)["n"].sum()) == 0
    tab.write(str(tmp_path / "table.tsv"))
    alpha, k = model.alphabet()
    assert (tmp_path / "table.tsv").read_text() == ref.table_lines(t.kept_texts(), alpha, k)
    tab.close()


@pytest.fixture(scope="module")
def statistics(model):
    st = kc.statistics_table()
    tab = sa.KmerTable(model, st.table.n, 0.0)
    fill(tab, st.table)
    yield st, tab
    tab.close()


def test_statistics_table(model, statistics, tmp_path):
    st, tab = statistics
    t = st.table
    check_rows_and_stats(tab, t.expected_rows(0))   # (the units parsed from the "%f" texts)
    for med in (False, True):
        got = tab.stats(0, med)
        n = np.zeros(kc.N_KMERS, dtype=np.int64)
        for name, km in st.kmer.items():
            nn, m, s = ref.stats(st.units(name), med)       # (the units as planted)
            n[km] = nn
            assert got["m"][km].tobytes() == np.float64(m).tobytes(), (name, med)
            assert got["s"][km].tobytes() == np.float64(s).tobytes(), (name, med)
        assert got["n"].tolist() == n.tolist()
    flags = {km: sorted(z for z in st.cases[name][2].tolist()) for name, km in st.kmer.items()}
    rows = tab.rows(0)
    for km, z in flags.items():
        assert sorted(rows["neg_zero"][rows["kmer_id"] == km].tolist()) == z
    tab.write(str(tmp_path / "table.tsv"))
    alpha, k = model.alphabet()
    text = (tmp_path / "table.tsv").read_text()
    assert text == ref.table_lines(t.kept_texts(), alpha, k)
    assert "\t-0.000000\t" in text and "\t-2147.483648\t" in text and "\t2147.483648\t" in text


def test_statistics_do_not_depend_on_the_fill(model, statistics):
    st, three = statistics
    t = st.table
    want = [three.stats(0, med).tobytes() for med in (False, True)]
    for calls, reverse in (([(0, 0, len(t.km))], False), (t.calls, True), ([(0, 0, len(t.km))], True)):
        tab = sa.KmerTable(model, t.n, 0.0)
        fill(tab, t, calls=calls, reverse=reverse)
        assert len(tab.rows(0)) == len(t.km)
        assert [tab.stats(0, med).tobytes() for med in (False, True)] == want, (len(calls), reverse)
        tab.close()


def test_checkpoint_and_rollback_between_planted_calls(model):
    """the table of the old-against-new case: call 1, checkpoint, calls 2 and 3, rollback, calls 2 and 3 again"""
    t = kc.selection_table("n7")
    assert "old_against_new" in t.cases
    tab = sa.KmerTable(model, t.n, t.min_prob)
    fill(tab, t, calls=t.calls[:1])
    assert row_tuples(tab) == t.expected_rows(0, n_calls=1)
    tab.checkpoint()
    fill(tab, t, calls=t.calls[1:])
    straight = tab.rows(0).tobytes()
    tab.rollback()
    assert row_tuples(tab) == t.expected_rows(0, n_calls=1)
    fill(tab, t, calls=t.calls[1:])
    assert row_tuples(tab) == t.expected_rows(0)       # ordinals included: run_next went back with the rows
    assert tab.rows(0).tobytes() == straight
    tab.close()


def test_refusals_leave_the_table_as_it_was():
    pm = sa.Model.load(cases.MODEL_CPG)
    _, k = pm.alphabet()
    p = sa.default_params()
    jobs = cases.synthetic_jobs(cases.MODEL_CPG, 2, 600, 500, cpg_ambiguous=True)
    b = sa.Batch(pm, p, jobs, ambig=sa.default_ambig(CE))
    b.run()
    rows = batch_rows(b, jobs, pm.table5(), pm, k)
    some = sorted({r[1] for r in rows if float(r[3]) >= 0.8})[:20]
    planted = [("t", km, "%f" % (60.0 + 0.25 * i), "%f" % (0.8 + 0.01 * i)) for i, km in enumerate(some)]
    n, min_prob = 10, 0.8

    def good_rows(tab):
        tab.add_rows([r[1] for r in planted], [float(r[2]) for r in planted], [float(r[3]) for r in planted])

    tab = sa.KmerTable(pm, n, min_prob)
    good_rows(tab)
    before = tab.rows(0).tobytes()
    assert len(tab.rows(0)) == len(planted)
    L = sa.lib()

    def refused(change):
        arr = type(b._arr)()
        C.memmove(arr, b._arr, C.sizeof(arr))
        change(arr[1])
        rc = L.sa_kmer_table_add_batch(tab._h, b._h, arr, b.n_jobs, 0, None)
        assert tab.rows(0).tobytes() == before and len(tab.rows(1)) == 0
        return rc

    def far_shift(job):
        job.shift = 1e10

    def one_event(job):
        job.n_events = 1

    assert refused(far_shift) == -8    # SA_EUNSUPPORTED: a descaled mean the table does not hold (KT_ERR_RANGE)
    assert refused(one_event) == -1    # SA_EINVAL: a record's event beyond the job's events (KT_ERR_BOUNDS)
    for bad in (2147.483648, -2147.483648, 4294.967296, -1e9):
        with pytest.raises(sa.SaError) as ei:
            tab.add_rows([some[0], some[1]], [70.0, bad], [0.9, 0.9])
        assert ei.value.code == -8 and tab.rows(0).tobytes() == before, bad
    # run_next did not move: the batch's rows get the ordinals they get on a table that saw the good rows only
    tab.add_batch(b, 0)
    fresh = sa.KmerTable(pm, n, min_prob)
    good_rows(fresh)
    fresh.add_batch(b, 0)
    assert tab.rows(0).tobytes() == fresh.rows(0).tobytes()
    exp, _ = check_table(tab, planted + rows, n, min_prob)
    assert max(r[4] for r in exp) >= len(planted)
    fresh.close()
    tab.close()
    b.close()
