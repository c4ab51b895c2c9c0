"""The planted k-mer table cases (tests/kmer_table_cases.py) prove their own names on the CPU: the array form of the top-N
restatement equals the tuple form, every selection case settles at the radix level, owner lane and bin offset it is named
for when the table's merges are replayed with settle_shift, the carry cases do carry, and every statistics value prints the
units it was planted as."""
import numpy as np
import pytest

import kmer_table_cases as kc
import kmer_training_ref as ref

TUPLE_FORM_ROWS = 12000   # tables up to this many rows also go through the tuple form as a whole


def tuple_rows(km, pu):
    """top_n's rows with the position in the run as a fifth field"""
    return [("t", int(k), "0.000000", ref.f6(p / 1e6), i) for i, (k, p) in enumerate(zip(km.tolist(), pu.tolist()))]


def same_selection(km, pu, n, min_prob, first=0):
    got = ref.top_n_arrays(km, pu, n, ref.min_units(min_prob), first_ordinal=first)
    exp = ref.top_n(tuple_rows(km, pu), n, min_prob)
    assert sorted(got) == sorted(k for _, k in exp)
    for (_, k), rows in exp.items():
        assert got[k].tolist() == [first + r[4] for r in rows], k
    return len(exp)


@pytest.mark.parametrize("name", sorted(kc.SELECTION))
def test_array_form_equals_tuple_form_on_the_cases(name):
    t = kc.selection_table(name)
    for s in t.strands():
        lo, hi = t.span(s)
        if hi - lo <= TUPLE_FORM_ROWS:
            assert same_selection(t.km[lo:hi], t.pu[lo:hi], t.n, t.min_prob, first=lo) > 0
        else:   # the rows that pass the filter, k-mer by k-mer (the rest are the padding rows of posterior 0)
            assert t.min_units > 0
            got = t.kept(s)
            keep = lo + np.nonzero(t.pu[lo:hi] >= t.min_units)[0]
            assert 0 < len(keep) <= TUPLE_FORM_ROWS
            exp = ref.top_n([("t", int(t.km[o]), "0.000000", ref.f6(t.pu[o] / 1e6), int(o)) for o in keep], t.n, t.min_prob)
            assert sorted(got) == sorted(k for _, k in exp)
            for (_, k), rows in exp.items():
                assert got[k].tolist() == [r[4] for r in rows]


def test_array_form_equals_tuple_form_on_random_tables():
    rng = np.random.RandomState(5)
    for i in range(20):
        n_rows, n_kmers, n = int(rng.randint(1, 3000)), int(rng.randint(1, 60)), int(rng.randint(1, 12))
        grid = rng.randint(0, 1000001, int(rng.randint(1, 50)))   # few distinct posteriors: many ties
        km, pu = rng.randint(0, n_kmers, n_rows), rng.choice(grid, n_rows)
        min_prob = float(rng.choice([0.0, 0.25, 0.5, 0.999999, 1.0]))
        same_selection(km, pu, n, min_prob, first=int(rng.randint(0, 1 << 30)))
    assert ref.top_n_arrays([], [], 3, 0) == {}


def test_settle_shift_on_keys_written_out():
    key = ref.key
    assert ref.settle_shift([key(5, 0), key(7, 1)], 2) == (None, None, None)
    assert ref.settle_shift([key(1000000, 0), key(3, 1)], 1) == (50, 61, 976)
    assert ref.settle_shift([key(2048 + 5, 0), key(2048 + 4, 1), key(2048 + 3, 2)], 2) == (40, 0, 4)
    assert ref.settle_shift([key(9, 0), key(9, 1), key(9, 2)], 1) == (0, 63, 1023)
    assert ref.settle_shift([key(9, 1023), key(9, 1024), key(9, 1025)], 1) == (10, 63, 1023)
    assert ref.settle_shift([key(9, (1 << 30) - 1), key(9, 1 << 30), key(9, (1 << 30) + 1)], 1) == (30, 63, 1023)


def all_traces():
    out = []
    for name in sorted(kc.SELECTION):
        t = kc.selection_table(name)
        for case, c in t.cases.items():
            out.append((t, case, c, t.merge_trace(case)))
    return out


def test_every_selection_case_settles_where_its_name_says():
    shifts, at50 = set(), set()
    for t, case, c, trace in all_traces():
        assert len(trace) == sum(1 for q in t.calls if q[0] == c["strand"])
        shifts |= {q[0] for q in trace}
        assert all(q[0] != 30 for q in trace), (t.name, case)          # needs run ordinals of 2^30 and more
        if c["shift"] is None:
            continue
        assert 30 not in c["shift"]
        hits = [q for q in trace if q[0] in c["shift"]]
        assert hits, (t.name, case, trace)
        if c["lane"] is not None:
            assert [(q[1], q[2] % 16) for q in hits] == [(c["lane"], c["offset"])], (t.name, case, trace)
            at50.add((c["lane"], c["offset"]))
    assert shifts == {None, 50, 40, 20, 10, 0}
    assert {0, 61} <= {lane for lane, _ in at50} and {0, 15} <= {off for _, off in at50}


def test_the_named_cases_are_what_they_say():
    for name, base in (("n7", 1024), ("far", kc.BIG)):
        t = kc.selection_table(name)
        for mult, need in ((1, 2), (2, 4), (3, 6)):
            c = t.cases["tie_%d_need%d" % (base, need)]
            tied = np.nonzero((t.km == c["kmer"]) & (t.pu == 700000))[0]
            assert tied.tolist() == list(range(mult * base - 4, mult * base + 7))
            kept = t.kept(0)[c["kmer"]].tolist()
            assert kept[t.n - need:] == tied[:need].tolist() and (t.pu[kept[:t.n - need]] > 700000).all()
    far = kc.selection_table("far")
    assert far.min_units == 500000 and (far.km == kc.N_KMERS - 1).sum() > 3 * kc.BIG - 200 and kc.N_KMERS - 1 not in far.kept(0)
    for name in ("n2", "n7", "n1025"):   # posterior 0: some of the rows printed 0.000000 are kept, the first in run order
        t = kc.selection_table(name)
        c = t.cases["posterior_zero"]
        zeros = np.nonzero((t.km == c["kmer"]) & (t.pu == 0))[0]
        kept = t.kept(0)[c["kmer"]]
        assert 0 < c["n_zero_kept"] < len(zeros) and kept[t.pu[kept] == 0].tolist() == zeros[:c["n_zero_kept"]].tolist()
    n2 = kc.selection_table("n2")   # 300 k-mers open after the posterior levels in one and the same merge
    opened = [[q[0] in (20, 10, 0) for q in n2.merge_trace(case)] for case in n2.cases if case.startswith("open_")]
    assert len(opened) == 300 and max(np.sum(opened, axis=0)) == 300
    a, b = n2.cases["shift50_lane0_offset15"], n2.cases["strand1_same_rows"]   # both strands: the same rows, other ordinals
    r0, r1 = n2.kept(0)[a["kmer"]], n2.kept(1)[b["kmer"]]
    assert a["kmer"] == b["kmer"] and n2.pu[r0].tolist() == n2.pu[r1].tolist() and n2.desc[r0].tolist() == n2.desc[r1].tolist()
    assert r0.max() < n2.span(1)[0] <= r1.min()
    c = n2.cases["strand1_other_rows"]
    assert n2.pu[n2.kept(0)[c["kmer"]]].tolist() != n2.pu[n2.kept(1)[c["kmer"]]].tolist()
    n7 = kc.selection_table("n7")   # old rows against new
    c = n7.cases["old_against_new"]
    mine = np.nonzero(n7.km == c["kmer"])[0]
    call = np.searchsorted([q[2] for q in n7.calls], mine, side="right")
    assert np.bincount(call).tolist() == [7, 4, 2]
    weakest = mine[(n7.pu[mine] == c["weakest"])]
    assert len(weakest) == 5 and call[n7.pu[mine] == c["weakest"]].tolist() == [0, 1, 1, 2, 2]
    for n_calls, new in ((1, 0), (2, 2), (3, 2)):
        kept = n7.kept(0, n_calls)[c["kmer"]]
        assert len(kept) == 7 and (kept >= n7.calls[1][1]).sum() == new
        assert new == 0 or kept[-1] == weakest[0]   # (the old row at the cutoff stays; no later tie displaces it)
    for name in ("n1", "n2", "n7", "n1025"):   # counts around N, distinct posteriors
        t = kc.selection_table(name)
        for cnt in (t.n - 1, t.n, t.n + 1):
            if cnt:
                c = t.cases["count_%d" % cnt]
                mine = t.pu[t.km == c["kmer"]]
                assert len(mine) == cnt == len(set(mine.tolist())) and len(t.kept(0)[c["kmer"]]) == min(cnt, t.n)


def test_sums_of_squares_carry():
    st = kc.statistics_table()
    for name in kc.CARRY_CASES + ("limit_mixed",):
        u = st.units(name)
        assert all(abs(x) == 1 << 31 for x in u[:-1]) and sum(x * x for x in u) >= 1 << 64, name   # the tree carries
    assert abs(sum(st.units("limit_mixed"))) == 3
    # a thread's own rows (t, t + 256, ... of the k-mer's segment, in whatever order they arrived: all have the same square)
    per_thread = [sum(x * x for x in st.units("limit_4097")[t::256]) for t in range(256)]
    assert max(per_thread) >= 1 << 64
    assert all(sum(x * x for x in st.units(name)[t::256]) < 1 << 64 for name in ("limit_5", "limit_257") for t in range(256))


def test_statistics_values_print_their_planted_units():
    st = kc.statistics_table()
    n_neg_zero = 0
    for name, (values, units, flags) in st.cases.items():
        assert len(values) == len(units) == len(flags) > 0
        for v, u, z in zip(values.tolist(), units.tolist(), flags.tolist()):
            assert ref.units(ref.f6(v)) == (u, z), (name, v)
            n_neg_zero += z
    assert n_neg_zero == 2
    assert ref.f6(kc.LIMIT) == "2147.483648" and kc.LIMIT < 2147.483648 and ref.units(ref.f6(-kc.LIMIT)) == (-(1 << 31), 0)
    assert sorted(len(c[0]) for name, c in st.cases.items() if name.startswith("count_")) == [1, 2, 3, 4, 255, 256, 257, 513, 5000]
    for name, (_, units, _) in st.cases.items():
        if name.startswith("count_") and len(units) > 1:
            assert sorted(units.tolist()) == sorted((-units).tolist()) and units.min() < 0 < units.max()
    x = sorted(st.units("two_values"))
    assert len(set(x)) == 2 and x[len(x) // 2 - 1] != x[len(x) // 2] and (x[len(x) // 2 - 1] + x[len(x) // 2]) % 2 == 1
    biased = [(u + (1 << 63)) for u in st.units("lowest_byte_only")]
    assert len({b >> 8 for b in biased}) == 1 and len({b & 255 for b in biased}) == len(biased) == 200
    assert len({abs(u) for u in st.units("sign_only")}) == 1 and len(set(st.units("sign_only"))) == 2
    assert len({(u + (1 << 63)) >> 56 for u in st.units("sign_only")}) == 2   # two occupied bins in the top pass
    x = sorted(st.units("mad_middle_differs"))
    med2 = x[1] + x[2]
    dev = sorted(abs(2 * v - med2) for v in x)
    assert len(x) == 4 and dev[1] != dev[2]
    # one k-mer per case, all rows kept
    t = st.table
    assert len(set(st.kmer.values())) == len(st.cases) and max(st.kmer.values()) < kc.N_KMERS
    assert sum(len(v) for v in t.kept(0).values()) == len(t.km) and len(t.calls) == 3
