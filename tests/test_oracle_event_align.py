"""The CPU restatement of the event <-> k-mer pre-alignment (sao_event_align_ex, oracle/sa_oracle.c) against a plain
full-matrix Viterbi (tests/event_align_ref.py) on the shapes of tests/ea_cases.py.  The two share the recurrence as
impl/eventAligner.c states it and nothing else: the plain reference has no band, no band origin and no offset, so a
misreading of the banding (an origin off by one, a neighbour offset, the band's limits, the trace row addressed by the
walk) shows as a difference.  Where the band covered the whole matrix (fills == n_events * n_kmers) equality is forced.
Runs without a GPU.
"""
import numpy as np

import sa_cases
import ea_cases
import event_align_ref


def _all():
    for which, cs in (("6mer", ea_cases.cases_6mer()), ("rna", ea_cases.cases_rna())):
        for case, exp in zip(cs, ea_cases.expected(which)):
            yield which, case, exp


def _sizes(which, case):
    k = 5 if which == "rna" else 6
    return len(case[2]), len(case[1]) - (k - 1)


def _by_label():
    return {case[0]: exp for _, case, exp in _all()}


def test_the_walk_stays_inside_the_band_on_every_listed_case():
    """A condition on the inputs: with a flag set the reference itself reads memory it did not write, and there is
    nothing to compare.  Such an input does not belong in the list (and must not be sent to a GPU)."""
    assert len(ea_cases.cases_6mer()) + len(ea_cases.cases_rna()) <= 150
    bad = [(case[0], exp[4]) for _, case, exp in _all() if exp[4] != 0]
    assert not bad, bad


def test_oracle_equals_the_plain_viterbi():
    checked, above = 0, []
    for which, case, (ek, ee, st, fills, walk) in _all():
        label, seq, ev, scale, shift, var = case
        n_events, n_kmers = _sizes(which, case)
        if n_events * n_kmers > ea_cases.MAX_REF_CELLS:
            above.append(label)
            continue
        om, tab = ea_cases.oracle_model(sa_cases.MODEL_5MER if which == "rna" else sa_cases.MODEL_6MER)
        ids = ea_cases.oracle.kmer_ids_of(om, seq, rna=which == "rna")
        assert len(ids) == n_kmers
        pairs, ref_st = event_align_ref.event_align(tab, ids, ev, scale, shift, var)
        assert st == ref_st, (label, st, ref_st)
        if st == 0:
            assert np.array_equal(pairs[:, 0], ek) and np.array_equal(pairs[:, 1], ee), label
        else:
            assert len(ek) == 0 and len(ee) == 0, label
        checked += 1
    # only the four long mismatched reads are too large for the full matrix
    assert sorted(above) == ["half_noise_500x312", "long_2983x195", "noise_800x479", "short_300x1824"], above
    assert checked >= 90


def test_fills_is_the_whole_matrix_when_it_fits_the_band():
    small = 0
    for which, case, (ek, ee, st, fills, walk) in _all():
        n_events, n_kmers = _sizes(which, case)
        assert 0 < fills <= n_events * n_kmers, case[0]
        if n_events <= 45 and n_kmers <= 45:
            assert fills == n_events * n_kmers, (case[0], fills)
            small += 1
    assert small >= 25


def test_status_words_reached_and_thresholds():
    st = {label: exp[2] for label, exp in _by_label().items()}
    assert {0, 1, 5, 8, 9} <= set(st.values()), sorted(set(st.values()))
    # more than 50 k-mers skipped in a row: 1 event against n k-mers skips n - 1
    assert st["one_event_2k"] == 1 and st["one_event_51k"] == 1
    assert st["one_event_52k"] == 5 and st["one_event_53k"] == 5 and st["one_event_295k"] == 5
    # more than 5 events per k-mer: clear at exactly 5.0
    assert st["per_kmer_5x1"] == 0 and st["per_kmer_6x1"] == 8 and st["per_kmer_400x1"] == 8
    assert st["per_kmer_10x2"] == 0 and st["per_kmer_11x2"] == 8
    assert st["per_kmer_35x7"] == 0 and st["per_kmer_36x7"] == 8
    # the reads that do not fit their sequence
    assert st["noise_800x479"] == 1 and st["short_300x1824"] == 5
    assert st["long_2983x195"] == 8 and st["long_600x55"] == 8
    assert {st[l] for l in st if l.startswith("half_noise_")} <= {1, 8, 9}
    assert st["half_noise_300x187"] == 1 and st["half_noise_300x50"] == 9
    # every matched read is accepted, with every k-mer and a monotone path
    for label, (ek, ee, s, fills, walk) in _by_label().items():
        if label.startswith(("matched_", "events_", "rna_")):
            assert s == 0 and len(ek) > 0 and ek[0] == 0, label
            dk, de = np.diff(ek), np.diff(ee)
            assert ((dk == 0) | (dk == 1)).all() and ((de == 0) | (de == 1)).all() and ((dk + de) >= 1).all(), label


def test_event_align_is_event_align_ex(oracle):
    for which, case, (ek, ee, st, fills, walk) in list(_all())[::7]:
        label, seq, ev, scale, shift, var = case
        om, _ = ea_cases.oracle_model(sa_cases.MODEL_5MER if which == "rna" else sa_cases.MODEL_6MER)
        om.set_read_params(scale, shift, var)
        k, e, s = oracle.event_align(om, ev, oracle.kmer_ids_of(om, seq, rna=which == "rna"))
        assert s == st and np.array_equal(k, ek) and np.array_equal(e, ee), label
