"""The restatements of the site and position calls (tests/calls_ref.py) pinned without a device: a hand-worked table whose expected
units, sums and probabilities are literals derived from variantCaller.py:141-172 and alignmentAnalysisLib.py:217-233; the argument
checks of sa_site_calls_records / sa_position_calls_records, which answer before the device; and the proof that the planted
buckets of tests/test_gpu_calls_edges.py can tell a wrong row order."""
import ctypes as C

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import _capi

import calls_ref as ref
import sa_cases as cases

ALPHA, K = "ACEGT", 6
#      0123456789
REF = "ACGTAXGTAXGTAC"          # X at 5 and 9: the k-mers at x = 0 and x = 4 end in it (sites); positions 5 and 9
# (x, path k-mer, prob_e7) in row order
ROWS = [
    (0, "ACGTAC", 6000000),    # 1  site 0: C += 600000.       position 5: digit 5 - 0 = 5 is C, += 0.6
    (0, "ACGTAE", 2500005),    # 2  site 0: E += 250001 ("%f" of 0.2500005 rounds up).  position 5: E is no letter of ACGT: nothing, no row
    (0, "ACGTAT", 1000000),    # 3  site 0: T is no letter of CE: nothing.  position 5: T += 0.1
    (2, "GTAGGT", 1234567),    # 4  no site (ref[7] = T).  position 5: digit 5 - 2 = 3 is G (the last letter is T), += 0.123457
    (4, "ACGTAC", 4),          # 5  site 4: C += 0 (prints 0.000000).  position 5: digit 1 is C, += 0.0, a row; position 9: digit 5 is C, += 0.0
    (4, "AAGTAE", 9999995),    # 6  site 4: E += 1000000 (prints 1.000000).  position 5: digit 1 is A, += 1.0; position 9: E: nothing
    (5, "TGTACG", 2000000),    # 7  no site.  position 5: digit 0 is T, += 0.2 (0.1 + 0.2 = 0.30000000000000004); position 9: digit 4 is C, += 0.2
    (0, "ACGTAC", 3000000),    # 8  site 0: C += 300000.  position 5: C: (0.6 + 0.0) + 0.3 = 0.8999999999999999
    (3, "TAEGTA", 7000000),    # 9  no site.  position 5: digit 2 is E: nothing
    (8, "AACGTA", 1000000),    # 10 position 9: digit 1 is A, += 0.1
    (6, "ACGGTA", 3000000),    # 11 position 9: digit 3 is G, += 0.3
    (7, "ACTGTA", 15),         # 12 position 9: digit 2 is T, += 0.000002 ("%f" of 0.0000015 rounds up)
]


def test_printed_units_literals():
    assert ref.printed_units([0, 4, 5, 6, 15, 25, 35, 45, 1234567, 2500005, 9999995, 10000000]).tolist() == [
        0, 0, 0, 1, 2, 3, 3, 5, 123457, 250001, 1000000, 1000000]


def test_sites_of_the_hand_worked_table():
    got = ref.restate_sites(ref.records(ROWS, ALPHA), REF, K, ALPHA, {"X": "EC"})
    assert sorted(got) == [0, 4]
    letters, units, prob = got[0]
    assert letters == "CE" and units == [900000, 250001]          # sorted letters; 900000 / 1150001, 250001 / 1150001
    assert [float(p) for p in prob] == [0.7826080151234651, 0.21739198487653488]
    letters, units, prob = got[4]
    assert letters == "CE" and units == [0, 1000000] and [float(p) for p in prob] == [0.0, 1.0]
    # a site whose rows all print zero, or all carry a letter outside the kind, is no call
    none = ref.restate_sites(ref.records([(0, "ACGTAC", 4), (4, "ACGTAT", 9000000)], ALPHA), REF, K, ALPHA, {"X": "CE"})
    assert none == {}


def test_positions_of_the_hand_worked_table():
    got = ref.restate_positions(ref.records(ROWS, ALPHA), REF, K, ALPHA, {"X": "TGCA"})
    assert sorted(got) == [5, 9]
    letters, n, sums, probs = got[5]
    assert letters == "ACGT" and n == 7                            # rows 1, 3, 4, 5, 6, 7, 8
    assert sums == [1.0, 0.8999999999999999, 0.123457, 0.30000000000000004]
    # total = (((0 + 1.0) + 0.8999999999999999) + 0.123457) + 0.30000000000000004 = 2.3234570000000003 (right to left: 2.323457)
    assert probs == [0.43039315984758914, 0.38735384386283017, 0.05313504833530381, 0.12911794795427675]
    assert probs == [s / 2.3234570000000003 for s in sums] and probs != [s / 2.323457 for s in sums]
    letters, n, sums, probs = got[9]
    assert letters == "ACGT" and n == 5                            # rows 5, 7, 10, 11, 12
    assert sums == [0.1, 0.2, 0.3, 2e-06]
    assert probs == [0.16666611111296295, 0.3333322222259259, 0.4999983333388888, 3.333322222259259e-06]   # total 0.600002


def test_zero_total_position_is_reported_with_zero_probabilities():
    # the reference divides by zero here; the pinned rule is the site fold's for a zero sum
    got = ref.restate_positions(ref.records([(4, "ACGTAC", 4), (5, "TGTACG", 0), (3, "TAEGTA", 9000000)], ALPHA), REF, K, ALPHA,
                                {"X": "ACGT"})
    assert got == {5: ("ACGT", 2, [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]), 9: ("ACGT", 2, [0.0] * 4, [0.0] * 4)}


def test_the_chunk_edge_bucket_tells_its_halves_exchanged():
    """the 12-row bucket the GPU edge test feeds from records 4090 .. 4101: were the row ordinal to restart at the 4096-record
    chunk edge (i in place of C.local + i), the six rows of the second chunk would be folded before the six of the first"""
    ref5, alpha = "ACGTXACGTA", "ACGT"
    rows = [(4, "ACGT"[i % 4] + "ACGT", p) for i, p in enumerate(ref.bucket_prob_e7(12))]
    right, wrong = (ref.restate_positions(ref.records(r, alpha), ref5, 5, alpha, {"X": "ACGT"})[4] for r in (rows, rows[6:] + rows[:6]))
    assert right[1] == wrong[1] == 12
    assert np.asarray(right[2]).tobytes() != np.asarray(wrong[2]).tobytes()


@pytest.mark.parametrize("n", [16, 63, 64, 65, 300])
def test_planted_buckets_tell_a_wrong_row_order(n):
    """the buckets of the GPU edge test: n rows at one position, the letters in turn; folded in another order -- reversed, the two
    halves exchanged (a chunk edge crossed the wrong way), and at least one exchange of two successive rows of one letter -- the
    sums have other bits.  Most single exchanges round to the same double with these values: what they catch for certain is a
    bucket left unsorted or put in another order as a whole.  (One or two rows per letter commute: buckets of 1 and 2 rows
    have no order to get wrong.)"""
    ref5, alpha = "ACGTXACGTA", "ACGT"
    rows = [(4, "ACGT"[i % 4] + "ACGT", p) for i, p in enumerate(ref.bucket_prob_e7(n))]

    def sums(in_order):
        letters, n_rows, s, _ = ref.restate_positions(ref.records(in_order, alpha), ref5, 5, alpha, {"X": "ACGT"})[4]
        assert letters == "ACGT" and n_rows == n
        return np.asarray(s).tobytes()
    right = sums(rows)
    assert sums(rows[::-1]) != right
    assert sums(rows[n // 2:] + rows[:n // 2]) != right
    exchanged = [rows[:a] + [rows[a + 4]] + rows[a + 1:a + 4] + [rows[a]] + rows[a + 5:] for a in range(n - 4)]
    assert any(sums(e) != right for e in exchanged)


def _rc(pm, refs, first, x, kmer_id, prob_e7, amb={"X": "CE"}, position=False):
    refs = [r.encode() for r in refs]
    n = len(refs)
    jobs = (_capi.Job * max(n, 1))()
    for i, r in enumerate(refs):
        jobs[i].ref, jobs[i].ref_len = r, len(r)
    first = np.asarray(first, dtype=np.int64)
    arrs = [None if a is None else np.asarray(a, dtype=t) for a, t in ((x, np.int32), (kmer_id, np.int32), (prob_e7, np.int64))]
    ptr = [None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32 if a.dtype == np.int32 else C.c_int64)) for a in arrs]
    cnt = np.zeros(max(n, 1), dtype=np.int64)
    pcnt = cnt.ctypes.data_as(C.POINTER(C.c_int64))
    pfirst = first.ctypes.data_as(C.POINTER(C.c_int64))
    if position:
        out = (C.POINTER(_capi.PositionCall) * max(n, 1))()
        rc = sa.lib().sa_position_calls_records(pm._h, jobs, n, sa.default_ambig(amb), pfirst, ptr[0], ptr[1], ptr[2], 0, out, pcnt,
                                                None, None, None)
    else:
        out = (C.POINTER(_capi.SiteCall) * max(n, 1))()
        rc = sa.lib().sa_site_calls_records(pm._h, jobs, n, sa.default_ambig(amb), pfirst, ptr[0], ptr[1], ptr[2], 0, out, pcnt, None)
    if rc == 0:
        for i in range(n):
            sa.lib().sa_free(out[i])
    return rc, cnt[:n].tolist()


@pytest.mark.parametrize("position", [False, True])
def test_records_entries_check_their_arguments_before_the_device(position):
    pm = sa.Model.load(cases.MODEL_CPG)                       # ACEGT, k = 6: 15625 k-mers
    refs = [REF, "ACGTA", REF]                                 # the second holds no k-mer
    def rc(first, x, kid, p, refs=refs, amb={"X": "CE"}):
        return _rc(pm, refs, first, x, kid, p, amb=amb, position=position)[0]
    EINVAL, EUNSUPPORTED = -1, -8
    ok = ([0, 1, 1, 2], [0, 8], [0, 15624], [0, 10000000])
    assert rc([1, 1, 1, 2], *ok[1:]) == EINVAL                  # first[0] != 0
    assert rc([0, 2, 1, 2], *ok[1:]) == EINVAL                  # first not monotone
    assert rc(ok[0], [0, 9], *ok[2:]) == EINVAL                 # x beyond ref_len - k = 8
    assert rc(ok[0], [-1, 8], *ok[2:]) == EINVAL
    assert rc([0, 1, 2, 2], [0, 0], *ok[2:]) == EINVAL          # a record in the job without a k-mer
    assert rc(ok[0], ok[1], [0, 15625], ok[3]) == EINVAL        # kmer_id = n_alpha^k
    assert rc(ok[0], ok[1], [-1, 0], ok[3]) == EINVAL
    assert rc(ok[0], ok[1], ok[2], [0, 10000001]) == EINVAL     # prob_e7 above 10^7
    assert rc(ok[0], ok[1], ok[2], [-1, 0]) == EINVAL
    for missing in range(3):                                    # a NULL array with records
        args = [ok[1], ok[2], ok[3]]
        args[missing] = None
        assert rc(ok[0], *args) == EINVAL
    # more than eight options: as at creation, and before the records' device
    assert rc(*ok, amb={"X": "ABCDEFGHI"}) == EUNSUPPORTED


def test_site_records_without_a_site_need_no_device():
    pm = sa.Model.load(cases.MODEL_CPG)
    plain = REF.replace("X", "C")
    assert _rc(pm, [plain, plain], [0, 1, 2], [0, 8], [0, 15624], [5000000, 10000000]) == (0, [0, 0])
    assert _rc(pm, [], [0], None, None, None) == (0, [])
