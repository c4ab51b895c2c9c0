"""The site fold and the position fold (sa_calls.hip) on planted records, through sa_site_calls_records and
sa_position_calls_records: the shapes a batch of aligned reads never produces -- more jobs than the scan has threads, jobs whose
sites fill 64-lane rounds exactly, sites at the edges of a bitmap word, records that straddle a word or end the reference,
buckets fed across a 4096-record chunk, letters outside a kind, kinds of different width, printed units at their edges, a
position whose rows all print zero.  Everything is compared exactly with the restatements of tests/calls_ref.py (pinned by
tests/test_host_calls_ref.py): integers with ==, doubles by their bytes."""
import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import synth

import calls_ref as ref
import sa_cases as cases

pytestmark = pytest.mark.gpu

CHUNK = 4096          # SA_CHAIN_CHUNK: records per block of the record kernels
# prob_e7 at the edges of sa_printed_units: 0-4 print 0.000000; a last digit of 5 is the tie rule; 10^7 prints 1.000000
EDGE_PROB = [0, 1, 4, 5, 6, 15, 25, 35, 45, 1000005, 2500005, 4999995, 9999995, 10000000, 10, 4999990, 1234567]


def model(path):
    alpha, k, _, _ = synth.parse_model_table(path)
    return sa.Model.load(path), "".join(sorted(alpha)), k


def make_ref(length, marks, phase=0):
    """ACGTACGT... of `length` with the letters of `marks` ({index: letter}) put in"""
    r = [("ACGT"[(i + phase) % 4]) for i in range(length)]
    for i, c in marks.items():
        r[i] = c
    return "".join(r)


def recs(x, kmer_id, prob_e7):
    out = np.zeros(len(x), dtype=ref.RECORD_DTYPE)
    out["x"], out["kmer_id"], out["prob_e7"] = x, kmer_id, prob_e7
    return out


NONE = recs([], [], [])


def random_records(rng, n, ref_len, k, n_kmers, xs=None):
    """n records over the job's k-mers (or over xs), any path k-mer, the posteriors from the edge values and from all of [0, 10^7]"""
    if ref_len < k or n == 0:
        return NONE
    x = rng.integers(0, ref_len - k + 1, n) if xs is None else rng.choice(np.asarray(xs), n)
    p = np.where(rng.random(n) < 0.5, rng.choice(np.asarray(EDGE_PROB), n), rng.integers(0, 10000001, n))
    return recs(x, rng.integers(0, n_kmers, n), p)


def flat(rows):
    first = np.zeros(len(rows) + 1, dtype=np.int64)
    first[1:] = np.cumsum([len(r) for r in rows])
    cat = np.concatenate(rows) if rows else NONE
    return first, cat


def site_calls(pm, refs, rows, amb):
    first, cat = flat(rows)
    return sa.site_calls_records(pm, refs, first, cat["x"], cat["kmer_id"], cat["prob_e7"], ambig=sa.default_ambig(amb))


def position_calls(pm, refs, rows, amb):
    first, cat = flat(rows)
    return sa.position_calls_records(pm, refs, first, cat["x"], cat["kmer_id"], cat["prob_e7"], ambig=sa.default_ambig(amb))


def same_bytes(a, b, fields):
    assert len(a) == len(b)
    for ca, cb in zip(a, b):
        for f in fields:
            assert np.asarray(ca[f]).tobytes() == np.asarray(cb[f]).tobytes(), f
        assert ca["letters"].tolist() == cb["letters"].tolist()


SITE_FIELDS = ("x", "units", "prob")
POS_FIELDS = ("p", "n_rows", "sum", "prob", "x_min", "x_max")


def check_sites(pm, alpha, k, refs, rows, amb):
    """the call, twice (the same bytes), against the restatement job by job; then the jobs in another order give each job the
    same calls (pre[] counts sites over the whole call, word_off per job: k_site_accum's slot)"""
    calls = site_calls(pm, refs, rows, amb)
    assert len(calls) == len(refs)
    exp = [ref.restate_sites(r, j, k, alpha, amb) for r, j in zip(rows, refs)]
    for c, e in zip(calls, exp):
        ref.check_site_calls(c, e)
    same_bytes(calls, site_calls(pm, refs, rows, amb), SITE_FIELDS)
    order = np.random.default_rng(5).permutation(len(refs)).tolist()
    moved = site_calls(pm, [refs[i] for i in order], [rows[i] for i in order], amb)
    same_bytes([calls[i] for i in order], moved, SITE_FIELDS)
    return calls, exp


def check_positions(pm, alpha, k, refs, rows, amb):
    calls = position_calls(pm, refs, rows, amb)
    assert len(calls) == len(refs)
    exp = [ref.restate_positions(r, j, k, alpha, amb) for r, j in zip(rows, refs)]
    for c, e, r in zip(calls, exp, rows):
        ref.check_position_calls(c, e, r)
    same_bytes(calls, position_calls(pm, refs, rows, amb), POS_FIELDS)
    order = np.random.default_rng(6).permutation(len(refs)).tolist()
    moved = position_calls(pm, [refs[i] for i in order], [rows[i] for i in order], amb)
    same_bytes([calls[i] for i in order], moved, POS_FIELDS)
    return calls, exp


# ---- sites ----------------------------------------------------------------------------------------------------------------
# X: the two-letter kind; Z: eight options (three of them no letters of the model: they can get nothing), so that the call's
# stride is 8 next to kinds of 2 -- k_site_final / k_site_compact walk nl letters of a site's `stride` entries, and a narrow
# site's letters must not be taken from its wide neighbour's.  (The columns past a site's letters are zero in the copy-out by
# construction -- a cleared struct filled per letter -- so the checks' look at them says nothing of the device's tail.)
SITE_AMB = {"X": "EC", "Z": "TNGOECPA"}


def site_job(rng, k, n_alpha, n_sites, lead=0):
    """a job with n_sites sites, two k-mer indices apart from `lead` on: every third gets no record, every fifth only records that
    print zero units, every seventh is of the wide kind; the others get a few records of every letter, letters outside the kind
    (k_site_accum's l < 0) among them.  Records at indices that are no site lie between them."""
    xs = [lead + 2 * i for i in range(n_sites)]
    marks = {x + k - 1: ("Z" if i % 7 == 6 else "X") for i, x in enumerate(xs)}
    length = max(k + lead + 2 * n_sites + 1, k + 2)
    x, kid, p = [], [], []
    for i, s in enumerate(xs):
        if i % 3 == 2:
            continue
        for r in range(1 + i % 4):
            x.append(s)
            any_kmer = int(rng.integers(0, n_alpha ** k))
            kid.append(any_kmer if r else any_kmer // n_alpha * n_alpha + 1)      # (the site's first record ends in C)
            p.append(int(rng.integers(0, 5)) if i % 5 == 4 else int(rng.choice(EDGE_PROB[3:])) if r % 2 else int(rng.integers(5, 10000001)))
        x.append(s + 1)                                     # no site: k_site_accum's bit test
        kid.append(int(rng.integers(0, n_alpha ** k)))
        p.append(9000000)
    o = rng.permutation(len(x))
    return make_ref(length, marks, lead), recs(np.asarray(x, dtype=np.int64)[o], np.asarray(kid, dtype=np.int64)[o], np.asarray(p, dtype=np.int64)[o])


def test_site_rounds_words_units_and_chunks():
    pm, alpha, k = model(cases.MODEL_CPG)
    n_alpha, nk = len(alpha), len(alpha) ** k
    rng = np.random.default_rng(11)
    refs, rows = [], []

    def add(r, rec):
        refs.append(r)
        rows.append(rec)
    # 0, 1, 63, 64, 65 and 129 sites: the 64-lane rounds of k_site_final (ballot count) and k_site_compact (prefix and carried w)
    for n in (0, 1, 63, 64, 65, 129):
        add(*site_job(rng, k, n_alpha, n, lead=n % 3))
    # sites at bits 0, 63 and 64 of the job's words, first and last site of a job that is not the call's first (pre[w] is the
    # call-wide index of the word's first site; k_site_accum: site = pre[w] + popcount below the bit).  130 k-mers, then 64:
    # the last k-mer at bit 63 of the job's last, full word
    for lx, at in ((130, (0, 63, 64, 127, 128, 129)), (64, (0, 63)), (65, (64,)), (128, (63, 64))):
        r = make_ref(lx + k - 1, {x + k - 1: "XZ"[i % 2] for i, x in enumerate(at)})
        add(r, random_records(rng, 40, len(r), k, nk, xs=list(at) + [1, 62, 65 % lx]))
    # printed units at their edges on one site, every value to each of the two letters and to a letter outside the kind
    r = make_ref(k + 3, {k + 1: "X"})
    ids = [ref.kmer_id("ACGTA" + c, alpha) for c in "CEA"]
    add(r, recs([2] * (3 * len(EDGE_PROB)), ids * len(EDGE_PROB), np.repeat(EDGE_PROB, 3)))
    # a site whose only unit comes from one record of prob_e7 6, beside one whose records all print zero
    r = make_ref(k + 3, {k - 1: "X", k + 1: "X"})
    add(r, recs([0, 0, 2, 2], [ids[0], ids[1], ids[0], ids[1]], [4, 5, 6, 0]))
    # no k-mer at all (ref_len < k, though it holds the letter), no record, no site
    add("ACX", NONE)
    add(make_ref(40, {10: "X", 30: "Z"}), NONE)
    add(make_ref(40, {}), random_records(rng, 30, 40, k, nk))
    # the chunk edge: 4095, 4096 and 4097 records of one job (k_site_accum: C.n of the last block 4095, 4096, 1)
    for n in (CHUNK - 1, CHUNK, CHUNK + 1):
        r = make_ref(90, {i: "XZ"[i % 2] for i in range(k - 1, 90, 9)})
        add(r, random_records(rng, n, 90, k, nk))
    # 4300 records of 10^7 on one site: 4.3e9 units pass 2^32 (the 64-bit atomic add, k_site_final's 64-bit total)
    r = make_ref(k + 3, {k + 1: "X"})
    add(r, recs([2] * 4300, [ids[0]] * 4300, [10000000] * 4300))
    calls, exp = check_sites(pm, alpha, k, refs, rows, SITE_AMB)
    assert [len(e) > 0 for e in exp[:6]] == [False, True, True, True, True, True]
    assert exp[-1][2][1] == [4300 * 1000000, 0] and 4300 * 1000000 > 2 ** 32
    assert exp[11][2] == ("CE", [1, 0], [1.0, 0.0]) and sorted(exp[11]) == [2]
    assert any(l == "ACEGNOPT" for c in calls for l in c["letters"]) and any(l == "CE" for c in calls for l in c["letters"])


@pytest.mark.parametrize("others", [False, True])
@pytest.mark.parametrize("n_jobs", [1, 1024, 1025, 2049])
def test_site_calls_of_many_one_site_jobs(n_jobs, others):
    """k_site_scan: one block of 1024 threads, one element per thread up to 1024 jobs, two from 1025 on, three from 2049 on.
    others: jobs without a k-mer and jobs without records stand among the one-site jobs (their count is 0); without them the
    call has exactly n_jobs jobs.  Every fourth one-site job's records print zero: kept and dropped sites alternate."""
    pm, alpha, k = model(cases.MODEL_CPG)
    rng = np.random.default_rng(100 + n_jobs)
    one = make_ref(k + 2, {k: "X"})                       # its site: x = 1
    ids = [ref.kmer_id("CGTAC" + c, alpha) for c in "CEG"]
    refs, rows = [], []
    for j in range(n_jobs):
        if others and j % 7 == 3:
            refs.append("ACXGT"[:2 + j % 4])
            rows.append(NONE)
        if others and j % 5 == 2:
            refs.append(one)
            rows.append(NONE)
        refs.append(one)
        n = 1 + j % 3
        p = rng.integers(0, 5, n) if j % 4 == 1 else rng.integers(5, 10000001, n)
        rows.append(recs([1] * n, rng.choice(ids, n), p))
    calls, exp = check_sites(pm, alpha, k, refs, rows, {"X": "CE"})
    assert len(refs) == n_jobs or others
    if n_jobs > 1:
        assert 0 < sum(len(e) for e in exp) < n_jobs


def test_site_call_without_any_site():
    pm, alpha, k = model(cases.MODEL_CPG)
    rng = np.random.default_rng(12)
    refs = [make_ref(30, {}), "ACG", make_ref(80, {})]
    rows = [random_records(rng, 20, 30, k, len(alpha) ** k), NONE, NONE]
    calls, _ = check_sites(pm, alpha, k, refs, rows, SITE_AMB)
    assert [len(c["x"]) for c in calls] == [0, 0, 0]


# ---- positions ------------------------------------------------------------------------------------------------------------
# X: ACGT (E, a letter of the model, is outside it: pos_for_each_covered's l < 0); Y: two letters; Z: eight options
POS_AMB = {"X": "TGCA", "Y": "EC", "Z": "TNGOECPA"}


def test_position_words_ends_and_kinds():
    pm, alpha, k = model(cases.MODEL_CPG)          # k = 6
    nk = len(alpha) ** k
    rng = np.random.default_rng(21)
    refs, rows = [], []
    # x = 60, k = 6: positions 60 .. 65 straddle the word edge (pos_for_each_covered takes word and pre[] anew for every d);
    # ambiguous at d = 0 (60), at 63 and 64, at d = k - 1 (65) and at x + k (66: not covered by x = 60); 127 is the last bit of
    # the last word of a reference of 128 = 2 * 64 positions, 122 its last k-mer
    marks = {60: "X", 63: "Y", 64: "X", 65: "Z", 66: "X", 122: "X", 127: "Y", 0: "X"}
    r = make_ref(128, marks)
    xs = [60] * 6 + [55, 59, 61, 66, 122, 122, 117, 0, 1, 30]
    refs.append(r)
    rows.append(random_records(rng, 200, 128, k, nk, xs=xs))
    # the same with 70 positions (not a multiple of 64): the last k-mer, x = 64, ends at bit 5 of the second word
    r = make_ref(70, {0: "Y", 63: "X", 64: "X", 69: "Z"})
    refs.append(r)
    rows.append(random_records(rng, 120, 70, k, nk, xs=[58, 59, 63, 64, 64, 0, 20]))
    # 64 positions exactly: one full word, the last k-mer x = 58 covers bit 63
    r = make_ref(64, {58: "X", 63: "X"})
    refs.append(r)
    rows.append(random_records(rng, 60, 64, k, nk, xs=[58, 58, 53, 57]))
    # positions but no record (x_min = x_max = -1); a position but no k-mer; records but no position (its x range still)
    refs += [make_ref(50, {7: "X", 40: "Y"}), "ACXG", make_ref(50, {})]
    rows += [NONE, NONE, random_records(rng, 40, 50, k, nk)]
    # every position ambiguous, the three kinds in turn: a record adds to k buckets, kinds of 4, 2 and 8 letters side by side
    r = "".join("XYZ"[i % 3] for i in range(40))
    refs.append(r)
    rows.append(random_records(rng, 150, 40, k, nk))
    calls, exp = check_positions(pm, alpha, k, refs, rows, POS_AMB)
    assert {60, 63, 64, 65, 66, 122, 127} <= set(exp[0]) and 69 in exp[1] and 63 in exp[2]
    assert [c["x_min"] for c in calls[3:5]] == [-1, -1] and calls[5]["x_min"] >= 0 and len(calls[5]["p"]) == 0
    assert {l for c in calls for l in c["letters"]} == {"ACGT", "CE", "ACEGNOPT"}
    # l < 0 happened: some record that covers position 60 of the first job has an E there and is no row of it
    p60 = rows[0][(rows[0]["x"] <= 60) & (rows[0]["x"] >= 55)]
    assert exp[0][60][1] < len(p60)


def bucket_job(k, sizes, lead_records=0, salt=0):
    """one job of the ACGT model with a bucket of sizes[i] rows at position 10 * i + 4: row r of a bucket is a record at
    x = p - r % k whose path k-mer has letter r % 4 of ACGT at p, the posteriors ref.bucket_prob_e7's; the buckets' rows are
    dealt out in turn, so that no bucket's rows are neighbours in the record order, after lead_records records that cover no
    ambiguous position.  k_pos_scatter writes row ordinal << 24 | letter << 20 | units, k_pos_fold sorts and folds serially."""
    alpha = "ACGT"
    length = 10 * len(sizes) + 2 * k
    r = make_ref(length, {10 * i + 4: "X" for i in range(len(sizes))})
    per = []
    for i, n in enumerate(sizes):
        p = 10 * i + 4
        probs = ref.bucket_prob_e7(n, salt)
        b = []
        for q in range(n):
            d = q % k
            kmer = ["ACGT"[(q // 4 + t) % 4] for t in range(k)]
            kmer[d] = "ACGT"[q % 4]
            b.append((p - d, ref.kmer_id("".join(kmer), alpha), probs[q]))
        per.append(b)
    out = [(length - k, 0, 5000000)] * lead_records      # (the last k-mer lies beyond the last marked position)
    for q in range(max(sizes)):
        out += [b[q] for b in per if q < len(b)]
    return r, np.array(out, dtype=ref.RECORD_DTYPE)


def test_position_buckets_in_row_order():
    pm, alpha, k = model(cases.MODEL_5MER)
    assert alpha == "ACGT" and k == 5
    sizes = [1, 2, 16, 63, 64, 65, 300]
    # a job before and after it (base[j], loc[] per job: k_pos_job_scan and k_site_scan), the second with the sizes reversed
    jobs = [bucket_job(k, [3, 5]), bucket_job(k, sizes), bucket_job(k, sizes[::-1], salt=1)]
    # a bucket of 12 rows fed from records 4090 .. 4101 of its job: six from the first 4096-record chunk, six from the second
    # (k_pos_scatter's ordinal is C.local + i, which must run on through the chunk edge)
    r, rec = bucket_job(k, [12], lead_records=CHUNK - 6)
    assert len(rec) == CHUNK + 6 and (rec["x"][:CHUNK - 6] == len(r) - k).all() and (rec["x"][CHUNK - 6:] <= 4).all()
    jobs.append((r, rec))
    refs, rows = [j[0] for j in jobs], [j[1] for j in jobs]
    calls, exp = check_positions(pm, alpha, k, refs, rows, {"X": "ACGT"})
    assert [exp[1][10 * i + 4][1] for i in range(len(sizes))] == sizes
    assert exp[3][4][1] == 12
    # the planted order is what is folded: the same rows in reversed record order give other sums for the large buckets
    back = position_calls(pm, refs[1:2], [rows[1][::-1].copy()], {"X": "ACGT"})[0]
    for i, n in enumerate(sizes):
        same = back["sum"][i].tobytes() == calls[1]["sum"][i].tobytes()
        assert same == (n <= 2), n


def test_position_whose_rows_all_print_zero():
    """A position covered only by rows that print 0.000000 has total 0.  The reference divides by zero there
    (alignmentAnalysisLib.py:230-233); the rule here is the site fold's for a zero sum: the record is reported with its n_rows,
    sum all 0.0 and prob all 0.0.  Before k_pos_fold guarded acc[l] / total this test got prob = [nan, nan, nan, nan] at
    position 4 on the device."""
    pm, alpha, k = model(cases.MODEL_5MER)
    r = make_ref(40, {4: "X", 20: "X", 30: "X"})
    ida, idc = ref.kmer_id("ACGTA", alpha), ref.kmer_id("CCGTA", alpha)
    #            position 4: three rows, all zero      position 20: zero rows and one that prints 0.000001     30: no row
    rec = recs([4, 4, 0, 20, 20, 16], [ida, idc, ida, ida, idc, idc], [0, 4, 5, 3, 6, 0])
    calls, exp = check_positions(pm, alpha, k, [r, r], [rec, NONE], {"X": "ACGT"})
    got = calls[0]
    assert got["p"].tolist() == [4, 20] and got["n_rows"].tolist() == [3, 3]
    print("zero-total position: sum", got["sum"][0][:4], "prob", got["prob"][0][:4])
    assert not np.isnan(got["prob"]).any()
    assert got["sum"][0].tobytes() == np.zeros(8).tobytes() and got["prob"][0].tobytes() == np.zeros(8).tobytes()
    assert got["prob"][1][:4].tolist() == [0.0, 1.0, 0.0, 0.0]


# ---- the records entries against the chained path ---------------------------------------------------------------------------
def test_batch_calls_equal_the_records_entries_fed_the_batch_own_pairs():
    p = sa.default_params()
    # two 300-event CpG reads: sa_batch_site_calls
    pm, alpha, k = model(cases.MODEL_CPG)
    jobs = cases.synthetic_jobs(cases.MODEL_CPG, 2, 300, 410, cpg_ambiguous=True)
    assert all("X" in j["ref"] for j in jobs)
    b = sa.Batch(pm, p, jobs, ambig=sa.default_ambig({"X": "CE"}), flags=sa.FLAG_SITE_CALLS)
    b.run()
    calls = b.site_calls()
    pairs = [b.pairs(j) for j in range(2)]
    b.close()
    assert sum(len(c["x"]) for c in calls) > 5
    same_bytes(calls, site_calls(pm, [j["ref"] for j in jobs], pairs, {"X": "CE"}), SITE_FIELDS)
    # two 300-event reads with X every 10th position: sa_batch_position_calls
    pm, alpha, k = model(cases.MODEL_6MER)
    jobs = cases.synthetic_jobs(cases.MODEL_6MER, 2, 300, 420)
    for j in jobs:
        r = list(j["ref"])
        r[3::10] = "X" * len(r[3::10])
        j["ref"] = "".join(r)
    b = sa.Batch(pm, p, jobs, ambig=sa.default_ambig({"X": "ACGT"}), flags=sa.FLAG_POSITION_CALLS)
    b.run()
    calls = b.position_calls()
    pairs = [b.pairs(j) for j in range(2)]
    b.close()
    assert sum(len(c["p"]) for c in calls) > 20
    same_bytes(calls, position_calls(pm, [j["ref"] for j in jobs], pairs, {"X": "ACGT"}), POS_FIELDS)
