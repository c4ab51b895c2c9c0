"""Per-position profile of all reads' posteriors on the GPU (sa_position_profile_*): the table must equal the restatement in
profile_ref.py field for field and bit for bit -- the restatement's entropy sums use sa_profile_entropy_term, so they are exactly
equal -- with the LDS window and with SA_PROFILE_DIRECT alike, in one call or in many, across checkpoint and rollback; a refused
call adds nothing; and chained onto a finished batch it equals add_records fed from the same batch's pairs."""
import numpy as np
import pytest

import signalalign_amd as sa

import sa_cases as cases
import profile_ref as ref

pytestmark = pytest.mark.gpu

LENS = [30000, 900]
NAMES = ["big", "small"]
MODELS = {"acgt5": cases.MODEL_5MER, "acegt6": cases.MODEL_CPG}
_TERMS = {}


def _term(u):
    if u not in _TERMS:
        _TERMS[u] = sa.profile_entropy_term(u)
    return _TERMS[u]


def _refs():
    rng = np.random.default_rng(3)
    return ["".join(rng.choice(list("ACGTacgtN"), size=n)) for n in LENS]


def _job(contig, pos0, sign, x, rng=None, n_kmers=None, kmer_id=None, prob_e7=None):
    x = np.asarray(x, dtype=np.int32)
    if kmer_id is None:
        kmer_id = rng.integers(0, n_kmers, size=len(x))
    if prob_e7 is None:
        prob_e7 = rng.integers(0, 10 ** 7 + 1, size=len(x))
    return dict(contig=contig, pos0=int(pos0), pos_sign=sign, x=x, kmer_id=np.asarray(kmer_id, dtype=np.int32),
                prob_e7=np.asarray(prob_e7, dtype=np.int64))


def _shape_jobs(k, n_alpha, seed):
    """every shape the kernels treat differently, as jobs of one call"""
    rng = np.random.default_rng(seed)
    nk = n_alpha ** k
    J = lambda *a, **kw: _job(*a, rng=rng, n_kmers=nk, **kw)
    jobs = [
        J(0, 50, 1, [3]),                                               # a single record
        J(0, 70, 1, []),                                                # no record, among others
        J(0, 0, 1, np.arange(120) // 2),                                # forward, the first k-mer starts at contig position 0
        J(1, LENS[1] - (99 + k), 1, np.arange(100)),                    # forward, the last letter is the contig's last position
        J(0, 149 + k - 1, -1, np.arange(150)),                          # backward, the last letter lies at contig position 0
        J(1, LENS[1] - 1, -1, np.arange(80)),                           # backward, the first letter is the contig's last position
        J(0, 1000, 1, np.arange(4095) // 2),                            # the chunk boundary: 4095, 4096 and 4097 records
        J(0, 6000, -1, np.arange(4096) // 2),
        J(0, 5000, 1, np.arange(4097) // 2),
        J(0, 100, 1, np.tile([0, 20000], 100)),                         # consecutive records jump by more than any window
        J(0, 25000, -1, np.tile([20000, 0], 37)),
        J(0, 9000, 1, np.zeros(6000), kmer_id=np.full(6000, nk - 2), prob_e7=np.full(6000, 10 ** 7)),   # 6000 x 10^6 units > 2^32
        J(0, 9100, 1, [0, 1, 2, 3, 4], prob_e7=[0, 4, 5, 5000000, 10 ** 7]),
        J(0, 9200, 1, [0, 1, 40, 41]),                                  # a span with an untouched hole inside it
        J(1, 100, 1, np.arange(21 - k + 1)),                            # spans on contig 1: [100, 120],
        J(1, 121, 1, np.arange(20 - k + 1)),                            # adjacent [121, 140],
        J(1, 110, -1, np.arange(6 - k + 1) if k <= 6 else [0]),         # nested [105, 110] (backward),
        J(1, 200, 1, np.arange(11 - k + 1)),                            # disjoint [200, 210]
    ]
    for i in range(40):                                                 # 40 jobs piled on the same 30 positions, mixed signs
        x = rng.integers(0, 30 - k + 1, size=25)
        jobs.append(J(0, 8000, 1, x) if i % 3 else J(0, 8029, -1, x))
    return jobs


def _expected(calls, alphabet, k, refs, names=NAMES):
    P = ref.Profile(term=_term)
    for jobs in calls:
        for j in jobs:
            if len(j["x"]):
                P.add_file(ref.rows_of_records(names[j["contig"]], j["pos0"], j["pos_sign"], k, alphabet, j["x"].tolist(),
                                               j["kmer_id"].tolist(), j["prob_e7"].tolist()), j["pos_sign"] > 0)
    return P.finish(alphabet, names, refs), P.letters_seen(alphabet)


def _add(t, jobs, flags=0):
    first = np.concatenate([[0], np.cumsum([len(j["x"]) for j in jobs])]).astype(np.int64)
    cat = lambda f, dt: np.concatenate([j[f] for j in jobs]).astype(dt) if jobs else np.zeros(0, dtype=dt)
    t.add_records(jobs, first, cat("x", np.int32), cat("kmer_id", np.int32), cat("prob_e7", np.int64), flags=flags)


def _check(got, seen, exp, exp_seen, n_alpha):
    assert len(got) == len(exp)
    assert got["contig"].tolist() == [s["contig"] for s in exp] and got["pos"].tolist() == [s["pos"] for s in exp]
    for f in ("read_count", "kmer_count", "entropy_units"):
        assert got[f].tolist() == [s[f] for s in exp], f
    pad = [0] * (8 - n_alpha)
    assert got["units"].tolist() == [s["units"] + pad for s in exp]
    want_prob = np.asarray([s["prob"] + [0.0] * (8 - n_alpha) for s in exp], dtype=np.float64).reshape(-1, 8)
    assert got["prob"].tobytes() == want_prob.tobytes()
    assert got["entropy"].tobytes() == np.asarray([s["entropy"] for s in exp], dtype=np.float64).tobytes()
    assert [c.decode() for c in got["ref"]] == [s["ref"] for s in exp]
    assert seen == exp_seen


_SHAPES = {}


def _shapes(name):
    """the shape jobs of a model and what the restatement makes of them, computed once"""
    if name not in _SHAPES:
        m = sa.Model.load(MODELS[name])
        alphabet, k = m.alphabet()
        jobs = _shape_jobs(k, len(alphabet), 5)
        _SHAPES[name] = (m, alphabet, k, jobs, _refs(), _expected([jobs], alphabet, k, _refs()))
    return _SHAPES[name]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_shapes_with_and_without_the_window(name):
    m, alphabet, k, jobs, refs, (exp, exp_seen) = _shapes(name)
    assert (alphabet, k) == {"acgt5": ("ACGT", 5), "acegt6": ("ACEGT", 6)}[name]
    tables = []
    for flags in (0, sa.PROFILE_DIRECT):
        t = sa.PositionProfile(m, LENS)
        _add(t, jobs, flags)
        got, seen = t.finish(refs)
        t.close()
        _check(got, seen, exp, exp_seen, len(alphabet))
        tables.append(got)
    assert tables[0].tobytes() == tables[1].tobytes()
    by = {(s["contig"], s["pos"]): s for s in exp}
    assert exp[0]["pos"] == 0 and exp[0]["kmer_count"] > 0 and by[(1, LENS[1] - 1)]["kmer_count"] > 0
    assert by[(0, 9000)]["units"][alphabet.index(ref.kmer_of_id(len(alphabet) ** k - 2, alphabet, k)[0])] == 6000 * 10 ** 6 > 2 ** 32
    # the hole of the job at 9200: inside its span, touched by no record
    hole = by[(0, 9200 + k + 5)]
    # (the two jobs whose records jump by 20 000 span it as well)
    assert (hole["read_count"], hole["kmer_count"], hole["ref"], hole["entropy"]) == (3, 0, "", 0.0)
    # read_count at every boundary of the adjacent, nested and disjoint spans of contig 1 (the two jobs at the contig's end start
    # beyond 700)
    rc = lambda p: by[(1, p)]["read_count"] if (1, p) in by else 0
    assert [rc(p) for p in (99, 100, 104, 105, 110, 111, 120, 121, 140, 141, 199, 200, 210, 211)] == [0, 1, 1, 2, 2, 1, 1, 1, 1, 0, 0, 1, 1, 0]
    if "E" in alphabet:   # E is its own complement: it is seen, and backward jobs add to it
        assert exp_seen >> alphabet.index("E") & 1 and any(s["units"][alphabet.index("E")] for s in exp)


def test_printed_units_of_small_and_extreme_posteriors():
    m, alphabet, k, _jobs, _r, _e = _shapes("acgt5")
    # 0, 4 and 5 print 0.000000 (the double 5e-07 lies below the tie), 5000000 prints 0.500000, 10^7 prints 1.000000
    jobs = [_job(0, 10, 1, [0, 10, 20, 30, 40], kmer_id=[0] * 5, prob_e7=[0, 4, 5, 5000000, 10 ** 7])]
    t = sa.PositionProfile(m, LENS)
    _add(t, jobs)
    got, seen = t.finish()
    t.close()
    exp, exp_seen = _expected([jobs], alphabet, k, None)
    _check(got, seen, exp, exp_seen, 4)
    by = {int(s["pos"]): s for s in got}
    assert [int(by[p]["units"][0]) for p in (10, 20, 30, 40, 50)] == [0, 0, 0, 500000, 1000000]
    assert seen == 1 and by[10]["prob"][0] == 0.0 and by[10]["kmer_count"] == 1 and by[10]["ref"] == b"N"
    assert by[40]["entropy"] == 0.5 and by[50]["entropy"] == 0.0 and by[15]["read_count"] == 1 and by[15]["kmer_count"] == 0


def test_one_call_and_five_shuffled_calls_agree():
    m, alphabet, k, jobs, refs, (exp, exp_seen) = _shapes("acgt5")
    order = np.random.default_rng(9).permutation(len(jobs))
    t = sa.PositionProfile(m, LENS)
    for part in np.array_split(order, 5):
        _add(t, [jobs[i] for i in part], flags=int(part[0]) & 1)      # (some calls with the window, some without)
    got, seen = t.finish(refs)
    t.close()
    _check(got, seen, exp, exp_seen, 4)


def test_checkpoint_and_rollback():
    m, alphabet, k, jobs, refs, _ = _shapes("acegt6")
    a, b = jobs[:12], jobs[12:30]
    t = sa.PositionProfile(m, LENS)
    with pytest.raises(sa.SaError) as e:
        t.rollback()
    assert e.value.code == -7                                         # SA_ESTATE: no checkpoint yet
    _add(t, a)
    t.checkpoint()
    _add(t, b)
    t.rollback()
    only_a = _expected([a], alphabet, k, refs)
    _check(*t.finish(refs), *only_a, 5)
    _add(t, b)
    _check(*t.finish(refs), *_expected([a, b], alphabet, k, refs), 5)
    t.rollback()                                                      # the checkpoint stays
    _check(*t.finish(refs), *only_a, 5)
    t.close()


def test_a_refused_call_adds_nothing():
    m, alphabet, k, jobs, refs, _ = _shapes("acgt5")
    nk = 4 ** k
    t = sa.PositionProfile(m, LENS)
    _add(t, jobs[:6])
    before, seen = t.finish(refs)
    good = [jobs[6], jobs[12]]
    def bad_job(**kw):
        j = dict(good[1])
        j.update(kw)
        return j
    x, kid, pe7 = good[1]["x"], good[1]["kmer_id"], good[1]["prob_e7"]
    cases_ = [
        bad_job(contig=2), bad_job(contig=-1), bad_job(pos_sign=0), bad_job(pos_sign=2),
        bad_job(kmer_id=np.r_[kid[:-1], nk].astype(np.int32)), bad_job(kmer_id=np.r_[-1, kid[1:]].astype(np.int32)),
        bad_job(prob_e7=np.r_[pe7[:-1], 10 ** 7 + 1]), bad_job(prob_e7=np.r_[-1, pe7[1:]]),
        bad_job(x=np.r_[-1, x[1:]].astype(np.int32)),
        bad_job(pos0=LENS[0] - (4 + k) + 1),                            # forward: the last letter one past the contig's end
        bad_job(pos0=4 + k - 2, pos_sign=-1),                          # backward: the last letter at -1
        bad_job(pos0=-1), bad_job(pos0=2 ** 62), bad_job(contig=1, pos0=LENS[1] - 3),
    ]
    for bad in cases_:
        for flags in (0, sa.PROFILE_DIRECT):
            with pytest.raises(sa.SaError) as e:
                _add(t, [good[0], bad], flags)
            assert e.value.code == -1
            again, seen2 = t.finish(refs)
            assert again.tobytes() == before.tobytes() and seen2 == seen
    with pytest.raises(sa.SaError) as e:
        t.add_records([good[0], good[0]], [0, 5, 3], good[0]["x"][:3], good[0]["kmer_id"][:3], good[0]["prob_e7"][:3])   # offsets that go back
    assert e.value.code == -1
    _add(t, good)                                                       # the table still works
    _check(*t.finish(refs), *_expected([jobs[:6], good], alphabet, k, refs), 4)
    t.close()


def test_create_refuses_what_it_cannot_hold():
    m6 = sa.Model.load(cases.MODEL_R73)        # ACEGOT: six letters fit, and every one of A, C, G, T has its complement
    t = sa.PositionProfile(m6, [100])
    t.close()
    m = sa.Model.load(cases.MODEL_5MER)
    for lens in ([], [-1], [2 ** 41]):
        with pytest.raises(sa.SaError) as e:
            sa.PositionProfile(m, lens)
        assert e.value.code == -1


@pytest.mark.parametrize("last_len", [2038, 2039])
def test_empty_contigs_and_a_span_that_ends_on_an_extra_slot(last_len):
    """2048 slots (the positions and one more per contig): one block of finish; 2049: a second block of one slot.  A k-mer ends on
    the last position of contig 3, so the -1 of its span lies on that contig's extra slot; no extra slot and no empty contig may
    get a site."""
    m, alphabet, k, _jobs, _r, _e = _shapes("acgt5")
    lens = [0, 5, 0, last_len, 0]
    assert sum(lens) + len(lens) == (2048 if last_len == 2038 else 2049)
    rng = np.random.default_rng(43)
    J = lambda *a: _job(*a, rng=rng, n_kmers=4 ** k)
    jobs = [J(1, 0, 1, [0]),                                            # all of contig 1
            J(3, last_len - (3 + k), 1, [0, 1, 3]),                     # forward, the last letter on the contig's last position
            J(3, k + 1, -1, [0, 2])]                                    # backward, the last letter on position 0
    names = ["c%d" % c for c in range(len(lens))]
    refs = ["", "acGTn", "", "".join(rng.choice(list("ACGTacgtN"), size=last_len)), ""]
    t = sa.PositionProfile(m, lens)
    _add(t, jobs)
    got, seen = t.finish(refs)
    t.close()
    _check(got, seen, *_expected([jobs], alphabet, k, refs, names), 4)
    where = list(zip(got["contig"].tolist(), got["pos"].tolist()))
    assert where[:5] == [(1, p) for p in range(5)] and where[5] == (3, 0) and where[-1] == (3, last_len - 1)
    assert all(c in (1, 3) and p < lens[c] for c, p in where) and got["read_count"].min() == 1


def test_a_table_whose_contigs_are_all_empty():
    m, alphabet, k, _jobs, _r, _e = _shapes("acgt5")
    t = sa.PositionProfile(m, [0, 0])
    assert [len(t.finish()[0]), t.finish(["", ""])[1]] == [0, 0]
    _add(t, [])                                                         # no record: nothing to refuse
    t.checkpoint()
    t.rollback()
    for contig in (0, 1):
        with pytest.raises(sa.SaError) as e:
            _add(t, [_job(contig, 0, 1, [0], kmer_id=[0], prob_e7=[10 ** 7])])
        assert e.value.code == -1                                       # SA_EINVAL: there is no position 0
    got, seen = t.finish()
    assert len(got) == 0 and seen == 0
    t.close()


# ---- chained onto a real batch ------------------------------------------------------------------------------------------------
def _batch_jobs():
    """two reads of sa_cases, an ambiguity letter in each so that path k-mers differ from the reference; the second is mapped
    with sign -1"""
    base = cases.synthetic_jobs(cases.MODEL_6MER, 2, 520, 400)
    jobs = []
    for j in base:
        r = j["ref"]
        jobs.append(dict(j, ref=r[:60] + "X" + r[61:200] + "X" + r[201:]))
    job_map = [dict(contig=0, pos0=700, pos_sign=1), dict(contig=0, pos0=900 + len(jobs[1]["ref"]) - 1, pos_sign=-1)]
    return jobs, job_map


def _new_batch(jobs, flags=0, run=True):
    pm = sa.Model.load(cases.MODEL_6MER)
    b = sa.Batch(pm, sa.default_params(), jobs, ambig=sa.default_ambig({"X": "ACGT"}), flags=flags)
    if run:
        b.run()
    return pm, b


@pytest.mark.parametrize("batch_flags", [0, sa.FLAG_EXACT])
def test_add_batch_equals_add_records_of_its_pairs(batch_flags):
    jobs, job_map = _batch_jobs()
    pm, b = _new_batch(jobs, batch_flags)
    rows, first = b.pairs_all()
    assert first[1] > 300 and first[2] - first[1] > 300
    refs = _refs()

    def table(add):
        t = sa.PositionProfile(pm, LENS)
        add(t)
        out = t.finish(refs)
        t.close()
        return out

    exp, exp_seen = table(lambda t: t.add_records(job_map, first, rows["x"], rows["kmer_id"], rows["prob_e7"]))
    assert len(exp) > 450 and exp["read_count"].max() == 2 and exp_seen == 0b1111
    # the path k-mers of an X position differ from the reference: more than one letter has units there
    assert ((exp["units"] > 0).sum(axis=1) > 1).any()
    # ... and the records path equals the restatement
    as_jobs = [dict(m, x=rows["x"][first[j]:first[j + 1]], kmer_id=rows["kmer_id"][first[j]:first[j + 1]],
                    prob_e7=rows["prob_e7"][first[j]:first[j + 1]]) for j, m in enumerate(job_map)]
    _check(exp, exp_seen, *_expected([as_jobs], "ACGT", 6, refs), 4)
    for flags in (0, sa.PROFILE_DIRECT):
        st = {}
        got, seen = table(lambda t: t.add_batch(b, job_map, flags=flags, stats=st))
        assert got.tobytes() == exp.tobytes() and seen == exp_seen and st["kernel_ms"] > 0
    if batch_flags == 0:
        b.release_device()                                              # the records go up again
        got, seen = table(lambda t: t.add_batch(b, job_map))
        assert got.tobytes() == exp.tobytes() and seen == exp_seen
    b.close()


def test_add_batch_refusals():
    jobs, job_map = _batch_jobs()
    pm = sa.Model.load(cases.MODEL_6MER)
    t = sa.PositionProfile(pm, LENS)

    def refused(b, code, the_map=job_map, table=t):
        with pytest.raises(sa.SaError) as e:
            table.add_batch(b, the_map)
        assert e.value.code == code

    plain = [dict(j, ref=j["ref"].replace("X", "A")) for j in jobs]     # (8-byte records need one path per cell)
    _, b = _new_batch(plain, sa.FLAG_PAIRS8)
    refused(b, -8)                                                      # SA_EUNSUPPORTED: no k-mer in the record
    b.close()
    _, b = _new_batch(jobs, sa.FLAG_VC_ROWS)
    refused(b, -1)                                                      # SA_EINVAL: rows dropped
    b.close()
    _, b = _new_batch(jobs, run=False)
    refused(b, -7)                                                      # SA_ESTATE: not run
    b.run()
    refused(b, -1, job_map[:1])                                         # not the batch's number of jobs
    refused(b, -1, [job_map[0], dict(job_map[1], pos0=100)])            # the backward read would end below position 0
    other = sa.PositionProfile(sa.Model.load(cases.MODEL_5MER), LENS)   # a model of another k
    refused(b, -1, table=other)
    assert len(other.finish()[0]) == 0 and len(t.finish()[0]) == 0      # nothing was added by any of them
    other.close()
    t.add_batch(b, job_map)
    assert len(t.finish()[0]) > 450
    b.close()
    t.close()
