"""Single-nucleotide probabilities marginalised over reads on the GPU (sa_snp_marginals_*): the accumulator must equal the
restatement in snp_marginals_ref.py bit for bit -- at every bucket depth its three fold kernels take (at most 16 rows, at most
1024, more), with rows arriving in shuffled order, whether the rows come in one call or in many, across checkpoint and rollback
-- and chained onto a finished batch it must equal the same batch's position calls carried over the host."""
import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import _capi

import sa_cases as cases
import snp_marginals_ref as ref

pytestmark = pytest.mark.gpu

LENS = [3000, 700]
# a site at each depth: both sides of the short / LDS boundary (16) and of the LDS / global one (1024), and powers of two
DEPTHS = [1, 2, 16, 17, 63, 64, 65, 300, 1024, 1025, 5000]


def _values(rng, n):
    """n x 4 values spread over 1e-12 .. 1: a sum of them in another order differs in its last bits"""
    return 10.0 ** rng.uniform(-12.0, 0.0, size=(n, 4))


def _site_array(rows):
    arr = np.zeros(len(rows), dtype=_capi.SNP_SITE_DTYPE)
    arr["pos"] = [r[1] for r in rows]
    arr["strand"] = [r[3] for r in rows]
    arr["p"] = [r[5] for r in rows]
    return arr


def _add(t, call):
    """one add_sites call: rows (contig, pos, run, strand, direction, p) of one contig, run and direction"""
    assert len({(r[0], r[2], r[4]) for r in call}) == 1
    t.add_sites(call[0][0], _site_array(call), call[0][4], run=call[0][2])


def _check(got, exp):
    assert len(got) == len(exp)
    assert got["contig"].tolist() == [s["contig"] for s in exp] and got["pos"].tolist() == [s["pos"] for s in exp]
    assert got["depth"].tolist() == [s["depth"] for s in exp]
    for f in ("fwd", "bwd", "prob"):
        assert np.array_equal(got[f], np.asarray([s[f] for s in exp], dtype=np.float64).reshape(-1, 4)), f
    assert np.array_equal(got["delta"], np.asarray([s["delta"] for s in exp], dtype=np.float64))
    assert [c.decode() for c in got["called"]] == [s["called"] for s in exp]
    assert [c.decode() for c in got["ref"]] == [s["ref"] for s in exp]
    assert got["is_proposal"].tolist() == [int(s["is_proposal"]) for s in exp]


def _random_calls(seed, n_calls=12, rows_per_call=60):
    rng = np.random.default_rng(seed)
    calls = []
    for run in range(n_calls):
        contig = int(rng.integers(0, 2))
        direction = int(rng.integers(0, 2))
        pos = rng.integers(0, 40, size=rows_per_call) * 3 + 100     # few sites, so that they collect rows from many calls
        pos[:2] = [0, LENS[contig] - 1]                              # the contig's first and last position
        strand = rng.integers(0, 2, size=rows_per_call)
        vals = _values(rng, rows_per_call)
        calls.append([(contig, int(pos[i]), run, int(strand[i]), direction, tuple(vals[i].tolist())) for i in range(rows_per_call)])
    return calls


def test_random_rows_two_contigs_both_directions_and_strands():
    calls = _random_calls(1)
    refs = ["".join(np.random.default_rng(2).choice(list("ACGTacgtN"), size=n)) for n in LENS]
    t = sa.SnpMarginals(LENS)
    for call in calls:
        _add(t, call)
    exp = ref.finish(ref.accumulate(calls), 1, refs)
    got = t.finish(1, refs)
    _check(got, exp)
    assert {s["contig"] for s in exp} == {0, 1} and exp[0]["pos"] == 0 and exp[-1]["pos"] == LENS[1] - 1
    assert any(s["is_proposal"] for s in exp) and any(s["ref"] == "N" for s in exp)
    assert any(any(s["fwd"]) and any(s["bwd"]) for s in exp)
    # without a reference: the same numbers, no proposal
    plain = t.finish(1)
    assert np.array_equal(plain["prob"], got["prob"]) and not plain["is_proposal"].any() and set(plain["ref"]) == {b"N"}
    t.close()


def _deep_call(seed=7):
    """one call whose rows hit one site per depth of DEPTHS, both strands, in shuffled order"""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([np.full(d, 50 + 10 * i) for i, d in enumerate(DEPTHS)])
    order = rng.permutation(len(pos))
    pos = pos[order]
    strand = rng.integers(0, 2, size=len(pos))
    vals = _values(rng, len(pos))
    return [(0, int(pos[i]), 4, int(strand[i]), 1, tuple(vals[i].tolist())) for i in range(len(pos))]


def test_every_depth_in_shuffled_order():
    call = _deep_call()
    acc = ref.accumulate([call])
    exp = ref.finish(acc)
    assert [s["depth"] for s in exp] == DEPTHS
    # the test means something only if the order matters for these values: folded backwards, every deep site differs
    back = ref.finish(ref.accumulate([call], reverse=True))
    for a, b in zip(exp, back):
        if a["depth"] >= 16:
            assert a["fwd"] != b["fwd"], a["depth"]
    t = sa.SnpMarginals(LENS)
    _add(t, call)
    _check(t.finish(), exp)
    # a second call on top of the stored sums, in the other direction and in another shuffle
    again = [(c, p, 5, s, 0, v) for (c, p, _r, s, _d, v) in _deep_call(8)]
    for a, b in zip(ref.finish(ref.accumulate([again])), ref.finish(ref.accumulate([again], reverse=True))):
        if a["depth"] >= 16:
            assert a["bwd"] != b["bwd"], a["depth"]                  # the order matters for the backward sums of this call too
    _add(t, again)
    _check(t.finish(), ref.finish(ref.accumulate([again], acc)))
    t.close()


def test_one_call_three_calls_and_one_row_per_call_agree():
    rng = np.random.default_rng(11)
    n = 240
    pos = rng.integers(0, 6, size=n) * 7 + 20
    strand = np.sort(rng.integers(0, 2, size=n))   # t rows first: cutting the list anywhere keeps the order of the whole
    vals = _values(rng, n)
    rows = [(1, int(pos[i]), 0, int(strand[i]), 1, tuple(vals[i].tolist())) for i in range(n)]
    exp = ref.finish(ref.accumulate([rows]))
    tables = []
    for cuts in ([0, n], [0, 70, 71, n], list(range(n + 1))):
        t = sa.SnpMarginals(LENS)
        for a, b in zip(cuts[:-1], cuts[1:]):
            _add(t, rows[a:b])
        tables.append(t.finish())
        t.close()
    for got in tables:
        _check(got, exp)
    assert tables[0].tobytes() == tables[1].tobytes() == tables[2].tobytes()


def test_checkpoint_and_rollback():
    calls = _random_calls(21, n_calls=6)
    t = sa.SnpMarginals(LENS)
    with pytest.raises(sa.SaError) as e:
        t.rollback()
    assert e.value.code == -7                                      # SA_ESTATE: no checkpoint yet
    for call in calls[:3]:
        _add(t, call)
    t.checkpoint()
    for call in calls[3:]:
        _add(t, call)
    t.rollback()
    _check(t.finish(), ref.finish(ref.accumulate(calls[:3])))
    for call in calls[3:]:
        _add(t, call)
    _check(t.finish(), ref.finish(ref.accumulate(calls)))
    t.rollback()                                                   # the checkpoint stays
    _check(t.finish(), ref.finish(ref.accumulate(calls[:3])))
    t.close()


def test_min_depth_zero_total_and_reference_letters():
    rows = [(0, 10, 0, 0, 1, (0.5, 0.25, 0.125, 0.125)), (0, 10, 0, 1, 1, (0.5, 0.25, 0.125, 0.125)),
            (0, 11, 0, 0, 1, (0.0, 0.0, 0.0, 0.0)), (0, 12, 0, 0, 1, (0.1, 0.7, 0.1, 0.1)), (0, 13, 0, 0, 1, (0.1, 0.1, 0.1, 0.7)),
            (0, 14, 0, 0, 1, (0.25, 0.25, 0.25, 0.25))]
    back = [(0, 10, 1, 0, 0, (0.0, 0.0, 0.0, 3.0)), (0, 13, 1, 0, 0, (0.9, 0.0, 0.0, 0.0))]
    refs = ["A" * 10 + "gCntA" + "A" * (LENS[0] - 15), "C" * LENS[1]]
    t = sa.SnpMarginals(LENS)
    _add(t, rows)
    _add(t, back)
    acc = ref.accumulate([rows, back])
    for md in (0, 1, 2, 3, 4):
        _check(t.finish(md, refs), ref.finish(acc, md, refs))
    got = t.finish(1, refs)
    # pos 10: backward T counts as A (4.0 of 5.0), reference g is G: a proposal.  11: total 0, no call.  12: reference n, no
    # proposal.  13: backward A counts as T, reference t is T.  14: a tie goes to the first letter, A == A
    assert [c.decode() for c in got["called"]] == ["A", "N", "C", "T", "A"]
    assert [c.decode() for c in got["ref"]] == ["G", "C", "N", "T", "A"]
    assert got["is_proposal"].tolist() == [1, 0, 0, 0, 0]
    assert got["prob"][0].tolist() == [0.8, 0.1, 0.05, 0.05] and got["delta"][0] == 0.8 - 0.05
    assert got["depth"].tolist() == [3, 1, 1, 2, 1] and len(t.finish(3, refs)) == 1
    t.close()


def test_a_site_outside_its_contig_is_refused_and_nothing_is_added():
    calls = _random_calls(31, n_calls=2)
    t = sa.SnpMarginals(LENS)
    _add(t, calls[0])
    before = t.finish()
    good = [r for r in calls[1] if r[0] == calls[1][0][0]]
    for bad_pos in (LENS[good[0][0]], -1):
        bad = good[:5] + [(good[0][0], bad_pos) + good[0][2:]] + good[5:]
        with pytest.raises(sa.SaError) as e:
            _add(t, bad)
        assert e.value.code == -1
        assert t.finish().tobytes() == before.tobytes()
    with pytest.raises(sa.SaError) as e:
        t.add_sites(2, _site_array(good), 1)                        # no such contig
    assert e.value.code == -1
    t.close()


@pytest.mark.parametrize("last_len", [2043, 2044])
def test_empty_contigs_around_a_last_slot_that_is_reported(last_len):
    """2048 positions: one block of finish, whose last slot is reported; 2049: a second block of one slot, reported.  The empty
    contigs share their offset with the next one, and no site may be given to them."""
    lens = [0, 5, 0, last_len, 0]
    assert sum(lens) == (2048 if last_len == 2043 else 2049)
    vals = _values(np.random.default_rng(41), 4)
    calls = [[(1, 0, 0, 0, 1, tuple(vals[0].tolist())), (1, 4, 0, 1, 1, tuple(vals[1].tolist()))],
             [(3, 0, 1, 0, 0, tuple(vals[2].tolist())), (3, last_len - 1, 1, 0, 0, tuple(vals[3].tolist()))]]
    refs = ["", "acGTn", "", "C" * last_len, ""]
    t = sa.SnpMarginals(lens)
    for call in calls:
        _add(t, call)
    got = t.finish(1, refs)
    t.close()
    _check(got, ref.finish(ref.accumulate(calls), 1, refs))
    assert list(zip(got["contig"].tolist(), got["pos"].tolist())) == [(1, 0), (1, 4), (3, 0), (3, last_len - 1)]


def test_a_table_whose_contigs_are_all_empty():
    t = sa.SnpMarginals([0, 0])
    assert len(t.finish()) == 0 and len(t.finish(1, ["", ""])) == 0
    t.add_sites(0, np.zeros(0, dtype=_capi.SNP_SITE_DTYPE), 1)     # no row: nothing to refuse
    t.checkpoint()
    t.rollback()
    for contig in (0, 1):
        with pytest.raises(sa.SaError) as e:
            _add(t, [(contig, 0, 0, 0, 1, (0.25, 0.25, 0.25, 0.25))])
        assert e.value.code == -1                                   # SA_EINVAL: there is no position 0
    assert len(t.finish()) == 0
    t.close()


# ---- chained onto a real batch ------------------------------------------------------------------------------------------------
STEP = 5
K = 6


def _batch_case():
    """6 reads: three pairs, each the t and c strand of one read (one run ordinal, one window per step), 5 jobs per read with X
    at the contig positions = s (mod 5); the middle pair is mapped backward (2 of the 6, not half: with the pairs' c strands
    that is 3 jobs' targets running along the contig and 3 against it, which is what the map has to get right).  Jobs are laid out c before t, so the order of the
    rows is not the order of the jobs."""
    base = cases.synthetic_jobs(cases.MODEL_6MER, 6, 520, 400)
    place = [(0, 100), (0, 100), (0, 180), (0, 180), (1, 40), (1, 40)]   # (contig, contig position of the read's lowest base)
    jobs, job_map = [], []
    for r in (1, 0, 3, 2, 5, 4):
        pair, strand = r // 2, r % 2
        backward = pair == 1
        same = (not backward and strand == 0) or (backward and strand == 1)   # the job's ref runs along the contig
        contig, lo = place[r]
        n = len(base[r]["ref"])
        pos0, sign = (lo, 1) if same else (lo + n - 1, -1)
        for s in range(STEP):
            jobs.append(dict(base[r], ref=sa.snp_substitute(base[r]["ref"], pos0, not same, STEP, s)))
            job_map.append(dict(contig=contig, pos0=pos0, pos_sign=sign, x0=lo if same else lo + n - K, x_sign=sign, strand=strand,
                                direction=int(same), run=pair, group=pair * STEP + s))
    return jobs, job_map


def _unchained(b, job_map):
    """Batch.position_calls() turned into rows on the host, window-filtered per group, added job after job in (run, strand,
    job) order"""
    calls = b.position_calls()
    window = {}
    for c, m in zip(calls, job_map):
        if c["x_min"] < 0:
            continue
        idx = [m["x0"] + m["x_sign"] * c["x_min"], m["x0"] + m["x_sign"] * c["x_max"]]
        lo, hi = window.get(m["group"], (min(idx), max(idx)))
        window[m["group"]] = (min(lo, *idx), max(hi, *idx))
    t = sa.SnpMarginals(LENS, step=STEP)
    n_rows = n_dropped = 0
    for j in sorted(range(len(job_map)), key=lambda j: (job_map[j]["run"], job_map[j]["strand"], j)):
        c, m = calls[j], job_map[j]
        if not len(c["p"]):
            continue
        w_lo, w_hi = sa.snp_site_window(*window[m["group"]], STEP)
        rows = []
        for i, p in enumerate(c["p"].tolist()):
            pos = m["pos0"] + m["pos_sign"] * p
            if not w_lo <= pos < w_hi:
                n_dropped += 1
                continue
            letters = c["letters"][i]
            rows.append((pos, m["strand"], [float(c["prob"][i][letters.index(l)]) if l in letters else 0.0 for l in "ACGT"]))
        n_rows += len(rows)
        t.add_sites(m["contig"], rows, m["direction"], run=m["run"])
    out = t.finish()
    t.close()
    return out, n_rows, n_dropped


def _chained(b, job_map):
    t = sa.SnpMarginals(LENS, step=STEP)
    st = {}
    t.add_batch(b, job_map, stats=st)
    out = t.finish()
    t.close()
    return out, st


def _new_batch(jobs, flags=0):
    pm = sa.Model.load(cases.MODEL_6MER)
    b = sa.Batch(pm, sa.default_params(), jobs, ambig=sa.default_ambig({"X": "ACGT"}), flags=flags | sa.FLAG_POSITION_CALLS)
    b.run()
    return b


@pytest.mark.parametrize("flags", [0, sa.FLAG_EXACT])
def test_chained_equals_unchained(flags):
    jobs, job_map = _batch_case()
    b = _new_batch(jobs, flags)
    exp, n_rows, n_dropped = _unchained(b, job_map)
    got, st = _chained(b, job_map)
    assert n_rows > 1000 and len(exp) > 400 and exp["depth"].max() >= 4 and set(exp["contig"].tolist()) == {0, 1}
    assert got.tobytes() == exp.tobytes()
    assert st["kernel_ms"] > 0 and st["kernel_ms_position_fold"] > 0
    if flags == 0:
        # the position calls are as before the accumulator read them, and the same table comes out after the device storage
        # went back (the records go up again)
        b.release_device()
        again, _ = _chained(b, job_map)
        assert again.tobytes() == exp.tobytes()
    b.close()


# read 516 with 40 foreign bases: position 227 of the job of phase 2 is covered by seven rows, each of 1e-7 .. 4e-7 (found by
# running reads 500 .. 529 once; about one in six has such a position)
ZERO_READ, ZERO_TAIL = 516, 40


def _zero_total_case(read=ZERO_READ, tail=ZERO_TAIL):
    """one forward read of 300 events whose reference runs on for `tail` foreign bases past its last event, as STEP jobs with X at
    the contig positions = s (mod STEP), at threshold 1e-7: out in the tail the posteriors fall off, and somewhere every row that
    covers an X prints 0.000000"""
    job = cases.synthetic_jobs(cases.MODEL_6MER, 1, 300, read)[0]
    other = cases.synthetic_jobs(cases.MODEL_6MER, 1, 300, read + 1000)[0]
    ref_, lo = job["ref"] + other["ref"][:tail], 100
    jobs = [dict(job, ref=sa.snp_substitute(ref_, lo, False, STEP, s)) for s in range(STEP)]
    job_map = [dict(contig=0, pos0=lo, pos_sign=1, x0=lo, x_sign=1, strand=0, direction=1, run=0, group=s) for s in range(STEP)]
    pm = sa.Model.load(cases.MODEL_6MER)
    b = sa.Batch(pm, sa.default_params(threshold=1e-7), jobs, ambig=sa.default_ambig({"X": "ACGT"}), flags=sa.FLAG_POSITION_CALLS)
    b.run()
    return b, job_map, lo


def _zero_total_positions(b):
    """[(job, position, rows)] of the batch's position calls whose sums are all zero"""
    return [(j, int(p), int(n)) for j, c in enumerate(b.position_calls())
            for p, n, s in zip(c["p"], c["n_rows"], c["sum"]) if n > 0 and not s.any()]


def test_add_batch_adds_a_row_of_zeros_for_a_position_whose_rows_all_print_zero():
    """k_pos_fold reports such a position with probabilities of 0.0 (the reference divides by zero there); k_mg_batch_rows copies
    them into a row: the site gains depth and nothing else, as add_sites fed the same zeros"""
    b, job_map, lo = _zero_total_case()
    zero = _zero_total_positions(b)
    assert (2, 227, 7) in zero, "the batch no longer holds the position whose rows all print zero"
    calls = b.position_calls()
    assert not any(np.isnan(c["prob"]).any() for c in calls)
    exp, n_rows, _ = _unchained(b, job_map)
    got, _ = _chained(b, job_map)
    assert n_rows > 50 and got.tobytes() == exp.tobytes()
    for j, p, n in zero:
        site = got[(got["contig"] == 0) & (got["pos"] == lo + p)]
        # (one job per phase: no other job has an X at this contig position)
        assert len(site) == 1 and site["depth"][0] == 1
        assert not site["fwd"].any() and not site["bwd"].any() and not site["prob"].any() and site["called"][0] == b"N"
        assert calls[j]["prob"][calls[j]["p"].tolist().index(p)].tobytes() == np.zeros(8).tobytes()
    b.close()


def test_chained_over_several_forward_passes(monkeypatch):
    jobs, job_map = _batch_case()
    monkeypatch.setenv("SA_F_BUDGET_CELLPATHS", "400000")
    b = _new_batch(jobs)
    assert b.stats().n_chunks >= 2
    exp, _, _ = _unchained(b, job_map)
    got, _ = _chained(b, job_map)
    assert len(exp) > 400 and got.tobytes() == exp.tobytes()
    b.close()


def test_add_batch_error_contract():
    jobs, job_map = _batch_case()
    jobs, job_map = jobs[:STEP], job_map[:STEP]
    pm = sa.Model.load(cases.MODEL_6MER)
    amb = sa.default_ambig({"X": "ACGT"})
    t = sa.SnpMarginals(LENS, step=STEP)
    b = sa.Batch(pm, sa.default_params(), jobs, ambig=amb)          # without the flag
    b.run()
    with pytest.raises(sa.SaError) as e:
        t.add_batch(b, job_map)
    assert e.value.code == -7
    b.close()
    b = sa.Batch(pm, sa.default_params(), jobs, ambig=amb, flags=sa.FLAG_POSITION_CALLS)
    with pytest.raises(sa.SaError) as e:
        t.add_batch(b, job_map)                                     # not run
    assert e.value.code == -7
    b.run()
    with pytest.raises(sa.SaError) as e:
        t.add_batch(b, job_map[:-1])                                # not the batch's number of jobs
    assert e.value.code == -1
    short = sa.SnpMarginals([150, LENS[1]], step=STEP)              # the read lies at 100 .. 400 of contig 0
    with pytest.raises(sa.SaError) as e:
        short.add_batch(b, job_map)                                 # positions inside the window and outside the contig
    assert e.value.code == -1
    assert len(short.finish()) == 0 and len(t.finish()) == 0        # nothing was added by any of them
    short.close()
    t.add_batch(b, job_map)
    assert len(t.finish()) > 100
    b.close()
    t.close()
