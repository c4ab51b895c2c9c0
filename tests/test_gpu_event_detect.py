"""Event detection from raw current on the GPU (sa_detect.hip) and the chain into event alignment
(sa_raw_event_align_batch, the reference's load_from_raw2).  The detector is held bit for bit to the CPU restatement
tests/event_detect_ref.py, which tests/test_host_event_detect.py pins to the reference's literals; the chain's literals
are asserted here on the GPU's own output, with the reference test (tests/eventAlignerTests.c) and line cited."""
import os

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import synth

import event_detect_ref as R
from test_host_event_detect import DNA_MODEL, RNA_MODEL, dna_sequence, fixture, rna_sequence

pytestmark = pytest.mark.gpu

READS = ("read61_rna", "read108_dna", "read1108_dna")


def job_of(name):
    f = fixture(name)
    a = np.asarray(f["attrs_f64_bits"], dtype=np.uint64).view(np.float64)
    return dict(raw=f["raw"], digitisation=a[0], offset=a[1], range=a[2], sample_rate=a[3], start_time=a[4])


def expected(job, params):
    a = dict(digitisation=np.float32(job["digitisation"]), offset=np.float32(job["offset"]), range=np.float32(job["range"]),
             sample_rate=np.float32(job["sample_rate"]), start_time=np.float32(job["start_time"]))
    return R.basecalled_table(R.detect_events(R.raw_to_pa(job["raw"], **a), params), **a)


def assert_same_events(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    assert np.array_equal(got["raw_start"], exp["raw_start"]), what
    assert np.array_equal(got["raw_length"], exp["raw_length"]), what
    # event_t's mean / stdv are floats: compared as float32 bit patterns
    for f in ("mean", "stdv"):
        g, e = got[f].astype(np.float32).view(np.uint32), exp[f].astype(np.float32).view(np.uint32)
        assert np.array_equal(got[f], got[f].astype(np.float32).astype(np.float64)), (what, f)
        assert np.array_equal(g, e), (what, f, int(np.argmax(g != e)))
    for f in ("start", "length"):
        assert np.array_equal(got[f].view(np.uint64), exp[f].view(np.uint64)), (what, f)
    assert (got["kmer_idx"] == -1).all() and (got["move"] == 0).all() and (got["p_model_state"] == 0).all()


@pytest.mark.parametrize("params", [R.DEFAULTS, R.RNA], ids=["dna_params", "rna_params"])
def test_real_reads_bit_identical_to_the_restatement(params):
    jobs = [job_of(n) for n in READS]
    st = {}
    got = sa.detect_events_batch(jobs, params=params, stats=st)
    for name, job, g in zip(READS, jobs, got):
        assert_same_events(g, expected(job, params), name)
    assert (st["status"] == 0).all() and st["kernel_ms"] > 0
    # params=None picks the preset by the RNA flag
    dflt = sa.detect_events_batch(jobs, rna=params == R.RNA)
    for g, d in zip(got, dflt):
        assert np.array_equal(g, d)


def test_rna_chain_reference_literals():
    job = job_of("read61_rna")
    out = sa.raw_event_align_batch(sa.Model.load(RNA_MODEL), [job], [rna_sequence()], rna=True)[0]
    ev = out["events"]
    # test_event_table_to_basecalled_table (:131-150)
    e = ev[1]
    assert e["raw_start"] == 7 and e["raw_length"] == 15
    assert abs(e["mean"] - 87.082771) < 1e-3 and abs(e["stdv"] - 1.637721) < 1e-3
    assert abs(e["start"] - 77.195221) < 1e-4 and abs(e["length"] - 0.004980) < 1e-4
    # test_estimate_scalings_using_mom (:320-345)
    assert abs(out["scale"] - 1.016111) < 1e-4 and abs(out["shift"] - 20.720264) < 1e-4
    # test_adaptive_banded_simple_event_align (:404-433): the popped (last) pair
    assert out["status"] == 0 and (out["kmer_idx"][-1], out["event_idx"][-1]) == (453, 1219)
    # test_load_from_raw_rna (:436-466): 1220 rows written, time order, first AACCT, last CCTAC
    ms = [m for m in out["model_state"] if m]
    assert len(ms) == 1220 and ms[0] == "AACCT" and ms[-1] == "CCTAC"
    mapped = ev[ev["kmer_idx"] >= 0]
    assert (mapped["p_model_state"] > 0).all() and (mapped["p_model_state"] <= 1).all()
    assert (ev[ev["kmer_idx"] < 0]["p_model_state"] == 0).all()


def test_dna_chain_reference_literals():
    job = job_of("read108_dna")
    out = sa.raw_event_align_batch(sa.Model.load(DNA_MODEL), [job], [dna_sequence()])[0]
    assert len(out["events"]) == 11100 and out["status"] == 0
    # test_load_from_raw_dna (:468-490)
    ms = [m for m in out["model_state"] if m]
    assert len(ms) == 11020 and ms[0] == "TGCAT" and ms[-1] == "AAACT"
    # test_alignment_to_base_event_map (:223-263): consecutive rows overlap by k - move letters
    k, prev = 5, None
    for m, mv in zip(out["model_state"], out["events"]["move"].tolist()):
        if not m:
            continue
        if prev is not None:
            assert 0 <= mv and prev[mv:] == m[:k - mv], (prev, m, mv)
        prev = m


def _mixed_jobs():
    jobs = []
    w2 = R.DEFAULTS[1]
    lengths = [1, 2, 3, 5, 2 * w2 - 1, 2 * w2, 2 * w2 + 1, 2 * 14 - 1, 2 * 14, 2 * 14 + 1, 64, 100, 1000, 4097]
    for i, n in enumerate(lengths):
        jobs.append(synth.make_raw(9000 + i, n, n_samples=n))
    for i in range(280):
        n = int(np.random.default_rng(i).integers(20, 6000))
        jobs.append(synth.make_raw(9100 + i, n // 8 + 1, n_samples=n))
    # constant current with unit = 1 pA per count: every window sum is exact, every t-statistic 0, no peak.  (A constant
    # current whose sums round is not flat to the detector: a rounding difference over a variance clamped to FLT_MIN
    # is a huge t-statistic, in the reference as here.)
    jobs.append(dict(raw=np.full(5000, 80, dtype=np.int16), digitisation=8192.0, offset=0.0, range=8192.0,
                     sample_rate=4000.0, start_time=1234.0))
    jobs.append(synth.make_raw(2, 45000, n_samples=400000))
    jobs.append(synth.make_raw(3, 130000, n_samples=(1 << 20) + 12345))
    return jobs


@pytest.mark.parametrize("params", [R.DEFAULTS, R.RNA, (4, 9, 2.0, 8.0, 0.5)], ids=["dna", "rna", "custom"])
def test_mixed_synthetic_batch_bit_identical(params):
    jobs = _mixed_jobs()
    st = {}
    got = sa.detect_events_batch(jobs, params=params, stats=st)
    for j, (job, g) in enumerate(zip(jobs, got)):
        exp = expected(job, params)
        assert_same_events(g, exp, j)
        # the table tiles the read
        assert g["raw_start"][0] == 0 and (g["raw_start"][1:] == g["raw_start"][:-1] + g["raw_length"][:-1]).all()
        assert g["raw_start"][-1] + g["raw_length"][-1] == len(job["raw"])
        assert (st["status"][j] == sa.RAW_NO_PEAK) == (len(g) == 1)
    assert st["status"][-3] == sa.RAW_NO_PEAK and len(got[-3]) == 1
    # the synthetic levels are found: with the DNA preset nearly every true boundary of the long reads has a detected one
    # within 2 samples (the detector also splits some levels: it is not checked for precision)
    for job, g in zip(jobs[-2:], got[-2:]):
        if params == R.DEFAULTS:
            b, s = np.asarray(job["boundaries"]), np.sort(g["raw_start"][1:])
            i = np.searchsorted(s, b)
            d = np.minimum(np.abs(b - s[np.clip(i - 1, 0, len(s) - 1)]), np.abs(b - s[np.clip(i, 0, len(s) - 1)]))
            assert (d <= 2).mean() > 0.9, (d <= 2).mean()


def test_chain_equals_its_composition():
    pm = sa.Model.load(DNA_MODEL)
    jobs = [job_of("read108_dna"), job_of("read1108_dna")]
    seqs = [dna_sequence(), dna_sequence()]          # the second read does not belong to this sequence: a failing status
    chain = sa.raw_event_align_batch(pm, jobs, seqs)
    det = sa.detect_events_batch(jobs)
    ea_jobs = []
    for d, s in zip(det, seqs):
        sh, sc = sa.scalings_mom(pm, s, d["mean"])
        ea_jobs.append(dict(sequence=s, event_mean=d["mean"], scale=sc, shift=sh, var=1.0))
    ea = sa.event_align_batch(pm, ea_jobs)
    for c, d, (k, e, st), j in zip(chain, det, ea, ea_jobs):
        assert np.array_equal(c["events"][["raw_start", "raw_length", "mean", "stdv", "start", "length"]],
                              d[["raw_start", "raw_length", "mean", "stdv", "start", "length"]])
        assert c["shift"] == j["shift"] and c["scale"] == j["scale"]
        assert c["status"] == st and np.array_equal(c["kmer_idx"], k) and np.array_equal(c["event_idx"], e)
        if st:
            assert (c["events"]["kmer_idx"] == -1).all()
    # RNA: the aligner sees the reversed events
    rm = sa.Model.load(RNA_MODEL)
    job = job_of("read61_rna")
    c = sa.raw_event_align_batch(rm, [job], [rna_sequence()], rna=True)[0]
    d = sa.detect_events_batch([job], rna=True)[0]
    mean_rev = d["mean"][::-1].copy()
    sh, sc = sa.scalings_mom(rm, rna_sequence(), mean_rev, flags=sa.FLAG_RNA)
    k, e, st = sa.event_align_batch(rm, [dict(sequence=rna_sequence(), event_mean=mean_rev, scale=sc, shift=sh)],
                                    flags=sa.FLAG_RNA)[0]
    assert (c["shift"], c["scale"], c["status"]) == (sh, sc, st)
    assert np.array_equal(c["kmer_idx"], k) and np.array_equal(c["event_idx"], e)


def test_empty_read_is_einval():
    good = synth.make_raw(5, 100)
    empty = dict(good, raw=np.zeros(0, dtype=np.int16))
    with pytest.raises(sa.SaError) as ei:
        sa.detect_events_batch([good, empty])
    assert ei.value.code == -1
    with pytest.raises(sa.SaError) as ei:
        sa.raw_event_align_batch(sa.Model.load(DNA_MODEL), [empty], [dna_sequence()])
    assert ei.value.code == -1


def test_a_batch_equals_its_jobs_one_at_a_time_and_scratch_is_reused():
    """Release, a call of three reads, the full call twice (the first grows every slot of the scratch, the second reuses it),
    every read alone, release, the full call again: the same event tables and status words each time."""
    jobs = [synth.make_raw(9500 + i, n // 8 + 1, n_samples=n) for i, n in enumerate((2000, 6000, 2345, 4097, 3001, 5555, 2600, 4800))]

    def run(some):
        st = {}
        got = sa.detect_events_batch(some, stats=st)
        return got, np.asarray(st["status"]).copy()

    def same(a, b):
        return len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])
    sa.detect_release()
    small = run(jobs[:3])
    first = run(jobs)
    second = run(jobs)
    assert all(len(g) > 1 for g in first[0])
    assert same(first, second) and same((first[0][:3], first[1][:3]), small)
    singles = [run([j]) for j in jobs]
    assert same(([s[0][0] for s in singles], np.concatenate([s[1] for s in singles])), first)
    sa.detect_release()
    assert same(run(jobs), first)
