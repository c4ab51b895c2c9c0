"""Labelled signal on the GPU (sa_signal_labels_records, sa_batch_signal_labels): every field of the four sets and of the per-read
record must equal (==) the restatement in signal_labels_ref.py over the smallest shapes at which the kernels can go wrong, all of
them separate jobs of one call; and chained onto a finished batch the call equals signal_labels_records fed from the batch's pairs."""
import numpy as np
import pytest

import signalalign_amd as sa

import sa_cases as cases
import signal_labels_ref as ref

pytestmark = pytest.mark.gpu

TILE = sa.LABEL_SAMPLE_TILE
ALL = sa.LABEL_MEA | sa.LABEL_FULL | sa.LABEL_BANDS | sa.LABEL_SAMPLES
AUTO = "auto"


def _job(rng, n_events, y, x=None, lengths=None, gaps=None, lead=0, tail=0, ref_first=0, ref_step=1, base_shift=2, path=AUTO, prob_e7=None):
    """a job from the events of its records (y, in record order); raw starts from the events' lengths and the gaps after them"""
    y = np.asarray(y, dtype=np.int32)
    lengths = np.asarray(lengths if lengths is not None else rng.integers(1, 12, size=n_events), dtype=np.int64)
    gaps = np.asarray(gaps if gaps is not None else rng.integers(0, 6, size=n_events) * (rng.random(n_events) < 0.2), dtype=np.int64)
    raw_start = lead + np.concatenate([[0], np.cumsum(lengths + gaps)[:-1]]).astype(np.int64)
    n_samples = int(raw_start[-1] + lengths[-1] + tail)
    x = np.asarray(x if x is not None else 100 + y // 2 + rng.integers(0, 3, size=len(y)), dtype=np.int32)
    if prob_e7 is None:
        prob_e7 = rng.integers(0, 4, size=len(y)) * 2500000 + rng.integers(0, 2, size=len(y))   # few values: many ties
    if path is AUTO:
        path = []
        for e in range(n_events):
            at = np.flatnonzero(y == e)
            u = rng.random()
            if len(at) and u < 0.8:
                path.append((int(x[rng.choice(at)]), e))
            elif u > 0.93:
                path.append((7, e))                                   # a pair whose cell holds no record
        path = np.array(path, dtype=np.int32).reshape(-1, 2)
    return dict(raw_start=raw_start, raw_length=lengths, n_events=int(n_events), n_samples=n_samples, ref_first=int(ref_first),
                ref_step=int(ref_step), base_shift=int(base_shift), x=x, y=y, kmer_id=rng.integers(0, 4096, size=len(y)).astype(np.int32),
                prob_e7=np.asarray(prob_e7, dtype=np.int64), path=path)


def _diagonal(rng, n_records, **kw):
    """records ordered by x + y as a batch leaves them: three per event on neighbouring x, so equal events lie apart"""
    n_events = (n_records + 2) // 3
    x = np.repeat(np.arange(n_events), 3)[:n_records] + np.tile([0, 1, 2], n_events)[:n_records]
    y = np.repeat(np.arange(n_events), 3)[:n_records]
    order = np.argsort(x + y, kind="stable")
    return _job(rng, n_events, y[order], x=200 + x[order], **kw)


def _shape_jobs():
    rng = np.random.default_rng(23)
    ev = lambda n_events, n: np.sort(rng.integers(0, n_events, size=n))
    jobs = [
        _job(rng, 1, [0], lengths=[1], gaps=[0]),                                        # one event, one record, one sample
        _job(rng, 40, ev(40, 60)),
        _job(rng, 40, [], x=[]),                                                         # no record, among jobs that have them
        _diagonal(rng, 63), _diagonal(rng, 64), _diagonal(rng, 65),                      # the wave boundary
        _diagonal(rng, 4095), _diagonal(rng, 4096), _diagonal(rng, 4097),                # SA_CHAIN_CHUNK
        _job(rng, 9, [4] * 300, x=100 + rng.integers(0, 5, size=300), path=np.array([(102, 4)], dtype=np.int32)),                # 300 records on one event
        _job(rng, 30, np.clip(ev(30, 50), 1, 28)),                                       # no record at the first and last event
        _job(rng, 50, ev(50, 80), ref_first=90000, ref_step=-1, base_shift=3),           # a descending reference_index
        _job(rng, 20, ev(20, 30), path=np.zeros((0, 2), dtype=np.int32)),                # an empty path
        _job(rng, 20, ev(20, 30), path=None),                                            # a NULL path
        _job(rng, 20, ev(20, 30), path=np.array([(7, 3), (7, 9)], dtype=np.int32)),      # a path without any record
        _job(rng, 30, ev(30, 60), lead=700, tail=900),                                   # samples before the first and after the last segment
    ]
    for n_samples in (TILE - 1, TILE, TILE + 1):                                         # the fill's tile
        lengths = np.full(400, 10)
        lengths[-1] = n_samples - 10 * 399
        jobs.append(_job(rng, 400, ev(400, 700), lengths=lengths, gaps=np.zeros(400)))
        assert jobs[-1]["n_samples"] == n_samples
    lengths = rng.integers(1, 12, size=60)
    lengths[20] = 2 * TILE + 77                                                          # a segment longer than two tiles
    jobs.append(_job(rng, 60, np.arange(60).repeat(2), lengths=lengths, lead=TILE - 40))
    gaps = np.zeros(60)
    gaps[30] = 3 * TILE                                                                  # unmapped: tiles in which no segment starts
    jobs.append(_job(rng, 60, np.arange(60).repeat(2), gaps=gaps))
    jobs.append(_job(rng, 10, [0, 0, 0, 5, 5, 5, 5], x=[50, 50, 50, 60, 60, 61, 60], prob_e7=[9, 4, 4, 3, 2, 1, 2],
                     path=np.array([(50, 0), (60, 5)], dtype=np.int32)))                 # three records in a cell, two tied for lowest
    jobs.append(_job(rng, 10, [2, 3], x=[0, (1 << 20) + 5], prob_e7=[0, 10 ** 7]))       # far apart x; prob_e7 of 0 and of 1e7
    return jobs


_SHARED = {}


def _call_arrays(jobs):
    first = np.concatenate([[0], np.cumsum([len(j["x"]) for j in jobs])]).astype(np.int64)
    cat = lambda f, dt: np.concatenate([np.asarray(j[f], dtype=dt) for j in jobs]) if jobs else np.zeros(0, dtype=dt)
    return first, cat("x", np.int32), cat("y", np.int32), cat("kmer_id", np.int32), cat("prob_e7", np.int64)


def _expected(jobs, want_mea=True, want_bands=True):
    return [ref.labels(j, j["x"], j["y"], j["kmer_id"], j["prob_e7"], j["path"], want_mea=want_mea, want_bands=want_bands) for j in jobs]


def _shapes():
    if not _SHARED:
        _SHARED["jobs"] = _shape_jobs()
        _SHARED["exp"] = _expected(_SHARED["jobs"])
    return _SHARED["jobs"], _SHARED["exp"]


def _check(got, exp, flags=ALL):
    reads = got["reads"]
    assert len(reads) == len(exp)
    for f in ref.READ_FIELDS:
        assert reads[f].tolist() == [e["read"][f] for e in exp], f
    for first, count in (("mea_first", "n_mea"), ("full_first", "n_full"), ("band_first", "n_bands"), ("sample_first", "n_samples")):
        assert reads[first].tolist() == np.concatenate([[0], np.cumsum(reads[count])[:-1]]).astype(np.int64).tolist(), first
    for j, e in enumerate(exp):
        if flags & sa.LABEL_MEA:
            assert ref.as_tuples(got["mea"][j], ref.SEGMENT_FIELDS) == e["mea"], j
        if flags & sa.LABEL_FULL:
            assert ref.as_tuples(got["full"][j], ref.SEGMENT_FIELDS) == e["full"], j
        if flags & sa.LABEL_BANDS:
            assert ref.as_tuples(got["bands"][j], ref.BAND_FIELDS) == e["bands"], j
        if flags & sa.LABEL_SAMPLES:
            assert got["samples"][j].dtype == np.int32 and np.array_equal(got["samples"][j], e["samples"]), j


def _run(jobs, flags=ALL, **kw):
    return sa.signal_labels_records(jobs, *_call_arrays(jobs), mea=[j["path"] for j in jobs], flags=flags, **kw)


def test_every_set_equals_the_restatement_on_the_edge_shapes():
    jobs, exp = _shapes()
    # the shapes are what they are meant to be
    assert [len(j["x"]) for j in jobs[3:9]] == [63, 64, 65, 4095, 4096, 4097] and len(jobs[2]["x"]) == 0
    assert exp[0]["samples"].tolist() == [0] and exp[0]["read"]["n_mea"] == 1
    assert max(np.bincount(jobs[9]["y"])) == 300 and exp[9]["read"]["n_mea"] == 1
    assert 0 not in jobs[10]["y"] and 29 not in jobs[10]["y"]
    assert exp[11]["read"]["minus_strand"] == 1 and exp[1]["read"]["minus_strand"] == 0
    assert [exp[i]["read"]["status"] for i in (2, 12, 13, 14)] == [ref.NO_RECORDS, ref.NO_PATH, ref.NO_PATH, 0]
    assert exp[14]["read"]["mea_without_record"] == 2 and exp[14]["read"]["n_mea"] == 0 and (exp[14]["samples"] == -1).all()
    assert exp[15]["samples"][0] == -1 and exp[15]["samples"][-1] == -1 and exp[15]["read"]["first_sample"] >= 700
    assert [j["n_samples"] for j in jobs[16:19]] == [TILE - 1, TILE, TILE + 1]
    assert max(np.bincount(exp[19]["samples"][exp[19]["samples"] >= 0])) > 2 * TILE
    s = exp[20]["samples"]
    assert any(len(set(s[t:t + TILE].tolist())) == 1 and s[t] >= 0 for t in range(0, len(s) - TILE, TILE))     # a tile of one segment's gap
    assert [m[6] for m in exp[21]["mea"]] == [0, 0] and [m[5] for m in exp[21]["mea"]] == [int(jobs[21]["kmer_id"][i]) for i in (1, 4)]
    assert sum(e["read"]["mea_without_record"] for e in exp) > 20 and sum(e["read"]["stay_events"] for e in exp) > 50
    assert sum(e["read"]["skipped_positions"] for e in exp) > 5
    got = _run(jobs, ALL | sa.LABEL_TIMES)
    _check(got, exp)
    assert got["kernel_ms"] > 0
    times = sa.signal_labels_last_kernel_ms()
    assert list(times) == list(sa.LABEL_KERNELS) and all(v > 0 for v in times.values())
    again = _run(jobs)
    for f in ("mea", "full", "bands", "samples"):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[f], again[f])), f
    assert got["reads"].tobytes() == again["reads"].tobytes()


def test_each_set_alone_and_no_job_at_all():
    jobs, exp = _shapes()
    got = _run(jobs, sa.LABEL_MEA)
    assert set(got) == {"reads", "kernel_ms", "mea"}
    no_bands = _expected(jobs, want_bands=False)
    _check(got, no_bands, sa.LABEL_MEA)
    _check(_run(jobs, sa.LABEL_MEA | sa.LABEL_SAMPLES), no_bands, sa.LABEL_MEA | sa.LABEL_SAMPLES)
    _check(_run(jobs, sa.LABEL_FULL), _expected(jobs, want_mea=False, want_bands=False), sa.LABEL_FULL)
    _check(_run(jobs, sa.LABEL_BANDS), _expected(jobs, want_mea=False), sa.LABEL_BANDS)
    # without any path: SA_LABEL_NO_PATH wherever there are records
    got = sa.signal_labels_records(jobs, *_call_arrays(jobs), mea=None, flags=ALL)
    _check(got, [ref.labels(j, j["x"], j["y"], j["kmer_id"], j["prob_e7"], None) for j in jobs])
    none = sa.signal_labels_records([], [0], [], [], [], [], flags=ALL)
    assert len(none["reads"]) == 0 and all(none[f] == [] for f in ("mea", "full", "bands", "samples"))
    sa.signal_labels_release()


@pytest.mark.parametrize("n_jobs", [1, 257])
def test_one_job_and_many_jobs_in_a_call(n_jobs):
    rng = np.random.default_rng(100 + n_jobs)
    jobs = []
    for i in range(n_jobs):
        n_events = int(rng.integers(1, 40))
        n = 0 if i % 50 == 7 else int(rng.integers(1, 70))
        jobs.append(_job(rng, n_events, np.sort(rng.integers(0, n_events, size=n)), ref_step=1 if i % 3 else -1, ref_first=5000 + i))
    _check(_run(jobs), _expected(jobs))


def test_refusals_on_the_device_side():
    jobs, _ = _shapes()
    with pytest.raises(sa.SaError) as e:
        _run(jobs[:2], device=99)
    assert e.value.code == -1                                                    # a device outside [0, count)
    with pytest.raises(sa.SaError) as e:
        _run(jobs[:2], flags=sa.LABEL_SAMPLES)
    assert e.value.code == -1


# ---- chained onto a real batch ------------------------------------------------------------------------------------------------
def _batch(jobs, flags=0, run=True, model=cases.MODEL_6MER, ambig=None):
    b = sa.Batch(sa.Model.load(model), sa.default_params(), jobs, flags=flags, ambig=ambig)
    if run:
        b.run()
    return b


def _label_jobs(jobs, rng):
    out = []
    for i, j in enumerate(jobs):
        n_events = len(j["events"])
        lengths = rng.integers(3, 15, size=n_events)
        raw_start = 50 + np.concatenate([[0], np.cumsum(lengths)[:-1]])
        out.append(dict(raw_start=raw_start, raw_length=lengths, n_events=n_events, n_samples=int(raw_start[-1] + lengths[-1] + 30),
                        ref_first=10000 * (i + 1), ref_step=-1 if i == 1 else 1, base_shift=3 if i == 1 else 2))
    return out


def test_chained_onto_a_batch_equals_the_records_of_its_pairs():
    # two plain reads and one with ambiguity letters at its CpGs, so that its cells hold several paths
    jobs = cases.synthetic_jobs(cases.MODEL_CPG, 2, 400, 720) + cases.synthetic_jobs(cases.MODEL_CPG, 1, 400, 722, cpg_ambiguous=True)
    b = _batch(jobs, model=cases.MODEL_CPG, ambig=sa.default_ambig({"X": "CE"}))
    paths = [m[0] for m in b.mea()]
    assert all(len(m) > 200 for m in paths)
    rows, first = b.pairs_all()
    cells = list(zip(rows["x"][first[2]:first[3]].tolist(), rows["y"][first[2]:first[3]].tolist()))
    assert len(cells) > len(set(cells))                                          # several records in one cell
    ljobs = _label_jobs(jobs, np.random.default_rng(5))
    exp = [ref.labels(ljobs[j], *(rows[f][first[j]:first[j + 1]] for f in ("x", "y", "kmer_id", "prob_e7")), paths[j]) for j in range(3)]
    assert all(e["read"]["n_mea"] > 200 and e["read"]["mea_without_record"] == 0 for e in exp)
    assert exp[1]["read"]["minus_strand"] == 1 and exp[0]["read"]["minus_strand"] == 0
    from_records = sa.signal_labels_records(ljobs, first, rows["x"], rows["y"], rows["kmer_id"], rows["prob_e7"], mea=paths, flags=ALL)
    _check(from_records, exp)
    got = sa.batch_signal_labels(b, ljobs, mea=b.mea(), flags=ALL)
    _check(got, exp)
    b.release_device()                                                           # the records go up again
    again = sa.batch_signal_labels(b, ljobs, mea=paths, flags=ALL)
    _check(again, exp)
    assert again["reads"].tobytes() == got["reads"].tobytes()
    # not the batch's number of jobs, not the batch's n_events
    for bad in (ljobs[:2], [ljobs[0], ljobs[1], dict(ljobs[2], raw_start=ljobs[2]["raw_start"][:-1], raw_length=ljobs[2]["raw_length"][:-1],
                                                      n_events=ljobs[2]["n_events"] - 1)]):
        with pytest.raises(sa.SaError) as e:
            sa.batch_signal_labels(b, bad, flags=sa.LABEL_FULL)
        assert e.value.code == -1
    b.close()


def test_batches_that_are_refused():
    jobs = cases.realistic_anchor_jobs(cases.MODEL_6MER, 2, 200, 730)
    ljobs = _label_jobs(jobs, np.random.default_rng(6))

    def refused(b, code):
        with pytest.raises(sa.SaError) as e:
            sa.batch_signal_labels(b, ljobs, flags=sa.LABEL_FULL)
        assert e.value.code == code

    b = _batch(jobs, run=False)
    refused(b, -7)                                                               # SA_ESTATE: not run
    b.run()
    assert sa.batch_signal_labels(b, ljobs, flags=sa.LABEL_FULL)["reads"]["n_full"].min() > 100
    b.close()
    b = _batch(jobs, sa.FLAG_PAIRS8)
    refused(b, -7)                                                               # SA_ESTATE: 8-byte records name no k-mer
    b.close()
