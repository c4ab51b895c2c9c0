"""Raw current -> the in-memory .npRead of a 1D read (sa_npread_from_raw_batch, k_raw_finish in sa_detect.hip).  The rows are
held bit for bit to the mapped rows of sa_raw_event_align_batch on the same input (whose detector and event aligner
tests/test_gpu_event_detect.py pins), the strand event map and the written file to the restatement tests/raw_npread_ref.py."""
import numpy as np
import pytest

import signalalign_amd as sa

import raw_npread_ref as N
from test_host_event_detect import DNA_MODEL, dna_sequence
from test_gpu_event_detect import job_of

pytestmark = pytest.mark.gpu

K = 5


@pytest.fixture(scope="module")
def model():
    return sa.Model.load(DNA_MODEL)


@pytest.fixture(scope="module")
def full(model):
    """read 108 through the existing chain, once"""
    job, seq = job_of("read108_dna"), dna_sequence()
    return job, seq, sa.raw_event_align_batch(model, [job], [seq])[0]


def assert_rows_equal_chain(got, chain, what):
    """got: one read of npread_from_raw_batch with status 0; chain: the same read of raw_event_align_batch"""
    rows = N.mapped_rows(chain["events"])
    assert got["status"] == 0 and chain["status"] == 0, what
    assert got["n_events"] == len(rows) and got["events4"].shape == (len(rows), 4), (what, got["n_events"], len(rows))
    exp4 = N.events4_of(rows)
    for c, name in enumerate(("mean", "stdv", "length", "start - start0")):
        g, e = np.ascontiguousarray(got["events4"][:, c]).view(np.uint64), np.ascontiguousarray(exp4[:, c]).view(np.uint64)
        assert np.array_equal(g, e), (what, name, int(np.argmax(g != e)))
    for f in ("kmer_idx", "move", "raw_start", "raw_length"):
        assert np.array_equal(got[f], rows[f]), (what, f)
    assert np.array_equal(got["p_model_state"].view(np.uint64), rows["p_model_state"].view(np.uint64)), what
    assert (got["shift"], got["scale"]) == (chain["shift"], chain["scale"]), what
    exp_map = N.make_event_map(rows["move"], rows["p_model_state"], K)
    assert got["read_len"] == len(exp_map) and np.array_equal(got["strand_event_map"], exp_map), what


def same_read(a, b):
    if a["status"] != b["status"] or a["status"] != 0:
        return a["status"] == b["status"]
    return all(np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8))
               for f in ("events4", "kmer_idx", "move", "p_model_state", "raw_start", "raw_length", "strand_event_map"))


def prefix_of(full, n_samples):
    """the first n_samples of read 108 with the bases its own base-to-event map places in them: up to the last k-mer of an
    event that ends inside the prefix"""
    job, seq, chain = full
    ev = chain["events"]
    inside = (ev["raw_start"] + ev["raw_length"] <= n_samples) & (ev["kmer_idx"] >= 0)
    return dict(job, raw=job["raw"][:n_samples]), seq[:int(ev["kmer_idx"][inside].max()) + K]


def test_read108_rows_map_and_reference_literals(model, full):
    job, seq, chain = full
    st = {}
    got = sa.npread_from_raw_batch(model, [job], [seq], stats=st)[0]
    assert_rows_equal_chain(got, chain, "read108")
    # test_load_from_raw_dna (tests/eventAlignerTests.c:468-490): 11020 rows written, first TGCAT, last AAACT
    assert got["n_events"] == 11020
    assert seq[got["kmer_idx"][0]:][:K] == "TGCAT" and seq[got["kmer_idx"][-1]:][:K] == "AAACT"
    assert len(got["strand_event_map"]) == 6542 == len(seq)
    assert got["events4"][0, 3] == 0.0 and (np.diff(got["events4"][:, 3]) > 0).all()
    assert st["kernel_ms"] > st["finish_ms"] > 0


def test_edge_batch_fails_reads_alone_and_matches_the_chain(model, full):
    job, seq, _ = full
    rng = np.random.default_rng(20240)
    reads = [prefix_of(full, 2000), prefix_of(full, 4096), prefix_of(full, 4097),
             (dict(job, raw=job["raw"][:1]), seq[:20]),                               # one sample: one event, no peak
             (dict(raw=np.full(5000, 80, dtype=np.int16), digitisation=8192.0, offset=0.0, range=8192.0, sample_rate=4000.0,
                   start_time=1234.0), seq[:50]),                                      # constant current: flat to the detector
             (job, "".join(rng.choice(list("ACGT"), 200)))]                          # a sequence the signal does not belong to
    # a failed read between good ones: the prefixes again behind the rejects
    reads += reads[:3]
    jobs, seqs = [r[0] for r in reads], [r[1] for r in reads]
    chain = sa.raw_event_align_batch(model, jobs, seqs)
    got = sa.npread_from_raw_batch(model, jobs, seqs)
    n_ok = 0
    for j, (g, c) in enumerate(zip(got, chain)):
        assert g["status"] == c["status"], (j, g["status"], c["status"])
        assert g["read_len"] == len(seqs[j])
        if g["status"] == 0:
            n_ok += 1
            assert_rows_equal_chain(g, c, j)
        else:
            assert g["n_events"] == 0
            assert all(g[f] is None for f in ("events4", "kmer_idx", "move", "p_model_state", "raw_start", "raw_length",
                                              "strand_event_map")), j
    # the three prefixes pass under the existing chain (checked with event_detect_ref.py + the oracle on the CPU: status 0 at
    # 2000, 4096 and 4097 samples with 202, 433 and 433 bases); the other three do not
    assert [g["status"] == 0 for g in got] == [True] * 3 + [False] * 3 + [True] * 3 and n_ok == 6
    assert got[3]["status"] & sa.RAW_NO_PEAK and got[4]["status"] & sa.RAW_NO_PEAK
    assert got[5]["status"] != 0 and not got[5]["status"] & sa.RAW_NO_PEAK
    # the neighbours of the failed reads are what they are alone
    for j in (0, 1, 2):
        alone = sa.npread_from_raw_batch(model, [jobs[j]], [seqs[j]])[0]
        assert same_read(alone, got[j]) and same_read(alone, got[j + 6]), j


def test_many_reads_per_launch(model, full):
    job, seq = prefix_of(full, 2000)
    alone = sa.npread_from_raw_batch(model, [job], [seq])[0]
    assert alone["status"] == 0 and alone["n_events"] > 64
    got = sa.npread_from_raw_batch(model, [job] * 130, [seq] * 130)
    assert len(got) == 130
    for j, g in enumerate(got):
        assert same_read(alone, g), j


def test_writer_equals_the_restatement(model, full, tmp_path):
    job, seq, chain = full
    path = tmp_path / "read108.npRead"
    got = sa.npread_from_raw_batch(model, [job], [seq], write=[str(path)])[0]
    assert got["status"] == 0
    text = N.npread_text(seq, N.mapped_rows(chain["events"]), K)
    assert path.read_bytes() == text.encode()
    assert text.count("\n") == 14


def test_custom_detector_parameters_reach_the_detector(model, full):
    job, seq, _ = full
    params = (4, 9, 2.0, 8.0, 0.5)
    got = sa.npread_from_raw_batch(model, [job], [seq], params=params)[0]
    chain = sa.raw_event_align_batch(model, [job], [seq], params=params)[0]
    assert got["status"] == chain["status"]
    if got["status"] == 0:
        assert_rows_equal_chain(got, chain, "custom")
