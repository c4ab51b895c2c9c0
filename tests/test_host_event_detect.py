"""The raw-current front end's CPU restatement (tests/event_detect_ref.py) chained into the existing CPU oracle reproduces
the reference's own literals for detect_events and load_from_raw2 (tests/eventAlignerTests.c of the reference), on the
raw reads under tests/golden/raw/.  This pins the restatement, which tests/test_gpu_event_detect.py then holds the GPU
to bit for bit, as test_oracle_kats.py does for the pair-HMM."""
import os

import numpy as np
import pytest

import event_detect_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RNA_MODEL = os.path.join(GOLDEN, "models", "testModelR9p4_5mer_acgt_RNA.model")
DNA_MODEL = os.path.join(GOLDEN, "models", "testModelR9p4_5mer_acegt_template.model")


def fixture(name):
    return np.load(os.path.join(GOLDEN, "raw", name + ".npz"))


def rna_sequence():
    return open(os.path.join(GOLDEN, "raw", "rna_8898d755.txt")).read().strip()


def dna_sequence():
    return open(os.path.join(GOLDEN, "npReads", "r9p4_oneD.npRead")).read().split("\n")[2].strip()


def test_fixtures_hold_the_reads_the_reference_tests_read():
    # test_fast5_get_raw_samples (:107-121) and test_fast5_get_start_time (:123-128), read 61
    f = fixture("read61_rna")
    a = R.attrs_of(f)
    pa = R.raw_to_pa(f["raw"], **a)
    assert len(pa) == 25794
    assert abs(float(pa[0]) - 93.797729) < 1e-4 and abs(float(pa[1]) - 94.230644) < 1e-4
    assert int(a["start_time"]) == 232505
    assert str(f["read_id"]).startswith("8898d755")
    assert str(fixture("read108_dna")["read_id"]).startswith("6deaf971") and len(fixture("read108_dna")["raw"]) == 56345
    assert len(fixture("read1108_dna")["raw"]) == 70346
    assert len(rna_sequence()) == 458 and rna_sequence().startswith("CAUCCUGCCC")
    assert dna_sequence().startswith("TGCATGCCGTTTCCG")


def test_event_table_to_basecalled_table_literals():
    # test_event_table_to_basecalled_table (:131-150): RNA parameters, event[1]
    f = fixture("read61_rna")
    a = R.attrs_of(f)
    b = R.basecalled_table(R.detect_events(R.raw_to_pa(f["raw"], **a), R.RNA), **a)
    e = b[1]
    assert e["raw_start"] == 7 and e["raw_length"] == 15
    assert abs(e["mean"] - 87.082771) < 1e-3 and abs(e["stdv"] - 1.637721) < 1e-3
    assert abs(e["start"] - 77.195221) < 1e-4 and abs(e["length"] - 0.004980) < 1e-4


def _chain(oracle, name, model_path, seq, rna):
    f = fixture(name)
    a = R.attrs_of(f)
    ev = R.detect_events(R.raw_to_pa(f["raw"], **a), R.RNA if rna else R.DEFAULTS)
    al = ev[::-1] if rna else ev
    om = oracle.Model.from_file(model_path)
    ids = oracle.kmer_ids_of(om, seq, rna=rna)
    shift, scale = oracle.scalings_mom(om, al["mean"].astype(np.float64), ids)
    om.set_read_params(scale, shift, 1.0)
    k, e, st = oracle.event_align(om, al["mean"].astype(np.float64), ids)
    km, mv = R.base_event_map(k, e, len(ev), len(ids), rna)
    if rna:
        km, mv = km[::-1], mv[::-1]
    return dict(events=ev, shift=shift, scale=scale, k=k, e=e, status=st, km=km, kmers=R.kmer_strings(seq, om.k, rna))


def test_rna_chain_literals(oracle):
    c = _chain(oracle, "read61_rna", RNA_MODEL, rna_sequence(), True)
    # test_estimate_scalings_using_mom (:320-345)
    assert abs(c["scale"] - 1.016111) < 1e-4 and abs(c["shift"] - 20.720264) < 1e-4
    # test_adaptive_banded_simple_event_align (:404-433): the last pair of the (reversed-event) alignment
    assert c["status"] == 0 and (c["k"][-1], c["e"][-1]) == (453, 1219)
    # test_load_from_raw_rna (:436-466): 1220 events written, first AACCT, last CCTAC
    mapped = np.nonzero(c["km"] >= 0)[0]
    assert len(mapped) == 1220
    assert c["kmers"][c["km"][mapped[0]]] == "AACCT" and c["kmers"][c["km"][mapped[-1]]] == "CCTAC"


def test_dna_chain_literals(oracle):
    # test_load_from_raw_dna (:468-490): read 108, 11020 events written, first TGCAT, last AAACT
    c = _chain(oracle, "read108_dna", DNA_MODEL, dna_sequence(), False)
    assert len(c["events"]) == 11100 and c["status"] == 0
    mapped = np.nonzero(c["km"] >= 0)[0]
    assert len(mapped) == 11020
    assert c["kmers"][c["km"][mapped[0]]] == "TGCAT" and c["kmers"][c["km"][mapped[-1]]] == "AAACT"


def test_no_peak_and_short_reads():
    # the departure from undefined behaviour: no peak -> one event spanning the read
    for n in (1, 2, 5, 13, 200):
        ev = R.detect_events(np.full(n, 80.0, dtype=np.float32))
        assert len(ev) == 1 and ev["start"][0] == 0 and ev["length"][0] == n
        assert ev["mean"][0] == np.float32(80.0) and ev["stdv"][0] == 0
    with pytest.raises(ValueError):
        R.detect_events(np.zeros(0, dtype=np.float32))
