"""signalMachine with a read given as raw current: -q names a raw-read file (signalalign_amd/rawio.py), the events come from
sa_npread_from_raw_batch, and the .npRead the run writes with --npread-out gives the same bytes when a second run reads it
back with -q -- alone and in a manifest, where a read whose sequence does not belong to its signal fails alone."""
import os
import subprocess

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import rawio

import guide_ref as g
import raw_npread_ref as N
from test_gpu_cli_guide import BIN, MODEL, PRE, _contig, _write_fasta
from test_gpu_event_detect import job_of
from test_host_event_detect import dna_sequence

pytestmark = pytest.mark.gpu


def _run(argv):
    return subprocess.run(argv, capture_output=True, text=True, timeout=300)


def _argv(read, fasta, out, label, *more):
    return [BIN, "-T", MODEL, "-q", read, "-f", fasta, "-u", out, "-L", label, "-x", "50", "-D", "0.01", "-m", "14", "-g", "100",
            "-s", "0"] + list(more)


@pytest.fixture(scope="module")
def raw_run(tmp_path_factory):
    """read 108 as a raw-read file through signalMachine once, with the window of r9p4_oneD's bundled guide"""
    d = tmp_path_factory.mktemp("raw_cli")
    _, window = g.ecoli_pair()
    fasta = str(d / "ref.fa")
    _write_fasta(fasta, "chrE", _contig(window))
    spec = "chrE:%d-%d" % (PRE - 50, PRE + len(window) + 100)
    raw = str(d / "read108.saraw")
    rawio.write_raw(raw, sequence=dna_sequence(), **job_of("read108_dna"))
    out = str(d / "a.tsv")
    pr = _run(_argv(raw, fasta, out, "read108", "--guide-window", spec, "--npread-out", str(d / "np")))
    assert pr.returncode == 0, pr.stderr
    assert "NOTICE: read108 from raw current: 56345 samples, 11020 events on 6542 bases" in pr.stderr
    assert "signalAlign - SUCCESS: finished alignment of query read108, exiting" in pr.stderr
    return d, fasta, spec, raw, open(out, "rb").read(), pr.stdout


def test_raw_read_and_the_npread_it_wrote_give_the_same_bytes(raw_run, tmp_path):
    d, fasta, spec, raw, tsv, stdout = raw_run
    assert len(tsv) > 100000
    written = d / "np" / "read108.npRead"
    chain = sa.raw_event_align_batch(sa.Model.load(MODEL), [job_of("read108_dna")], [dna_sequence()])[0]
    assert written.read_bytes() == N.npread_text(dna_sequence(), N.mapped_rows(chain["events"]), 5).encode()
    out = str(tmp_path / "b.tsv")
    pr = _run(_argv(str(written), fasta, out, "read108", "--guide-window", spec))     # sa_npread_load accepts the file
    assert pr.returncode == 0, pr.stderr
    assert "from raw current" not in pr.stderr
    assert open(out, "rb").read() == tsv and pr.stdout == stdout


def test_manifest_mixes_raw_reads_and_npreads_and_a_foreign_sequence_fails_alone(raw_run, tmp_path):
    d, fasta, spec, raw, tsv, _ = raw_run
    rng = np.random.default_rng(11)
    foreign = str(tmp_path / "foreign.saraw")
    rawio.write_raw(foreign, sequence="".join(rng.choice(list("ACGT"), 200)), **job_of("read108_dna"))
    lines = [("fromraw", raw, "@" + spec, str(tmp_path / "fromraw.tsv")),
             ("fromnp", str(d / "np" / "read108.npRead"), "@" + spec, str(tmp_path / "fromnp.tsv")),
             ("foreign", foreign, "@" + spec, str(tmp_path / "foreign.tsv"))]
    manifest = str(tmp_path / "manifest.tsv")
    with open(manifest, "w") as f:
        for row in lines:
            f.write("\t".join(row) + "\n")
    pr = _run([BIN, "-T", MODEL, "-f", fasta, "-x", "50", "-D", "0.01", "-m", "14", "-g", "100", "-s", "0", "--batch", manifest])
    assert pr.returncode == 1, pr.stderr                      # one read failed: as any batch with a skipped read
    assert "read foreign skipped" in pr.stderr
    assert "no event table for the raw read" in pr.stderr.split("read foreign skipped")[1].split("\n")[0]
    assert "batch: 2 of 3 reads aligned" in pr.stderr
    assert "finished alignment of query foreign," not in pr.stderr and not os.path.exists(str(tmp_path / "foreign.tsv"))
    relabel = lambda path, label: open(path, "rb").read().replace(b"\t" + label + b"\t", b"\tread108\t")
    assert relabel(str(tmp_path / "fromraw.tsv"), b"fromraw") == tsv
    assert relabel(str(tmp_path / "fromnp.tsv"), b"fromnp") == tsv


@pytest.mark.parametrize("more, word", [(("--twoD", "-C", MODEL), "--twoD"), (("--rna",), "--rna"), (("-C", MODEL), "complement")])
def test_raw_read_refusals_come_before_any_gpu_work(raw_run, tmp_path, more, word):
    d, fasta, spec, raw, _, _ = raw_run
    out = str(tmp_path / "o.tsv")
    pr = _run(_argv(raw, fasta, out, "r", "-p", str(tmp_path / "none.cigar"), "-n", "chrE", *more))
    assert pr.returncode != 0 and not os.path.exists(out)
    err = [l for l in pr.stderr.split("\n") if l.strip()]
    assert len(err) == 1 and "a raw read" in err[0] and word in err[0], pr.stderr


def test_raw_detector_option(raw_run, tmp_path):
    d, fasta, spec, raw, tsv, _ = raw_run
    pr = _run(_argv(raw, fasta, str(tmp_path / "o.tsv"), "r", "--guide-window", spec, "--raw-detector", "3,6,1.4,9.0"))
    assert pr.returncode != 0 and "--raw-detector takes w1,w2,t1,t2,peak" in pr.stderr
    # the defaults spelled out: the same bytes
    out = str(tmp_path / "same.tsv")
    pr = _run(_argv(raw, fasta, out, "read108", "--guide-window", spec, "--raw-detector", "3,6,1.4,9.0,0.2"))
    assert pr.returncode == 0, pr.stderr
    assert open(out, "rb").read() == tsv
