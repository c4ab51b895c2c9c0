"""signalMachine with a guide window instead of a cigar file: the guide alignment is computed on the GPU (sa_guide_align_batch),
written out on request, and a second run that reads it back with -p produces the same bytes."""
import os
import subprocess

import numpy as np
import pytest

import signalalign_amd as sa

import guide_ref as g
import sa_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
MODEL = os.path.join(cases.GOLDEN, "models", "testModelR9p4_5mer_acegt_template.model")
NPREAD = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")
PRE, POST = 300, 200          # unrelated bases around the window inside the contig


def _write_fasta(path, name, seq, width=60):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for i in range(0, len(seq), width):
            f.write(seq[i:i + width] + "\n")
    with open(path + ".fai", "w") as f:
        f.write("%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), len(name) + 2, width, width + 1))


def _contig(window, seed=3):
    rng = np.random.default_rng(seed)
    pre = "".join("ACGT"[i] for i in rng.integers(0, 4, PRE))
    post = "".join("ACGT"[i] for i in rng.integers(0, 4, POST))
    return pre + window + post


def _argv(fasta, out, label, *more):
    return [BIN, "-T", MODEL, "-q", NPREAD, "-f", fasta, "-u", out, "-L", label, "-x", "50", "-D", "0.01", "-m", "14", "-g", "100",
            "-s", "0"] + list(more)


def _run(argv):
    return subprocess.run(argv, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def plus_run(tmp_path_factory):
    """one run with --guide-window on the plus strand, shared: (directory, fasta, TSV bytes, loaded cigar)"""
    d = tmp_path_factory.mktemp("guide_plus")
    read, window = g.ecoli_pair()
    fasta = str(d / "ref.fa")
    _write_fasta(fasta, "chrE", _contig(window))
    out = str(d / "out.tsv")
    spec = "chrE:%d-%d" % (PRE - 50, PRE + len(window) + 100)
    pr = _run(_argv(fasta, out, "read1", "--guide-window", spec, "--guide-cigars-out", str(d / "cigars")))
    assert pr.returncode == 0, pr.stderr
    assert "NOTICE: Guide alignment computed on the GPU inside " + spec in pr.stderr
    assert "signalAlign - SUCCESS: finished alignment of query read1, exiting" in pr.stderr
    return d, fasta, open(out, "rb").read(), sa.cigar_load(str(d / "cigars" / "read1.cigar")), pr.stdout


def test_guide_window_then_the_written_cigar_gives_the_same_bytes(plus_run, tmp_path):
    d, fasta, tsv, cig, stdout = plus_run
    read, window = g.ecoli_pair()
    lib = sa.guide_align_batch([(read, window)])[0]
    assert (cig["contig1"], cig["contig2"], cig["strand1"], cig["strand2"]) == ("chrE", "read1", 1, 1)
    assert (cig["start2"], cig["end2"]) == (lib["read_start"], lib["read_end"]) == (42, lib["read_end"])
    assert (cig["start1"], cig["end1"]) == (PRE + lib["ref_start"], PRE + lib["ref_end"]) and cig["score"] == lib["score"]
    assert len(tsv) > 100000
    out2 = str(tmp_path / "out2.tsv")
    pr = _run(_argv(fasta, out2, "read1", "-p", str(d / "cigars" / "read1.cigar"), "-n", "chrE"))
    assert pr.returncode == 0, pr.stderr
    assert open(out2, "rb").read() == tsv and pr.stdout == stdout
    # both at once is refused
    pr = _run(_argv(fasta, out2, "read1", "-p", str(d / "cigars" / "read1.cigar"), "--guide-window", "chrE:0-100"))
    assert pr.returncode != 0 and "exclude each other" in pr.stderr


@pytest.mark.parametrize("told", [False, True])
def test_minus_strand_mirrors_the_coordinates_and_keeps_the_operations(plus_run, tmp_path, told):
    """the plus run's contig reverse-complemented, the mirrored window: the same alignment, on the minus strand"""
    _, _, _, cig_plus, _ = plus_run
    read, window = g.ecoli_pair()
    contig = g.reverse_complement(_contig(window))
    total = len(contig)
    fasta = str(tmp_path / "ref.fa")
    _write_fasta(fasta, "chrM", contig)
    out = str(tmp_path / "out.tsv")
    spec = "chrM:%d-%d" % (total - (PRE + len(window) + 100), total - (PRE - 50)) + (":-" if told else "")
    pr = _run(_argv(fasta, out, "readm", "--guide-window", spec, "--guide-cigars-out", str(tmp_path / "c")))
    assert pr.returncode == 0, pr.stderr
    cig = sa.cigar_load(str(tmp_path / "c" / "readm.cigar"))
    assert cig["strand1"] == 0 and (cig["start1"], cig["end1"]) == (total - cig_plus["start1"], total - cig_plus["end1"])
    assert cig["start1"] > cig["end1"] and cig["score"] == cig_plus["score"]
    assert (cig["start2"], cig["end2"]) == (cig_plus["start2"], cig_plus["end2"]) and cig["ops"] == cig_plus["ops"]
    assert "signalAlign - SUCCESS" in pr.stderr and len(open(out).readlines()) > 10000


def test_manifest_mixes_cigar_files_and_windows_and_a_lost_read_fails_alone(plus_run, tmp_path):
    d, _, tsv, _, _ = plus_run
    read, window = g.ecoli_pair()
    rng = np.random.default_rng(9)
    desert = "".join("ACGT"[i] for i in rng.integers(0, 4, 8000))
    contig = _contig(window) + desert
    fasta = str(tmp_path / "ref.fa")
    _write_fasta(fasta, "chrE", contig)
    elsewhere = PRE + len(window) + POST + 500
    lines = [
        ("win", NPREAD, "@chrE:%d-%d:+" % (PRE - 50, PRE + len(window) + 100), str(tmp_path / "win.tsv")),
        ("lost", NPREAD, "@chrE:%d-%d" % (elsewhere, elsewhere + 7000), str(tmp_path / "lost.tsv")),
        ("file", NPREAD, str(d / "cigars" / "read1.cigar"), str(tmp_path / "file.tsv")),
    ]
    manifest = str(tmp_path / "manifest.tsv")
    with open(manifest, "w") as f:
        f.write("# label\tnpRead\tcigar or @window\tposteriors\n")
        for row in lines:
            f.write("\t".join(row) + "\n")
    argv = [BIN, "-T", MODEL, "-f", fasta, "-x", "50", "-D", "0.01", "-m", "14", "-g", "100", "-s", "0", "--batch", manifest]
    pr = _run(argv)
    assert pr.returncode == 1, pr.stderr                      # one read failed
    assert "read lost skipped" in pr.stderr and "guide alignment" in pr.stderr.split("read lost skipped")[1].split("\n")[0]
    assert "finished alignment of query win," in pr.stderr and "finished alignment of query file," in pr.stderr
    assert "finished alignment of query lost," not in pr.stderr and not os.path.exists(str(tmp_path / "lost.tsv"))
    assert "batch: 2 of 3 reads aligned" in pr.stderr
    relabel = lambda path, label: open(path, "rb").read().replace(b"\t" + label + b"\t", b"\tread1\t")
    assert relabel(str(tmp_path / "win.tsv"), b"win") == tsv
    assert relabel(str(tmp_path / "file.tsv"), b"file") == tsv


def test_rna_with_a_window_dies(plus_run, tmp_path):
    _, fasta, _, _, _ = plus_run
    pr = _run(_argv(fasta, str(tmp_path / "o.tsv"), "r", "--guide-window", "chrE:0-5000", "--rna"))
    assert pr.returncode != 0 and "cannot be combined with --rna" in pr.stderr and not os.path.exists(str(tmp_path / "o.tsv"))
