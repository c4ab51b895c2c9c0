"""signalMachine --guide-locate: the read is located in the whole -f reference on the GPU (sa_guide_locate_batch), the window that
gives goes through the guide stage unchanged, and runs with that window or with the written cigar produce the same bytes."""
import os
import re
import subprocess

import numpy as np
import pytest

import signalalign_amd as sa

import guide_ref as g
import locate_ref as L
import sa_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
MODEL = os.path.join(cases.GOLDEN, "models", "testModelR9p4_5mer_acegt_template.model")
NPREAD = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")
COMMON = ["-x", "50", "-D", "0.01", "-m", "14", "-g", "100", "-s", "0"]


def _run(argv):
    return subprocess.run(argv, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    """the shared reference as a FASTA with its .fai"""
    d = tmp_path_factory.mktemp("locate_ref")
    path, width, off = str(d / "ref.fa"), 60, 0
    with open(path, "w") as f, open(path + ".fai", "w") as fai:
        for name, s in zip(L.NAMES, L.shared_reference()):
            head = ">%s\n" % name
            f.write(head)
            off += len(head)
            fai.write("%s\t%d\t%d\t%d\t%d\n" % (name, len(s), off, width, width + 1))
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + "\n")
            off += len(s) + (len(s) + width - 1) // width
    return path


def _argv(fasta, out, label, *more):
    return [BIN, "-T", MODEL, "-q", NPREAD, "-f", fasta, "-u", out, "-L", label] + COMMON + list(more)


def test_locate_then_its_window_then_its_cigar_give_the_same_bytes(fasta, tmp_path):
    out = str(tmp_path / "out.tsv")
    pr = _run(_argv(fasta, out, "read1", "--guide-locate", "--guide-cigars-out", str(tmp_path / "cigars")))
    assert pr.returncode == 0, pr.stderr
    m = re.search(r"NOTICE: Read located at (\S+) \((\d+) votes, next (\d+)\)", pr.stderr)
    assert m, pr.stderr
    spec = m.group(1)
    read, _ = g.ecoli_pair()
    exp = L.located(read)
    a, b = L.window(L.shared_index(), exp, len(read), 128)
    assert spec == "%s:%d-%d:+" % (L.NAMES[0], a, b) and (int(m.group(2)), int(m.group(3))) == (exp["votes"], exp["second_votes"])
    assert "NOTICE: Guide alignment computed on the GPU inside " + spec in pr.stderr and "is ambiguous" not in pr.stderr and "(overflow)" not in pr.stderr
    assert "signalAlign - SUCCESS: finished alignment of query read1, exiting" in pr.stderr
    tsv = open(out, "rb").read()
    assert len(tsv) > 100000
    # the same window named by hand
    out2 = str(tmp_path / "out2.tsv")
    pr2 = _run(_argv(fasta, out2, "read1", "--guide-window", spec))
    assert pr2.returncode == 0, pr2.stderr
    assert open(out2, "rb").read() == tsv and pr2.stdout == pr.stdout
    # the written cigar
    cigar = str(tmp_path / "cigars" / "read1.cigar")
    out3 = str(tmp_path / "out3.tsv")
    pr3 = _run(_argv(fasta, out3, "read1", "-p", cigar, "-n", L.NAMES[0]))
    assert pr3.returncode == 0, pr3.stderr
    assert open(out3, "rb").read() == tsv and pr3.stdout == pr.stdout
    cig = sa.cigar_load(cigar)
    assert cig["contig1"] == L.NAMES[0] and cig["strand1"] == 1
    assert L.WINDOW_AT <= cig["start1"] < cig["end1"] <= L.WINDOW_AT + 6817


def test_manifest_of_located_reads_and_one_that_is_nowhere(fasta, tmp_path):
    """@ in the cigar column.  The second read is the first again under another label: a reverse-complemented .npRead needs its
    events and maps mirrored, not only its read line swapped (the minus strand itself is covered by test_gpu_locate.py and by the
    guide stage's own minus-strand case).  The third read's bases are random: it has no location and fails alone."""
    rng = np.random.default_rng(11)
    lines = open(NPREAD).read().split("\n")
    toks = lines[2].split()
    toks[0] = "".join("ACGT"[i] for i in rng.integers(0, 4, len(toks[0])))
    lines[2] = " ".join(toks)
    nowhere = str(tmp_path / "nowhere.npRead")
    with open(nowhere, "w") as f:
        f.write("\n".join(lines))
    rows = [("one", NPREAD, "@", str(tmp_path / "one.tsv")), ("two", NPREAD, "@", str(tmp_path / "two.tsv")),
            ("lost", nowhere, "@", str(tmp_path / "lost.tsv"))]
    manifest = str(tmp_path / "manifest.tsv")
    with open(manifest, "w") as f:
        for row in rows:
            f.write("\t".join(row) + "\n")
    pr = _run([BIN, "-T", MODEL, "-f", fasta] + COMMON + ["--batch", manifest])
    assert pr.returncode == 1, pr.stderr                      # what a manifest with one unreadable cigar gives
    assert pr.stderr.count("NOTICE: Read located at ") == 2 and pr.stderr.count("NOTICE: Indexed ") == 1
    assert "read lost skipped" in pr.stderr and "no location for the read" in pr.stderr.split("read lost skipped")[1].split("\n")[0]
    assert "finished alignment of query one," in pr.stderr and "finished alignment of query two," in pr.stderr
    assert "finished alignment of query lost," not in pr.stderr and not os.path.exists(str(tmp_path / "lost.tsv"))
    assert "batch: 2 of 3 reads aligned" in pr.stderr
    one = open(str(tmp_path / "one.tsv"), "rb").read()
    assert len(one) > 100000 and open(str(tmp_path / "two.tsv"), "rb").read().replace(b"\ttwo\t", b"\tone\t") == one


def test_locate_is_refused_next_to_a_cigar_a_window_and_rna(fasta, tmp_path):
    out = str(tmp_path / "o.tsv")
    for more, msg in ((["--guide-locate", "-p", "x.cigar"], "--guide-locate excludes -p and --guide-window"),
                      (["--guide-locate", "--guide-window", L.NAMES[0] + ":0-9000"], "--guide-locate excludes -p and --guide-window"),
                      (["--guide-locate", "--rna"], "cannot be combined with --rna")):
        pr = _run(_argv(fasta, out, "r", *more))
        assert pr.returncode != 0 and msg in pr.stderr and not os.path.exists(out), (more, pr.stderr)
