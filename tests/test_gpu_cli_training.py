"""signalMachine --train-assignments / --train-template-model / --train-complement-model: the table and the retrained models
against the restatement (tests/kmer_training_ref.py) applied to the -s 2 files the same run wrote, concatenated in manifest
order; the same outputs without any TSV (posteriors '-'); a 2-D run; buildHdpUtil -l takes the table."""
import json
import os
import subprocess

import pytest

import kmer_training_ref as ref
import sa_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
HDP_TOOL = os.path.join(ROOT, "signalalign_amd", "bin", "buildHdpUtil")


def _write_fasta(path, name, seq, width=60):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for i in range(0, len(seq), width):
            f.write(seq[i:i + width] + "\n")
    with open(path + ".fai", "w") as f:
        f.write("%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), len(name) + 2, width, width + 1))


def _kmer_ids(alphabet, k):
    a = sorted(alphabet)
    return lambda s: sum(a.index(c) * len(a) ** (k - 1 - i) for i, c in enumerate(s))


def _restate(tsv_paths, alphabet, k, n, min_prob):
    kid = _kmer_ids(alphabet, k)
    rows = []
    for p in tsv_paths:
        for line in open(p):
            f = line.rstrip("\n").split("\t")
            rows.append((f[1], kid(f[0]), f[2], f[3]))
    return ref.top_n(rows, n, min_prob)


def _four_windows(oracle, tmp_path):
    """Four 1200-base windows of r9p4_oneD.npRead on a contig made of the read itself: the manifest rows with and without TSVs"""
    npread = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")
    read = oracle.parse_npread(npread)["template_read"]
    L = 1200
    fasta = str(tmp_path / "ref.fa")
    _write_fasta(fasta, "chrA", read[:L + 400] + "ACGTACGTAC")
    lines, lines_dash, tsvs = [], [], []
    for i, s in enumerate((0, 120, 250, 330)):
        cigar = str(tmp_path / ("g%d.cigar" % i))
        with open(cigar, "w") as f:
            f.write("cigar: r%d %d %d + chrA %d %d + 1 M %d\n" % (i, s, s + L, s, s + L, L))
        tsvs.append(str(tmp_path / ("r%d.tsv" % i)))
        lines.append("r%d\t%s\t%s\t%s\t-\tchrA\n" % (i, npread, cigar, tsvs[-1]))
        lines_dash.append("r%d\t%s\t%s\t-\t-\tchrA\n" % (i, npread, cigar))
    return npread, read, fasta, lines, lines_dash, tsvs


def test_batch_table_and_model(oracle, tmp_path):
    _, _, fasta, lines, lines_dash, tsvs = _four_windows(oracle, tmp_path)
    man, man_dash = str(tmp_path / "m.tsv"), str(tmp_path / "m_dash.tsv")
    open(man, "w").writelines(lines)
    open(man_dash, "w").writelines(lines_dash)
    base = [BIN, "-T", cases.MODEL_6MER, "-f", fasta, "-s", "2", "-g", "100", "--batch-reads", "3"]
    train = ["--train-max-assignments", "3", "--train-min-prob", "0.5"]
    A, M, A2, M2 = (str(tmp_path / n) for n in ("a.tsv", "t.model", "a2.tsv", "t2.model"))
    pr = subprocess.run(base + ["--batch", man, "--train-assignments", A, "--train-template-model", M] + train,
                        capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr[-2000:]
    assert "4 of 4 reads aligned" in pr.stderr
    kept = _restate(tsvs, "ACGT", 6, 3, 0.5)
    exp_text = ref.table_lines(kept, "ACGT", 6)
    assert exp_text.count("\n") > 300
    assert open(A).read() == exp_text
    st = {km: ref.stats([ref.units(r[2])[0] for r in v], False) for (s, km), v in kept.items() if s == "t"}
    want = str(tmp_path / "want.model")
    ref.write_trained(cases.MODEL_6MER, st, want)
    assert open(M, "rb").read() == open(want, "rb").read()
    # no TSV at all: the same outputs
    for t in tsvs:
        os.remove(t)
    pr = subprocess.run(base + ["--batch", man_dash, "--train-assignments", A2, "--train-template-model", M2] + train,
                        capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr[-2000:]
    assert not any(os.path.exists(t) for t in tsvs)
    assert open(A2, "rb").read() == open(A, "rb").read() and open(M2, "rb").read() == open(M, "rb").read()
    # the median variant and a k-mer list
    kl = str(tmp_path / "kmers.txt")
    names = sorted({ref.kmer_name(km, "ACGT", 6) for (_, km) in kept})[:40]
    open(kl, "w").write("\n".join(names) + "\n")
    M3 = str(tmp_path / "t3.model")
    pr = subprocess.run(base + ["--batch", man_dash, "--train-template-model", M3, "--train-median", "--train-kmers", kl,
                                "--train-weight", "20", "--train-min-sd", "1.5"] + train, capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr[-2000:]
    st3 = {km: ref.stats([ref.units(r[2])[0] for r in v], True) for (s, km), v in kept.items() if s == "t"}
    ref.write_trained(cases.MODEL_6MER, st3, want, weight=20.0, min_sd=1.5, kmers=set(names))
    assert open(M3, "rb").read() == open(want, "rb").read()
    # buildHdpUtil -l takes the table as it is
    out = str(tmp_path / "t.nhdp")
    cmd = [HDP_TOOL, "-p", "14", "-v", out, "-w", "None", "-l", A, "-a", "6", "-n", "5", "-I", "20", "-t", "2", "-s", "40", "-e", "140",
           "-k", "50", "--oneD", "-C", "None", "-T", cases.MODEL_6MER, "-B", "1", "-M", "1", "-L", "1", "-b", "ACGT"]
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr[-2000:]
    assert os.path.exists(out)


def test_refused_read_rolls_the_tables_back(oracle, tmp_path):
    """A read the planner refuses (an N in its reference window) shares the first slice with two good reads: the slice is
    retried without it, and the rows its first attempt put into the run's k-mer table are taken back (checkpoint / rollback).
    Everything the four good reads produce is byte for byte what the manifest without the refused read produces."""
    npread, read, fasta, lines, _, tsvs = _four_windows(oracle, tmp_path)
    L = 1200
    base = [BIN, "-T", cases.MODEL_6MER, "-f", fasta, "-s", "2", "-g", "100", "--batch-reads", "3",
            "--train-max-assignments", "3", "--train-min-prob", "0.5"]
    man, man_bad = str(tmp_path / "m.tsv"), str(tmp_path / "m_bad.tsv")
    open(man, "w").writelines(lines)
    A, M, A2, M2 = (str(tmp_path / n) for n in ("a.tsv", "t.model", "a2.tsv", "t2.model"))
    pr = subprocess.run(base + ["--batch", man, "--train-assignments", A, "--train-template-model", M],
                        capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr[-2000:]
    want = [open(t, "rb").read() for t in tsvs]
    assert all(want) and open(A, "rb").read()
    for t in tsvs:
        os.remove(t)
    # the refused read, second in the manifest: the first slice is [r0, bad, r1], the second [r2, r3]
    contig = read[:L + 400] + "ACGTACGTAC"
    fasta_n = str(tmp_path / "refN.fa")
    _write_fasta(fasta_n, "chrN", contig[:700] + "N" + contig[701:])
    os.remove(fasta_n + ".fai")                  # two records in one file: let the loader scan it (no index)
    with open(fasta, "a") as f:
        f.write(open(fasta_n).read())
    os.remove(fasta + ".fai")
    cigar_n = str(tmp_path / "bad.cigar")
    with open(cigar_n, "w") as f:
        f.write("cigar: bad %d %d + chrN %d %d + 1 M %d\n" % (60, 60 + L, 60, 60 + L, L))
    bad_tsv = str(tmp_path / "bad.tsv")
    lines.insert(1, "bad\t%s\t%s\t%s\t-\tchrN\n" % (npread, cigar_n, bad_tsv))
    open(man_bad, "w").writelines(lines)
    pr = subprocess.run(base + ["--batch", man_bad, "--train-assignments", A2, "--train-template-model", M2],
                        capture_output=True, text=True, timeout=600)
    assert pr.returncode == 1, pr.stderr[-2000:]
    assert "read bad skipped: alignment job rejected" in pr.stderr
    assert "4 of 5 reads aligned" in pr.stderr
    assert not os.path.exists(bad_tsv)
    assert [open(t, "rb").read() for t in tsvs] == want
    assert open(A2, "rb").read() == open(A, "rb").read()
    assert open(M2, "rb").read() == open(M, "rb").read()


def test_two_d_run_writes_both_strands(tmp_path):
    cig = json.load(open(os.path.join(cases.GOLDEN, "cigars", "zymoC_lastz_anchors.json")))["calls"][0]["cigars"][0].split()
    cigar2 = str(tmp_path / "guide2d.cigar")
    with open(cigar2, "w") as f:
        f.write(" ".join(["cigar:", "read2d"] + cig[2:5] + ["ZYMO"] + cig[6:]) + "\n")
    zymo = "".join(l.strip() for l in open(os.path.join(cases.GOLDEN, "sequences", "zymo_sequence.fasta")) if not l.startswith(">"))
    fasta2 = str(tmp_path / "zymo.fa")
    _write_fasta(fasta2, "ZYMO", zymo)
    model_c = os.path.join(cases.GOLDEN, "models", "testModelR73_acegot_complement.model")
    npread2 = os.path.join(cases.GOLDEN, "npReads", "ZymoC_ch_1_file1.npRead")
    out2, A, MT, MC = (str(tmp_path / n) for n in ("twod.tsv", "a.tsv", "t.model", "c.model"))
    pr = subprocess.run([BIN, "-T", cases.MODEL_R73, "-C", model_c, "-q", npread2, "-f", fasta2, "-n", "ZYMO", "-p", cigar2, "-u", out2,
                         "-L", "read2d", "--twoD", "-s", "2", "-g", "100", "--train-assignments", A, "--train-template-model", MT,
                         "--train-complement-model", MC, "--train-min-prob", "0.3"], capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr[-2000:]
    kept = _restate([out2], "ACEGOT", 6, 10, 0.3)
    assert {s for (s, _) in kept} == {"t", "c"}
    assert open(A).read() == ref.table_lines(kept, "ACEGOT", 6)
    assert not os.path.exists(A + ".c")
    for strand, prior, got in (("t", cases.MODEL_R73, MT), ("c", model_c, MC)):
        st = {km: ref.stats([ref.units(r[2])[0] for r in v], False) for (s, km), v in kept.items() if s == strand}
        want = str(tmp_path / ("want_%s.model" % strand))
        ref.write_trained(prior, st, want)
        assert open(got, "rb").read() == open(want, "rb").read(), strand
