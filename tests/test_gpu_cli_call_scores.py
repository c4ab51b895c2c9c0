"""signalMachine --site-calls-accuracy: a --batch run of forward- and reverse-mapped reads scored against a positions file and
read labels.  The summary and the curves equal the restatement (call_scores_ref.py) computed from the files the same run wrote: the
sites, positions and mapping strands of the .calls files, each site's probabilities as the exact division of the printed posteriors
of its full-TSV rows (the .calls file prints them with six decimals, which is checked), and level 2 from the six-decimal values of
the aggregate file.  A second run with posteriors '-' and without --site-calls / --site-calls-aggregate writes the same bytes."""
import os
import re
import subprocess

import numpy as np
import pytest

import call_scores_ref as ref
import sa_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
N_BINS = 50


def _revcomp(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def _write_fasta_records(path, records, width=60):
    fai, off = [], 0
    with open(path, "w") as f:
        for name, seq in records:
            head = ">%s\n" % name
            f.write(head)
            off += len(head)
            fai.append("%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), off, width, width + 1))
            for i in range(0, len(seq), width):
                line = seq[i:i + width] + "\n"
                f.write(line)
                off += len(line)
    with open(path + ".fai", "w") as f:
        f.writelines(fai)


def _site_probs(tsv_rows, pos, strand, letters):
    """the call of one site from its rows of the full TSV: per letter the printed posteriors in integers of 1e-6, divided by their sum"""
    rows = [r for r in tsv_rows if int(r[1]) == pos and r[4] == strand]
    k1 = len(rows[0][2]) - 1
    units = [sum(int(round(float(r[12]) * 1e6)) for r in rows if r[15].rstrip("\n")[k1] == l) for l in letters]
    return [np.float64(u) / np.float64(sum(units)) for u in units]


def test_accuracy_of_a_batch_run(oracle, tmp_path):
    npread_path = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")
    read = oracle.parse_npread(npread_path)["template_read"]
    L = 1500
    ref_a = list(read[:L + 400])
    for i in range(60, len(ref_a) - 60):
        if read[i:i + 2] == "CG":
            ref_a[i] = "X"
    ref_a = "".join(ref_a) + "ACGTACGTAC"
    m0, L2 = 100, 1380
    pre, post = "GATTACA" * 9, "CCGGTTAA" * 6
    contig = list(pre + _revcomp(read[m0:m0 + L2]) + post)
    for p in range(len(pre) + 20, len(pre) + L2 - 20):
        if contig[p] == "C" and contig[p + 1] == "G":
            contig[p + 1] = "X"
    ref_m = "".join(contig)
    comp = str.maketrans("ACGT", "TGCA")
    fasta, bfasta = str(tmp_path / "two.fa"), str(tmp_path / "two_bwd.fa")
    _write_fasta_records(fasta, [("chrA", ref_a), ("chrM", ref_m)])
    _write_fasta_records(bfasta, [("chrA", ref_a.translate(comp)), ("chrM", ref_m.translate(comp))])
    amb = str(tmp_path / "ce.ambig")
    with open(amb, "w") as f:
        f.write("X\tCE\n")
    lines, lines_dash, tsvs, labels = [], [], [], []
    for i, s in enumerate((0, 120, 250, 330)):
        cigar = str(tmp_path / ("g%d.cigar" % i))
        with open(cigar, "w") as f:
            f.write("cigar: r%d %d %d + chrA %d %d + 1 M %d\n" % (i, s, s + L, s, s + L, L))
        tsvs.append(str(tmp_path / ("r%d.tsv" % i)))
        labels.append("r%d" % i)
        lines.append("r%d\t%s\t%s\t%s\t-\tchrA\n" % (i, npread_path, cigar, tsvs[-1]))
        lines_dash.append("r%d\t%s\t%s\t-\t-\tchrA\n" % (i, npread_path, cigar))
    for i, (s, n) in enumerate(((m0, L2), (m0 + 90, L2 - 200))):
        cigar = str(tmp_path / ("gm%d.cigar" % i))
        t_hi = len(pre) + L2 - (s - m0)
        with open(cigar, "w") as f:
            f.write("cigar: rm%d %d %d + chrM %d %d - 1 M %d\n" % (i, s, s + n, t_hi, t_hi - n, n))
        tsvs.append(str(tmp_path / ("rm%d.tsv" % i)))
        labels.append("rm%d" % i)
        lines.append("rm%d\t%s\t%s\t%s\t-\tchrM\n" % (i, npread_path, cigar, tsvs[-1]))
        lines_dash.append("rm%d\t%s\t%s\t-\t-\tchrM\n" % (i, npread_path, cigar))
    man, man_dash = str(tmp_path / "m.tsv"), str(tmp_path / "m_dash.tsv")
    open(man, "w").writelines(lines)
    open(man_dash, "w").writelines(lines_dash)
    # truth: every position of both contigs on both strands, change_to alternating by position, every fifth position left out,
    # and some keys named again with the other letter (the first line wins); two reads labelled as a whole
    truth_lines, table = [], {}
    for name, seq in (("chrA", ref_a), ("chrM", ref_m)):
        for pos in range(len(seq)):
            for strand in "+-":
                if pos % 5:
                    truth_lines.append("%s\t%d\t%s\tC\t%s\n" % (name, pos, strand, "CE"[pos % 2]))
                    table[(name, pos, strand)] = "CE"[pos % 2]
    truth_lines += [l[:-2] + ("E" if l[-2] == "C" else "C") + "\n" for l in truth_lines[::7]]
    truth, truth_reads = str(tmp_path / "positions.tsv"), str(tmp_path / "labels.tsv")
    open(truth, "w").writelines(truth_lines)
    read_label = {"r1": "E", "rm0": "C"}
    open(truth_reads, "w").writelines("%s\t%s\n" % kv for kv in read_label.items())

    base = [BIN, "-T", cases.MODEL_CPG, "-f", fasta, "-b", bfasta, "-s", "0", "-g", "100", "-a", amb, "--batch-reads", "3",
            "--site-calls-truth", truth, "--site-calls-truth-reads", truth_reads, "--site-calls-accuracy-bins", str(N_BINS)]
    agg, summ, curves = str(tmp_path / "agg.tsv"), str(tmp_path / "acc.tsv"), str(tmp_path / "curves.tsv")
    pr = subprocess.run(base + ["--batch", man, "--site-calls", "--site-calls-aggregate", agg, "--site-calls-accuracy", summ,
                                "--site-calls-accuracy-curves", curves], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    assert "6 of 6 reads aligned" in pr.stderr, pr.stderr

    exp = ref.Scores("CE", N_BINS, 0.500000001)
    n_sites = 0
    for label, tsv in zip(labels, tsvs):
        tsv_rows = [l.split("\t") for l in open(tsv).read().splitlines()]
        calls = [l.split("\t") for l in open(tsv + ".calls").read().splitlines()]
        per_strand = {}
        for c in calls:
            assert c[0] == label and c[5] == "CE"
            contig_name, pos, strand, mapped = c[1], int(c[2]), c[3], c[4]
            probs = _site_probs(tsv_rows, pos, strand, "CE")
            assert all(abs(float(a) - b) <= 1e-6 + 1e-12 for a, b in zip(c[6:], probs))
            n_sites += 1
            per_strand.setdefault(strand, []).append(probs)        # (file order: the order get_data walks the sites in)
            if label in read_label:
                exp.add(0, "tc".index(strand), probs, "CE".index(read_label[label]))
            elif (contig_name, pos, mapped) in table:
                exp.add(0, "tc".index(strand), probs, "CE".index(table[(contig_name, pos, mapped)]))
            else:
                exp.unlabelled += 1
        for strand, plist in per_strand.items():
            if label in read_label:
                exp.add(1, "tc".index(strand), [ref.read_mean([p[l] for p in plist]) for l in range(2)], "CE".index(read_label[label]))
    got_agg = open(agg).read().splitlines()
    assert got_agg[0] == "contig\tposition\tstrand\tforward_mapped\tC\tE"
    for l in got_agg[1:]:
        f = l.split("\t")
        letter = table.get((f[0], int(f[1]), f[3]))
        if letter is not None:
            exp.add(2, "tc".index(f[2]), [float(f[4]), float(f[5])], "CE".index(letter))
    rows = exp.rows()
    assert n_sites > 150 and exp.unlabelled > 10
    assert {r["level"] for r in rows} == {0, 1, 2} and {r["group"] for r in rows} == {0, 2}      # a 1-D run has template calls only
    assert all(r["n_pos"] > 0 and r["n_neg"] > 0 for r in rows if r["level"] != 1)
    assert open(summ).read() == ref.summary_text(rows)
    assert open(curves).read() == ref.curves_text(rows, N_BINS)
    m = re.search(r"accuracy: (\d+) rows; (\d+) calls without truth dropped, (\d+) sites of other letters skipped", pr.stderr)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (len(rows), exp.unlabelled, 0), pr.stderr

    # posteriors '-', neither --site-calls nor --site-calls-aggregate: the same summary, no TSV, no table
    summ2 = str(tmp_path / "acc_dash.tsv")
    for t in tsvs:
        os.remove(t)
        os.remove(t + ".calls")
    os.remove(agg)
    pr = subprocess.run(base + ["--batch", man_dash, "--site-calls-accuracy", summ2], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    assert open(summ2).read() == open(summ).read()
    assert not any(os.path.exists(t) or os.path.exists(t + ".calls") for t in tsvs) and not os.path.exists(agg)

    # the options' own rules
    plain = base[:-6] + ["--batch", man_dash]
    for extra, word in ((["--site-calls-truth", truth], "need --site-calls-accuracy"),
                        (["--site-calls-accuracy", summ2], "needs --site-calls-truth"),
                        (["--site-calls-accuracy", summ2, "--site-calls-truth", truth, "--site-calls-accuracy-bins", "0"], "takes n >= 1"),
                        (["--site-calls-accuracy", summ2, "--site-calls-truth", truth, "--snp-step", "4", "--snp-dir", str(tmp_path / "snp")],
                         "cannot be combined")):
        pr = subprocess.run(plain + extra, capture_output=True, text=True, timeout=120)
        assert pr.returncode != 0 and word in pr.stderr, (extra, pr.stderr[-400:])


def _restate_calls(exp, label, tsv, letters, table, read_label):
    """levels 0 and 1 of one read's .calls file into `exp`; returns the (strand, mapped) pairs seen"""
    tsv_rows = [l.split("\t") for l in open(tsv).read().splitlines()]
    per_strand, seen = {}, set()
    for c in [l.split("\t") for l in open(tsv + ".calls").read().splitlines()]:
        assert c[0] == label and c[5] == letters
        contig_name, pos, strand, mapped = c[1], int(c[2]), c[3], c[4]
        probs = _site_probs(tsv_rows, pos, strand, letters)
        assert all(abs(float(a) - b) <= 1e-6 + 1e-12 for a, b in zip(c[6:], probs))
        per_strand.setdefault(strand, []).append(probs)
        seen.add((strand, mapped))
        if label in read_label:
            exp.add(0, "tc".index(strand), probs, letters.index(read_label[label]))
        elif (contig_name, pos, mapped) in table:
            exp.add(0, "tc".index(strand), probs, letters.index(table[(contig_name, pos, mapped)]))
        else:
            exp.unlabelled += 1
    for strand, plist in per_strand.items():
        if label in read_label:
            exp.add(1, "tc".index(strand), [ref.read_mean([p[l] for p in plist]) for l in range(len(letters))],
                    letters.index(read_label[label]))
    return seen


def test_two_d_read_both_strands(tmp_path):
    """The bundled 2-D read with X at cytosines of its window (default table: X -> ACGT): the complement's calls carry the other
    mapping strand, which the rendering finds out, so its batch is scored after it; once against a positions file, once with the
    read labelled as a whole."""
    import json
    cig = json.load(open(os.path.join(cases.GOLDEN, "cigars", "zymoC_lastz_anchors.json")))["calls"][0]["cigars"][0].split()
    cigar2 = str(tmp_path / "guide2d.cigar")
    with open(cigar2, "w") as f:
        f.write(" ".join(["cigar:", "read2d"] + cig[2:5] + ["ZYMO"] + cig[6:]) + "\n")
    zymo = "".join(l.strip() for l in open(os.path.join(cases.GOLDEN, "sequences", "zymo_sequence.fasta")) if not l.startswith(">"))
    t0, t1 = sorted((int(cig[6]), int(cig[7])))
    z = list(zymo)
    cs = [i for i in range(t0 + 20, t1 - 20) if z[i] == "C"]
    for i in cs[::max(1, len(cs) // 15)][:15]:
        z[i] = "X"
    fasta2 = str(tmp_path / "zymo_x.fa")
    _write_fasta_records(fasta2, [("ZYMO", "".join(z))])
    model_c = os.path.join(cases.GOLDEN, "models", "testModelR73_acegot_complement.model")
    npread2 = os.path.join(cases.GOLDEN, "npReads", "ZymoC_ch_1_file1.npRead")
    truth_lines, table = [], {}
    for pos in range(len(z)):
        for strand in "+-":
            if pos % 4:
                truth_lines.append("ZYMO\t%d\t%s\tC\t%s\n" % (pos, strand, "ACGT"[pos % 4]))
                table[("ZYMO", pos, strand)] = "ACGT"[pos % 4]
    truth, truth_reads = str(tmp_path / "positions.tsv"), str(tmp_path / "labels.tsv")
    open(truth, "w").writelines(truth_lines)
    open(truth_reads, "w").write("read2d\tC\n")
    base = [BIN, "-T", cases.MODEL_R73, "-C", model_c, "-q", npread2, "-f", fasta2, "-n", "ZYMO", "-p", cigar2, "-L", "read2d", "--twoD",
            "-s", "0", "-g", "100", "--site-calls", "--site-calls-accuracy-bins", str(N_BINS)]
    for name, opts, tab, lab in (("pos", ["--site-calls-truth", truth], table, {}), ("lab", ["--site-calls-truth-reads", truth_reads], {}, {"read2d": "C"})):
        out, summ = str(tmp_path / (name + ".tsv")), str(tmp_path / (name + "_acc.tsv"))
        pr = subprocess.run(base + opts + ["-u", out, "--site-calls-accuracy", summ], capture_output=True, text=True, timeout=300)
        assert pr.returncode == 0, pr.stderr
        exp = ref.Scores("ACGT", N_BINS, 0.500000001)
        seen = _restate_calls(exp, "read2d", out, "ACGT", tab, lab)
        assert {s for s, _ in seen} == {"t", "c"} and len({m for _, m in seen}) == 2      # the strands map to opposite strands
        rows = [r for r in exp.rows() if r["level"] < 2]
        assert {r["group"] for r in rows} == {0, 1, 2} and ({r["level"] for r in rows} == ({0, 1} if lab else {0}))
        got = open(summ).read()
        assert "".join(l + "\n" for l in got.splitlines() if not l.startswith("2\t")) == ref.summary_text(rows)
    # refused with what ends a 2-D batch before its rendering
    pr = subprocess.run(base + ["--site-calls-truth", truth, "-u", str(tmp_path / "x.tsv"), "--site-calls-accuracy", summ, "--mea"],
                        capture_output=True, text=True, timeout=120)
    assert pr.returncode != 0 and "--mea" in pr.stderr


def test_refused_reads_leave_the_scores_of_the_others(oracle, tmp_path):
    """The six reads of the batch run with two reads the planner refuses (an N in their reference window) among them: one at the
    head of the first slice, ahead of any call, so that the slice that would make the accumulator is the one started over, and one
    in the second slice, which is checkpointed and rolled back.  6 of 8 reads align, and every file of the good reads and of the
    run equals the six-read run's."""
    npread_path = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")
    read = oracle.parse_npread(npread_path)["template_read"]
    L, m0, L2 = 1500, 100, 1380
    ref_a = list(read[:L + 400])
    for i in range(60, len(ref_a) - 60):
        if read[i:i + 2] == "CG":
            ref_a[i] = "X"
    ref_a = "".join(ref_a) + "ACGTACGTAC"
    pre, post = "GATTACA" * 9, "CCGGTTAA" * 6
    contig = list(pre + _revcomp(read[m0:m0 + L2]) + post)
    for p in range(len(pre) + 20, len(pre) + L2 - 20):
        if contig[p] == "C" and contig[p + 1] == "G":
            contig[p + 1] = "X"
    ref_m = "".join(contig)
    ref_n = ref_a[:700] + "N" + ref_a[701:]
    comp = str.maketrans("ACGT", "TGCA")
    fasta, bfasta = str(tmp_path / "three.fa"), str(tmp_path / "three_bwd.fa")
    _write_fasta_records(fasta, [("chrA", ref_a), ("chrM", ref_m), ("chrN", ref_n)])
    _write_fasta_records(bfasta, [("chrA", ref_a.translate(comp)), ("chrM", ref_m.translate(comp)), ("chrN", ref_n.translate(comp))])
    amb = str(tmp_path / "ce.ambig")
    with open(amb, "w") as f:
        f.write("X\tCE\n")

    def line(run, label, chrom, cigar_text):
        cigar = str(tmp_path / (label + ".cigar"))
        with open(cigar, "w") as f:
            f.write(cigar_text)
        return "%s\t%s\t%s\t%s\t-\t%s\n" % (label, npread_path, cigar, str(tmp_path / run / (label + ".tsv")), chrom)

    def manifest(run):
        os.mkdir(str(tmp_path / run))
        good = [line(run, "r%d" % i, "chrA", "cigar: r%d %d %d + chrA %d %d + 1 M %d\n" % (i, s, s + L, s, s + L, L))
                for i, s in enumerate((0, 120, 250, 330))]
        for i, (s, n) in enumerate(((m0, L2), (m0 + 90, L2 - 200))):
            t_hi = len(pre) + L2 - (s - m0)
            good.append(line(run, "rm%d" % i, "chrM", "cigar: rm%d %d %d + chrM %d %d - 1 M %d\n" % (i, s, s + n, t_hi, t_hi - n, n)))
        return good

    truth, truth_reads = str(tmp_path / "positions.tsv"), str(tmp_path / "labels.tsv")
    with open(truth, "w") as f:
        for name, seq in (("chrA", ref_a), ("chrM", ref_m)):
            f.writelines("%s\t%d\t%s\tC\t%s\n" % (name, pos, strand, "CE"[pos % 2]) for pos in range(len(seq)) for strand in "+-" if pos % 5)
    open(truth_reads, "w").write("r1\tE\nrm0\tC\n")
    base = [BIN, "-T", cases.MODEL_CPG, "-f", fasta, "-b", bfasta, "-s", "0", "-g", "100", "-a", amb, "--batch-reads", "3", "--site-calls",
            "--site-calls-truth", truth, "--site-calls-truth-reads", truth_reads, "--site-calls-accuracy-bins", str(N_BINS)]

    def run(name, lines, status, word):
        man = str(tmp_path / (name + ".manifest"))
        open(man, "w").writelines(lines)
        outs = [str(tmp_path / name / f) for f in ("agg.tsv", "acc.tsv", "curves.tsv")]
        pr = subprocess.run(base + ["--batch", man, "--site-calls-aggregate", outs[0], "--site-calls-accuracy", outs[1],
                                    "--site-calls-accuracy-curves", outs[2]], capture_output=True, text=True, timeout=300)
        assert pr.returncode == status, pr.stderr[-2000:]
        assert word in pr.stderr, pr.stderr[-2000:]
        return pr, {f: open(os.path.join(str(tmp_path / name), f), "rb").read() for f in sorted(os.listdir(str(tmp_path / name)))}

    _, want = run("six", manifest("six"), 0, "6 of 6 reads aligned")
    assert len(want) == 3 + 2 * 6 and all(want.values())
    lines = manifest("eight")    # slices of three: [bad0, r0, r1], [r2, bad1, r3], [rm0, rm1]
    for at, label in ((0, "bad0"), (4, "bad1")):
        lines.insert(at, line("eight", label, "chrN", "cigar: %s %d %d + chrN %d %d + 1 M %d\n" % (label, 60, 60 + L, 60, 60 + L, L)))
    pr, got = run("eight", lines, 1, "6 of 8 reads aligned")
    assert "read bad0 skipped: alignment job rejected" in pr.stderr and "read bad1 skipped: alignment job rejected" in pr.stderr
    assert sorted(got) == sorted(want)        # (no file of a refused read)
    assert got == want
