"""signalMachine --site-calls / --site-calls-aggregate: the per-read .calls rows against a restatement of
MarginalizeFullVariants.get_data (src/signalalign/variantCaller.py:92-187) applied to the full TSV the same run wrote, and the
over-reads table against a restatement of AggregateOverReadsFull._normalize_all_data / write_data (:393-410)."""
import json
import os
import subprocess

import numpy as np
import pytest

import sa_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")


def _write_fasta(path, name, seq, width=60):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for i in range(0, len(seq), width):
            f.write(seq[i:i + width] + "\n")
    with open(path + ".fai", "w") as f:
        f.write("%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), len(name) + 2, width, width + 1))


def _revcomp(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def get_data(tsv_text, variants, forward_mapped):
    """MarginalizeFullVariants.get_data (:125-187) over the rows of a full TSV: [(position, strand, forward_mapped, probs)]"""
    rows = [l.split("\t") for l in tsv_text.splitlines()]
    variant_data = [r for r in rows if "X" in r[2]]
    out = []
    if not variant_data:
        return out
    k1 = len(variant_data[0][2]) - 1
    mapping_strands = ["+", "-"] if forward_mapped else ["-", "+"]
    mapping_index = 0
    for read_strand in ("t", "c"):
        sd = [r for r in variant_data if r[4] == read_strand]
        if not sd:
            continue
        positions = sorted({int(r[1]) for r in sd})
        if mapping_strands[mapping_index] == "-":
            positions = positions[::-1]
        for pos in positions:
            pos_data = [r for r in sd if int(r[1]) == pos]
            if pos_data[0][9][k1] != "X":
                continue
            nuc = {n: sum(float(r[12]) for r in pos_data if r[15].rstrip("\n")[k1] == n) for n in variants}
            total = sum(nuc.values())
            assert total > 0
            out.append((pos, read_strand, mapping_strands[mapping_index], [nuc[n] / total for n in variants]))
        mapping_index += 1
    return out


def check_calls_file(calls_text, tsv_text, label, contig, variants, forward):
    exp = get_data(tsv_text, variants, forward)
    got = [l.split("\t") for l in calls_text.splitlines()]
    assert len(got) == len(exp) > 0
    for g, (pos, strand, mapped, probs) in zip(got, exp):
        assert g[:6] == [label, contig, str(pos), strand, mapped, variants], (g, pos, strand, mapped)
        assert len(g) == 6 + len(variants)
        for a, b in zip(g[6:], probs):
            assert abs(float(a) - b) <= 1e-6 + 1e-12
    return exp


def _oned_inputs(oracle, tmp_path):
    npread_path = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")
    read = oracle.parse_npread(npread_path)["template_read"]
    L = 1500
    ref = list(read[:L + 400])
    for i in range(60, len(ref) - 60):
        if read[i:i + 2] == "CG":
            ref[i] = "X"
    fasta = str(tmp_path / "ref.fa")
    _write_fasta(fasta, "chrA", "".join(ref) + "ACGTACGTAC")
    amb = str(tmp_path / "ce.ambig")
    with open(amb, "w") as f:
        f.write("X\tCE\n")
    return npread_path, fasta, amb, L


def test_per_read_calls_one_d_two_d_and_minus(oracle, tmp_path):
    npread_path, fasta, amb, L = _oned_inputs(oracle, tmp_path)
    cigar = str(tmp_path / "guide.cigar")
    with open(cigar, "w") as f:
        f.write("cigar: r 0 %d + chrA 0 %d + 1 M %d\n" % (L, L, L))
    base = [BIN, "-T", cases.MODEL_CPG, "-q", npread_path, "-f", fasta, "-n", "chrA", "-p", cigar, "-L", "r", "-s", "0", "-g", "100",
            "-a", amb]
    plain, withc = str(tmp_path / "plain.tsv"), str(tmp_path / "with.tsv")
    for out, extra in ((plain, []), (withc, ["--site-calls"])):
        pr = subprocess.run(base + ["-u", out] + extra, capture_output=True, text=True, timeout=300)
        assert pr.returncode == 0, pr.stderr
    tsv = open(withc).read()
    assert tsv == open(plain).read()                 # the posteriors are byte-identical with and without the option
    assert not os.path.exists(plain + ".calls")
    exp = check_calls_file(open(withc + ".calls").read(), tsv, "r", "chrA", "CE", True)
    assert len(exp) > 20

    # both strands of the bundled 2-D read, X at cytosines of the aligned window (default table: X -> ACGT)
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
    _write_fasta(fasta2, "ZYMO", "".join(z))
    model_c = os.path.join(cases.GOLDEN, "models", "testModelR73_acegot_complement.model")
    npread2 = os.path.join(cases.GOLDEN, "npReads", "ZymoC_ch_1_file1.npRead")
    out2 = str(tmp_path / "twod.tsv")
    pr = subprocess.run([BIN, "-T", cases.MODEL_R73, "-C", model_c, "-q", npread2, "-f", fasta2, "-n", "ZYMO", "-p", cigar2, "-u", out2,
                         "-L", "read2d", "--twoD", "-s", "0", "-g", "100", "--site-calls"], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    fwd = cig[8] == "+" if len(cig) > 8 else True
    exp2 = check_calls_file(open(out2 + ".calls").read(), open(out2).read(), "read2d", "ZYMO", "ACGT", fwd)
    assert {e[1] for e in exp2} == {"t", "c"}

    # a read mapped to the reverse strand: positions run backwards, forward_mapped '-'
    npread3 = os.path.join(cases.GOLDEN, "npReads", "c2925_ecoli_ch34_read1023.npRead")
    read = oracle.parse_npread(npread3)["template_read"]
    start2, L3 = 6, len(read) - 14
    part = read[start2:start2 + L3]
    pre, post = "GATTACA" * 9, "CCGGTTAA" * 6
    contig = list(pre + _revcomp(part) + post)
    for i in range(len(pre) + 20, len(pre) + L3 - 20, 11):
        if contig[i] in "CG":
            contig[i] = "X"
    contig = "".join(contig)
    fasta3, bfasta3 = str(tmp_path / "m_fwd.fa"), str(tmp_path / "m_bwd.fa")
    _write_fasta(fasta3, "chrM", contig)
    _write_fasta(bfasta3, "chrM", contig.translate(str.maketrans("ACGT", "TGCA")))
    cigar3 = str(tmp_path / "guide_m.cigar")
    with open(cigar3, "w") as f:
        f.write("cigar: rm %d %d + chrM %d %d - 1 M %d\n" % (start2, start2 + L3, len(pre) + L3, len(pre), L3))
    out3 = str(tmp_path / "minus.tsv")
    pr = subprocess.run([BIN, "-T", cases.MODEL_5MER, "-q", npread3, "-f", fasta3, "-b", bfasta3, "-n", "chrM", "-p", cigar3, "-u", out3,
                         "-L", "rm", "-s", "0", "-g", "100", "--site-calls"], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    exp3 = check_calls_file(open(out3 + ".calls").read(), open(out3).read(), "rm", "chrM", "ACGT", False)
    assert len(exp3) > 3 and exp3[0][2] == "-" and exp3[0][0] > exp3[-1][0]

    # refused in expectations mode
    pr = subprocess.run(base + ["-u", str(tmp_path / "e.tsv"), "-t", str(tmp_path / "t.expectations"), "--site-calls"],
                        capture_output=True, text=True, timeout=120)
    assert pr.returncode != 0 and "--site-calls" in pr.stderr


def _repr6(v):
    return repr(float(np.round(v, 6)))


def _write_fasta_records(path, records, width=60):
    """several records and their .fai (name, length, offset of the first base, bases per line, bytes per line)"""
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


def test_aggregate_over_reads(oracle, tmp_path):
    """Four forward-mapped windows of the 1-D read on chrA and two windows mapped to the reverse strand of chrM (template
    strand, forward_mapped '-'), across slices of three reads: every key kind the table of a 1-D run holds, and its row order."""
    npread_path, _, amb, L = _oned_inputs(oracle, tmp_path)
    read = oracle.parse_npread(npread_path)["template_read"]
    ref_a = list(read[:L + 400])
    for i in range(60, len(ref_a) - 60):
        if read[i:i + 2] == "CG":
            ref_a[i] = "X"
    ref_a = "".join(ref_a) + "ACGTACGTAC"
    # chrM: the reverse complement of read[100:1480]; X at the G of every CpG of the contig -- the C of a CpG of the read
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
    lines, lines_dash, tsvs, forward = [], [], [], []
    for i, s in enumerate((0, 120, 250, 330)):
        cigar = str(tmp_path / ("g%d.cigar" % i))
        with open(cigar, "w") as f:
            f.write("cigar: r%d %d %d + chrA %d %d + 1 M %d\n" % (i, s, s + L, s, s + L, L))
        tsvs.append(str(tmp_path / ("r%d.tsv" % i)))
        forward.append(True)
        lines.append("r%d\t%s\t%s\t%s\t-\tchrA\n" % (i, npread_path, cigar, tsvs[-1]))
        lines_dash.append("r%d\t%s\t%s\t-\t-\tchrA\n" % (i, npread_path, cigar))
    for i, (s, n) in enumerate(((m0, L2), (m0 + 90, L2 - 200))):
        cigar = str(tmp_path / ("gm%d.cigar" % i))
        t_hi = len(pre) + L2 - (s - m0)            # the window's read start maps to this contig position (reverse strand)
        with open(cigar, "w") as f:
            f.write("cigar: rm%d %d %d + chrM %d %d - 1 M %d\n" % (i, s, s + n, t_hi, t_hi - n, n))
        tsvs.append(str(tmp_path / ("rm%d.tsv" % i)))
        forward.append(False)
        lines.append("rm%d\t%s\t%s\t%s\t-\tchrM\n" % (i, npread_path, cigar, tsvs[-1]))
        lines_dash.append("rm%d\t%s\t%s\t-\t-\tchrM\n" % (i, npread_path, cigar))
    man, man_dash = str(tmp_path / "m.tsv"), str(tmp_path / "m_dash.tsv")
    open(man, "w").writelines(lines)
    open(man_dash, "w").writelines(lines_dash)
    agg, agg_dash = str(tmp_path / "agg.tsv"), str(tmp_path / "agg_dash.tsv")
    base = [BIN, "-T", cases.MODEL_CPG, "-f", fasta, "-b", bfasta, "-s", "0", "-g", "100", "-a", amb, "--batch-reads", "3"]
    pr = subprocess.run(base + ["--batch", man_dash, "--site-calls-aggregate", agg_dash], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    assert not any(os.path.exists(t) or os.path.exists(t + ".calls") for t in tsvs)   # the text-free path writes no TSV
    pr = subprocess.run(base + ["--batch", man, "--site-calls-aggregate", agg], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    assert "6 of 6 reads aligned" in pr.stderr, pr.stderr
    got_text = open(agg).read()
    assert got_text == open(agg_dash).read()        # the same table with and without the TSVs
    # _normalize_all_data over the per-read get_data of the TSVs the first run wrote
    per_key = {}
    for tsv, fwd in zip(tsvs, forward):
        contig_name = open(tsv).readline().split("\t")[0]
        for pos, strand, mapped, probs in get_data(open(tsv).read(), "CE", fwd):
            acc = per_key.setdefault((contig_name, pos, strand, mapped), [0.0, 0.0])
            acc[0] += probs[0]
            acc[1] += probs[1]
    got = got_text.splitlines()
    assert got[0] == "contig\tposition\tstrand\tforward_mapped\tC\tE"
    rows = {}
    for l in got[1:]:
        f = l.split("\t")
        rows[(f[0], int(f[1]), f[2], f[3])] = f[4:]
    assert set(rows) == set(per_key) and len(rows) > 40
    kinds = {(k[0], k[2], k[3]) for k in rows}
    assert kinds == {("chrA", "t", "+"), ("chrM", "t", "-")}, kinds
    assert sum(k[0] == "chrM" for k in rows) > 10
    for key, (c, e) in per_key.items():
        tot = c + e
        for a, b in zip(rows[key], (c / tot, e / tot)):
            assert abs(float(a) - float(np.round(b, 6))) <= 1.5e-6, (key, a, b)
            assert a == repr(float(a)) or a == _repr6(float(a))
    keys = [tuple(l.split("\t")[:4]) for l in got[1:]]
    assert keys == sorted(keys, key=lambda t: (t[0], t[2], t[3], int(t[1])))
