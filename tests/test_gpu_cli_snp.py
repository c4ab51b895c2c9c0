"""signalMachine --snp-step N --snp-dir D against the reference's route for single-nucleotide probabilities
(singleNucleotideProbabilities.py:551-723) run on the same binary: for every step s a FASTA with X at the positions = s (mod N),
one `-s 0` run on it, CallMethylation.call_methyls with a step offset restated over that run's TSV (the posterior column read
with float(), row by row), and the merge of discover_single_nucleotide_probabilities.  The files must be byte-identical."""
import json
import os
import subprocess

import pytest

import sa_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
MODEL_R73_C = os.path.join(cases.GOLDEN, "models", "testModelR73_acegot_complement.model")
COMP = str.maketrans("ACGT", "TGCA")


def write_fasta(path, records, width=60):
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


def periodic(seq, step, phase):
    chars = list(seq)
    for i in range(phase, len(chars), step):
        chars[i] = "X"
    return "".join(chars).upper()


def marginals(tsv_text, step, phase, k, forward):
    """call_methyls with step_offset = phase over one step's TSV: [(contig, site, strand, {letter: prob})]"""
    rows = [l.split("\t") for l in tsv_text.splitlines()]
    if not rows:
        return []   # (an empty file does not parse: the step yields no marginals)
    ref_index = [int(r[1]) for r in rows]
    lo, hi = min(ref_index) - step, max(ref_index) + step
    while lo % step:
        lo -= 1
    while hi % step:
        hi += 1
    out = []
    for strand, regular in (("t", forward), ("c", not forward)):
        by_index = {}
        for i, r in enumerate(rows):
            if r[4] == strand:
                by_index.setdefault(int(r[1]), []).append(i)
        for site in range(lo + phase, hi, step):
            chosen = sorted(i for x in range(site - (k - 1), site + 1) for i in by_index.get(x, []))
            if not chosen:
                continue
            marg = {"A": 0, "C": 0, "G": 0, "T": 0}
            for i in chosen:
                r = rows[i]
                off = site - int(r[1]) if regular else (k - 1) - (site - int(r[1]))
                marg[r[15][off]] += float(r[12])
            total = 0
            for v in marg.values():   # the serial fold of sum() over the dict, A C G T (no compensated summation)
                total += v
            out.append((rows[chosen[0]][0], site, strand, {l: v / total for l, v in marg.items()}))
    return out


def merged(lines, fast5, read_id, backward):
    lines = sorted(lines, key=lambda l: l[1])
    text = "## fast5_input: %s\n## read_id: %s\n## contig: %s\n## strand: %s\n#CHROM\tPOS\tpA\tpC\tpG\tpT\n" % (
        fast5, read_id, ",".join(sorted({l[0] for l in lines})), "complement" if backward else "template")
    for contig, site, _strand, p in lines:
        cols = [p["T"], p["G"], p["C"], p["A"]] if backward else [p["A"], p["C"], p["G"], p["T"]]
        text += "\t".join([contig, str(site)] + [str(v) for v in cols]) + "\n"
    return text


class Case:
    """one read: its FASTA records (and whether -b gets their complement), guide alignment, models and orientation"""

    def __init__(self, label, npread, records, cigar_line, models, forward, k, seq_name, backward_fasta=False, two_d=False):
        self.label, self.npread, self.records, self.cigar_line = label, npread, records, cigar_line
        self.models, self.forward, self.k, self.seq_name = models, forward, k, seq_name
        self.backward_fasta, self.two_d = backward_fasta, two_d


def _fastas(tmp, tag, records, backward_fasta, sub=None):
    recs = [(n, periodic(s, *sub) if sub else s) for n, s in records]
    f = str(tmp / ("%s.fa" % tag))
    write_fasta(f, recs)
    args = ["-f", f]
    if backward_fasta:
        b = str(tmp / ("%s_bwd.fa" % tag))
        write_fasta(b, [(n, s.translate(COMP)) for n, s in recs])
        args += ["-b", b]
    return args


def _cigar(tmp, case):
    path = str(tmp / ("%s.cigar" % case.label))
    with open(path, "w") as f:
        f.write(case.cigar_line)
    return path


def _common(case):
    args = ["-T", case.models[0]] + (["-C", case.models[1], "--twoD"] if case.two_d else [])
    return [BIN] + args + ["-n", case.seq_name, "-g", "100"]


def reference_route(tmp, case, step):
    """the N -s 0 runs and the merge: (file text, stdout lines)"""
    lines, stdout = [], []
    cigar = _cigar(tmp, case)
    for s in range(step):
        tsv = str(tmp / ("%s_step%d.tsv" % (case.label, s)))
        cmd = _common(case) + _fastas(tmp, "%s_s%d" % (case.label, s), case.records, case.backward_fasta, (step, s)) + [
            "-q", case.npread, "-p", cigar, "-L", case.label, "-s", "0", "-u", tsv]
        pr = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert pr.returncode == 0, pr.stderr
        stdout += pr.stdout.splitlines(True)
        lines += marginals(open(tsv).read(), step, s, case.k, case.forward)
    return merged(lines, os.path.basename(case.npread), case.label, not case.forward), stdout


def snp_route(tmp, case, step, extra=()):
    out = str(tmp / ("snp_%s_%d" % (case.label, step)))
    cmd = _common(case) + _fastas(tmp, case.label + "_plain", case.records, case.backward_fasta) + [
        "-q", case.npread, "-p", _cigar(tmp, case), "-L", case.label, "--snp-step", str(step), "--snp-dir", out] + list(extra)
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    return open(os.path.join(out, case.label + ".tsv")).read(), pr.stdout.splitlines(True)


def oned_case(oracle, L=1200, label="r9"):
    npread = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")
    read = oracle.parse_npread(npread)["template_read"]
    name = "chr_" + label
    return Case(label, npread, [(name, read[:L + 300] + "ACGTACGTAC")], "cigar: %s 0 %d + %s 0 %d + 1 M %d\n" % (label, L, name, L, L),
                [cases.MODEL_5MER], True, 5, name)


def minus_case(oracle):
    npread = os.path.join(cases.GOLDEN, "npReads", "c2925_ecoli_ch34_read1023.npRead")
    read = oracle.parse_npread(npread)["template_read"]
    start2, L = 6, len(read) - 14
    pre, post = "GATTACA" * 9, "CCGGTTAA" * 6
    contig = pre + read[start2:start2 + L].translate(COMP)[::-1] + post
    return Case("rm", npread, [("chrM", contig)], "cigar: rm %d %d + chrM %d %d - 1 M %d\n" % (start2, start2 + L, len(pre) + L, len(pre), L),
                [cases.MODEL_5MER], False, 5, "chrM", backward_fasta=True)


def twod_case():
    cig = json.load(open(os.path.join(cases.GOLDEN, "cigars", "zymoC_lastz_anchors.json")))["calls"][0]["cigars"][0].split()
    zymo = "".join(l.strip() for l in open(os.path.join(cases.GOLDEN, "sequences", "zymo_sequence.fasta")) if not l.startswith(">"))
    fwd = cig[8] == "+" if len(cig) > 8 else True
    return Case("read2d", os.path.join(cases.GOLDEN, "npReads", "ZymoC_ch_1_file1.npRead"), [("ZYMO", zymo)],
                " ".join(["cigar:", "read2d"] + cig[2:5] + ["ZYMO"] + cig[6:]) + "\n", [cases.MODEL_R73, MODEL_R73_C], fwd, 6, "ZYMO",
                two_d=True)


def _same(tmp, case, step):
    exp, exp_out = reference_route(tmp, case, step)
    got, got_out = snp_route(tmp, case, step)
    assert got == exp
    assert got_out == exp_out
    assert exp.count("\n") > 5 + 20
    return got


def test_one_d_forward_reference_setting(oracle, tmp_path):
    _same(tmp_path, oned_case(oracle), 5)             # the reference's own test: N = 5 with the R9 5-mer model


def test_one_d_forward_six_mer_step_ten(oracle, tmp_path):
    case = oned_case(oracle)
    case.models, case.k = [cases.MODEL_6MER], 6
    _same(tmp_path, case, 10)


def test_reverse_strand_with_backward_reference(oracle, tmp_path):
    text = _same(tmp_path, minus_case(oracle), 5)
    assert "## strand: complement\n" in text


def test_two_d_both_strands_in_one_file(tmp_path):
    _same(tmp_path, twod_case(), 10)


def test_step_below_k_many_paths_per_cell(oracle, tmp_path):
    # N = 3 < k = 5: up to 16 paths per cell, and the site window clips the last k-mers' positions
    _same(tmp_path, oned_case(oracle, L=300, label="short"), 3)


def _refused(oracle, label):
    """a read whose window holds letters outside the model's alphabet in every step's copy: the planner refuses it, alone"""
    bad = oned_case(oracle, L=400, label=label)
    name, seq = bad.records[0]
    bad.records = [(name, seq[:201] + "NN" + seq[203:])]
    return bad


def test_batch_manifest_three_slices_and_refused_reads(oracle, tmp_path):
    step = 5
    good = [oned_case(oracle, L=800, label="a"), minus_case(oracle), oned_case(oracle, L=500, label="b")]
    # two reads per slice (--batch-reads counts jobs: N per read): [bad1, a] -- the refused read first, a good one moves down
    # into its place --, [rm, bad2] -- the refused read last --, [b] -- a slice after both
    reads = [_refused(oracle, "bad1"), good[0], good[1], _refused(oracle, "bad2"), good[2]]
    expected = {}
    for c in good:
        expected[c.label] = reference_route(tmp_path, c, step)
    records = [r for c in reads for r in c.records]
    fastas = _fastas(tmp_path, "all", records, True)
    manifest = str(tmp_path / "reads.tsv")
    with open(manifest, "w") as f:
        for c in reads:
            f.write("\t".join([c.label, c.npread, _cigar(tmp_path, c), "-", "-", c.seq_name]) + "\n")
    out = str(tmp_path / "snp_batch")
    pr = subprocess.run([BIN, "-T", cases.MODEL_5MER, "-g", "100"] + fastas + ["--batch", manifest, "--batch-reads", str(2 * step),
                        "--snp-step", str(step), "--snp-dir", out], capture_output=True, text=True, timeout=600)
    assert pr.returncode == 1, pr.stderr                  # as -s 0: a refused read makes the run's status 1
    assert "read bad1 skipped" in pr.stderr and "read bad2 skipped" in pr.stderr
    assert "batch: 3 of 5 reads aligned" in pr.stderr      # every slice ran to its end
    assert sorted(os.listdir(out)) == ["a.tsv", "b.tsv", "rm.tsv"]
    for c in good:
        assert open(os.path.join(out, c.label + ".tsv")).read() == expected[c.label][0], c.label
    assert pr.stdout.splitlines(True) == [l for c in good for l in expected[c.label][1]]


def test_usage_errors(oracle, tmp_path):
    case = oned_case(oracle, L=300, label="u")
    base = _common(case) + _fastas(tmp_path, "u", case.records, False) + ["-q", case.npread, "-p", _cigar(tmp_path, case), "-L", "u"]
    d = str(tmp_path / "d")
    for extra, word in ((["--snp-step", "5", "--snp-dir", d, "-u", str(tmp_path / "x.tsv")], "-u"),
                        (["--snp-step", "5", "--snp-dir", d, "--mea"], "--mea"),
                        (["--snp-step", "0", "--snp-dir", d], "--snp-step")):
        pr = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert pr.returncode != 0 and word in pr.stderr.splitlines()[-1], (extra, pr.stderr[-300:])
        assert not os.path.exists(os.path.join(d, "u.tsv"))
