"""signalMachine --train-positions / --train-positions-coverage: the table file and the coverage file of a --batch run with forward-
and backward-mapped reads equal, byte for byte, the restatement (tests/train_positions_ref.py, then kmer_training_ref.top_n) applied
to the full TSVs the same run wrote; the same two files without any TSV; and a model trained on the filtered table changes only
k-mers that have rows in it."""
import os
import subprocess

import pytest

import kmer_training_ref as kref
import sa_cases as cases
import train_positions_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
K, N, MIN_PROB = 6, 2, 0.3


def _revcomp(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def _write_fasta_records(path, records, width=60):
    with open(path, "w") as f:
        for name, seq in records:
            f.write(">%s\n" % name)
            for i in range(0, len(seq), width):
                f.write(seq[i:i + width] + "\n")


def _kmer_id(name, alphabet="ACGT"):
    a = sorted(alphabet)
    return sum(a.index(c) * len(a) ** (len(name) - 1 - i) for i, c in enumerate(name))


def test_batch_run_with_forward_and_backward_reads(oracle, tmp_path):
    npread = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")
    read = oracle.parse_npread(npread)["template_read"]
    L, m0, L2 = 900, 100, 800
    ref_a = read[:L + 300] + "ACGTACGTAC"
    pre, post = "GATTACA" * 9, "CCGGTTAA" * 6
    ref_m = pre + _revcomp(read[m0:m0 + L2]) + post
    comp = str.maketrans("ACGT", "TGCA")
    fasta, bfasta = str(tmp_path / "two.fa"), str(tmp_path / "two_bwd.fa")
    _write_fasta_records(fasta, [("chrA", ref_a), ("chrM", ref_m)])
    _write_fasta_records(bfasta, [("chrA", ref_a.translate(comp)), ("chrM", ref_m.translate(comp))])
    reads = [("r0", "chrA", "cigar: r0 %d %d + chrA %d %d + 1 M %d\n" % (0, L, 0, L, L), True),
             ("rm", "chrM", "cigar: rm %d %d + chrM %d %d - 1 M %d\n" % (m0, m0 + L2, len(pre) + L2, len(pre), L2), False),
             ("r1", "chrA", "cigar: r1 %d %d + chrA %d %d + 1 M %d\n" % (150, 150 + L, 150, 150 + L, L), True)]
    lines, lines_dash, tsvs = [], [], []
    for label, contig, cigar_line, _ in reads:
        cigar = str(tmp_path / (label + ".cigar"))
        open(cigar, "w").write(cigar_line)
        tsvs.append(str(tmp_path / (label + ".tsv")))
        lines.append("%s\t%s\t%s\t%s\t-\t%s\n" % (label, npread, cigar, tsvs[-1], contig))
        lines_dash.append("%s\t%s\t%s\t-\t-\t%s\n" % (label, npread, cigar, contig))
    man, man_dash = str(tmp_path / "m.tsv"), str(tmp_path / "m_dash.tsv")
    open(man, "w").writelines(lines)
    open(man_dash, "w").writelines(lines_dash)
    # positions: chrM first (the coverage file keeps the file's order of contigs), both strands, a contig without reads, a
    # position closer than k to its neighbour, duplicate lines with other letters
    pos_lines = ["chrM\t%d\t%s\tC\tE\n" % (p, s) for s in "-+" for p in range(5, len(ref_m), 13)]
    pos_lines += ["chrA\t%d\t%s\tC\tE\n" % (p, s) for s in "+-" for p in range(0, len(ref_a), 11)]
    pos_lines += ["chrZ\t40\t+\tC\tE\n", "chrA\t24\t+\tA\tT\n", "chrA\t22\t+\tC\tO\n", "chrM\t18\t-\tG\tX\n", "# a comment\n", "\n"]
    positions = str(tmp_path / "positions.tsv")
    open(positions, "w").writelines(pos_lines)

    base = [BIN, "-T", cases.MODEL_6MER, "-f", fasta, "-b", bfasta, "-s", "0", "-g", "100", "--batch-reads", "2",
            "--train-max-assignments", str(N), "--train-min-prob", str(MIN_PROB), "--train-positions", positions]
    A, CV, M = (str(tmp_path / n) for n in ("a.tsv", "cover.tsv", "t.model"))
    pr = subprocess.run(base + ["--batch", man, "--train-assignments", A, "--train-positions-coverage", CV, "--train-template-model", M],
                        capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr[-2000:]
    assert "3 of 3 reads aligned" in pr.stderr

    rows = []   # the run's own full TSVs in manifest order: (contig, reference_index, strand, forward-mapped, k-mer, descaled, posterior)
    for (label, contig, _, forward), tsv in zip(reads, tsvs):
        for line in open(tsv):
            f = line.rstrip("\n").split("\t")
            assert f[0] == contig and f[4] == "t"
            rows.append((f[0], int(f[1]), f[4], forward, _kmer_id(f[15]), f[13], f[12]))
    plines = ref.parse_positions("".join(pos_lines))
    idx, counts = ref.offered([(r[0], r[1], r[2], r[3], r[6]) for r in rows], plines, K, MIN_PROB)
    assert {rows[i][3] for i in idx} == {True, False} and 100 < len(idx) < len(rows) // 2
    kept = kref.top_n([(rows[i][2], rows[i][4], rows[i][5], rows[i][6]) for i in idx], N, MIN_PROB)
    want = kref.table_lines(kept, "ACGT", K)
    assert want.count("\n") > 100
    assert open(A).read() == want
    want_cover = ref.coverage_lines(plines, counts)
    assert want_cover.startswith("chrM\t") and want_cover.count("\n") == len(set(plines))
    assert open(CV).read() == want_cover
    by_strand = {s: sum(n for (c, p, q), n in counts.items() if c == "chrM" and q == s) for s in "+-"}
    assert by_strand["-"] > 0 and by_strand["+"] == 0                            # the backward read's t rows pair with '-'
    assert sum(n for (c, p, q), n in counts.items() if c == "chrA" and q == "-") == 0 and counts[("chrZ", 40, "+")] == 0

    # the model trained on the filtered table: only k-mers with rows in it change
    st = {km: kref.stats([kref.units(r[2])[0] for r in v], False) for (s, km), v in kept.items()}
    want_model = str(tmp_path / "want.model")
    kref.write_trained(cases.MODEL_6MER, st, want_model)
    assert open(M, "rb").read() == open(want_model, "rb").read()
    _, _, prior = kref.read_model(cases.MODEL_6MER)
    _, _, got = kref.read_model(M)
    changed = {i // 5 for i, (a, b) in enumerate(zip(prior, got)) if a != b}
    assert changed and changed <= {km for (_, km) in kept} and len(changed) < len({r[4] for r in rows})

    # no TSV at all: the same two files
    for t in tsvs:
        os.remove(t)
    A2, CV2 = str(tmp_path / "a2.tsv"), str(tmp_path / "cover2.tsv")
    pr = subprocess.run(base + ["--batch", man_dash, "--train-assignments", A2, "--train-positions-coverage", CV2],
                        capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr[-2000:]
    assert not any(os.path.exists(t) for t in tsvs)
    assert open(A2, "rb").read() == open(A, "rb").read() and open(CV2, "rb").read() == open(CV, "rb").read()
