"""signalMachine --snp-marginals / --snp-proposals / --snp-sites / --snp-reference-out: the over-reads table of a --batch run must
be byte-identical to the restatement (snp_marginals_ref.py) run over the per-read files the same run wrote, with and without
--snp-dir, across three slices with a minus-strand read and refused reads; the second pass must equal the restatement over a
`-s 0` run on a FASTA with X at the listed sites; the corrected reference must equal sa_snp_apply_calls; and the options' usage
errors must be refused.  The case builders follow test_gpu_cli_snp.py's."""
import os
import subprocess

import numpy as np
import pytest

import signalalign_amd as sa

import sa_cases as cases
import snp_marginals_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
COMP = str.maketrans("ACGT", "TGCA")
STEP = 5
K = 5


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


def fasta_text(records, width=60):
    return "".join(">%s\n" % n + "".join(s[i:i + width] + "\n" for i in range(0, len(s), width)) for n, s in records)


def fastas(tmp, tag, records, width=60):
    f, b = str(tmp / ("%s.fa" % tag)), str(tmp / ("%s_bwd.fa" % tag))
    write_fasta(f, records, width)
    write_fasta(b, [(n, s.translate(COMP)) for n, s in records], width)
    return ["-f", f, "-b", b]


class Read:
    def __init__(self, label, npread, cigar_line, seq_name, forward):
        self.label, self.npread, self.cigar_line, self.seq_name, self.forward = label, npread, cigar_line, seq_name, forward


def the_reads(oracle):
    """5 reads on three records: a and b overlap on chr_ab (depth 2), rm is mapped to the minus strand of chrM, bad1 and bad2
    lie on a record with letters outside the alphabet and are refused.  With --batch-reads 2 * STEP the slices are [bad1, a],
    [rm, bad2], [b]: a refused read first in its slice, one last, and a slice after both."""
    one_d = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")
    read = oracle.parse_npread(one_d)["template_read"]
    chr_ab = read[:1100] + "ACGTACGTAC"
    chr_bad = read[:201] + "NN" + read[203:700]
    minus = os.path.join(cases.GOLDEN, "npReads", "c2925_ecoli_ch34_read1023.npRead")
    mread = oracle.parse_npread(minus)["template_read"]
    start2, L = 6, len(mread) - 14
    pre, post = "GATTACA" * 9, "CCGGTTAA" * 6
    chr_m = pre + mread[start2:start2 + L].translate(COMP)[::-1] + post
    records = [("chr_ab", chr_ab), ("chrM", chr_m), ("chr_bad", chr_bad)]

    def fwd(label, L, name):
        return Read(label, one_d, "cigar: %s 0 %d + %s 0 %d + 1 M %d\n" % (label, L, name, L, L), name, True)
    reads = [fwd("bad1", 400, "chr_bad"), fwd("a", 800, "chr_ab"),
             Read("rm", minus, "cigar: rm %d %d + chrM %d %d - 1 M %d\n" % (start2, start2 + L, len(pre) + L, len(pre), L), "chrM", False),
             fwd("bad2", 400, "chr_bad"), fwd("b", 500, "chr_ab")]
    return reads, records


def manifest(tmp, reads, tag, posteriors=None):
    path = str(tmp / ("%s.manifest" % tag))
    with open(path, "w") as f:
        for r in reads:
            cig = str(tmp / ("%s.cigar" % r.label))
            with open(cig, "w") as c:
                c.write(r.cigar_line)
            f.write("\t".join([r.label, r.npread, cig, posteriors[r.label] if posteriors else "-", "-", r.seq_name]) + "\n")
    return path


def run(args, status):
    pr = subprocess.run([BIN, "-T", cases.MODEL_5MER, "-g", "100"] + args, capture_output=True, text=True, timeout=600)
    assert pr.returncode == status, pr.stderr[-2000:]
    return pr


def rows_of_read_file(text, contig_index, run_ordinal):
    """the lines of one <label>.tsv as rows of the restatement: a 1-D read's strand is t, its direction is the read's mapping
    strand, and a backward read's file holds the columns in T G C A order"""
    backward = "## strand: complement\n" in text
    rows = []
    for line in text.splitlines():
        if line.startswith("#"):
            continue
        c = line.split("\t")
        p = [float(v) for v in c[2:6]]
        rows.append((contig_index[c[0]], int(c[1]), run_ordinal, 0, 0 if backward else 1, tuple(p[::-1] if backward else p)))
    return rows


def restated(calls, records):
    names = [n for n, _ in records]
    sites = ref.finish(ref.accumulate(calls), 1, [s for _, s in records])
    proposals = ""
    for ci, name in enumerate(names):
        mine = {s["pos"]: s["delta"] for s in sites if s["contig"] == ci and s["is_proposal"]}
        for pos in ref.group_sites(sorted(mine.items()), 6, True):
            proposals += "%s\t%d\t%s\n" % (name, pos, repr(float(mine[pos])))
    return sites, ref.marginals_file(sites, names), proposals


def calls_from_dir(d, good, records):
    index = {n: i for i, (n, _) in enumerate(records)}
    return [rows_of_read_file(open(os.path.join(d, r.label + ".tsv")).read(), index, i) for i, r in enumerate(good)]


def as_array(sites):
    arr = np.zeros(len(sites), dtype=sa.SNP_MARGINAL_DTYPE)
    for a, s in zip(arr, sites):
        a["pos"], a["contig"], a["depth"], a["delta"] = s["pos"], s["contig"], s["depth"], s["delta"]
        a["fwd"], a["bwd"], a["prob"] = s["fwd"], s["bwd"], s["prob"]
        a["called"], a["ref"], a["is_proposal"] = s["called"].encode(), s["ref"].encode(), int(s["is_proposal"])
    return arr


def marginals_at_sites(tsv_text, sites, k, forward):
    """call_methyls with `positions` over one read's full TSV: [(contig, site, {letter: prob})] for the template strand"""
    rows = [l.split("\t") for l in tsv_text.splitlines()]
    by_index = {}
    for i, r in enumerate(rows):
        if r[4] == "t":
            by_index.setdefault(int(r[1]), []).append(i)
    out = []
    for site in sites:
        chosen = sorted(i for x in range(site - (k - 1), site + 1) for i in by_index.get(x, []))
        if not chosen:
            continue
        marg = {"A": 0, "C": 0, "G": 0, "T": 0}
        for i in chosen:
            r = rows[i]
            off = site - int(r[1]) if forward else (k - 1) - (site - int(r[1]))
            marg[r[15][off]] += float(r[12])
        total = 0
        for v in marg.values():
            total += v
        out.append((rows[chosen[0]][0], site, {l: v / total for l, v in marg.items()}))
    return out


@pytest.fixture(scope="module")
def first_pass(oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("snp_marginals")
    reads, records = the_reads(oracle)
    fa = fastas(tmp, "all", records)
    base = fa + ["--batch", manifest(tmp, reads, "all"), "--batch-reads", str(2 * STEP), "--snp-step", str(STEP)]
    d0, d1 = str(tmp / "d_plain"), str(tmp / "d_new")
    m1, p1, m2 = str(tmp / "m1.tsv"), str(tmp / "p1.tsv"), str(tmp / "m2.tsv")
    plain = run(base + ["--snp-dir", d0], 1)
    new = run(base + ["--snp-dir", d1, "--snp-marginals", m1, "--snp-proposals", p1], 1)
    no_dir = run(base + ["--snp-marginals", m2], 1)
    good = [r for r in reads if not r.label.startswith("bad")]
    return dict(tmp=tmp, reads=reads, good=good, records=records, fa=fa, d0=d0, d1=d1, m1=m1, p1=p1, m2=m2, plain=plain, new=new,
                no_dir=no_dir)


def test_table_and_proposals_equal_the_restatement_over_the_per_read_files(first_pass):
    c = first_pass
    assert "read bad1 skipped" in c["new"].stderr and "read bad2 skipped" in c["new"].stderr
    assert "batch: 3 of 5 reads aligned" in c["new"].stderr
    sites, table, proposals = restated(calls_from_dir(c["d1"], c["good"], c["records"]), c["records"])
    assert open(c["m1"]).read() == table
    assert open(c["p1"]).read() == proposals
    assert len(sites) > 1000 and max(s["depth"] for s in sites) == 2 and {s["contig"] for s in sites} == {0, 1}
    assert any(any(s["bwd"]) for s in sites) and any(any(s["fwd"]) for s in sites)
    assert proposals.count("\n") >= 1


def test_per_read_files_and_stdout_are_unchanged_by_the_new_options(first_pass):
    c = first_pass
    assert sorted(os.listdir(c["d0"])) == sorted(os.listdir(c["d1"])) == ["a.tsv", "b.tsv", "rm.tsv"]
    for name in os.listdir(c["d0"]):
        assert open(os.path.join(c["d0"], name)).read() == open(os.path.join(c["d1"], name)).read(), name
    assert c["plain"].stdout == c["new"].stdout == c["no_dir"].stdout


def test_same_table_without_the_per_read_files(first_pass):
    c = first_pass
    assert open(c["m2"]).read() == open(c["m1"]).read()


def test_second_pass_and_corrected_reference(first_pass):
    c = first_pass
    tmp, records, good = c["tmp"], c["records"], c["good"]
    m3, r3 = str(tmp / "m3.tsv"), str(tmp / "corrected.fa")
    run(c["fa"] + ["--batch", manifest(tmp, c["reads"], "second"), "--batch-reads", "2", "--snp-sites", c["p1"], "--snp-marginals", m3,
                   "--snp-reference-out", r3], 1)
    # the reference's route: X at the listed sites in the FASTA, one -s 0 run, call_methyls with positions over each read's TSV
    listed = {}
    for line in open(c["p1"]):
        name, pos = line.split("\t")[:2]
        listed.setdefault(name, []).append(int(pos))
    with_x = []
    for name, seq in records:
        chars = list(seq.upper())
        for pos in listed.get(name, []):
            chars[pos] = "X"
        with_x.append((name, "".join(chars)))
    tsv = {r.label: str(tmp / ("%s_full.tsv" % r.label)) for r in c["reads"]}
    run(fastas(tmp, "with_x", with_x) + ["--batch", manifest(tmp, c["reads"], "route", tsv), "--batch-reads", "2", "-s", "0"], 1)
    index = {n: i for i, (n, _) in enumerate(records)}
    calls = []
    for i, r in enumerate(good):
        marg = marginals_at_sites(open(tsv[r.label]).read(), sorted(listed.get(r.seq_name, [])), K, r.forward)
        calls.append([(index[contig], site, i, 0, 1 if r.forward else 0, tuple(p[l] for l in "ACGT")) for contig, site, p in marg])
    assert sum(len(x) for x in calls) >= 1
    sites = ref.finish(ref.accumulate(calls), 1, [s for _, s in records])
    assert open(m3).read() == ref.marginals_file(sites, [n for n, _ in records])
    arr = as_array(sites)
    assert open(r3).read() == fasta_text([(n, sa.snp_apply_calls(s, arr, i)) for i, (n, s) in enumerate(records)])
    assert open(r3).read() == fasta_text([(n, ref.apply_calls(s, sites, i)) for i, (n, s) in enumerate(records)])


def test_recovery_of_planted_substitutions(tmp_path):
    """A reference with three planted substitutions, 12 synthetic reads of the true sequence: exactly the sites the restatement
    proposes are in the proposals file.  How many of the planted sites come back is a finding about the aligner, so
    a planted site is asserted only where the restatement proposes it."""
    rng = np.random.default_rng(77)
    true = "".join(rng.choice(list("ACGT"), size=420))
    planted = {110: None, 210: None, 310: None}
    wrong = list(true)
    for pos in planted:
        wrong[pos] = "ACGT"[("ACGT".index(true[pos]) + 1 + pos % 3) % 4]
        planted[pos] = true[pos]
    records = [("chr_planted", "".join(wrong))]
    reads = []
    for i in range(12):
        events4, emap = cases.events_for_sequence(true, cases.MODEL_5MER, 900 + i)
        path = str(tmp_path / ("syn%d.npRead" % i))
        cases.write_npread_1d(path, true, emap, events4)
        reads.append(Read("syn%d" % i, path, "cigar: syn%d 0 %d + chr_planted 0 %d + 1 M %d\n" % (i, len(true), len(true), len(true)),
                          "chr_planted", True))
    d, m, p = str(tmp_path / "d"), str(tmp_path / "m.tsv"), str(tmp_path / "p.tsv")
    run(fastas(tmp_path, "planted", records) + ["--batch", manifest(tmp_path, reads, "planted"), "--snp-step", "10", "--snp-dir", d,
                                                "--snp-marginals", m, "--snp-proposals", p], 0)
    sites, table, proposals = restated(calls_from_dir(d, reads, records), records)
    assert open(m).read() == table and open(p).read() == proposals
    by_pos = {s["pos"]: s for s in sites}
    got = {int(l.split("\t")[1]) for l in open(p)}
    back = []
    for pos, letter in planted.items():
        s = by_pos.get(pos)
        if s is not None and s["is_proposal"] and pos in ref.group_sites([(q["pos"], q["delta"]) for q in sites if q["is_proposal"]], 6, True):
            assert pos in got
            back.append((pos, s["called"] == letter, s["delta"]))
    print("planted sites proposed: %d of 3 %r; proposals in all: %d" % (len(back), back, len(got)))


def test_usage_errors(oracle, tmp_path):
    reads, records = the_reads(oracle)
    base = fastas(tmp_path, "u", records) + ["--batch", manifest(tmp_path, reads[1:2], "u")]
    sites = str(tmp_path / "sites.tsv")
    with open(sites, "w") as f:
        f.write("chr_ab\t100\n")
    outs = [str(tmp_path / n) for n in ("m.tsv", "p.tsv", "r.fa")]
    for extra, word in ((["--snp-sites", sites, "--snp-step", "5", "--snp-marginals", outs[0]], "--snp-sites"),
                        (["--snp-step", "5", "--snp-dir", str(tmp_path / "d"), "--snp-proposals", outs[1]], "--snp-proposals"),
                        (["--snp-step", "5", "--snp-marginals", outs[0], "--snp-reference-out", outs[2]], "--snp-reference-out"),
                        (["--snp-sites", sites, "--snp-marginals", outs[0], "--mea"], "--snp-sites"),
                        (["--snp-step", "5"], "--snp-step")):
        pr = subprocess.run([BIN, "-T", cases.MODEL_5MER] + base + extra, capture_output=True, text=True, timeout=120)
        assert pr.returncode != 0 and word in pr.stderr.splitlines()[-1], (extra, pr.stderr[-300:])
        assert not any(os.path.exists(o) for o in outs) and not os.path.exists(str(tmp_path / "d"))
