"""signalMachine --batch ... --position-profile: the profile file of a run must be byte-identical to the restatement
(profile_ref.py) run over the full TSVs the same run wrote, across three slices with a minus-strand read and refused reads; a run
whose manifest writes no TSV at all must give the same bytes; and the option's usage errors must be refused.  The case builders
are test_gpu_cli_snp_marginals.py's."""
import os
import subprocess

import pytest

import signalalign_amd as sa

import sa_cases as cases
import profile_ref as ref
import test_gpu_cli_snp_marginals as base

pytestmark = pytest.mark.gpu

_TERMS = {}


def _term(u):
    if u not in _TERMS:
        _TERMS[u] = sa.profile_entropy_term(u)
    return _TERMS[u]


@pytest.fixture(scope="module")
def runs(oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("position_profile")
    reads, records = base.the_reads(oracle)
    fa = base.fastas(tmp, "all", records)
    tsv = {r.label: str(tmp / ("%s_full.tsv" % r.label)) for r in reads}
    p1, p2 = str(tmp / "p1.tsv"), str(tmp / "p2.tsv")
    with_tsv = base.run(fa + ["--batch", base.manifest(tmp, reads, "with_tsv", tsv), "--batch-reads", "2", "--position-profile", p1], 1)
    without = base.run(fa + ["--batch", base.manifest(tmp, reads, "without"), "--batch-reads", "2", "--position-profile", p2], 1)
    good = [r for r in reads if not r.label.startswith("bad")]
    return dict(tmp=tmp, reads=reads, good=good, records=records, tsv=tsv, p1=p1, p2=p2, with_tsv=with_tsv, without=without)


def test_profile_equals_the_restatement_over_the_tsvs_of_the_same_run(runs):
    c = runs
    assert "read bad1 skipped" in c["with_tsv"].stderr and "read bad2 skipped" in c["with_tsv"].stderr
    assert "batch: 3 of 5 reads aligned" in c["with_tsv"].stderr
    names, seqs = [n for n, _ in c["records"]], [s for _, s in c["records"]]
    P = ref.Profile(term=_term)
    for r in c["good"]:
        text = open(c["tsv"][r.label]).read()
        # orientation is given here and guessed by the script: on these 1-D files the two agree
        assert ref.is_forward_alignment(text) is r.forward, r.label
        P.add_file(ref.rows_of_tsv(text), r.forward)
    sites = P.finish("ACGT", names, seqs)
    assert open(c["p1"]).read() == ref.file_text(sites, "ACGT", P.letters_seen("ACGT"), names)
    assert len(sites) > 1000 and max(s["read_count"] for s in sites) == 2 and {s["contig"] for s in sites} == {0, 1}
    assert not os.path.exists(c["tsv"]["bad1"]) and not os.path.exists(c["tsv"]["bad2"])
    # where the path letters agree with the reference the whole mass is on the reference letter
    assert any(s["prob"]["ACGT".index(s["ref"])] == 1.0 for s in sites if s["ref"] in "ACGT" and s["kmer_count"])


def test_same_profile_without_any_tsv(runs):
    c = runs
    assert open(c["p2"]).read() == open(c["p1"]).read()
    assert c["without"].stdout == c["with_tsv"].stdout


def test_usage_errors(oracle, tmp_path):
    reads, records = base.the_reads(oracle)
    fa = base.fastas(tmp_path, "u", records)
    batch = ["--batch", base.manifest(tmp_path, reads[1:2], "u")]
    out = str(tmp_path / "p.tsv")
    sites = str(tmp_path / "sites.tsv")
    with open(sites, "w") as f:
        f.write("chr_ab\t100\n")
    cigar = str(tmp_path / "a.cigar")   # (written by the manifest builder)
    single = ["-q", reads[1].npread, "-p", cigar, "-u", str(tmp_path / "single.tsv"), "-n", "chr_ab", "-L", "a"]
    for extra in (batch + ["--twoD", "-C", cases.MODEL_5MER],
                  batch + ["--rna"],
                  batch + ["-s", "1"],
                  batch + ["--snp-step", "5", "--snp-dir", str(tmp_path / "d")],
                  batch + ["--snp-sites", sites, "--snp-marginals", str(tmp_path / "m.tsv")],
                  single):
        pr = subprocess.run([base.BIN, "-T", cases.MODEL_5MER] + fa + extra + ["--position-profile", out], capture_output=True, text=True,
                            timeout=120)
        assert pr.returncode != 0 and "--position-profile" in pr.stderr.splitlines()[-1], (extra, pr.stderr[-300:])
        assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "d")) and not os.path.exists(str(tmp_path / "single.tsv"))
