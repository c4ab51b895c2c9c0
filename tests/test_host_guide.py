"""The guide-alignment stage without a GPU: the band-by-band restatement (tests/guide_ref.py) against the unbanded optimum and
against bwa's alignment of the bundled read, the seed, the exonerate line, the command line's window syntax, the ABI."""
import json
import os
import subprocess

import numpy as np
import pytest

import signalalign_amd as sa

import guide_ref as g
import sa_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")

# share of the base pairs of bwa's alignment (tests/golden/cigars/r9p4_oneD_bwa.json) that the restatement reproduces at the
# default scores and band: 6369 of 6425.  The bar is 0.01 below, the room for alternatives of equal score.
BWA_SHARE_MEASURED = 0.9913


@pytest.mark.parametrize("band", [64, 128, 256])
def test_restatement_reaches_the_unbanded_optimum_on_the_ecoli_read(band):
    read, window = g.ecoli_pair()
    assert len(read) == 6542 and len(window) == 6817
    res = g.banded_cached(read, window, 0, band)
    assert res["score"] == g.unbanded(read, window) and res["status"] == 0


def test_restatement_reaches_the_unbanded_optimum_on_the_zymo_read():
    read, ref = g.zymo_pair()
    assert len(read) == 950 and len(ref) == 897
    for band in (64, 128):
        res = g.banded_cached(read, ref, 0, band)
        assert res["score"] == g.unbanded(read, ref) and res["status"] == 0


def test_restatement_reaches_the_unbanded_optimum_on_the_synthetic_pairs():
    pairs = g.synthetic_pairs()
    assert len(pairs) == 64 and all(200 <= len(w) <= 1500 for _, w in pairs)
    for k, (read, window) in enumerate(pairs):
        res = g.banded_cached(read, window, 0, 128)
        assert res["score"] == g.unbanded(read, window) and res["status"] == 0, k


def test_restatement_reproduces_the_alignment_bwa_made():
    read, window = g.ecoli_pair()
    bwa = json.load(open(os.path.join(cases.GOLDEN, "cigars", "r9p4_oneD_bwa.json")))
    assert bwa["flag"] == 0
    z = np.load(os.path.join(cases.GOLDEN, "expected", "reference_output_ecoli1d.npz"))
    theirs = g.sam_match_pairs(bwa["cigar"], bwa["pos"] - 1 - int(z["first_position"]))
    res = g.banded_cached(read, window, 0, 128)
    mine = g.match_pairs(res["read_start"], res["ref_start"], res["ops"])
    share = len(theirs & mine) / len(theirs)
    print("bwa's base pairs reproduced: %d of %d = %.4f" % (len(theirs & mine), len(theirs), share))
    assert len(theirs) == 6425 and res["read_start"] == 42          # bwa soft-clipped 42S
    assert share >= BWA_SHARE_MEASURED - 0.01
    # the operations add up to the spans
    m = sum(n for t, n in res["ops"] if t == 0)
    assert m + sum(n for t, n in res["ops"] if t == 2) == res["read_end"] - res["read_start"]
    assert m + sum(n for t, n in res["ops"] if t == 1) == res["ref_end"] - res["ref_start"]


def _pad(rng, n):
    return "".join("ACGT"[k] for k in rng.integers(4, size=n))


@pytest.mark.parametrize("padding", [2000, 20000])
def test_seed_places_the_read_inside_a_padded_window(padding):
    """Read base 42 lies on window base 0, so read base 0 belongs at padding - 42.  A band of W cells covers the diagonals within
    W of its centre; the seed must land within W / 2 = 64 of the truth at the default band, which leaves as much again for the
    drift of the alignment itself (the vote is a median over 2000 read bases, along which this read drifts by ~90 diagonals)."""
    read, window = g.ecoli_pair()
    rng = np.random.Generator(np.random.PCG64(padding))
    padded = _pad(rng, padding) + window + _pad(rng, padding)
    s = sa.guide_seed(read, padded, True)
    assert s["found"] and not s["reverse"] and s["votes"] >= 400 and s["hits"] >= s["votes"]
    assert abs(s["diag"] - (padding - 42)) <= 64
    one = sa.guide_seed(read, padded, False)
    assert one == s
    # the reverse-complemented read, strand unknown: the same place in the reverse-complemented window
    rc = sa.guide_seed(read, g.reverse_complement(padded), True)
    assert rc["found"] and rc["reverse"] and rc["diag"] == s["diag"] and rc["votes"] == s["votes"]
    # ... and told to look at the forward strand only, it finds nothing
    assert not sa.guide_seed(read, g.reverse_complement(padded), False)["found"]


def test_seed_reports_a_read_that_is_not_there():
    read, window = g.ecoli_pair()
    rng = np.random.Generator(np.random.PCG64(1))
    s = sa.guide_seed(_pad(rng, 3000), window, True)
    assert not s["found"] and s["diag"] == 0 and not s["reverse"] and s["votes"] < 8
    assert not sa.guide_seed("ACGT", window, True)["found"]          # shorter than a 15-mer
    assert not sa.guide_seed(read, "", True)["found"]


def test_cigar_line_round_trip_on_both_strands(tmp_path):
    ops = [(0, 30), (1, 2), (0, 11), (2, 3), (0, 7)]
    for forward in (True, False):
        line = sa.guide_format_cigar("read_7", 42, 93, "chr:1", 1000, 1050, forward, 77, ops)
        toks = line.split()
        assert toks[:6] == ["cigar:", "read_7", "42", "93", "+", "chr:1"] and toks[9] == "77"
        assert toks[6:9] == (["1000", "1050", "+"] if forward else ["1050", "1000", "-"])
        path = str(tmp_path / ("f.cigar" if forward else "r.cigar"))
        with open(path, "w") as f:
            f.write(line + "\n")
        c = sa.cigar_load(path)
        assert c == dict(contig1="chr:1", contig2="read_7", start1=1000 if forward else 1050, end1=1050 if forward else 1000,
                         start2=42, end2=93, strand1=int(forward), strand2=1, score=77.0, ops=ops)
    assert sa.guide_format_cigar("r", 0, 0, "c", 0, 0, True, 0, []) == "cigar: r 0 0 + c 0 0 + 0"


def test_cigar_line_follows_the_golden_minus_strand_cigar():
    """the line the reference's bwa wrapper wrote (src/signalalign/tests/test_bwaWrapper.py:42-47), loaded and written again"""
    path = os.path.join(cases.GOLDEN, "cigars", "ecoli_minus_strand.cigar")
    c = sa.cigar_load(path)
    assert c["strand1"] == 0 and c["start1"] > c["end1"]
    line = sa.guide_format_cigar(c["contig2"], c["start2"], c["end2"], c["contig1"], c["end1"], c["start1"], False, int(c["score"]), c["ops"])
    assert line == " ".join(open(path).read().split())


def _cli(*args):
    model = os.path.join(cases.GOLDEN, "models", "testModelR9p4_5mer_acegt_template.model")
    return subprocess.run([BIN, "-T", model] + list(args), capture_output=True, text=True, timeout=60)


def test_manifest_window_column_and_option_are_parsed_before_anything_runs(tmp_path):
    """the refusals need no device: a window that cannot be read, a window with --rna, a window next to -p"""
    npread = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")

    def manifest(column):
        path = str(tmp_path / "m.tsv")
        with open(path, "w") as f:
            f.write("r1\t%s\t%s\t%s\n" % (npread, column, str(tmp_path / "o.tsv")))
        return path
    for bad in ("@chrE", "@chrE:100", "@chrE:100-", "@chrE:200-100", "@:1-2", "@chrE:1-2:x", "@chrE:a-b"):
        pr = _cli("-f", "none.fa", "--batch", manifest(bad))
        assert pr.returncode != 0 and "cannot read the guide window " + bad[1:] in pr.stderr, (bad, pr.stderr)
    for good in ("@chrE:100-200", "@chrE:100-200:+", "@chrE:100-200:-", "@gi|1:a:100-200"):
        pr = _cli("-f", "none.fa", "--rna", "--batch", manifest(good))       # accepted as a window, then refused for --rna
        assert pr.returncode != 0 and "guide window (%s) cannot be combined with --rna" % good[1:] in pr.stderr, (good, pr.stderr)
    pr = _cli("-f", "none.fa", "-q", npread, "--guide-window", "chrE:1-2", "-p", "x.cigar")
    assert pr.returncode != 0 and "-p and --guide-window exclude each other" in pr.stderr
    pr = _cli("-f", "none.fa", "-q", npread, "--guide-window", "chrE:1-2", "--guide-band", "100")
    assert pr.returncode != 0 and "--guide-band takes 64, 128, 192 or 256" in pr.stderr
    pr = _cli("-q", npread)
    assert pr.returncode != 0 and "Need to provide input guide alignments" in pr.stderr       # as before
    assert not os.path.exists(str(tmp_path / "o.tsv"))


def test_abi_exports_the_guide_symbols():
    L = sa.lib()
    for name in ("sa_guide_align_batch", "sa_guide_release", "sa_guide_seed", "sa_guide_format_cigar", "sa_guide_to_anchors",
                 "sa_cigar_load"):
        assert hasattr(L, name), name
    header = open(os.path.join(ROOT, "include", "signalalign_hip.h")).read()
    for name in ("sa_guide_job_t", "sa_guide_params_t", "sa_guide_result_t", "sa_guide_align_batch", "sa_guide_release", "sa_guide_seed"):
        assert name in header
    p = sa.guide_params()
    assert (p.match, p.mismatch, p.gap_open, p.gap_extend, p.ambiguous, p.band, p.min_read_fraction) == (2, -4, 4, 2, -1, 128, 0.5)
    # argument checks come before any device use
    with pytest.raises(sa.SaError) as e:
        sa.guide_align_batch([("ACGT", "ACGT")], sa.guide_params(band=100))
    assert e.value.args and "-1" in str(e.value)
