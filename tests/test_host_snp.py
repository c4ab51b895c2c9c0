"""CPU checks of the host pieces of single-nucleotide probabilities (signalMachine --snp-step): the periodic substitution of a
reference window, the site window of call_methyls with a step offset, and the per-read file the merge writes.  Each is held
against a restatement written here."""
import os
import random

import pytest

import signalalign_amd as sa


def _periodic(record, step, phase, letter):
    # the whole record with `letter` at every index = phase (mod step), upper-cased
    chars = list(record)
    for i in range(phase, len(chars), step):
        chars[i] = letter
    return "".join(chars).upper()


def _revcomp(s):
    pair = {"A": "T", "C": "G", "G": "C", "T": "A"}
    return "".join(pair.get(c, c) for c in reversed(s))


@pytest.mark.parametrize("step", [1, 3, 5, 10])
def test_substitute_matches_the_record_cut_into_windows(step):
    rng = random.Random(step)
    record = "".join(rng.choice("ACGTacgt") for _ in range(400))
    for phase in range(step):
        whole = _periodic(record, step, phase, "X")
        for lo, hi in ((0, 399), (17, 250), (133, 134), (391, 399)):
            window = record[lo:hi + 1]
            # forward: the window's first letter sits at contig coordinate lo
            assert sa.snp_substitute(window, lo, False, step, phase) == whole[lo:hi + 1]
            # reversed: the target runs backwards along the contig (a backward-mapped read's template, a complement strand)
            target = _revcomp(window.upper())
            assert sa.snp_substitute(target, hi, True, step, phase) == _revcomp(whole[lo:hi + 1])


def test_substitute_rejects_bad_arguments():
    for step, phase in ((0, 0), (5, 5), (5, -1)):
        with pytest.raises(sa.SaError):
            sa.snp_substitute("ACGT", 0, False, step, phase)


def _window(lo_index, hi_index, step):
    lo, hi = lo_index - step, hi_index + step
    while lo % step:
        lo -= 1
    while hi % step:
        hi += 1
    return lo, hi


@pytest.mark.parametrize("step", [1, 2, 3, 5, 6, 10, 13])
def test_site_window(step):
    rng = random.Random(100 + step)
    for _ in range(200):
        a = rng.randrange(0, 5000)
        b = a + rng.randrange(0, 800)
        assert sa.snp_site_window(a, b, step) == _window(a, b, step)


def test_site_window_clips_only_below_k():
    # The last row's k-mer, at reference_index max, covers max .. max + k - 1; the window ends at max + step raised to a multiple
    # of step.  With k = 5: (step, max) -> (window end, the covered positions at or past it)
    k = 5
    cases = [(3, 102, 105, [105, 106]), (3, 100, 105, []), (4, 100, 104, [104]), (4, 101, 108, []), (2, 101, 104, [104, 105]),
             (1, 100, 101, [101, 102, 103, 104])]
    for step, mx, end, clipped in cases:
        lo, hi = sa.snp_site_window(50, mx, step)
        assert hi == end, (step, mx)
        assert [q for q in range(mx, mx + k) if q >= hi] == clipped, (step, mx)
        # a clipped position is no site of its phase; the last position below the end is
        for q in clipped:
            assert q not in range(lo + q % step, hi, step)
        assert (hi - 1) in range(lo + (hi - 1) % step, hi, step)
    # from step = k on nothing a row covers is cut off, at any largest index
    for step in (5, 6, 10):
        for mx in range(100, 140):
            assert sa.snp_site_window(50, mx, step)[1] >= mx + k, (step, mx)


def _expected_file(fast5, read_id, contig, backward, sites):
    lines = sorted(sites, key=lambda s: s[0])   # stable: t before c at one position, file order otherwise
    out = ["## fast5_input: %s\n" % fast5, "## read_id: %s\n" % read_id, "## contig: %s\n" % (contig if sites else ""),
           "## strand: %s\n" % ("complement" if backward else "template"), "#CHROM\tPOS\tpA\tpC\tpG\tpT\n"]
    for pos, _strand, p in lines:
        cols = [p[3], p[2], p[1], p[0]] if backward else list(p)
        out.append("\t".join([contig, str(pos)] + [str(float(v)) for v in cols]) + "\n")
    return "".join(out)


def test_write_read_header_order_and_repr(tmp_path):
    sites = [
        # step file 0: template sites, then complement sites
        (20, 0, (0.25, 0.25, 0.5, 0.0)), (30, 0, (1.0, 0.0, 0.0, 0.0)), (20, 1, (5e-05, 0.99995, 0.0, 0.0)),
        # step file 1
        (11, 0, (0.1, 0.2, 0.30000000000000004, 0.4)), (31, 0, (0.123456789, 1e-07, 0.876543111, 0.0)),
        (11, 1, (0.3333333333333333, 0.6666666666666666, 0.0, 0.0)), (31, 1, (0.0, 0.0, 0.0, 1.0)),
    ]
    for backward in (False, True):
        path = str(tmp_path / ("r%d.tsv" % backward))
        sa.snp_write_read(path, "read.npRead", "read_label", "chr_x", backward, sites)
        got = open(path).read()
        assert got == _expected_file("read.npRead", "read_label", "chr_x", backward, sites)
    # the repr of the corner values, as Python's str(float) prints them
    text = open(str(tmp_path / "r0.tsv")).read()
    assert "\t1.0\t0.0\t0.0\t0.0\n" in text and "\t5e-05\t0.99995\t" in text and "\t1e-07\t" in text
    # t before c at one position
    rows = [l.split("\t") for l in text.splitlines() if not l.startswith("#")]
    assert [r[1] for r in rows] == ["11", "11", "20", "20", "30", "31", "31"]
    assert rows[0][2:] == ["0.1", "0.2", "0.30000000000000004", "0.4"]


def test_write_read_without_sites_is_only_the_header(tmp_path):
    path = str(tmp_path / "empty.tsv")
    sa.snp_write_read(path, "x.npRead", "lbl", "contig1", False, [])
    assert open(path).read() == ("## fast5_input: x.npRead\n## read_id: lbl\n## contig: \n## strand: template\n"
                                 "#CHROM\tPOS\tpA\tpC\tpG\tpT\n")
