"""signalMachine itself against the file the reference's signalMachine wrote for the bundled R9.4 1-D read: bwa's guide alignment
(tests/golden/cigars/r9p4_oneD_bwa.json) handed over with -p as an exonerate cigar, the window inside a contig, and the reference's
own traceback length, -g 40.  The command line has no switch for the reference-ordered kernels, so the run is the default one
(register kernels) and the bars are theirs: every one of the reference's 11,892 rows, at most two more just under the threshold,
posteriors within 1e-5 of the printed ones (sa_cases.check_reference_rows and tests/test_gpu_reference_outputs.py, which holds the
library to the same file).  The 600 rows of the file that are committed whole (tests/golden/format) are compared column by column."""
import os

import numpy as np
import pytest

import signalalign_amd as sa

import guide_ref as g
import sa_cases as cases
from test_gpu_cli_guide import BIN, MODEL, NPREAD, PRE, _contig, _run, _write_fasta

pytestmark = pytest.mark.gpu

EXCERPT = os.path.join(cases.GOLDEN, "format", "ecoli1D_sm3_6deaf971.forward.head300_tail300.tsv")
CONTIG, LABEL = "gi_ecoli", "6deaf971-6506-4e37-b486-cdf5e9d416ac"       # the reference's, so that whole rows can be compared
# both files print the posterior with six decimals (5e-7 each) and signalMachine prints prob_e7 (1e-7)
CLI_PRINT = 5e-7 + 5e-7 + 1e-7


def _argv(d, out, trace_back):
    q = cases.REFERENCE_RUN
    return [BIN, "-T", MODEL, "-q", NPREAD, "-p", str(d / "bwa.cigar"), "-f", str(d / "ref.fa"), "-n", CONTIG, "-L", LABEL, "-u", out, "-s", "0",
            "-x", str(q["expansion"]), "-D", str(q["threshold"]), "-m", str(q["trim"]), "-g", str(trace_back), "--emission", "twoDist"]


def _rows(path):
    return [l.rstrip("\n").split("\t") for l in open(path)]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, oracle):
    """bwa's alignment as the cigar file --guide-cigars-out would write, the contig pre + window + post: (directory, file's rows)"""
    d = tmp_path_factory.mktemp("reference_output")
    gold, window, _, (s1, e1, s2, e2), ops = cases.reference_output_ecoli1d_inputs(oracle)
    assert window == g.ecoli_pair()[1]
    with open(str(d / "bwa.cigar"), "w") as f:
        f.write(sa.guide_format_cigar(LABEL, s2, e2, CONTIG, PRE + s1, PRE + e1, True, 0, ops) + "\n")
    c = sa.cigar_load(str(d / "bwa.cigar"))
    assert (c["start2"], c["end2"], c["strand2"], c["start1"], c["end1"], c["strand1"]) == (42, 6540, 1, PRE, PRE + 6817, 1) and c["ops"] == ops
    _write_fasta(str(d / "ref.fa"), CONTIG, _contig(window))
    return d, gold


@pytest.fixture(scope="module")
def run_at_40(inputs):
    d, gold = inputs
    out = str(d / "out40.tsv")
    pr = _run(_argv(d, out, cases.REFERENCE_RUN["trace_back"]))
    assert pr.returncode == 0, pr.stderr
    assert "signalAlign - SUCCESS: finished alignment of query %s, exiting" % LABEL in pr.stderr
    return _rows(out)


def test_signalmachine_writes_the_rows_the_reference_wrote(inputs, run_at_40):
    _, gold = inputs
    rows = run_at_40
    assert all(len(r) == 16 and r[0] == CONTIG and r[3] == LABEL and r[4] == "t" for r in rows)
    mine = {(int(r[1]) - PRE, int(r[5])): float(r[12]) for r in rows}
    assert len(mine) == len(rows)
    missing, extra, worst = cases.against_reference_rows(mine, gold)
    print("signalMachine -g 40 against the reference's file: %d rows, %d missing, %d extra, max |dp| %.3g" % (len(rows), len(missing), len(extra), worst))
    assert not missing, (len(missing), missing[:5])
    assert len(extra) <= 2 and all(mine[k] < cases.REFERENCE_RUN["threshold"] + 1e-5 + 5e-7 for k in extra), [(k, mine[k]) for k in extra[:5]]
    assert worst <= 1e-5 + CLI_PRINT, worst
    diag = np.array([int(r[1]) + int(r[5]) for r in rows])
    assert np.all(np.diff(diag) >= 0)


def test_signalmachine_writes_whole_rows_of_the_reference(run_at_40):
    """The reference's first and last 300 rows: k-mers, strand, event index, the seven parameter columns and the path k-mer byte for
    byte, contig and read label as given with -n and -L, the position by its offset, the posterior within the bar."""
    theirs = _rows(EXCERPT)
    assert len(theirs) == 600
    first = min(int(t[1]) for t in theirs)
    z = np.load(os.path.join(cases.GOLDEN, "expected", "reference_output_ecoli1d.npz"))
    assert first == int(z["first_position"])
    mine = {(int(r[1]) - PRE, int(r[5])): r for r in run_at_40}
    same = (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15)
    worst = 0.0
    for t in theirs:
        key = (int(t[1]) - first, int(t[5]))
        assert key in mine, key
        m = mine[key]
        assert [m[c] for c in same] == [t[c] for c in same], (key, m, t)
        worst = max(worst, abs(float(m[12]) - float(t[12])))
    print("signalMachine -g 40, the 600 committed rows: max |dp| %.3g" % worst)
    assert worst <= 1e-5 + CLI_PRINT, worst


def test_the_traceback_option_reaches_the_scheduler(inputs):
    """-g 100 (what the Python driver passes) writes another set of rows: fewer than nine in ten of the reference's"""
    d, gold = inputs
    out = str(d / "out100.tsv")
    pr = _run(_argv(d, out, 100))
    assert pr.returncode == 0, pr.stderr
    mine = {(int(r[1]) - PRE, int(r[5])) for r in _rows(out)}
    found = len(mine & set(gold)) / len(gold)
    print("signalMachine -g 100: found %.4f of the reference's rows" % found)
    assert found < 0.9, found
