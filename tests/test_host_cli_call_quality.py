"""signalMachine's refusals around --site-calls-accuracy-quality, none of which needs a device: each new option alone meets the
message the accuracy options have always met, with the usage text before it; the sub-options need the option; a bad grid or gap;
--twoD; -t/-c (the accuracy options' own message); a single read that is not given as raw current.  No case leaves a file behind."""
import os
import subprocess

import pytest

import sa_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
MODEL = os.path.join(cases.GOLDEN, "models", "testModelR9p4_5mer_acegt_template.model")
NPREAD = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")

ONE = ["-T", MODEL, "-q", NPREAD, "-p", "none.cigar", "-f", "none.fa", "-n", "chr"]
ACC = ["--site-calls-accuracy", "{tmp}/acc.tsv", "--site-calls-truth", "none.truth"]
QUALITY = ACC + ["--site-calls-accuracy-quality", "{tmp}/quality.tsv"]
NEEDS_ACCURACY = "signalMachine: --site-calls-truth* and --site-calls-accuracy-* need --site-calls-accuracy <file>"
NEEDS_QUALITY = "signalMachine: --site-calls-accuracy-quality-* need --site-calls-accuracy-quality <file>"
BAD_GRID = "signalMachine: --site-calls-accuracy-quality-bins takes lo,width,n with width >= 1 and 1 <= n <= 1024, -min-gap n >= 0"

CASES = {
    # each new option alone: the pinned message of the accuracy group
    "quality_alone": (ONE + ["--site-calls-accuracy-quality", "{tmp}/quality.tsv"], NEEDS_ACCURACY),
    "calls_alone": (ONE + ["--site-calls-accuracy-quality-calls", "{tmp}/calls.tsv"], NEEDS_ACCURACY),
    "bins_alone": (ONE + ["--site-calls-accuracy-quality-bins", "-100,10,20"], NEEDS_ACCURACY),
    "min_gap_alone": (ONE + ["--site-calls-accuracy-quality-min-gap", "5"], NEEDS_ACCURACY),
    # the sub-options need the option
    "calls_without_quality": (ONE + ACC + ["--site-calls-accuracy-quality-calls", "{tmp}/calls.tsv"], NEEDS_QUALITY),
    "bins_without_quality": (ONE + ACC + ["--site-calls-accuracy-quality-bins", "-100,10,20"], NEEDS_QUALITY),
    "min_gap_without_quality": (ONE + ACC + ["--site-calls-accuracy-quality-min-gap", "5"], NEEDS_QUALITY),
    # the grid and the gap
    "bins_malformed": (ONE + QUALITY + ["--site-calls-accuracy-quality-bins", "-100,10"], BAD_GRID),
    "bins_trailing": (ONE + QUALITY + ["--site-calls-accuracy-quality-bins", "-100,10,20x"], BAD_GRID),
    "bin_width_zero": (ONE + QUALITY + ["--site-calls-accuracy-quality-bins", "-100,0,20"], BAD_GRID),
    "no_bins": (ONE + QUALITY + ["--site-calls-accuracy-quality-bins", "-100,10,0"], BAD_GRID),
    "too_many_bins": (ONE + QUALITY + ["--site-calls-accuracy-quality-bins", "-100,10,1025"], BAD_GRID),
    "min_gap_negative": (ONE + QUALITY + ["--site-calls-accuracy-quality-min-gap", "-1"], BAD_GRID),
    # the runs it does not take
    "two_d": (ONE + QUALITY + ["--twoD", "-C", MODEL], "signalMachine: --site-calls-accuracy-quality does not take --twoD runs"),
    "expectations": (ONE + QUALITY + ["-t", "{tmp}/t.expectations"],
                     "signalMachine: --site-calls / --site-calls-aggregate / --site-calls-accuracy need the alignment mode, not -t/-c"),
    "not_raw": (ONE + QUALITY,
                "signalMachine: --site-calls-accuracy-quality needs a read given as raw current: an .npRead has no raw starts"),
    # two rules broken: the accuracy group's own rules come first, as they always have
    "first_of_accuracy_truth_and_quality": (ONE + ["--site-calls-accuracy", "{tmp}/acc.tsv", "--site-calls-accuracy-quality", "{tmp}/q.tsv",
                                                   "--twoD", "-C", MODEL],
                                            "signalMachine: --site-calls-accuracy needs --site-calls-truth <file> or --site-calls-truth-reads <file>"),
}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    d = tmp_path_factory.mktemp("call_quality_refusals") / "out"
    os.mkdir(d)
    return str(d)


def run(args, tmp):
    argv = [a.format(tmp=tmp) if "{" in a else a for a in args]
    pr = subprocess.run([BIN] + argv, capture_output=True, text=True, timeout=60, cwd=os.path.dirname(tmp))
    return pr.returncode, pr.stdout, pr.stderr


@pytest.fixture(scope="module")
def usage(tmp):
    status, _, stderr = run(["--help"], tmp)
    assert status == 1 and len(stderr.splitlines()) == 103            # (the usage text has not grown a line)
    assert "--site-calls-accuracy-quality <file>" in stderr and "-quality-calls <file>" in stderr
    assert "-quality-bins lo,width,n (-10000,100,200)" in stderr and "-quality-min-gap n (30)" in stderr
    return stderr


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusal(name, tmp, usage):
    args, message = CASES[name]
    status, stdout, stderr = run(args, tmp)
    assert status == 1 and stdout == ""
    assert stderr == usage + message + "\n"                            # the usage text, then the message verbatim, nothing else
    assert os.listdir(tmp) == [], "a refused command line left a file behind"
