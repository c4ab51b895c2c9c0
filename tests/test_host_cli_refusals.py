"""signalMachine's refusals: every command line that main() turns down before anything needs a device.  One case per refusal; for
each the exit status (1), the last line of stderr verbatim and whether the usage text precedes it are pinned against
golden/cli_refusals/expected.json, which holds what the binary printed before its option checks became a table (the order of the
checks is part of the command line's contract: the first refused rule wins, which the cases that break two rules pin).  No case
leaves a file behind.  Paths that need not exist are relative names, so the messages that quote them are the same everywhere."""
import json
import os
import subprocess

import numpy as np
import pytest

from signalalign_amd import rawio

import sa_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
EXPECTED = os.path.join(cases.GOLDEN, "cli_refusals", "expected.json")
MODEL = os.path.join(cases.GOLDEN, "models", "testModelR9p4_5mer_acegt_template.model")
NPREAD = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")
USAGE_LINES = 104       # lines of stderr of a refusal that prints the usage text first; 1 without

T = ["-T", MODEL]
ONE = T + ["-q", NPREAD, "-p", "none.cigar", "-f", "none.fa", "-n", "chr"]      # a single read that passes the first checks
TWO_D = ["--twoD", "-C", MODEL]
MAN, MAN_EXPECT, MAN_MIXED, MAN_AT, MAN_WINDOW, MAN_POST, MAN_RAW = ("{%s}" % n for n in
                                                                     ("man", "man_expect", "man_mixed", "man_at", "man_window", "man_post", "man_raw"))
BATCH = T + ["--batch", MAN, "-f", "none.fa"]                                    # ... and a one-line manifest, posteriors '-'
SNP = ["--snp-step", "4", "--snp-dir", "{tmp}/snp"]
ACC = ["--site-calls-accuracy", "{tmp}/acc.tsv", "--site-calls-truth", "none.truth"]
MIX = ["--train-mixture-motifs", "CCAGG:CEAGG", "--train-mixture-distances", "{tmp}/dist.tsv"]

CASES = {
    # the option parser itself
    "help": ["--help"],
    "unknown_option": T + ["--no-such-option"],
    "raw_detector_malformed": T + ["--raw-detector", "3,6,x"],
    "raw_detector_window_zero": T + ["--raw-detector", "0,6,1.4,9.0,0.2"],
    "emission_unknown": T + ["--emission", "other"],
    # before the reads are loaded
    "profile_needs_batch": ONE + ["--position-profile", "{tmp}/p.tsv"],
    "no_template_model": ["-p", "none.cigar"],
    "no_complement_model": T + ["--twoD", "-p", "none.cigar"],
    "both_formats_need_second_file": ONE + ["-s", "3"],
    "cigar_and_window": ONE + ["--guide-window", "chr:1-2"],
    "locate_and_cigar": ONE + ["--guide-locate"],
    "locate_and_window": T + ["-f", "none.fa", "--guide-locate", "--guide-window", "chr:1-2"],
    "locate_and_manifest": BATCH + ["--guide-locate"],
    "no_guide": T + ["-q", NPREAD],
    "guide_band": ONE + ["--guide-band", "100"],
    "guide_band_too_wide": ONE + ["--guide-band", "320"],
    # loading the reads
    "manifest_unreadable": T + ["--batch", "none.manifest"],
    "manifest_mixes_modes": T + ["--batch", MAN_MIXED, "-f", "none.fa"],
    "window_needs_reference": T + ["-q", NPREAD, "--guide-window", "chr:1-2"],
    "locate_needs_reference": T + ["-q", NPREAD, "--guide-locate"],
    "cigar_probe_no_file": T + ["-q", NPREAD, "-p", "none.cigar"],
    "cigar_probe_then_reference": T + ["-q", NPREAD, "-p", "{cigar}", "-f", "none.fa"],
    "cigar_probe_then_name": T + ["-q", NPREAD, "-p", "{cigar}", "-n", "chr"],
    "locate_rna": T + ["-q", NPREAD, "-f", "none.fa", "--guide-locate", "--rna"],
    "manifest_locate_rna": T + ["--batch", MAN_AT, "-f", "none.fa", "--rna"],
    "window_rna": T + ["-q", NPREAD, "-f", "none.fa", "--guide-window", "chr:1-2", "--rna"],
    "manifest_window_rna": T + ["--batch", MAN_WINDOW, "-f", "none.fa", "--rna"],
    "window_malformed": T + ["-q", NPREAD, "-f", "none.fa", "--guide-window", "chr"],
    "window_empty_range": T + ["-q", NPREAD, "-f", "none.fa", "--guide-window", "chr:5-5"],
    "raw_two_d": T + ["-q", "{raw}", "-f", "none.fa", "--guide-locate"] + TWO_D,
    "raw_complement_model": T + ["-q", "{raw}", "-f", "none.fa", "--guide-locate", "-C", MODEL],
    "raw_rna": T + ["-q", "{raw}", "-p", "none.cigar", "-f", "none.fa", "-n", "chr", "--rna"],
    "raw_hdp": T + ["-q", "{raw}", "-f", "none.fa", "--guide-locate", "--sm3Hdp"],
    "raw_nhdp": T + ["--batch", MAN_RAW, "-f", "none.fa", "-v", "none.nhdp"],
    "npread_out_not_creatable": ONE + ["--npread-out", "none/dir"],
    "guide_cigars_out_not_creatable": ONE + ["--guide-cigars-out", "none/dir"],
    # the options against each other
    "two_dist_nhdp": ONE + ["--emission", "twoDist", "-v", "none.nhdp"],
    "two_dist_sm3hdp": ONE + ["--emission", "twoDist", "--sm3Hdp"],
    "two_dist_expectations": ONE + ["--emission", "twoDist", "-t", "{tmp}/t.expectations"],
    "two_dist_manifest_expectations": T + ["--batch", MAN_EXPECT, "-f", "none.fa", "--emission", "twoDist"],
    "mixture_motifs_alone": ONE + ["--train-mixture-motifs", "CCAGG:CEAGG"],
    "mixture_output_alone": ONE + ["--train-mixture-template-model", "{tmp}/m.model"],
    "train_mea": ONE + ["--train-assignments", "{tmp}/a.tsv", "--mea"],
    "train_expectations": ONE + ["--train-template-model", "{tmp}/t.model", "-t", "{tmp}/t.expectations"],
    "train_complement_one_d": ONE + ["--train-complement-model", "{tmp}/c.model"],
    "mixture_complement_one_d": ONE + ["--train-mixture-motifs", "CCAGG:CEAGG", "--train-mixture-complement-model", "{tmp}/c.model"],
    "train_max_assignments": ONE + ["--train-assignments", "{tmp}/a.tsv", "--train-max-assignments", "0"],
    "train_min_prob": ONE + ["--train-assignments", "{tmp}/a.tsv", "--train-min-prob", "1.5"],
    "accuracy_curves_alone": ONE + ["--site-calls-accuracy-curves", "{tmp}/c.tsv"],
    "accuracy_truth_alone": ONE + ["--site-calls-truth", "none.truth"],
    "accuracy_truth_reads_alone": ONE + ["--site-calls-truth-reads", "none.labels"],
    "accuracy_bins_alone": ONE + ["--site-calls-accuracy-bins", "10"],
    "accuracy_threshold_alone": ONE + ["--site-calls-accuracy-threshold", "0.5"],
    "accuracy_without_truth": ONE + ["--site-calls-accuracy", "{tmp}/acc.tsv"],
    "accuracy_bins_zero": ONE + ACC + ["--site-calls-accuracy-bins", "0"],
    "accuracy_threshold_nan": ONE + ACC + ["--site-calls-accuracy-threshold", "nan"],
    "accuracy_two_d_mea": ONE + ACC + TWO_D + ["--mea"],
    "accuracy_two_d_deviation": ONE + ACC + TWO_D + ["--guide-deviation", "{tmp}/dev.tsv"],
    "expectations_site_calls": ONE + ["-t", "{tmp}/t.expectations", "--site-calls"],
    "expectations_aggregate": ONE + ["-c", "{tmp}/c.expectations", "--site-calls-aggregate", "{tmp}/agg.tsv"],
    "expectations_accuracy": T + ["--batch", MAN_EXPECT, "-f", "none.fa"] + ACC,
    "proposals_without_marginals": ONE + SNP + ["--snp-proposals", "{tmp}/prop.tsv"],
    "sites_and_step": ONE + SNP + ["--snp-sites", "none.sites", "--snp-marginals", "{tmp}/m.tsv"],
    "reference_out_without_sites": ONE + SNP + ["--snp-reference-out", "{tmp}/fixed.fa"],
    "sites_without_marginals": ONE + ["--snp-sites", "none.sites"],
    "sites_and_dir": ONE + ["--snp-sites", "none.sites", "--snp-marginals", "{tmp}/m.tsv", "--snp-dir", "{tmp}/snp"],
    "marginals_alone": ONE + ["--snp-marginals", "{tmp}/m.tsv"],
    "profile_two_d": BATCH + ["--position-profile", "{tmp}/p.tsv"] + TWO_D,
    "profile_rna": BATCH + ["--position-profile", "{tmp}/p.tsv", "--rna"],
    "profile_variant_caller_format": BATCH + ["--position-profile", "{tmp}/p.tsv", "-s", "1"],
    "profile_snp_step": BATCH + ["--position-profile", "{tmp}/p.tsv"] + SNP,
    "profile_snp_sites": BATCH + ["--position-profile", "{tmp}/p.tsv", "--snp-sites", "none.sites", "--snp-marginals", "{tmp}/m.tsv"],
    "profile_expectations": T + ["--batch", MAN_EXPECT, "-f", "none.fa", "--position-profile", "{tmp}/p.tsv"],
    "profile_without_reference": T + ["--batch", MAN, "--position-profile", "{tmp}/p.tsv"],
    "deviation_events_alone": ONE + ["--guide-deviation-events", "{tmp}/ev.tsv"],
    "deviation_threshold": ONE + ["--guide-deviation", "{tmp}/dev.tsv", "--guide-deviation-threshold", "-1"],
    "deviation_expectations": ONE + ["--guide-deviation", "{tmp}/dev.tsv", "-t", "{tmp}/t.expectations"],
    "deviation_train": ONE + ["--guide-deviation", "{tmp}/dev.tsv", "--train-assignments", "{tmp}/a.tsv"],
    "deviation_snp_step": ONE + ["--guide-deviation", "{tmp}/dev.tsv"] + SNP,
    "deviation_snp_dir": ONE + ["--guide-deviation", "{tmp}/dev.tsv", "--snp-dir", "{tmp}/snp"],
    "deviation_snp_sites": ONE + ["--guide-deviation", "{tmp}/dev.tsv", "--snp-sites", "none.sites", "--snp-marginals", "{tmp}/m.tsv"],
    "snp_step_zero": ONE + ["--snp-step", "0", "--snp-dir", "{tmp}/snp"],
    "snp_step_not_a_number": ONE + ["--snp-step", "x", "--snp-dir", "{tmp}/snp"],
    "snp_dir_alone": ONE + ["--snp-dir", "{tmp}/snp"],
    "snp_step_without_dir": ONE + ["--snp-step", "4"],
    "marginals_two_d": ONE + SNP + TWO_D + ["--snp-marginals", "{tmp}/m.tsv"],
    "snp_step_expectations": ONE + SNP + ["-t", "{tmp}/t.expectations"],
    "snp_sites_expectations": ONE + ["--snp-sites", "none.sites", "--snp-marginals", "{tmp}/m.tsv", "-t", "{tmp}/t.expectations"],
    "snp_step_mea": ONE + SNP + ["--mea"],
    "snp_sites_mea": ONE + ["--snp-sites", "none.sites", "--snp-marginals", "{tmp}/m.tsv", "--mea"],
    "snp_step_site_calls": ONE + SNP + ["--site-calls"],
    "snp_step_aggregate": ONE + SNP + ["--site-calls-aggregate", "{tmp}/agg.tsv"],
    "snp_step_accuracy": ONE + SNP + ACC,
    "snp_step_train": ONE + SNP + ["--train-assignments", "{tmp}/a.tsv"],
    "snp_step_posteriors": ONE + SNP + ["-u", "{tmp}/o.tsv"],
    "snp_step_second_posteriors": ONE + SNP + ["-i", "{tmp}/o2.tsv"],
    "snp_step_manifest_posteriors": T + ["--batch", MAN_POST, "-f", "none.fa"] + SNP,
    "snp_sites_posteriors": ONE + ["--snp-sites", "none.sites", "--snp-marginals", "{tmp}/m.tsv", "-u", "{tmp}/o.tsv"],
    # models and what is read before the first slice
    "nhdp_complement_missing": ONE + TWO_D + ["-v", "none.nhdp"],
    "nhdp_template_missing": ONE + ["-w", "none.nhdp"],
    "sm3hdp_without_nhdp": ONE + ["--sm3Hdp"],
    "template_model_not_found": ["-T", "none.model", "-q", NPREAD, "-p", "none.cigar", "-f", "none.fa", "-n", "chr"],
    "complement_model_not_found": ONE + ["--twoD", "-C", "none.model"],
    "nhdp_not_found": ONE + ["-v", "none.nhdp"],
    "mixture_list_trailing_comma": ONE + ["--train-mixture-motifs", "CCAGG:CEAGG,", "--train-mixture-distances", "{tmp}/dist.tsv"],
    "mixture_list_empty": ONE + ["--train-mixture-motifs", "", "--train-mixture-distances", "{tmp}/dist.tsv"],
    "mixture_item_without_colon": ONE + ["--train-mixture-motifs", "CCAGG", "--train-mixture-distances", "{tmp}/dist.tsv"],
    "mixture_letter_outside_alphabet": ONE + ["--train-mixture-motifs", "CCZGG:CEZGG", "--train-mixture-distances", "{tmp}/dist.tsv"],
    "mixture_pair_does_not_differ": ONE + ["--train-mixture-motifs", "CCAGG:CCAGG", "--train-mixture-distances", "{tmp}/dist.tsv"],
    "ambiguity_table_not_found": ONE + ["-a", "none.ambig"],
    "snp_dir_not_creatable": ONE + ["--snp-step", "4", "--snp-dir", "none/dir"],
    "marginals_reference_unreadable": ONE + ["--snp-step", "4", "--snp-marginals", "{tmp}/m.tsv"],
    "profile_reference_unreadable": BATCH + ["--position-profile", "{tmp}/p.tsv"],
    "truth_unreadable": ONE + ACC,
    "truth_malformed": ONE + ["--site-calls-accuracy", "{tmp}/acc.tsv", "--site-calls-truth", "{bad_truth}"],
    "truth_reads_unreadable": ONE + ["--site-calls-accuracy", "{tmp}/acc.tsv", "--site-calls-truth-reads", "none.labels"],
    "truth_reads_malformed": ONE + ["--site-calls-accuracy", "{tmp}/acc.tsv", "--site-calls-truth-reads", "{bad_truth}"],
    "deviation_not_writable": ONE + ["--guide-deviation", "none/dev.tsv"],
    # the single read's own files (the host side of its slice; a manifest's read would be skipped instead)
    "cigar_not_found": ONE,
    "npread_not_found": T + ["-q", "none.npRead", "-p", "{cigar}", "-f", "none.fa", "-n", "chr"],
    "reference_not_found": T + ["-q", NPREAD, "-p", "{cigar}", "-f", "none.fa", "-n", "chr"],
    # two rules broken: the first one checked wins
    "first_of_profile_and_model": ["--position-profile", "{tmp}/p.tsv", "-p", "none.cigar"],
    "first_of_cigar_window_and_band": ONE + ["--guide-window", "chr:1-2", "--guide-band", "100"],
    "first_of_manifest_and_two_dist": T + ["--batch", "none.manifest", "--emission", "twoDist", "-v", "none.nhdp"],
    "first_of_accuracy_and_proposals": ONE + ["--site-calls-truth", "none.truth", "--snp-proposals", "{tmp}/prop.tsv"],
    "first_of_train_and_deviation_and_snp": ONE + SNP + ["--guide-deviation", "{tmp}/dev.tsv", "--train-assignments", "{tmp}/a.tsv"],
    "first_of_expectations_calls_and_profile": T + ["--batch", MAN_EXPECT, "-f", "none.fa", "--site-calls", "--position-profile", "{tmp}/p.tsv", "-s", "1"],
    "first_of_mixture_and_accuracy": ONE + ["--train-mixture-motifs", "CCAGG:CEAGG", "--site-calls-accuracy-bins", "10"],
    "first_of_options_and_models": ["-T", "none.model", "-q", NPREAD, "-p", "none.cigar", "-f", "none.fa", "-n", "chr", "--snp-step", "4"],
    "first_of_window_rna_and_raw": T + ["-q", "{raw}", "-f", "none.fa", "--guide-window", "chr:1-2", "--rna"],
}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """what the cases' placeholders stand for: manifests of one bundled read, a cigar file, a raw-read file, a bad truth file"""
    d = tmp_path_factory.mktemp("refusals")
    out = {"tmp": str(d / "out")}
    os.mkdir(out["tmp"])
    for name, lines in (("man", ["r1\t%s\tnone.cigar\t-\n" % NPREAD]),
                        ("man_post", ["r1\t%s\tnone.cigar\t%s/o.tsv\n" % (NPREAD, out["tmp"])]),
                        ("man_expect", ["r1\t%s\tnone.cigar\t-\t-\t-\t%s/t.expectations\n" % (NPREAD, out["tmp"])]),
                        ("man_mixed", ["r1\t%s\tnone.cigar\t-\t-\t-\t%s/t.expectations\n" % (NPREAD, out["tmp"]), "r2\t%s\tnone.cigar\t-\n" % NPREAD]),
                        ("man_at", ["r1\t%s\t@\t-\n" % NPREAD]),
                        ("man_window", ["r1\t%s\t@chr:1-2\t-\n" % NPREAD]),
                        ("man_raw", ["r1\t%s\t@\t-\n" % str(d / "read.saraw")])):
        out[name] = str(d / (name + ".tsv"))
        open(out[name], "w").writelines(lines)
    out["cigar"] = str(d / "guide.cigar")
    open(out["cigar"], "w").write("cigar: r1 0 100 + chr 0 100 + 1 M 100\n")
    out["raw"] = str(d / "read.saraw")
    rawio.write_raw(out["raw"], raw=np.zeros(64, dtype=np.int16), digitisation=8192.0, offset=0.0, range=1400.0, sample_rate=4000.0,
                    start_time=0, sequence="ACGTACGTACGT")
    out["bad_truth"] = str(d / "bad_truth.tsv")
    open(out["bad_truth"], "w").write("one two three four five six\n")
    return out


def run_case(args, files, binary=BIN):
    """(exit status, stdout, stderr) of one case, run where its relative paths name nothing; the directories read as {dir}, {root}"""
    argv = [a.format(**files) if "{" in a else a for a in args]
    there = os.path.dirname(files["tmp"])
    pr = subprocess.run([binary] + argv, capture_output=True, text=True, timeout=60, cwd=there)
    return (pr.returncode,) + tuple(t.replace(binary, "signalMachine").replace(there, "{dir}").replace(ROOT, "{root}") for t in (pr.stdout, pr.stderr))


def collapse_usage(stderr, usage):
    """stderr with the usage text, where it holds it, written as one line {usage}"""
    return stderr.replace(usage, "{usage}\n")


@pytest.fixture(scope="module")
def usage(files):
    status, _, stderr = run_case(["--help"], files)
    assert status == 1 and len(stderr.splitlines()) == USAGE_LINES - 1
    return stderr


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusal(name, files, usage):
    want = json.load(open(EXPECTED))[name]
    status, stdout, stderr = run_case(CASES[name], files)
    got = collapse_usage(stderr, usage)
    assert status == 1
    assert got.splitlines()[-1:] == want["stderr"].splitlines()[-1:]                   # the message
    assert ("{usage}" in got.splitlines()[:-1]) == ("{usage}" in want["stderr"].splitlines()[:-1])   # ... and whether the usage text precedes it
    assert got == want["stderr"] and stdout == want["stdout"]                           # every other line, too
    assert os.listdir(files["tmp"]) == [], "a refused command line left a file behind"


def test_every_case_has_its_expectation():
    assert sorted(json.load(open(EXPECTED))) == sorted(CASES)
