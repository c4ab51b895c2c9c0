"""signalMachine --site-calls-accuracy-quality on the bundled read 108 given as raw current, against its window with X written over
a few dozen reference positions: the quality file and the calls file agree with each other and with the run's own .calls, .mea and
band files joined with the raw starts of sa.npread_from_raw_batch through the restatement's rules (call_quality_ref.py); every
other output is what a run without the options writes; in a manifest only the raw read gets quality lines."""
import os

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import rawio

import call_quality_ref as ref
import guide_ref as g
from test_gpu_cli_guide import BIN, MODEL, PRE, _contig, _write_fasta
from test_gpu_cli_raw import _argv, _run
from test_gpu_event_detect import job_of
from test_host_event_detect import dna_sequence

pytestmark = pytest.mark.gpu

GRID = (-4000, 50, 160, 20)          # bin_lo, bin_width, n_bins, min_gap


@pytest.fixture(scope="module")
def quality_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("quality_cli")
    _, window = g.ecoli_pair()
    w = list(window)
    cs = [i for i in range(200, len(w) - 200) if w[i] == "C"]
    for i in cs[::max(1, len(cs) // 60)][:60]:
        w[i] = "X"
    fasta = str(d / "ref.fa")
    _write_fasta(fasta, "chrE", _contig("".join(w)))
    spec = "chrE:%d-%d" % (PRE - 50, PRE + len(window) + 100)
    raw = str(d / "read108.saraw")
    rawio.write_raw(raw, sequence=dna_sequence(), **job_of("read108_dna"))
    amb = str(d / "ce.ambig")
    open(amb, "w").write("X\tCE\n")
    common = ["--guide-window", spec, "-a", amb, "--site-calls", "--mea", "--npread-out", str(d / "np")]
    # a first run for the sites: the truth names every third one C, every third one E and leaves the rest out
    first = str(d / "first.tsv")
    pr = _run(_argv(raw, fasta, first, "read108", *common))
    assert pr.returncode == 0, pr.stderr
    sites = [l.split("\t") for l in open(first + ".calls").read().splitlines()]
    assert len(sites) > 30
    truth = str(d / "truth.tsv")
    named = []
    with open(truth, "w") as f:
        for i, s in enumerate(sites):
            if i % 3 < 2:
                f.write("%s\t%s\t%s\tC\t%s\n" % (s[1], s[2], s[4], "CE"[i % 3]))
                named.append(float(s[6 + i % 3]))
    threshold = float(np.median(named))        # the calls' own median: at least one call is not above it
    acc = ["--site-calls-accuracy", "{}", "--site-calls-truth", truth, "--site-calls-accuracy-threshold", repr(threshold)]
    plain = str(d / "plain.tsv")
    pr = _run(_argv(raw, fasta, plain, "read108", *common, *[a.format(str(d / "plain.acc")) for a in acc]))
    assert pr.returncode == 0, pr.stderr
    out = str(d / "q.tsv")
    pr = _run(_argv(raw, fasta, out, "read108", *common, *[a.format(str(d / "q.acc")) for a in acc], "--signal-labels", str(d / "lab"),
                    "--signal-labels-bands", "--signal-labels-kmer-index", "0", "--site-calls-accuracy-quality", str(d / "quality.tsv"),
                    "--site-calls-accuracy-quality-calls", str(d / "quality_calls.tsv"), "--site-calls-accuracy-quality-bins",
                    "%d,%d,%d" % GRID[:3], "--site-calls-accuracy-quality-min-gap", str(GRID[3])))
    assert pr.returncode == 0, pr.stderr
    np_read = sa.npread_from_raw_batch(sa.Model.load(MODEL), [job_of("read108_dna")], [dna_sequence()])[0]
    assert np_read["status"] == 0
    return d, fasta, spec, raw, amb, truth, sites, plain, out, np_read, threshold


def test_every_other_output_is_what_a_run_without_the_options_writes(quality_run):
    d, fasta, spec, raw, amb, truth, sites, plain, out, np_read, THRESHOLD = quality_run
    for suffix in ("", ".calls", ".mea"):
        assert open(out + suffix, "rb").read() == open(plain + suffix, "rb").read() and os.path.getsize(out + suffix) > 1000
    assert (d / "q.acc").read_bytes() == (d / "plain.acc").read_bytes() and len((d / "q.acc").read_text().splitlines()) > 2


def test_quality_and_calls_files(quality_run):
    d, fasta, spec, raw, amb, truth, sites, plain, out, np_read, THRESHOLD = quality_run
    start, length = [int(v) for v in np_read["raw_start"]], [int(v) for v in np_read["raw_length"]]
    lines = (d / "quality.tsv").read_text().splitlines()
    assert lines[0].startswith("#call-quality bin_lo=%d bin_width=%d n_bins=%d min_gap=%d;" % GRID)
    R = [l.split("\t") for l in lines if l.startswith("R\t")]
    G = [l.split("\t") for l in lines if l.startswith("G\t")]
    H = [l.split("\t") for l in lines if l.startswith("H\t")]
    assert len(R) == 1 and len(R[0]) == 16 and R[0][:3] == ["R", "read108", "t"] and len(lines) == 1 + len(R) + len(G) + len(H)
    status, n_calls, n_correct, n_unl, n_other, n_outside, sum_abs, max_abs, max_ref, n_path, n_gaps, sum_gap, max_gap = (int(v) for v in R[0][3:])
    # the calls file: one line per site the truth names, in ascending x, with the probability the .calls file prints
    calls = [l.split("\t") for l in (d / "quality_calls.tsv").read_text().splitlines()[1:]]
    named = {(l.split("\t")[1]): l.split("\t")[4] for l in open(truth).read().splitlines()}
    by_pos = {s[2]: s for s in sites}
    assert status == 0 and n_calls == len(calls) == len(named) and n_unl == len(sites) - len(named) > 5 and n_other == 0
    assert sorted(c[2] for c in calls) == sorted(named)
    steps = {int(b[2]) - int(a[2]) > 0 for a, b in zip(calls, calls[1:])}
    assert len(steps) == 1                                              # ascending x: reference_index runs one way
    # --signal-labels-kmer-index 0 labels the k-mer's first base as the reference_index counts them: the k-mer's own index when it
    # ascends with x, K - 1 = 4 further when it descends
    shift = 0 if steps == {True} else 4
    bands = {str(int(l.split("\t")[0]) - shift): l.split("\t")[1:3] for l in (d / "lab" / "read108.bands.tsv").read_text().splitlines()}
    deltas, inside = [], 0
    for c in calls:
        label, strand, pos, b_start, b_length, guide_event, delta, letter, prob, correct, outside = c
        assert (label, strand, letter) == ("read108", "t", named[pos])
        site = by_pos[pos]
        p = float(site[6 + "CE".index(letter)])
        assert abs(float(prob) - p) <= 1e-6 + 1e-12 and int(correct) == (float(prob) > THRESHOLD)
        assert [b_start, b_length] == bands[pos]                         # the band of --signal-labels-bands
        delta2 = int(round(2 * float(delta)))
        assert delta == ("-" if delta2 < 0 else "") + str(abs(delta2) // 2) + (".5" if delta2 % 2 else "")
        if int(outside):
            assert int(guide_event) == -1 and delta2 == 0
            continue
        inside += 1
        e = int(guide_event)
        assert delta2 == 2 * int(b_start) + int(b_length) - 2 * ref.round_mid(start[e], length[e])
        deltas.append((delta2, int(correct)))
    assert n_correct == sum(int(c[9]) for c in calls) < n_calls
    assert n_outside == n_calls - inside and inside > 20
    assert sum_abs == sum(abs(v) for v, _ in deltas) and max_abs == max(abs(v) for v, _ in deltas)
    assert max_ref == int(min((c for c in calls if not int(c[10])), key=lambda c: (-abs(float(c[6])), calls.index(c)))[2])
    # the gaps of the .mea file's events, in samples
    mea_events = sorted(int(l.split("\t")[5]) for l in open(out + ".mea").read().splitlines())
    gaps = ref.gaps_of(mea_events, start, length, GRID[3])
    assert n_path == len(mea_events) and n_gaps == len(gaps) == len(G) > 0
    assert [(int(a[3]), int(a[4]), int(a[5])) for a in G] == gaps and all(a[1:3] == ["read108", "t"] for a in G)
    assert sum_gap == sum(v for _, _, v in gaps) and max_gap == max(v for _, _, v in gaps)
    # the histogram, summed over the run: one read
    want = np.zeros((GRID[2] + 2, 2), dtype=np.int64)
    for delta2, correct in deltas:
        want[ref.hist_slot(delta2, *GRID[:3]), correct] += 1
    assert len(H) == GRID[2] + 2 and H[0][1] == "under" and H[-1][1] == "over"
    assert [h[1] for h in H[1:-1]] == [str(GRID[0] + q * GRID[1]) for q in range(GRID[2])]
    assert [[int(h[2]), int(h[3])] for h in H] == want.tolist() and want[1:-1].sum() > 10


def test_manifest_writes_quality_lines_for_the_raw_read_only(quality_run, tmp_path):
    d, fasta, spec, raw, amb, truth, sites, plain, out, np_read, THRESHOLD = quality_run
    manifest = str(tmp_path / "manifest.tsv")
    with open(manifest, "w") as f:
        f.write("\t".join(("fromnp", str(d / "np" / "read108.npRead"), "@" + spec, "-")) + "\n")
        f.write("\t".join(("read108", raw, "@" + spec, "-")) + "\n")
    pr = _run([BIN, "-T", MODEL, "-f", fasta, "-x", "50", "-D", "0.01", "-m", "14", "-g", "100", "-s", "0", "-a", amb, "--batch", manifest,
               "--site-calls-accuracy", str(tmp_path / "acc.tsv"), "--site-calls-truth", truth, "--site-calls-accuracy-threshold", repr(THRESHOLD),
               "--site-calls-accuracy-quality", str(tmp_path / "quality.tsv"), "--site-calls-accuracy-quality-calls", str(tmp_path / "calls.tsv"),
               "--site-calls-accuracy-quality-bins", "%d,%d,%d" % GRID[:3], "--site-calls-accuracy-quality-min-gap", str(GRID[3])])
    assert pr.returncode == 0, pr.stderr
    assert "batch: 2 of 2 reads aligned" in pr.stderr
    assert "NOTICE: fromnp is not given as raw current: no call quality" in pr.stderr
    assert (tmp_path / "quality.tsv").read_bytes() == (d / "quality.tsv").read_bytes()         # the posteriors file is '-': no text was needed
    assert (tmp_path / "calls.tsv").read_bytes() == (d / "quality_calls.tsv").read_bytes()
