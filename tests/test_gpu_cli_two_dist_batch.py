"""signalMachine --batch --emission twoDist: the reads of a manifest in ONE GPU batch, every read with the noise scaling its own
parameter estimation left (sa_batch_create_noise_scaled on the strand's model, SA_FLAG_TWO_DIST_ALL_KERNELS) -- against the same reads
run one process each, where a read is aligned with a model cloned for it."""
import os
import subprocess

import numpy as np
import pytest

import sa_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
THRESHOLD = 0.01


def _write_fasta(path, records, width=60):
    with open(path, "w") as f:
        for name, seq in records:
            f.write(">%s\n" % name)
            for i in range(0, len(seq), width):
                f.write(seq[i:i + width] + "\n")


def _rows(path):
    """(position, event index, k-mer) and the printed posterior of every row of a full TSV"""
    keys, post = [], []
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        keys.append((int(f[1]), int(f[5]), f[15]))
        post.append(float(f[12]))
    return keys, post


def _same_alignment(batch_path, single_path, label):
    kb, pb = _rows(batch_path)
    ks, ps = _rows(single_path)
    b, s = dict(zip(kb, pb)), dict(zip(ks, ps))
    assert len(b) == len(kb) and len(s) == len(ks) and len(ks) > 300, label
    lonely = [(k, v) for k, v in list(b.items()) + list(s.items()) if not (k in b and k in s)]
    for k, v in lonely:     # a row on one side only: its printed posterior within 1e-5 of the threshold
        assert abs(v - THRESHOLD) <= 1e-5 + 5e-7, (label, k, v)
    assert len(lonely) <= 2, (label, lonely)
    assert [k for k in kb if k in s] == [k for k in ks if k in b], label                    # same row order
    worst = max(abs(b[k] - s[k]) for k in b if k in s)
    print("%s: %d rows, %d on one side only, worst |dp| of the printed posteriors = %.1e" % (label, len(ks), len(lonely), worst))
    assert worst <= 1.1e-5, (label, worst)      # the bar plus half a unit of the six printed decimals on each side


def test_batch_mode_two_distribution_emission_per_read_noise(oracle, tmp_path):
    assert os.path.exists(BIN), "signalMachine is not built"
    model = cases.MODEL_6MER
    np_a = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")
    read_a = oracle.parse_npread(np_a)["template_read"]
    rng = np.random.default_rng(11)
    records, reads = [], []
    # the bundled read with the single-M guide alignment the other command-line tests give it
    pre = "".join("ACGT"[i] for i in rng.integers(0, 4, 200))
    start_a, len_a = 10, len(read_a) - 25
    records.append(("chrA", pre + read_a[start_a:] + "GATTACA" * 20))
    reads.append(("readA", np_a, "cigar: readA %d %d + chrA %d %d + 1 M %d\n" % (start_a, start_a + len_a, 200, 200 + len_a, len_a)))
    # two synthetic reads of about 600 bases, their noise column scaled by 0.7 / 1.5; guide alignments with a stretch of match runs
    # too short to leave an anchor (-m 14 trims both ends of a run): 330 bases without anchors, a band wider than a wave
    for name, seed, factor in (("readB", 21, 0.7), ("readC", 22, 1.5)):
        seq = "".join("ACGT"[i] for i in rng.integers(0, 4, 600))
        ev, emap = cases.events_for_sequence(seq, model, seed)
        ev[:, 1] *= factor
        path = str(tmp_path / (name + ".npRead"))
        cases.write_npread_1d(path, seq, emap, ev)
        ops = "M 150" + " M 20 D 1 M 20 I 1" * 8
        done = 150 + 8 * 41
        L = 590
        ops += " M %d" % (L - done)
        records.append(("chr" + name[-1], "TTGACC" * 10 + seq + "ACGT" * 10))
        reads.append((name, path, "cigar: %s 0 %d + chr%s 60 %d + 1 %s\n" % (name, L, name[-1], 60 + L, ops)))
    fasta = str(tmp_path / "ref.fa")
    _write_fasta(fasta, records)
    common = ["-T", model, "-f", fasta, "-g", "100", "-x", "50", "-D", str(THRESHOLD), "-m", "14", "-s", "0", "--emission", "twoDist"]
    manifest_rows = []
    for name, npread, cigar_line in reads:
        cigar = str(tmp_path / (name + ".cigar"))
        with open(cigar, "w") as f:
            f.write(cigar_line)
        single = str(tmp_path / (name + ".single.tsv"))
        pr = subprocess.run([BIN] + common + ["-n", "chr" + name[-1], "-q", npread, "-p", cigar, "-u", single, "-L", name],
                            capture_output=True, text=True, timeout=300)
        assert pr.returncode == 0, pr.stderr
        manifest_rows.append([name, npread, cigar, str(tmp_path / (name + ".batch.tsv")), "-", "chr" + name[-1]])
    manifest = str(tmp_path / "manifest.tsv")
    with open(manifest, "w") as f:
        f.write("".join("\t".join(r) + "\n" for r in manifest_rows))
    pr = subprocess.run([BIN] + common + ["--batch", manifest], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    assert "3 of 3 reads aligned" in pr.stderr
    for name, _, _ in reads:
        _same_alignment(str(tmp_path / (name + ".batch.tsv")), str(tmp_path / (name + ".single.tsv")), name)
    # a read's rows do not depend on what else is in its batch: a noise scaling that leaks between reads would show here
    alone = str(tmp_path / "alone.tsv")
    with open(manifest, "w") as f:
        f.write("\t".join(manifest_rows[0][:3] + [alone] + manifest_rows[0][4:]) + "\n")
    pr = subprocess.run([BIN] + common + ["--batch", manifest], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    assert open(alone, "rb").read() == open(str(tmp_path / "readA.batch.tsv"), "rb").read()
    # still refused, with the message: an HDP model, the expectation pass
    for extra in (["-v", cases.NHDP], ["-t", str(tmp_path / "expectations.tsv")]):
        pr = subprocess.run([BIN] + common + ["--batch", manifest] + extra, capture_output=True, text=True, timeout=300)
        assert pr.returncode != 0 and "--emission twoDist aligns reads with a Gaussian model" in pr.stderr, pr.stderr
