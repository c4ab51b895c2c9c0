"""compareDistributions --model --compare [--assignments]: the lines of the comparison file and the <kmer>_kde.txt files of a
run against the same steps through the library (HdpState.vs_gaussian, KmerTable.kde, hdp_distances_paired), the files of the
two-argument form byte for byte with and without the new options, and the refusals."""
import math
import os
import subprocess

import numpy as np
import pytest

import signalalign_amd as sa

import sa_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "signalalign_amd", "bin", "compareDistributions")
BIG = 1 << 20


def run(args):
    return subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """five k-mers of the bundled HDP (four observed, one not), a listing of them and an assignments table with rows of both
    strands for four of them"""
    tmp = tmp_path_factory.mktemp("compare")
    s = sa.HdpState(cases.NHDP)
    model = sa.Model.load(cases.MODEL_R73)
    alphabet, k = s.alphabet(), int(s.info.kmer_length)
    assert (alphabet, k) == model.alphabet()
    observed = s.array("observed")[:len(alphabet) ** k]

    def name(dp):
        return "".join(alphabet[(int(dp) // len(alphabet) ** (k - 1 - q)) % len(alphabet)] for q in range(k))
    dps = [int(d) for d in np.flatnonzero(observed == 1)[[0, 5, 20, 77]]] + [int(np.flatnonzero(observed == 0)[3])]
    kmers = [name(d) for d in dps]
    assert [s.kmer_dp(km) for km in kmers] == dps and [model.kmer_id(km) for km in kmers] == dps
    listing = tmp / "kmers.txt"
    listing.write_text("\n".join(kmers) + "\n")
    t5 = model.table5().reshape(-1, 5)
    rng = np.random.RandomState(17)
    rows = []
    for i, (km, dp) in enumerate(zip(kmers, dps)):
        if i == 2:
            continue   # a k-mer without rows
        for strand, n, shift in (("t", 40 + 150 * i, 0.0), ("c", 25, 3.0)):
            for v in rng.normal(t5[dp, 0] + shift, 1.5 * t5[dp, 1], n):
                rows.append("%s\t%s\t%f\t%f\n" % (km, strand, v, rng.uniform(0.2, 1.0)))
    order = rng.permutation(len(rows))
    table = tmp / "table.tsv"
    table.write_text("".join(rows[i] for i in order))
    yield s, model, kmers, dps, listing, table, t5, tmp
    s.close()


def kde_by_api(model, table, kmers, dps, strand, bandwidth, x):
    raw = [ln.split() for ln in open(str(table)) if ln.strip()]
    raw = [r for r in raw if r[1] == strand]
    tab = sa.KmerTable(model, BIG, 0.0)
    tab.add_rows([model.kmer_id(r[0]) for r in raw], [float(r[2]) for r in raw], [float(r[3]) for r in raw])
    info = {}
    log_density = tab.kde(x, dps, bandwidth=bandwidth, info=info)
    tab.close()
    return log_density, info["n_rows"]


def test_compare_without_assignments(setup):
    s, model, kmers, dps, listing, table, t5, tmp = setup
    out_dir, out = tmp / "plain", tmp / "plain.tsv"
    out_dir.mkdir()
    pr = run([cases.NHDP, out_dir, "--kmers", listing, "--model", cases.MODEL_R73, "--compare", out])
    assert pr.returncode == 0, pr.stderr[-2000:]
    want = s.vs_gaussian(dps, t5[dps, 0], t5[dps, 1])
    assert all(int(v) in (0, 2) for v in want["status"][:4]) and want["status"][4] == 1
    assert out.read_text() == "".join("%s\t%d\t%.17g\t%.17g\t%.17g\n" % (km, w["status"], w["kl_bits"], w["hellinger"], w["mode_delta"])
                                      for km, w in zip(kmers, want))
    assert sorted(os.listdir(str(out_dir))) == sorted(["x_vals.txt"] + [km + "_distr.txt" for km in kmers])


@pytest.mark.parametrize("strand,bandwidth,metric", [("t", None, None), ("c", "0.25", "l2")])
def test_compare_with_assignments(setup, strand, bandwidth, metric):
    s, model, kmers, dps, listing, table, t5, tmp = setup
    out_dir, out = tmp / ("kde_" + strand), tmp / ("kde_%s.tsv" % strand)
    out_dir.mkdir()
    args = [cases.NHDP, out_dir, "--kmers", listing, "--model", cases.MODEL_R73, "--compare", out, "--assignments", table]
    if strand != "t":
        args += ["--strand", strand]
    if bandwidth:
        args += ["--bandwidth", bandwidth]
    if metric:
        args += ["--distances", metric]
    pr = run(args)
    assert pr.returncode == 0, pr.stderr[-2000:]
    assert sorted(os.listdir(str(out_dir))) == sorted(["x_vals.txt"] + [km + sfx for km in kmers for sfx in ("_distr.txt", "_kde.txt")])
    x = np.array([float(v) for v in (out_dir / "x_vals.txt").read_text().split()])
    assert len(x) == 600
    log_density, n_rows = kde_by_api(model, table, kmers, dps, strand, float(bandwidth or 0.5), x)
    want_rows = [25 if strand == "c" else 40 + 150 * i for i in range(5)]
    want_rows[2] = 0
    assert list(n_rows) == want_rows
    # the density files: exp of the library's log density (two exponentials, each within an ulp: 4 ulp between them)
    kde = np.array([[float(v) for v in (out_dir / (km + "_kde.txt")).read_text().split()] for km in kmers])
    assert kde.shape == (5, 600) and np.all(np.abs(kde - np.exp(log_density)) <= 4 * 2.3e-16 * np.exp(log_density))
    assert not kde[2].any() and (kde[[0, 1, 3, 4]].max(axis=1) > 0.01).all()
    # the distances: the library's, on the curves the tool wrote
    hdp = s.densities(dps, x)
    for km, row in zip(kmers, hdp):
        assert (out_dir / (km + "_distr.txt")).read_text() == "".join("%.17g\n" % v for v in row)

    def pdf(g, mu, sd):
        z = (g - mu) / sd
        return math.exp(-(z * z) / 2.0) / 2.5066282746310002 / sd
    normal = np.array([[pdf(float(g), float(t5[d, 0]), float(t5[d, 1])) for g in x] for d in dps])
    m = {None: sa.HDP_METRIC_HELLINGER, "l2": sa.HDP_METRIC_L2}[metric]
    d_hdp, d_gauss = sa.hdp_distances_paired(x, kde, hdp, m), sa.hdp_distances_paired(x, kde, normal, m)
    vs = s.vs_gaussian(dps, t5[dps, 0], t5[dps, 1])
    lines = out.read_text().splitlines()
    assert len(lines) == 5
    for i, (km, ln) in enumerate(zip(kmers, lines)):
        f = ln.split("\t")
        assert f[:6] == [km, "%d" % vs[i]["status"], "%.17g" % vs[i]["kl_bits"], "%.17g" % vs[i]["hellinger"],
                         "%.17g" % vs[i]["mode_delta"], "%d" % want_rows[i]], km
        assert f[6] == "%.17g" % d_hdp[i], km
        # (the tool's normal density is C's exp, this one Python's: equal up to an ulp of each point)
        assert abs(float(f[7]) - d_gauss[i]) <= 1e-12 * max(1.0, abs(d_gauss[i])), km
        assert len(f) == 8
    assert 0 < float(lines[0].split("\t")[6]) < float("inf")


def test_two_argument_form_is_untouched(setup):
    s, model, kmers, dps, listing, table, t5, tmp = setup
    before, after = tmp / "before", tmp / "after"
    before.mkdir()
    after.mkdir()
    a = run([cases.NHDP, before, "--kmers", listing])
    b = run([cases.NHDP, after, "--kmers", listing, "--model", cases.MODEL_R73, "--compare", tmp / "after.tsv", "--assignments", table])
    assert a.returncode == 0 and b.returncode == 0, (a.stderr[-1000:], b.stderr[-1000:])
    names = sorted(os.listdir(str(before)))
    assert names == sorted(["x_vals.txt"] + [km + "_distr.txt" for km in kmers])
    for n in names:
        assert (before / n).read_bytes() == (after / n).read_bytes(), n
    assert a.stderr.replace(str(before), "DIR") == b.stderr.replace(str(after), "DIR") and a.stdout == b.stdout == ""


def test_refusals(setup):
    s, model, kmers, dps, listing, table, t5, tmp = setup
    out_dir = tmp / "refused"
    out_dir.mkdir()
    base = [cases.NHDP, out_dir, "--kmers", listing]
    for extra in (["--model", cases.MODEL_6MER, "--compare", tmp / "r.tsv"],      # another alphabet and k-mer set
                  ["--model", cases.MODEL_R73],                                    # the two go together
                  ["--compare", tmp / "r.tsv"],
                  ["--assignments", table],                                        # needs --compare
                  ["--model", cases.MODEL_R73, "--compare", tmp / "r.tsv", "--strand", "t"],
                  ["--model", cases.MODEL_R73, "--compare", tmp / "r.tsv", "--assignments", table, "--strand", "x"],
                  ["--model", cases.MODEL_R73, "--compare", tmp / "r.tsv", "--assignments", table, "--bandwidth", "0"],
                  ["--model", cases.MODEL_R73, "--compare", tmp / "r.tsv", "--assignments", tmp / "missing.tsv"]):
        pr = run(base + extra)
        assert pr.returncode != 0 and "[compareDistributions] ERROR: " in pr.stderr, extra
    assert not (tmp / "r.tsv").exists() or (tmp / "r.tsv").read_text() == ""
