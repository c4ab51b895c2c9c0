"""signalMachine --guide-deviation: single reads and --batch write the same lines per read; the events file joins with the full TSV
of the same run; the restatement (deviation_ref.py) over the events file's columns reproduces the R, H, S and T lines; a run whose
manifest writes no TSV gives the same file; and every existing output is byte-identical with and without the new options.  The
case builders are test_gpu_cli_snp_marginals.py's."""
import os
import subprocess

import pytest

import sa_cases as cases
import deviation_ref as ref
import test_gpu_cli_snp_marginals as base

pytestmark = pytest.mark.gpu


def _batch_run(tmp, reads, fa, tag, tsv=True, mea=False, dev=True):
    d = tmp / tag
    d.mkdir()
    post = {r.label: str(d / ("%s.tsv" % r.label)) for r in reads} if tsv else None
    args = fa + ["--batch", base.manifest(d, reads, tag, post), "--batch-reads", "2"] + (["--mea"] if mea else [])
    if dev:
        args += ["--guide-deviation", str(d / "dev.tsv"), "--guide-deviation-events", str(d / "events.tsv")]
    return dict(dir=d, post=post, pr=base.run(args, 1))


@pytest.fixture(scope="module")
def runs(oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("guide_deviation")
    reads, records = base.the_reads(oracle)
    fa = base.fastas(tmp, "all", records)
    good = [r for r in reads if not r.label.startswith("bad")]
    c = dict(tmp=tmp, reads=reads, good=good, fa=fa)
    # three runs: --mea alone, --mea with the new options, and the new options alone with no posteriors file at all
    c["plain"] = _batch_run(tmp, reads, fa, "plain", mea=True, dev=False)
    c["dev"] = _batch_run(tmp, reads, fa, "dev", mea=True)
    c["no_tsv"] = _batch_run(tmp, reads, fa, "no_tsv", tsv=False)
    return c


def _lines(path, kinds="RHS"):
    """label -> the read's lines of the deviation file, in file order"""
    out = {}
    for line in open(path).read().splitlines():
        if line[0] in kinds:
            out.setdefault(line.split("\t")[1], []).append(line)
    return out


def _event_lines(path):
    """label -> the read's rows of the events file"""
    out = {}
    for line in open(path).read().splitlines()[1:]:
        out.setdefault(line.split("\t")[0], []).append(line)
    return out


def test_the_file_of_a_batch(runs):
    c = runs
    text = open(c["dev"]["dir"] / "dev.tsv").read()
    assert text.startswith("#guide-deviation threshold=10 bucket_size=5 n_buckets=64;") and text.splitlines()[-1].startswith("T\t")
    batch = _lines(c["dev"]["dir"] / "dev.tsv")
    assert sorted(batch) == ["a", "b", "rm"]                                   # a skipped read writes nothing
    events = _event_lines(c["dev"]["dir"] / "events.tsv")
    assert open(c["dev"]["dir"] / "events.tsv").readline().startswith("#label\tstrand\tevent_index\t")
    assert sorted(events) == ["a", "b", "rm"] and all(len(v) > 300 for v in events.values())


@pytest.mark.parametrize("label", ["rm", "b"])                                 # a minus-strand read and a forward one
def test_a_single_read_writes_the_lines_of_the_batch(runs, label):
    c = runs
    batch = _lines(c["dev"]["dir"] / "dev.tsv")
    events = _event_lines(c["dev"]["dir"] / "events.tsv")
    for r in [q for q in c["good"] if q.label == label]:
        d = c["tmp"] / ("single_" + r.label)
        d.mkdir()
        cigar = str(d / "one.cigar")
        with open(cigar, "w") as f:
            f.write(r.cigar_line)
        base.run(c["fa"] + ["-q", r.npread, "-p", cigar, "-u", str(d / "one.tsv"), "-n", r.seq_name, "-L", r.label,
                            "--guide-deviation", str(d / "dev.tsv"), "--guide-deviation-events", str(d / "events.tsv")], 0)
        assert _lines(d / "dev.tsv")[r.label] == batch[r.label]
        assert _event_lines(d / "events.tsv") == {r.label: events[r.label]}
        assert open(d / "one.tsv").read() == open(c["dev"]["post"][r.label]).read()
        # one read: its histogram is the sum
        h, t = [l for l in open(d / "dev.tsv").read().splitlines() if l[0] in "HT"]
        assert h.split("\t")[3:] == t.split("\t")[1:]


def _events_by_read(path):
    rows = {}
    for line in open(path).read().splitlines():
        if line.startswith("#"):
            continue
        label, strand, ev, x, g, diff, on_mea, flagged = line.split("\t")
        assert strand == "t"
        rows.setdefault(label, []).append(dict(y=int(ev), x=int(x), guide=int(g), diff=int(diff), abs=abs(int(diff)), on_mea=on_mea == "1",
                                               flagged=flagged == "1"))
    return rows


def test_events_file_joins_with_the_full_tsv(runs):
    c = runs
    events = _events_by_read(c["dev"]["dir"] / "events.tsv")
    summary = {l[0].split("\t")[1]: l[0].split("\t") for l in _lines(c["dev"]["dir"] / "dev.tsv", "R").values()}
    for r in c["good"]:
        best, cells = {}, set()
        for line in open(c["dev"]["post"][r.label]).read().splitlines():
            f = line.split("\t")
            ev, x, p = int(f[5]), int(f[1]), f[12]
            cells.add((ev, x, p))
            best[ev] = max(best.get(ev, "0"), p)                               # ("%f" of values in [0, 1]: string order is numeric order)
        rows = events[r.label]
        assert [q["y"] for q in rows] == sorted(best) and int(summary[r.label][4]) == len(best) > 300
        for q in rows:
            assert (q["y"], q["x"], best[q["y"]]) in cells, (r.label, q)
            assert q["flagged"] == (q["abs"] > 10)
        # the events on the path are the events of the .mea file
        on_path = {int(l.split("\t")[5]) for l in open(c["dev"]["post"][r.label] + ".mea").read().splitlines()}
        assert {q["y"] for q in rows if q["on_mea"]} == on_path and len(on_path) > 300
        # the guide: interpolated positions move with the events (forward read: up; minus-strand read: down), by at most a few a step
        step = [b["guide"] - a["guide"] for a, b in zip(rows, rows[1:])]
        assert all(s >= 0 for s in step) if r.forward else all(s <= 0 for s in step)


def test_restatement_over_the_events_file_reproduces_the_lines(runs):
    c = runs
    events = _events_by_read(c["dev"]["dir"] / "events.tsv")
    want, total = [], [0] * 64
    for r in c["good"]:                                                        # (manifest order without the refused reads)
        rows = events[r.label]
        sets = ref.flagged_sets(rows)
        s = ref.read_summary([0], rows, 1, sets)
        h = ref.histogram(rows, 5, 64)
        total = [p + q for p, q in zip(total, h)]
        head = "\t%s\tt" % r.label
        want.append("R" + head + "\t%d\t%d\t%d\t%d\t%f\t%d\t%d\t%d\t%d" % (s["status"], s["n_aligned"], s["n_flagged"], s["n_on_mea"],
                                                                              s["sum_abs"] / s["n_aligned"], s["max_abs"], s["max_abs_mea"],
                                                                              s["max_event"], s["n_sets"]))
        want.append("H" + head + "".join("\t%d" % v for v in h))
        want += ["S" + head + "\t%d\t%d\t%d\t%d\t%d\t%d\t%d" % tuple(q[f] for f in ("first_event", "last_event", "count", "peak", "mea_peak",
                                                                                       "center_event", "open_end")) for q in sets]
    want.append("T" + "".join("\t%d" % v for v in total))
    assert open(c["dev"]["dir"] / "dev.tsv").read().splitlines()[1:] == want
    assert sum(total) > 1000


def test_same_file_without_any_tsv(runs):
    c = runs
    for name in ("dev.tsv", "events.tsv"):
        assert open(c["no_tsv"]["dir"] / name).read() == open(c["dev"]["dir"] / name).read()
    assert sorted(os.listdir(c["no_tsv"]["dir"])) == sorted(["dev.tsv", "events.tsv", "no_tsv.manifest"] + ["%s.cigar" % r.label for r in c["reads"]])
    assert c["no_tsv"]["pr"].stdout == c["dev"]["pr"].stdout


def test_existing_outputs_are_unchanged_by_the_new_options(runs):
    c = runs
    for plain, new, suffixes in (("plain", "dev", ["", ".mea"]),):
        assert c[plain]["pr"].stdout == c[new]["pr"].stdout
        # (the host stage's threads write their lines in any order, and the lines name the run's own directory)
        err = {k: sorted(c[k]["pr"].stderr.replace(str(c[k]["dir"]), "").splitlines()) for k in (plain, new)}
        assert err[plain] == err[new]
        assert "batch: 3 of 5 reads aligned" in c[new]["pr"].stderr
        for r in c["good"]:
            for sfx in suffixes:
                assert open(c[plain]["post"][r.label] + sfx).read() == open(c[new]["post"][r.label] + sfx).read(), (new, r.label, sfx)
        assert not [f for f in os.listdir(c["no_tsv"]["dir"]) if f.endswith(".mea")]   # the paths are computed, the .mea files are --mea's
        extra = set(os.listdir(c[new]["dir"])) - set(os.listdir(c[plain]["dir"]))
        assert extra == {"dev.tsv", "events.tsv", "%s.manifest" % new}


def test_usage_errors_and_help(runs, tmp_path):
    c = runs
    out = str(tmp_path / "d.tsv")
    batch = c["fa"] + ["--batch", base.manifest(tmp_path, c["good"][2:], "u")]
    for extra in (batch + ["--guide-deviation", out, "--snp-step", "5", "--snp-dir", str(tmp_path / "d")],
                  batch + ["--guide-deviation", out, "--guide-deviation-threshold", "-1"],
                  batch + ["--guide-deviation-events", out]):
        pr = subprocess.run([base.BIN, "-T", cases.MODEL_5MER] + extra, capture_output=True, text=True, timeout=120)
        assert pr.returncode != 0 and "--guide-deviation" in pr.stderr.splitlines()[-1], (extra, pr.stderr[-300:])
        assert not os.path.exists(out)
    pr = subprocess.run([base.BIN, "--help"], capture_output=True, text=True, timeout=60)
    for opt in ("--guide-deviation <file>", "--guide-deviation-threshold <n>", "--guide-deviation-events <file>"):
        assert opt in pr.stderr
    # another threshold: the flags follow it, the histogram does not
    d10 = _lines(c["dev"]["dir"] / "dev.tsv", "RH")["b"]
    p3, e3 = str(tmp_path / "t3.tsv"), str(tmp_path / "e3.tsv")
    base.run(batch + ["--guide-deviation", p3, "--guide-deviation-threshold", "3", "--guide-deviation-events", e3], 0)
    d3 = _lines(p3, "RH")["b"]
    rows = _events_by_read(e3)["b"]
    assert d3[1] == d10[1] and int(d3[0].split("\t")[5]) == sum(q["abs"] > 3 for q in rows) >= int(d10[0].split("\t")[5])
    assert all(q["flagged"] == (q["abs"] > 3) for q in rows)
    assert open(p3).read().startswith("#guide-deviation threshold=3 ")
