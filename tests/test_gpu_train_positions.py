"""The k-mer table from the rows that cover labelled positions, on the GPU (sa_kmer_table_set_positions, _add_batch_at,
_position_counts): the rows the table keeps and the coverage counts equal the restatement (tests/train_positions_ref.py, then
kmer_training_ref.top_n) fed from the batch's own pairs -- exactly, integers only -- for 16- and 8-byte records, after the
batch's device storage went back, with x_sign -1, several contigs, strand 1, at the edges of the key table, over two batches,
across checkpoint and rollback, and with the tie levels of the selection running; the SA_ESTATE contract; and the reference's own
property on the bundled E. coli read: with positions at the second C of every CCAGG / CCTGG, every kept row's k-mer is one of the
motifs' k-mers."""
import os
import subprocess

import numpy as np
import pytest

import signalalign_amd as sa

import guide_ref as g
import kmer_training_ref as kref
import sa_cases as cases
import train_positions_ref as ref

pytestmark = pytest.mark.gpu

MIN_PROB = 0.05
SA_ESTATE = -7


def _params():
    p = sa.default_params()
    p.threshold = 0.01          # low, so that every k-mer of a read has rows
    return p


def _mean(job, y):
    ev = np.asarray(job["events"], dtype=np.float64)
    return float(ev[y] if ev.ndim == 1 else ev[y, 0])


def _place(jobs, k, seed, contigs=1, signs=(1,), site_strands=(0,)):
    """a job map: every read somewhere on a contig of about 400 bases, as signalMachine's adjust_ref would place it"""
    rng = np.random.default_rng(seed)
    maps = []
    for j, job in enumerate(jobs):
        n_x = len(job["ref"]) - k + 1
        sign = signs[j % len(signs)]
        start = int(rng.integers(0, 60))
        maps.append(dict(contig=j % contigs, x_sign=sign, x0=start if sign == 1 else start + n_x - 1,
                         site_strand=site_strands[j % len(site_strands)]))
    return maps


def batch_rows(b, jobs, maps, model, k, strand, p8=False):
    """the batch's rows in run order, as the restatement takes them"""
    level = model.table5()
    letter = "tc"[strand]
    out = []
    for j, (job, m) in enumerate(zip(jobs, maps)):
        if p8:
            recs = b.pairs8(j)
            kmers = [model.kmer_id(job["ref"][x:x + k]) for x in recs["x"].tolist()]
        else:
            recs = b.pairs(j)
            kmers = recs["kmer_id"].tolist()
        forward = (m["site_strand"] == 0) == (strand == 0)       # (strand_pairs, read backwards)
        assert ref.site_strand(forward, letter) == "+-"[m["site_strand"]]
        for x, km, y, pe7 in zip(recs["x"].tolist(), kmers, recs["y"].tolist(), recs["prob_e7"].tolist()):
            d = kref.descaled(_mean(job, y), float(level[5 * km]), job.get("scale", 1.0), job.get("shift", 0.0), job.get("var", 1.0))
            out.append((m["contig"], m["x0"] + m["x_sign"] * x, letter, forward, km, "%f" % d, "%f" % (pe7 / 1e7)))
    return out


def expected(rows, sites, k, n, min_prob=MIN_PROB):
    """(the table's rows as KMER_ROW-shaped tuples in its order, the counts in the key table's order)"""
    lines = [(c, p, "+-"[s]) for c, p, s in sites]
    idx, counts = ref.offered([(r[0], r[1], r[2], r[3], r[6]) for r in rows], lines, k, min_prob)
    kept = kref.top_n([(rows[i][2], rows[i][4], rows[i][5], rows[i][6], i) for i in idx], n, min_prob)
    out = []
    for key in sorted(kept):
        for r in kept[key]:
            du, nz = kref.units(r[2])
            out.append((key[1], kref.units(r[3])[0], du, nz, r[4]))
    keys = sorted(counts, key=lambda c: (c[0], c[2] == "-", c[1]))
    return out, [(c, p, int(s == "-"), counts[(c, p, s)]) for c, p, s in keys], idx


def got_rows(tab, strand=0):
    r = tab.rows(strand)
    return list(zip(r["kmer_id"].tolist(), r["prob_units"].tolist(), r["descaled_units"].tolist(), r["neg_zero"].tolist(), r["run"].tolist()))


def got_counts(tab):
    s, c = tab.position_counts()
    return list(zip(s["contig"].tolist(), s["pos"].tolist(), s["mapped_strand"].tolist(), c.tolist()))


def check(tab, rows, sites, k, n, strand=0, min_prob=MIN_PROB):
    exp_rows, exp_counts, idx = expected(rows, sites, k, n, min_prob)
    assert got_rows(tab, strand) == exp_rows
    assert got_counts(tab) == exp_counts
    return exp_rows, exp_counts, idx


def every(step, lo, hi, contigs=(0,), strands=(0, 1)):
    return [(c, p, s) for c in contigs for s in strands for p in range(lo + 2 * s + c, hi, step)]


@pytest.fixture(scope="module", params=["5mer", "6mer"])
def aligned(request):
    """4 reads of 200-400 events with the 5-mer and the 6-mer model: the batch with 16-byte records, the one with 8-byte records"""
    path = cases.MODEL_5MER if request.param == "5mer" else cases.MODEL_6MER
    model = sa.Model.load(path)
    k = model.alphabet()[1]
    jobs = [cases.synthetic_jobs(path, 1, n, 900 + i)[0] for i, n in enumerate((200, 310, 400, 260))]
    b16, b8 = sa.Batch(model, _params(), jobs), sa.Batch(model, _params(), jobs, flags=sa.FLAG_PAIRS8)
    b16.run()
    b8.run()
    return model, k, jobs, b16, b8


def test_both_record_widths_and_after_release(aligned):
    model, k, jobs, b16, b8 = aligned
    maps = _place(jobs, k, 1)
    sites = every(9, 3, 400) + [(0, 50, 0), (0, 50, 0), (0, 52, 0)]            # a duplicate, two positions closer than k
    rows = batch_rows(b16, jobs, maps, model, k, 0)
    assert rows == batch_rows(b8, jobs, maps, model, k, 0, p8=True)
    tabs = []
    for b in (b16, b8):
        tab = sa.KmerTable(model, 3, MIN_PROB)
        tab.set_positions(sites)
        info = {}
        tab.add_batch_at(b, maps, 0, stats=info)
        assert info["kernel_ms"] >= info["mask_ms"] + info["counts_ms"] > 0 and info["mask_ms"] > 0 and info["counts_ms"] > 0
        exp_rows, exp_counts, idx = check(tab, rows, sites, k, 3)
        assert 50 < len(idx) < len(rows) and len(exp_rows) > 30
        assert sum(c[3] for c in exp_counts) > len(idx)                         # some rows count twice
        assert tab.stats(0)["n"].sum() == len(exp_rows)
        tabs.append(tab)
    for b in (b16, b8):                                                         # the records go up again from the host copy
        b.release_device()
        tab = sa.KmerTable(model, 3, MIN_PROB)
        tab.set_positions(sites)
        tab.add_batch_at(b, maps, 0)
        assert got_rows(tab) == got_rows(tabs[0]) and got_counts(tab) == got_counts(tabs[0])


@pytest.fixture(scope="module")
def small():
    """5 reads of 200-400 events with the 5-mer model, placed on three contigs, some of them against the coordinate"""
    model = sa.Model.load(cases.MODEL_5MER)
    k = model.alphabet()[1]
    jobs = [cases.synthetic_jobs(cases.MODEL_5MER, 1, n, 950 + i)[0] for i, n in enumerate((220, 400, 300, 200, 350))]
    b = sa.Batch(model, _params(), jobs)
    b.run()
    return model, k, jobs, b


def _table(model, sites, n=3):
    tab = sa.KmerTable(model, n, MIN_PROB)
    tab.set_positions(sites)
    return tab


def test_minus_sign_mixed_contigs_and_strand_one(small):
    model, k, jobs, b = small
    maps = _place(jobs, k, 2, contigs=3, signs=(1, -1), site_strands=(0, 1, 1))
    assert {m["x_sign"] for m in maps} == {1, -1} and {m["contig"] for m in maps} == {0, 1, 2}
    sites = every(7, 0, 300, contigs=(0, 2, 5))                                 # contig 1 has no line, contig 5 no read
    for strand in (0, 1):
        rows = batch_rows(b, jobs, maps, model, k, strand)
        tab = _table(model, sites)
        tab.add_batch_at(b, maps, strand)
        exp_rows, exp_counts, idx = check(tab, rows, sites, k, 3, strand)
        assert len(exp_rows) > 30 and not got_rows(tab, 1 - strand)
        assert {rows[i][0] for i in idx} == {0, 2}
        assert any(c[3] for c in exp_counts if c[2] == 0) and any(c[3] for c in exp_counts if c[2] == 1)
        assert not any(c[3] for c in exp_counts if c[0] == 5)


def test_key_table_edges(small):
    model, k, jobs, b = small
    maps = [dict(contig=1, x_sign=1, x0=100, site_strand=0) for _ in jobs]
    rows = batch_rows(b, jobs, maps, model, k, 0)
    hi = max(r[1] for r in rows)
    for sites, some in (([(1, 150, 0)], True),                                  # one key
                        ([(0, 150, 0), (1, 100 - k, 0), (1, 40, 0)], False),    # keys only before every job's window
                        ([(1, hi + k, 0), (2, 120, 0), (1, 150, 1)], False),    # only after it (and on the other strand)
                        ([], False)):                                           # n == 0: nothing kept, nothing counted
        tab = _table(model, sites)
        tab.add_batch_at(b, maps, 0)
        exp_rows, exp_counts, idx = check(tab, rows, sites, k, 3)
        assert bool(exp_rows) == some and len(exp_counts) == len(set(sites))
    # a key at reference_index 0, under reads that start there and reads that end there
    maps = _place(jobs, k, 3, signs=(1, -1))
    for j, m in enumerate(maps):                                                # (the job's first record along the coordinate at 0)
        x = b.pairs(j)["x"]
        m["x0"] = -int(x.min()) if m["x_sign"] == 1 else int(x.max())
    rows = batch_rows(b, jobs, maps, model, k, 0)
    assert min(r[1] for r in rows) == 0
    sites = [(0, 0, 0), (0, 2, 0)]
    tab = _table(model, sites)
    tab.add_batch_at(b, maps, 0)
    exp_rows, exp_counts, idx = check(tab, rows, sites, k, 3)
    assert exp_counts[0][3] > 0 and 0 in {rows[i][1] for i in idx} <= {0, 1, 2}


def test_two_batches_equal_one_and_rollback_restores(small):
    model, k, jobs, b = small
    maps = _place(jobs, k, 4, contigs=2, signs=(1, 1, -1))
    sites = every(5, 1, 320, contigs=(0, 1))
    rows = batch_rows(b, jobs, maps, model, k, 0)
    one = _table(model, sites, 2)
    one.add_batch_at(b, maps, 0)
    exp_rows, exp_counts, _ = check(one, rows, sites, k, 2)
    b1, b2 = sa.Batch(model, _params(), jobs[:2]), sa.Batch(model, _params(), jobs[2:])
    b1.run()
    b2.run()
    two = _table(model, sites, 2)
    two.add_batch_at(b1, maps[:2], 0)
    first_rows, first_counts = got_rows(two), got_counts(two)
    assert first_rows and first_rows != exp_rows
    two.checkpoint()
    two.add_batch_at(b2, maps[2:], 0)
    assert got_rows(two) == exp_rows and got_counts(two) == exp_counts        # run-order ties across batches
    two.rollback()
    assert got_rows(two) == first_rows and got_counts(two) == first_counts
    two.add_batch_at(b2, maps[2:], 0)                                           # the slice again, as signalMachine --batch adds it
    assert got_rows(two) == exp_rows and got_counts(two) == exp_counts


def test_more_records_than_a_block_and_the_tie_levels():
    """one read with more records than one block of the record kernels takes (4096) and more reference positions than a wave; with
    max_per_kmer 1 many k-mers have ties at the cutoff, which the run-order levels settle"""
    model = sa.Model.load(cases.MODEL_5MER)
    k = model.alphabet()[1]
    jobs = cases.synthetic_jobs(cases.MODEL_5MER, 1, 6000, 990) + cases.synthetic_jobs(cases.MODEL_5MER, 1, 300, 991)
    b = sa.Batch(model, _params(), jobs)
    b.run()
    maps = [dict(contig=0, x_sign=-1, x0=len(jobs[0]["ref"]) + 10, site_strand=1), dict(contig=0, x_sign=1, x0=30, site_strand=1)]
    rows = batch_rows(b, jobs, maps, model, k, 0)
    assert len(b.pairs(0)) > 4096 and len(jobs[0]["ref"]) - k + 1 > 64
    sites = every(3, 0, 3700, strands=(1,))
    tab = _table(model, sites, 1)
    tab.add_batch_at(b, maps, 0)
    exp_rows, exp_counts, idx = check(tab, rows, sites, k, 1)
    by = {}
    for i in idx:
        by.setdefault(rows[i][4], []).append(kref.units(rows[i][6])[0])
    assert sum(1 for v in by.values() if v.count(max(v)) > 1) > 3               # the best posterior of a k-mer is held by several rows


def test_state_contract(small):
    model, k, jobs, b = small
    maps = _place(jobs, k, 5)
    plain = sa.KmerTable(model, 3, MIN_PROB)
    for call in (lambda: plain.add_batch_at(b, maps, 0), plain.position_counts):   # no positions set
        with pytest.raises(sa.SaError) as ei:
            call()
        assert ei.value.code == SA_ESTATE
    plain.add_batch(b, 0)
    with pytest.raises(sa.SaError) as ei:                                       # only on an empty table
        plain.set_positions([(0, 10, 0)])
    assert ei.value.code == SA_ESTATE
    tab = _table(model, [(0, 10, 0)])
    for call in (lambda: tab.add_batch(b, 0), lambda: tab.add_rows([1], [80.0], [0.9])):   # they carry no coordinates
        with pytest.raises(sa.SaError) as ei:
            call()
        assert ei.value.code == SA_ESTATE
    for bad in ([(0, 10, 2)], [(-1, 10, 0)], [(1 << 21, 10, 0)], [(0, -1, 0)], [(0, 1 << 41, 0)]):
        with pytest.raises(sa.SaError) as ei:
            sa.KmerTable(model, 3, MIN_PROB).set_positions(bad)
        assert ei.value.code == -1
    for field, value in (("x_sign", 0), ("x_sign", 2), ("site_strand", 2), ("contig", -1), ("x0", 1 << 42)):
        wrong = [dict(m) for m in maps]
        wrong[-1][field] = value
        with pytest.raises(sa.SaError) as ei:
            tab.add_batch_at(b, wrong, 0)
        assert ei.value.code == -1
    with pytest.raises(sa.SaError) as ei:                                       # n_jobs must be the batch's
        tab.add_batch_at(b, maps[:-1], 0)
    assert ei.value.code == -1
    assert not got_rows(tab) and got_counts(tab) == [(0, 10, 0, 0)]             # the refused adds added nothing
    tab.add_batch_at(b, maps, 0)
    assert got_rows(tab)


# ---- the reference's own property (tests/test_trainModels.py:432-459), through signalMachine on the bundled E. coli 1-D read ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "signalalign_amd", "bin", "signalMachine")
MODEL_ACEGT = os.path.join(cases.GOLDEN, "models", "testModelR9p4_5mer_acegt_template.model")
NPREAD = os.path.join(cases.GOLDEN, "npReads", "r9p4_oneD.npRead")
PRE, POST = 300, 200


def _write_fasta(path, name, seq, width=60):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for i in range(0, len(seq), width):
            f.write(seq[i:i + width] + "\n")
    with open(path + ".fai", "w") as f:
        f.write("%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), len(name) + 2, width, width + 1))


def motif_positions(contig, name):
    """the second C of every CCAGG / CCTGG on '+', the matching base (the second C of the motif read on the other strand) on '-'"""
    lines = []
    for motif in ("CCAGG", "CCTGG"):
        at = contig.find(motif)
        while at >= 0:
            lines += ["%s\t%d\t+\tC\tE\n" % (name, at + 1), "%s\t%d\t-\tC\tE\n" % (name, at + 3)]
            at = contig.find(motif, at + 1)
    return lines


@pytest.mark.parametrize("minus", [False, True])
def test_kept_kmers_are_the_motifs_kmers_on_the_ecoli_read(tmp_path, minus):
    read, window = g.ecoli_pair()
    rng = np.random.default_rng(3)
    contig = "".join("ACGT"[i] for i in rng.integers(0, 4, PRE)) + window + "".join("ACGT"[i] for i in rng.integers(0, 4, POST))
    lo, hi = PRE - 50, PRE + len(window) + 100
    if minus:
        contig, lo, hi = g.reverse_complement(contig), len(contig) - hi, len(contig) - lo
    fasta, positions, table, cover = (str(tmp_path / n) for n in ("ref.fa", "positions.tsv", "table.tsv", "coverage.tsv"))
    _write_fasta(fasta, "chrE", contig)
    lines = motif_positions(contig, "chrE")
    assert len(lines) > 20
    open(positions, "w").writelines(lines)
    pr = subprocess.run([BIN, "-T", MODEL_ACEGT, "-q", NPREAD, "-f", fasta, "-L", "read1", "-x", "50", "-D", "0.01", "-m", "14", "-g", "100",
                         "-s", "0", "-u", str(tmp_path / "out.tsv"), "--guide-window", "chrE:%d-%d" % (lo, hi), "--train-assignments", table,
                         "--train-positions", positions, "--train-positions-coverage", cover, "--train-min-prob", "0.3"],
                        capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr[-2000:]
    motif_kmers = {c for a, b in (("CCAGG", "CEAGG"), ("CCTGG", "CETGG")) for c, _ in sa.motif_kmer_pairs(5, a, b)}
    kept = [l.split("\t") for l in open(table)]
    assert len(kept) >= 20                                                      # (enough rows for the subset below to say something)
    assert {f[0] for f in kept} <= motif_kmers and {f[1] for f in kept} == {"t"}
    cov = [l.split("\t") for l in open(cover)]
    assert len(cov) == len(set(lines))
    used, idle = ("-", "+") if minus else ("+", "-")                           # a 1-D read's t rows pair with its mapping strand
    assert sum(int(f[3]) for f in cov if f[2] == used) >= len(kept) and sum(int(f[3]) for f in cov if f[2] == idle) == 0
