"""Gaussian emission training on the GPU (sa_kmer_table_*): the rows a table keeps and its per-k-mer statistics must equal a
restatement (tests/kmer_training_ref.py) over the batch's own pairs exactly -- integer units and bits -- on every kernel
family, with host-finalised pairs, with an HDP model, with 8- and 16-byte records, after the device storage went back, and
whether the reads come in one batch or three; the device "%f" rounding equals the host's; the error contract."""
import gzip
import os

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import synth

import kmer_training_ref as ref
import sa_cases as cases

pytestmark = pytest.mark.gpu

CE = {"X": "CE"}
FIXTURE = os.path.join(cases.GOLDEN, "hdp", "d6160b0b-a35e-43b5-947f-adaa1abade28.sm.assignments.tsv.gz")


def test_device_f6_rounding_equals_the_host():
    rng = np.random.default_rng(17)
    v = np.concatenate([rng.uniform(-300, 300, 200000), [(2 * i + 1) / 128 for i in range(-20000, 20000)],
                        rng.standard_normal(20000) * 1e-6, [0.0, -0.0, -1e-9, 5e-7, -5e-7, 2147483647.5, 2.0**31, -2.0**31]])
    u, z, r = sa.f6_units_device(v)
    for i, x in enumerate(v.tolist()):
        hu, hz, hr = sa.f6_units(x)
        assert (int(u[i]), int(z[i]), int(r[i])) == (hu, hz, hr), x
        if hr == 0:
            assert (hu, hz) == ref.units("%f" % x)
    assert int(r[-2]) == -8 and int(r[-1]) == -8   # (|v| < 2^31 only)


def _mean(job, y):
    ev = np.asarray(job["events"], dtype=np.float64)
    return float(ev[y] if ev.ndim == 1 else ev[y, 0])


def batch_rows(b, jobs, level, model, k, p8=False):
    """the batch's rows in run order: (strand placeholder, kmer_id, descaled text, prob text)"""
    out = []
    for j, job in enumerate(jobs):
        if p8:
            recs = b.pairs8(j)
            kmers = [model.kmer_id(job["ref"][x:x + k]) for x in recs["x"].tolist()]
        else:
            recs = b.pairs(j)
            kmers = recs["kmer_id"].tolist()
        for km, y, pe7 in zip(kmers, recs["y"].tolist(), recs["prob_e7"].tolist()):
            d = ref.descaled(_mean(job, y), float(level[5 * km]), job.get("scale", 1.0), job.get("shift", 0.0), job.get("var", 1.0))
            out.append(("t", km, "%f" % d, "%f" % (pe7 / 1e7)))
    return out


def expected_rows(rows, n, min_prob):
    """KMER_ROW-shaped tuples (kmer_id, prob_units, descaled_units, neg_zero, run) in the table's order"""
    keyed = [(r[0], r[1], r[2], r[3], i) for i, r in enumerate(rows)]
    kept = ref.top_n(keyed, n, min_prob)
    out = []
    for (s, km) in sorted(kept):
        for r in kept[(s, km)]:
            du, nz = ref.units(r[2])
            out.append((km, ref.units(r[3])[0], du, nz, r[4]))
    return out, kept


def check_table(tab, rows, n, min_prob, strand=0):
    exp, kept = expected_rows(rows, n, min_prob)
    check_rows_and_stats(tab, exp, strand)
    return exp, kept


def check_rows_and_stats(tab, exp, strand=0):
    """exp: the KMER_ROW-shaped tuples the strand has to hold, in the table's order"""
    got = tab.rows(strand)
    g = list(zip(got["kmer_id"].tolist(), got["prob_units"].tolist(), got["descaled_units"].tolist(), got["neg_zero"].tolist(),
                 got["run"].tolist()))
    assert len(g) == len(exp)
    assert g == exp
    for med in (False, True):
        st = tab.stats(strand, use_median=med)
        by = {}
        for r in exp:
            by.setdefault(r[0], []).append(r[2])
        assert int(st["n"].sum()) == len(exp)
        for km, vals in by.items():
            nn, m, s = ref.stats(vals, med)
            assert st["n"][km] == nn
            assert st["m"][km].tobytes() == np.float64(m).tobytes(), (km, med)
            assert st["s"][km].tobytes() == np.float64(s).tobytes(), (km, med)


def cpg_jobs():
    jobs = cases.synthetic_jobs(cases.MODEL_CPG, 3, 1200, 40, cpg_ambiguous=True)
    jobs += cases.synthetic_jobs(cases.MODEL_CPG, 2, 900, 60)
    jobs += cases.thin_anchors_like_a_guide_alignment(cases.synthetic_jobs(cases.MODEL_CPG, 1, 1500, 70, cpg_ambiguous=True, cpg_every=3))
    # one-path reads with anchors as sparse as smoke() uses: bands wider than a wave (the strip kernels)
    for sparse in cases.synthetic_jobs(cases.MODEL_CPG, 2, 1500, 80):
        keep = np.zeros(len(sparse["ax"]), dtype=bool)
        keep[::37] = True
        sparse["ax"], sparse["ay"] = np.asarray(sparse["ax"])[keep], np.asarray(sparse["ay"])[keep]
        jobs.append(sparse)
    return jobs


@pytest.mark.parametrize("flags", [0, sa.FLAG_EXACT, sa.FLAG_FORCE_GENERIC])
def test_rows_and_stats_equal_the_restatement(flags, tmp_path):
    pm = sa.Model.load(cases.MODEL_CPG)
    alpha, k = pm.alphabet()
    p = sa.default_params()
    jobs = cpg_jobs()
    b = sa.Batch(pm, p, jobs, ambig=sa.default_ambig(CE), flags=flags)
    b.run()
    if flags == 0:
        st = b.stats()
        assert st.n_ring_regions > st.n_strip_regions > 0 and st.n_fast_regions > 0   # register, ring and strip kernels
    rows = batch_rows(b, jobs, pm.table5(), pm, k)
    assert any("E" in ref.kmer_name(r[1], alpha, k) for r in rows)
    for n, min_prob in ((3, 0.5), (40, 0.8)):
        tab = sa.KmerTable(pm, n, min_prob)
        info = {}
        tab.add_batch(b, 0, stats=info)
        assert info["kernel_ms"] > 0
        exp, kept = check_table(tab, rows, n, min_prob)
        assert len(exp) > 200
        # the M-step with mod_only: only k-mers holding E change
        stt = tab.stats(0)
        out, want = tmp_path / "got.model", tmp_path / "exp.model"
        sa.model_write_trained(cases.MODEL_CPG, stt, str(out), mod_only=True)
        ref.write_trained(cases.MODEL_CPG, {i: tuple(stt[i]) for i in range(len(stt))}, str(want), mod_only=True)
        assert out.read_bytes() == want.read_bytes()
        tab.close()
    # after the working storage went back the records are uploaded again
    b.release_device()
    tab = sa.KmerTable(pm, 3, 0.5)
    tab.add_batch(b, 0)
    check_table(tab, rows, 3, 0.5)
    tab.close()
    b.close()


def test_hdp_model():
    pm = sa.Model.load(cases.MODEL_R73, cases.NHDP)
    pm.set_to_hdp_expected_values()
    _, k = pm.alphabet()
    p = sa.default_params(threshold=0.05)
    jobs = cases.hdp_jobs(3, 900, 11, table5=pm.table5())
    for flags in (0, sa.FLAG_EXACT):
        b = sa.Batch(pm, p, jobs, flags=flags)
        b.run()
        rows = batch_rows(b, jobs, pm.table5(), pm, k)
        tab = sa.KmerTable(pm, 5, 0.3)
        tab.add_batch(b, 1)   # (the complement side of the table)
        assert len(tab.rows(0)) == 0
        exp, _ = check_table(tab, rows, 5, 0.3, strand=1)
        assert len(exp) > 20   # (broad HDP densities: few posteriors reach 0.3)
        tab.close()
        b.close()


def test_8_and_16_byte_records_give_the_same_table():
    pm = sa.Model.load(cases.MODEL_6MER)
    _, k = pm.alphabet()
    p = sa.default_params()
    jobs = cases.synthetic_jobs(cases.MODEL_6MER, 4, 1000, 300)
    res = []
    for flags in (0, sa.FLAG_PAIRS8):
        b = sa.Batch(pm, p, jobs, flags=flags)
        b.run()
        rows = batch_rows(b, jobs, pm.table5(), pm, k, p8=bool(flags))
        tab = sa.KmerTable(pm, 4, 0.6)
        tab.add_batch(b, 0)
        check_table(tab, rows, 4, 0.6)
        res.append((tab.rows(0).tobytes(), tab.stats(0).tobytes(), tab.stats(0, True).tobytes()))
        tab.close()
        b.close()
    assert res[0] == res[1]


def test_three_batches_equal_one(tmp_path):
    pm = sa.Model.load(cases.MODEL_CPG)
    _, k = pm.alphabet()
    p = sa.default_params()
    jobs = cpg_jobs()
    one = sa.KmerTable(pm, 2, 0.7)
    b = sa.Batch(pm, p, jobs, ambig=sa.default_ambig(CE))
    b.run()
    one.add_batch(b, 0)
    b.close()
    three = sa.KmerTable(pm, 2, 0.7)
    rows = []
    for part in (jobs[:2], jobs[2:5], jobs[5:]):
        assert part
        b = sa.Batch(pm, p, part, ambig=sa.default_ambig(CE))
        b.run()
        three.add_batch(b, 0)
        rows += batch_rows(b, part, pm.table5(), pm, k)
        b.close()
    check_table(three, rows, 2, 0.7)
    assert one.rows(0).tobytes() == three.rows(0).tobytes()
    for med in (False, True):
        assert one.stats(0, med).tobytes() == three.stats(0, med).tobytes()
    one.write(str(tmp_path / "a.tsv"))
    three.write(str(tmp_path / "b.tsv"))
    assert (tmp_path / "a.tsv").read_bytes() == (tmp_path / "b.tsv").read_bytes()
    _, kept = expected_rows(rows, 2, 0.7)
    alpha, _ = pm.alphabet()
    assert (tmp_path / "a.tsv").read_text() == ref.table_lines(kept, alpha, k)


def test_error_contract():
    pm = sa.Model.load(cases.MODEL_CPG)
    p = sa.default_params()
    jobs = cases.synthetic_jobs(cases.MODEL_CPG, 2, 600, 500, cpg_ambiguous=True)
    with pytest.raises(sa.SaError) as ei:
        sa.KmerTable(pm, 0, 0.8)
    assert ei.value.code == -1
    tab = sa.KmerTable(pm, 10, 0.8)
    b = sa.Batch(pm, p, jobs, ambig=sa.default_ambig(CE))
    with pytest.raises(sa.SaError) as ei:
        tab.add_batch(b, 0)
    assert ei.value.code == -7
    b.close()
    b = sa.Batch(pm, p, jobs, ambig=sa.default_ambig(CE), flags=sa.FLAG_VC_ROWS)
    b.run()
    with pytest.raises(sa.SaError) as ei:
        tab.add_batch(b, 0)
    assert ei.value.code == -1
    b.close()
    assert len(tab.rows(0)) == 0
    tab.close()


def test_mean_and_sd_agree_with_numpy():
    pm = sa.Model.load(cases.MODEL_6MER)
    p = sa.default_params()
    jobs = cases.synthetic_jobs(cases.MODEL_6MER, 3, 1500, 900)
    b = sa.Batch(pm, p, jobs)
    b.run()
    tab = sa.KmerTable(pm, 25, 0.2)
    tab.add_batch(b, 0)
    rows = tab.rows(0)
    st = tab.stats(0)
    vals = {}
    for km, du in zip(rows["kmer_id"].tolist(), rows["descaled_units"].tolist()):
        vals.setdefault(km, []).append(float("%d.%06d" % divmod(du, 1000000)) if du >= 0 else -float("%d.%06d" % divmod(-du, 1000000)))
    assert len(vals) > 100
    for km, v in vals.items():
        a = np.array(v)
        assert abs(st["m"][km] - np.mean(a)) <= 1e-12 * abs(np.mean(a))
        assert abs(st["s"][km] - np.std(a)) <= 1e-12 * max(abs(np.std(a)), 1e-300) or np.std(a) == st["s"][km]
    tab.close()
    b.close()


def test_reference_assignments_through_add_rows():
    """the reference's test file read twice, N = 1, min_prob 0 (test_trainModels.py:181-203): 3182 rows"""
    pm = sa.Model.load(cases.MODEL_6MER)
    with gzip.open(FIXTURE, "rt") as f:
        raw = [ln.split() for ln in f if ln.strip()]
    km = np.array([pm.kmer_id(r[0]) for r in raw], dtype=np.int32)
    desc = np.array([float(r[2]) for r in raw])
    prob = np.array([float(r[3]) for r in raw])
    tab = sa.KmerTable(pm, 1, 0.0)
    tab.add_rows(km, desc, prob)
    tab.add_rows(km, desc, prob)
    assert len(tab.rows(0)) == 3182
    tab.close()
    tab = sa.KmerTable(pm, 10, 0.0)
    for _ in range(2):
        tab.add_rows(km, desc, prob)
    rows = [("t", int(km[i]), raw[i][2], raw[i][3]) for i in range(len(raw))] * 2
    check_table(tab, rows, 10, 0.0)
    got = tab.rows(0)
    for kid in np.unique(got["kmer_id"]):
        p = got["prob_units"][got["kmer_id"] == kid]
        assert np.all(np.diff(p) <= 0)
    tab.close()


def test_checkpoint_and_rollback(tmp_path):
    """a slice added again after a rollback leaves the table as one add would"""
    pm = sa.Model.load(cases.MODEL_CPG)
    p = sa.default_params()
    jobs = cpg_jobs()
    b1 = sa.Batch(pm, p, jobs[:3], ambig=sa.default_ambig(CE))
    b2 = sa.Batch(pm, p, jobs[3:], ambig=sa.default_ambig(CE))
    b1.run()
    b2.run()
    ref_tab = sa.KmerTable(pm, 2, 0.5)
    ref_tab.add_batch(b1, 0)
    ref_tab.add_batch(b2, 0)
    ref_tab.add_batch(b2, 1)
    tab = sa.KmerTable(pm, 2, 0.5)
    with pytest.raises(sa.SaError) as ei:
        tab.rollback()
    assert ei.value.code == -7
    tab.add_batch(b1, 0)
    tab.checkpoint()
    before = tab.rows(0).tobytes()
    tab.add_batch(b2, 0)
    tab.add_batch(b2, 1)
    tab.rollback()
    assert tab.rows(0).tobytes() == before and len(tab.rows(1)) == 0
    tab.add_batch(b2, 0)
    tab.add_batch(b2, 1)
    for s in (0, 1):
        assert tab.rows(s).tobytes() == ref_tab.rows(s).tobytes()
    # the file by strand, appended: the same bytes as both strands at once
    tab.write(str(tmp_path / "both.tsv"))
    tab.write(str(tmp_path / "parts.tsv"), strand=0)
    tab.write(str(tmp_path / "parts.tsv"), strand=1, append=True)
    assert (tmp_path / "both.tsv").read_bytes() == (tmp_path / "parts.tsv").read_bytes()
    assert "\tc\t" in (tmp_path / "both.tsv").read_text()
    for t in (tab, ref_tab):
        t.close()
    b1.close()
    b2.close()


@pytest.mark.parametrize("flags", [0, sa.FLAG_PAIRS8])
def test_rows_tied_at_the_cutoff_take_run_order(flags):
    """N = 1 over reads whose best rows print 1.000000 many times: the run-order levels decide, on the tied rows only (copied
    out of 16- and of 8-byte records)"""
    pm = sa.Model.load(cases.MODEL_6MER)
    _, k = pm.alphabet()
    p = sa.default_params()
    jobs = cases.synthetic_jobs(cases.MODEL_6MER, 6, 1500, 1300)
    b = sa.Batch(pm, p, jobs, flags=flags)
    b.run()
    rows = batch_rows(b, jobs, pm.table5(), pm, k, p8=bool(flags))
    tied = {}
    for r in rows:
        if r[3] == "1.000000":
            tied[r[1]] = tied.get(r[1], 0) + 1
    assert any(v > 1 for v in tied.values())
    tab = sa.KmerTable(pm, 1, 0.8)
    tab.add_batch(b, 0)
    check_table(tab, rows, 1, 0.8)
    tab.close()
    b.close()


def test_planted_rows_win_ties_against_a_batch():
    """rows from add_rows and records of a batch tied at 1.000000, N = 1: the planted rows came first and are the ones kept"""
    pm = sa.Model.load(cases.MODEL_6MER)
    _, k = pm.alphabet()
    p = sa.default_params()
    jobs = cases.synthetic_jobs(cases.MODEL_6MER, 6, 1500, 1300)
    b = sa.Batch(pm, p, jobs)
    b.run()
    rows = batch_rows(b, jobs, pm.table5(), pm, k)
    ten = sorted({r[1] for r in rows if r[3] == "1.000000"})[:10]
    assert len(ten) == 10
    planted = [("t", km, "%f" % (50.0 + 1.5 * i), "1.000000") for i, km in enumerate(ten)]
    tab = sa.KmerTable(pm, 1, 0.8)
    tab.add_rows([r[1] for r in planted], [float(r[2]) for r in planted], [1.0] * 10)
    tab.add_batch(b, 0)
    exp, _ = check_table(tab, planted + rows, 1, 0.8)
    by = {r[0]: r for r in exp}
    for i, km in enumerate(ten):
        assert by[km][1:] == (1000000, ref.units(planted[i][2])[0], 0, i)
    tab.close()
    b.close()
