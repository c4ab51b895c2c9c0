"""SA_FLAG_TWO_DIST_ALL_KERNELS: the two-distribution emission (Gaussian on the level x inverse Gaussian on the event noise) on the
ring and strip kernels, and sa_batch_create_noise_scaled: the noise columns of the model rescaled per read.

The yardstick throughout is the same batch under SA_FLAG_EXACT -- the reference-ordered kernels, which the existing tests hold
bit-identical to the CPU restatement (tests/test_gpu_reference_kats.py).  The bar is the project's own: 1e-5 on a posterior
(cases.compare_pairs(got, exact, 100, threshold)), at most 2 rows per job on one side only, the same row order.

Worst |posterior difference| against SA_FLAG_EXACT measured on an MI355X, in units of 1e-7: see DESIGN.md section 4, "Two-distribution
emission on the ring and strip kernels" (the tests print the figure before they assert).
"""
import os

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import synth

import sa_cases as cases
import zymo_wholeread as z

pytestmark = pytest.mark.gpu

GOLDEN = z.GOLDEN
EM_TWO_DIST, EM_TWO_DIST_SCALED_MODEL = 1, 2
TWO = sa.FLAG_TWO_DIST_ALL_KERNELS
TOL_E7 = 100
SA_EINVAL, SA_EUNSUPPORTED = -1, -8


def _run(model, params, jobs, flags, ambig=None, noise=None):
    b = sa.Batch(model, params, jobs, ambig=ambig, flags=flags, noise=noise)
    b.run()
    got = [b.pairs(j) for j in range(len(jobs))]
    st = b.stats()
    b.close()
    return got, st


def _model(path, emission, table=None):
    alpha, k, t10, tab = synth.parse_model_table(path)
    m = sa.Model.create(alpha, k, t10, tab if table is None else table)
    m.set_emission(emission)
    return m


def _identity_scaling(jobs, emission):
    # (the scaled-model emission takes the event as it is: the model is not scaled to these reads, give them the identity instead)
    return [dict(j, scale=1.0, shift=0.0, var=1.0) for j in jobs] if emission == EM_TWO_DIST_SCALED_MODEL else jobs


def _within_the_bar(got, exact, threshold, what):
    worst = 0
    for j in range(len(exact)):
        w, lonely = cases.compare_pairs(got[j], exact[j], TOL_E7, threshold)
        worst = max(worst, w)
        assert lonely <= 2 and cases.same_order(got[j], exact[j]), (what, j, lonely)
    print("%s: worst |dp| against SA_FLAG_EXACT = %d e-7" % (what, worst))
    return worst


def _cpg_ring_jobs():
    jobs = cases.synthetic_jobs(cases.MODEL_CPG, 2, 1400, 20, cpg_ambiguous=True)                     # dense instance, 1-8 paths
    jobs += cases.synthetic_jobs(cases.MODEL_CPG, 1, 1100, 330, cpg_ambiguous=True, cpg_every=30)     # sparse instance
    wide = cases.realistic_anchor_jobs(cases.MODEL_CPG, 1, 1200, 77)[0]
    jobs.append(dict(wide, ref=wide["ref"].replace("CG", "XG")))
    return jobs


def _r73_ring_jobs():
    jobs = []
    for j, job in enumerate(cases.synthetic_jobs(cases.MODEL_R73, 2, 600, 50)):
        ref = list(job["ref"])
        for i in range(7 + j, len(ref) - 6, 23):
            if ref[i] == "C":
                ref[i] = "L"                                                                          # three paths
        jobs.append(dict(job, ref="".join(ref)))
    return jobs


@pytest.mark.parametrize("emission", [EM_TWO_DIST, EM_TWO_DIST_SCALED_MODEL])
@pytest.mark.parametrize("model_path,amb_tab,make_jobs", [(cases.MODEL_CPG, {"X": "CE"}, _cpg_ring_jobs),
                                                          (cases.MODEL_R73, None, _r73_ring_jobs)])
def test_ring_kernels_several_paths_per_cell(model_path, amb_tab, make_jobs, emission, monkeypatch):
    """Ambiguity letters: the dense and the sparse instance of the ring kernels, 1-8 paths per cell, a band wider than a wave,
    the three-way code L -- every path of a cell with the noise constants of its own k-mer."""
    m = _model(model_path, emission)
    amb = sa.default_ambig(amb_tab)
    p = sa.default_params()
    jobs = _identity_scaling(make_jobs(), emission)
    got, st = _run(m, p, jobs, TWO, ambig=amb)
    assert st.n_ring_regions == st.n_regions == len(jobs) and st.n_fast_regions == 0
    exact, st_e = _run(m, p, jobs, sa.FLAG_EXACT, ambig=amb)
    assert st_e.n_ring_regions == 0 and st_e.n_fast_regions == 0
    for j in range(len(jobs)):
        assert exact[j]["path"].max() >= 1
        assert len(got[j]) > 0.3 * len(jobs[j]["events"])
    _within_the_bar(got, exact, p.threshold, "ring, emission %d, %s" % (emission, os.path.basename(model_path)))
    for j in range(len(jobs)):      # the k-mer of a row both sides hold
        ek = {(int(r["x"]), int(r["y"]), int(r["path"])): int(r["kmer_id"]) for r in exact[j]}
        assert all(ek.get((int(r["x"]), int(r["y"]), int(r["path"])), int(r["kmer_id"])) == int(r["kmer_id"]) for r in got[j])
    for waves in ("1", "2", "4"):   # every workgroup shape: one to eight cell-paths per thread and diagonal
        monkeypatch.setenv("SA_RING_WAVES", waves)
        again, _ = _run(m, p, jobs, TWO, ambig=amb)
        for j in range(len(jobs)):
            assert np.array_equal(again[j], got[j]), (waves, j)
    monkeypatch.delenv("SA_RING_WAVES")
    m.close()


def _strip_jobs():
    # (four reads with the anchors of a real guide alignment: of the reads without anchors only the one of 260 events has a band
    # wider than a wave, those of 90 and 35 events are register-kernel regions with any emission)
    jobs = cases.realistic_anchor_jobs(cases.MODEL_6MER, 4, 2500, 600)
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_6MER)
    for n_ev, idx in ((260, 41), (90, 43), (35, 44)):      # no anchors at all; reads shorter than one strip
        r = synth.make_read(idx, n_ev, alpha, k, tab)
        jobs.append(dict(r, ax=np.zeros(0, dtype=np.int64), ay=np.zeros(0, dtype=np.int64)))
    jobs += cases.synthetic_jobs(cases.MODEL_6MER, 1, 900, 300)   # dense anchors: register kernels
    return jobs


@pytest.mark.parametrize("emission", [EM_TWO_DIST, EM_TWO_DIST_SCALED_MODEL])
def test_strip_kernels_and_one_path_ring_kernels(emission, monkeypatch):
    """One-path regions with wide bands: the strip kernels do the ring kernels' arithmetic in the ring kernels' order, noise term
    included, so their pairs equal the one-path ring instance's (SA_STRIP=0) byte for byte; both within the bar of SA_FLAG_EXACT."""
    m = _model(cases.MODEL_6MER, emission)
    p = sa.default_params()
    jobs = _identity_scaling(_strip_jobs(), emission)
    strip, st = _run(m, p, jobs, TWO)
    assert st.n_strip_regions == st.n_ring_regions >= 5 and st.n_fast_regions >= 1
    assert st.n_fast_regions + st.n_ring_regions == st.n_regions
    mean_only = _model(cases.MODEL_6MER, 0)                # every region in the kernel family a MeanOnly model gets
    _, st_m = _run(mean_only, p, jobs, 0)
    mean_only.close()
    assert (st_m.n_fast_regions, st_m.n_ring_regions, st_m.n_strip_regions) == (st.n_fast_regions, st.n_ring_regions, st.n_strip_regions)
    monkeypatch.setenv("SA_STRIP", "0")
    ring, st_r = _run(m, p, jobs, TWO)
    monkeypatch.delenv("SA_STRIP")
    assert st_r.n_strip_regions == 0 and st_r.n_ring_regions == st.n_ring_regions
    for j in range(len(jobs)):
        assert np.array_equal(strip[j], ring[j]), (j, len(strip[j]), len(ring[j]))
    exact, st_e = _run(m, p, jobs, sa.FLAG_EXACT)
    assert st_e.n_fast_regions == 0 and st_e.n_ring_regions == 0
    _within_the_bar(strip, exact, p.threshold, "strip, emission %d" % emission)
    _within_the_bar(ring, exact, p.threshold, "one-path ring, emission %d" % emission)
    for j in range(len(jobs)):
        assert len(strip[j]) > 0.5 * len(jobs[j]["events"])
    again, _ = _run(m, p, jobs, TWO)                       # same bytes on a second batch (seams, atomics, planes)
    for j in range(len(jobs)):
        assert np.array_equal(again[j], strip[j]), j
    for kw in (dict(threshold=0.0005), dict(expansion=20, trace_back=30, min_diags=150)):
        q = sa.default_params(**kw)
        s2, st1 = _run(m, q, jobs, TWO)
        monkeypatch.setenv("SA_STRIP", "0")
        r2, st2 = _run(m, q, jobs, TWO)
        monkeypatch.delenv("SA_STRIP")
        assert st1.n_strip_regions >= 5 and st2.n_strip_regions == 0
        for j in range(len(jobs)):
            assert np.array_equal(s2[j], r2[j]), (kw, j, len(s2[j]), len(r2[j]))
    m.close()


# the literal event records of tests/stateMachineTests.c:444-453 (mean, noise, duration, start)
SY6 = [58.743435, 0.887833, 0.0571, 0.0,
       53.604965, 0.816836, 0.0571, 0.1,
       58.432015, 0.735143, 0.0571, 0.2,
       63.684352, 0.795437, 0.0571, 0.3,
       58.921430, 0.812959, 0.0571, 0.4,
       59.895882, 0.740952, 0.0571, 0.5,
       61.684303, 0.722332, 0.0571, 0.67]


def test_literal_matrix_with_the_three_way_code_on_the_ring_kernels():
    """tests/stateMachineTests.c:441-565: ACGATALGGACAT, getStateMachine3, no anchors, band expansion 2, ends not ragged, threshold
    0.2: exactly 14 pairs inside the listed set -- out of the ring kernels (the nearest posterior is 0.13 from the threshold)."""
    m = _model(os.path.join(GOLDEN, "models", "testModelR73_acegot_template.model"), EM_TWO_DIST_SCALED_MODEL)
    p = sa.default_params(threshold=0.2, expansion=2, trace_back=40)
    job = dict(ref="ACGATALGGACAT", events=np.array(SY6, dtype=np.float64).reshape(7, 4), ax=[], ay=[], ragged=(0, 0))
    got, st = _run(m, p, [job], TWO)
    assert st.n_ring_regions == st.n_regions >= 1 and st.n_fast_regions == 0
    got = got[0]
    assert len(got) == 14
    assert {(int(q["x"]), int(q["y"])) for q in got} <= {(0, 0), (1, 1), (2, 2), (3, 3), (4, 3), (5, 4), (6, 5), (7, 6)}
    assert got["prob_e7"].min() >= 2000000 and got["prob_e7"].max() <= 10000000
    m.close()


def _noise_scaled(table5, scale_sd, var_sd):
    """emissions_signal_scaleNoise (impl/stateMachine.c:721-741) on the five columns of the model table"""
    t = np.array(table5, dtype=np.float64).reshape(-1, 5).copy()
    t[:, 2] = t[:, 2] * scale_sd
    t[:, 4] = t[:, 4] * var_sd
    t[:, 3] = np.sqrt(np.power(t[:, 2], 3.0) / t[:, 4])
    return t.reshape(-1)


def _zymo_degenerate(letters):
    r = z.read_fixture()
    alpha, k, t10, tab = synth.parse_model_table(os.path.join(GOLDEN, "models", "testModelR73_acegot_template.model"))
    ax, ay = z.remapped_anchors()
    bd = z.BANDING
    p = sa.default_params(threshold=bd["threshold"], expansion=bd["expansion"], trace_back=bd["trace_back"], min_diags=bd["min_diags"],
                          split=bd["split"])
    tp = r["template_params"]
    lX, lY = len(r["ref"]) - (k - 1), r["template_events"].shape[0]
    m = sa.Model.create(alpha, k, t10, _noise_scaled(tab, tp["scale_sd"], tp["var_sd"]))
    m.set_emission(EM_TWO_DIST)
    jobs = [dict(ref=r["ref"].replace("C", letter), events=r["template_events"], ax=ax, ay=ay, scale=tp["scale"], shift=tp["shift"],
                 var=tp["var"], ragged=(0, 0)) for letter in letters]
    got, st = _run(m, p, jobs, TWO)             # (default ambiguity table: L -> C / E / O)
    m.close()
    for j, letter in enumerate(letters):
        assert len(got[j]) == z.N_PAIRS_DEGENERATE[letter], (letter, len(got[j]))
        g = got[j]
        assert g["x"].min() >= 0 and g["x"].max() < lX and g["y"].min() >= 0 and g["y"].max() < lY
        assert g["prob_e7"].min() > 0 and g["prob_e7"].max() <= 10000000
    return st


def test_zymo_whole_read_c_e_o_from_the_strip_kernels():
    """tests/stateMachineTests.c:920-983, the three one-path jobs: the Zymo read with every C kept / replaced by E / by O, ends not
    ragged: exactly 1076 pairs each.  The lastz anchors leave a band wider than a wave: with the flag the read is a strip-kernel region
    (without it the batch takes the reference-ordered kernels).  With the CPU restatement no posterior of these jobs lies within
    4.1e-5 of the threshold: the count is safe under the 1e-5 bar."""
    st = _zymo_degenerate("CEO")
    assert st.n_fast_regions + st.n_ring_regions == st.n_regions == 3 and st.n_strip_regions >= 1


def test_zymo_whole_read_degenerate_nucleotides_c_e_o_l():
    """tests/stateMachineTests.c:920-983 as tests/test_gpu_reference_kats.py sets it up -- C / E / O / the three-way code L in one batch:
    exactly 1076 / 1076 / 1076 / 7349 pairs -- with the flag, and every region on the register or ring kernels.

    The L job is the widest thing the ring kernels take: every C a three-way code gives its cells up to 81 paths, 1 241 724 cell-paths
    on 140 468 cells, diagonals of up to 2023 cell-paths (band of up to 93 cells; 932 of the 1692 diagonals hold more than the 512
    cell-paths of the ring's other classes).  It runs on the wide class (SA_RING_WIDE_MAX_ROWPATHS, k_bwd_ring<WIDE>), which exists
    for flagged two-distribution batches only: a MeanOnly model sends this read to the memory-resident kernels as before."""
    st = _zymo_degenerate("CEOL")
    assert st.n_fast_regions + st.n_ring_regions == st.n_regions and st.n_ring_regions >= 1


def test_wide_ring_class_against_the_reference_ordered_kernels(monkeypatch):
    """The wide class of the ring kernels (rows of more than 512 cell-paths: eight per thread and diagonal on four waves, the
    checkpoint sums of the backward sweep in global scratch instead of LDS) against SA_FLAG_EXACT, under the bar of every other test
    here: the Zymo read with every C the three-way code L (diagonals of up to 2023 cell-paths) and with every second C only (narrower
    diagonals, still above 512), for both emissions; the same bytes whatever SA_RING_WAVES asks for (the wide class takes four)."""
    r = z.read_fixture()
    alpha, k, t10, tab = synth.parse_model_table(os.path.join(GOLDEN, "models", "testModelR73_acegot_template.model"))
    ax, ay = z.remapped_anchors()
    bd = z.BANDING
    p = sa.default_params(threshold=bd["threshold"], expansion=bd["expansion"], trace_back=bd["trace_back"], min_diags=bd["min_diags"],
                          split=bd["split"])
    tp = r["template_params"]
    half = "".join("L" if c == "C" and i % 2 == 0 else c for i, c in enumerate(r["ref"]))
    assert "L" in half and "C" in half
    for emission in (EM_TWO_DIST, EM_TWO_DIST_SCALED_MODEL):
        m = sa.Model.create(alpha, k, t10, _noise_scaled(tab, tp["scale_sd"], tp["var_sd"]))
        m.set_emission(emission)
        jobs = [dict(ref=ref, events=r["template_events"], ax=ax, ay=ay, scale=tp["scale"], shift=tp["shift"], var=tp["var"],
                     ragged=(0, 0)) for ref in (r["ref"].replace("C", "L"), half)]
        for job in jobs:    # both on the wide class: some diagonal holds more than 512 cell-paths
            info, _, rows, _ = sa.plan_describe(m, p, job, flags=TWO)
            assert info.n_ring_regions == info.n_regions == 1
            ref = job["ref"]
            per_column = np.array([1] + [3 ** ref[x:x + k].count("L") for x in range(len(ref) - k + 1)], dtype=np.int64)
            poff = np.concatenate([[0], np.cumsum(per_column)])
            x0 = (np.arange(len(rows)) + rows[:, 1]) // 2
            rowpaths = poff[x0 + (rows[:, 2] - rows[:, 1]) // 2 + 1] - poff[x0]
            assert 512 < rowpaths.max() <= 2048, rowpaths.max()
        got, st = _run(m, p, jobs, TWO)
        assert st.n_ring_regions == st.n_regions == 2 and st.n_fast_regions == 0
        exact, st_e = _run(m, p, jobs, sa.FLAG_EXACT)
        assert st_e.n_ring_regions == 0 and st_e.n_fast_regions == 0
        assert exact[0]["path"].max() >= 9 and len(got[1]) > 0
        # (emission 1: the reference's known answer; the scaled-model emission meets a model that is not scaled to this read)
        assert len(got[0]) == z.N_PAIRS_DEGENERATE["L"] if emission == EM_TWO_DIST else len(got[0]) > 0
        _within_the_bar(got, exact, p.threshold, "wide ring, emission %d" % emission)
        for j in range(len(jobs)):
            ek = {(int(q["x"]), int(q["y"]), int(q["path"])): int(q["kmer_id"]) for q in exact[j]}
            assert all(ek.get((int(q["x"]), int(q["y"]), int(q["path"])), int(q["kmer_id"])) == int(q["kmer_id"]) for q in got[j])
        monkeypatch.setenv("SA_RING_WAVES", "1")
        again, _ = _run(m, p, jobs, TWO)
        monkeypatch.delenv("SA_RING_WAVES")
        for j in range(len(jobs)):
            assert np.array_equal(again[j], got[j]), j
        m.close()


NOISE = [(1.0, 1.0), (0.8, 1.3), (1.25, 0.7), (1.1, 1.1)]


@pytest.mark.parametrize("emission", [EM_TWO_DIST, EM_TWO_DIST_SCALED_MODEL])
def test_noise_scaling_per_read(emission):
    """sa_batch_create_noise_scaled: job j as if its model were clone_with_table(emissions_signal_scaleNoise(table, noise[j])) -- the same
    bytes as a one-job batch on that model, whatever else is in the batch and in whatever order."""
    # one register, one strip and two ring jobs as in the tests above, under ONE model: the CpG model holds every ACGT k-mer too
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_CPG)
    one_path = cases.synthetic_jobs(cases.MODEL_CPG, 1, 900, 300) + cases.realistic_anchor_jobs(cases.MODEL_CPG, 1, 2500, 600)
    jobs = _identity_scaling(one_path + cases.synthetic_jobs(cases.MODEL_CPG, 2, 1400, 20, cpg_ambiguous=True), emission)
    m = _model(cases.MODEL_CPG, emission)
    amb = sa.default_ambig({"X": "CE"})
    p = sa.default_params()
    got, st = _run(m, p, jobs, TWO, ambig=amb, noise=NOISE)
    assert st.n_fast_regions >= 1 and st.n_strip_regions >= 1 and st.n_ring_regions - st.n_strip_regions >= 2
    assert st.n_fast_regions + st.n_ring_regions == st.n_regions
    plain, _ = _run(m, p, jobs, TWO, ambig=amb)
    assert any(not np.array_equal(got[j], plain[j]) for j in range(len(jobs)))
    assert np.array_equal(got[0], plain[0])                # (factors 1, 1: the model's own table)
    for j, (scale_sd, var_sd) in enumerate(NOISE):
        mj = m.clone_with_table(_noise_scaled(tab, scale_sd, var_sd))
        alone, _ = _run(mj, p, [jobs[j]], TWO, ambig=amb)
        assert np.array_equal(alone[0], got[j]), j
        if j > 0:
            assert not np.array_equal(got[j], plain[j]), j
        mj.close()
    back, _ = _run(m, p, jobs[::-1], TWO, ambig=amb, noise=NOISE[::-1])
    for j in range(len(jobs)):
        assert np.array_equal(back[len(jobs) - 1 - j], got[j]), j
    m.close()


def _rc(fn):
    with pytest.raises(sa.SaError) as e:
        fn()
    return e.value.code


def test_error_contract(monkeypatch):
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_6MER)
    jobs = cases.synthetic_jobs(cases.MODEL_6MER, 2, 300, 900)
    p = sa.default_params()
    two = _model(cases.MODEL_6MER, EM_TWO_DIST)
    mean_only = _model(cases.MODEL_6MER, 0)
    ok = [(1.0, 1.0), (0.9, 1.2)]
    assert _rc(lambda: sa.Batch(two, p, jobs, flags=0, noise=ok)) == SA_EINVAL               # without the flag
    assert _rc(lambda: sa.Batch(mean_only, p, jobs, flags=TWO, noise=ok)) == SA_EINVAL       # a MeanOnly model
    means = [dict(j, events=np.ascontiguousarray(j["events"][:, 0])) for j in jobs]
    assert _rc(lambda: sa.Batch(two, p, means, flags=TWO, noise=ok)) == SA_EINVAL            # event_stride 1
    for bad in (0.0, float("nan"), -1.0, float("inf")):
        assert _rc(lambda: sa.Batch(two, p, jobs, flags=TWO, noise=[(1.0, 1.0), (bad, 1.0)])) == SA_EINVAL
        assert _rc(lambda: sa.Batch(two, p, jobs, flags=TWO, noise=[(1.0, bad), (1.0, 1.0)])) == SA_EINVAL
    hdp = sa.Model.load(cases.MODEL_R73, cases.NHDP)
    hjobs = cases.synthetic_jobs(cases.MODEL_R73, 1, 300, 900)
    assert _rc(lambda: sa.Batch(hdp, p, hjobs, flags=TWO)) == SA_EUNSUPPORTED                # an HDP model with the flag
    hdp.close()
    # regions sent to the memory-resident kernels: never aligned with the model's own noise without a word
    sparse = cases.realistic_anchor_jobs(cases.MODEL_6MER, 2, 1500, 600)
    monkeypatch.setenv("SA_RING", "0")

    def forced():
        amb = sa.default_ambig({"X": "CT"})
        xj = [dict(j, ref=j["ref"].replace("CG", "XG")) for j in sparse]
        b = sa.Batch(two, p, xj, ambig=amb, flags=TWO, noise=ok)
        b.run()
    assert _rc(forced) == SA_EUNSUPPORTED
    monkeypatch.delenv("SA_RING")
    assert _rc(lambda: sa.Batch(two, p, jobs, flags=TWO | sa.FLAG_EXACT, noise=ok)) == SA_EUNSUPPORTED
    # the flag with a MeanOnly model: the bytes of flags 0
    mixed = jobs + sparse
    a, st_a = _run(mean_only, p, mixed, TWO)
    b, st_b = _run(mean_only, p, mixed, 0)
    assert st_a.n_ring_regions == st_b.n_ring_regions >= 2 and st_a.n_fast_regions == st_b.n_fast_regions
    for j in range(len(mixed)):
        assert np.array_equal(a[j], b[j]), j
    two.close(); mean_only.close()
