"""Reads that do not fit their model, on every kernel family, against the CPU oracle (inputs: tests/outlier_cases.py; what the
oracle makes of them and why the bars below apply: tests/test_oracle_outlier_events.py).

One batch per model holds the unmodified reads and their outlier variants together and runs under SA_FLAG_EXACT, the default flags
and SA_FLAG_FORCE_GENERIC:
  * SA_FLAG_EXACT: bit for bit the oracle's rows, at every magnitude -- identical operations in identical order;
  * "tail" jobs (|total| < 1e8) under the other flags: the project's bar, 1e-5 on a posterior (cases.compare_pairs(got, exp, 100,
    threshold)), the oracle's row order, at most 2 rows per job on one side only (the cap of test_gpu_two_dist_kernels.py);
  * "far" jobs (|total| >= 1e8, the reference itself has lost the digits): rc OK, no duplicate (x, y, path), k-mer and path of every
    row those of the reference position, rows in the oracle's order; the worst |dp| is printed, not bounded;
  * "neginf" jobs (an emission of -inf on every path): run() returns OK and the rows are the oracle's -- none where it has none --
    and every other read of the batch returns the bytes it returns in a batch without them.
Every test asserts from Batch.stats() which kernel family ran and prints the worst |dp| per read family before it asserts; the
figures measured on an MI355X are in DESIGN.md section 4, "Reads that do not fit their model".
"""
import math
import os

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import synth

import sa_cases as cases
import outlier_cases as oc

pytestmark = pytest.mark.gpu

FLAGS = (("exact", sa.FLAG_EXACT), ("default", 0), ("generic", sa.FLAG_FORCE_GENERIC))
TOL_E7 = 100
SA_EINVAL = -1
TWO = sa.FLAG_TWO_DIST_ALL_KERNELS


def _run(model, params, jobs, flags, ambig=None):
    b = sa.Batch(model, params, jobs, ambig=ambig, flags=flags)
    b.run()                                   # (raises SaError unless sa_batch_run returned SA_OK)
    got = [b.pairs(j) for j in range(len(jobs))]
    st = b.stats()
    b.close()
    return got, st


def _key(a):
    return [(int(r["x"]), int(r["y"]), int(r["path"])) for r in a]


def _same_bits(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for f in ("x", "y", "path", "kmer_id", "prob_e7"):
        assert np.array_equal(got[f], exp[f]), (what, f)


def _within_the_bar(got, exp, threshold, what):
    try:
        worst, lonely = cases.compare_pairs(got, exp, TOL_E7, threshold)
    except AssertionError as e:
        raise AssertionError((what,) + e.args)
    assert lonely <= 2 and cases.same_order(got, exp), (what, lonely)
    return worst


def _far_tail_rules(got, exp, job, k, alphabet, what):
    """what does not depend on the digits the total has lost; returns the worst |dp| over the rows both sides hold"""
    keys = _key(got)
    assert len(set(keys)) == len(keys), (what, "duplicate (x, y, path)")
    alpha = "".join(sorted(alphabet))
    for r in got:                              # (one path per cell in every far-tail read: path 0, the k-mer at x)
        x = int(r["x"])
        kid = 0
        for c in job["ref"][x:x + k]:
            kid = kid * len(alpha) + alpha.index(c)
        assert int(r["path"]) == 0 and int(r["kmer_id"]) == kid and 0 <= int(r["y"]) < len(job["events"]), (what, x)
    assert cases.same_order(got, exp), what
    e = dict(zip(_key(exp), exp["prob_e7"].tolist()))
    return max([abs(int(p) - e[q]) for q, p in zip(keys, got["prob_e7"].tolist()) if q in e] + [0])


def _check(jobs, exp, got, flag_name, threshold, k, alphabet, name):
    """every job of a suite against the oracle by the rules of its kind; prints the worst |dp| per read family and kind"""
    worst = {}
    for j, job in enumerate(jobs):
        what = "%s, %s flags, job %d: %s" % (name, flag_name, j, job["label"])
        e, g = exp[j][0], got[j]
        if flag_name == "exact" or (job["kind"] == "neginf" and len(e) == 0):
            _same_bits(g, e, what)
            continue
        fam = (job["label"].split()[0], job["kind"])
        if job["kind"] == "far":
            w = _far_tail_rules(g, e, job, k, alphabet, what)
        else:
            w = _within_the_bar(g, e, threshold, what)
        worst[fam] = max(worst.get(fam, 0), w)
    for fam in sorted(worst):
        print("%s, %s flags, %s (%s): worst |dp| against the oracle = %d e-7" % (name, flag_name, fam[0], fam[1], worst[fam]))
    return worst


def _others_keep_their_bytes(model, params, jobs, got, flags, ambig=None):
    """the reads that are not -inf reads return the bytes they return in a batch without the -inf reads"""
    keep = [j for j, job in enumerate(jobs) if job["kind"] != "neginf"]
    assert 0 < len(keep) < len(jobs)
    alone, _ = _run(model, params, [jobs[j] for j in keep], flags, ambig=ambig)
    for i, j in enumerate(keep):
        assert np.array_equal(alone[i], got[j]), (j, jobs[j]["label"])


@pytest.mark.parametrize("split", [3000 * 3000, oc.SPLIT_SMALL])
@pytest.mark.parametrize("model_path", [cases.MODEL_6MER, cases.MODEL_5MER])
def test_gaussian_tails_far_tails_and_minus_infinity(oracle, model_path, split, monkeypatch):
    """Means shifted by +-30, +-200 and +1e4 (tails), +1e6 (far tails) and set to 1e300 (finite, so k_check_events passes it; its
    squared deviation overflows: -inf rows) at every place of outlier_cases.WHERE, on register (a*), ring / strip (b1500, c900, c260)
    reads; with the small split limit c900 is two rectangles of which only one may hold the event."""
    alpha, k, t10, tab = synth.parse_model_table(model_path)
    jobs, k, n_reads = oc.gaussian_suite(model_path)
    exp = oc.oracle_rows(("gauss", model_path, split), lambda: oracle.Model(alpha, k, t10, tab), jobs, oracle.default_params(split=split))
    pm = sa.Model.load(model_path)
    p = sa.default_params(split=split)
    name = "%d-mer Gaussian%s" % (k, ", split" if split == oc.SPLIT_SMALL else "")
    for flag_name, flags in FLAGS:
        got, st = _run(pm, p, jobs, flags)
        if flags == 0:
            n_a = sum(1 for job in jobs if job["label"].startswith("a"))
            assert st.n_fast_regions == n_a and st.n_strip_regions >= 1 and st.n_fast_regions + st.n_ring_regions == st.n_regions, \
                (st.n_fast_regions, st.n_ring_regions, st.n_strip_regions, st.n_regions)
        else:
            assert st.n_fast_regions == 0 and st.n_ring_regions == 0
        _check(jobs, exp, got, flag_name, p.threshold, k, alpha, name)
        _others_keep_their_bytes(pm, p, jobs, got, flags)
        if flags == 0 and split != oc.SPLIT_SMALL:
            # the other classes the wide one-path reads can take: the one-path ring kernels (no strips) and the register kernels' own
            # wide-band path (SA_RING_WIDE=0)
            for env, fam in (("SA_STRIP", "one-path ring"), ("SA_RING_WIDE", "register, wide path")):
                monkeypatch.setenv(env, "0")
                again, st2 = _run(pm, p, jobs, 0)
                monkeypatch.delenv(env)
                if env == "SA_STRIP":
                    assert st2.n_strip_regions == 0 and st2.n_ring_regions == st.n_ring_regions
                else:
                    assert st2.n_ring_regions == 0 and st2.n_fast_regions == st.n_regions
                _check(jobs, exp, again, "default", p.threshold, k, alpha, "%s [%s]" % (name, fam))
    pm.close()


def test_cpg_ambiguous_tails(oracle):
    """(d): several paths per cell, the dense and the sparse instance of the multi-path ring kernels, the same shifts"""
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_CPG)
    jobs, k, n_reads = oc.cpg_suite()
    exp = oc.oracle_rows("cpg", lambda: oracle.Model(alpha, k, t10, tab), jobs, oracle.default_params(), ambig=oracle.ambig_map({"X": "CE"}))
    pm = sa.Model.load(cases.MODEL_CPG)
    p = sa.default_params()
    amb = sa.default_ambig({"X": "CE"})
    for flag_name, flags in FLAGS:
        got, st = _run(pm, p, jobs, flags, ambig=amb)
        if flags == 0:
            assert st.n_ring_regions == st.n_regions == len(jobs) and st.n_strip_regions == 0 and st.n_fast_regions == 0
        else:
            assert st.n_fast_regions == 0 and st.n_ring_regions == 0
        _check(jobs, exp, got, flag_name, p.threshold, k, alpha, "CpG ambiguous")
    pm.close()


def _hdp_oracle_model(oracle):
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_R73)
    om = oracle.Model(alpha, k, t10, tab)
    om.load_hdp(cases.NHDP)
    om.set_to_hdp_expected_values()
    return om


def test_hdp_tails_grid_ends_and_minus_infinity(oracle, monkeypatch):
    """R7.3 with the bundled .nhdp (grid: 100 points on [0, 100]): +-30 shifts, every grid-end value that keeps a positive density
    (hdp_density_coef's wave-uniform extrapolation branch: taken by one lane of a wave among interior ones, and by all active lanes of
    diagonals 1 and 2 and of the run of 70), and the values without a density (gN + 50, g0 - 50, +200): -inf rows.  Register, strip and
    ring (L / P codes: k_emit_hdp_ring) regions; once more with SA_HDP_HOT=0, the flavours without a hot row: the same bytes."""
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_R73)
    grid = synth.parse_nhdp(cases.NHDP)["grid"]
    om = _hdp_oracle_model(oracle)            # (kept in a name: match_table() is a view into the model's own memory)
    jobs, k, n_reads = oc.hdp_suite(om.match_table().copy(), grid)
    exp = oc.oracle_rows("hdp", lambda: _hdp_oracle_model(oracle), jobs, oracle.default_params(threshold=0.1))
    pm = sa.Model.load(cases.MODEL_R73, cases.NHDP)
    pm.set_to_hdp_expected_values()
    p = sa.default_params(threshold=0.1)
    for flag_name, flags in FLAGS:
        got, st = _run(pm, p, jobs, flags)
        if flags == 0:
            n_lp = sum(1 for job in jobs if job["label"].startswith("h400LP"))
            assert st.n_fast_regions >= 1 and st.n_strip_regions >= 1 and st.n_ring_regions - st.n_strip_regions >= n_lp, \
                (st.n_fast_regions, st.n_ring_regions, st.n_strip_regions, st.n_regions)
            assert st.n_fast_regions + st.n_ring_regions == st.n_regions
        else:
            assert st.n_fast_regions == 0 and st.n_ring_regions == 0
        _check(jobs, exp, got, flag_name, p.threshold, k, alpha, "R7.3 HDP")
        _others_keep_their_bytes(pm, p, jobs, got, flags)
        if flags == 0:
            monkeypatch.setenv("SA_HDP_HOT", "0")
            cold, st2 = _run(pm, p, jobs, 0)
            monkeypatch.delenv("SA_HDP_HOT")
            assert (st2.n_fast_regions, st2.n_ring_regions, st2.n_strip_regions) == (st.n_fast_regions, st.n_ring_regions, st.n_strip_regions)
            for j in range(len(jobs)):
                assert np.array_equal(cold[j], got[j]), (j, jobs[j]["label"])
    pm.close()


def _two_dist_model(emission):
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_CPG)
    m = sa.Model.create(alpha, k, t10, tab)
    m.set_emission(emission)
    return m


@pytest.mark.parametrize("emission,oracle_emission", [(1, 2), (2, 1)])
def test_two_distribution_noise(oracle, emission, oracle_emission):
    """SA_FLAG_TWO_DIST_ALL_KERNELS, both emissions (the numbers are crossed: the project's SA_EMISSION_TWO_DIST, 1, is the oracle's
    EM_TWODIST_DESCALED, 2): event noise x 1e-3, x 1e-6, x 30, x 1e3 (tails), exactly 0 under SA_EMISSION_TWO_DIST (the 1e-9
    replacement, |total| about 1e10: far tail) and 1e300 (-inf rows) on a register, a strip and two ring reads."""
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_CPG)
    jobs, k, n_reads = oc.two_dist_suite(emission)
    exp = oc.oracle_rows(("two", emission), lambda: oracle.Model(alpha, k, t10, tab, emission=oracle_emission), jobs,
                         oracle.default_params(), ambig=oracle.ambig_map({"X": "CE"}))
    m = _two_dist_model(emission)
    p = sa.default_params()
    amb = sa.default_ambig({"X": "CE"})
    name = "two-distribution emission %d" % emission
    for flag_name, flags in (("exact", sa.FLAG_EXACT), ("default", TWO)):
        got, st = _run(m, p, jobs, flags, ambig=amb)
        if flags == TWO:
            n_reg = sum(1 for job in jobs if job["label"].startswith("reg400"))
            n_cpg = sum(1 for job in jobs if job["label"].startswith("d1100"))
            assert st.n_fast_regions == n_reg and st.n_strip_regions >= 1 and st.n_ring_regions - st.n_strip_regions >= n_cpg, \
                (st.n_fast_regions, st.n_ring_regions, st.n_strip_regions, st.n_regions)
            assert st.n_fast_regions + st.n_ring_regions == st.n_regions
        else:
            assert st.n_fast_regions == 0 and st.n_ring_regions == 0
        far = [j for j, job in enumerate(jobs) if job["kind"] == "far" and job["label"].startswith("d1100")]
        worst_far = 0
        for j in far:      # (_far_tail_rules knows one path per cell: the multi-path far tails by the rules that do not need it)
            if flag_name != "exact":
                keys = _key(got[j])
                assert len(set(keys)) == len(keys) and cases.same_order(got[j], exp[j][0]), jobs[j]["label"]
                e = dict(zip(_key(exp[j][0]), exp[j][0]["prob_e7"].tolist()))
                worst_far = max([worst_far] + [abs(int(v) - e[q]) for q, v in zip(keys, got[j]["prob_e7"].tolist()) if q in e])
        if flag_name != "exact" and far:
            print("%s, %s flags, d1100 (far): worst |dp| against the oracle = %d e-7" % (name, flag_name, worst_far))
        rest = [j for j in range(len(jobs)) if j not in far or flag_name == "exact"]
        _check([jobs[j] for j in rest], [exp[j] for j in rest], [got[j] for j in rest], flag_name, p.threshold, k, alpha, name)
        _others_keep_their_bytes(m, p, jobs, got, flags, ambig=amb)
    m.close()


BAD_NOISE = (float("nan"), float("inf"), -float("inf"), -1.0)


def _rc(fn):
    with pytest.raises(sa.SaError) as e:
        fn()
    return e.value.code


@pytest.mark.parametrize("emission", [1, 2])
def test_bad_event_noise_is_refused_at_creation(emission, capfd):
    """NaN, +-inf, a negative noise, and zero under SA_EMISSION_TWO_DIST_SCALED_MODEL: SA_EINVAL from sa_batch_create with one line that
    names "event noise" and the job -- at the first, a middle and the last event, in job 0 and in the last job, from pageable memory
    and from the caller's page-locked block; zero under SA_EMISSION_TWO_DIST stays legal; the same batch without the value gives the
    bytes it gave before; a SA_EMISSION_MEAN_ONLY model does not read the column at all."""
    jobs, k, n_reads = oc.two_dist_suite(emission)
    jobs = jobs[:n_reads]
    m = _two_dist_model(emission)
    p = sa.default_params()
    amb = sa.default_ambig({"X": "CE"})
    before, _ = _run(m, p, jobs, TWO, ambig=amb)
    bad_values = BAD_NOISE + ((0.0,) if emission == 2 else ())
    capfd.readouterr()
    for value in bad_values:
        for j in (0, len(jobs) - 1):
            n = len(jobs[j]["events"])
            for at in (0, n // 2, n - 1):
                bad = list(jobs)
                bad[j] = oc.with_noise(jobs[j], [at], value=value, k=k)
                for flags in (TWO, sa.FLAG_EXACT, 0):
                    assert _rc(lambda: sa.Batch(m, p, bad, ambig=amb, flags=flags)) == SA_EINVAL, (value, j, at, flags)
                    err = capfd.readouterr().err
                    assert err.count("\n") == 1 and "event noise" in err and "job %d," % j in err and "event %d)" % at in err, err
        ja = sa.JobArray(bad, host_block=True)
        assert _rc(lambda: sa.Batch(m, p, ja, ambig=amb, flags=TWO | sa.FLAG_INPUTS_IN_HOST_BLOCK)) == SA_EINVAL, value
        assert "event noise" in capfd.readouterr().err
        ja.block.close()
        with pytest.raises(sa.SaError) as e:
            sa.expect_batch(m, p, bad, ambig=amb)
        assert e.value.code == SA_EINVAL and "event noise" in capfd.readouterr().err
    after, _ = _run(m, p, jobs, TWO, ambig=amb)
    for j in range(len(jobs)):
        assert np.array_equal(after[j], before[j]), j
    if emission == 1:                        # zero keeps its 1e-9: a batch, not a refusal
        zero = [oc.with_noise(jobs[0], [0], value=0.0, k=k)] + jobs[1:]
        got, _ = _run(m, p, zero, TWO, ambig=amb)
        assert len(got[0]) > 0 and all(np.array_equal(got[j], before[j]) for j in range(1, len(jobs)))
    m.close()
    mean_only = _two_dist_model(0)
    clean, _ = _run(mean_only, p, jobs, 0, ambig=amb)
    for value in BAD_NOISE + (0.0,):
        dirty = [oc.with_noise(job, "every37", value=value, k=k) for job in jobs]
        got, _ = _run(mean_only, p, dirty, 0, ambig=amb)
        for j in range(len(jobs)):
            assert np.array_equal(got[j], clean[j]), (value, j)
    mean_only.close()
    assert capfd.readouterr().err == ""


def _expect_jobs(suite_jobs, reads, places):
    out = []
    for job in suite_jobs:
        parts = job["label"].split(" ", 1)
        if parts[0] not in reads:
            continue
        if len(parts) == 1 or (job["kind"] == "neginf") or any(parts[1] == "mean%s@%s" % (d, w) for d in ("+30", "-30", "+200", "-200")
                                                                 for w in places):
            if job["kind"] != "far":
                out.append(job)
    return out


@pytest.mark.parametrize("model_path,ambiguous", [(cases.MODEL_6MER, False), (cases.MODEL_CPG, True)])
def test_expectation_pass(oracle, model_path, ambiguous):
    """sa_expect_batch on tail reads against oracle.expectations at test_gpu_fuzz.py's tolerances (rtol 1e-9, atol 1e-10, likelihood
    1e-12 relative), and the contract for a read whose total is -inf (include/signalalign_hip.h, sa_expect_batch): every checkpoint
    group whose total is -inf adds -inf to the likelihood and NOTHING to the transition expectations (the reference adds NaN), so the
    read's likelihood is -inf, its table is finite -- all zero when no traceback of the read escapes the event -- and the same from
    the register (fast), ring and memory-resident (SA_FLAG_FORCE_GENERIC) kernels; no other read's table is touched."""
    alpha, k, t10, tab = synth.parse_model_table(model_path)
    if ambiguous:
        suite, k, n = oc.cpg_suite()
        suite += [dict(oc.with_outlier_means(r, w, 1e300, k), kind="neginf") for r in suite[:n] for w in ("first", "last", "run3")]
        jobs = _expect_jobs(suite, ("d1100/1", "d1100/20"), ("every37", "first", "seg_edge"))
        amb_p, amb_o = sa.default_ambig({"X": "CE"}), oracle.ambig_map({"X": "CE"})
    else:
        suite, k, n = oc.gaussian_suite(model_path)
        jobs = _expect_jobs(suite, ("a400", "a1700", "b1500"), ("every37", "first", "last", "seg_edge"))
        amb_p, amb_o = None, None
    assert sum(1 for j in jobs if j["kind"] == "neginf") >= 6 and sum(1 for j in jobs if j["kind"] == "tail") >= 10
    pm = sa.Model.load(model_path)
    om = oracle.Model(alpha, k, t10, tab)
    p = sa.default_params()
    op = cases.oracle_params(oracle, p)
    ft, fl, _ = sa.expect_batch(pm, p, jobs, ambig=amb_p)
    st = sa.expect_last_stats()
    if ambiguous:
        assert st.n_ring_regions == st.n_regions == len(jobs) and st.n_fast_regions == 0
    else:      # (one-path regions keep the register kernels' expectation variant whatever their band: sa_route_kind)
        assert st.n_fast_regions == st.n_regions == len(jobs) and st.n_ring_regions == 0
    gt, gl, _ = sa.expect_batch(pm, p, jobs, ambig=amb_p, flags=sa.FLAG_FORCE_GENERIC)
    st = sa.expect_last_stats()
    assert st.n_fast_regions == 0 and st.n_ring_regions == 0
    assert np.isfinite(ft).all() and np.isfinite(gt).all()          # no NaN in any read's table
    for j, job in enumerate(jobs):
        om.set_read_params(job["scale"], job["shift"], job["var"])
        t, l, _, _, ost = oracle.expectations(om, job["ref"], job["events"], job["ax"], job["ay"], op, ambig=amb_o)
        if job["kind"] == "tail":
            np.testing.assert_allclose(ft[j], t, rtol=1e-9, atol=1e-10, err_msg=job["label"])
            np.testing.assert_allclose(gt[j], t, rtol=1e-9, atol=1e-10, err_msg=job["label"])
            assert abs(fl[j] - l) <= 1e-12 * max(abs(l), 1.0) and abs(gl[j] - l) <= 1e-12 * max(abs(l), 1.0), job["label"]
            continue
        assert l == -math.inf and np.isnan(t).any(), job["label"]     # (the reference's answer)
        assert fl[j] == -math.inf and gl[j] == -math.inf, (job["label"], fl[j], gl[j])
        np.testing.assert_allclose(ft[j], gt[j], rtol=1e-9, atol=1e-10, err_msg=job["label"])
        if ost.n_tracebacks == 1:
            assert not ft[j].any() and not gt[j].any(), job["label"]
    pm.close()
