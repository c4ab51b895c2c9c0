"""What the CPU oracle makes of reads that do not fit their model (tests/outlier_cases.py), and the conditions that
tests/test_gpu_outlier_events.py leans on: a "tail" input keeps |total| < 1e8, so that a re-associated sum cannot reach the 1e-5
bar by rounding (one ulp of 1e8 is 1.5e-8); a "-inf" input has a total of -inf and no row from any traceback that reaches the
event; with the small split limit such a read keeps rows, all in rectangles without an outlier; the HDP's density at and beyond the
grid's ends is what was measured when these tests were written; and a +-30 shift leaves rows AT outlier events -- otherwise the tail tests would only
measure how an alignment routes around them.  Runs without a GPU.
"""
import math

import numpy as np
import pytest

from signalalign_amd import synth

import sa_cases as cases
import outlier_cases as oc

SPLITS = (3000 * 3000, oc.SPLIT_SMALL)


def _pin(jobs, res, k, split):
    """the properties of each kind, for one suite under one split limit"""
    n_checked = {"tail": 0, "far": 0, "neginf": 0}
    for job, (rows, st) in zip(jobs, res):
        # (Stats.last_total_prob is the total of the lowest checkpoint of the last traceback of the LAST rectangle: it speaks for the
        # read when the read is one rectangle; a split read's rectangles are checked through their rows)
        total, kind = st.last_total_prob, job["kind"]
        n_checked[kind] += 1
        regions = oc.regions_of(job, k, split)
        if kind == "tail":
            assert math.isfinite(total) and abs(total) < 1e8, (job["label"], total)
            continue
        if kind == "far":
            assert math.isfinite(total) and (abs(total) >= 1e8 or len(regions) > 1), (job["label"], total)
            continue
        assert total == -math.inf or len(regions) > 1, (job["label"], total)
        single_traceback = st.n_tracebacks == len(regions)
        clean_rows = 0
        for y1, y2 in regions:
            inside = job["outliers"][(job["outliers"] >= y1) & (job["outliers"] < y2)]
            here = rows[(rows["y"] >= y1) & (rows["y"] < y2)]
            if len(inside) == 0:
                clean_rows += len(here)
            elif single_traceback:
                assert len(here) == 0, (job["label"], y1, y2, len(here))
            else:   # an earlier traceback of the same rectangle never met the event: its rows lie before it
                assert len(here) == 0 or here["y"].max() < inside.min(), (job["label"], y1, y2)
        if any(len(job["outliers"][(job["outliers"] >= y1) & (job["outliers"] < y2)]) == 0 for y1, y2 in regions):
            assert clean_rows > 0, job["label"]     # (the small split limit: rows, all in rectangles without an outlier)
    return n_checked


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("model_path", [cases.MODEL_6MER, cases.MODEL_5MER])
def test_gaussian_tails_far_tails_and_minus_infinity(oracle, model_path, split):
    alpha, k, t10, tab = synth.parse_model_table(model_path)
    jobs, k, n = oc.gaussian_suite(model_path)
    res = oc.oracle_rows(("gauss", model_path, split), lambda: oracle.Model(alpha, k, t10, tab), jobs, oracle.default_params(split=split))
    seen = _pin(jobs, res, k, split)
    assert seen["tail"] > 100 and seen["far"] >= 20 and seen["neginf"] >= 20
    # under the small limit some read is several rectangles of which only some hold the 1e300 event, and it keeps rows
    if split == oc.SPLIT_SMALL:
        assert any(j["kind"] == "neginf" and len(oc.regions_of(j, k, split)) > 1 and len(r[0]) > 0 for j, r in zip(jobs, res))
    # +-30: rows AT outlier events, for either sign and for every read of 400 events and more
    for sign in ("+30", "-30"):
        for read in ("a400", "a1700", "b1500", "c900"):
            hit = [len(set(r[0]["y"].tolist()) & set(j["outliers"].tolist())) for j, r in zip(jobs, res)
                   if j["label"] == "%s mean%s@every37" % (read, sign)]
            assert len(hit) == 1 and hit[0] >= 3, (read, sign, hit)
    # the three tracebacks the 1700-event read stands for
    assert res[2][1].n_tracebacks == 3 and oc.seg_edge_event(jobs[2], k) is not None


def test_cpg_tails(oracle):
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_CPG)
    jobs, k, n = oc.cpg_suite()
    res = oc.oracle_rows("cpg", lambda: oracle.Model(alpha, k, t10, tab), jobs, oracle.default_params(), ambig=oracle.ambig_map({"X": "CE"}))
    assert _pin(jobs, res, k, SPLITS[0])["tail"] == len(jobs) > 30
    assert all(r[0]["path"].max() >= 1 for r in res)


def _hdp_model(oracle):
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_R73)
    om = oracle.Model(alpha, k, t10, tab)
    om.load_hdp(cases.NHDP)
    om.set_to_hdp_expected_values()
    return om


def test_hdp_density_at_and_beyond_the_grid_ends(oracle):
    om = _hdp_model(oracle)
    grid = synth.parse_nhdp(cases.NHDP)["grid"]
    assert (grid[0], grid[-1], len(grid)) == (0.0, 100.0, 100)
    d = {name: om.hdp_density(float(f(grid[0], grid[-1])), 0) for name, f, _ in oc.GRID_END}
    measured = {"g0": 7.43e-5, "g0-5": 4.6e-5, "gN": 1.099e-3, "gN+0.5": 1.014e-3, "gN+5": 2.4e-4}
    for name, v in measured.items():      # (figures of two to four digits)
        assert abs(d[name] - v) <= 0.02 * v, (name, d[name])
    assert d["g0-50"] == 0.0 and d["gN+50"] == 0.0
    for name, _, positive in oc.GRID_END:
        assert (d[name] > 0.0) == positive, name
    # one ulp either side of an end: the same density to 1e-12 relative (the cubic inside, the straight line outside)
    for end in ("g0", "gN"):
        for side in ("-ulp", "+ulp"):
            assert abs(d[end + side] - d[end]) <= 1e-12 * d[end]


def test_hdp_tails_and_minus_infinity(oracle):
    grid = synth.parse_nhdp(cases.NHDP)["grid"]
    om = _hdp_model(oracle)                    # (kept in a name: match_table() is a view into the model's own memory)
    jobs, k, n = oc.hdp_suite(om.match_table().copy(), grid)
    res = oc.oracle_rows("hdp", lambda: _hdp_model(oracle), jobs, oracle.default_params(threshold=0.1))
    seen = _pin(jobs, res, k, SPLITS[0])
    assert seen["tail"] > 50 and seen["neginf"] > 40
    for j, r in zip(jobs, res):
        what = j["label"].split(" ", 1)[1] if " " in j["label"] else ""
        if what in ("mean+30@every37", "mean-30@every37"):      # rows at some outlier event
            assert len(set(r[0]["y"].tolist()) & set(j["outliers"].tolist())) >= 1, j["label"]
        if what.startswith("grid ends gN+0.5,g0-5,gN+5"):      # ... and at the events that sit beyond the grid
            assert len(set(r[0]["y"].tolist()) & set(j["outliers"].tolist())) == 3, j["label"]
        if j["kind"] == "tail":
            assert len(r[0]) > 100, j["label"]


@pytest.mark.parametrize("emission,oracle_emission", [(1, 2), (2, 1)])
def test_two_distribution_noise(oracle, emission, oracle_emission):
    """(the emission numbers are crossed: the project's SA_EMISSION_TWO_DIST (1) is the oracle's EM_TWODIST_DESCALED (2))"""
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_CPG)
    assert (oracle.EM_TWODIST_DESCALED, oracle.EM_TWODIST) == (2, 1)
    jobs, k, n = oc.two_dist_suite(emission)
    amb = oracle.ambig_map({"X": "CE"})

    def make():
        return oracle.Model(alpha, k, t10, tab, emission=oracle_emission)
    res = oc.oracle_rows(("two", emission), make, jobs, oracle.default_params(), ambig=amb)
    seen = _pin(jobs, res, k, SPLITS[0])
    assert seen["tail"] == 4 + 4 * 12 and seen["far"] == (12 if emission == 1 else 0) and seen["neginf"] >= 15
    # what the library refuses: the reference's total is NaN and the alignment empty
    om = make()
    job = jobs[0]
    om.set_read_params(job["scale"], job["shift"], job["var"])
    bad = [-1.0, float("nan"), float("inf"), -float("inf")] + ([0.0] if emission == 2 else [])
    for value in bad:
        q = oc.with_noise(job, "every37", value=value, k=k)
        rows, st = oracle.align(om, q["ref"], q["events"], q["ax"], q["ay"], oracle.default_params(), ambig=amb, want_stats=True)
        assert len(rows) == 0 and (math.isnan(st.last_total_prob) or value == float("inf")), (value, st.last_total_prob)


def test_expectations_of_a_read_whose_total_is_minus_infinity(oracle):
    """getExpectationsUsingAnchors on such a read: the likelihood is -inf and the transition expectations are NaN (exp(-inf - -inf));
    the tail reads keep finite tables."""
    alpha, k, t10, tab = synth.parse_model_table(cases.MODEL_6MER)
    om = oracle.Model(alpha, k, t10, tab)
    jobs, k, n = oc.gaussian_suite(cases.MODEL_6MER)
    for job in jobs:
        if not job["label"].startswith("a400"):
            continue
        om.set_read_params(job["scale"], job["shift"], job["var"])
        t, lik, _, _, _ = oracle.expectations(om, job["ref"], job["events"], job["ax"], job["ay"], oracle.default_params())
        if job["kind"] == "neginf":
            assert lik == -math.inf and np.isnan(t).sum() >= 7, (job["label"], lik, t)
        else:
            assert math.isfinite(lik) and np.isfinite(t).all(), (job["label"], lik)
