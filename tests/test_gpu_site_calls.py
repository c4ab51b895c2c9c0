"""Per-site variant / methylation calls on the GPU (sa_batch_site_calls, SA_FLAG_SITE_CALLS): MarginalizeFullVariants.get_data
(src/signalalign/variantCaller.py:92-187) restated in numpy over the batch's own pairs must give the same integer sums exactly
and the same probabilities bit for bit, on every kernel family, with host-finalised pairs, after the device storage went back,
and with HDP models; the error contract of the flag."""
import ctypes as C

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import _capi, synth

import sa_cases as cases
from calls_ref import check_site_calls as check_calls, restate_sites as restate

pytestmark = pytest.mark.gpu

CE = {"X": "CE"}


def _model(path, nhdp=None):
    alpha, k, _, _ = synth.parse_model_table(path)
    return sa.Model.load(path, nhdp), "".join(sorted(alpha)), k


def cpg_jobs():
    jobs = cases.synthetic_jobs(cases.MODEL_CPG, 3, 1200, 40, cpg_ambiguous=True)
    jobs += cases.synthetic_jobs(cases.MODEL_CPG, 3, 1200, 50, cpg_ambiguous=True, cpg_every=3)
    jobs += cases.synthetic_jobs(cases.MODEL_CPG, 1, 900, 60)          # no site at all
    # one read with anchors as sparse as a guide alignment leaves them: wide bands (strip / ring kernels)
    jobs += cases.thin_anchors_like_a_guide_alignment(cases.synthetic_jobs(cases.MODEL_CPG, 1, 1500, 70, cpg_ambiguous=True, cpg_every=3))
    assert sum("X" in j["ref"] for j in jobs) == len(jobs) - 1
    return jobs


def _calls_and_pairs(pm, p, jobs, amb, flags):
    b = sa.Batch(pm, p, jobs, ambig=sa.default_ambig(amb), flags=flags | sa.FLAG_SITE_CALLS)
    b.run()
    st = {}
    calls = b.site_calls(stats=st)
    pairs = [b.pairs(j) for j in range(len(jobs))]
    return b, calls, pairs, st


@pytest.mark.parametrize("flags", [0, sa.FLAG_EXACT, sa.FLAG_FORCE_GENERIC])
def test_calls_equal_the_restatement_of_the_pairs(flags):
    pm, alpha, k = _model(cases.MODEL_CPG)
    p = sa.default_params()
    jobs = cpg_jobs()
    b, calls, pairs, st = _calls_and_pairs(pm, p, jobs, CE, flags)
    stats = b.stats()
    if flags == 0:   # several kernel families in one batch
        assert stats.n_ring_regions > 0 and stats.n_fast_regions > 0
    assert st["kernel_ms"] > 0
    n_sites = 0
    for j, job in enumerate(jobs):
        exp = restate(pairs[j], job["ref"], k, alpha, CE)
        check_calls(calls[j], exp)
        n_sites += len(exp)
    assert len(calls[6]["x"]) == 0 and n_sites > 100
    # deterministic: a second call gives the same bytes
    again = b.site_calls()
    for a, c in zip(calls, again):
        for f in ("x", "units", "prob"):
            assert a[f].tobytes() == c[f].tobytes()
    # after the working storage went back (the pairs are uploaded again)
    b.release_device()
    after = b.site_calls()
    for a, c in zip(calls, after):
        for f in ("x", "units", "prob"):
            assert a[f].tobytes() == c[f].tobytes()
    b.close()


def test_exact_calls_equal_the_restatement_of_the_oracle_pairs(oracle):
    pm, alpha, k = _model(cases.MODEL_CPG)
    a_, k_, t10, tab = synth.parse_model_table(cases.MODEL_CPG)
    om = oracle.Model(a_, k_, t10, tab)
    p = sa.default_params()
    op = cases.oracle_params(oracle, p)
    jobs = cases.synthetic_jobs(cases.MODEL_CPG, 2, 700, 80, cpg_ambiguous=True)
    jobs += cases.synthetic_jobs(cases.MODEL_CPG, 1, 700, 90, cpg_ambiguous=True, cpg_every=3)
    b, calls, _, _ = _calls_and_pairs(pm, p, jobs, CE, sa.FLAG_EXACT)
    for j, job in enumerate(jobs):
        exp = restate(cases.oracle_pairs(oracle, om, job, op, ambig=oracle.ambig_map(CE)), job["ref"], k, alpha, CE)
        assert len(exp) > 5
        check_calls(calls[j], exp)
    b.close()


def test_pairs_are_the_same_with_and_without_the_flag():
    pm, _, _ = _model(cases.MODEL_CPG)
    p = sa.default_params()
    jobs = cpg_jobs()
    b0 = sa.Batch(pm, p, jobs, ambig=sa.default_ambig(CE))
    b0.run()
    b1, _, pairs1, _ = _calls_and_pairs(pm, p, jobs, CE, 0)
    for j in range(len(jobs)):
        assert b0.pairs(j).tobytes() == pairs1[j].tobytes()
    b0.close()
    b1.close()


def test_hdp_model_with_ambiguity():
    pm, alpha, k = _model(cases.MODEL_R73, cases.NHDP)
    pm.set_to_hdp_expected_values()
    p = sa.default_params(threshold=0.05)
    jobs = cases.hdp_jobs(3, 900, 11, table5=pm.table5())
    for job in jobs:
        job["ref"] = job["ref"].replace("CG", "XG")
    assert all("X" in j["ref"] for j in jobs)
    for flags in (0, sa.FLAG_EXACT):
        b, calls, pairs, _ = _calls_and_pairs(pm, p, jobs, CE, flags)
        n = 0
        for j, job in enumerate(jobs):
            exp = restate(pairs[j], job["ref"], k, alpha, CE)
            check_calls(calls[j], exp)
            n += len(exp)
        assert n > 5
        b.close()


def test_four_and_six_letter_sites():
    """X -> ACGT and U -> ACEGOT (the default table's six-way code) on the ACEGOT model: cells of up to 24 paths"""
    pm, alpha, k = _model(cases.MODEL_R73)
    amb = {"X": "ACGT", "U": "ACEGOT"}
    p = sa.default_params()
    jobs = cases.synthetic_jobs(cases.MODEL_R73, 3, 800, 100)
    for i, job in enumerate(jobs):
        ref = list(job["ref"])
        for n, q in enumerate(range(20 + 7 * i, len(ref) - 10, 37)):
            ref[q] = "XU"[n % 2]
        job["ref"] = "".join(ref)
    b, calls, pairs, _ = _calls_and_pairs(pm, p, jobs, amb, 0)
    six = 0
    for j, job in enumerate(jobs):
        exp = restate(pairs[j], job["ref"], k, alpha, amb)
        check_calls(calls[j], exp)
        six += sum(len(v[0]) == 6 for v in exp.values())
    assert six > 10
    b.close()


def _site_calls_rc(b):
    ptrs = (C.POINTER(_capi.SiteCall) * max(b.n_jobs, 1))()
    cnt = np.zeros(max(b.n_jobs, 1), dtype=np.int64)
    return sa.lib().sa_batch_site_calls(b._h, 0, ptrs, cnt.ctypes.data_as(C.POINTER(C.c_int64)), None)


def test_error_contract():
    pm, _, _ = _model(cases.MODEL_CPG)
    p = sa.default_params()
    jobs = cases.synthetic_jobs(cases.MODEL_CPG, 2, 600, 120, cpg_ambiguous=True)
    amb = sa.default_ambig(CE)
    b = sa.Batch(pm, p, jobs, ambig=amb)                          # without the flag
    b.run()
    assert _site_calls_rc(b) == -7                               # SA_ESTATE
    b.close()
    b = sa.Batch(pm, p, jobs, ambig=amb, flags=sa.FLAG_SITE_CALLS)
    assert _site_calls_rc(b) == -7                               # not run yet
    b.run()
    assert _site_calls_rc(b) == 0
    b.close()
    with pytest.raises(sa.SaError) as e:
        sa.Batch(pm, p, jobs, ambig=amb, flags=sa.FLAG_SITE_CALLS | sa.FLAG_VC_ROWS)
    assert e.value.code == -1                                    # SA_EINVAL
    with pytest.raises(sa.SaError) as e:
        sa.Batch(pm, p, jobs, ambig=sa.default_ambig({"X": "ABCDEFGHI"}), flags=sa.FLAG_SITE_CALLS)
    assert e.value.code == -8                                    # SA_EUNSUPPORTED: nine letters
    # a batch without sites -- 8-byte records among them -- has zero calls per job
    plain = cases.synthetic_jobs(cases.MODEL_CPG, 2, 600, 130)
    for flags in (sa.FLAG_PAIRS8, 0):
        b = sa.Batch(pm, p, plain, ambig=amb, flags=flags | sa.FLAG_SITE_CALLS)
        b.run()
        assert [len(c["x"]) for c in b.site_calls()] == [0, 0]
        b.close()
