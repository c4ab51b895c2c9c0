"""Per-position marginals on the GPU (sa_batch_position_calls, SA_FLAG_POSITION_CALLS): CallMethylation.call_methyls
(src/signalalign/scripts/alignmentAnalysisLib.py:159-247) restated over the batch's own pairs, in the order the TSV prints them,
must give the same sums and probabilities bit for bit -- on the register, ring, strip and memory-resident kernels, with
host-finalised pairs, after the device storage went back, over several forward-storage passes and with an HDP model -- and
the flag's error contract must hold."""
import ctypes as C

import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import _capi, synth

import sa_cases as cases
from calls_ref import check_position_calls as check, restate_positions as restate

pytestmark = pytest.mark.gpu

ACGT = {"X": "ACGT"}


def with_x(jobs, step, phase=0):
    """every position = phase (mod step) of each job's ref replaced by X, as the substituted FASTA of one step holds it"""
    out = []
    for job in jobs:
        ref = list(job["ref"])
        for i in range(phase, len(ref), step):
            ref[i] = "X"
        out.append(dict(job, ref="".join(ref)))
    return out


def _model(path, nhdp=None):
    alpha, k, _, _ = synth.parse_model_table(path)
    return sa.Model.load(path, nhdp), "".join(sorted(alpha)), k


def snp_jobs():
    base = cases.synthetic_jobs(cases.MODEL_6MER, 3, 1000, 300)
    jobs = with_x(base, 10, 0) + with_x(base[:2], 10, 7) + with_x(base[:1], 3, 2)
    jobs += cases.synthetic_jobs(cases.MODEL_6MER, 1, 700, 310)     # no ambiguous position at all
    # anchors as sparse as a guide alignment leaves them: wide bands (strip / ring kernels)
    jobs += with_x(cases.thin_anchors_like_a_guide_alignment(cases.synthetic_jobs(cases.MODEL_6MER, 1, 1300, 320)), 10, 4)
    # one path per cell and an anchor every 37th: a band wider than a wave, swept by the strip kernels.  They take one-path
    # regions only, so no record of theirs covers an ambiguous position; the reduction reads past them (and their x range)
    sparse = cases.synthetic_jobs(cases.MODEL_6MER, 1, 1500, 330)[0]
    keep = np.zeros(len(sparse["ax"]), dtype=bool)
    keep[::37] = True
    jobs.append(dict(sparse, ax=np.asarray(sparse["ax"])[keep], ay=np.asarray(sparse["ay"])[keep]))
    return jobs


def _run(pm, p, jobs, amb, flags):
    b = sa.Batch(pm, p, jobs, ambig=sa.default_ambig(amb), flags=flags | sa.FLAG_POSITION_CALLS)
    b.run()
    st = {}
    calls = b.position_calls(stats=st)
    pairs = [b.pairs(j) for j in range(len(jobs))]
    return b, calls, pairs, st


def _check_all(calls, pairs, jobs, k, alpha, amb):
    n = 0
    for j, job in enumerate(jobs):
        exp = restate(pairs[j], job["ref"], k, alpha, amb)
        check(calls[j], exp, pairs[j])
        n += len(exp)
    return n


@pytest.mark.parametrize("flags", [0, sa.FLAG_EXACT, sa.FLAG_FORCE_GENERIC])
def test_marginals_equal_the_restatement_of_the_rows(flags):
    pm, alpha, k = _model(cases.MODEL_6MER)
    p = sa.default_params()
    jobs = snp_jobs()
    b, calls, pairs, st = _run(pm, p, jobs, ACGT, flags)
    if flags == 0:
        stats = b.stats()
        assert stats.n_ring_regions > 0 and stats.n_fast_regions > 0 and stats.n_strip_regions > 0
    assert st["kernel_ms"] > 0
    n = _check_all(calls, pairs, jobs, k, alpha, ACGT)
    assert len(calls[6]["p"]) == 0 and n > 300
    # deterministic, and the same after the working storage went back (the records go up again)
    again = b.position_calls()
    b.release_device()
    after = b.position_calls()
    for a, c, d in zip(calls, again, after):
        for f in ("p", "n_rows", "sum", "prob"):
            assert a[f].tobytes() == c[f].tobytes() == d[f].tobytes()
        assert a["x_min"] == c["x_min"] == d["x_min"] and a["x_max"] == c["x_max"] == d["x_max"]
    b.close()


def test_several_forward_passes(monkeypatch):
    pm, alpha, k = _model(cases.MODEL_6MER)
    p = sa.default_params()
    jobs = snp_jobs()
    monkeypatch.setenv("SA_F_BUDGET_CELLPATHS", "400000")
    b, calls, pairs, _ = _run(pm, p, jobs, ACGT, 0)
    assert b.stats().n_chunks >= 2
    assert _check_all(calls, pairs, jobs, k, alpha, ACGT) > 300
    b.close()


def test_pairs_are_the_same_with_and_without_the_flag():
    pm, _, _ = _model(cases.MODEL_6MER)
    p = sa.default_params()
    jobs = snp_jobs()
    b0 = sa.Batch(pm, p, jobs, ambig=sa.default_ambig(ACGT))
    b0.run()
    b1, _, pairs1, _ = _run(pm, p, jobs, ACGT, 0)
    for j in range(len(jobs)):
        assert b0.pairs(j).tobytes() == pairs1[j].tobytes()
    b0.close()
    b1.close()


def test_hdp_model():
    pm, alpha, k = _model(cases.MODEL_R73, cases.NHDP)
    pm.set_to_hdp_expected_values()
    p = sa.default_params(threshold=0.05)
    jobs = with_x(cases.hdp_jobs(3, 900, 11, table5=pm.table5()), 10, 3)
    for flags in (0, sa.FLAG_EXACT):
        b, calls, pairs, _ = _run(pm, p, jobs, ACGT, flags)
        assert _check_all(calls, pairs, jobs, k, alpha, ACGT) > 5
        b.close()


def test_several_kinds_of_letter():
    # X (4 options) and a two-letter code side by side; a position of a k-mer may hold both kinds
    pm, alpha, k = _model(cases.MODEL_6MER)
    amb = {"X": "ACGT", "Y": "CT"}
    p = sa.default_params()
    jobs = cases.synthetic_jobs(cases.MODEL_6MER, 2, 800, 340)
    for i, job in enumerate(jobs):
        ref = list(job["ref"])
        for n, q in enumerate(range(15 + i, len(ref) - 3, 13)):
            ref[q] = "XY"[n % 2]
        job["ref"] = "".join(ref)
    b, calls, pairs, _ = _run(pm, p, jobs, amb, 0)
    assert _check_all(calls, pairs, jobs, k, alpha, amb) > 50
    assert any(len(l) == 2 for c in calls for l in c["letters"])
    b.close()


def _rc(b):
    n = max(b.n_jobs, 1)
    ptrs = (C.POINTER(_capi.PositionCall) * n)()
    cnt = np.zeros(n, dtype=np.int64)
    return sa.lib().sa_batch_position_calls(b._h, 0, ptrs, cnt.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None)


def test_error_contract():
    pm, _, _ = _model(cases.MODEL_6MER)
    p = sa.default_params()
    jobs = with_x(cases.synthetic_jobs(cases.MODEL_6MER, 2, 600, 350), 10)
    amb = sa.default_ambig(ACGT)
    b = sa.Batch(pm, p, jobs, ambig=amb)                            # without the flag
    b.run()
    assert _rc(b) == -7                                            # SA_ESTATE
    b.close()
    b = sa.Batch(pm, p, jobs, ambig=amb, flags=sa.FLAG_POSITION_CALLS)
    assert _rc(b) == -7                                            # not run yet
    b.run()
    assert _rc(b) == 0
    b.close()
    with pytest.raises(sa.SaError) as e:
        sa.Batch(pm, p, jobs, ambig=amb, flags=sa.FLAG_POSITION_CALLS | sa.FLAG_VC_ROWS)
    assert e.value.code == -1                                      # SA_EINVAL
    plain = cases.synthetic_jobs(cases.MODEL_6MER, 2, 600, 360)
    with pytest.raises(sa.SaError) as e:
        sa.Batch(pm, p, plain, ambig=amb, flags=sa.FLAG_POSITION_CALLS | sa.FLAG_PAIRS8)
    assert e.value.code == -8                                      # SA_EUNSUPPORTED
    with pytest.raises(sa.SaError) as e:
        sa.Batch(pm, p, jobs, ambig=sa.default_ambig({"X": "ABCDEFGHI"}), flags=sa.FLAG_POSITION_CALLS)
    assert e.value.code == -8                                      # nine letters
    # a batch without ambiguous positions: no records, but each job's x range
    b = sa.Batch(pm, p, plain, ambig=amb, flags=sa.FLAG_POSITION_CALLS)
    b.run()
    calls = b.position_calls()
    for j, c in enumerate(calls):
        pr = b.pairs(j)
        assert len(c["p"]) == 0 and c["x_min"] == int(pr["x"].min()) and c["x_max"] == int(pr["x"].max())
    b.close()
