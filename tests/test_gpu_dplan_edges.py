"""The device planner (signalalign_amd/csrc/sa_dplan.inc) against the host planner at the edges of the device's own walk: the
cases of tests/dplan_cases.py, which tests/test_host_dplan_cases.py pins to the CPU oracle through the host planner.  Every
array the kernels read must be the host planner's bytes (sa.dplan_compare; no sweep kernel runs); one batch of each group is
then aligned device-planned and host-planned, and the anchor-list and split-limit cases are planned and aligned again with the
inputs left in a page-locked block, where the device itself checks the anchors (k_dplan_ingest)."""
import numpy as np
import pytest

import signalalign_amd as sa
from signalalign_amd import synth

import dplan_cases as dc
import sa_cases as cases

pytestmark = pytest.mark.gpu

MASK_BITS = ((1, "regions"), (2, "rows"), (4, "packed words"), (8, "path offsets"), (16, "k-mer ids"), (32, "events"),
             (64, "segments"), (128, "checkpoints"), (256, "totals"), (512, "per-path records"))
_MODELS = {}


def _model(key):
    if key not in _MODELS:
        path, nhdp = dc.MODELS[key]
        _MODELS[key] = sa.Model.load(path, nhdp) if nhdp else sa.Model.load(path)
    return _MODELS[key]


def _ambig(case):
    return sa.default_ambig(case.ambig) if case.ambig else None


def _decode(rc):
    if rc == dc.NOT_TAKEN:
        return "not taken by the device planner"
    if rc == 0:
        return "identical"
    return "differs in: " + ", ".join(name for bit, name in MASK_BITS if rc & bit) + " (mask %d)" % rc


def _compare(case, jobs, flags, monkeypatch):
    for key, value in case.env or ():
        monkeypatch.setenv(key, value)
    return sa.dplan_compare(_model(case.model), sa.default_params(**dict(case.params)), jobs, ambig=_ambig(case), flags=flags)


@pytest.mark.parametrize("name", list(dc.CASES))
def test_device_plan_equals_host_plan_at_the_edge(name, monkeypatch):
    case = dc.CASES[name]
    rc = _compare(case, dc.jobs_of(case), case.flags, monkeypatch)
    assert rc == case.expect, "%s: %s, expected: %s" % (name, _decode(rc), _decode(case.expect))


def _pairs(case, jobs, flags=0):
    b = sa.Batch(_model(case.model), sa.default_params(**dict(case.params)), jobs, ambig=_ambig(case), flags=flags)
    b.run()
    n = jobs.n if isinstance(jobs, sa.JobArray) else len(jobs)
    got = [b.pairs(j) for j in range(n)]
    b.close()
    return got


@pytest.mark.parametrize("name", dc.ALIGNED)
def test_device_planned_and_host_planned_pairs_are_the_same_bytes(name, oracle, monkeypatch):
    case = dc.CASES[name]
    jobs = dc.jobs_of(case)
    got = _pairs(case, jobs)
    monkeypatch.setenv("SA_DEVICE_PLAN", "0")
    host = _pairs(case, jobs)
    monkeypatch.delenv("SA_DEVICE_PLAN")
    assert sum(len(q) for q in got) > len(jobs)                # (pairs there are)
    for j in range(len(jobs)):
        assert np.array_equal(got[j], host[j]), (name, j)
    if name in dc.ALIGNED_AGAINST_ORACLE:
        alpha, k, t10, tab = synth.parse_model_table(dc.MODELS[case.model][0])
        om = oracle.Model(alpha, k, t10, tab)
        p = sa.default_params(**dict(case.params))
        op = cases.oracle_params(oracle, p)
        for j, job in enumerate(jobs):
            cases.compare_pairs(got[j], cases.oracle_pairs(oracle, om, job, op), 100, p.threshold)


@pytest.mark.parametrize("name", [c.name for c in dc.CASES.values() if c.group in (3, 6)])
def test_anchor_edges_checked_on_the_device(name, monkeypatch):
    """FLAG_INPUTS_IN_HOST_BLOCK: the anchors are checked by k_dplan_ingest, not by the host; same answer, and the same pairs
    (the reads of 8191 .. 8193 anchors are planned only: no aligned read is longer than 4000 events)."""
    case = dc.CASES[name]
    jobs = dc.jobs_of(case)
    ja = sa.JobArray(jobs, host_block=True)
    rc = _compare(case, ja, case.flags | sa.FLAG_INPUTS_IN_HOST_BLOCK, monkeypatch)
    assert rc == case.expect, "%s in a host block: %s, expected: %s" % (name, _decode(rc), _decode(case.expect))
    if max(len(j["events"]) for j in jobs) > 4000:
        return
    plain = _pairs(case, jobs, case.flags)
    block = _pairs(case, ja, case.flags | sa.FLAG_INPUTS_IN_HOST_BLOCK)
    for j in range(len(jobs)):
        assert np.array_equal(block[j], plain[j]), (name, j)
