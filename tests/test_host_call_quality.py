"""Call quality without a device: the header's exports and the mirror agree; the restatement (call_quality_ref.py) equals what
signalAlign's own get_distance_from_guide_alignment and find_gaps_in_alignment_data gave on the recorded cases
(tests/golden/call_quality/reference_cases.json), exactly; a hand-worked table; and the one case in which the script's
one-guide-row-per-call walk and the rule of this library part.  The argument checks need an accumulator, which needs a device:
tests/test_gpu_call_quality.py holds them."""
import ctypes as C
import json
import os
import re

import numpy as np

import signalalign_amd as sa
from signalalign_amd import _capi

import abi_header as hdr
import call_quality_ref as ref

CASES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_quality", "reference_cases.json")
SA_EINVAL = -1


def test_header_exports_and_mirror_agree():
    text = hdr.header_text()
    protos = hdr.prototypes(text)
    for name in ("sa_batch_call_quality", "sa_call_quality_records", "sa_call_quality_release", "sa_call_quality_last_kernel_ms"):
        assert name in protos and name in _capi.SIGNATURES and hasattr(sa.lib(), name)
        assert protos[name] == hdr.signature_kinds(*_capi.SIGNATURES[name])
    assert len(protos["sa_batch_call_quality"][1]) == 17 and len(protos["sa_call_quality_records"][1]) == 23
    structs = hdr.struct_names(text)
    for c_name in ("sa_callq_params_t", "sa_callq_job_t", "sa_callq_read_t", "sa_callq_call_t", "sa_callq_gap_t"):
        assert c_name in structs and c_name in _capi.ABI
    # the sizes the header's comments state, and a multiple of 8 bytes each
    assert (sa.CALLQ_READ_DTYPE.itemsize, sa.CALLQ_CALL_DTYPE.itemsize, sa.CALLQ_GAP_DTYPE.itemsize) == (112, 56, 16)
    assert C.sizeof(sa.CallqParams) == 24 and C.sizeof(sa.CallqJob) == 48
    defines = dict(re.findall(r"#define\s+(SA_CQ_\w+)\s+(\d+)u?", text))
    assert {k: int(v) for k, v in defines.items()} == dict(
        SA_CQ_NO_GUIDE=sa.CQ_NO_GUIDE, SA_CQ_NO_SITES=sa.CQ_NO_SITES, SA_CQ_NO_PATH=sa.CQ_NO_PATH, SA_CQ_CALLS=sa.CQ_CALLS,
        SA_CQ_BAND_DIRECT=sa.CQ_BAND_DIRECT, SA_CQ_MAX_BINS=sa.CQ_MAX_BINS)
    assert (ref.NO_GUIDE, ref.NO_SITES, ref.NO_PATH) == (sa.CQ_NO_GUIDE, sa.CQ_NO_SITES, sa.CQ_NO_PATH)
    for name in ("batch_call_quality", "call_quality_records", "call_quality_release", "call_quality_last_kernel_ms"):
        assert callable(getattr(sa, name))


def test_calls_without_an_accumulator_are_refused_and_the_scratch_calls_need_no_device():
    L = sa.lib()
    gaps, n_gaps = C.c_void_p(), np.zeros(1, dtype=np.int64)
    first = np.zeros(1, dtype=np.int64)
    rc = L.sa_call_quality_records(None, None, None, 0, _capi._ip(first), None, None, None, _capi._ip(first), None, None, None, None,
                                   None, 0, None, None, None, C.byref(gaps), _capi._ip(n_gaps), None, None, None)
    assert rc == SA_EINVAL and gaps.value is None
    rc = L.sa_batch_call_quality(None, None, None, None, 0, None, None, None, 0, None, None, None, C.byref(gaps), _capi._ip(n_gaps),
                                 None, None, None)
    assert rc == SA_EINVAL
    sa.call_quality_release()
    assert sa.call_quality_last_kernel_ms() == dict(band=0.0, calls=0.0, gaps=0.0)


def _case_inputs(c):
    """a recorded case as the restatement takes it: every site labelled by the read, one record at each end of its band"""
    job_map = dict(contig=0, x_sign=c["x_sign"], x0=c["x0"], strand=0, mapped_strand=0, true_letter=0)
    job = dict(ax=c["ax"], ay=c["ay"], raw_start=c["raw_start"], raw_length=c["raw_length"])
    rec_x, rec_y = [], []
    for x, (y0, y1) in zip(c["site_x"], c["band_y"]):
        rec_x += [x, x]
        rec_y += [y1, y0]
    return job_map, job, rec_x, rec_y, [[1.0, 0.0]] * len(c["site_x"])


def test_the_restatement_equals_the_recorded_reference_outputs():
    cases = json.load(open(CASES))["cases"]
    own = [c for c in cases if c["own_row"]]
    assert len(own) >= 200 and len(own) < len(cases)
    assert {c["x_sign"] for c in own} == {1, -1}
    n_half = n_calls = n_gaps = 0
    for c in cases:
        job_map, job, rec_x, rec_y, prob = _case_inputs(c)
        params = (-10000, 100, 200, c["min_gap"])
        for walk in (False, True):
            if not walk and not c["own_row"]:
                continue
            read, calls, gaps, _ = ref.call_quality(job_map, job, c["site_x"], prob, rec_x, rec_y, c["path_y"], 0.5, {},
                                                    params=params, script_walk=walk)
            assert read["n_outside"] == 0 and read["n_calls"] == len(c["call_x"])
            by_x = {k["x"]: k for k in calls}
            for x, delta in zip(c["call_x"], c["guide_delta"]):
                assert 2 * delta == by_x[x]["delta2"], (c, x, walk)          # (exact: delta is a multiple of 0.5)
                n_half += by_x[x]["delta2"] % 2
                n_calls += 1
            assert [g for _, _, g in gaps] == c["gaps"]
            n_gaps += len(gaps)
    assert n_calls > 500 and n_half > 50 and n_gaps > 200
    # where the script's walk gives a call a later row, the rule's delta differs from the script's
    apart = [c for c in cases if not c["own_row"]]
    for c in apart:
        job_map, job, rec_x, rec_y, prob = _case_inputs(c)
        rule = ref.call_quality(job_map, job, c["site_x"], prob, rec_x, rec_y, c["path_y"], 0.5, {})[1]
        walk = ref.call_quality(job_map, job, c["site_x"], prob, rec_x, rec_y, c["path_y"], 0.5, {}, script_walk=True)[1]
        assert [k["guide_event"] for k in rule] != [k["guide_event"] for k in walk]


def test_hand_worked_table():
    h = ref.HAND
    read, calls, gaps, hist = ref.call_quality(h["job_map"], h["job"], h["site_x"], h["site_prob"], h["rec_x"], h["rec_y"], h["path_y"],
                                               h["threshold"], {})
    # x = 1 lies before the first guide row (the script's iloc[-1] would wrap), x = 10 beyond the last (the script leaves NaN)
    # x = 4: band of events 2..4 = samples 17..32, mid2 = 2 * 17 + 15 = 49; guide row (4, 3): np.round(22 + 4 / 2) = 24; delta 0.5
    # x = 7: band of events 6..8 = samples 75..89, mid2 = 164; the row before it is (5, 5): np.round(32 + 3 / 2) = 34; delta 48
    assert calls == [
        dict(x=1, guide_event=-1, raw_start=10, raw_length=7, delta2=0, prob_true=0.9, true_letter=1, correct=1, outside=1),
        dict(x=4, guide_event=3, raw_start=17, raw_length=15, delta2=1, prob_true=0.5, true_letter=1, correct=0, outside=0),
        dict(x=7, guide_event=5, raw_start=75, raw_length=14, delta2=96, prob_true=0.7, true_letter=1, correct=1, outside=0),
        dict(x=10, guide_event=-1, raw_start=130, raw_length=2, delta2=0, prob_true=0.2, true_letter=1, correct=0, outside=1)]
    assert gaps == [(5, 6, 40)]                                   # (8 -> 9 is a hole of exactly min_gap: none)
    assert read == dict(status=0, max_x=7, n_calls=4, n_correct=2, n_unlabelled=0, n_other_sites=0, n_outside=2, sum_abs_delta2=97,
                        max_abs_delta2=96, n_path=9, n_gaps=1, sum_gap=40, max_gap=40)
    want = np.zeros((202, 2), dtype=np.int64)
    want[101, 0] = want[101, 1] = 1                               # both in [0, 100): the bin that starts at 0
    assert (hist == want).all()
    # np.round's halves, each parity: events 1 and 5 round up, 7 and 10 down
    rs, rl = h["job"]["raw_start"], h["job"]["raw_length"]
    assert [ref.round_mid(rs[y], rl[y]) for y in (1, 5, 7, 10)] == [16, 34, 82, 126]
    assert [float(np.round(rs[y] + rl[y] / 2)) for y in (1, 5, 7, 10)] == [16.0, 34.0, 82.0, 126.0]
    # the floor of the histogram: a negative delta2 that C's truncation would put one bin too high
    assert ref.hist_slot(-1, 0, 100, 4) == 0 and ref.hist_slot(-1, -100, 100, 4) == 1 and ref.hist_slot(-201, -200, 100, 4) == 1
    assert ref.hist_slot(-20001, -10000, 100, 200) == 0 and ref.hist_slot(-20000, -10000, 100, 200) == 1
    assert ref.hist_slot(19999, -10000, 100, 200) == 200 and ref.hist_slot(20000, -10000, 100, 200) == 201


def test_the_scripts_walk_and_the_rule_part_for_two_calls_that_share_a_guide_gap():
    # guide rows at x = 2, 6, 8, 9 (events 1, 4, 6, 7); calls at x = 3 and x = 4 share the gap between the rows at 2 and 6, x = 9 is
    # a row
    job = dict(ax=[2, 6, 8, 9], ay=[1, 4, 6, 7], raw_start=[0, 10, 20, 30, 40, 50, 60, 70, 80], raw_length=[10] * 9)
    job_map = dict(contig=0, x_sign=1, x0=0, strand=0, mapped_strand=0, true_letter=0)
    site_x, prob = [3, 4, 9], [[1.0, 0.0]] * 3
    rec_x, rec_y = [3, 4, 9], [2, 3, 7]
    rule = ref.call_quality(job_map, job, site_x, prob, rec_x, rec_y, None, 0.5, {})[1]
    walk = ref.call_quality(job_map, job, site_x, prob, rec_x, rec_y, None, 0.5, {}, script_walk=True)[1]
    assert [c["guide_event"] for c in rule] == [1, 1, 7]          # both measured against the row before them
    assert [c["guide_event"] for c in walk] == [1, 4, 7]          # the script has moved on by one row for the second
    assert [c["delta2"] for c in rule] == [20, 40, 0] and [c["delta2"] for c in walk] == [20, -20, 0]
    differ = [a["x"] for a, b in zip(rule, walk) if a != b]
    assert differ == [4]
